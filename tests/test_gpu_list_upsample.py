"""GPU: half-resolution light lists (rtsh_subsample_gbuffer_device, rtsh_upsample_retrace_map_device, rtsh_upsample_light_list_device,
rtsh_upsample_soft_light_list_device; raytracedshadows_amd/csrc/rts_upsample.inc, included by rts_primary.hip) on the frames of
tests/list_upsample_cases.py: the device forms equal the host twins byte for byte (the twins equal the numpy rules in
tests/test_list_upsample_host.py) over every shape and phase -- single pixels, rows and columns, sizes on either side of one 32 x 8
block and of one wave, several blocks --, lists of 1 and 8 lights, soft and hard, maps and keep present and absent; every buffer one
element into a larger allocation preset to 0xAB, whose other bytes must come back unchanged.  One kernel node each under capture;
anchor 4 on the device through the device traces; the refusals write nothing."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import list_combine_cases as lc
import list_upsample_cases as uc
from raytracedshadows_amd import api
from soft_list_cases import make_list, workload

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID = 1
f32 = np.float32
CASES = [(kind, wh, phase) for kind in ("planes", "random") for wh in uc.SHAPES for phase in uc.PHASES if uc.valid(wh, phase)]


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def other_stream(ctx):
    s = ctx.stream_create()
    yield s
    ctx.stream_destroy(s)


class _Guarded:
    """A device buffer of shift + nbytes + 256 bytes preset to 0xAB; the payload starts `shift` bytes in."""

    def __init__(self, ctx, nbytes, shift, fill=None):
        self.ctx, self.nbytes, self.shift = ctx, nbytes, shift
        self.base = ctx.malloc(shift + nbytes + GUARD)
        self.ptr = self.base + shift
        self.reset(fill)

    def reset(self, fill=None):
        raw = np.full(self.shift + self.nbytes + GUARD, 0xAB, np.uint8)
        if fill is not None:
            raw[self.shift:self.shift + self.nbytes] = np.ascontiguousarray(fill).view(np.uint8).reshape(-1)
        self.ctx.h2d(self.base, raw)

    def read(self, shape, dtype=np.uint8):
        raw = np.zeros(self.shift + self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.base)
        assert (raw[:self.shift] == 0xAB).all() and (raw[self.shift + self.nbytes:] == 0xAB).all(), "bytes around the buffer were written"
        return raw[self.shift:self.shift + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        raw = np.zeros(self.shift + self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.base)
        return bool((raw == 0xAB).all())

    def free(self):
        self.ctx.free(self.base)


class _Frame:
    """A frame of the cases and its low-resolution side in one phase, on the device; float buffers one float, byte buffers one byte
    into their blocks."""

    def __init__(self, ctx, kind, wh, phase, arrays=None):
        self.ctx, self.wh, self.phase = ctx, wh, phase
        self.W, self.H = wh
        self.w, self.h = uc.size(self.W, self.H, *phase)
        self.pos, self.nrm, self.map = arrays if arrays is not None else uc.gbuffer(kind, wh)
        self.planes, self.mask, self.own_map = uc.low_planes(wh, phase)
        self.keep = uc.keep_map(wh)
        self.lo_pos, self.lo_nrm, self.lo_map = uc.subsample_rule(phase, self.pos, self.nrm, self.map)
        n, m = self.W * self.H, self.w * self.h
        up = lambda a, shift: _Guarded(ctx, a.nbytes, shift, a)
        self.bufs = dict(pos=up(self.pos, 4), nrm=up(self.nrm, 4), map=up(self.map, 1), keep=up(self.keep, 1), lo_pos=up(self.lo_pos, 4),
                         lo_nrm=up(self.lo_nrm, 4), lo_map=up(self.lo_map, 1), own_map=up(self.own_map, 1), lo_planes=up(self.planes, 1),
                         lo_mask=up(self.mask, 1), out=_Guarded(ctx, 8 * n, 1), out_lo_pos=_Guarded(ctx, 16 * m, 4),
                         out_lo_nrm=_Guarded(ctx, 16 * m, 4), out_lo_map=_Guarded(ctx, m, 1))
        self.d = {k: b.ptr for k, b in self.bufs.items()}

    def free(self):
        for b in self.bufs.values():
            b.free()


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2][0]}{c[2][1]}")
def frame(ctx, request):
    f = _Frame(ctx, *request.param)
    yield f
    f.free()


def test_device_equals_the_host_twin(ctx, frame, other_stream):
    f, d = frame, frame.d
    p = uc.params(f.phase)
    n, m = f.W * f.H, f.w * f.h
    # subsample, with and without a map
    for with_map in (True, False):
        for k in ("out_lo_pos", "out_lo_nrm", "out_lo_map"):
            f.bufs[k].reset()
        api.subsample_gbuffer_device(ctx, p, d["pos"], d["nrm"], f.W, f.H, d["out_lo_pos"], d["out_lo_nrm"], d_lights_map=d["map"] if with_map else None,
                                     d_lo_lights_map=d["out_lo_map"] if with_map else None)
        ctx.synchronize()
        want = api.subsample_gbuffer(p, f.pos, f.nrm, f.map if with_map else None)
        assert np.array_equal(f.bufs["out_lo_pos"].read((f.h, f.w, 4), np.uint32), want[0].view(np.uint32))
        assert np.array_equal(f.bufs["out_lo_nrm"].read((f.h, f.w, 4), np.uint32), want[1].view(np.uint32))
        assert np.array_equal(f.bufs["out_lo_map"].read((f.h, f.w)), want[2]) if with_map else f.bufs["out_lo_map"].untouched()
    for count in uc.COUNTS:
        soft, hard = uc.soft_list(count), uc.hard_list(count)
        for i, (with_map, own_low_map) in enumerate(((False, False), (True, False), (True, True))):
            fm, d_fm = (f.map, d["map"]) if with_map else (None, None)
            lm, d_lm = (f.own_map, d["own_map"]) if own_low_map else ((f.lo_map, d["lo_map"]) if with_map else (None, None))
            stream = other_stream if i == 1 and count == 8 else None
            what = (f.wh, f.phase, count, with_map, own_low_map)
            f.bufs["out"].reset()
            api.upsample_retrace_map_device(ctx, count, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], f.W, f.H, d["out"], d_lights_map=d_fm,
                                            d_lo_lights_map=d_lm, stream=stream)
            ctx.synchronize(stream)
            got = f.bufs["out"].read((8, f.H, f.W))
            assert np.array_equal(got[0], api.upsample_retrace_map(count, p, f.pos, f.nrm, f.lo_pos, f.lo_nrm, fm, lm)), ("retrace",) + what
            assert (got[1:] == 0xAB).all()
            for with_keep in (False, True):
                k, d_k = (f.keep, d["keep"]) if with_keep else (None, None)
                f.bufs["out"].reset()
                api.upsample_soft_light_list_device(ctx, soft, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], d["lo_planes"], f.W, f.H, d["out"],
                                                    d_lights_map=d_fm, d_lo_lights_map=d_lm, d_keep=d_k, stream=stream)
                ctx.synchronize(stream)
                got = f.bufs["out"].read((8, f.H, f.W))
                want = api.upsample_soft_light_list(soft, p, f.pos, f.nrm, f.lo_pos, f.lo_nrm, f.planes, fm, lm, k, out=np.full((8, f.H, f.W), 0xAB, np.uint8))
                assert np.array_equal(got, want), ("soft", with_keep) + what
                f.bufs["out"].reset()
                api.upsample_light_list_device(ctx, hard, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], d["lo_mask"], f.W, f.H, d["out"],
                                               d_lights_map=d_fm, d_lo_lights_map=d_lm, d_keep=d_k, stream=stream)
                ctx.synchronize(stream)
                got = f.bufs["out"].read((8, f.H, f.W))
                want = api.upsample_light_list(hard, p, f.pos, f.nrm, f.lo_pos, f.lo_nrm, f.mask, fm, lm, k, out=np.full((f.H, f.W), 0xAB, np.uint8))
                assert np.array_equal(got[0], want), ("hard", with_keep) + what
                assert (got[1:] == 0xAB).all()


@pytest.fixture(scope="module")
def cornell(ctx):
    wl = workload(61, 37)
    ctx.set_bvh(wl.packed)
    return wl


@pytest.mark.parametrize("phase", uc.PHASES, ids=str)
def test_anchor_end_to_end_on_the_device(ctx, cornell, phase):
    """Anchor 4 through the device forms on cornell at 61 x 37, facing map made on the device: G-buffer -> facing map -> subsample ->
    trace at w x h -> retrace map -> masked trace at W x H -> upsample with keep, equal to the plain device trace byte for byte, soft
    and hard; and the same chain at the ordinary thresholds equal to the host twins over the device's own planes."""
    wl, (W, H) = cornell, (61, 37)
    w, h = api.subsampled_size(W, H, *phase)
    n, m, k = W * H, w * h, wl.constants
    soft = make_list("mixed")
    hard = soft.hard_list()
    count = soft.count
    sizes = dict(pos=16 * n, nrm=16 * n, map=n, lo_pos=16 * m, lo_nrm=16 * m, lo_map=m, lo=count * m, keep=n, out=count * n, want=count * n)
    d = {name: ctx.malloc(size) for name, size in sizes.items()}
    try:
        ctx.h2d(d["pos"], wl.pos)
        ctx.h2d(d["nrm"], wl.nrm)
        api.facing_lights_device(ctx, k, hard, d["pos"], d["nrm"], W, H, d["map"])

        def read(name, shape):
            a = np.zeros(shape, np.uint8)
            ctx.d2h(a, d[name])
            return a

        for thresholds in (uc.NONE_ACCEPTED, uc.ORDINARY):
            p = uc.params(phase, thresholds)
            api.subsample_gbuffer_device(ctx, p, d["pos"], d["nrm"], W, H, d["lo_pos"], d["lo_nrm"], d_lights_map=d["map"], d_lo_lights_map=d["lo_map"])
            api.upsample_retrace_map_device(ctx, count, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], W, H, d["keep"], d_lights_map=d["map"],
                                            d_lo_lights_map=d["lo_map"])
            for form in ("soft", "hard"):
                lst, planes = (soft, count) if form == "soft" else (hard, 1)
                trace = ctx.trace_soft_light_list_device if form == "soft" else ctx.trace_light_list_device
                upsample = api.upsample_soft_light_list_device if form == "soft" else api.upsample_light_list_device
                trace(k, lst, d["pos"], W, H, d["want"], d_lights_map=d["map"])
                trace(k, lst, d["lo_pos"], w, h, d["lo"], d_lights_map=d["lo_map"])
                trace(k, lst, d["pos"], W, H, d["out"], d_lights_map=d["keep"])
                upsample(ctx, lst, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], d["lo"], W, H, d["out"], d_lights_map=d["map"],
                         d_lo_lights_map=d["lo_map"], d_keep=d["keep"])
                ctx.synchronize()
                got, want = read("out", (planes, H, W)), read("want", (planes, H, W))
                if thresholds is uc.NONE_ACCEPTED:
                    assert np.array_equal(got, want), (form, phase)
                    assert len(np.unique(want)) > (3 if form == "soft" else 1)
                else:
                    fm, keep = read("map", (H, W)), read("keep", (H, W))
                    lo_pos, lo_nrm, lo_map = api.subsample_gbuffer(p, wl.pos, wl.nrm, fm)
                    assert np.array_equal(keep, api.upsample_retrace_map(count, p, wl.pos, wl.nrm, lo_pos, lo_nrm, fm, lo_map))
                    assert 0 < (keep != 0).sum() < n // 2
                    lo, masked = read("lo", (planes, h, w)), want * 0
                    ctx.h2d(d["out"], np.full(planes * n, 0x5A, np.uint8))
                    upsample(ctx, lst, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], d["lo"], W, H, d["out"], d_lights_map=d["map"],
                             d_lo_lights_map=d["lo_map"], d_keep=d["keep"])
                    ctx.synchronize()
                    masked[:] = 0x5A
                    twin = api.upsample_soft_light_list if form == "soft" else api.upsample_light_list
                    host = twin(lst, p, wl.pos, wl.nrm, lo_pos, lo_nrm, lo if form == "soft" else lo[0], fm, lo_map, keep,
                                out=masked if form == "soft" else masked[0])
                    assert np.array_equal(read("out", (planes, H, W)).reshape(host.shape), host), (form, phase)
    finally:
        for ptr in d.values():
            ctx.free(ptr)


@pytest.mark.parametrize("form", ["subsample", "retrace", "soft", "hard"])
def test_graph_capture_adds_one_kernel_node(ctx, other_stream, form):
    """Captured, every device form is ONE kernel node, parameters by value: the host struct may change before the graph runs."""
    f = _Frame(ctx, "planes", (64, 40), (1, 1))
    d = f.d
    try:
        p = uc.params(f.phase)
        soft, hard = uc.soft_list(8), uc.hard_list(8)
        s = other_stream
        launch = dict(
            subsample=lambda: api.subsample_gbuffer_device(ctx, p, d["pos"], d["nrm"], f.W, f.H, d["out_lo_pos"], d["out_lo_nrm"], d_lights_map=d["map"],
                                                           d_lo_lights_map=d["out_lo_map"], stream=s),
            retrace=lambda: api.upsample_retrace_map_device(ctx, 8, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], f.W, f.H, d["out"],
                                                            d_lights_map=d["map"], d_lo_lights_map=d["lo_map"], stream=s),
            soft=lambda: api.upsample_soft_light_list_device(ctx, soft, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], d["lo_planes"], f.W, f.H,
                                                             d["out"], d_lights_map=d["map"], d_lo_lights_map=d["lo_map"], d_keep=d["keep"], stream=s),
            hard=lambda: api.upsample_light_list_device(ctx, hard, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], d["lo_mask"], f.W, f.H, d["out"],
                                                        d_lights_map=d["map"], d_lo_lights_map=d["lo_map"], d_keep=d["keep"], stream=s))[form]
        g = hipgraph.capture(s, launch)
        try:
            assert g.node_types() == [hipgraph.KERNEL], (form, g.node_types())
            assert f.bufs["out"].untouched() and f.bufs["out_lo_map"].untouched(), "the capture itself ran the kernel"
            p.phase_x, p.plane_eps = 0, -1.0                              # by value: the graph holds its own copy
            g.launch(s)
            ctx.synchronize(s)
            p = uc.params(f.phase)
            if form == "subsample":
                assert np.array_equal(f.bufs["out_lo_map"].read((f.h, f.w)), f.lo_map)
                assert np.array_equal(f.bufs["out_lo_nrm"].read((f.h, f.w, 4), np.uint32), f.lo_nrm.view(np.uint32))
            elif form == "retrace":
                assert np.array_equal(f.bufs["out"].read((8, f.H, f.W))[0], api.upsample_retrace_map(8, p, f.pos, f.nrm, f.lo_pos, f.lo_nrm, f.map, f.lo_map))
            elif form == "soft":
                want = api.upsample_soft_light_list(soft, p, f.pos, f.nrm, f.lo_pos, f.lo_nrm, f.planes, f.map, f.lo_map, f.keep,
                                                    out=np.full((8, f.H, f.W), 0xAB, np.uint8))
                assert np.array_equal(f.bufs["out"].read((8, f.H, f.W)), want)
            else:
                want = api.upsample_light_list(hard, p, f.pos, f.nrm, f.lo_pos, f.lo_nrm, f.mask, f.map, f.lo_map, f.keep,
                                               out=np.full((f.H, f.W), 0xAB, np.uint8))
                assert np.array_equal(f.bufs["out"].read((8, f.H, f.W))[0], want)
        finally:
            g.close()
    finally:
        f.free()


def test_refusals_write_nothing(ctx):
    """Every refusal of include/rts_scene.h: RTS_ERR_INVALID_ARG, nothing launched, and not a byte of any output."""
    lib, h, v = api._lib, ctx.handle, C.c_void_p
    f = _Frame(ctx, "planes", (9, 7), (1, 0))
    d = f.d
    ref = lambda s: C.byref(s) if s is not None else None
    good = uc.params(f.phase)

    def bad_params():
        out = [None]
        for field, value in (("phase_x", 2), ("phase_y", 2), ("normal_cos_min", np.nan), ("plane_eps", np.inf)):
            q = uc.params(f.phase)
            setattr(q, field, value)
            out.append(q)
        return out

    def sub(c=h, p=good, P=d["pos"], N=d["nrm"], a=d["out_lo_pos"], b=d["out_lo_nrm"], m=d["out_lo_map"], W=9, H=7):
        return lib.rtsh_subsample_gbuffer_device(c, ref(p), v(P), v(N), v(d["map"]), W, H, v(a), v(b), v(m), None)

    def ret(c=h, count=3, p=good, P=d["pos"], N=d["nrm"], LP=d["lo_pos"], LN=d["lo_nrm"], W=9, H=7, out=d["out"]):
        return lib.rtsh_upsample_retrace_map_device(c, count, ref(p), v(P), v(N), v(d["map"]), v(LP), v(LN), v(d["lo_map"]), W, H, v(out), None)

    def up(form, lst, c=h, p=good, P=d["pos"], N=d["nrm"], LP=d["lo_pos"], LN=d["lo_nrm"], LC=True, W=9, H=7, out=d["out"], alias=False):
        fn = lib.rtsh_upsample_soft_light_list_device if form == "soft" else lib.rtsh_upsample_light_list_device
        lo = d["lo_planes"] if form == "soft" else d["lo_mask"]
        return fn(c, ref(lst), ref(p), v(P), v(N), v(d["map"]), v(LP), v(LN), v(d["lo_map"]), v(lo if LC else 0), v(d["keep"]), W, H,
                  v(lo if alias else out), None)

    try:
        for p in bad_params():
            assert sub(p=p) == INVALID and ret(p=p) == INVALID
        for kw in (dict(c=None), dict(P=0), dict(N=0), dict(a=0), dict(b=0), dict(m=0), dict(W=0), dict(H=0)):
            assert sub(**kw) == INVALID, kw
        for kw in (dict(c=None), dict(count=0), dict(count=9), dict(P=0), dict(N=0), dict(LP=0), dict(LN=0), dict(W=0), dict(H=0), dict(out=0),
                   dict(H=8 * 65535 + 1)):
            assert ret(**kw) == INVALID, kw
        hard_bad, soft_bad = lc.bad_lists()
        for form, lst, bad in (("soft", uc.soft_list(3), soft_bad), ("hard", uc.hard_list(3), hard_bad)):
            for b in bad:
                assert up(form, b) == INVALID, form
            for p in bad_params():
                assert up(form, lst, p=p) == INVALID, form
            for kw in (dict(c=None), dict(P=0), dict(N=0), dict(LP=0), dict(LN=0), dict(LC=False), dict(W=0), dict(H=0), dict(out=0),
                       dict(alias=True), dict(H=8 * 65535 + 1)):
                assert up(form, lst, **kw) == INVALID, (form, kw)
        q = uc.params((1, 1))
        for W, H in ((1, 5), (5, 1), (1, 1)):                             # phase 1 on a frame one pixel wide or tall
            assert sub(p=q, W=W, H=H) == INVALID and ret(p=q, W=W, H=H) == INVALID
            assert up("soft", uc.soft_list(3), p=q, W=W, H=H) == INVALID and up("hard", uc.hard_list(3), p=q, W=W, H=H) == INVALID
        ctx.synchronize()
        for name in ("out", "out_lo_pos", "out_lo_nrm", "out_lo_map"):
            assert f.bufs[name].untouched(), name
        before = f.bufs["lo_planes"].read((8, f.h, f.w))
        assert np.array_equal(before, f.planes), "the aliased call wrote the low-resolution planes"
    finally:
        f.free()
