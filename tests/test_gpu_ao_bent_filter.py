"""GPU: the wide filter of the bent plane (rtsh_wide_filter_bent_device; wideBentKernel of raytracedshadows_amd/csrc/rts_wide_bent.inc,
included by rts_primary.hip): device = host twin = the numpy rule of tests/ao_bent_filter_cases.py, bit for bit.
passes 0 .. 5 take every kernel: the conversion (passes 0), the dense LDS window (steps 1, 2, 4) and the direct global taps (steps 8,
16).  `out`, `ao` and the scratch carry 256 spare bytes preset to 0xAB on both sides that must come back unchanged; the scratch's second
half stays untouched for passes <= 2 and all of it for passes <= 1."""
import ctypes as C

import numpy as np
import pytest

import ao_bent_filter_cases as bf
import hipgraph
import list_wide_filter_cases as wc
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID = 1
f32 = np.float32
FRAMES = [(72, 40), (17, 1), (3, 2), (72, 72)]
SAMPLES = (4, 48)


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
    """A device buffer of 256 + nbytes + 256 bytes, all of it preset to 0xAB; the payload starts 256 bytes in (16-byte aligned)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.base = ctx.malloc(2 * GUARD + nbytes)
        self.ptr = self.base + GUARD
        self.reset()

    def reset(self):
        self.ctx.h2d(self.base, np.full(2 * GUARD + self.nbytes, 0xAB, np.uint8))

    def raw(self):
        raw = np.zeros(2 * GUARD + self.nbytes, np.uint8)
        self.ctx.d2h(raw, self.base)
        return raw

    def read(self, shape, dtype=np.uint8):
        raw = self.raw()
        assert (raw[:GUARD] == 0xAB).all() and (raw[GUARD + self.nbytes:] == 0xAB).all(), "bytes around the buffer were written"
        return raw[GUARD:GUARD + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.raw() == 0xAB).all())

    def free(self):
        self.ctx.free(self.base)


class _Frame:
    """A G-buffer on the device with room for one bent plane and one `active` map, and guarded out, ao and scratch."""

    def __init__(self, ctx, W, H, pos, nrm):
        self.ctx, self.W, self.H, self.pos, self.nrm = ctx, W, H, np.ascontiguousarray(pos, f32), np.ascontiguousarray(nrm, f32)
        n = W * H
        self.d_pos, self.d_nrm, self.d_bent, self.d_act = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n + 8)
        ctx.h2d(self.d_pos, self.pos)
        ctx.h2d(self.d_nrm, self.nrm)
        self.out, self.ao, self.scratch = _Guarded(ctx, n * 16), _Guarded(ctx, n * 4), _Guarded(ctx, 2 * n * 8)
        assert api.wide_filter_bent_scratch_bytes(W, H) == 2 * n * 8

    def upload(self, bent=None, active=None):
        if bent is not None:
            self.ctx.h2d(self.d_bent, np.ascontiguousarray(bent, f32))
        if active is not None:
            self.ctx.h2d(self.d_act, np.ascontiguousarray(active, np.uint8))

    def launch(self, p, n, with_active, stream=None, scratch=True, ao=True):
        api.wide_filter_bent_device(self.ctx, p, n, self.d_pos, self.d_nrm, self.d_bent, self.W, self.H, self.out.ptr,
                                    d_ao=self.ao.ptr if ao else None, d_scratch=self.scratch.ptr if scratch else None,
                                    d_active=self.d_act if with_active else None, stream=stream)

    def run(self, p, n, with_active, stream=None, scratch=True, ao=True):
        """One call into freshly preset out, ao and scratch -> (out[H, W, 4], ao[H, W] or None); nothing else may be written: the
        guard bytes, the scratch's second half for passes <= 2, all of it for passes <= 1, `ao` when it is not given."""
        for g in (self.out, self.ao, self.scratch):
            g.reset()
        self.launch(p, n, with_active, stream, scratch, ao)
        self.ctx.synchronize(stream)
        texels = self.scratch.read((2, self.W * self.H), np.uint64)
        if p.passes <= 2:
            assert (texels[1] == 0xABABABABABABABAB).all(), "the second half of the scratch was written"
        if p.passes <= 1:
            assert (texels[0] == 0xABABABABABABABAB).all(), "the scratch was written"
        plane = self.ao.read((self.H, self.W), f32)
        if not ao:
            assert (plane.view(np.uint32) == 0xABABABAB).all(), "ao was written"
        return self.out.read((self.H, self.W, 4), f32), plane if ao else None

    def free(self):
        for d in (self.d_pos, self.d_nrm, self.d_bent, self.d_act):
            self.ctx.free(d)
        for g in (self.out, self.ao, self.scratch):
            g.free()


@pytest.mark.parametrize("wh", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_twin_and_the_rule(ctx, other_stream, wh):
    """Awkward, geometric and flat frames; passes 0 .. 5; n of 4 and 48; with and without `active`; one run per frame on a second
    stream, one without `ao`, the passes <= 1 runs of one case without scratch."""
    for kind in wc.kinds(wh):
        nrm, pos, _, _, lights_map, _ = wc.frame(kind, wh)
        f = _Frame(ctx, wh[0], wh[1], pos, nrm)
        try:
            active = bf.active_map(lights_map)
            f.upload(active=active)
            for n in SAMPLES:
                bent = bf.synthetic_bent(wh, n)
                f.upload(bent=bent)
                for with_active in (False, True):
                    a = active if with_active else None
                    want = bf.bent_filter_rule(bf.params(0, kind), n, pos, nrm, bent, a)
                    for passes in bf.PASSES:
                        p = bf.params(passes, kind)
                        stream = other_stream if passes == 3 and n == 4 else None
                        with_ao = not (passes == 4 and n == 48)
                        got, plane = f.run(p, n, with_active, stream, scratch=not (passes <= 1 and n == 48), ao=with_ao)
                        what = (kind, wh, n, with_active, passes)
                        bf.same_bits(got, want[passes], what)
                        if with_ao:
                            bf.same_bits(plane, want[passes][..., 3], what + ("ao",))
                        twin, twin_ao = api.wide_filter_bent(p, n, pos, nrm, bent, a)
                        bf.same_bits(got, twin, what + ("twin",))
        finally:
            f.free()


def test_fed_from_the_trace_and_anchor_1(ctx):
    """The bent plane straight from trace_ambient_occlusion_bent_device on the (48, 40) cornell frame -- never through the host --:
    the filter's planes equal the rule over the rule's trace, and out.w and ao equal wide_filter_soft_light_list_device over the trace's
    own counts under the stand-in list, bit for bit, for every passes."""
    n = 4
    fr, ao, counts, bent = bf.traced("cornell_128", 48, 40, n, 64, 0.05)
    W, H = fr.W, fr.H
    f = _Frame(ctx, W, H, fr.pos, fr.nrm)
    d_counts, vis = ctx.malloc(W * H), _Guarded(ctx, W * H * 4)
    d_wide = ctx.malloc(api.wide_filter_scratch_bytes(1, W, H))
    try:
        ctx.set_bvh(fr.packed)
        ctx.trace_ambient_occlusion_bent_device(fr.k, ao, f.d_pos, f.d_nrm, W, H, d_counts, f.d_bent)
        ctx.synchronize()
        want = bf.bent_filter_rule(bf.traced_params(fr, 0), n, fr.pos, fr.nrm, bent)
        lst = ao.stand_in_list()
        for passes in bf.PASSES:
            p = bf.traced_params(fr, passes)
            got, plane = f.run(p, n, False)
            bf.same_bits(got, want[passes], ("traced", passes))
            vis.reset()
            api.wide_filter_soft_light_list_device(ctx, lst, p, f.d_pos, f.d_nrm, d_counts, W, H, vis.ptr, d_scratch=d_wide)
            ctx.synchronize()
            shipped = vis.read((H, W), f32)
            bf.same_bits(plane, shipped, ("anchor 1: ao", passes))
            bf.same_bits(got[..., 3], shipped, ("anchor 1: out.w", passes))
    finally:
        f.free()
        vis.free()
        ctx.free(d_counts)
        ctx.free(d_wide)


def test_a_lonely_pixel_and_an_empty_frame(ctx):
    """A frame of whole blocks (32 x 48) whose only active pixel is the last lane of the last block, and one with no active pixel: all +0
    but the lonely texel, at the conversion, at dense steps and at direct ones."""
    wh = (32, 48)
    nrm, pos, _, _, _, _ = wc.frame("flat", wh)
    nrm = np.array(nrm)
    nrm[-1, -1, :3] = (0.0, 1.0, 0.0)                                        # a surface there whatever the frame sprinkled
    W, H = wh
    bent = bf.synthetic_bent(wh, 4)
    f = _Frame(ctx, W, H, pos, nrm)
    try:
        f.upload(bent=bent)
        for lonely in (True, False):
            active = np.zeros((H, W), np.uint8)
            active[-1, -1] = 7 if lonely else 0
            f.upload(active=active)
            want = bf.bent_filter_rule(bf.params(0, "flat"), 4, pos, nrm, bent, active)
            for passes in (0, 1, 3, 5):
                got, plane = f.run(bf.params(passes, "flat"), 4, True)
                bf.same_bits(got, want[passes], (lonely, passes))
                bf.same_bits(plane, want[passes][..., 3], (lonely, passes, "ao"))
                assert (bf.bits(got).reshape(-1, 4)[:-1] == 0).all() and (bf.bits(plane).reshape(-1)[:-1] == 0).all()
                assert bool(bf.bits(got)[-1, -1].any()) == lonely
    finally:
        f.free()


@pytest.mark.parametrize("passes", [0, 1, 2, 5])
def test_graph_capture_adds_one_kernel_node_per_pass(ctx, other_stream, passes):
    """Captured, the device form is max(1, passes) kernel nodes, parameters by value; a replay filters `bent` and `active` as they are
    on the device THEN."""
    wh, n = (72, 40), 4
    nrm, pos, _, _, lights_map, _ = wc.frame("flat", wh)
    f = _Frame(ctx, wh[0], wh[1], pos, nrm)
    try:
        bent, active = bf.synthetic_bent(wh, n), bf.active_map(lights_map)
        f.upload(bent, active)
        p = bf.params(passes, "flat")
        want = bf.bent_filter_rule(p, n, pos, nrm, bent, active)[passes]
        g = hipgraph.capture(other_stream, lambda: f.launch(p, n, True, other_stream))
        try:
            assert g.node_types() == [hipgraph.KERNEL] * max(1, passes), (passes, g.node_types())
            assert f.out.untouched() and f.ao.untouched() and f.scratch.untouched(), "the capture itself ran a kernel"
            p.passes, p.plane_eps = (passes + 1) % 6, 0.0                    # by value: the graph holds its own copy
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            bf.same_bits(f.out.read((f.H, f.W, 4), f32), want, (passes, "first replay"))
            bent2 = np.array(bent)[::-1, ::-1].copy()
            active2 = (np.asarray(active) ^ 0xFF).astype(np.uint8)
            f.upload(bent2, active2)
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            want2 = bf.bent_filter_rule(bf.params(passes, "flat"), n, pos, nrm, bent2, active2)[passes]
            assert (bf.bits(want2) != bf.bits(want)).any()
            bf.same_bits(f.out.read((f.H, f.W, 4), f32), want2, (passes, "replay over changed planes"))
            bf.same_bits(f.ao.read((f.H, f.W), f32), want2[..., 3], (passes, "replay, ao"))
        finally:
            g.close()
    finally:
        f.free()


def test_refusals_launch_nothing(ctx):
    """Every refusal of include/rts_scene.h: RTS_ERR_INVALID_ARG, and not a byte of out, ao or scratch."""
    lib = api._lib
    nrm, pos, _, _, lights_map, _ = wc.frame("geometric", (16, 16))
    f = _Frame(ctx, 16, 16, pos, nrm)
    f.upload(bf.synthetic_bent((16, 16), 4), bf.active_map(lights_map))
    h, v = ctx.handle, C.c_void_p
    ref = lambda s: C.byref(s) if s is not None else None
    good = bf.params(3)
    half = 16 * 16 * 8

    def call(p, n=4, ctx_=h, pos_=f.d_pos, nrm_=f.d_nrm, bent=f.d_bent, W=16, H=16, out=f.out.ptr, ao=f.ao.ptr, scratch=f.scratch.ptr):
        return lib.rtsh_wide_filter_bent_device(ctx_, ref(p), n, v(pos_), v(nrm_), v(f.d_act), v(bent), W, H, v(out), v(ao), v(scratch), None)

    try:
        bad = [None]
        for field, value in (("passes", 6), ("passes", 0xFFFFFFFF), ("normal_cos_min", np.nan), ("normal_cos_min", np.inf),
                             ("plane_eps", -np.inf), ("plane_eps", np.nan)):
            p = bf.params(3)
            setattr(p, field, value)
            bad.append(p)
        for p in bad:
            assert call(p) == INVALID
        for n in (49, 0xFFFFFFFF):
            assert call(good, n=n) == INVALID
        assert call(good, ctx_=None) == INVALID
        assert call(good, pos_=0) == INVALID
        assert call(good, nrm_=0) == INVALID
        assert call(good, bent=0) == INVALID
        assert call(good, out=0) == INVALID
        assert call(good, W=0) == INVALID
        assert call(good, H=0) == INVALID
        assert call(good, W=0x7FFFFFF1, H=1) == INVALID
        assert call(good, W=1, H=16 * 65535 + 1) == INVALID                  # the grid's y extent
        assert call(bf.params(2), scratch=0) == INVALID                      # passes >= 2 need the scratch
        for alias in (f.d_bent, f.scratch.ptr, f.scratch.ptr + half):
            assert call(good, out=alias) == INVALID                          # out on bent, on the scratch, on its second half
            assert call(good, ao=alias) == INVALID                           # ... and ao
        assert call(good, bent=f.d_bent + 4) == INVALID                      # whole texels: 16-byte alignment
        assert call(good, out=f.out.ptr + 8) == INVALID
        assert call(good, scratch=f.scratch.ptr + 4) == INVALID              # 8-byte texels
        ctx.synchronize()
        assert f.out.untouched() and f.ao.untouched() and f.scratch.untouched()
        bent_back = np.zeros((16, 16, 4), f32)
        ctx.d2h(bent_back, f.d_bent)
        bf.same_bits(bent_back, bf.synthetic_bent((16, 16), 4), "bent")
        assert call(bf.params(1), scratch=0) == 0 and call(bf.params(0), scratch=0, ao=0) == 0   # no scratch needed, ao optional
        ctx.synchronize()
    finally:
        f.free()
