"""GPU: the wide (a-trous) filter of a light list's planes (rtsh_wide_filter_light_list_device, rtsh_wide_filter_soft_light_list_device;
wideFilterKernel of raytracedshadows_amd/csrc/rts_wide_filter.inc, included by rts_primary.hip) on the frames of
tests/list_wide_filter_cases.py: the device forms equal the host twins bit for bit (the twins equal the numpy rule in
tests/test_list_wide_filter_host.py).  passes 0 .. 5 take every kernel: the conversion (passes 0), the dense LDS window (steps 1, 2, 4)
and the direct global taps (steps 8, 16) -- each step ships with ONE staging form whatever the list, so there is no second branch of the
launcher to steer.  Every frame runs once with all pointers as allocated and once with the byte planes and the map one byte, the float
planes one float and the scratch one uint16_t into a larger allocation.  Visibility and scratch carry 256 spare bytes preset to 0xAB
(and the bytes in front of a shifted one) that must come back unchanged.  No BVH is installed: the passes need none."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import list_combine_cases as lc
import list_wide_filter_cases as wc
import scene_pass_cases as sp
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID = 1
f32 = np.float32
#: (form, count, rotation, with map) of the runs over a frame
RUNS = [("soft", 8, 1, True), ("hard", 8, 0, False), ("soft", 4, 0, False), ("hard", 4, 0, True), ("soft", 1, 1, True)]


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
    """A device buffer of shift + nbytes + 256 bytes, all of it preset to 0xAB; the payload starts `shift` bytes in."""

    def __init__(self, ctx, nbytes, shift):
        self.ctx, self.nbytes, self.shift = ctx, nbytes, shift
        self.base = ctx.malloc(shift + nbytes + GUARD)
        self.ptr = self.base + shift
        self.reset()

    def reset(self):
        self.ctx.h2d(self.base, np.full(self.shift + self.nbytes + GUARD, 0xAB, np.uint8))

    def raw(self):
        raw = np.zeros(self.shift + self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.base)
        return raw

    def read(self, shape, dtype=np.uint8):
        raw = self.raw()
        assert (raw[:self.shift] == 0xAB).all() and (raw[self.shift + self.nbytes:] == 0xAB).all(), "bytes around the buffer were written"
        return raw[self.shift:self.shift + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.raw() == 0xAB).all())

    def free(self):
        self.ctx.free(self.base)


class _Frame:
    """A frame of the cases on the device; `shift` 1 puts the byte planes and the map one byte, the float planes one float and the
    scratch one uint16_t into their blocks.  The scratch is allocated for eight lights; a run with fewer must leave the rest alone."""

    def __init__(self, ctx, kind, wh, shift):
        self.ctx, self.kind, self.wh, self.shift = ctx, kind, wh, shift
        self.W, self.H = wh
        self.nrm, self.pos, self.planes, self.mask, self.map, _ = wc.frame(kind, wh)
        n = self.W * self.H
        self._blocks = [ctx.malloc(n * 16 + 16), ctx.malloc(n * 16 + 16), ctx.malloc(8 * n + 8), ctx.malloc(n + 8), ctx.malloc(n + 8)]
        self.d_nrm, self.d_pos = (b + 4 * shift for b in self._blocks[:2])
        self.d_planes, self.d_mask, self.d_map = (b + shift for b in self._blocks[2:])
        ctx.h2d(self.d_nrm, self.nrm)
        ctx.h2d(self.d_pos, self.pos)
        self.upload(self.planes, self.mask, self.map)
        self.vis = _Guarded(ctx, 8 * n * 4, 4 * shift)
        self.scratch = _Guarded(ctx, 2 * 8 * n * 2, 2 * shift)
        self.rgb = _Guarded(ctx, n * 3, shift)

    def upload(self, planes=None, mask=None, lights_map=None):
        for ptr, a in ((self.d_planes, planes), (self.d_mask, mask), (self.d_map, lights_map)):
            if a is not None:
                self.ctx.h2d(ptr, np.ascontiguousarray(a))

    def launch(self, form, lst, p, with_map, stream=None, scratch=True):
        fn = api.wide_filter_light_list_device if form == "hard" else api.wide_filter_soft_light_list_device
        fn(self.ctx, lst, p, self.d_pos, self.d_nrm, self.d_mask if form == "hard" else self.d_planes, self.W, self.H, self.vis.ptr,
           d_scratch=self.scratch.ptr if scratch else None, d_lights_map=self.d_map if with_map else None, stream=stream)

    def run(self, form, lst, p, with_map, stream=None, scratch=True):
        """One call into the freshly preset visibility and scratch; returns planes 0 .. count - 1 and checks that nothing else was
        written: the planes of visibility from the count up, the scratch behind its 2 * count planes (all of it for passes <= 1), and
        the guard bytes of both."""
        self.vis.reset()
        self.scratch.reset()
        self.launch(form, lst, p, with_map, stream, scratch)
        self.ctx.synchronize(stream)
        vis = self.vis.read((8, self.H, self.W), f32)
        assert (vis[lst.count:].view(np.uint32) == 0xABABABAB).all(), "a plane of visibility from the count up was written"
        words = self.scratch.read((2 * 8 * self.W * self.H,), np.uint16)
        used = 2 * lst.count * self.W * self.H if p.passes >= 2 else 0
        assert (words[used:] == 0xABAB).all(), "the scratch was written behind its 2 * count planes"
        return vis[:lst.count]

    def twin(self, form, lst, p, with_map, planes=None, mask=None):
        m = self.map if with_map else None
        if form == "hard":
            return api.wide_filter_light_list(lst, p, self.pos, self.nrm, self.mask if mask is None else mask, m)
        return api.wide_filter_soft_light_list(lst, p, self.pos, self.nrm, self.planes if planes is None else planes, m)

    def free(self):
        for b in self._blocks:
            self.ctx.free(b)
        self.vis.free()
        self.scratch.free()
        self.rgb.free()


@pytest.fixture(scope="module", params=[(wh, shift) for wh in wc.FRAMES for shift in (0, 1)], ids=lambda p: f"{p[0][0]}x{p[0][1]}+{p[1]}")
def frames(ctx, request):
    wh, shift = request.param
    group = [_Frame(ctx, kind, wh, shift) for kind in wc.kinds(wh)]
    yield group
    for f in group:
        f.free()


def test_device_equals_the_host_twin(ctx, frames, other_stream):
    """passes 0 .. 5 on the awkward, geometric and flat frames; hard and soft lists of 1, 4 and 8 lights, with and without the map; one
    run per frame on a second stream; a passes <= 1 run without scratch."""
    for f in frames:
        for i, (form, count, rotation, with_map) in enumerate(RUNS):
            lst = wc.the_list(form, count, rotation)
            for passes in wc.PASSES:
                p = wc.params(passes, f.kind)
                stream = other_stream if i == 0 and passes == 3 else None
                got = f.run(form, lst, p, with_map, stream, scratch=not (i == 1 and passes <= 1))
                wc.same_bits(got, f.twin(form, lst, p, with_map), (f.kind, f.wh, f.shift, form, count, rotation, with_map, passes))


def test_downstream_passes_equal_their_twins(ctx, frames):
    """The device visibility combine, and accumulate_visibility_list_device with max_length 1, over a wide-filtered plane equal their
    host twins over the twin's plane; and the combine over a passes == 0 plane of clamped counts gives the list combine's bytes."""
    k = sp.constants("unit")
    f = frames[-1]
    n = f.W * f.H
    soft = wc.the_list("soft", 8, 1)
    hard = soft.hard_list()
    out, lengths = _Guarded(ctx, 8 * n * 4, 4 * f.shift), _Guarded(ctx, 8 * n, f.shift)
    try:
        for passes in (0, 3, 5):
            p = wc.params(passes, f.kind)
            want = f.twin("soft", soft, p, True)
            f.vis.reset()
            f.launch("soft", soft, p, True)
            f.rgb.reset()
            api.combine_visibility_list_device(ctx, k, hard, f.d_pos, f.d_nrm, f.vis.ptr, f.W, f.H, f.rgb.ptr, d_lights_map=f.d_map)
            tp = api.TemporalParams.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, -1), 1.0, 1.0, max_length=1)
            out.reset()
            lengths.reset()
            api.accumulate_visibility_list_device(ctx, hard, tp, f.d_pos, f.d_nrm, f.vis.ptr, f.W, f.H, out.ptr, lengths.ptr, d_lights_map=f.d_map)
            ctx.synchronize()
            assert (f.rgb.read((f.H, f.W, 3)) == api.combine_visibility_list(k, hard, f.pos, f.nrm, want, f.map)).all(), (f.wh, passes)
            want_vis, want_len = api.accumulate_visibility_list(hard, tp, f.pos, f.nrm, want, None, f.map)
            wc.same_bits(out.read((8, f.H, f.W), f32)[:8], want_vis, ("accumulate", f.wh, passes))
            assert (lengths.read((8, f.H, f.W)) == want_len).all()
        tame = np.minimum(f.planes, np.array(wc.samples_of(soft)).reshape(-1, 1, 1)).astype(np.uint8)
        f.upload(planes=tame)
        f.vis.reset()
        f.launch("soft", soft, wc.params(0, f.kind), True)
        f.rgb.reset()
        api.combine_visibility_list_device(ctx, k, hard, f.d_pos, f.d_nrm, f.vis.ptr, f.W, f.H, f.rgb.ptr, d_lights_map=f.d_map)
        ctx.synchronize()
        assert (f.rgb.read((f.H, f.W, 3)) == api.combine_soft_light_list(k, soft, f.pos, f.nrm, tame, f.map)).all(), f.wh
    finally:
        f.upload(planes=f.planes)
        out.free()
        lengths.free()


def test_refusals_launch_nothing(ctx):
    """Every refusal of include/rts_scene.h: RTS_ERR_INVALID_ARG, and not a byte of visibility or scratch."""
    lib = api._lib
    f = _Frame(ctx, "geometric", (16, 16), 0)
    h, v = ctx.handle, C.c_void_p
    ref = lambda s: C.byref(s) if s is not None else None
    good = wc.params(3)
    hard_bad, soft_bad = lc.bad_lists()
    hard, soft = wc.the_list("hard", 4), wc.the_list("soft", 4, 1)
    half = 4 * 16 * 16 * 2                                               # bytes of one ping-pong set of four planes

    def call(form, lst, p, ctx_=h, pos=f.d_pos, nrm=f.d_nrm, plane=True, W=16, H=16, out=f.vis.ptr, scratch=f.scratch.ptr):
        fn = lib.rtsh_wide_filter_light_list_device if form == "hard" else lib.rtsh_wide_filter_soft_light_list_device
        return fn(ctx_, ref(lst), ref(p), v(pos), v(nrm), v(f.d_map), v((f.d_mask if form == "hard" else f.d_planes) if plane else 0), W, H,
                  v(out), v(scratch), None)

    def bad_params():
        out = [None]
        for field, value in (("passes", 6), ("passes", 0xFFFFFFFF), ("normal_cos_min", np.nan), ("normal_cos_min", np.inf),
                             ("plane_eps", -np.inf), ("plane_eps", np.nan)):
            p = wc.params(3)
            setattr(p, field, value)
            out.append(p)
        return out

    try:
        for form, lst, bad in (("hard", hard, hard_bad), ("soft", soft, soft_bad)):
            for b in bad:
                assert call(form, b, good) == INVALID, form
            for p in bad_params():
                assert call(form, lst, p) == INVALID, form
            assert call(form, lst, good, ctx_=None) == INVALID
            assert call(form, lst, good, pos=0) == INVALID
            assert call(form, lst, good, nrm=0) == INVALID
            assert call(form, lst, good, plane=False) == INVALID
            assert call(form, lst, good, out=0) == INVALID
            assert call(form, lst, good, W=0) == INVALID
            assert call(form, lst, good, H=0) == INVALID
            assert call(form, lst, good, W=0x7FFFFFF1, H=1) == INVALID
            assert call(form, lst, good, W=1, H=16 * 65535 + 1) == INVALID             # the grid's y extent
            assert call(form, lst, wc.params(2), scratch=0) == INVALID                  # passes >= 2 need the scratch
            assert call(form, lst, good, out=f.scratch.ptr) == INVALID                  # visibility overlapping the scratch
            assert call(form, lst, good, out=f.scratch.ptr + half) == INVALID           # ... or its second half
        ctx.synchronize()
        assert f.vis.untouched() and f.scratch.untouched()
    finally:
        f.free()


@pytest.mark.parametrize("form,passes", [("soft", 0), ("soft", 1), ("soft", 3), ("hard", 5)], ids=["soft-0", "soft-1", "soft-3", "hard-5"])
def test_graph_capture_adds_one_kernel_node_per_pass(ctx, other_stream, form, passes):
    """Captured, a device form is max(1, passes) kernel nodes -- list and parameters by value, so the host structs may change before the
    graph runs -- and a replay filters the planes as they are THEN: overwritten counts give the changed frame's floats."""
    f = _Frame(ctx, "flat", (72, 40), 1)
    try:
        lst = wc.the_list(form, 8, 1)
        p = wc.params(passes)
        want = f.twin(form, lst, p, True)
        f.vis.reset()
        g = hipgraph.capture(other_stream, lambda: f.launch(form, lst, p, True, other_stream))
        try:
            assert g.node_types() == [hipgraph.KERNEL] * max(1, passes), (form, passes, g.node_types())
            assert f.vis.untouched(), "the capture itself ran a kernel"
            p.passes, p.plane_eps = (passes + 1) % 6, 0.0                  # by value: the graph holds its own copy
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            wc.same_bits(f.vis.read((8, f.H, f.W), f32), want, (form, passes, "first replay"))
            changed, changed_mask = (f.planes[::-1] // 2).copy(), f.mask ^ 0x5A
            f.upload(changed, changed_mask)
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            want2 = f.twin(form, lst, wc.params(passes), True, planes=changed, mask=changed_mask)
            assert (want2 != want).any()
            wc.same_bits(f.vis.read((8, f.H, f.W), f32), want2, (form, passes, "replay over changed planes"))
        finally:
            g.close()
    finally:
        f.free()
