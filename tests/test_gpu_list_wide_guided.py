"""GPU: the variance-guided wide filter of a soft light list's planes (rtsh_wide_filter_guided_soft_light_list_device; wideGuidedKernel
of raytracedshadows_amd/csrc/rts_wide_guided.inc, included by rts_primary.hip) on the frames and count planes of
tests/list_wide_guided_cases.py: the device form equals the host twin bit for bit (the twin equals the numpy rule in
tests/test_list_wide_guided_host.py).  passes 0 .. 5 take every kernel form: the conversion (passes 0), a first pass that is also the
last (passes 1: T is formed and not stored), the first pass that stores T, the dense LDS window (steps 1, 2, 4) and the direct global
taps (steps 8, 16) reading T back; guide_k4 0, 12 and 255.  Every frame runs once with all pointers as allocated and once with the byte
planes and the map one byte, the float planes one float and the scratch one uint16_t into a larger allocation.  Visibility and scratch
carry 256 spare bytes preset to 0xAB (and the bytes in front of a shifted one) that must come back unchanged; the scratch is allocated
for eight lights and a run may write its 3 * count planes only, none of them for passes <= 1.  No BVH is installed."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import list_combine_cases as lc
import list_wide_guided_cases as gc
import scene_pass_cases as sp
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID = 1
f32 = np.float32
K4 = [0, 12, 255]
#: (count, rotation, with map) of the runs over a frame
RUNS = [(8, 1, True), (4, 0, False), (1, 1, True)]


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


_TWINS = {}


class _Frame:
    """A frame of the cases on the device; `shift` 1 puts the byte planes and the map one byte, the float planes one float and the
    scratch one uint16_t into their blocks.  The count planes are uploaded per list (they depend on its n_l)."""

    def __init__(self, ctx, kind, wh, shift):
        self.ctx, self.kind, self.wh, self.shift = ctx, kind, wh, shift
        self.W, self.H = wh
        self.nrm, self.pos, self.map = gc.frame(kind, wh)
        n = self.W * self.H
        self._blocks = [ctx.malloc(n * 16 + 16), ctx.malloc(n * 16 + 16), ctx.malloc(8 * n + 8), ctx.malloc(n + 8)]
        self.d_nrm, self.d_pos = (b + 4 * shift for b in self._blocks[:2])
        self.d_planes, self.d_map = (b + shift for b in self._blocks[2:])
        ctx.h2d(self.d_nrm, self.nrm)
        ctx.h2d(self.d_pos, self.pos)
        ctx.h2d(self.d_map, np.ascontiguousarray(self.map))
        self.planes = None
        self.vis = _Guarded(ctx, 8 * n * 4, 4 * shift)
        self.scratch = _Guarded(ctx, 3 * 8 * n * 2, 2 * shift)
        self.rgb = _Guarded(ctx, n * 3, shift)

    def upload(self, planes):
        self.planes = planes
        self.ctx.h2d(self.d_planes, np.ascontiguousarray(planes))

    def launch(self, lst, p, with_map, stream=None, scratch=True):
        api.wide_filter_guided_soft_light_list_device(self.ctx, lst, p, self.d_pos, self.d_nrm, self.d_planes, self.W, self.H, self.vis.ptr,
                                                      d_scratch=self.scratch.ptr if scratch else None,
                                                      d_lights_map=self.d_map if with_map else None, stream=stream)

    def run(self, lst, p, with_map, stream=None, scratch=True):
        """One call into the freshly preset visibility and scratch; returns planes 0 .. count - 1 and checks that nothing else was
        written: the planes of visibility from the count up, the scratch behind its 3 * count planes (all of it for passes <= 1), and
        the guard bytes of both."""
        self.vis.reset()
        self.scratch.reset()
        self.launch(lst, p, with_map, stream, scratch)
        self.ctx.synchronize(stream)
        vis = self.vis.read((8, self.H, self.W), f32)
        assert (vis[lst.count:].view(np.uint32) == 0xABABABAB).all(), "a plane of visibility from the count up was written"
        words = self.scratch.read((3 * 8 * self.W * self.H,), np.uint16)
        used = 3 * lst.count * self.W * self.H if p.passes >= 2 else 0
        assert (words[used:] == 0xABAB).all(), "the scratch was written behind its 3 * count planes"
        return vis[:lst.count]

    def twin(self, lst, p, with_map, planes=None, key=None):
        if key is not None:
            key = (self.kind, self.wh, with_map, p.passes, p.guide_k4) + key
            if key in _TWINS:
                return _TWINS[key]
        out = api.wide_filter_guided_soft_light_list(lst, p, self.pos, self.nrm, self.planes if planes is None else planes,
                                                     self.map if with_map else None)
        if key is not None:
            _TWINS[key] = out
        return out

    def free(self):
        for b in self._blocks:
            self.ctx.free(b)
        self.vis.free()
        self.scratch.free()
        self.rgb.free()


@pytest.fixture(scope="module", params=[(wh, shift) for wh in gc.FRAMES for shift in (0, 1)], ids=lambda p: f"{p[0][0]}x{p[0][1]}+{p[1]}")
def frames(ctx, request):
    wh, shift = request.param
    group = [_Frame(ctx, kind, wh, shift) for kind in gc.kinds(wh)]
    yield group
    for f in group:
        f.free()


def test_device_equals_the_host_twin(ctx, frames, other_stream):
    """passes 0 .. 5 and guide_k4 0, 12, 255 on the awkward, geometric and flat frames; lists of 1, 4 and 8 lights, with and without
    the map; one run per frame on a second stream; the passes <= 1 runs of one list without scratch."""
    for f in frames:
        for i, (count, rotation, with_map) in enumerate(RUNS):
            lst = gc.the_list(count, rotation)
            f.upload(gc.counts(f.wh, lst))
            for passes in gc.PASSES:
                for k4 in K4:
                    p = gc.params(passes, k4, f.kind)
                    stream = other_stream if i == 0 and passes == 3 and k4 == 12 else None
                    got = f.run(lst, p, with_map, stream, scratch=not (i == 1 and passes <= 1))
                    gc.same_bits(got, f.twin(lst, p, with_map, key=(count, rotation)),
                                 (f.kind, f.wh, f.shift, count, rotation, with_map, passes, k4))


def test_the_first_pass_leaves_the_threshold_in_the_third_set(ctx):
    """After a passes >= 2 call the third set of count planes of the scratch holds T(p, l) of the numpy rule at every active pixel."""
    f = _Frame(ctx, "flat", (72, 40), 1)
    try:
        lst = gc.the_list(8, 1)
        planes = gc.counts(f.wh, lst)
        f.upload(planes)
        f.run(lst, gc.params(2, 12), True)
        n = f.W * f.H
        words = f.scratch.read((3 * 8 * n,), np.uint16)
        got = words[2 * 8 * n:3 * 8 * n].reshape(8, f.H, f.W).astype(np.int64)
        T, active = gc.thresholds(lst, 12, f.nrm, planes, f.map)
        assert (got[active] == T[active]).all()
        assert (T[active] == 0).any() and ((T[active] > 0) & (T[active] < 65535)).any() and (T[active] == 65535).any()
    finally:
        f.free()


def test_downstream_passes_equal_their_twins(ctx, frames):
    """The device visibility combine, and accumulate_visibility_list_device with max_length 1, over a guided plane equal their host
    twins over the twin's plane."""
    k = sp.constants("unit")
    f = frames[-1]
    n = f.W * f.H
    soft = gc.the_list(8, 1)
    hard = soft.hard_list()
    f.upload(gc.counts(f.wh, soft))
    out, lengths = _Guarded(ctx, 8 * n * 4, 4 * f.shift), _Guarded(ctx, 8 * n, f.shift)
    try:
        for passes in (0, 3, 5):
            p = gc.params(passes, 12, f.kind)
            want = f.twin(soft, p, True, key=(8, 1))
            f.vis.reset()
            f.launch(soft, p, True)
            f.rgb.reset()
            api.combine_visibility_list_device(ctx, k, hard, f.d_pos, f.d_nrm, f.vis.ptr, f.W, f.H, f.rgb.ptr, d_lights_map=f.d_map)
            tp = api.TemporalParams.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, -1), 1.0, 1.0, max_length=1)
            out.reset()
            lengths.reset()
            api.accumulate_visibility_list_device(ctx, hard, tp, f.d_pos, f.d_nrm, f.vis.ptr, f.W, f.H, out.ptr, lengths.ptr, d_lights_map=f.d_map)
            ctx.synchronize()
            assert (f.rgb.read((f.H, f.W, 3)) == api.combine_visibility_list(k, hard, f.pos, f.nrm, want, f.map)).all(), (f.wh, passes)
            want_vis, want_len = api.accumulate_visibility_list(hard, tp, f.pos, f.nrm, want, None, f.map)
            gc.same_bits(out.read((8, f.H, f.W), f32)[:8], want_vis, ("accumulate", f.wh, passes))
            assert (lengths.read((8, f.H, f.W)) == want_len).all()
    finally:
        out.free()
        lengths.free()


def test_refusals_launch_nothing(ctx):
    """Every refusal of include/rts_scene.h: RTS_ERR_INVALID_ARG, and not a byte of visibility or scratch."""
    lib = api._lib
    f = _Frame(ctx, "geometric", (16, 16), 0)
    h, v = ctx.handle, C.c_void_p
    ref = lambda s: C.byref(s) if s is not None else None
    good = gc.params(3, 12)
    _, soft_bad = lc.bad_lists()
    soft = gc.the_list(4, 1)
    f.upload(gc.counts(f.wh, soft))
    one_set = 4 * 16 * 16 * 2                                            # bytes of one set of four planes

    def call(lst, p, ctx_=h, pos=f.d_pos, nrm=f.d_nrm, plane=True, W=16, H=16, out=f.vis.ptr, scratch=f.scratch.ptr):
        return lib.rtsh_wide_filter_guided_soft_light_list_device(ctx_, ref(lst), ref(p), v(pos), v(nrm), v(f.d_map), v(f.d_planes if plane else 0),
                                                                  W, H, v(out), v(scratch), None)

    def bad_params():
        out = [None]
        for field, value in (("passes", 6), ("passes", 0xFFFFFFFF), ("normal_cos_min", np.nan), ("normal_cos_min", np.inf),
                             ("plane_eps", -np.inf), ("plane_eps", np.nan), ("guide_k4", 256), ("guide_k4", 0xFFFFFFFF)):
            p = gc.params(3, 12)
            setattr(p, field, value)
            out.append(p)
        return out

    try:
        for b in soft_bad:
            assert call(b, good) == INVALID
        for p in bad_params():
            assert call(soft, p) == INVALID
        assert call(soft, good, ctx_=None) == INVALID
        assert call(soft, good, pos=0) == INVALID
        assert call(soft, good, nrm=0) == INVALID
        assert call(soft, good, plane=False) == INVALID
        assert call(soft, good, out=0) == INVALID
        assert call(soft, good, W=0) == INVALID
        assert call(soft, good, H=0) == INVALID
        assert call(soft, good, W=0x7FFFFFF1, H=1) == INVALID
        assert call(soft, good, W=1, H=16 * 65535 + 1) == INVALID                     # the grid's y extent
        assert call(soft, gc.params(2, 12), scratch=0) == INVALID                     # passes >= 2 need the scratch
        for i in range(3):
            assert call(soft, good, out=f.scratch.ptr + i * one_set) == INVALID       # visibility on one of the three sets
        ctx.synchronize()
        assert f.vis.untouched() and f.scratch.untouched()
    finally:
        f.free()


@pytest.mark.parametrize("passes", [0, 1, 3, 5])
def test_graph_capture_adds_one_kernel_node_per_pass(ctx, other_stream, passes):
    """Captured, the device form is max(1, passes) kernel nodes -- list and parameters by value, so the host struct may change before
    the graph runs -- and a replay filters the planes as they are THEN: overwritten counts give the changed frame's floats."""
    f = _Frame(ctx, "flat", (72, 40), 1)
    try:
        lst = gc.the_list(8, 1)
        planes = gc.counts(f.wh, lst)
        f.upload(planes)
        p = gc.params(passes, 12)
        want = f.twin(lst, p, True)
        f.vis.reset()
        g = hipgraph.capture(other_stream, lambda: f.launch(lst, p, True, other_stream))
        try:
            assert g.node_types() == [hipgraph.KERNEL] * max(1, passes), (passes, g.node_types())
            assert f.vis.untouched(), "the capture itself ran a kernel"
            p.passes, p.plane_eps, p.guide_k4 = (passes + 1) % 6, 0.0, 200      # by value: the graph holds its own copy
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            gc.same_bits(f.vis.read((8, f.H, f.W), f32), want, (passes, "first replay"))
            changed = np.ascontiguousarray(planes[:, ::-1, ::-1] // 2)
            f.upload(changed)
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            want2 = f.twin(lst, gc.params(passes, 12), True, planes=changed)
            assert (want2 != want).any()
            gc.same_bits(f.vis.read((8, f.H, f.W), f32), want2, (passes, "replay over changed planes"))
        finally:
            g.close()
    finally:
        f.free()
