"""GPU: the filter of a light list's planes (rtsh_filter_light_list_device, rtsh_filter_soft_light_list_device; filterListKernel of
raytracedshadows_amd/csrc/rts_filter.inc, included by rts_primary.hip) and the visibility combine (rtsh_combine_visibility_list_device) on the frames of
tests/list_filter_cases.py: the device forms equal the host twins bit for bit (the twins equal the numpy rules in
tests/test_list_filter_host.py).  Every frame runs once with all pointers as allocated and once with the byte planes and the map one
byte, and the float planes one float, into a larger allocation: the passes ask for no alignment beyond the element type's.  The
outputs carry 256 spare bytes preset to 0xAB (and the bytes in front of a shifted one) that must come back unchanged.  No BVH is
installed: the passes need none."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import list_combine_cases as lc
import list_filter_cases as fc
import scene_pass_cases as sp
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID = 1
f32 = np.float32
#: the frames of the cases, and 40 x 40: several blocks in both directions, halos crossing block edges, a partial last block
FRAMES = fc.FRAMES + [(40, 40)]


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
    """A frame of the cases on the device; `shift` 1 puts the byte planes and the map one byte, the float planes one float, into
    their blocks."""

    def __init__(self, ctx, kind, wh, shift):
        self.ctx, self.kind, self.wh, self.shift = ctx, kind, wh, shift
        self.W, self.H = wh
        self.nrm, self.pos, self.planes, self.mask, self.map, self.dist = fc.frame(kind, wh)
        n = self.W * self.H
        self._blocks = [ctx.malloc(n * 16 + 16), ctx.malloc(n * 16 + 16), ctx.malloc(8 * n * 4 + 16), ctx.malloc(8 * n + 8), ctx.malloc(n + 8),
                        ctx.malloc(n + 8)]
        self.d_nrm, self.d_pos, self.d_dist = (b + 4 * shift for b in self._blocks[:3])
        self.d_planes, self.d_mask, self.d_map = (b + shift for b in self._blocks[3:])
        ctx.h2d(self.d_nrm, self.nrm)
        ctx.h2d(self.d_pos, self.pos)
        ctx.h2d(self.d_dist, self.dist)
        self.upload(self.planes, self.mask, self.map)
        self.vis = _Guarded(ctx, 8 * n * 4, 4 * shift)
        self.rgb = _Guarded(ctx, n * 3, shift)

    def upload(self, planes=None, mask=None, lights_map=None):
        for ptr, a in ((self.d_planes, planes), (self.d_mask, mask), (self.d_map, lights_map)):
            if a is not None:
                self.ctx.h2d(ptr, np.ascontiguousarray(a))

    def launch(self, form, lst, p, with_map, with_dist, stream=None):
        if form == "hard":
            api.filter_light_list_device(self.ctx, lst, p, self.d_pos, self.d_nrm, self.d_mask, self.W, self.H, self.vis.ptr,
                                         d_lights_map=self.d_map if with_map else None, stream=stream)
        else:
            api.filter_soft_light_list_device(self.ctx, lst, p, self.d_pos, self.d_nrm, self.d_planes, self.W, self.H, self.vis.ptr,
                                              d_lights_map=self.d_map if with_map else None, d_distances=self.d_dist if with_dist else None,
                                              stream=stream)

    def run(self, form, lst, p, with_map, with_dist, stream=None):
        """One launch into the freshly preset visibility; returns planes 0 .. count - 1 and checks that nothing else was written."""
        self.vis.reset()
        self.launch(form, lst, p, with_map, with_dist, stream)
        self.ctx.synchronize(stream)
        vis = self.vis.read((8, self.H, self.W), f32)
        assert (vis[lst.count:].view(np.uint32) == 0xABABABAB).all(), "a plane from the count up was written"
        return vis[:lst.count]

    def twin(self, form, lst, p, with_map, with_dist, planes=None):
        m, d = (self.map if with_map else None), (self.dist if with_dist else None)
        if form == "hard":
            return api.filter_light_list(lst, p, self.pos, self.nrm, self.mask, m)
        return api.filter_soft_light_list(lst, p, self.pos, self.nrm, self.planes if planes is None else planes, m, d)

    def free(self):
        for b in self._blocks:
            self.ctx.free(b)
        self.vis.free()
        self.rgb.free()


@pytest.fixture(scope="module", params=[(wh, shift) for wh in FRAMES for shift in (0, 1)], ids=lambda p: f"{p[0][0]}x{p[0][1]}+{p[1]}")
def frames(ctx, request):
    wh, shift = request.param
    pair = [_Frame(ctx, kind, wh, shift) for kind in ("awkward", "geometric")]
    yield pair
    for f in pair:
        f.free()


def test_device_equals_the_host_twin(ctx, frames, other_stream):
    """Every run of the cases at R = 0, 1, 2 and 8 on the awkward and the geometric frame -- the geometric one uniform per light over
    some blocks' windows and not over their neighbours', so that both the shortcut and the walk run; one run per frame on a second
    stream."""
    for f in frames:
        for radius in fc.RADII:
            p = fc.params(radius, f.kind)
            for i, (form, name, with_map, with_dist) in enumerate(fc.runs(radius)):
                lst = fc.the_list(form, name)
                want = f.twin(form, lst, p, with_map, with_dist)
                stream = other_stream if i == 0 and radius == 2 else None
                fc.same_bits(f.run(form, lst, p, with_map, with_dist, stream), want,
                             (f.kind, f.wh, f.shift, radius, form, name, with_map, with_dist, stream is not None))


def test_every_tile_geometry(ctx, frames):
    """The three tile layouts of the launcher: the padded pitch (eight lights, R = 8, no distances), the bare pitch (eight lights with
    distances at R = 5: the padded tile would pass 64 KiB) and the block of 16 x 8 pixels (eight lights with distances at R = 8)."""
    lst = fc.the_list("soft", "8")
    for f in frames:
        for radius, with_dist in ((8, False), (5, True), (8, True)):
            p = fc.params(radius, f.kind)
            fc.same_bits(f.run("soft", lst, p, True, with_dist), f.twin("soft", lst, p, True, with_dist), (f.kind, f.wh, f.shift, radius, with_dist))


def test_visibility_combine_device(ctx, frames):
    """The visibility combine on the device equals its host twin byte for byte on wild visibility (NaN, Inf, negative, huge), and over
    the device's own R = 0 filter it gives the list combine's bytes (both anchors: soft and hard)."""
    k = sp.constants("unit")
    f = frames[0]
    n = f.W * f.H
    wild = fc.wild_visibility(f.wh)
    d_wild = ctx.malloc(8 * n * 4 + 16)
    try:
        ctx.h2d(d_wild + 4 * f.shift, wild)
        for name in ("3", "8"):
            soft, hard = fc.the_list("soft", name), fc.the_list("hard", name)
            for with_map in (False, True):
                m = f.map if with_map else None
                for colours, colors in lc.colour_sets(hard.count).items():
                    def combine(d_vis):
                        f.rgb.reset()
                        api.combine_visibility_list_device(ctx, k, hard, f.d_pos, f.d_nrm, d_vis, f.W, f.H, f.rgb.ptr,
                                                           d_lights_map=f.d_map if with_map else None, colors=colors)
                        ctx.synchronize()
                        return f.rgb.read((f.H, f.W, 3))
                    what = (f.wh, f.shift, name, with_map, colours)
                    assert (combine(d_wild + 4 * f.shift) == api.combine_visibility_list(k, hard, f.pos, f.nrm, wild, m, colors)).all(), what
                    if colours == "wild":
                        continue
                    f.vis.reset()
                    f.launch("soft", soft, fc.params(0), with_map, False)
                    assert (combine(f.vis.ptr) == api.combine_soft_light_list(k, soft, f.pos, f.nrm, f.planes, m, colors)).all(), ("soft",) + what
                    f.vis.reset()
                    f.launch("hard", hard, fc.params(0), with_map, False)
                    assert (combine(f.vis.ptr) == api.combine_light_list(k, hard, f.pos, f.nrm, f.mask, m, colors)).all(), ("hard",) + what
    finally:
        ctx.free(d_wild)


def test_refusals_write_nothing(ctx):
    """Every refusal of include/rts_scene.h: RTS_ERR_INVALID_ARG, and not a byte of visibility or rgb."""
    lib = api._lib
    f = _Frame(ctx, "geometric", (16, 16), 0)
    k = sp.constants("unit")
    kk, h, v = C.byref(k), ctx.handle, C.c_void_p
    ref = lambda s: C.byref(s) if s is not None else None
    good = fc.params(2)
    hard_bad, soft_bad = lc.bad_lists()
    hard, soft = fc.the_list("hard", "3"), fc.the_list("soft", "3")

    def call(form, lst, p, ctx_=h, pos=f.d_pos, nrm=f.d_nrm, plane=True, dist=f.d_dist, W=16, H=16, out=f.vis.ptr):
        if form == "hard":
            return lib.rtsh_filter_light_list_device(ctx_, ref(lst), ref(p), v(pos), v(nrm), v(f.d_map), v(f.d_mask if plane else 0), W, H, v(out), None)
        return lib.rtsh_filter_soft_light_list_device(ctx_, ref(lst), ref(p), v(pos), v(nrm), v(f.d_map), v(f.d_planes if plane else 0), v(dist),
                                                      W, H, v(out), None)

    def bad_params():
        out = [None]
        for field, value in (("radius", 9), ("radius", 0xFFFFFFFF), ("normal_cos_min", np.nan), ("normal_cos_min", np.inf),
                             ("plane_eps", -np.inf), ("plane_eps", np.nan)):
            p = fc.params(2)
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
        for l, value in ((0, -1.0), (1, np.nan), (2, np.inf)):
            p = fc.params(2)
            p.spread[l] = value
            assert call("soft", soft, p) == INVALID, (l, value)
        fn = lib.rtsh_combine_visibility_list_device
        two, three = lc.the_list("hard", "2_directional"), lc.the_list("hard", "3")
        rest = (v(f.d_map), v(f.d_dist), 16, 16, v(f.rgb.ptr), None)
        for lst in hard_bad:
            assert fn(h, kk, ref(lst), None, v(f.d_pos), v(f.d_nrm), *rest) == INVALID
        assert fn(None, kk, ref(two), None, v(f.d_pos), v(f.d_nrm), *rest) == INVALID
        assert fn(h, None, ref(two), None, v(f.d_pos), v(f.d_nrm), *rest) == INVALID
        assert fn(h, kk, ref(two), None, v(f.d_pos), None, *rest) == INVALID
        assert fn(h, kk, ref(two), None, v(f.d_pos), v(f.d_nrm), v(f.d_map), None, 16, 16, v(f.rgb.ptr), None) == INVALID
        assert fn(h, kk, ref(two), None, v(f.d_pos), v(f.d_nrm), v(f.d_map), v(f.d_dist), 16, 16, None, None) == INVALID
        assert fn(h, kk, ref(three), None, None, v(f.d_nrm), *rest) == INVALID                          # a point light, no positions
        assert fn(h, kk, ref(two), None, v(f.d_pos), v(f.d_nrm), v(f.d_map), v(f.d_dist), 0, 16, v(f.rgb.ptr), None) == INVALID
        assert fn(h, kk, ref(two), None, v(f.d_pos), v(f.d_nrm), v(f.d_map), v(f.d_dist), 16, 0, v(f.rgb.ptr), None) == INVALID
        ctx.synchronize()
        assert f.vis.untouched() and f.rgb.untouched()
    finally:
        f.free()


@pytest.mark.parametrize("form,with_dist", [("soft", True), ("soft", False), ("hard", False)], ids=["soft+distances", "soft", "hard"])
def test_graph_capture_adds_one_kernel_node(ctx, other_stream, form, with_dist):
    """Captured, a device form is ONE kernel node -- list and parameters by value, so the host structs may change before the graph
    runs -- and a replay filters the planes as they are THEN: changed counts give the changed frame's floats."""
    f = _Frame(ctx, "geometric", (40, 40), 1)
    try:
        lst = fc.the_list(form, "8")
        p = fc.params(2)
        want = f.twin(form, lst, p, True, with_dist)
        f.vis.reset()
        g = hipgraph.capture(other_stream, lambda: f.launch(form, lst, p, True, with_dist, other_stream))
        try:
            assert g.node_types() == [hipgraph.KERNEL], (form, g.node_types())
            assert f.vis.untouched(), "the capture itself ran the kernel"
            p.radius, p.plane_eps = 7, 0.0                            # by value: the graph holds its own copy
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            fc.same_bits(f.vis.read((8, f.H, f.W), f32), want, (form, "first replay"))
            changed, changed_mask = (f.planes[::-1] // 2).copy(), f.mask ^ 0x5A
            f.upload(changed, changed_mask)
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            p = fc.params(2)
            if form == "hard":
                want2 = api.filter_light_list(lst, p, f.pos, f.nrm, changed_mask, f.map)
            else:
                want2 = f.twin(form, lst, p, True, with_dist, planes=changed)
            assert (want2 != want).any()
            fc.same_bits(f.vis.read((8, f.H, f.W), f32), want2, (form, "replay over changed planes"))
        finally:
            g.close()
    finally:
        f.free()
