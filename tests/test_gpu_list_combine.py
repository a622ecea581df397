"""GPU: the combine pass of a light list (rtsh_combine_light_list_device, rtsh_combine_soft_light_list_device; combineListKernel of
raytracedshadows_amd/csrc/rts_primary.hip) on the frames of tests/list_combine_cases.py: the device forms equal
the host twins equal the float32 numpy rule, byte for byte.  Every frame runs once with all pointers as allocated and once with rgb, the
planes, the mask and the light map one byte into a larger allocation: the pass asks for no alignment beyond a byte's, whatever the
launcher makes of aligned buffers.  Output buffers carry 256 spare bytes preset
to 0xAB (and the byte in front of a shifted one) that must come back unchanged.  No BVH is installed: the pass needs none."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import list_combine_cases as lc
import scene_pass_cases as sp
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID = 1
f32 = np.float32
#: the frames of the cases, and 4 x 257: a multiple of 4 pixels in more than one workgroup
FRAMES = lc.FRAMES + [(4, 257)]


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

    def read(self, shape):
        raw = np.zeros(self.shift + self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.base)
        assert (raw[:self.shift] == 0xAB).all() and (raw[self.shift + self.nbytes:] == 0xAB).all(), "bytes around the buffer were written"
        return raw[self.shift:self.shift + self.nbytes].reshape(shape)

    def untouched(self):
        raw = np.zeros(self.shift + self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.base)
        return bool((raw == 0xAB).all())

    def free(self):
        self.ctx.free(self.base)


class _Frame:
    """A frame of the cases on the device; `shift` 1 puts rgb, the planes, the mask and the light map one byte into their blocks."""

    def __init__(self, ctx, wh, shift):
        self.ctx, self.wh, self.shift = ctx, wh, shift
        self.W, self.H = wh
        self.nrm, self.pos, self.planes, self.mask, self.map = lc.frame(wh)
        n = self.W * self.H
        self._blocks = [ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(8 * n + 8), ctx.malloc(n + 8), ctx.malloc(n + 8)]
        self.d_nrm, self.d_pos = self._blocks[:2]
        self.d_planes, self.d_mask, self.d_map = (b + shift for b in self._blocks[2:])
        ctx.h2d(self.d_nrm, self.nrm)
        ctx.h2d(self.d_pos, self.pos)
        self.upload(self.planes, self.mask, self.map)
        self.rgb = _Guarded(ctx, n * 3, shift)

    def upload(self, planes=None, mask=None, lights_map=None, pos=None):
        for ptr, a in ((self.d_planes, planes), (self.d_mask, mask), (self.d_map, lights_map), (self.d_pos, pos)):
            if a is not None:
                self.ctx.h2d(ptr, np.ascontiguousarray(a))

    def run(self, form, k, lst, with_pos, with_map, colors, stream=None):
        """One launch into the freshly preset rgb; returns the bytes (and checks the spare ones)."""
        self.rgb.reset()
        fn = api.combine_light_list_device if form == "hard" else api.combine_soft_light_list_device
        fn(self.ctx, k, lst, self.d_pos if with_pos else None, self.d_nrm, self.d_mask if form == "hard" else self.d_planes, self.W, self.H,
           self.rgb.ptr, d_lights_map=self.d_map if with_map else None, colors=colors, stream=stream)
        self.ctx.synchronize(stream)
        return self.rgb.read((self.H, self.W, 3))

    def free(self):
        for b in self._blocks:
            self.ctx.free(b)
        self.rgb.free()


def _twin(form, k, lst, pos, nrm, planes, mask, lights_map, colors):
    if form == "hard":
        return api.combine_light_list(k, lst, pos, nrm, mask, lights_map, colors)
    return api.combine_soft_light_list(k, lst, pos, nrm, planes, lights_map, colors)


def _same(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.shape[0] == 0, (what, bad.shape[0], [(y, x, got[y, x].tolist(), want[y, x].tolist()) for y, x in bad[:6].tolist()])


@pytest.fixture(scope="module", params=[(wh, shift) for wh in FRAMES for shift in (0, 1)], ids=lambda p: f"{p[0][0]}x{p[0][1]}+{p[1]}")
def frame(ctx, request):
    f = _Frame(ctx, *request.param)
    yield f
    f.free()


def test_device_equals_the_host_twin_equals_the_rule(ctx, frame, other_stream):
    """Every run of the cases (lists of 1, 3 and 8 lights, both forms, with and without map and positions, white, tame and wild
    colours); the wild-colour runs once more on a non-default stream."""
    k = sp.constants("unit")
    for form, name, with_pos, with_map, colours in lc.runs():
        lst = lc.the_list(form, name)
        colors = lc.colour_sets(lst.count)[colours]
        p, m = (frame.pos if with_pos else None), (frame.map if with_map else None)
        want = lc.list_combine_rule(k, lst, p, frame.nrm, frame.mask if form == "hard" else frame.planes, m, colors)
        what = (frame.wh, frame.shift, form, name, with_pos, with_map, colours)
        _same(_twin(form, k, lst, p, frame.nrm, frame.planes, frame.mask, m, colors), want, ("twin",) + what)
        for stream in ((None, other_stream) if colours == "wild" else (None,)):
            _same(frame.run(form, k, lst, with_pos, with_map, colors, stream), want, ("device", stream is not None) + what)


def test_other_constants(ctx, frame):
    """cameraDirection zero and unnormalised: the ambient term's view vector."""
    for kind in ("zero", "long"):
        k = sp.constants(kind)
        for form in ("hard", "soft"):
            lst = lc.the_list(form, "3")
            colors = lc.colour_sets(3)["tame"]
            want = lc.list_combine_rule(k, lst, frame.pos, frame.nrm, frame.mask if form == "hard" else frame.planes, frame.map, colors)
            _same(frame.run(form, k, lst, True, True, colors), want, (frame.wh, frame.shift, kind, form))


def test_anchor_a_list_of_one_white_light_is_combine_device(ctx, frame):
    """One light, white or no colours, no map: the bytes of api.combine_device for that light over that plane."""
    k = sp.constants("unit")
    white = np.ones((1, 3), f32)
    n = frame.W * frame.H
    d_plane0, d_bit0, d_want = ctx.malloc(n), ctx.malloc(n), ctx.malloc(n * 3)
    try:
        ctx.h2d(d_plane0, np.ascontiguousarray(frame.planes[0]))
        ctx.h2d(d_bit0, np.ascontiguousarray(frame.mask & 1))
        for name in ("directional1", "point1", "directional16", "point16"):
            light = sp.lights()[name]
            with_pos = light.type == api.Light.POINT
            forms = [("soft", lc.one_soft(light), d_plane0)] + ([("hard", api.LightList.make([light]), d_bit0)] if light.nsamples == 1 else [])
            for form, lst, d_one in forms:
                api.combine_device(ctx, k, light, frame.d_pos, frame.d_nrm, d_one, frame.W, frame.H, d_want)
                ctx.synchronize()
                want = np.zeros((frame.H, frame.W, 3), np.uint8)
                ctx.d2h(want, d_want)
                for colors in (None, white):
                    _same(frame.run(form, k, lst, with_pos, False, colors), want, (frame.wh, frame.shift, name, form, colors is not None))
    finally:
        for p in (d_plane0, d_bit0, d_want):
            ctx.free(p)


def test_bytes_that_are_never_looked_at(ctx, frame):
    """Plane bytes whose map bit is clear and every plane from the count up poisoned to 0xFF; a background pixel's position NaN and
    its map, mask and plane bytes flipped: the same image."""
    k = sp.constants("unit")
    lst, hard = lc.the_list("soft", "3"), lc.the_list("hard", "3")
    colors = lc.colour_sets(3)["wild"]
    want = lc.list_combine_rule(k, lst, frame.pos, frame.nrm, frame.planes, frame.map, colors)
    want_hard = lc.list_combine_rule(k, hard, frame.pos, frame.nrm, frame.mask, frame.map, colors)
    poisoned = frame.planes.copy()
    for l in range(3):
        poisoned[l][((frame.map >> l) & 1) == 0] = 0xFF
    poisoned[3:] = 0xFF
    background = (frame.nrm[..., :3] == 0).all(axis=-1)
    pos2, map2, mask2 = frame.pos.copy(), frame.map.copy(), frame.mask | 0xF8
    pos2[background] = np.nan
    map2[background] ^= 0xFF
    poisoned[:, background] ^= 0xFF
    mask2[background] ^= 0xFF
    try:
        frame.upload(poisoned, mask2, map2, pos2)
        got = frame.run("soft", k, lst, True, True, colors)
        _same(got, want, (frame.wh, frame.shift, "soft"))
        assert (got[background] == 0).all()
        _same(frame.run("hard", k, hard, True, True, colors), want_hard, (frame.wh, frame.shift, "hard"))
    finally:
        frame.upload(frame.planes, frame.mask, frame.map, frame.pos)


def test_refusals_write_nothing(ctx):
    """Every refusal of include/rts_scene.h: RTS_ERR_INVALID_ARG, and not a byte of rgb."""
    lib = api._lib
    f = _Frame(ctx, (16, 16), 0)
    k = sp.constants("unit")
    kk, h, v = C.byref(k), ctx.handle, C.c_void_p
    ref = lambda s: C.byref(s) if s is not None else None
    hard_bad, soft_bad = lc.bad_lists()
    forms = {"hard": (lib.rtsh_combine_light_list_device, lc.the_list("hard", "2_directional"), lc.the_list("hard", "3"), f.d_mask, hard_bad),
             "soft": (lib.rtsh_combine_soft_light_list_device, lc.the_list("soft", "2_directional"), lc.the_list("soft", "3"), f.d_planes, soft_bad)}
    try:
        for form, (fn, two, three, d_plane, bad) in forms.items():
            rest = (v(f.d_map), v(d_plane), 16, 16, v(f.rgb.ptr), None)
            for lst in bad:
                assert fn(h, kk, ref(lst), None, v(f.d_pos), v(f.d_nrm), *rest) == INVALID, form
            assert fn(None, kk, ref(two), None, v(f.d_pos), v(f.d_nrm), *rest) == INVALID
            assert fn(h, None, ref(two), None, v(f.d_pos), v(f.d_nrm), *rest) == INVALID
            assert fn(h, kk, ref(two), None, v(f.d_pos), None, *rest) == INVALID
            assert fn(h, kk, ref(two), None, v(f.d_pos), v(f.d_nrm), v(f.d_map), None, 16, 16, v(f.rgb.ptr), None) == INVALID
            assert fn(h, kk, ref(two), None, v(f.d_pos), v(f.d_nrm), v(f.d_map), v(d_plane), 16, 16, None, None) == INVALID
            assert fn(h, kk, ref(three), None, None, v(f.d_nrm), *rest) == INVALID                      # a point light, no positions
            assert fn(h, kk, ref(two), None, v(f.d_pos), v(f.d_nrm), v(f.d_map), v(d_plane), 0, 16, v(f.rgb.ptr), None) == INVALID
            assert fn(h, kk, ref(two), None, v(f.d_pos), v(f.d_nrm), v(f.d_map), v(d_plane), 16, 0, v(f.rgb.ptr), None) == INVALID
        ctx.synchronize()
        assert f.rgb.untouched()
    finally:
        f.free()


@pytest.mark.parametrize("wh,shift", [((16, 16), 0), ((3, 333), 0), ((16, 16), 1)], ids=["16x16", "3x333", "shifted"])
def test_graph_capture_adds_one_kernel_node(ctx, other_stream, wh, shift):
    """Captured, each device form is ONE kernel node -- list, colours and constants by value, so the host arrays may be gone by the
    time the graph runs -- and a replay writes the host twin's bytes."""
    f = _Frame(ctx, wh, shift)
    k = sp.constants("unit")
    try:
        for form in ("hard", "soft"):
            lst = lc.the_list(form, "8")
            colors = lc.colour_sets(8)["tame"].copy()
            want = _twin(form, k, lst, f.pos, f.nrm, f.planes, f.mask, f.map, colors)
            fn = api.combine_light_list_device if form == "hard" else api.combine_soft_light_list_device
            f.rgb.reset()
            g = hipgraph.capture(other_stream, lambda: fn(ctx, k, lst, f.d_pos, f.d_nrm, f.d_mask if form == "hard" else f.d_planes, f.W, f.H,
                                                          f.rgb.ptr, d_lights_map=f.d_map, colors=colors, stream=other_stream))
            try:
                assert g.node_types() == [hipgraph.KERNEL], (form, g.node_types())
                assert f.rgb.untouched(), "the capture itself ran the kernel"
                colors[:] = 0                                         # by value: the graph holds its own copy
                g.launch(other_stream)
                ctx.synchronize(other_stream)
                _same(f.rgb.read((f.H, f.W, 3)), want, (wh, shift, form))
            finally:
                g.close()
    finally:
        f.free()
