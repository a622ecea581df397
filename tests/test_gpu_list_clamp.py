"""GPU: the clamped temporal accumulation (rtsh_accumulate_visibility_list_clamped_device; accumulateListClampedKernel of
raytracedshadows_amd/csrc/rts_temporal.inc) on the cases of tests/list_clamp_cases.py: the device form equals the host twin bit for bit
(the twin equals the numpy rule in tests/test_list_clamp_host.py).  The frames are list_temporal_cases.FRAMES: 1 x 1, 1 x 5 and 5 x 1
(a block with nearly every lane outside the frame: all of them must still reach the kernel's barriers), 7 x 9 (windows larger than
the frame), 16 x 16, 17 x 15 and 33 x 18 (partial blocks both ways), 3 x 333 and 40 x 40 (windows crossing block edges).  Every case
runs once with all pointers as allocated and once with the byte planes one byte, the float planes one float, into a larger allocation.
The outputs carry 256 spare bytes preset to 0xAB (and the bytes in front of a shifted one), which must come back unchanged, as must
the planes from the count up.  No BVH is installed: the pass needs none."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import list_clamp_cases as cc
import list_combine_cases as lc
import list_temporal_cases as tc
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID = 1
f32 = np.float32
FRAMES = tc.FRAMES


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


class _Pair:
    """A case on the device; `shift` 1 puts the byte planes and the map one byte, the float planes one float, into their blocks.
    Two guarded output sets (visibility, lengths) for the ping-pong."""

    FLOATS = ("nrm", "pos", "prev_nrm", "prev_pos", "vis", "prev_vis")
    BYTES = ("map", "prev_len")

    def __init__(self, ctx, kind, wh, shift):
        self.ctx, self.kind, self.wh, self.shift = ctx, kind, wh, shift
        self.W, self.H = wh
        self.case = cc.case(kind, wh)
        self._blocks, self.d = [], {}
        for name in self.FLOATS + self.BYTES:
            a = np.ascontiguousarray(self.case[name])
            block = ctx.malloc(a.nbytes + 16)
            self._blocks.append(block)
            self.d[name] = block + (4 if name in self.FLOATS else 1) * shift
            ctx.h2d(self.d[name], a)
        n = self.W * self.H
        self.out = [(_Guarded(ctx, 8 * n * 4, 4 * shift), _Guarded(ctx, 8 * n, shift)) for _ in range(2)]

    def prev(self):
        return (self.d["prev_pos"], self.d["prev_nrm"], self.d["prev_vis"], self.d["prev_len"])

    def host_prev(self):
        c = self.case
        return (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"])

    def launch(self, lst, p, clamp, with_map=True, first=False, stream=None, out=0, d_prev=None):
        api.accumulate_visibility_list_device(self.ctx, lst, p, self.d["pos"], self.d["nrm"], self.d["vis"], self.W, self.H,
                                              self.out[out][0].ptr, self.out[out][1].ptr, d_prev=None if first else (d_prev or self.prev()),
                                              d_lights_map=self.d["map"] if with_map else None, stream=stream, clamp=clamp)

    def read(self, count, out=0):
        """Planes 0 .. count - 1 of an output set; checks that nothing else was written."""
        vis = self.out[out][0].read((8, self.H, self.W), f32)
        lengths = self.out[out][1].read((8, self.H, self.W))
        assert (vis[count:].view(np.uint32) == 0xABABABAB).all() and (lengths[count:] == 0xAB).all(), "a plane from the count up was written"
        return vis[:count], lengths[:count]

    def run(self, lst, p, clamp, with_map=True, first=False, stream=None):
        for g in self.out[0]:
            g.reset()
        self.launch(lst, p, clamp, with_map, first, stream)
        self.ctx.synchronize(stream)
        return self.read(lst.count)

    def twin(self, lst, p, clamp, with_map=True, first=False, vis=None, prev=None):
        c = self.case
        return api.accumulate_visibility_list(lst, p, c["pos"], c["nrm"], c["vis"] if vis is None else vis,
                                              None if first else (prev or self.host_prev()), c["map"] if with_map else None, clamp=clamp)

    def free(self):
        for b in self._blocks:
            self.ctx.free(b)
        for pair in self.out:
            for g in pair:
                g.free()


@pytest.fixture(scope="module", params=[(wh, shift) for wh in FRAMES for shift in (0, 1)], ids=lambda p: f"{p[0][0]}x{p[0][1]}+{p[1]}")
def pairs(ctx, request):
    wh, shift = request.param
    out = [_Pair(ctx, kind, wh, shift) for kind in cc.KINDS]
    yield out
    for f in out:
        f.free()


#: (radius, margin, count, with_map, first, max_length, reset_lights): every radius, two margins, lists of 1, 3 and 8 lights, without a
#: map, the first frame and max_length 1 (no box is built), a reset light beside free ones (its box is skipped)
RUNS = [(0, 0.0, 1, True, False, 5, 0), (1, 0.125, 3, True, False, 5, 0), (2, 0.0, 8, True, False, 5, 0), (4, 0.125, 8, True, False, 255, 0),
        (4, 0.0, 3, False, False, 5, 0), (1, 0.0, 8, True, True, 5, 0), (2, 0.125, 8, True, False, 255, 0b101), (4, 0.0, 8, True, False, 1, 0)]


def test_device_equals_the_host_twin(ctx, pairs):
    for f in pairs:
        for radius, margin, count, with_map, first, max_length, reset in RUNS:
            lst, clamp = cc.the_list(count), cc.clamp_of(radius, margin)
            p = tc.with_params(f.case["params"], max_length, reset)
            cc.same_bits(f.run(lst, p, clamp, with_map, first), f.twin(lst, p, clamp, with_map, first),
                         (f.kind, f.wh, f.shift, radius, margin, count, with_map, first, max_length, reset))


def test_unclamped_call_after_a_clamped_one(ctx, pairs):
    """The existing device form, right after a clamped launch on the same buffers, still equals its twin."""
    lst = cc.the_list(8)
    for f in pairs[-2:]:
        p = f.case["params"]
        f.launch(lst, p, cc.clamp_of(4, 0.0))
        cc.same_bits(f.run(lst, p, None), f.twin(lst, p, None), (f.kind, f.wh, f.shift, "unclamped after clamped"))


def test_two_frames_ping_pong_on_a_second_stream(ctx, other_stream):
    """Frame 1 (first frame) into output set 0, frame 2 with set 0 as its history into set 1, queued on one stream without a
    synchronisation between them: the twin's chain."""
    for kind in ("bite-subpixel", "bite-turn"):
        f = _Pair(ctx, kind, (40, 40), 1)
        try:
            c, lst, clamp = f.case, cc.the_list(3), cc.clamp_of(2, 0.0)
            back = tc.with_params(tc.reverse_params(kind[5:], (40, 40)), 3, 0)
            p = tc.with_params(c["params"], 3, 0)
            # frame 1: the pair's previous frame seen as a first frame (its "current" visibility is the pair's history plane)
            api.accumulate_visibility_list_device(ctx, lst, back, f.d["prev_pos"], f.d["prev_nrm"], f.d["prev_vis"], 40, 40, f.out[0][0].ptr,
                                                  f.out[0][1].ptr, d_lights_map=f.d["map"], stream=other_stream, clamp=clamp)
            f.launch(lst, p, clamp, stream=other_stream, out=1, d_prev=(f.d["prev_pos"], f.d["prev_nrm"], f.out[0][0].ptr, f.out[0][1].ptr))
            ctx.synchronize(other_stream)
            one = api.accumulate_visibility_list(lst, back, c["prev_pos"], c["prev_nrm"], c["prev_vis"], None, c["map"], clamp=clamp)
            two = f.twin(lst, p, clamp, prev=(c["prev_pos"], c["prev_nrm"]) + one)
            cc.same_bits(f.read(3, 0), one, (kind, "frame 1"))
            cc.same_bits(f.read(3, 1), two, (kind, "frame 2"))
            assert two[1].max() == 2
        finally:
            f.free()


def test_refusals_write_nothing(ctx):
    """Every refusal of include/rts_scene.h: RTS_ERR_INVALID_ARG, nothing launched, not a byte of either output."""
    lib = api._lib
    f = _Pair(ctx, "turn", (16, 16), 0)
    v, h = C.c_void_p, ctx.handle
    ref = lambda s: C.byref(s) if s is not None else None
    good, lst, box = f.case["params"], cc.the_list(3), cc.clamp_of(2, 0.125)
    out, out_len = f.out[0][0].ptr, f.out[0][1].ptr

    def call(ctx_=h, lst_=lst, p=good, W=16, H=16, o=out, ol=out_len, k=box, **swap):
        d = dict(f.d, **swap)
        return lib.rtsh_accumulate_visibility_list_clamped_device(ctx_, ref(lst_), ref(p), v(d["pos"]), v(d["nrm"]), v(d["map"]), v(d["vis"]),
                                                                  v(d["prev_pos"]), v(d["prev_nrm"]), v(d["prev_vis"]), v(d["prev_len"]), W, H,
                                                                  v(o), v(ol), ref(k), None)

    try:
        assert call(ctx_=None) == INVALID and call(k=None) == INVALID
        for radius in (5, 0x80000000, 0xFFFFFFFF):
            assert call(k=cc.clamp_of(radius)) == INVALID, radius
        for margin in (-1.0, np.nan, np.inf, -np.inf):
            assert call(k=cc.clamp_of(1, margin)) == INVALID, margin
        assert call(o=f.d["vis"]) == INVALID                            # visibility_out == visibility
        for bad in lc.bad_lists()[0]:
            assert call(lst_=bad) == INVALID
        bad_params = [None]
        for field, value in (("max_length", 0), ("max_length", 256), ("normal_cos_min", np.nan), ("plane_eps", np.inf), ("prev_scale_x", 0.0),
                             ("prev_scale_y", -1.0), ("prev_scale_y", np.nan)):
            p = tc.with_params(good)
            setattr(p, field, value)
            bad_params.append(p)
        for field in ("eye_delta", "prev_right", "prev_up", "prev_fwd"):
            p = tc.with_params(good)
            getattr(p, field)[1] = np.inf
            bad_params.append(p)
        for p in bad_params:
            assert call(p=p) == INVALID
        for name in ("pos", "nrm", "vis"):
            assert call(**{name: 0}) == INVALID, name
        assert call(o=0) == INVALID and call(ol=0) == INVALID
        prevs = ("prev_pos", "prev_nrm", "prev_vis", "prev_len")
        for keep in range(1, 15):
            assert call(**{name: 0 for i, name in enumerate(prevs) if not (keep >> i) & 1}) == INVALID, keep
        for W, H in ((0, 16), (16, 0), (65537, 1), (1, 65537)):
            assert call(W=W, H=H) == INVALID, (W, H)
        assert call(prev_vis=out) == INVALID and call(prev_len=out_len) == INVALID
        ctx.synchronize()
        assert f.out[0][0].untouched() and f.out[0][1].untouched()
        vis = np.zeros((8, 16, 16), f32)
        ctx.d2h(vis, f.d["vis"])
        assert (vis.view(np.uint32) == np.ascontiguousarray(f.case["vis"]).view(np.uint32)).all()
    finally:
        f.free()


@pytest.mark.parametrize("first", [False, True], ids=["history", "first-frame"])
def test_graph_capture_adds_one_kernel_node(ctx, other_stream, first):
    """Captured, the device form is ONE kernel node -- list, params and clamp by value, so the host structs may change before the graph
    runs -- and a replay accumulates the planes as they are THEN."""
    f = _Pair(ctx, "bite-turn", (40, 40), 1)
    try:
        lst = cc.the_list(8)
        p = tc.with_params(f.case["params"])
        clamp = cc.clamp_of(2, 0.125)
        want = f.twin(lst, p, clamp, first=first)
        eager = f.run(lst, p, clamp, first=first, stream=other_stream)
        cc.same_bits(eager, want, ("eager", first))
        for g_ in f.out[0]:
            g_.reset()
        g = hipgraph.capture(other_stream, lambda: f.launch(lst, p, clamp, first=first, stream=other_stream))
        try:
            assert g.node_types() == [hipgraph.KERNEL], g.node_types()
            assert f.out[0][0].untouched() and f.out[0][1].untouched(), "the capture itself ran the kernel"
            p.max_length, p.reset_lights = 1, 0xFF                       # by value: the graph holds its own copies
            clamp.radius, clamp.margin = 0, 3.0e38
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            cc.same_bits(f.read(8), eager, ("first replay", first))
            changed = np.ascontiguousarray(f.case["prev_vis"][::-1] * f32(0.5))
            changed_vis = np.ascontiguousarray(f.case["vis"][::-1])
            ctx.h2d(f.d["prev_vis"], changed)
            ctx.h2d(f.d["vis"], changed_vis)
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            c = f.case
            want2 = f.twin(lst, tc.with_params(c["params"]), cc.clamp_of(2, 0.125), first=first, vis=changed_vis,
                           prev=(c["prev_pos"], c["prev_nrm"], changed, c["prev_len"]))
            assert (want2[0].view(np.uint32) != want[0].view(np.uint32)).any()
            cc.same_bits(f.read(8), want2, ("replay over changed planes", first))
        finally:
            g.close()
    finally:
        f.free()
