"""GPU: the count moments (rtsh_accumulate_moments_soft_light_list_device; accumulateMomentsKernel) and the guided wide filter with a
temporal threshold (rtsh_wide_filter_guided_temporal_soft_light_list_device; wideGuidedTemporalKernel as the first pass of the guided
filter's chain), both of raytracedshadows_amd/csrc/rts_moments.inc: the device forms equal the host twins bit for bit (the twins equal
the numpy rules in tests/test_list_moments_host.py).  Frames: (3, 2) and (17, 1), one partial block; (40, 40), (40, 72) and (72, 40),
several blocks with partial edges and every dense window clipped; the 1920 x 8 strip for the still camera.  Every frame runs once with
all pointers as allocated and once with every buffer one ELEMENT into a larger allocation -- the uint16 planes on 2 bytes, the uint32
planes on 4.  Every output and the scratch carry spare bytes preset to 0xAB that must come back unchanged.  No BVH is installed but in
the chain test."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import list_combine_cases as lc
import list_moments_cases as mc
import list_temporal_cases as tc
import list_wide_guided_cases as gc
from raytracedshadows_amd import api, scenes

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID = 1
f32 = np.float32
FRAMES = [(3, 2), (17, 1), (40, 40), (40, 72), (72, 40)]
DTYPES = (np.uint16, np.uint32, np.uint8)


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


class _Pool:
    """Device buffers that live as long as a test; `up` uploads an array `shift` ELEMENTS into its block."""

    def __init__(self, ctx, shift):
        self.ctx, self.shift, self.blocks = ctx, shift, []

    def up(self, array):
        a = np.ascontiguousarray(array)
        base = self.ctx.malloc(a.nbytes + 16)
        self.blocks.append(base)
        self.ctx.h2d(base + self.shift * a.itemsize, a)
        return base + self.shift * a.itemsize

    def out(self, n, dtype):
        g = _Guarded(self.ctx, 8 * n * np.dtype(dtype).itemsize, self.shift * np.dtype(dtype).itemsize)
        self.blocks.append(g)
        return g

    def free(self):
        for b in self.blocks:
            b.free() if isinstance(b, _Guarded) else self.ctx.free(b)


def _read_moments(outs, count, H, W):
    got = []
    for g, dtype in zip(outs, DTYPES):
        a = g.read((8, H, W), dtype)
        assert (a[count:].view(np.uint8) == 0xAB).all(), "a plane from the count up was written"
        got.append(a[:count])
    return tuple(got)


# ------------------------------------------------------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("wh", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_device_equals_the_host_twin(ctx, other_stream, wh, shift):
    """All four motions; max_length 1, 2, 5, 255 and resets 0, 0b101, 0xFF in turn (every value with every motion over the frames);
    lists of 8, 4 and 1 lights, with and without the map; the first frame; one run per frame on a second stream."""
    W, H = wh
    n = W * H
    pool = _Pool(ctx, shift)
    try:
        outs = [pool.out(n, t) for t in DTYPES]
        for i, motion in enumerate(mc.MOTIONS):
            count, rotation = [(8, 1), (4, 0), (1, 1), (8, 3)][i]
            lst = mc.the_list(count, rotation)
            c = mc.moments_case(motion, wh, lst)
            d = {k: pool.up(c[k]) for k in ("pos", "nrm", "map", "counts", "prev_pos", "prev_nrm", "prev_len")}
            d_prev = (d["prev_pos"], d["prev_nrm"], pool.up(c["prev"][2]), pool.up(c["prev"][3]), d["prev_len"])
            for j, max_length in enumerate(mc.MAX_LENGTHS):
                for k, reset in enumerate(mc.RESETS):
                    first = (i + j + k) % 5 == 4
                    with_map = (j + k) % 2 == 0
                    p = tc.with_params(c["params"], max_length, reset)
                    stream = other_stream if (j, k) == (2, 0) else None
                    for g in outs:
                        g.reset()
                    api.accumulate_moments_soft_light_list_device(ctx, lst, p, d["pos"], d["nrm"], d["counts"], W, H, *(g.ptr for g in outs),
                                                                  d_prev=None if first else d_prev, d_lights_map=d["map"] if with_map else None,
                                                                  stream=stream)
                    ctx.synchronize(stream)
                    want = api.accumulate_moments_soft_light_list(lst, p, c["pos"], c["nrm"], c["counts"], None if first else c["prev"],
                                                                  c["map"] if with_map else None)
                    mc.same_moments(_read_moments(outs, count, H, W), want, (motion, wh, shift, count, max_length, reset, first, with_map))
    finally:
        pool.free()


def test_moments_still_camera_on_the_strip(ctx):
    """Anchor 2 on the 1920 x 8 strip: four chained frames on the device, ping-ponging the history, equal the integer recurrence at
    every pixel that keeps its history, and the host twin everywhere."""
    W, H = 1920, 8
    n = W * H
    y, x = np.mgrid[0:H, 0:W]
    cam = tc._camera((0.3, 2.0, -4.0), (0.1, 0.2, 0.6), 0.6, W, H)
    # a plane that fills every column, as in list_temporal_cases' strip test: z from the previous camera's own rays
    sx = ((x + 0.5) / W * 2.0 - 1.0) * np.float64(cam["scale_x"])
    sy = (1.0 - (y + 0.5) / H * 2.0) * np.float64(cam["scale_y"])
    d = cam["fwd"].astype(np.float64) + sx[..., None] * cam["right"].astype(np.float64) + sy[..., None] * cam["up"].astype(np.float64)
    depth = 2.0 + 7.0 * (x / (W - 1.0))
    pos = np.zeros((H, W, 4), f32)
    pos[..., :3] = (depth[..., None] * d).astype(f32)
    pos[..., 3] = 1.0
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., :3] = (-cam["fwd"]).astype(f32)
    p = api.TemporalParams.make((0, 0, 0), cam["right"], cam["up"], cam["fwd"], cam["scale_x"], cam["scale_y"], 0.5, 1.0, 3, 0)
    lst = mc.the_list(4, 1)
    n_l = np.array(mc.samples_of(lst), np.int64).reshape(-1, 1, 1)
    pool = _Pool(ctx, 1)
    try:
        d_pos, d_nrm = pool.up(pos), pool.up(nrm)
        sets = [[pool.out(n, t) for t in DTYPES] for _ in range(2)]
        rs = np.random.RandomState(3)
        prev, want1, want2 = None, None, None
        for k in range(1, 5):
            counts = rs.randint(0, 50, (4, H, W)).astype(np.uint8)
            d_counts = pool.up(counts)
            cur, old = sets[k & 1], sets[(k - 1) & 1]
            for g in cur:
                g.reset()
            api.accumulate_moments_soft_light_list_device(ctx, lst, p, d_pos, d_nrm, d_counts, W, H, *(g.ptr for g in cur),
                                                          d_prev=None if k == 1 else (d_pos, d_nrm) + tuple(g.ptr for g in old))
            ctx.synchronize()
            got = _read_moments(cur, 4, H, W)
            host = api.accumulate_moments_soft_light_list(lst, p, pos, nrm, counts, prev)
            mc.same_moments(got, host, ("strip", k))
            cur1 = np.minimum(counts.astype(np.int64), n_l) * (65535 // n_l)
            m = min(k, 3)
            if k == 1:
                want1, want2 = cur1, cur1 * cur1
            else:
                want1 = (2 * ((m - 1) * want1 + cur1) + m) // (2 * m)
                want2 = (2 * ((m - 1) * want2 + cur1 * cur1) + m) // (2 * m)
            assert (got[2] == m).all(), ("a pixel of the strip lost its history", k)
            assert (got[0] == want1).all() and (got[1] == want2).all(), k
            prev = (pos, nrm) + host
    finally:
        pool.free()


def test_moments_refusals_launch_nothing_and_capture_adds_one_kernel_node(ctx, other_stream):
    lib = api._lib
    wh = (40, 40)
    W, H = wh
    lst = mc.the_list(4, 1)
    c = mc.moments_case("turn", wh, lst)
    pool = _Pool(ctx, 0)
    h, v = ctx.handle, C.c_void_p
    ref = lambda s: C.byref(s) if s is not None else None
    try:
        outs = [pool.out(W * H, t) for t in DTYPES]
        d = {k: pool.up(c[k]) for k in ("pos", "nrm", "map", "counts")}
        prev = [pool.up(a) for a in c["prev"]]
        good = c["params"]
        _, soft_bad = lc.bad_lists()

        def call(lst_=lst, p=good, ctx_=h, pos=d["pos"], nrm=d["nrm"], cnt=d["counts"], prev_=prev, W_=W, H_=H, out=None):
            out = out or [g.ptr for g in outs]
            return lib.rtsh_accumulate_moments_soft_light_list_device(ctx_, ref(lst_), ref(p), v(pos), v(nrm), v(d["map"]), v(cnt),
                                                                      *(v(a) for a in prev_), W_, H_, *(v(a) for a in out), None)

        for b in soft_bad:
            assert call(lst_=b) == INVALID
        for field, value in (("max_length", 0), ("max_length", 256), ("plane_eps", np.nan), ("prev_scale_x", 0.0)):
            p = tc.with_params(good)
            setattr(p, field, value)
            assert call(p=p) == INVALID
        assert call(p=None) == INVALID and call(ctx_=None) == INVALID
        assert call(pos=0) == INVALID and call(nrm=0) == INVALID and call(cnt=0) == INVALID
        for i in range(3):
            assert call(out=[0 if j == i else g.ptr for j, g in enumerate(outs)]) == INVALID
            assert call(prev_=prev[:2] + [outs[j].ptr if j == i else prev[2 + j] for j in range(3)]) == INVALID
        for i in range(5):
            assert call(prev_=[0 if j == i else a for j, a in enumerate(prev)]) == INVALID
        assert call(W_=0) == INVALID and call(H_=0) == INVALID and call(W_=65537, H_=1) == INVALID
        ctx.synchronize()
        assert all(g.untouched() for g in outs)
        # under capture: one kernel node, list and params by value; two replays, the second over changed counts
        p = tc.with_params(good)
        launch = lambda: api.accumulate_moments_soft_light_list_device(ctx, lst, p, d["pos"], d["nrm"], d["counts"], W, H, *(g.ptr for g in outs),
                                                                       d_prev=tuple(prev), d_lights_map=d["map"], stream=other_stream)
        g = hipgraph.capture(other_stream, launch)
        try:
            assert g.node_types() == [hipgraph.KERNEL], g.node_types()
            assert all(o.untouched() for o in outs), "the capture itself ran a kernel"
            p.max_length, p.reset_lights = 1, 0xFF                       # by value: the graph holds its own copy
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            want = api.accumulate_moments_soft_light_list(lst, good, c["pos"], c["nrm"], c["counts"], c["prev"], c["map"])
            mc.same_moments(_read_moments(outs, 4, H, W), want, "first replay")
            changed = np.ascontiguousarray(c["counts"][:, ::-1, ::-1] // 2)
            ctx.h2d(d["counts"], changed)
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            want2 = api.accumulate_moments_soft_light_list(lst, good, c["pos"], c["nrm"], changed, c["prev"], c["map"])
            assert (want2[0] != want[0]).any()
            mc.same_moments(_read_moments(outs, 4, H, W), want2, "replay over changed counts")
        finally:
            g.close()
    finally:
        pool.free()


# ------------------------------------------------------------------------------------------------------------------ stage 2
class _Filter:
    """A frame of list_wide_guided_cases on the device with this file's moments; `shift` puts every buffer one element in."""

    def __init__(self, ctx, kind, wh, shift):
        self.ctx, self.kind, self.wh, self.shift = ctx, kind, wh, shift
        self.W, self.H = wh
        self.nrm, self.pos, self.map = gc.frame(kind, wh)
        self.pool = _Pool(ctx, shift)
        n = self.W * self.H
        self.d_nrm, self.d_pos, self.d_map = self.pool.up(self.nrm), self.pool.up(self.pos), self.pool.up(self.map)
        self.vis = _Guarded(ctx, 8 * n * 4, 4 * shift)
        self.scratch = _Guarded(ctx, 3 * 8 * n * 2, 2 * shift)
        self.pool.blocks += [self.vis, self.scratch]

    def upload(self, planes, moments):
        self.planes, self.moments = planes, moments
        self.d_planes = self.pool.up(planes)
        self.d_moments = tuple(self.pool.up(a) for a in moments)

    def launch(self, lst, p, with_map, stream=None, scratch=True):
        api.wide_filter_guided_temporal_soft_light_list_device(self.ctx, lst, p, self.d_pos, self.d_nrm, self.d_planes, self.d_moments, self.W,
                                                               self.H, self.vis.ptr, d_scratch=self.scratch.ptr if scratch else None,
                                                               d_lights_map=self.d_map if with_map else None, stream=stream)

    def run(self, lst, p, with_map, stream=None, scratch=True):
        self.vis.reset()
        self.scratch.reset()
        self.launch(lst, p, with_map, stream, scratch)
        self.ctx.synchronize(stream)
        vis = self.vis.read((8, self.H, self.W), f32)
        assert (vis[lst.count:].view(np.uint32) == 0xABABABAB).all(), "a plane of visibility from the count up was written"
        words = self.scratch.read((3 * 8 * self.W * self.H,), np.uint16)
        used = 3 * lst.count * self.W * self.H if p.passes >= 2 else 0
        assert (words[used:] == 0xABAB).all(), "the scratch was written behind its 3 * count planes (all of it for passes <= 1)"
        return vis[:lst.count]

    def twin(self, lst, p, with_map):
        return api.wide_filter_guided_temporal_soft_light_list(lst, p, self.pos, self.nrm, self.planes, self.moments, self.map if with_map else None)

    def free(self):
        self.pool.free()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("wh", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_device_equals_the_host_twin(ctx, other_stream, wh, shift):
    """passes 0 .. 5, guide_k4 0, 12, 255, min_history 1, 2, 255 (in turn over passes and k4), on the awkward, geometric and flat
    frames; lists of 8, 4 and 1 lights, with and without the map; one run on a second stream; the passes <= 1 runs of one list
    without scratch."""
    for kind in gc.kinds(wh):
        f = _Filter(ctx, kind, wh, shift)
        try:
            for i, (count, rotation, with_map) in enumerate([(8, 1, True), (4, 0, False), (1, 1, True)]):
                lst = mc.the_list(count, rotation)
                f.upload(gc.counts(wh, lst), mc.history(wh, lst) + (mc.filter_lengths(wh),))
                for passes in gc.PASSES:
                    for j, k4 in enumerate((0, 12, 255)):
                        p = mc.params(passes, k4, mc.MIN_HISTORY[(passes + j + i) % 3], kind)
                        stream = other_stream if i == 0 and passes == 3 and k4 == 12 else None
                        got = f.run(lst, p, with_map, stream, scratch=not (i == 1 and passes <= 1))
                        gc.same_bits(got, f.twin(lst, p, with_map), (kind, wh, shift, count, passes, k4, p.min_history))
        finally:
            f.free()


def test_filter_leaves_the_temporal_threshold_in_the_third_set(ctx):
    """After a passes >= 2 call the third set of count planes of the scratch holds T(p, l) of the numpy rule at every active pixel."""
    f = _Filter(ctx, "flat", (72, 40), 1)
    try:
        lst = mc.the_list(8, 1)
        planes, moments = gc.counts(f.wh, lst), mc.history(f.wh, lst) + (mc.filter_lengths(f.wh),)
        f.upload(planes, moments)
        f.run(lst, mc.params(2, 12, 2), True)
        n = f.W * f.H
        words = f.scratch.read((3 * 8 * n,), np.uint16)
        got = words[2 * 8 * n:3 * 8 * n].reshape(8, f.H, f.W).astype(np.int64)
        T, active = mc.temporal_thresholds(lst, 12, 2, f.nrm, planes, moments, f.map)
        assert (got[active] == T[active]).all()
        assert (T[active] == 0).any() and ((T[active] > 0) & (T[active] < 65535)).any() and (T[active] == 65535).any()
    finally:
        f.free()


def test_filter_refusals_launch_nothing(ctx):
    lib = api._lib
    f = _Filter(ctx, "geometric", (16, 16), 0)
    h, v = ctx.handle, C.c_void_p
    ref = lambda s: C.byref(s) if s is not None else None
    good = mc.params(3, 12, 2)
    _, soft_bad = lc.bad_lists()
    soft = mc.the_list(4, 1)
    f.upload(gc.counts(f.wh, soft), mc.history(f.wh, soft) + (mc.filter_lengths(f.wh),))
    one_set = 4 * 16 * 16 * 2

    def call(lst=soft, p=good, ctx_=h, pos=f.d_pos, nrm=f.d_nrm, cnt=None, mom=None, W=16, H=16, out=f.vis.ptr, scratch=f.scratch.ptr):
        mom = f.d_moments if mom is None else mom
        return lib.rtsh_wide_filter_guided_temporal_soft_light_list_device(ctx_, ref(lst), ref(p), v(pos), v(nrm), v(f.d_map),
                                                                           v(f.d_planes if cnt is None else cnt), *(v(a) for a in mom), W, H,
                                                                           v(out), v(scratch), None)

    try:
        for b in soft_bad:
            assert call(lst=b) == INVALID
        for field, value in (("passes", 6), ("normal_cos_min", np.nan), ("plane_eps", np.inf), ("guide_k4", 256), ("min_history", 0),
                             ("min_history", 256)):
            p = mc.params(3, 12, 2)
            setattr(p, field, value)
            assert call(p=p) == INVALID
        assert call(p=None) == INVALID and call(ctx_=None) == INVALID
        assert call(pos=0) == INVALID and call(nrm=0) == INVALID and call(cnt=0) == INVALID and call(out=0) == INVALID
        for i in range(3):
            assert call(mom=[0 if j == i else a for j, a in enumerate(f.d_moments)]) == INVALID
            assert call(out=f.scratch.ptr + i * one_set) == INVALID      # visibility on one of the three sets
        assert call(W=0) == INVALID and call(H=0) == INVALID and call(W=0x7FFFFFF1, H=1) == INVALID and call(W=1, H=16 * 65535 + 1) == INVALID
        assert call(p=mc.params(2, 12, 2), scratch=0) == INVALID         # passes >= 2 need the scratch
        ctx.synchronize()
        assert f.vis.untouched() and f.scratch.untouched()
    finally:
        f.free()


@pytest.mark.parametrize("passes", [0, 1, 3, 5])
def test_filter_capture_adds_one_kernel_node_per_pass(ctx, other_stream, passes):
    """Captured, the device form is max(1, passes) kernel nodes, list and parameters by value; two replays, the second over changed
    moments."""
    f = _Filter(ctx, "flat", (72, 40), 1)
    try:
        lst = mc.the_list(8, 1)
        planes, moments = gc.counts(f.wh, lst), mc.history(f.wh, lst) + (mc.filter_lengths(f.wh),)
        f.upload(planes, moments)
        p = mc.params(passes, 12, 2)
        want = f.twin(lst, p, True)
        f.vis.reset()
        g = hipgraph.capture(other_stream, lambda: f.launch(lst, p, True, other_stream))
        try:
            assert g.node_types() == [hipgraph.KERNEL] * max(1, passes), (passes, g.node_types())
            assert f.vis.untouched(), "the capture itself ran a kernel"
            p.passes, p.guide_k4, p.min_history = (passes + 1) % 6, 200, 255   # by value: the graph holds its own copy
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            gc.same_bits(f.vis.read((8, f.H, f.W), f32), want, (passes, "first replay"))
            changed = np.ascontiguousarray(moments[2][:, ::-1, ::-1])
            ctx.h2d(f.d_moments[2], changed)
            f.moments = moments[:2] + (changed,)
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            want2 = f.twin(lst, mc.params(passes, 12, 2), True)
            if passes:
                assert (want2 != want).any()
            gc.same_bits(f.vis.read((8, f.H, f.W), f32), want2, (passes, "replay over changed lengths"))
        finally:
            g.close()
    finally:
        f.free()


def test_two_frame_chain_on_the_device_equals_the_chain_of_host_twins(ctx):
    """Two frames of a traced scene, the camera moving between them: trace counts, moments, temporal-guided filter, visibility
    accumulation, visibility combine -- all on the device, histories ping-ponged -- against the same chain of host twins, byte for
    byte."""
    W, H = 72, 40
    n = W * H
    sc = scenes.cornell()
    verts, idx = sc.flat()
    packed = api.BVHBuilder().build(verts, 8, idx, sc.triangle_count).m_packedNodes
    ctx.set_bvh(packed)
    eyes = [np.asarray(sc.eye, f32), np.asarray(sc.eye, f32) + f32(0.05) * np.array([1.0, 0.5, 0.0], f32)]
    entries = [(api.Light.POINT, [5.0, 9.5, 5.0], 4, 0, 1.0), (api.Light.POINT, [3.0, 8.0, 6.0], 16, 4, 0.3), (api.Light.POINT, [7.0, 7.0, 4.0], 1, 0, 0.0)]
    table = scenes.jitter_offsets(48, 1.0, 19)
    lst = api.SoftLightList.make(entries, table)
    hard = lst.hard_list()
    fp = api.WideGuideTemporalParams.make(3, 12, 2, 0.9, 0.05)
    pool = _Pool(ctx, 0)
    try:
        d_g = [(ctx.malloc(n * 16), ctx.malloc(n * 16)) for _ in range(2)]
        pool.blocks += [b for pair in d_g for b in pair]
        d_map, d_counts, d_vis, d_rgb, d_scratch = (ctx.malloc(s) for s in (n, 8 * n, 32 * n, 3 * n, 48 * n))
        pool.blocks += [d_map, d_counts, d_vis, d_rgb, d_scratch]
        d_mom = [[pool.out(n, t) for t in DTYPES] for _ in range(2)]
        d_acc = [(pool.out(n, f32), pool.out(n, np.uint8)) for _ in range(2)]
        h_prev = None
        for k in range(2):
            eye = eyes[k]
            k_ = api.RayTracingConstants.make(eye, (0.0, -1.0, 0.0), W, H)
            tp = api.TemporalParams.from_cameras((eye, sc.target, sc.fovy), (eyes[k - 1], sc.target, sc.fovy), W, H, 0.9, 0.02, 8, 0)
            d_pos, d_nrm = d_g[k]
            api.primary_gbuffer_device(ctx, eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
            api.facing_lights_device(ctx, k_, hard, d_pos, d_nrm, W, H, d_map)
            ctx.trace_soft_light_list_device(k_, lst, d_pos, W, H, d_counts, d_lights_map=d_map)
            cur, old = d_mom[k], d_mom[k - 1]
            api.accumulate_moments_soft_light_list_device(ctx, lst, tp, d_pos, d_nrm, d_counts, W, H, *(g.ptr for g in cur),
                                                          d_prev=None if k == 0 else d_g[0] + tuple(g.ptr for g in old), d_lights_map=d_map)
            api.wide_filter_guided_temporal_soft_light_list_device(ctx, lst, fp, d_pos, d_nrm, d_counts, tuple(g.ptr for g in cur), W, H, d_vis,
                                                                   d_scratch=d_scratch, d_lights_map=d_map)
            api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_acc[k][0].ptr, d_acc[k][1].ptr,
                                                  d_prev=None if k == 0 else d_g[0] + (d_acc[0][0].ptr, d_acc[0][1].ptr), d_lights_map=d_map)
            api.combine_visibility_list_device(ctx, k_, hard, d_pos, d_nrm, d_acc[k][0].ptr, W, H, d_rgb, d_lights_map=d_map)
            ctx.synchronize()
            # the same chain of host twins
            pos, nrm, _ = api.primary_gbuffer(packed, eye, sc.target, sc.fovy, W, H)
            fmap = api.facing_lights(k_, hard, pos, nrm)
            counts = api.soft_light_list(packed, k_, lst, pos, W, H, lights_map=fmap)
            mom = api.accumulate_moments_soft_light_list(lst, tp, pos, nrm, counts, None if k == 0 else h_prev[:2] + h_prev[2], fmap)
            vis = api.wide_filter_guided_temporal_soft_light_list(lst, fp, pos, nrm, counts, mom, fmap)
            acc = api.accumulate_visibility_list(hard, tp, pos, nrm, vis, None if k == 0 else h_prev[:2] + h_prev[3], fmap)
            rgb = api.combine_visibility_list(k_, hard, pos, nrm, acc[0], fmap)
            mc.same_moments(_read_moments(cur, 3, H, W), mom, ("chain, moments", k))
            gc.same_bits(d_acc[k][0].read((8, H, W), f32)[:3], acc[0], ("chain, accumulated visibility", k))
            assert (d_acc[k][1].read((8, H, W))[:3] == acc[1]).all()
            got_rgb = np.zeros((H, W, 3), np.uint8)
            ctx.d2h(got_rgb, d_rgb)
            assert (got_rgb == rgb).all(), ("chain, image", k)
            if k == 1:
                assert (mom[2] > 1).sum() > 1000, "the second frame found no history"
            h_prev = (pos, nrm, mom, acc)
    finally:
        pool.free()
