"""GPU: the device forms under hipGraph stream capture (include/rts.h, "GRAPH CAPTURE").

Every captured graph is one stream's linear chain.  For each capture: every call returns RTS_OK, the capture ends valid, the graph
holds kernel nodes only (one per trace, plus the planner's four in follow mode), and every replay -- on a guard-filled output, two
of them on another camera's G-buffer, after the host's constants and light structs were overwritten -- equals the CPU oracle for
the positions then in the buffer and the light as it was at the capture."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import oracle
from raytracedshadows_amd import api, workloads
from test_gpu_active import GUARD, _Dev, _expect, _family, _maps, _stripe_rows

pytestmark = pytest.mark.gpu

W = H = 256
ROWS = (37, 171)                                     # a row range that cuts tiles at both ends
STRIPE = (32, 2, 1)                                  # band, n, stripe: a band every family and workgroup shape accepts


def _copy(struct):
    return type(struct).from_buffer_copy(struct) if struct is not None else None


def _scribble(*structs):
    """What a caller may do to its structs between the capture and a replay."""
    for s in structs:
        if s is not None:
            C.memset(C.byref(s), 0x7F, C.sizeof(s))


class _Scene:
    """The cornell box at 256 x 256 from three cameras (positions and normals on the host), lights, oracle masks per (light, camera)."""

    def __init__(self):
        self.wl = wl = workloads.prepare_config("cornell_256", cache=True)
        assert (wl.W, wl.H) == (W, H)
        sc = wl.scene
        self.k = wl.constants
        self.eyes = [sc.eye, (sc.eye + (sc.target - sc.eye) * np.float32(0.07)).astype(np.float32),
                     (sc.eye + np.array([0.11, -0.06, 0.02], np.float32) * np.float32(np.linalg.norm(sc.target - sc.eye))).astype(np.float32)]
        self.pos, self.nrm = [], []
        for eye in self.eyes:
            p, n, _ = api.primary_gbuffer(wl.packed, eye, sc.target, sc.fovy, W, H)
            self.pos.append(p)
            self.nrm.append(n)
        assert np.array_equal(self.pos[0].ravel(), np.asarray(wl.positions).ravel())
        assert not np.array_equal(self.pos[0], self.pos[1]) and not np.array_equal(self.pos[1], self.pos[2])
        self.lights = {"point": wl.light, "directional": None, "soft16": workloads.relight(wl, "point", 16).light}
        self.active = _maps(W, H)["random50"]
        self._want = {}

    def want(self, key, cam):
        """The oracle's mask under the constants of camera 0 (the captured ones) for the G-buffer of camera `cam`."""
        if (key, cam) not in self._want:
            m, _, _ = oracle.shadow_mask(self.wl.packed, self.k.as_array(), oracle.light_from_product(self.lights[key], self.k), self.pos[cam],
                                         W, H)
            assert 0 < np.count_nonzero(m) < m.size, (key, cam)
            self._want[(key, cam)] = m
        return self._want[(key, cam)]


@pytest.fixture(scope="module")
def scene():
    return _Scene()


@pytest.fixture()
def ctx(scene):
    with api.ShadowContext(0) as c:
        c.set_bvh(scene.wl.packed)
        assert c.get_option("wide_nodes") > 0
        yield c


def _stream(ctx, scene, dev, fresh):
    """A stream that has never run anything, or one that has traced a frame."""
    s = ctx.stream_create()
    if not fresh:
        ctx.trace_shadow_mask_device(scene.k, dev.d_pos, W, H, dev.d_mask, light=scene.lights["point"], stream=s)
        ctx.synchronize(s)
    return s


def _kernels_only(g, count, what):
    types = g.node_types()
    assert all(t == hipgraph.KERNEL for t in types), (what, types)
    assert len(types) == count, (what, types)


def _replay_masks(ctx, g, stream, dev, scene, want_of, cams=(0, 1, 2, 0), what=""):
    for n, cam in enumerate(cams):
        ctx.h2d(dev.d_pos, scene.pos[cam])
        dev.guard()
        g.launch(stream)
        got = dev.mask(stream)
        bad = int((got != want_of(cam)).sum())
        assert bad == 0, (what, "replay", n, "camera", cam, bad)


MASK_CASES = {
    # name: (kernel, light, form, with an active map)
    "plain_7": (7, "point", "whole", False), "plain_3": (3, "point", "whole", False), "plain_8": (8, "point", "whole", False),
    "plain_3_directional": (3, "directional", "whole", False),
    "rows_3": (3, "point", "rows", False), "rows_7": (7, "point", "rows", False),
    "stripe_3": (3, "point", "stripe", False), "stripe_8": (8, "point", "stripe", False),
    "soft16_3": (3, "soft16", "whole", False), "soft16_8": (8, "soft16", "whole", False), "soft16_7": (7, "soft16", "whole", False),
}
for _k in (7, 3, 8):                                 # the three active forms for each family
    for _form in ("whole", "rows", "stripe"):
        MASK_CASES[f"active_{_k}_{_form}"] = (_k, "point", _form, True)
MASK_CASES["active_8_soft16"] = (8, "soft16", "whole", True)


@pytest.mark.parametrize("fresh", [False, True], ids=["traced_before", "fresh_stream"])
@pytest.mark.parametrize("case", sorted(MASK_CASES))
def test_captured_trace_replays_exactly(ctx, scene, case, fresh):
    kernel, key, form, with_map = MASK_CASES[case]
    dev = _Dev(ctx, scene.pos[0], W, H)
    dev.set_map(scene.active)
    stream = _stream(ctx, scene, dev, fresh)
    k, light = _copy(scene.k), _copy(scene.lights[key])
    d_act = dev.d_act if with_map else None
    rows = None
    g = None
    try:
        ctx.set_option("kernel", kernel)
        if form == "whole":
            record = lambda: ctx.trace_shadow_mask_device(k, dev.d_pos, W, H, dev.d_mask, light=light, stream=stream, d_active=d_act)
        elif form == "rows":
            rows = (np.arange(H) >= ROWS[0]) & (np.arange(H) < ROWS[1])
            record = lambda: ctx.trace_shadow_mask_device(k, dev.d_pos, W, H, dev.d_mask, light=light, stream=stream, d_active=d_act,
                                                          row_begin=ROWS[0], row_end=ROWS[1])
        else:
            rows = _stripe_rows(H, *STRIPE)
            record = lambda: ctx.trace_shadow_mask_stripes_device(k, dev.d_pos, W, H, dev.d_mask, *STRIPE, light=light, stream=stream,
                                                                  d_active=d_act)
        launches = ctx.get_option("active_traces")
        g = hipgraph.capture(stream, record)                  # (an RTS status other than RTS_OK raises in the wrapper)
        assert ctx.get_option("active_traces") == launches + (1 if with_map else 0)
        name = ctx.last_kernel_name()
        if with_map:
            assert name == _family(ctx, kernel, W * H, key == "soft16"), (case, name)
        else:
            assert not name.startswith("shadowMaskActive") and not name.startswith("shadowMaskFollow"), (case, name)
        _kernels_only(g, 1, case)
        _scribble(k, light)
        active = scene.active if with_map else np.ones((H, W), np.uint8)
        _replay_masks(ctx, g, stream, dev, scene, lambda cam: _expect(scene.want(key, cam), active, rows), what=case)
    finally:
        if g:
            g.close()
        ctx.synchronize(stream)
        ctx.stream_destroy(stream)
        dev.close()


def _rays(seed, n=20000):
    rs = np.random.RandomState(seed)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = rs.random_sample((n, 3)) * 2.4 - 1.2
    d = rs.standard_normal((n, 3))
    r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 3] = rs.random_sample(n) * 3 + 0.01
    return r


@pytest.mark.parametrize("fresh", [False, True], ids=["traced_before", "fresh_stream"])
@pytest.mark.parametrize("kernel", [-1, 3, 8])
def test_captured_generic_rays(ctx, scene, kernel, fresh):
    sc = scene.wl.scene
    lo, ext = np.asarray(sc.bbox_min, np.float32), np.asarray(sc.bbox_max, np.float32) - np.asarray(sc.bbox_min, np.float32)
    sets = []
    for seed in (1, 2, 3):
        r = _rays(seed)
        r[:, 0:3] = lo + (r[:, 0:3] + 1.2) / 2.4 * ext
        r[:, 3] *= float(ext.max()) / 3
        want, _, _ = oracle.trace_rays(scene.wl.packed, r)
        assert 0 < np.count_nonzero(want) < want.size
        sets.append((r, want))
    n = sets[0][0].shape[0]
    dev = _Dev(ctx, scene.pos[0], W, H)
    d_rays, d_out = ctx.malloc(n * 32), ctx.malloc(n)
    stream = _stream(ctx, scene, dev, fresh)
    g = None
    try:
        ctx.set_option("kernel", kernel)
        g = hipgraph.capture(stream, lambda: ctx.trace_rays_device(d_rays, n, d_out, stream=stream))
        _kernels_only(g, 1, kernel)
        for i in (0, 1, 2, 0):
            ctx.h2d(d_rays, sets[i][0])
            ctx.h2d(d_out, np.full(n, GUARD, np.uint8))
            g.launch(stream)
            ctx.synchronize(stream)
            got = np.empty(n, np.uint8)
            ctx.d2h(got, d_out)
            assert int((got != sets[i][1]).sum()) == 0, (kernel, i)
    finally:
        if g:
            g.close()
        ctx.synchronize(stream)
        ctx.stream_destroy(stream)
        ctx.free(d_rays)
        ctx.free(d_out)
        dev.close()


class _Frame:
    """Device buffers of the scene-side passes: normals, active map, rgb beside _Dev's positions and mask."""

    def __init__(self, ctx, scene):
        self.ctx, self.dev = ctx, _Dev(ctx, scene.pos[0], W, H)
        self.d_nrm, self.d_rgb = ctx.malloc(W * H * 16), ctx.malloc(W * H * 3)
        ctx.h2d(self.d_nrm, scene.nrm[0])

    def read(self, d, shape, dtype, stream):
        out = np.empty(shape, dtype)
        self.ctx.synchronize(stream)
        self.ctx.d2h(out, d)
        return out

    def fill(self, d, nbytes):
        self.ctx.h2d(d, np.full(nbytes, GUARD, np.uint8))

    def close(self):
        self.ctx.free(self.d_nrm)
        self.ctx.free(self.d_rgb)
        self.dev.close()


@pytest.mark.parametrize("fresh", [False, True], ids=["traced_before", "fresh_stream"])
def test_captured_scene_passes(ctx, scene, fresh):
    """rtsh_primary_gbuffer_device, rtsh_facing_active_device, rtsh_combine_device: one graph each, against their host twins."""
    wl, sc = scene.wl, scene.wl.scene
    f = _Frame(ctx, scene)
    dev = f.dev
    stream = _stream(ctx, scene, dev, fresh)
    graphs = []
    try:
        for key in ("point", "directional"):
            k, light = _copy(scene.k), _copy(scene.lights[key])
            # G-buffer (the camera travels by value)
            g = hipgraph.capture(stream, lambda: api.primary_gbuffer_device(ctx, scene.eyes[1], sc.target, sc.fovy, W, H, dev.d_pos, f.d_nrm,
                                                                            stream=stream))
            graphs.append(g)
            _kernels_only(g, 1, "gbuffer")
            for _ in range(3):
                f.fill(dev.d_pos, W * H * 16)
                f.fill(f.d_nrm, W * H * 16)
                g.launch(stream)
                assert np.array_equal(f.read(dev.d_pos, (H, W, 4), np.float32, stream).view(np.uint32), scene.pos[1].view(np.uint32))
                assert np.array_equal(f.read(f.d_nrm, (H, W, 4), np.float32, stream).view(np.uint32), scene.nrm[1].view(np.uint32))
            # facing mark
            g = hipgraph.capture(stream, lambda: api.facing_active_device(ctx, k, light, dev.d_pos, f.d_nrm, W, H, dev.d_act, stream=stream))
            graphs.append(g)
            _kernels_only(g, 1, "facing")
            kc, lc = _copy(k), _copy(light)
            _scribble(k, light)
            marks = {}
            for cam in (0, 1, 2, 0):
                ctx.h2d(dev.d_pos, scene.pos[cam])
                ctx.h2d(f.d_nrm, scene.nrm[cam])
                f.fill(dev.d_act, W * H)
                g.launch(stream)
                marks[cam] = api.facing_active(kc, lc, scene.pos[cam], scene.nrm[cam])
                assert 0 < np.count_nonzero(marks[cam]) < marks[cam].size
                assert np.array_equal(f.read(dev.d_act, (H, W), np.uint8, stream), marks[cam]), (key, cam)
            # combine
            k, light = _copy(kc), _copy(lc)
            g = hipgraph.capture(stream, lambda: api.combine_device(ctx, k, light, dev.d_pos, f.d_nrm, dev.d_mask, W, H, f.d_rgb, stream=stream))
            graphs.append(g)
            _kernels_only(g, 1, "combine")
            _scribble(k, light)
            for cam in (0, 1, 2, 0):
                mask = _expect(scene.want(key, cam), marks[cam])
                ctx.h2d(dev.d_pos, scene.pos[cam])
                ctx.h2d(f.d_nrm, scene.nrm[cam])
                ctx.h2d(dev.d_mask, mask)
                f.fill(f.d_rgb, W * H * 3)
                g.launch(stream)
                want = api.combine(kc, lc, scene.pos[cam], scene.nrm[cam], mask)
                assert np.array_equal(f.read(f.d_rgb, (H, W, 3), np.uint8, stream), want), (key, cam)
    finally:
        for g in graphs:
            g.close()
        ctx.synchronize(stream)
        ctx.stream_destroy(stream)
        f.close()


def _follow_counters(ctx):
    return tuple(ctx.get_option(key) for key in ("follow_streams", "follow_traces", "follow_ordered"))


@pytest.mark.parametrize("kernel", [3, 8])
def test_follow_mode_under_capture(ctx, scene, kernel):
    dev = _Dev(ctx, scene.pos[0], W, H)
    s_fresh, s_used = ctx.stream_create(), ctx.stream_create()
    light = scene.lights["point"]
    want = lambda cam: scene.want("point", cam)
    bx, by = (W + 7) // 8, (H + 7) // 8
    graphs = []
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("follow", 1)
        # (a) a stream without state, captured: nothing is allocated, so the everyday launch, and no state appears
        before = _follow_counters(ctx)
        g = hipgraph.capture(s_fresh, lambda: ctx.trace_shadow_mask_device(scene.k, dev.d_pos, W, H, dev.d_mask, light=light, stream=s_fresh))
        graphs.append(g)
        assert ctx.last_kernel_name() == ("shadowMaskPacketKernel<1,wide>" if kernel == 8 else "shadowMaskPacketKernel<1>")
        assert _follow_counters(ctx) == before
        _kernels_only(g, 1, "follow, no state")
        _replay_masks(ctx, g, s_fresh, dev, scene, want, what="follow (a)")
        assert _follow_counters(ctx) == before
        # (b) two traces outside capture, the third captured: the follow kernel and the planner's four
        ctx.h2d(dev.d_pos, scene.pos[0])
        for _ in range(2):
            ctx.trace_shadow_mask_device(scene.k, dev.d_pos, W, H, dev.d_mask, light=light, stream=s_used)
        ctx.synchronize(s_used)
        streams, traces, ordered = _follow_counters(ctx)
        assert (streams, traces, ordered) == (before[0] + 1, before[1] + 2, before[2] + 1)
        k, lt = _copy(scene.k), _copy(light)
        g = hipgraph.capture(s_used, lambda: ctx.trace_shadow_mask_device(k, dev.d_pos, W, H, dev.d_mask, light=lt, stream=s_used))
        graphs.append(g)
        assert ctx.last_kernel_name() == ("shadowMaskFollowKernel<1,wide>" if kernel == 8 else "shadowMaskFollowKernel<1>")
        assert _follow_counters(ctx) == (streams, traces + 1, ordered + 1)
        assert ctx.get_option("follow_block") > 1
        _kernels_only(g, 5, "follow, with state")
        _scribble(k, lt)
        _replay_masks(ctx, g, s_used, dev, scene, want, cams=(0, 1, 2, 1), what="follow (b)")
        lives, order = ctx.read_follow(bx * by, stream=s_used)
        assert (lives > 0).all()
        ids = (order & 0xFFFF) + (order >> 16) * bx
        assert sorted(ids.tolist()) == list(range(bx * by))
        assert np.array_equal(ids, api.follow_order(lives, bx, by, 0, ctx.get_option("follow_square"), ctx.get_option("follow_block")))
    finally:
        for g in graphs:
            g.close()
        for s in (s_fresh, s_used):
            ctx.synchronize(s)
            ctx.stream_destroy(s)
        ctx.set_option("follow", 0)
        dev.close()


@pytest.mark.parametrize("kernel", [3, 8])
def test_split_table_under_capture(ctx, scene, kernel):
    """(b) is the defect this file found: the table's per-stream state used to be allocated and cleared at a stream's first trace
    even when that trace was being captured."""
    dev = _Dev(ctx, scene.pos[0], W, H)
    s1, s2 = ctx.stream_create(), ctx.stream_create()
    light = scene.lights["point"]
    want = lambda cam: scene.want("point", cam)
    graphs = []
    try:
        ctx.set_option("kernel", kernel)
        tiles, records = ctx.plan_splits(scene.k, dev.d_pos, W, H, dev.d_mask, light=light, min_life_us=4.0, piece_us=2.0, max_pieces=8,
                                         front_share=1.0 / 3.0)
        table = (ctx.get_option("split_tiles"), ctx.get_option("split_pieces"), ctx.get_option("front_tiles"))
        assert records > 0 and table[1] > 0, (tiles, records, table)
        # (a) s1 has traced with the table before the capture
        dev.guard()
        ctx.trace_shadow_mask_device(scene.k, dev.d_pos, W, H, dev.d_mask, light=light, stream=s1)
        assert int((dev.mask(s1) != want(0)).sum()) == 0
        k, lt = _copy(scene.k), _copy(light)
        g = hipgraph.capture(s1, lambda: ctx.trace_shadow_mask_device(k, dev.d_pos, W, H, dev.d_mask, light=lt, stream=s1))
        graphs.append(g)
        _kernels_only(g, 1, "split table, state exists")
        _scribble(k, lt)
        _replay_masks(ctx, g, s1, dev, scene, want, what="split (a)")
        assert (ctx.get_option("split_tiles"), ctx.get_option("split_pieces"), ctx.get_option("front_tiles")) == table
        # (b) the first ever trace on s2 is the captured one
        ctx.h2d(dev.d_pos, scene.pos[0])
        g = hipgraph.capture(s2, lambda: ctx.trace_shadow_mask_device(scene.k, dev.d_pos, W, H, dev.d_mask, light=light, stream=s2))
        graphs.append(g)
        _kernels_only(g, 1, "split table, first trace of the stream")
        _replay_masks(ctx, g, s2, dev, scene, want, what="split (b)")
        assert (ctx.get_option("split_tiles"), ctx.get_option("split_pieces"), ctx.get_option("front_tiles")) == table
        # ... and s2 gets its state at its first trace outside capture, after which a capture carries the table too
        dev.guard()
        ctx.h2d(dev.d_pos, scene.pos[0])
        ctx.trace_shadow_mask_device(scene.k, dev.d_pos, W, H, dev.d_mask, light=light, stream=s2)
        assert int((dev.mask(s2) != want(0)).sum()) == 0
        g = hipgraph.capture(s2, lambda: ctx.trace_shadow_mask_device(scene.k, dev.d_pos, W, H, dev.d_mask, light=light, stream=s2))
        graphs.append(g)
        _kernels_only(g, 1, "split table, second capture")
        _replay_masks(ctx, g, s2, dev, scene, want, what="split (b), second capture")
    finally:
        for g in graphs:
            g.close()
        for s in (s1, s2):
            ctx.synchronize(s)
            ctx.stream_destroy(s)
        ctx.clear_splits()
        dev.close()


@pytest.mark.parametrize("kernel", [7, 3, 8])
def test_whole_frame_in_one_graph(ctx, scene, kernel):
    """G-buffer -> facing mark -> active trace -> combine: four kernel nodes; rgb equals the host pipeline's and the uncaptured frame's."""
    wl, sc = scene.wl, scene.wl.scene
    f = _Frame(ctx, scene)
    dev = f.dev
    stream = ctx.stream_create()
    light = scene.lights["point"]
    cam = 1
    eye = scene.eyes[cam]
    kcam = api.RayTracingConstants.make(eye, sc.light_direction, W, H, sc.target - eye)
    g = None

    def frame(k, lt):
        api.primary_gbuffer_device(ctx, eye, sc.target, sc.fovy, W, H, dev.d_pos, f.d_nrm, stream=stream)
        api.facing_active_device(ctx, k, lt, dev.d_pos, f.d_nrm, W, H, dev.d_act, stream=stream)
        ctx.trace_shadow_mask_device(k, dev.d_pos, W, H, dev.d_mask, light=lt, stream=stream, d_active=dev.d_act)
        api.combine_device(ctx, k, lt, dev.d_pos, f.d_nrm, dev.d_mask, W, H, f.d_rgb, stream=stream)

    def scrub():
        for d, n in ((dev.d_pos, W * H * 16), (f.d_nrm, W * H * 16), (dev.d_act, W * H), (dev.d_mask, W * H), (f.d_rgb, W * H * 3)):
            f.fill(d, n)

    try:
        ctx.set_option("kernel", kernel)
        full, _, _ = oracle.shadow_mask(wl.packed, kcam.as_array(), oracle.light_from_product(light, kcam), scene.pos[cam], W, H)
        mark = api.facing_active(kcam, light, scene.pos[cam], scene.nrm[cam])
        mask = _expect(full, mark)
        assert 0 < np.count_nonzero(mask[mark != 0]) < np.count_nonzero(mark)
        want = api.combine(kcam, light, scene.pos[cam], scene.nrm[cam], mask)
        scrub()
        frame(kcam, light)
        uncaptured = f.read(f.d_rgb, (H, W, 3), np.uint8, stream)
        assert np.array_equal(uncaptured, want)
        k, lt = _copy(kcam), _copy(light)
        g = hipgraph.capture(stream, lambda: frame(k, lt))
        _kernels_only(g, 4, "whole frame")
        _scribble(k, lt)
        for _ in range(2):
            scrub()
            g.launch(stream)
            got = f.read(f.d_rgb, (H, W, 3), np.uint8, stream)
            assert np.array_equal(got, want) and np.array_equal(got, uncaptured)
            assert np.array_equal(f.read(dev.d_mask, (H, W), np.uint8, stream), mask)
    finally:
        if g:
            g.close()
        ctx.synchronize(stream)
        ctx.stream_destroy(stream)
        f.close()
