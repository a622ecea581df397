"""GPU: follow mode (option "follow") -- traces that record their tile lives and run the order the device planned from the stream's
last ones.  The device planner must equal its host twin (rtsh_follow_order) byte for byte; masks must equal the oracle's and those
of follow off over a moving camera; state is per stream and follows the rules of include/rts.h."""
import numpy as np
import pytest

import oracle
from raytracedshadows_amd import api, workloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


_WL = {}


def _wl(name):
    if name not in _WL:
        _WL[name] = workloads.prepare_config(name, cache=True)
    return _WL[name]


def _ids(order, bx):
    return (order & 0xFFFF) + (order >> 16) * bx


def _want(wl, positions, constants, light=None):
    light = wl.light if light is None else light
    m, _, _ = oracle.shadow_mask(wl.packed, constants.as_array(), oracle.light_from_product(light, constants), positions, wl.W, wl.H)
    return m


class _Frames:
    """A camera path: the eye moved `step` of eye -> target per frame; G-buffers made on the device (untimed, not checked here)."""

    def __init__(self, ctx, wl, step):
        self.ctx, self.wl, self.step = ctx, wl, step
        self.d_pos = ctx.malloc(wl.W * wl.H * 16)

    def constants(self, i):
        sc = self.wl.scene
        eye = (sc.eye + (sc.target - sc.eye) * np.float32(self.step * i)).astype(np.float32)
        return eye, api.RayTracingConstants.make(eye, sc.light_direction, self.wl.W, self.wl.H, sc.target - eye)

    def make(self, i, stream=None):
        eye, k = self.constants(i)
        api.primary_gbuffer_device(self.ctx, eye, self.wl.scene.target, self.wl.scene.fovy, self.wl.W, self.wl.H, self.d_pos, stream=stream)
        return k

    def positions(self):
        p = np.empty(self.wl.W * self.wl.H * 4, np.float32)
        self.ctx.synchronize()
        self.ctx.d2h(p, self.d_pos)
        return p

    def close(self):
        self.ctx.free(self.d_pos)


def _mask(ctx, d_mask, wl, stream=None):
    got = np.empty((wl.H, wl.W), np.uint8)
    ctx.synchronize(stream)
    ctx.d2h(got, d_mask)
    return got


@pytest.mark.parametrize("case", [("atrium_1080p", 3, None), ("atrium_1080p", 8, None), ("city_4k", -1, None),
                                  ("city_4k", -1, (32, 8, 3)), ("city_4k", 8, "directional")])
@pytest.mark.parametrize("S,B", [(0, 1), (32, 1), (0, 8), (32, 8)])
def test_device_order_equals_host_twin(ctx, case, S, B):
    name, kernel, form = case
    wl = _wl(name)
    ctx.set_bvh(wl.packed)
    ctx.set_option("kernel", kernel)
    ctx.set_option("follow", 1)
    ctx.set_option("follow_block", B)
    ctx.set_option("follow_square", S)
    d_pos, d_mask = ctx.malloc(wl.positions.nbytes), ctx.malloc(wl.W * wl.H)
    try:
        ctx.h2d(d_pos, wl.positions)
        bx = (wl.W + 7) // 8
        light = None if form == "directional" else wl.light
        if isinstance(form, tuple):
            rows = api.stripe_rows(wl.H, *form)
            by = (rows + 7) // 8
            go = lambda: ctx.trace_shadow_mask_stripes_device(wl.constants, d_pos, wl.W, wl.H, d_mask, *form, light=light)
        else:
            by = (wl.H + 7) // 8
            go = lambda: ctx.trace_shadow_mask_device(wl.constants, d_pos, wl.W, wl.H, d_mask, light=light)
        ordered = ctx.get_option("follow_ordered")
        for _ in range(3):
            go()
        assert ctx.get_option("follow_ordered") == ordered + 2                # the first trace records, the next two run the order
        assert ctx.last_kernel_name().startswith("shadowMaskFollowKernel<1")
        lives, order = ctx.read_follow(bx * by)
        assert (lives > 0).all(), "every tile's wave recorded its life"
        ids = _ids(order, bx)
        assert sorted(ids.tolist()) == list(range(bx * by))
        assert np.array_equal(ids, api.follow_order(lives, bx, by, 0, S, B))
        if not isinstance(form, tuple):
            m, _, _ = oracle.shadow_mask(wl.packed, wl.constants.as_array(), oracle.light_from_product(light, wl.constants), wl.positions,
                                         wl.W, wl.H)
            assert int((_mask(ctx, d_mask, wl) != m).sum()) == 0
    finally:
        ctx.set_option("follow", 0)
        ctx.set_option("kernel", -1)
        ctx.free(d_pos)
        ctx.free(d_mask)


@pytest.mark.parametrize("name", ["atrium_1080p", "city_4k"])
def test_camera_path_masks_are_exact(name):
    wl = _wl(name)
    with api.ShadowContext(0) as on, api.ShadowContext(0) as off:
        on.set_bvh(wl.packed)
        off.set_bvh(wl.packed)
        on.set_option("follow", 1)
        frames = _Frames(on, wl, 0.001)
        d_a, d_b = on.malloc(wl.W * wl.H), on.malloc(wl.W * wl.H)
        try:
            for i in range(20):
                k = frames.make(i)
                before = on.get_option("follow_ordered")
                on.trace_shadow_mask_device(k, frames.d_pos, wl.W, wl.H, d_a, light=wl.light)
                assert on.get_option("follow_ordered") == before + (1 if i >= 1 else 0), f"frame {i + 1}"
                on.synchronize()
                off.trace_shadow_mask_device(k, frames.d_pos, wl.W, wl.H, d_b, light=wl.light)
                a, b = _mask(on, d_a, wl), _mask(off, d_b, wl)
                assert np.array_equal(a, b), f"frame {i}: follow on and off differ"
                if name == "atrium_1080p" or i in (0, 1, 2, 19):
                    assert int((a != _want(wl, frames.positions(), k)).sum()) == 0, f"frame {i}"
        finally:
            on.free(d_a)
            on.free(d_b)
            frames.close()


def test_two_streams_keep_their_own_state(ctx):
    wl = _wl("atrium_1080p")
    ctx.set_bvh(wl.packed)
    ctx.set_option("follow", 1)
    s1, s2 = ctx.stream_create(), ctx.stream_create()
    fa, fb = _Frames(ctx, wl, 0.001), _Frames(ctx, wl, -0.003)
    d_a, d_b = ctx.malloc(wl.W * wl.H), ctx.malloc(wl.W * wl.H)
    bx, by = (wl.W + 7) // 8, (wl.H + 7) // 8
    try:
        for i in range(6):
            ka = fa.make(i, stream=s1)
            kb = fb.make(i, stream=s2)
            ctx.trace_shadow_mask_device(ka, fa.d_pos, wl.W, wl.H, d_a, light=wl.light, stream=s1)
            ctx.trace_shadow_mask_device(kb, fb.d_pos, wl.W, wl.H, d_b, light=wl.light, stream=s2)
        assert ctx.get_option("follow_streams") == 2
        for s, f, d, k in ((s1, fa, d_a, ka), (s2, fb, d_b, kb)):
            lives, order = ctx.read_follow(bx * by, stream=s)
            assert np.array_equal(_ids(order, bx), api.follow_order(lives, bx, by, 0, ctx.get_option("follow_square"),
                                                                    ctx.get_option("follow_block")))
            ctx.synchronize(s)
            assert int((_mask(ctx, d, wl, s) != _want(wl, f.positions(), k)).sum()) == 0
        la, _ = ctx.read_follow(bx * by, stream=s1)
        lb, _ = ctx.read_follow(bx * by, stream=s2)
        assert not np.array_equal(la, lb)
    finally:
        ctx.synchronize(s1)
        ctx.synchronize(s2)
        ctx.stream_destroy(s1)
        ctx.stream_destroy(s2)
        assert ctx.get_option("follow_streams") == 0
        ctx.set_option("follow", 0)
        for p in (d_a, d_b):
            ctx.free(p)
        fa.close()
        fb.close()


def test_state_rules(ctx):
    wl = _wl("cornell_256")
    want = _want(wl, wl.positions, wl.constants)
    ctx.set_bvh(wl.packed)
    ctx.set_option("kernel", 3)
    ctx.set_option("follow", 1)
    d_pos, d_mask = ctx.malloc(wl.positions.nbytes), ctx.malloc(wl.W * wl.H)
    n = ((wl.W + 7) // 8) * ((wl.H + 7) // 8)

    def trace(**kw):
        ctx.h2d(d_mask, np.full(wl.W * wl.H, 7, np.uint8))
        ctx.trace_shadow_mask_device(wl.constants, d_pos, wl.W, wl.H, d_mask, light=wl.light, **kw)
        got = _mask(ctx, d_mask, wl, kw.get("stream"))
        rows = slice(kw.get("row_begin", 0), kw.get("row_end", wl.H))
        assert int((got[rows] != want[rows]).sum()) == 0

    try:
        ctx.h2d(d_pos, wl.positions)
        with pytest.raises(api.RtsError):
            ctx.read_follow(n)                                                 # no state yet
        trace()
        o = ctx.get_option("follow_ordered")
        trace()
        assert ctx.get_option("follow_ordered") == o + 1 and ctx.get_option("follow_streams") == 1
        assert ctx.last_kernel_name() == "shadowMaskFollowKernel<1>"
        # a geometry change resets the stream's state
        trace(row_begin=0, row_end=128)
        assert ctx.get_option("follow_ordered") == o + 1
        with pytest.raises(api.RtsError):
            ctx.read_follow(n)
        ctx.read_follow(n // 2)
        trace()
        trace()
        assert ctx.get_option("follow_ordered") == o + 2
        # a refit keeps it
        api.bvh_refit_device(ctx, wl.vertices, 8, wl.indices, wl.prim_count)
        assert ctx.get_option("follow_streams") == 1
        trace()
        assert ctx.get_option("follow_ordered") == o + 3
        # an explicit split table wins
        ctx.plan_splits(wl.constants, d_pos, wl.W, wl.H, d_mask, light=wl.light, min_life_us=4.0, piece_us=2.0, max_pieces=8,
                        front_share=1.0 / 3.0)
        assert ctx.get_option("split_tiles") + ctx.get_option("front_tiles") > 0
        trace()
        assert ctx.get_option("follow_ordered") == o + 3
        assert ctx.last_kernel_name() == "shadowMaskPacketKernel<1>"
        ctx.clear_splits()
        trace()
        assert ctx.get_option("follow_ordered") == o + 4
        # set_bvh drops everything
        ctx.set_bvh(wl.packed)
        assert ctx.get_option("follow_streams") == 0
        trace()
        trace()
        assert ctx.get_option("follow_ordered") == o + 5
        # "follow" 0 drops it and restores the everyday kernel
        ctx.set_option("follow", 0)
        assert ctx.get_option("follow_streams") == 0
        trace()
        assert ctx.last_kernel_name() == "shadowMaskPacketKernel<1>"
        assert ctx.get_option("follow_ordered") == o + 5
        # rts_stream_destroy releases the stream's state
        ctx.set_option("follow", 1)
        s = ctx.stream_create()
        trace(stream=s)
        assert ctx.get_option("follow_streams") == 1
        ctx.stream_destroy(s)
        assert ctx.get_option("follow_streams") == 0
    finally:
        ctx.clear_splits()
        ctx.set_option("follow", 0)
        ctx.set_option("kernel", -1)
        ctx.free(d_pos)
        ctx.free(d_mask)


def test_steady_frames_allocate_nothing(ctx):
    wl = _wl("atrium_1080p")
    ctx.set_bvh(wl.packed)
    ctx.set_option("follow", 1)
    frames = _Frames(ctx, wl, 0.001)
    pos = []
    for i in range(2):                                                         # two G-buffers, alternated: a camera that moves
        frames.make(5 * i)
        pos.append(frames.positions())
    d_pos, d_mask = ctx.malloc(wl.positions.nbytes), ctx.malloc(wl.W * wl.H)
    try:
        free = []
        for i in range(20):
            ctx.h2d(d_pos, pos[i % 2])
            ctx.trace_shadow_mask_device(wl.constants, d_pos, wl.W, wl.H, d_mask, light=wl.light)
            ctx.synchronize()
            if i >= 1:
                free.append(ctx.mem_info()[0])
        assert len(set(free)) == 1, free
        assert ctx.get_option("follow_ordered") >= 19
    finally:
        ctx.set_option("follow", 0)
        ctx.free(d_pos)
        ctx.free(d_mask)
        frames.close()


def test_a_stream_starts_over_when_any_field_of_the_geometry_changes(ctx):
    """A stream's follow state belongs to one dispatch: W, H, the row range, the band, the number of stripes and the stripe.  After two
    traces of a dispatch (the second runs the planned order), a first trace that differs in ONE of the seven runs no order, resets
    the stream's state in place, and gives the mask of the same trace with follow off."""
    wl = workloads.prepare("cornell", 64, 64, via_obj=False)
    rows = lambda W, H, b, e: lambda **kw: ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_mask, light=wl.light, row_begin=b, row_end=e, **kw)
    stripes = lambda band, n, r: lambda **kw: ctx.trace_shadow_mask_stripes_device(wl.constants, d_pos, 64, 64, d_mask, band, n, r, light=wl.light, **kw)
    cases = {"W": (rows(64, 64, 0, 64), rows(56, 64, 0, 64)),
             "H": (rows(64, 64, 0, 56), rows(64, 56, 0, 56)),
             "row_begin": (rows(64, 64, 0, 64), rows(64, 64, 8, 64)),
             "row_end": (rows(64, 64, 0, 64), rows(64, 64, 0, 56)),
             "band_rows": (stripes(8, 2, 0), stripes(16, 2, 0)),
             "n_stripes": (stripes(8, 2, 0), stripes(8, 4, 0)),
             "stripe": (stripes(8, 2, 0), stripes(8, 2, 1))}
    ctx.set_bvh(wl.packed)
    ctx.set_option("kernel", 3)
    d_pos, d_mask = ctx.malloc(wl.positions.nbytes), ctx.malloc(64 * 64)

    def mask_of(trace):
        ctx.h2d(d_mask, np.full(64 * 64, 7, np.uint8))
        trace()
        got = np.empty(64 * 64, np.uint8)
        ctx.synchronize()
        ctx.d2h(got, d_mask)
        return got

    try:
        ctx.h2d(d_pos, wl.positions)
        ctx.set_option("follow", 0)
        plain = {field: mask_of(changed) for field, (_, changed) in cases.items()}
        assert ctx.last_kernel_name() == "shadowMaskPacketKernel<1>"
        ctx.set_option("follow", 1)
        for field, (base, changed) in cases.items():
            base()
            ordered = ctx.get_option("follow_ordered")
            base()
            assert ctx.get_option("follow_ordered") == ordered + 1, field
            traces = ctx.get_option("follow_traces")
            got = mask_of(changed)
            assert ctx.get_option("follow_ordered") == ordered + 1, f"{field}: the order of another dispatch was run"
            assert ctx.get_option("follow_traces") == traces + 1 and ctx.last_kernel_name() == "shadowMaskFollowKernel<1>", field
            assert ctx.get_option("follow_streams") == 1, field
            assert np.array_equal(got, plain[field]), f"{field}: follow on and off differ"
            assert (got != 7).any(), field
    finally:
        ctx.set_option("follow", 0)
        ctx.set_option("kernel", -1)
        ctx.free(d_pos)
        ctx.free(d_mask)
