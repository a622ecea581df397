"""GPU: soft light list distance traces (rts_trace_soft_light_list_distance*; include/rts.h) against the host twin
(rtsh_soft_light_list_distance, which tests/test_soft_list_distance_host.py pins to the oracle), bit for bit, on guard-filled buffers of
8 planes each -- the distances' guard a NaN's bit pattern no trace writes: every list in the three forms -- lane per ray, the packet
with four waves per tile, with one --, light maps (the facing map made on the device, poisoned unmarked pixels, empty tiles and blocks,
a light with no pixel or a single one), row ranges and stripes, counts left out, options that may only change speed, installed state
that must stay, the counters and kernel names, the device's own one-light soft distance traces and soft light list, graph capture,
the far-before-near stream, the refusals, and the smallest stream.  Planes at or above the count must keep the guard in both outputs."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
from distance_cases import INF_BITS, bits, far_before_near, far_before_near_frame
from raytracedshadows_amd import api, workloads
from soft_list_distance_cases import DIST_GUARD, FORMS, FRAMES, LISTS, TABLE, distance_frame, make_list, samples, under
from test_gpu_soft_light_list import _maps
from test_soft_light_list_host import bad_lists

pytestmark = pytest.mark.gpu

GUARD = 0xAB
SHARE = "shadowSoftLightListDistanceShareKernel"
POISON = np.array([np.nan, np.inf, 1e38, -np.inf], np.float32)
COUNTER = "soft_list_distance_traces"
OTHERS = ("active_traces", "distance_traces", "soft_distance_traces", "light_list_traces", "adaptive_traces", "soft_light_list_traces",
          "soft_list_adaptive_traces", "soft_list_jitter_traces")


def _name(kernel, split, geom="rows"):
    return SHARE if kernel in (0, 1, 2, 7) else "shadowSoftLightListDistancePacketKernel<%d,%s>" % (4 if split else 1, geom)


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


def _reset(ctx):
    for key, v in (("kernel", -1), ("soft_split", 1), ("xcd_swizzle", 0), ("row_order", 0)):
        ctx.set_option(key, v)


def _form(ctx, kernel, split):
    ctx.set_option("kernel", kernel)
    ctx.set_option("soft_split", split)


class _Dev:
    """Positions, a map and 8 planes of distances and of counts on the device."""

    def __init__(self, ctx, positions, W, H):
        self.ctx, self.W, self.H = ctx, W, H
        positions = np.ascontiguousarray(positions, np.float32)
        self.d_pos, self.d_map = ctx.malloc(positions.nbytes), ctx.malloc(W * H)
        self.d_dist, self.d_counts = ctx.malloc(8 * W * H * 4), ctx.malloc(8 * W * H)
        ctx.h2d(self.d_pos, positions)

    def guard(self):
        self.ctx.h2d(self.d_dist, np.full(8 * self.W * self.H, DIST_GUARD, np.uint32))
        self.ctx.h2d(self.d_counts, np.full(8 * self.W * self.H, GUARD, np.uint8))

    def read(self, stream=None):
        """(uint32[8, H, W] the distances' bits, uint8[8, H, W] the counts)"""
        d, c = np.empty((8, self.H, self.W), np.uint32), np.empty((8, self.H, self.W), np.uint8)
        self.ctx.synchronize(stream)
        self.ctx.d2h(d, self.d_dist)
        self.ctx.d2h(c, self.d_counts)
        return d, c

    def read_plane(self, what, dtype):
        m = np.empty((self.H, self.W), dtype)
        self.ctx.synchronize()
        self.ctx.d2h(m, what)
        return m

    def close(self):
        for d in (self.d_pos, self.d_map, self.d_dist, self.d_counts):
            self.ctx.free(d)


def _expect(want, lights_map=None, rows=None):
    """All 8 planes of both outputs: the twin's planes under the map's bits in the rows, the guards in the other rows and in the planes
    from the count up."""
    wd, wc = want if lights_map is None else under(want[0], want[1], lights_map)
    n = wd.shape[0]
    d, c = np.full((8,) + wd.shape[1:], DIST_GUARD, np.uint32), np.full((8,) + wd.shape[1:], GUARD, np.uint8)
    d[:n] = bits(wd) if rows is None else np.where(rows[None, :, None], bits(wd), DIST_GUARD)
    c[:n] = wc if rows is None else np.where(rows[None, :, None], wc, GUARD)
    return d, c


def _same(got, want, what):
    for g, w, which in ((got[0], want[0], "distance bits"), (got[1], want[1], "counts")):
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, which, bad.shape[0], bad[:4].tolist(), [hex(int(g[tuple(b)])) for b in bad[:4]],
                                   [hex(int(w[tuple(b)])) for b in bad[:4]])


def _trace(ctx, dev, fr, lights, want, what, lights_map=None, rows=None, **kw):
    if lights_map is not None:
        ctx.h2d(dev.d_map, np.ascontiguousarray(lights_map, np.uint8))
    dev.guard()
    ctx.trace_soft_light_list_distance_device(fr.k, lights, dev.d_pos, fr.W, fr.H, dev.d_dist, dev.d_counts,
                                              d_lights_map=dev.d_map if lights_map is not None else None, **kw)
    _same(dev.read(), _expect(want, lights_map, rows), what)


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("name", list(LISTS))
def test_every_list_in_the_three_forms_equals_the_twin(ctx, name, W, H):
    """Also "3pairs" (wave 3 of four owns no pair and contributes +Inf / 0), "48" (one light of 48 samples) and "8x2" (all eight minimum
    words and both count words of a lane in use): the extremes of the packet kernel's LDS."""
    fr = distance_frame(W, H)
    lights, want = make_list(name), fr.want(name)
    for l in range(lights.count):                        # counts == n exactly where the distance is +Inf
        assert np.array_equal(bits(want[0][l]) == INF_BITS, want[1][l] == samples(lights, l))
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, W, H)
    try:
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            _trace(ctx, dev, fr, lights, want, (name, kernel, split))
            assert ctx.last_kernel_name() == _name(kernel, split), (kernel, split, ctx.last_kernel_name())
        # the host form: its rows alone travel, and both outputs come back to planes of H rows
        out_d, out_c = np.full((8, H, W), DIST_GUARD, np.uint32).view(np.float32), np.full((8, H, W), GUARD, np.uint8)
        got = ctx.trace_soft_light_list_distance(fr.k, lights, fr.pos, W, H, row_begin=3, row_end=30, out=out_d, counts=out_c)
        assert got[0] is out_d and got[1] is out_c
        rows = (np.arange(H) >= 3) & (np.arange(H) < 30)
        _same((bits(out_d), out_c), _expect(want, None, rows), (name, "host rows"))
    finally:
        _reset(ctx)
        dev.close()


def test_auto_takes_the_lane_walk_below_256k_pixels(ctx):
    fr = distance_frame(61, 37)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        assert ctx.get_option("kernel") == -1
        _trace(ctx, dev, fr, make_list("3pairs"), fr.want("3pairs"), "defaults")
        assert ctx.last_kernel_name() == SHARE
    finally:
        dev.close()


# ---- 2. the map -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", FORMS)
@pytest.mark.parametrize("name", ["overlap", "8x2"])
def test_light_maps(ctx, name, kernel, split):
    fr = distance_frame(64, 48)
    lights, want = make_list(name), fr.want(name)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    below = (1 << lights.count) - 1
    try:
        _form(ctx, kernel, split)
        for what, m in _maps(fr, lights.count).items():
            dirty = fr.pos.copy()                        # a pixel no light is marked for may hold anything
            dirty[(m & below) == 0] = POISON
            ctx.h2d(dev.d_pos, dirty)
            _trace(ctx, dev, fr, lights, want, (name, kernel, split, what), lights_map=m)
            got = dev.read()
            if what == "full":                           # NULL equals a map of 0xFF
                _trace(ctx, dev, fr, lights, want, (name, kernel, split, "NULL"))
                _same(dev.read(), got, "NULL against 0xFF")
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("W,H", FRAMES)
def test_the_facing_map_made_on_the_device(ctx, W, H):
    fr = distance_frame(W, H)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, W, H)
    d_nrm = ctx.malloc(fr.nrm.nbytes)
    try:
        ctx.h2d(d_nrm, fr.nrm)
        for name in ("mixed", "8x2"):
            lights, host_map = make_list(name), fr.facing(name)
            ctx.h2d(dev.d_map, np.full(W * H, GUARD, np.uint8))
            api.facing_lights_device(ctx, fr.k, lights.hard_list(), dev.d_pos, d_nrm, W, H, dev.d_map)
            assert np.array_equal(dev.read_plane(dev.d_map, np.uint8), host_map), (name, "device map against host map")
            assert 0 < int((host_map != 0).sum()) < host_map.size
            for kernel, split in FORMS:
                _form(ctx, kernel, split)
                dev.guard()
                ctx.trace_soft_light_list_distance_device(fr.k, lights, dev.d_pos, W, H, dev.d_dist, dev.d_counts, d_lights_map=dev.d_map)
                _same(dev.read(), _expect(fr.want(name), host_map), (name, kernel, split, "facing"))
    finally:
        _reset(ctx)
        ctx.free(d_nrm)
        dev.close()


# ---- 3. geometry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", FORMS)
def test_row_ranges_leave_the_other_rows(ctx, kernel, split):
    fr = distance_frame(64, 48)
    lights, want = make_list("mixed"), fr.want("mixed")
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    m = _maps(fr, 5)["mixed"]
    try:
        _form(ctx, kernel, split)
        for b, e in ((8, 40), (16, 32), (5, 41)):
            rows = (np.arange(fr.H) >= b) & (np.arange(fr.H) < e)
            _trace(ctx, dev, fr, lights, want, (kernel, split, b, e), rows=rows, row_begin=b, row_end=e)
            _trace(ctx, dev, fr, lights, want, (kernel, split, b, e, "map"), lights_map=m, rows=rows, row_begin=b, row_end=e)
        n0 = ctx.get_option(COUNTER)
        _trace(ctx, dev, fr, lights, want, "empty range", rows=np.zeros(fr.H, bool), row_begin=7, row_end=7)
        assert ctx.get_option(COUNTER) == n0
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel,split,band", [(3, 1, 8), (3, 1, 16), (3, 0, 8), (3, 0, 16), (7, 1, 16)])
def test_stripes(ctx, kernel, split, band):
    fr = distance_frame(61, 37)
    lights, want = make_list("mixed"), fr.want("mixed")
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    m = _maps(fr, 5)["mixed"]
    ctx.h2d(dev.d_map, m)
    try:
        _form(ctx, kernel, split)
        for with_map in (False, True):
            for stripe in range(3):                      # (37 rows in bands of 16: stripe 2 owns band 2, rows 32..36)
                rows = ((np.arange(fr.H) // band) % 3) == stripe
                dev.guard()
                ctx.trace_soft_light_list_distance_stripes_device(fr.k, lights, dev.d_pos, fr.W, fr.H, dev.d_dist, band, 3, stripe,
                                                                  d_counts=dev.d_counts, d_lights_map=dev.d_map if with_map else None)
                _same(dev.read(), _expect(want, m if with_map else None, rows), (kernel, split, band, with_map, stripe))
                assert ctx.last_kernel_name() == _name(kernel, split, "bands"), ctx.last_kernel_name()
        # a stripe that owns no band launches nothing, writes nothing and returns OK (37 rows in bands of 16: bands 0..2, stripe 3 of 4)
        n0 = ctx.get_option(COUNTER)
        dev.guard()
        ctx.trace_soft_light_list_distance_stripes_device(fr.k, lights, dev.d_pos, fr.W, fr.H, dev.d_dist, 16, 4, 3, d_counts=dev.d_counts)
        d, c = dev.read()
        assert (d == DIST_GUARD).all() and (c == GUARD).all() and ctx.get_option(COUNTER) == n0
        if kernel == 3:                                  # 24 rows: not a power of two -- the general form
            rows = ((np.arange(fr.H) // 24) % 2) == 1
            dev.guard()
            ctx.trace_soft_light_list_distance_stripes_device(fr.k, lights, dev.d_pos, fr.W, fr.H, dev.d_dist, 24, 2, 1,
                                                              d_counts=dev.d_counts)
            _same(dev.read(), _expect(want, None, rows), (kernel, split, 24))
            assert ctx.last_kernel_name() == _name(kernel, split, "general")
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel,split", FORMS)
def test_the_general_grid_and_the_row_orders(ctx, kernel, split):
    fr = distance_frame(61, 37)
    lights, want = make_list("8x2"), fr.want("8x2")
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    m = _maps(fr, 8)["mixed"]
    try:
        _form(ctx, kernel, split)
        ctx.set_option("xcd_swizzle", 1)
        _trace(ctx, dev, fr, lights, want, (kernel, split, "swizzle"), lights_map=m)
        assert ctx.last_kernel_name() == _name(kernel, split, "general")
        rows = (np.arange(fr.H) >= 5) & (np.arange(fr.H) < 30)
        _trace(ctx, dev, fr, lights, want, (kernel, split, "swizzle rows"), rows=rows, row_begin=5, row_end=30)
        ctx.set_option("xcd_swizzle", 0)
        for order in (1, 2):
            ctx.set_option("row_order", order)
            _trace(ctx, dev, fr, lights, want, (kernel, split, "row_order", order), lights_map=m)
            assert ctx.last_kernel_name() == _name(kernel, split, "rows")
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel,split", FORMS)
def test_counts_null_leaves_the_counts_alone(ctx, kernel, split):
    fr = distance_frame(61, 37)
    lights, want = make_list("overlap"), fr.want("overlap")
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    maps = _maps(fr, 3)
    try:
        _form(ctx, kernel, split)
        for m in (None, maps["mixed"], maps["zeros"], maps["holes"]):
            if m is not None:
                ctx.h2d(dev.d_map, m)
            dev.guard()
            ctx.trace_soft_light_list_distance_device(fr.k, lights, dev.d_pos, fr.W, fr.H, dev.d_dist, None,
                                                      d_lights_map=dev.d_map if m is not None else None)
            d, c = dev.read()
            assert np.array_equal(d, _expect(want, m)[0]) and (c == GUARD).all(), (kernel, split)
        d, none = ctx.trace_soft_light_list_distance(fr.k, lights, fr.pos, fr.W, fr.H, want_counts=False)
        assert none is None and np.array_equal(bits(d), bits(want[0]))
    finally:
        _reset(ctx)
        dev.close()


# ---- 4. options change no bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [1, 0])
def test_options_change_no_bit(ctx, split):
    fr = distance_frame(64, 48)
    lights, want = make_list("mixed"), fr.want("mixed")
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    before = (ctx.get_option("packet_budget"), ctx.get_option("packet_share"))
    m = _maps(fr, 5)["mixed"]
    try:
        ctx.set_option("soft_split", split)
        ctx.set_option("kernel", 3)
        ctx.set_option("packet_budget", 1)               # every packet dissolves at once
        ctx.set_option("packet_share", 16)
        _trace(ctx, dev, fr, lights, want, ("dissolve", split))
        _trace(ctx, dev, fr, lights, want, ("dissolve", split, "map"), lights_map=m)
        ctx.set_option("packet_budget", before[0])
        ctx.set_option("packet_share", before[1])
        ctx.set_option("kernel", 8)                      # the stream has a private copy; this trace runs the stackless packet all the same
        assert ctx.get_option("wide_nodes") > 0
        _trace(ctx, dev, fr, lights, want, ("kernel 8", split), lights_map=m)
        assert ctx.last_kernel_name() == _name(3, split)
        ctx.set_option("kernel", 9)
        _trace(ctx, dev, fr, lights, want, ("kernel 9", split))
        assert ctx.last_kernel_name() == _name(3, split)
    finally:
        ctx.set_option("packet_budget", before[0])
        ctx.set_option("packet_share", before[1])
        _reset(ctx)
        dev.close()


# ---- 5. installed state stays ---------------------------------------------------------------------------------------------------
def test_installed_state_stays(ctx):
    wl = workloads.prepare_config("cornell_256")
    W, H = wl.W, wl.H
    lights = api.SoftLightList.make([(wl.light.type, list(wl.light.xyz)),
                                     (api.Light.DIRECTIONAL, list(wl.scene.light_direction), 3, 7, 0.1)], TABLE)
    want = api.soft_light_list_distance(wl.packed, wl.constants, lights, wl.positions, W, H)
    plain = want[1][0]                                   # light 0 is the workload's own: the plain trace's byte
    assert 0 < int(plain.sum()) < plain.size
    ctx.set_bvh(wl.packed)
    dev = _Dev(ctx, wl.positions, W, H)

    def list_trace():
        n0 = ctx.get_option(COUNTER)
        dev.guard()
        ctx.trace_soft_light_list_distance_device(wl.constants, lights, dev.d_pos, W, H, dev.d_dist, dev.d_counts)
        _same(dev.read(), _expect(want), "list")
        assert ctx.get_option(COUNTER) == n0 + 1 and ctx.last_kernel_name() == _name(3, 1)

    def plain_trace():
        dev.guard()
        ctx.trace_shadow_mask_device(wl.constants, dev.d_pos, W, H, dev.d_counts, light=wl.light)
        assert np.array_equal(dev.read()[1][0], plain), "plain"
        return ctx.last_kernel_name()

    try:
        ctx.set_option("kernel", 3)
        # a split table
        tiles, records = ctx.plan_splits(wl.constants, dev.d_pos, W, H, dev.d_counts, light=wl.light, min_life_us=4.0, piece_us=2.0,
                                         max_pieces=8, front_share=1.0 / 3.0)
        assert tiles > 0
        table = tuple(ctx.get_option(k) for k in ("split_tiles", "front_tiles", "split_pieces"))
        name_before = plain_trace()
        list_trace()
        assert tuple(ctx.get_option(k) for k in ("split_tiles", "front_tiles", "split_pieces")) == table
        assert plain_trace() == name_before
        ctx.clear_splits()
        # a caller's tile order
        order = np.arange(((W + 7) // 8) * ((H + 7) // 8), dtype=np.uint32)[::-1].copy()
        ctx.set_tile_order(order)
        order_state = (ctx.get_option("tile_order_tiles"), ctx.get_option("tile_order"))
        assert order_state[0] == order.size
        name_before = plain_trace()
        list_trace()
        assert (ctx.get_option("tile_order_tiles"), ctx.get_option("tile_order")) == order_state
        assert plain_trace() == name_before
        ctx.set_tile_order(None)
        # follow mode
        ctx.set_option("follow", 1)
        plain_trace()
        name_follow = plain_trace()
        assert name_follow.startswith("shadowMaskFollowKernel<")
        traces, ordered = ctx.get_option("follow_traces"), ctx.get_option("follow_ordered")
        list_trace()
        assert (ctx.get_option("follow_traces"), ctx.get_option("follow_ordered"), ctx.get_option("follow")) == (traces, ordered, 1)
        assert plain_trace() == name_follow
        assert ctx.get_option("follow_traces") == traces + 1
    finally:
        ctx.set_option("follow", 0)
        ctx.set_tile_order(None)
        ctx.clear_splits()
        _reset(ctx)
        dev.close()


# ---- 6. counters and names ------------------------------------------------------------------------------------------------------
def test_counters_and_names(ctx):
    fr = distance_frame(64, 48)
    lights, want = make_list("overlap"), fr.want("overlap")
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        before = [ctx.get_option(k) for k in OTHERS]
        n0 = ctx.get_option(COUNTER)
        launches = 0
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            _trace(ctx, dev, fr, lights, want, (kernel, split))
            assert ctx.last_kernel_name() == _name(kernel, split, "rows")
            ctx.trace_soft_light_list_distance_stripes_device(fr.k, lights, dev.d_pos, fr.W, fr.H, dev.d_dist, 16, 2, 1, d_counts=dev.d_counts)
            assert ctx.last_kernel_name() == _name(kernel, split, "bands")
            ctx.set_option("xcd_swizzle", 1)
            ctx.trace_soft_light_list_distance_device(fr.k, lights, dev.d_pos, fr.W, fr.H, dev.d_dist, dev.d_counts)
            assert ctx.last_kernel_name() == _name(kernel, split, "general")
            ctx.set_option("xcd_swizzle", 0)
            launches += 3
        ctx.trace_soft_light_list_distance(fr.k, lights, fr.pos, fr.W, fr.H)
        ctx.synchronize()
        assert ctx.get_option(COUNTER) == n0 + launches + 1
        assert [ctx.get_option(k) for k in OTHERS] == before
        with pytest.raises(api.RtsError):                # read-only
            ctx.set_option(COUNTER, 0)
        # ... and neither the one-light soft distance trace nor the soft light list moves it
        n1 = ctx.get_option(COUNTER)
        ctx.trace_soft_distance_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, dev.d_counts, light=lights.light(0))
        ctx.trace_soft_light_list_device(fr.k, lights, dev.d_pos, fr.W, fr.H, dev.d_counts)
        ctx.synchronize()
        assert ctx.get_option(COUNTER) == n1
        assert ctx.get_option("soft_distance_traces") == before[2] + 1 and ctx.get_option("soft_light_list_traces") == before[5] + 1
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel,split", FORMS)
def test_plane_l_is_the_soft_distance_trace_of_light_l(ctx, kernel, split):
    """The definition on the device itself: plane l of both outputs = rts_trace_soft_distance_device for the derived light l with the
    map's bit l as its active byte; and the counts are those of rts_trace_soft_light_list_device."""
    fr = distance_frame(61, 37)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    n = fr.W * fr.H
    d_one, d_mask, d_act, d_planes = ctx.malloc(n * 4), ctx.malloc(n), ctx.malloc(n), ctx.malloc(8 * n)
    try:
        _form(ctx, kernel, split)
        for name in ("8x2", "mixed"):
            lights = make_list(name)
            m = _maps(fr, lights.count)["mixed"]
            _trace(ctx, dev, fr, lights, fr.want(name), "list", lights_map=m)
            got_d, got_c = dev.read()
            for l in range(lights.count):
                ctx.h2d(d_act, np.ascontiguousarray((m >> l) & 1, np.uint8))
                ctx.h2d(d_one, np.full(n, DIST_GUARD, np.uint32))
                ctx.h2d(d_mask, np.full(n, GUARD, np.uint8))
                ctx.trace_soft_distance_device(fr.k, dev.d_pos, fr.W, fr.H, d_one, d_mask, light=lights.light(l), d_active=d_act)
                assert np.array_equal(got_d[l], dev.read_plane(d_one, np.uint32)), (name, "distance of light", l)
                assert np.array_equal(got_c[l], dev.read_plane(d_mask, np.uint8)), (name, "count of light", l)
            ctx.h2d(d_planes, np.full(8 * n, GUARD, np.uint8))
            ctx.trace_soft_light_list_device(fr.k, lights, dev.d_pos, fr.W, fr.H, d_planes, d_lights_map=dev.d_map)
            planes = np.empty((8, fr.H, fr.W), np.uint8)
            ctx.synchronize()
            ctx.d2h(planes, d_planes)
            assert np.array_equal(got_c, planes), (name, "counts against the soft light list")
    finally:
        _reset(ctx)
        for d in (d_one, d_mask, d_act, d_planes):
            ctx.free(d)
        dev.close()


# ---- 7. graph capture -----------------------------------------------------------------------------------------------------------
def _copy(struct):
    return type(struct).from_buffer_copy(struct)


@pytest.mark.parametrize("form", ["whole", "rows", "stripe"])
@pytest.mark.parametrize("kernel,split", FORMS)
def test_device_forms_under_capture(ctx, kernel, split, form):
    fr = distance_frame(64, 48)
    want = fr.want("mixed")
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    maps = _maps(fr, 5)
    stream = ctx.stream_create()
    k, lights = _copy(fr.k), make_list("mixed")
    g = None
    try:
        _form(ctx, kernel, split)
        ctx.h2d(dev.d_map, maps["mixed"])
        ctx.trace_shadow_mask_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_counts, light=lights.light(0), stream=stream)   # a stream that has traced
        ctx.synchronize(stream)
        rows = None
        if form == "whole":
            record = lambda: ctx.trace_soft_light_list_distance_device(k, lights, dev.d_pos, fr.W, fr.H, dev.d_dist, dev.d_counts,
                                                                       d_lights_map=dev.d_map, stream=stream)
        elif form == "rows":
            rows = (np.arange(fr.H) >= 5) & (np.arange(fr.H) < 41)
            record = lambda: ctx.trace_soft_light_list_distance_device(k, lights, dev.d_pos, fr.W, fr.H, dev.d_dist, dev.d_counts,
                                                                       d_lights_map=dev.d_map, stream=stream, row_begin=5, row_end=41)
        else:
            rows = ((np.arange(fr.H) // 16) % 2) == 1
            record = lambda: ctx.trace_soft_light_list_distance_stripes_device(k, lights, dev.d_pos, fr.W, fr.H, dev.d_dist, 16, 2, 1,
                                                                               d_counts=dev.d_counts, d_lights_map=dev.d_map, stream=stream)
        n0 = ctx.get_option(COUNTER)
        g = hipgraph.capture(stream, record)
        assert ctx.get_option(COUNTER) == n0 + 1
        types = g.node_types()
        assert types == [hipgraph.KERNEL], (kernel, split, form, types)   # one kernel node; no memcpy, memset or allocation node
        for s in (k, lights):                            # what a caller may do to its structs between capture and replay
            C.memset(C.byref(s), 0x7F, C.sizeof(s))
        # the replay follows the buffers: the map and the positions the device holds at the replay, not those it held at the capture
        for replay, m in enumerate((maps["mixed"], (255 - maps["mixed"]).astype(np.uint8))):
            dirty = fr.pos.copy()
            dirty[(m & 31) == 0] = POISON
            ctx.h2d(dev.d_pos, dirty)
            ctx.h2d(dev.d_map, m)
            dev.guard()
            g.launch(stream)
            _same(dev.read(stream), _expect(want, m, rows), (kernel, split, form, replay))
    finally:
        if g:
            g.close()
        ctx.synchronize(stream)
        ctx.stream_destroy(stream)
        _reset(ctx)
        dev.close()


# ---- 8. far before near ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", FORMS)
def test_far_before_near(ctx, kernel, split):
    """Two triangles across +z, the far one first in depth-first order: the any-hit walk stops at it, the distance is the near one's."""
    packed, k, pos = far_before_near_frame()
    H, W = pos.shape[:2]
    near = far_before_near()[2]
    lights = api.SoftLightList.make([(api.Light.DIRECTIONAL, (0, 0, 1)), (api.Light.DIRECTIONAL, (0, 0, 1), 4, 0, 0.01)], TABLE)
    want = api.soft_light_list_distance(packed, k, lights, pos, W, H)
    assert (want[1] == 0).all() and (np.abs(want[0][0] - near) < 1e-3).all() and (np.abs(want[0][1] - near) < 0.03).all()

    class F:
        pass
    fr = F()
    fr.k, fr.W, fr.H = k, W, H
    ctx.set_bvh(packed)
    dev = _Dev(ctx, pos, W, H)
    try:
        _form(ctx, kernel, split)
        _trace(ctx, dev, fr, lights, want, (kernel, split, "far before near"))
        assert ctx.last_kernel_name() == _name(kernel, split)
    finally:
        _reset(ctx)
        dev.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx):
    fr = distance_frame(64, 48)
    good = make_list("mixed")
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        counters = [ctx.get_option(k) for k in (COUNTER,) + OTHERS]
        dev.guard()
        out_d, out_c = np.full((8, fr.H, fr.W), DIST_GUARD, np.uint32).view(np.float32), np.full((8, fr.H, fr.W), GUARD, np.uint8)
        for bad in bad_lists(good):
            with pytest.raises(api.RtsError) as e:
                ctx.trace_soft_light_list_distance_device(fr.k, bad, dev.d_pos, fr.W, fr.H, dev.d_dist, dev.d_counts)
            assert e.value.status == 1
            with pytest.raises(api.RtsError):
                ctx.trace_soft_light_list_distance_stripes_device(fr.k, bad, dev.d_pos, fr.W, fr.H, dev.d_dist, 16, 2, 0, d_counts=dev.d_counts)
            with pytest.raises(api.RtsError):
                ctx.trace_soft_light_list_distance(fr.k, bad, fr.pos, fr.W, fr.H, out=out_d, counts=out_c)
        with pytest.raises(api.RtsError):
            ctx.trace_soft_light_list_distance_device(fr.k, good, dev.d_pos, fr.W, fr.H, dev.d_dist, dev.d_counts, row_begin=9, row_end=8)
        with pytest.raises(api.RtsError):
            ctx.trace_soft_light_list_distance_device(fr.k, good, dev.d_pos, fr.W, fr.H, dev.d_dist, dev.d_counts, row_end=fr.H + 1)
        with pytest.raises(api.RtsError):                # distances NULL
            ctx.trace_soft_light_list_distance_device(fr.k, good, dev.d_pos, fr.W, fr.H, 0, dev.d_counts)
        with pytest.raises(api.RtsError):
            ctx.trace_soft_light_list_distance_stripes_device(fr.k, good, dev.d_pos, fr.W, fr.H, 0, 16, 2, 0, d_counts=dev.d_counts)
        assert api._lib.rts_trace_soft_light_list_distance(ctx._h, C.byref(fr.k), C.byref(good), api._ptr(fr.pos), None, fr.W, fr.H, 0, fr.H,
                                                           None, api._ptr(out_c)) == 1
        with pytest.raises(api.RtsError):                # no multiple of 8
            ctx.trace_soft_light_list_distance_stripes_device(fr.k, good, dev.d_pos, fr.W, fr.H, dev.d_dist, 12, 2, 0, d_counts=dev.d_counts)
        ctx.set_option("kernel", 7)                      # a band of 8 under the lane walk, as the soft light list refuses it
        with pytest.raises(api.RtsError):
            ctx.trace_soft_light_list_distance_stripes_device(fr.k, good, dev.d_pos, fr.W, fr.H, dev.d_dist, 8, 2, 0, d_counts=dev.d_counts)
        ctx.set_option("kernel", -1)
        d, c = dev.read()
        assert (d == DIST_GUARD).all() and (c == GUARD).all() and (bits(out_d) == DIST_GUARD).all() and (out_c == GUARD).all()
        assert [ctx.get_option(k) for k in (COUNTER,) + OTHERS] == counters
        good.reserved_[0], good.reserved_[2], good.lights[1].reserved_ = 0xFFFFFFFF, 77, 0xFFFFFFFF   # ignored
        _trace(ctx, dev, fr, good, fr.want("mixed"), "reserved_")
    finally:
        _reset(ctx)
        dev.close()


def test_no_bvh_before_a_stream_is_installed():
    fr = distance_frame(64, 48)
    n = 8 * fr.W * fr.H
    with api.ShadowContext(0) as fresh:
        d_pos, d_dist, d_counts = fresh.malloc(fr.pos.nbytes), fresh.malloc(n * 4), fresh.malloc(n)
        try:
            fresh.h2d(d_dist, np.full(n, DIST_GUARD, np.uint32))
            fresh.h2d(d_counts, np.full(n, GUARD, np.uint8))
            with pytest.raises(api.RtsError) as e:
                fresh.trace_soft_light_list_distance_device(fr.k, make_list("3pairs"), d_pos, fr.W, fr.H, d_dist, d_counts)
            assert e.value.status == 4                   # RTS_ERR_NO_BVH
            with pytest.raises(api.RtsError) as e:
                fresh.trace_soft_light_list_distance(fr.k, make_list("3pairs"), fr.pos, fr.W, fr.H)
            assert e.value.status == 4
            got_d, got_c = np.empty(n, np.uint32), np.empty(n, np.uint8)
            fresh.synchronize()
            fresh.d2h(got_d, d_dist)
            fresh.d2h(got_c, d_counts)
            assert (got_d == DIST_GUARD).all() and (got_c == GUARD).all() and fresh.get_option(COUNTER) == 0
        finally:
            for d in (d_pos, d_dist, d_counts):
                fresh.free(d)


# ---- 10. the smallest stream ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", FORMS)
def test_one_triangle_stream(ctx, kernel, split):
    """The root is the leaf.  A 21 x 13 grid of points on the plane z = 0 under a triangle at z = 1: lights above the triangle see
    part of the grid shadowed (the soft ones with a penumbra), a light below it sees all of it."""
    v = np.array([[0, 0, 1], [2, 0, 1], [0, 2, 1]], np.float32)
    packed = api.BVHBuilder().build(v, 3, np.arange(3, dtype=np.uint32), 1).m_packedNodes
    W, H = 21, 13
    pos = np.zeros((H, W, 4), np.float32)
    y, x = np.mgrid[0:H, 0:W]
    pos[..., 0], pos[..., 1], pos[..., 3] = x * 0.15 - 0.5, y * 0.2 - 0.5, 1.0
    k = api.RayTracingConstants.make((0, 0, 0), (0, 0, 1), W, H)
    lights = api.SoftLightList.make([(api.Light.POINT, (0.5, 0.5, 3.0), 7, 41, 0.6), (api.Light.DIRECTIONAL, (0.0, 0.0, 1.0), 5, 0, 0.3),
                                     (api.Light.POINT, (0.5, 0.5, 0.5), 4, 9, 0.2), (api.Light.POINT, (0.5, 0.5, 3.0))], TABLE)
    want = api.soft_light_list_distance(packed, k, lights, pos, W, H)
    wd, wc = want
    for l, n in ((0, 7), (1, 5)):
        assert (wc[l] == 0).any() and (wc[l] == n).any() and ((wc[l] > 0) & (wc[l] < n)).any(), l
        assert np.array_equal(bits(wd[l]) == INF_BITS, wc[l] == n) and np.isfinite(wd[l]).any()
    assert (wc[2] == 4).all() and (bits(wd[2]) == INF_BITS).all() and 0 < int(wc[3].sum()) < W * H
    m = ((x + 2 * y) & 15).astype(np.uint8)

    class F:
        pass
    fr = F()
    fr.k, fr.W, fr.H = k, W, H
    ctx.set_bvh(packed)
    dev = _Dev(ctx, pos, W, H)
    try:
        _form(ctx, kernel, split)
        _trace(ctx, dev, fr, lights, want, (kernel, split, "one triangle"))
        _trace(ctx, dev, fr, lights, want, (kernel, split, "one triangle", "map"), lights_map=m)
        assert ctx.last_kernel_name() == _name(kernel, split)
    finally:
        _reset(ctx)
        dev.close()
