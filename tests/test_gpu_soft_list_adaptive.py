"""GPU: adaptive soft light list traces (rts_trace_soft_light_list_adaptive*; include/rts.h) against the host twin
(rtsh_soft_light_list_adaptive, which tests/test_soft_list_adaptive_host.py pins to the oracle), byte for byte in the count planes and
in the refined plane, on guard-filled buffers of 8 * W * H and W * H bytes: every case in the three forms -- lane per ray, the packet
with four waves per tile, with one --, light maps (the facing map made on the device, poisoned unmarked pixels, empty tiles and
blocks, a light with no pixel or a single one), row ranges and stripes, options that may only change speed, installed state that must
stay, the counters and kernel names, the device's own soft list and one-light adaptive traces, graph capture, the refusals, and the
smallest stream.  Planes at or above the count must keep the guard."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
from raytracedshadows_amd import api, workloads
from soft_list_adaptive_cases import CASES, FORMS, FRAMES, TABLE, adaptive_list_frame, case_id, make_list, under
from test_soft_light_list_host import bad_lists
from test_soft_list_adaptive_host import bad_probes

pytestmark = pytest.mark.gpu

GUARD = 0xAB
SHARE = "shadowSoftLightListAdaptiveShareKernel"
POISON = np.array([np.nan, np.inf, 1e38, -np.inf], np.float32)
COUNTER = "soft_list_adaptive_traces"
OTHERS = ("active_traces", "distance_traces", "soft_distance_traces", "light_list_traces", "adaptive_traces", "soft_light_list_traces")
MIXED = ("mixed", (0, 2, 2, 0, 2))
OVERLAP = ("overlap", (3, 4, 2))


def _name(kernel, split, geom="rows"):
    return SHARE if kernel in (0, 1, 2, 7) else "shadowSoftLightListAdaptivePacketKernel<%d,%s>" % (4 if split else 1, geom)


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
    """Positions, a map, 8 planes of counts and the refined plane on the device."""

    def __init__(self, ctx, positions, W, H):
        self.ctx, self.W, self.H = ctx, W, H
        positions = np.ascontiguousarray(positions, np.float32)
        self.d_pos, self.d_map, self.d_counts, self.d_ref = ctx.malloc(positions.nbytes), ctx.malloc(W * H), ctx.malloc(8 * W * H), ctx.malloc(W * H)
        ctx.h2d(self.d_pos, positions)

    def guard(self):
        self.ctx.h2d(self.d_counts, np.full(8 * self.W * self.H, GUARD, np.uint8))
        self.ctx.h2d(self.d_ref, np.full(self.W * self.H, GUARD, np.uint8))

    def read(self, stream=None, what=None):
        """(counts[8, H, W], refined[H, W]), or the one plane at `what`."""
        self.ctx.synchronize(stream)
        if what is not None:
            m = np.empty((self.H, self.W), np.uint8)
            self.ctx.d2h(m, what)
            return m
        c, r = np.empty((8, self.H, self.W), np.uint8), np.empty((self.H, self.W), np.uint8)
        self.ctx.d2h(c, self.d_counts)
        self.ctx.d2h(r, self.d_ref)
        return c, r

    def close(self):
        for d in (self.d_pos, self.d_map, self.d_counts, self.d_ref):
            self.ctx.free(d)


def _expect(want, lights_map=None, rows=None):
    """(all 8 planes, refined): the twin's bytes under the map's bits in the rows, the guard in the other rows and in the planes from the
    count up."""
    c, r = want if lights_map is None else under(want[0], want[1], lights_map)
    out = np.full((8,) + c.shape[1:], GUARD, np.uint8)
    for l in range(c.shape[0]):
        out[l] = c[l] if rows is None else np.where(rows[:, None], c[l], GUARD)
    return out, (r if rows is None else np.where(rows[:, None], r, GUARD).astype(np.uint8))


def _same(got, want, what):
    if isinstance(got, tuple):
        _same(got[0], want[0], (what, "counts"))
        _same(got[1], want[1], (what, "refined"))
        return
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:4].tolist(), [got[tuple(b)] for b in bad[:4]], [want[tuple(b)] for b in bad[:4]])


def _trace(ctx, dev, fr, lights, probes, want, what, lights_map=None, rows=None, refined=True, **kw):
    if lights_map is not None:
        ctx.h2d(dev.d_map, np.ascontiguousarray(lights_map, np.uint8))
    dev.guard()
    ctx.trace_soft_light_list_adaptive_device(fr.k, lights, probes, dev.d_pos, fr.W, fr.H, dev.d_counts,
                                              d_refined=dev.d_ref if refined else None,
                                              d_lights_map=dev.d_map if lights_map is not None else None, **kw)
    c, r = _expect(want, lights_map, rows)
    _same(dev.read(), (c, r if refined else np.full_like(r, GUARD)), what)


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("name,probes", CASES, ids=case_id)
def test_every_case_in_the_three_forms_equals_the_twin(ctx, name, probes, W, H):
    fr = adaptive_list_frame(W, H)
    lights, want = make_list(name), fr.want(name, probes)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, W, H)
    try:
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            _trace(ctx, dev, fr, lights, probes, want, (name, probes, kernel, split))
            assert ctx.last_kernel_name() == _name(kernel, split), (kernel, split, ctx.last_kernel_name())
            _trace(ctx, dev, fr, lights, probes, want, (name, probes, kernel, split, "refined NULL"), refined=False)
        # the host form: its rows alone travel, and come back to planes of H rows
        out, ref = np.full((8, H, W), GUARD, np.uint8), np.full((H, W), GUARD, np.uint8)
        ctx.trace_soft_light_list_adaptive(fr.k, lights, probes, fr.pos, W, H, row_begin=3, row_end=30, out=out, refined=ref)
        rows = (np.arange(H) >= 3) & (np.arange(H) < 30)
        _same((out, ref), _expect(want, None, rows), (name, probes, "host rows"))
    finally:
        _reset(ctx)
        dev.close()


def test_auto_takes_the_lane_walk_below_256k_pixels(ctx):
    fr = adaptive_list_frame(61, 37)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        assert ctx.get_option("kernel") == -1
        _trace(ctx, dev, fr, make_list("3pairs"), (0, 1), fr.want("3pairs", (0, 1)), "defaults")
        assert ctx.last_kernel_name() == SHARE
    finally:
        dev.close()


# ---- 2. the map -----------------------------------------------------------------------------------------------------------------
def _maps(fr, count):
    y, x = np.mgrid[0:fr.H, 0:fr.W]
    below = (1 << count) - 1
    mixed = ((x * 7 + y * 13 + (x >> 3) * 5) & 0xFF).astype(np.uint8)
    mixed[(x + y) % 5 == 0] = 0
    holes = np.full((fr.H, fr.W), 0xFF, np.uint8)
    holes[8:16, 16:24] = 0                               # an 8 x 8 tile
    holes[16:32, 32:48] = 0                              # a 16 x 16 block
    holes[0:8, 0:8] = 0xFF & ~below                      # a tile whose bytes have bits, but none below the count
    absent = np.full((fr.H, fr.W), 0xFF, np.uint8) & ~np.uint8(1 << (count - 1))     # the last light has no pixel anywhere
    single = absent.copy()
    single[21, 34] |= 1 << (count - 1)                   # ... or a single one, in the middle of its tile
    lone = np.zeros((fr.H, fr.W), np.uint8)
    lone[21, 34] = 1                                     # one pixel of one light in the whole frame: every other lane stands in
    return {"mixed": mixed, "holes": holes, "absent": absent, "single": single, "lone": lone, "full": np.full((fr.H, fr.W), 0xFF, np.uint8),
            "zeros": np.zeros((fr.H, fr.W), np.uint8)}


@pytest.mark.parametrize("kernel,split", FORMS)
@pytest.mark.parametrize("name,probes", [OVERLAP, ("8x2", (1,) * 8)], ids=case_id)
def test_light_maps(ctx, name, probes, kernel, split):
    fr = adaptive_list_frame(64, 48)
    lights, want = make_list(name), fr.want(name, probes)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    below = (1 << lights.count) - 1
    try:
        _form(ctx, kernel, split)
        for what, m in _maps(fr, lights.count).items():
            dirty = fr.pos.copy()                        # a pixel no light is marked for may hold anything
            dirty[(m & below) == 0] = POISON
            ctx.h2d(dev.d_pos, dirty)
            _trace(ctx, dev, fr, lights, probes, want, (name, kernel, split, what), lights_map=m)
            got = dev.read()
            if what == "full":                           # NULL equals a map of 0xFF
                _trace(ctx, dev, fr, lights, probes, want, (name, kernel, split, "NULL"))
                _same(dev.read(), got, "NULL against 0xFF")
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("W,H", FRAMES)
def test_the_facing_map_made_on_the_device(ctx, W, H):
    fr = adaptive_list_frame(W, H)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, W, H)
    d_nrm = ctx.malloc(fr.nrm.nbytes)
    try:
        ctx.h2d(d_nrm, fr.nrm)
        for name, probes in (MIXED, ("8x2", (1,) * 8)):
            lights, host_map = make_list(name), fr.facing(name)
            ctx.h2d(dev.d_map, np.full(W * H, GUARD, np.uint8))
            api.facing_lights_device(ctx, fr.k, lights.hard_list(), dev.d_pos, d_nrm, W, H, dev.d_map)
            _same(dev.read(what=dev.d_map), host_map, (name, "device map against host map"))
            assert 0 < int((host_map != 0).sum()) < host_map.size
            for kernel, split in FORMS:
                _form(ctx, kernel, split)
                dev.guard()
                ctx.trace_soft_light_list_adaptive_device(fr.k, lights, probes, dev.d_pos, W, H, dev.d_counts, d_refined=dev.d_ref,
                                                          d_lights_map=dev.d_map)
                _same(dev.read(), _expect(fr.want(name, probes), host_map), (name, kernel, split, "facing"))
    finally:
        _reset(ctx)
        ctx.free(d_nrm)
        dev.close()


# ---- 3. geometry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", FORMS)
def test_row_ranges_leave_the_other_rows(ctx, kernel, split):
    fr = adaptive_list_frame(64, 48)
    (name, probes), lights = MIXED, make_list("mixed")
    want = fr.want(name, probes)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    m = _maps(fr, 5)["mixed"]
    try:
        _form(ctx, kernel, split)
        for b, e in ((8, 40), (16, 32), (5, 41)):
            rows = (np.arange(fr.H) >= b) & (np.arange(fr.H) < e)
            _trace(ctx, dev, fr, lights, probes, want, (kernel, split, b, e), rows=rows, row_begin=b, row_end=e)
            _trace(ctx, dev, fr, lights, probes, want, (kernel, split, b, e, "map"), lights_map=m, rows=rows, row_begin=b, row_end=e)
        n0 = ctx.get_option(COUNTER)
        _trace(ctx, dev, fr, lights, probes, want, "empty range", rows=np.zeros(fr.H, bool), row_begin=7, row_end=7)
        assert ctx.get_option(COUNTER) == n0
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel,split", FORMS)
def test_host_form_with_a_light_map_and_a_row_range(ctx, kernel, split):
    """The host-pointer form with a per-pixel map AND a row range: rows [3, 30) of the positions and of the map travel through the
    staging buffers as a frame of their own; the refined rows come back beside the planes."""
    fr = adaptive_list_frame(61, 37)
    (name, probes), lights = OVERLAP, make_list("overlap")
    m = _maps(fr, lights.count)["mixed"]
    rows = (np.arange(fr.H) >= 3) & (np.arange(fr.H) < 30)
    ctx.set_bvh(fr.packed)
    try:
        _form(ctx, kernel, split)
        out, ref = np.full((8, fr.H, fr.W), GUARD, np.uint8), np.full((fr.H, fr.W), GUARD, np.uint8)
        got = ctx.trace_soft_light_list_adaptive(fr.k, lights, probes, fr.pos, fr.W, fr.H, lights_map=m, row_begin=3, row_end=30, out=out,
                                                 refined=ref)
        assert got[0] is out and got[1] is ref
        assert ctx.last_kernel_name() == _name(kernel, split), ctx.last_kernel_name()
        _same((out, ref), _expect(fr.want(name, probes), m, rows), (kernel, split, "host rows with a map"))
        out[:] = GUARD                                   # ... and without the refined plane
        only, none = ctx.trace_soft_light_list_adaptive(fr.k, lights, probes, fr.pos, fr.W, fr.H, lights_map=m, row_begin=3, row_end=30,
                                                        out=out, want_refined=False)
        assert none is None
        _same(only, _expect(fr.want(name, probes), m, rows)[0], (kernel, split, "host rows, refined NULL"))
    finally:
        _reset(ctx)


@pytest.mark.parametrize("kernel,split,band", [(3, 1, 8), (3, 1, 16), (3, 0, 8), (3, 0, 16), (7, 1, 16)])
def test_stripes(ctx, kernel, split, band):
    fr = adaptive_list_frame(61, 37)
    (name, probes), lights = MIXED, make_list("mixed")
    want = fr.want(name, probes)
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
                ctx.trace_soft_light_list_adaptive_stripes_device(fr.k, lights, probes, dev.d_pos, fr.W, fr.H, dev.d_counts, band, 3, stripe,
                                                                  d_refined=dev.d_ref, d_lights_map=dev.d_map if with_map else None)
                _same(dev.read(), _expect(want, m if with_map else None, rows), (kernel, split, band, with_map, stripe))
                assert ctx.last_kernel_name() == _name(kernel, split, "bands"), ctx.last_kernel_name()
        # a stripe that owns no band launches nothing, writes nothing and returns OK (37 rows in bands of 16: bands 0..2, stripe 3 of 4)
        n0 = ctx.get_option(COUNTER)
        dev.guard()
        ctx.trace_soft_light_list_adaptive_stripes_device(fr.k, lights, probes, dev.d_pos, fr.W, fr.H, dev.d_counts, 16, 4, 3, d_refined=dev.d_ref)
        c, r = dev.read()
        assert (c == GUARD).all() and (r == GUARD).all() and ctx.get_option(COUNTER) == n0
        if kernel == 3:                                  # 24 rows: not a power of two -- the general form
            rows = ((np.arange(fr.H) // 24) % 2) == 1
            dev.guard()
            ctx.trace_soft_light_list_adaptive_stripes_device(fr.k, lights, probes, dev.d_pos, fr.W, fr.H, dev.d_counts, 24, 2, 1,
                                                              d_refined=dev.d_ref)
            _same(dev.read(), _expect(want, None, rows), (kernel, split, 24))
            assert ctx.last_kernel_name() == _name(kernel, split, "general")
    finally:
        _reset(ctx)
        dev.close()


def test_a_band_of_8_under_the_lane_walk_is_refused_as_the_soft_light_list_refuses_it(ctx):
    fr = adaptive_list_frame(61, 37)
    lights = make_list("3pairs")
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        ctx.set_option("kernel", 7)
        with pytest.raises(api.RtsError) as full:
            ctx.trace_soft_light_list_stripes_device(fr.k, lights, dev.d_pos, fr.W, fr.H, dev.d_counts, 8, 2, 0)
        dev.guard()
        n0 = ctx.get_option(COUNTER)
        with pytest.raises(api.RtsError) as mine:
            ctx.trace_soft_light_list_adaptive_stripes_device(fr.k, lights, (0, 1), dev.d_pos, fr.W, fr.H, dev.d_counts, 8, 2, 0,
                                                              d_refined=dev.d_ref)
        assert mine.value.status == full.value.status == 1
        c, r = dev.read()
        assert (c == GUARD).all() and (r == GUARD).all() and ctx.get_option(COUNTER) == n0
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel,split", FORMS)
def test_the_general_grid_and_the_row_orders(ctx, kernel, split):
    fr = adaptive_list_frame(61, 37)
    (name, probes), lights = OVERLAP, make_list("overlap")
    want = fr.want(name, probes)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    m = _maps(fr, 3)["mixed"]
    try:
        _form(ctx, kernel, split)
        ctx.set_option("xcd_swizzle", 1)
        _trace(ctx, dev, fr, lights, probes, want, (kernel, split, "swizzle"), lights_map=m)
        assert ctx.last_kernel_name() == _name(kernel, split, "general")
        rows = (np.arange(fr.H) >= 5) & (np.arange(fr.H) < 30)
        _trace(ctx, dev, fr, lights, probes, want, (kernel, split, "swizzle rows"), rows=rows, row_begin=5, row_end=30)
        ctx.set_option("xcd_swizzle", 0)
        for order in (1, 2):
            ctx.set_option("row_order", order)
            _trace(ctx, dev, fr, lights, probes, want, (kernel, split, "row_order", order), lights_map=m)
            assert ctx.last_kernel_name() == _name(kernel, split, "rows")
    finally:
        _reset(ctx)
        dev.close()


# ---- 4. options change no byte --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [1, 0])
def test_options_change_no_byte(ctx, split):
    fr = adaptive_list_frame(64, 48)
    (name, probes), lights = MIXED, make_list("mixed")
    want = fr.want(name, probes)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    before = (ctx.get_option("packet_budget"), ctx.get_option("packet_share"))
    m = _maps(fr, 5)["mixed"]
    try:
        ctx.set_option("soft_split", split)
        ctx.set_option("kernel", 3)
        ctx.set_option("packet_budget", 1)               # every packet dissolves at once
        ctx.set_option("packet_share", 16)
        _trace(ctx, dev, fr, lights, probes, want, ("dissolve", split))
        _trace(ctx, dev, fr, lights, probes, want, ("dissolve", split, "map"), lights_map=m)
        ctx.set_option("packet_budget", before[0])
        ctx.set_option("packet_share", before[1])
        ctx.set_option("kernel", 8)                      # the stream has a private copy; this trace runs the stackless packet all the same
        assert ctx.get_option("wide_nodes") > 0
        _trace(ctx, dev, fr, lights, probes, want, ("kernel 8", split), lights_map=m)
        assert ctx.last_kernel_name() == _name(3, split)
        ctx.set_option("kernel", 9)
        _trace(ctx, dev, fr, lights, probes, want, ("kernel 9", split))
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
    probes = (0, 2)
    want = api.soft_light_list_adaptive(wl.packed, wl.constants, lights, probes, wl.positions, W, H)
    plain = want[0][0]                                   # light 0 is the workload's own, in full: the plain trace's byte
    assert 0 < int(plain.sum()) < plain.size
    ctx.set_bvh(wl.packed)
    dev = _Dev(ctx, wl.positions, W, H)

    def list_trace():
        n0 = ctx.get_option(COUNTER)
        dev.guard()
        ctx.trace_soft_light_list_adaptive_device(wl.constants, lights, probes, dev.d_pos, W, H, dev.d_counts, d_refined=dev.d_ref)
        _same(dev.read(), _expect(want), "list")
        assert ctx.get_option(COUNTER) == n0 + 1 and ctx.last_kernel_name() == _name(3, 1)

    def plain_trace():
        dev.guard()
        ctx.trace_shadow_mask_device(wl.constants, dev.d_pos, W, H, dev.d_counts, light=wl.light)
        _same(dev.read()[0][0], plain, "plain")
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
    fr = adaptive_list_frame(64, 48)
    (name, probes), lights = OVERLAP, make_list("overlap")
    want = fr.want(name, probes)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        before = [ctx.get_option(k) for k in OTHERS]
        n0 = ctx.get_option(COUNTER)
        launches = 0
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            _trace(ctx, dev, fr, lights, probes, want, (kernel, split))
            assert ctx.last_kernel_name() == _name(kernel, split, "rows")
            ctx.trace_soft_light_list_adaptive_stripes_device(fr.k, lights, probes, dev.d_pos, fr.W, fr.H, dev.d_counts, 16, 2, 1)
            assert ctx.last_kernel_name() == _name(kernel, split, "bands")
            ctx.set_option("xcd_swizzle", 1)
            ctx.trace_soft_light_list_adaptive_device(fr.k, lights, probes, dev.d_pos, fr.W, fr.H, dev.d_counts)
            assert ctx.last_kernel_name() == _name(kernel, split, "general")
            ctx.set_option("xcd_swizzle", 0)
            launches += 3
        ctx.trace_soft_light_list_adaptive(fr.k, lights, probes, fr.pos, fr.W, fr.H)
        ctx.synchronize()
        assert ctx.get_option(COUNTER) == n0 + launches + 1
        assert [ctx.get_option(k) for k in OTHERS] == before
        with pytest.raises(api.RtsError):                # read-only
            ctx.set_option(COUNTER, 0)
        # ... and neither the soft list nor the one-light adaptive trace moves it
        n1 = ctx.get_option(COUNTER)
        ctx.trace_soft_light_list_device(fr.k, lights, dev.d_pos, fr.W, fr.H, dev.d_counts)
        ctx.trace_shadow_mask_adaptive_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_counts, lights.light(0), 3)
        ctx.synchronize()
        assert ctx.get_option(COUNTER) == n1
        assert ctx.get_option("soft_light_list_traces") == before[5] + 1 and ctx.get_option("adaptive_traces") == before[4] + 1
    finally:
        _reset(ctx)
        dev.close()


# ---- 7. pins on the device's own results ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", FORMS)
def test_all_probes_zero_is_the_soft_light_list_on_the_device(ctx, kernel, split):
    fr = adaptive_list_frame(61, 37)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    d_full = ctx.malloc(8 * fr.W * fr.H)
    try:
        _form(ctx, kernel, split)
        for name in ("mixed", "overlap", "48"):
            lights = make_list(name)
            m = _maps(fr, lights.count)["mixed"]
            ctx.h2d(dev.d_map, m)
            for d_map in (None, dev.d_map):
                dev.guard()
                ctx.h2d(d_full, np.full(8 * fr.W * fr.H, GUARD, np.uint8))
                ctx.trace_soft_light_list_adaptive_device(fr.k, lights, (0,) * lights.count, dev.d_pos, fr.W, fr.H, dev.d_counts,
                                                          d_refined=dev.d_ref, d_lights_map=d_map)
                ctx.trace_soft_light_list_device(fr.k, lights, dev.d_pos, fr.W, fr.H, d_full, d_lights_map=d_map)
                c, r = dev.read()
                full = np.empty((8, fr.H, fr.W), np.uint8)
                ctx.d2h(full, d_full)
                _same(c, full, (name, kernel, split, d_map is not None))
                assert not r.any(), (name, kernel, split)
    finally:
        _reset(ctx)
        ctx.free(d_full)
        dev.close()


@pytest.mark.parametrize("kernel,split", FORMS)
@pytest.mark.parametrize("name,probes", [OVERLAP, MIXED], ids=case_id)
def test_plane_l_is_the_adaptive_trace_of_light_l(ctx, name, probes, kernel, split):
    """The definition on the device itself: plane l and bit l of refined = rts_trace_shadow_mask_adaptive for the derived light l with
    probe k_l and the map's bit l as its active byte."""
    fr = adaptive_list_frame(61, 37)
    lights = make_list(name)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    d_one, d_took, d_act = ctx.malloc(fr.W * fr.H), ctx.malloc(fr.W * fr.H), ctx.malloc(fr.W * fr.H)
    m = _maps(fr, lights.count)["mixed"]
    try:
        _form(ctx, kernel, split)
        _trace(ctx, dev, fr, lights, probes, fr.want(name, probes), "list", lights_map=m)
        c, r = dev.read()
        checked = 0
        for l in range(lights.count):
            if probes[l] == 0:
                continue
            ctx.h2d(d_act, np.ascontiguousarray((m >> l) & 1, np.uint8))
            ctx.h2d(d_one, np.full(fr.W * fr.H, GUARD, np.uint8))
            ctx.h2d(d_took, np.full(fr.W * fr.H, GUARD, np.uint8))
            ctx.trace_shadow_mask_adaptive_device(fr.k, dev.d_pos, fr.W, fr.H, d_one, lights.light(l), probes[l], d_refined=d_took,
                                                  d_active=d_act)
            _same(c[l], dev.read(what=d_one), ("light", l))
            _same((r >> l) & 1, dev.read(what=d_took), ("light", l, "refined"))
            checked += 1
        assert checked >= 3
    finally:
        _reset(ctx)
        for d in (d_one, d_took, d_act):
            ctx.free(d)
        dev.close()


@pytest.mark.parametrize("name,probes", [MIXED, ("48", (3,)), ("shared16", (4, 3, 4))], ids=case_id)
def test_the_two_splits_agree_byte_for_byte(ctx, name, probes):
    fr = adaptive_list_frame(64, 48)
    lights = make_list(name)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    m = _maps(fr, lights.count)["mixed"]
    try:
        got = []
        for split in (1, 0):
            _form(ctx, 3, split)
            ctx.h2d(dev.d_map, m)
            dev.guard()
            ctx.trace_soft_light_list_adaptive_device(fr.k, lights, probes, dev.d_pos, fr.W, fr.H, dev.d_counts, d_refined=dev.d_ref,
                                                      d_lights_map=dev.d_map)
            got.append(dev.read())
        _same(got[0], got[1], (name, "four waves against one"))
    finally:
        _reset(ctx)
        dev.close()


# ---- 8. graph capture -----------------------------------------------------------------------------------------------------------
def _copy(struct):
    return type(struct).from_buffer_copy(struct)


@pytest.mark.parametrize("form", ["whole", "rows", "stripe"])
@pytest.mark.parametrize("kernel,split", FORMS)
def test_device_forms_under_capture(ctx, kernel, split, form):
    fr = adaptive_list_frame(64, 48)
    name, probes = MIXED
    want = fr.want(name, probes)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    maps = _maps(fr, 5)
    stream = ctx.stream_create()
    k, lights = _copy(fr.k), make_list("mixed")
    pr = (C.c_uint32 * 5)(*probes)                       # the caller's own array: read by value at the call
    lib, kp, lp = api._lib, C.byref(k), C.byref(lights)
    g = None
    try:
        _form(ctx, kernel, split)
        ctx.h2d(dev.d_map, maps["mixed"])
        ctx.trace_shadow_mask_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_counts, light=lights.light(0), stream=stream)   # a stream that has traced
        ctx.synchronize(stream)
        rows = None
        args = (C.c_void_p(dev.d_counts), pr, C.c_void_p(dev.d_ref), C.c_void_p(stream))
        if form == "whole":
            record = lambda: api._check(lib.rts_trace_soft_light_list_adaptive_device(
                ctx._h, kp, lp, C.c_void_p(dev.d_pos), C.c_void_p(dev.d_map), fr.W, fr.H, 0, fr.H, *args), "capture")
        elif form == "rows":
            rows = (np.arange(fr.H) >= 5) & (np.arange(fr.H) < 41)
            record = lambda: api._check(lib.rts_trace_soft_light_list_adaptive_device(
                ctx._h, kp, lp, C.c_void_p(dev.d_pos), C.c_void_p(dev.d_map), fr.W, fr.H, 5, 41, *args), "capture")
        else:
            rows = ((np.arange(fr.H) // 16) % 2) == 1
            record = lambda: api._check(lib.rts_trace_soft_light_list_adaptive_stripes_device(
                ctx._h, kp, lp, C.c_void_p(dev.d_pos), C.c_void_p(dev.d_map), fr.W, fr.H, 16, 2, 1, *args), "capture")
        n0 = ctx.get_option(COUNTER)
        g = hipgraph.capture(stream, record)
        assert ctx.get_option(COUNTER) == n0 + 1
        types = g.node_types()
        assert types == [hipgraph.KERNEL], (kernel, split, form, types)   # one kernel node; no memcpy, memset or allocation node
        for s in (k, lights, pr):                        # what a caller may do to its structs and its probes between capture and replay
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


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx):
    fr = adaptive_list_frame(64, 48)
    good, probes = make_list("mixed"), MIXED[1]
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        counters = [ctx.get_option(k) for k in (COUNTER,) + OTHERS]
        dev.guard()
        out, ref = np.full((8, fr.H, fr.W), GUARD, np.uint8), np.full((fr.H, fr.W), GUARD, np.uint8)
        # (a refused list with one probe of 0 per light it claims, so that the list is what is refused; then good lists with bad probes)
        cases = [(bad, (0,) * (bad.count if bad is not None else 8)) for bad in bad_lists(good)] + bad_probes(good)
        for bad, pr in cases:
            with pytest.raises(api.RtsError) as e:
                ctx.trace_soft_light_list_adaptive_device(fr.k, bad, pr, dev.d_pos, fr.W, fr.H, dev.d_counts, d_refined=dev.d_ref)
            assert e.value.status == 1
            with pytest.raises(api.RtsError):
                ctx.trace_soft_light_list_adaptive_stripes_device(fr.k, bad, pr, dev.d_pos, fr.W, fr.H, dev.d_counts, 16, 2, 0, d_refined=dev.d_ref)
            with pytest.raises(api.RtsError):
                ctx.trace_soft_light_list_adaptive(fr.k, bad, pr, fr.pos, fr.W, fr.H, out=out, refined=ref)
        with pytest.raises(api.RtsError):
            ctx.trace_soft_light_list_adaptive_device(fr.k, good, probes, dev.d_pos, fr.W, fr.H, dev.d_counts, d_refined=dev.d_ref, row_begin=9, row_end=8)
        with pytest.raises(api.RtsError):
            ctx.trace_soft_light_list_adaptive_device(fr.k, good, probes, dev.d_pos, fr.W, fr.H, dev.d_counts, d_refined=dev.d_ref, row_end=fr.H + 1)
        with pytest.raises(api.RtsError):
            ctx.trace_soft_light_list_adaptive_device(fr.k, good, probes, dev.d_pos, fr.W, fr.H, 0, d_refined=dev.d_ref)
        with pytest.raises(api.RtsError):
            ctx.trace_soft_light_list_adaptive_stripes_device(fr.k, good, probes, dev.d_pos, fr.W, fr.H, dev.d_counts, 12, 2, 0,
                                                              d_refined=dev.d_ref)                       # no multiple of 8
        c, r = dev.read()
        assert (c == GUARD).all() and (r == GUARD).all() and (out == GUARD).all() and (ref == GUARD).all()
        assert [ctx.get_option(k) for k in (COUNTER,) + OTHERS] == counters
        good.reserved_[0], good.reserved_[2], good.lights[1].reserved_ = 0xFFFFFFFF, 77, 0xFFFFFFFF   # ignored
        _trace(ctx, dev, fr, good, probes, fr.want(*MIXED), "reserved_")
    finally:
        dev.close()


def test_no_bvh_before_a_stream_is_installed():
    fr = adaptive_list_frame(64, 48)
    with api.ShadowContext(0) as fresh:
        d_pos, d_counts = fresh.malloc(fr.pos.nbytes), fresh.malloc(9 * fr.W * fr.H)
        try:
            fresh.h2d(d_counts, np.full(9 * fr.W * fr.H, GUARD, np.uint8))
            with pytest.raises(api.RtsError) as e:
                fresh.trace_soft_light_list_adaptive_device(fr.k, make_list("3pairs"), (0, 1), d_pos, fr.W, fr.H, d_counts,
                                                            d_refined=d_counts + 8 * fr.W * fr.H)
            assert e.value.status == 4                   # RTS_ERR_NO_BVH
            with pytest.raises(api.RtsError) as e:
                fresh.trace_soft_light_list_adaptive(fr.k, make_list("3pairs"), (0, 1), fr.pos, fr.W, fr.H)
            assert e.value.status == 4
            got = np.empty(9 * fr.W * fr.H, np.uint8)
            fresh.synchronize()
            fresh.d2h(got, d_counts)
            assert (got == GUARD).all() and fresh.get_option(COUNTER) == 0
        finally:
            fresh.free(d_pos)
            fresh.free(d_counts)


# ---- 10. the smallest stream ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", FORMS)
def test_one_triangle_stream(ctx, kernel, split):
    """The root is the leaf.  The scene of tests/test_gpu_soft_light_list.py's test_one_triangle_stream -- a 21 x 13 grid of points on
    the plane z = 0 under a triangle at z = 1 -- with the probes (3, 2, 2, 0): the two lights above the triangle refine along their
    penumbra, the light below it sees everything and never does, the hard light is traced in full."""
    v = np.array([[0, 0, 1], [2, 0, 1], [0, 2, 1]], np.float32)
    packed = api.BVHBuilder().build(v, 3, np.arange(3, dtype=np.uint32), 1).m_packedNodes
    W, H = 21, 13
    pos = np.zeros((H, W, 4), np.float32)
    y, x = np.mgrid[0:H, 0:W]
    pos[..., 0], pos[..., 1], pos[..., 3] = x * 0.15 - 0.5, y * 0.2 - 0.5, 1.0
    k = api.RayTracingConstants.make((0, 0, 0), (0, 0, 1), W, H)
    lights = api.SoftLightList.make([(api.Light.POINT, (0.5, 0.5, 3.0), 7, 41, 0.6), (api.Light.DIRECTIONAL, (0.0, 0.0, 1.0), 5, 0, 0.3),
                                     (api.Light.POINT, (0.5, 0.5, 0.5), 4, 9, 0.2), (api.Light.POINT, (0.5, 0.5, 3.0))], TABLE)
    probes = (3, 2, 2, 0)
    want = api.soft_light_list_adaptive(packed, k, lights, probes, pos, W, H)
    for l in (0, 1):
        assert ((want[1] >> l) & 1).any(), l             # lights 0 and 1 refine somewhere
    assert (want[0][2] == 4).all() and not ((want[1] >> 2) & 3).any() and 0 < int(want[0][3].sum()) < W * H
    m = ((x + 2 * y) & 15).astype(np.uint8)

    class F:
        pass
    fr = F()
    fr.k, fr.W, fr.H = k, W, H
    ctx.set_bvh(packed)
    dev = _Dev(ctx, pos, W, H)
    try:
        _form(ctx, kernel, split)
        _trace(ctx, dev, fr, lights, probes, want, (kernel, split, "one triangle"))
        _trace(ctx, dev, fr, lights, probes, want, (kernel, split, "one triangle", "map"), lights_map=m)
        assert ctx.last_kernel_name() == _name(kernel, split)
    finally:
        _reset(ctx)
        dev.close()
