"""GPU: the adaptive soft mask (rts_trace_shadow_mask_adaptive*; include/rts.h) against its host twin (rtsh_shadow_mask_adaptive, which
tests/test_adaptive_host.py pins to the oracle), as bytes, on guard-filled mask and refined buffers: every kernel family and split
with its name, (samples, probe) pairs that leave waves of the 4-wave deal without a sample in either phase, per-pixel jitter through
whole frames, row ranges and the host form, active maps with empty and unanimous tiles, the exit between the two barriers, stripes,
the optional refined plane, the counters, options that may only change speed, installed state that must stay, and graph capture."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
from adaptive_cases import (CASES, CASES_K1, DIR_4_OF_16, FRAMES, POINT_5_OF_16, POINT_6, POINT_16_OF_16, adaptive_frame, assert_case,
                            case_id, tiles_8x8)
from raytracedshadows_amd import api, workloads
from soft_distance_cases import RADIUS_FEW

pytestmark = pytest.mark.gpu

GUARD_M = 0xAB
GUARD_R = 0xCD
SHARE = "shadowMaskAdaptiveShareKernel"
POISON = np.array([np.nan, np.inf, 1e38, -np.inf], np.float32)
FORMS = [(7, 1), (7, 0), (3, 1), (3, 0), (8, 1), (8, 0), (-1, 1), (-1, 0)]       # ("kernel", "soft_split"); -1: below 256 K pixels here
FEW_FORMS = [(7, 1), (3, 1), (3, 0)]
COUNTERS = ["active_traces", "distance_traces", "soft_distance_traces", "light_list_traces"]


def _name(kernel, split, geom="rows"):
    return SHARE if kernel in (-1, 0, 1, 2, 7) else "shadowMaskAdaptivePacketKernel<%d,%s>" % (4 if split else 1, geom)


def _reset(ctx):
    for key, v in (("kernel", -1), ("soft_split", 1), ("xcd_swizzle", 0), ("row_order", 0)):
        ctx.set_option(key, v)


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    _reset(c)
    c.close()


class _Dev:
    def __init__(self, ctx, positions, W, H):
        self.ctx, self.W, self.H = ctx, W, H
        positions = np.ascontiguousarray(positions, np.float32)
        self.d_pos, self.d_act, self.d_mask, self.d_ref = ctx.malloc(positions.nbytes), ctx.malloc(W * H), ctx.malloc(W * H), ctx.malloc(W * H)
        ctx.h2d(self.d_pos, positions)

    def guard(self):
        self.ctx.h2d(self.d_mask, np.full(self.W * self.H, GUARD_M, np.uint8))
        self.ctx.h2d(self.d_ref, np.full(self.W * self.H, GUARD_R, np.uint8))

    def read(self, stream=None):
        m, r = np.empty((self.H, self.W), np.uint8), np.empty((self.H, self.W), np.uint8)
        self.ctx.synchronize(stream)
        self.ctx.d2h(m, self.d_mask)
        self.ctx.d2h(r, self.d_ref)
        return m, r

    def close(self):
        for d in (self.d_pos, self.d_act, self.d_mask, self.d_ref):
            self.ctx.free(d)


def _expect(want, active=None, rows=None):
    m, r = want[0], want[1]
    if active is not None:
        m, r = (m * (active != 0)).astype(np.uint8), (r * (active != 0)).astype(np.uint8)
    if rows is not None:
        m, r = np.where(rows[:, None], m, GUARD_M).astype(np.uint8), np.where(rows[:, None], r, GUARD_R).astype(np.uint8)
    return m, r


def _same(got, want, what):
    for g, w, part in ((got[0], want[0], "mask"), (got[1], want[1], "refined")):
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, part, bad.shape[0], bad[:4].tolist(), [g[tuple(b)] for b in bad[:4]], [w[tuple(b)] for b in bad[:4]])


def _trace(ctx, dev, af, light, probe, want, what, active=None, rows=None, **kw):
    if active is not None:
        ctx.h2d(dev.d_act, np.ascontiguousarray(active, np.uint8))
    dev.guard()
    ctx.trace_shadow_mask_adaptive_device(af.k, dev.d_pos, af.W, af.H, dev.d_mask, light, probe, d_refined=dev.d_ref,
                                          d_active=dev.d_act if active is not None else None, **kw)
    _same(dev.read(), _expect(want, active, rows), what)


# ---- 1. parity: every family and split, every (samples, probe) pair ----------------------------------------------------------------
@pytest.mark.parametrize("key,probe", CASES + CASES_K1, ids=case_id)
def test_every_family_and_split_equals_the_twin(ctx, key, probe):
    af = adaptive_frame(61, 37)
    light, want = af.light(key), af.want(key, probe)
    ctx.set_bvh(af.packed)
    dev = _Dev(ctx, af.pos, af.W, af.H)
    try:
        for kernel, split in FORMS:
            ctx.set_option("kernel", kernel)
            ctx.set_option("soft_split", split)
            _trace(ctx, dev, af, light, probe, want, (key, probe, kernel, split))
            assert ctx.last_kernel_name() == _name(kernel, split), (kernel, split, ctx.last_kernel_name())
    finally:
        _reset(ctx)
        dev.close()


def test_both_exits_between_the_barriers_are_taken():
    """Both frames hold, under the flagship light, an 8 x 8 tile whose pixels are all unanimous (the 4-wave form leaves between its
    two barriers) AND a tile that refines (it goes on to the second): checked on the host twin, so the parity tests above and below
    walk both paths."""
    for size in FRAMES:
        af = adaptive_frame(*size)
        for key, probe in ((POINT_16_OF_16, 4), (POINT_5_OF_16, 4)):
            t = tiles_8x8(af.want(key, probe)[1])          # (pad 255: no pixel)
            refines = (t == 1).any(axis=2)
            assert int(refines.sum()) >= 1 and int((~refines).sum()) >= 1, (size, key, int(refines.sum()))


# ---- 2. per-pixel jitter: whole frames, row ranges, the host form ------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", FEW_FORMS)
def test_table_jitter_whole_rows_and_host_form(ctx, kernel, split):
    af = adaptive_frame(64, 48)
    key, probe = POINT_5_OF_16, 4
    light, want = af.light(key), af.want(key, probe)
    assert light.table == 16 and light.nsamples == 5
    ctx.set_bvh(af.packed)
    dev = _Dev(ctx, af.pos, af.W, af.H)
    rows = (np.arange(af.H) >= 8) & (np.arange(af.H) < 24)
    assert_case(want[0][8:24], want[1][8:24], want[2][8:24], 5, "rows 8..24")
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        _trace(ctx, dev, af, light, probe, want, (kernel, split, "whole"))
        _trace(ctx, dev, af, light, probe, want, (kernel, split, "device rows"), rows=rows, row_begin=8, row_end=24)
        assert ctx.last_kernel_name() == _name(kernel, split)
        rows2 = (np.arange(af.H) >= 5) & (np.arange(af.H) < 41)
        _trace(ctx, dev, af, light, probe, want, (kernel, split, "ragged rows"), rows=rows2, row_begin=5, row_end=41)
        n0 = ctx.get_option("adaptive_traces")
        _trace(ctx, dev, af, light, probe, want, "empty range", rows=np.zeros(af.H, bool), row_begin=7, row_end=7)
        assert ctx.get_option("adaptive_traces") == n0
        # the host form stages rows 8..24 as a frame of their own: its pixel 0 is pixel 8 * W of the caller's frame ("pixelBase")
        om, orf = np.full((af.H, af.W), GUARD_M, np.uint8), np.full((af.H, af.W), GUARD_R, np.uint8)
        ctx.trace_shadow_mask_adaptive(af.k, af.pos, af.W, af.H, light, probe, row_begin=8, row_end=24, out=om, refined=orf)
        _same((om, orf), _expect(want, None, rows), (kernel, split, "host rows"))
        assert ctx.last_kernel_name() == _name(kernel, split)
        m, r = ctx.trace_shadow_mask_adaptive(af.k, af.pos, af.W, af.H, light, probe)
        _same((m, r), want, (kernel, split, "host whole"))
        m, r = ctx.trace_shadow_mask_adaptive(af.k, af.pos, af.W, af.H, light, probe, want_refined=False)
        assert r is None and np.array_equal(m, want[0])
        # ... with a map and a ragged row range
        active = _checker(af)
        dirty = af.pos.copy()
        dirty[active == 0] = POISON
        om, orf = np.full((af.H, af.W), GUARD_M, np.uint8), np.full((af.H, af.W), GUARD_R, np.uint8)
        ctx.trace_shadow_mask_adaptive(af.k, dirty, af.W, af.H, light, probe, row_begin=5, row_end=41, active=active, out=om, refined=orf)
        _same((om, orf), _expect(want, active, rows2), (kernel, split, "host rows with a map"))
    finally:
        _reset(ctx)
        dev.close()


# ---- 3. active maps ----------------------------------------------------------------------------------------------------------------
def _checker(af):
    y, x = np.mgrid[0:af.H, 0:af.W]
    return (((x + y) & 1) * 255).astype(np.uint8)


def _maps(af, want):
    """checker: every tile half active.  chosen: nothing but (a) one 8 x 8 tile that refines, wholly active, (b) in another tile that
    holds penumbra AND unanimous pixels only the unanimous ones (an active tile that must leave between the barriers although its
    full version would not), (c) one pixel alone in its tile; every other tile has no active pixel."""
    refined = want[1]
    t = tiles_8x8(refined)
    mixed = np.argwhere((t == 1).any(axis=2) & (t == 0).any(axis=2))
    assert mixed.shape[0] >= 2, "two tiles with penumbra and unanimous pixels"
    (ay, ax), (by, bx) = mixed[0], mixed[-1]
    chosen = np.zeros((af.H, af.W), np.uint8)
    chosen[ay * 8:ay * 8 + 8, ax * 8:ax * 8 + 8] = 1
    tile_b = np.zeros((af.H, af.W), bool)
    tile_b[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = True
    chosen[tile_b & (refined == 0)] = 200
    assert int((chosen == 200).sum()) >= 1 and int(refined[chosen == 200].sum()) == 0 and int(refined[chosen == 1].sum()) >= 1
    free = np.argwhere(~((t == 1).any(axis=2)) & (np.arange(t.shape[1])[None, :] * 8 + 8 <= af.W))
    cy, cx = [c for c in free.tolist() if c not in ([ay, ax], [by, bx])][0]
    chosen[cy * 8 + 3, cx * 8 + 5] = 7
    return {"checker": _checker(af), "chosen": chosen, "zeros": np.zeros((af.H, af.W), np.uint8)}


@pytest.mark.parametrize("kernel,split", FEW_FORMS)
@pytest.mark.parametrize("key,probe", [(POINT_16_OF_16, 4), (POINT_5_OF_16, 4)], ids=case_id)
def test_active_maps(ctx, key, probe, kernel, split):
    af = adaptive_frame(64, 48)
    light, want = af.light(key), af.want(key, probe)
    ctx.set_bvh(af.packed)
    dev = _Dev(ctx, af.pos, af.W, af.H)
    rows = (np.arange(af.H) >= 5) & (np.arange(af.H) < 42)
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        for name, active in _maps(af, want).items():
            dirty = af.pos.copy()                        # inactive texels may hold anything
            dirty[active == 0] = POISON
            ctx.h2d(dev.d_pos, dirty)
            _trace(ctx, dev, af, light, probe, want, (kernel, split, name), active=active)
            _trace(ctx, dev, af, light, probe, want, (kernel, split, name, "rows"), active=active, rows=rows, row_begin=5, row_end=42)
    finally:
        _reset(ctx)
        dev.close()


# ---- 4. stripes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split,band", [(3, 1, 8), (3, 1, 16), (3, 1, 32), (3, 0, 8), (3, 0, 16), (7, 1, 16), (7, 1, 32)])
def test_stripes(ctx, kernel, split, band):
    af = adaptive_frame(61, 37)
    key, probe = POINT_5_OF_16, 4
    light, want = af.light(key), af.want(key, probe)
    ctx.set_bvh(af.packed)
    dev = _Dev(ctx, af.pos, af.W, af.H)
    active = _checker(af)
    ctx.h2d(dev.d_act, active)
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        for with_map in (False, True):
            for stripe in range(3):                      # (37 rows in bands of 16 or more: a stripe that owns no band)
                rows = ((np.arange(af.H) // band) % 3) == stripe
                n0 = ctx.get_option("adaptive_traces")
                dev.guard()
                ctx.trace_shadow_mask_adaptive_stripes_device(af.k, dev.d_pos, af.W, af.H, dev.d_mask, band, 3, stripe, light, probe,
                                                              d_refined=dev.d_ref, d_active=dev.d_act if with_map else None)
                _same(dev.read(), _expect(want, active if with_map else None, rows), (kernel, split, band, with_map, stripe))
                # a stripe without a band launches nothing, and the counter does not move
                assert ctx.get_option("adaptive_traces") == n0 + (1 if rows.any() else 0), (band, stripe)
                if rows.any():
                    assert ctx.last_kernel_name() == _name(kernel, split, "bands"), ctx.last_kernel_name()
        # a band that is no whole number of workgroup rows is refused, and nothing is written: 8 rows for the lane-per-ray family
        bad = 12 if kernel == 3 else 8
        dev.guard()
        n0 = ctx.get_option("adaptive_traces")
        with pytest.raises(api.RtsError):
            ctx.trace_shadow_mask_adaptive_stripes_device(af.k, dev.d_pos, af.W, af.H, dev.d_mask, bad, 2, 0, light, probe, d_refined=dev.d_ref)
        _same(dev.read(), _expect(want, None, np.zeros(af.H, bool)), (kernel, bad, "refused"))
        assert ctx.get_option("adaptive_traces") == n0
        if kernel == 3:                                  # 24 rows: not a power of two -- the general form
            rows = ((np.arange(af.H) // 24) % 2) == 1
            dev.guard()
            ctx.trace_shadow_mask_adaptive_stripes_device(af.k, dev.d_pos, af.W, af.H, dev.d_mask, 24, 2, 1, light, probe, d_refined=dev.d_ref)
            _same(dev.read(), _expect(want, None, rows), (kernel, split, 24))
            assert ctx.last_kernel_name() == _name(kernel, split, "general")
    finally:
        _reset(ctx)
        dev.close()


# ---- 5. the refined plane is optional; the counters; the refusals ------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", FEW_FORMS)
def test_refined_null_and_the_counters(ctx, kernel, split):
    af = adaptive_frame(64, 48)
    key, probe = POINT_16_OF_16, 4
    light, want = af.light(key), af.want(key, probe)
    ctx.set_bvh(af.packed)
    dev = _Dev(ctx, af.pos, af.W, af.H)
    active = _checker(af)
    ctx.h2d(dev.d_act, active)
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        before = [ctx.get_option(k) for k in COUNTERS]
        n0 = ctx.get_option("adaptive_traces")
        for with_map in (False, True):
            dev.guard()
            ctx.trace_shadow_mask_adaptive_device(af.k, dev.d_pos, af.W, af.H, dev.d_mask, light, probe,
                                                  d_active=dev.d_act if with_map else None)
            m, r = dev.read()
            assert np.array_equal(m, _expect(want, active if with_map else None)[0]) and (r == GUARD_R).all(), (kernel, split, with_map)
        ctx.trace_shadow_mask_adaptive_stripes_device(af.k, dev.d_pos, af.W, af.H, dev.d_mask, 16, 2, 1, light, probe)
        ctx.trace_shadow_mask_adaptive_stripes_device(af.k, dev.d_pos, af.W, af.H, dev.d_mask, 32, 3, 2, light, probe)   # owns no band
        ctx.trace_shadow_mask_adaptive(af.k, af.pos, af.W, af.H, light, probe)
        ctx.synchronize()
        assert ctx.get_option("adaptive_traces") == n0 + 4
        assert [ctx.get_option(k) for k in COUNTERS] == before           # no other trace counter moves
        with pytest.raises(api.RtsError):                # read-only
            ctx.set_option("adaptive_traces", 0)
        # the refusals, with a context: nothing written, nothing counted
        dev.guard()
        many = type(light).from_buffer_copy(light)
        many.nsamples, many.table = 65, 0
        one = type(light).from_buffer_copy(light)
        one.nsamples, one.table = 1, 0
        for lt, k in ((light, 0), (light, 16), (light, 17), (many, 4), (one, 1), (None, 1)):
            with pytest.raises(api.RtsError):
                ctx.trace_shadow_mask_adaptive_device(af.k, dev.d_pos, af.W, af.H, dev.d_mask, lt, k, d_refined=dev.d_ref)
            with pytest.raises(api.RtsError):
                ctx.trace_shadow_mask_adaptive(af.k, af.pos, af.W, af.H, lt, k)
        m, r = dev.read()
        assert (m == GUARD_M).all() and (r == GUARD_R).all()
        assert ctx.get_option("adaptive_traces") == n0 + 4
    finally:
        _reset(ctx)
        dev.close()


# ---- 6. options change no byte -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [1, 0])
def test_options_change_no_byte(ctx, split):
    af = adaptive_frame(61, 37)
    ctx.set_bvh(af.packed)
    dev = _Dev(ctx, af.pos, af.W, af.H)
    before = (ctx.get_option("packet_budget"), ctx.get_option("packet_share"))
    try:
        ctx.set_option("kernel", 3)
        ctx.set_option("soft_split", split)
        for key, probe in ((POINT_16_OF_16, 4), (POINT_5_OF_16, 4), (DIR_4_OF_16, 2)):
            light, want = af.light(key), af.want(key, probe)
            active = _checker(af)
            ctx.set_option("packet_budget", 1)           # every packet dissolves at once
            ctx.set_option("packet_share", 16)
            _trace(ctx, dev, af, light, probe, want, ("dissolve", split, key))
            _trace(ctx, dev, af, light, probe, want, ("dissolve", split, key, "map"), active=active)
            ctx.set_option("packet_budget", before[0])
            ctx.set_option("packet_share", before[1])
            for order in (1, 2):
                ctx.set_option("row_order", order)
                _trace(ctx, dev, af, light, probe, want, ("row_order", order, split, key), active=active)
                assert ctx.last_kernel_name() == _name(3, split, "rows")
            ctx.set_option("row_order", 0)
            ctx.set_option("xcd_swizzle", 1)
            _trace(ctx, dev, af, light, probe, want, ("swizzle", split, key))
            assert ctx.last_kernel_name() == _name(3, split, "general")
            ctx.set_option("xcd_swizzle", 0)
        ctx.set_option("kernel", 7)
        for order in (1, 2):
            ctx.set_option("row_order", order)
            _trace(ctx, dev, af, light, probe, want, ("row_order", order, "share"))
    finally:
        ctx.set_option("packet_budget", before[0])
        ctx.set_option("packet_share", before[1])
        _reset(ctx)
        dev.close()


# ---- 7. installed state stays ------------------------------------------------------------------------------------------------------
def test_installed_state_stays(ctx):
    wl = workloads.prepare_config("cornell_256")
    W, H = wl.W, wl.H
    soft = workloads.relight(wl, "point", 6, RADIUS_FEW).light
    probe = 2
    want = api.shadow_mask_adaptive(wl.packed, wl.constants, soft, wl.positions, W, H, probe)
    assert 0 < int(want[1].sum()) < want[1].size
    plain = api.shadow_distance(wl.packed, wl.constants, wl.light, wl.positions, W, H)[1]
    assert 0 < int(plain.sum()) < plain.size
    ctx.set_bvh(wl.packed)
    dev = _Dev(ctx, wl.positions, W, H)
    options = ["kernel", "xcd_swizzle", "packet_budget", "packet_share", "block_waves", "row_order", "wide_lane", "soft_split", "tile_splits",
               "follow", "tile_order", "tile_order_tiles", "follow_traces"] + COUNTERS

    def adaptive_trace():
        n0 = ctx.get_option("adaptive_traces")
        before = {k: ctx.get_option(k) for k in options}
        dev.guard()
        ctx.trace_shadow_mask_adaptive_device(wl.constants, dev.d_pos, W, H, dev.d_mask, soft, probe, d_refined=dev.d_ref)
        _same(dev.read(), want, "adaptive")
        assert ctx.get_option("adaptive_traces") == n0 + 1 and ctx.last_kernel_name() == _name(3, 1)
        assert {k: ctx.get_option(k) for k in options} == before

    def plain_trace():
        dev.guard()
        ctx.trace_shadow_mask_device(wl.constants, dev.d_pos, W, H, dev.d_mask, light=wl.light)
        assert np.array_equal(dev.read()[0], plain)
        return ctx.last_kernel_name()

    try:
        ctx.set_option("kernel", 3)
        # a split table
        tiles, records = ctx.plan_splits(wl.constants, dev.d_pos, W, H, dev.d_mask, light=wl.light, min_life_us=4.0, piece_us=2.0,
                                         max_pieces=8, front_share=1.0 / 3.0)
        assert tiles > 0
        table = tuple(ctx.get_option(k) for k in ("split_tiles", "front_tiles", "split_pieces"))
        name_before = plain_trace()
        adaptive_trace()
        assert tuple(ctx.get_option(k) for k in ("split_tiles", "front_tiles", "split_pieces")) == table
        assert plain_trace() == name_before
        ctx.clear_splits()
        # a caller's tile order
        order = np.arange(((W + 7) // 8) * ((H + 7) // 8), dtype=np.uint32)[::-1].copy()
        ctx.set_tile_order(order)
        order_state = (ctx.get_option("tile_order_tiles"), ctx.get_option("tile_order"))
        assert order_state[0] == order.size
        name_before = plain_trace()
        adaptive_trace()
        assert (ctx.get_option("tile_order_tiles"), ctx.get_option("tile_order")) == order_state
        assert plain_trace() == name_before
        ctx.set_tile_order(None)
        # follow mode
        ctx.set_option("follow", 1)
        plain_trace()
        name_follow = plain_trace()
        assert name_follow.startswith("shadowMaskFollowKernel<")
        traces, ordered = ctx.get_option("follow_traces"), ctx.get_option("follow_ordered")
        adaptive_trace()
        assert (ctx.get_option("follow_traces"), ctx.get_option("follow_ordered"), ctx.get_option("follow")) == (traces, ordered, 1)
        assert plain_trace() == name_follow
    finally:
        ctx.set_option("follow", 0)
        ctx.set_tile_order(None)
        ctx.clear_splits()
        _reset(ctx)
        dev.close()


# ---- 8. graph capture --------------------------------------------------------------------------------------------------------------
def _copy(struct):
    return type(struct).from_buffer_copy(struct)


@pytest.mark.parametrize("form", ["whole", "rows", "stripe"])
@pytest.mark.parametrize("kernel,split", FEW_FORMS)
def test_device_forms_under_capture(ctx, kernel, split, form):
    af = adaptive_frame(64, 48)
    key, probe = POINT_5_OF_16, 4
    want = af.want(key, probe)
    ctx.set_bvh(af.packed)
    dev = _Dev(ctx, af.pos, af.W, af.H)
    checker = _checker(af)
    stream = ctx.stream_create()
    k, light = _copy(af.k), _copy(af.light(key))
    g = None
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        ctx.h2d(dev.d_act, checker)
        ctx.trace_shadow_mask_device(af.k, dev.d_pos, af.W, af.H, dev.d_mask, light=af.light(key), stream=stream)   # a stream that has traced
        ctx.synchronize(stream)
        rows = None
        if form == "whole":
            record = lambda: ctx.trace_shadow_mask_adaptive_device(k, dev.d_pos, af.W, af.H, dev.d_mask, light, probe, d_refined=dev.d_ref,
                                                                   stream=stream, d_active=dev.d_act)
        elif form == "rows":
            rows = (np.arange(af.H) >= 5) & (np.arange(af.H) < 41)
            record = lambda: ctx.trace_shadow_mask_adaptive_device(k, dev.d_pos, af.W, af.H, dev.d_mask, light, probe, d_refined=dev.d_ref,
                                                                   stream=stream, d_active=dev.d_act, row_begin=5, row_end=41)
        else:
            rows = ((np.arange(af.H) // 16) % 2) == 1
            record = lambda: ctx.trace_shadow_mask_adaptive_stripes_device(k, dev.d_pos, af.W, af.H, dev.d_mask, 16, 2, 1, light, probe,
                                                                           d_refined=dev.d_ref, stream=stream, d_active=dev.d_act)
        n0 = ctx.get_option("adaptive_traces")
        g = hipgraph.capture(stream, record)
        assert ctx.get_option("adaptive_traces") == n0 + 1
        types = g.node_types()
        assert types == [hipgraph.KERNEL], (kernel, split, form, types)   # one kernel node; no memcpy, memset or allocation node
        for s in (k, light):                             # what a caller may do to its structs between capture and replay
            C.memset(C.byref(s), 0x7F, C.sizeof(s))
        # the replay follows the buffers: the map the device holds at the replay, not the one it held at the capture
        for replay, active in enumerate((checker, (255 - checker).astype(np.uint8))):
            ctx.h2d(dev.d_act, active)
            dev.guard()
            g.launch(stream)
            _same(dev.read(stream), _expect(want, active, rows), (kernel, split, form, replay))
    finally:
        if g:
            g.close()
        ctx.synchronize(stream)
        ctx.stream_destroy(stream)
        _reset(ctx)
        dev.close()
