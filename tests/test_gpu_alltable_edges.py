"""GPU: the ALLTABLE instantiations of the wide packet kernel on the cases of tests/alltable_cases.py -- both of them,
SEG = true for a point light and SEG = false for the directional light, which tests/test_gpu_alltable.py never launches.

Every mask is compared byte for byte with the oracle's, over a mask preset to 77; the counter "alltable_traces" says which
instantiation ran.  Both lights on cornell, on a frame with sky tiles and on frames of 258 tiles along one axis; dissolves inside the
walk (and the proof, from wave statistics, that the budget makes waves dissolve); row ranges with both ends inside tiles; the clock
probe; several installs in one context (upload, the device builder's install, "wide_copy" off and on); the options and launches that
must de-select the instantiation, and its return; the options that must not matter; captured traces replayed after refits; texels
the fast ray set-up refuses, on sky tiles and in partial edge tiles."""
import numpy as np
import pytest

import alltable_cases as ac
import hipgraph
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

WIDE = "shadowMaskPacketKernel<1,wide>"       # every instantiation of kernel 8 reports this name; "alltable_traces" counts ALLTABLE's launches
FOLLOW = "shadowMaskFollowKernel<1,wide>"
FILL, WHOLE, LIGHTS = ac.FILL, ac.WHOLE, ac.LIGHTS


class _Dev:
    """tests/test_gpu_alltable.py's, with a row range, another light and stripes."""

    def __init__(self, ctx, wl, positions=None):
        self.ctx, self.wl = ctx, wl
        pos = np.ascontiguousarray(wl.positions if positions is None else positions)
        self.d_pos, self.d_mask = ctx.malloc(pos.nbytes), ctx.malloc(wl.W * wl.H)
        ctx.h2d(self.d_pos, pos)

    def fill(self):
        self.ctx.h2d(self.d_mask, np.full(self.wl.W * self.wl.H, FILL, np.uint8))

    def trace(self, stream=None, alltable=None, rows=None, light="own", stripes=None):
        """One trace (stripes = (band_rows, n): one per stripe) into the preset mask; alltable True / False: it must (not) have run the
        ALLTABLE instantiation, and when it must, the kernel is kernel 8."""
        wl, ctx = self.wl, self.ctx
        lt = wl.light if isinstance(light, str) else light
        before = ctx.get_option("alltable_traces")
        self.fill()
        if stripes:
            for s in range(stripes[1]):
                ctx.trace_shadow_mask_stripes_device(wl.constants, self.d_pos, wl.W, wl.H, self.d_mask, stripes[0], stripes[1], s, light=lt, stream=stream)
        else:
            r0, r1 = rows or (0, wl.H)
            ctx.trace_shadow_mask_device(wl.constants, self.d_pos, wl.W, wl.H, self.d_mask, light=lt, row_begin=r0, row_end=r1, stream=stream)
        if alltable is not None:
            ran = ctx.get_option("alltable_traces") - before
            assert ran == (1 if alltable else 0), ("alltable_traces", ran, "expected ALLTABLE", alltable)
            if alltable:
                assert ctx.last_kernel_name() == WIDE
        return self.read(stream)

    def read(self, stream=None):
        self.ctx.synchronize(stream)
        got = np.empty((self.wl.H, self.wl.W), np.uint8)
        self.ctx.d2h(got, self.d_mask)
        return got

    def plan(self, rows=None, **kw):
        """A whole-dispatch table of the frame (or of its rows [r0, r1)): every tile a front record, none split."""
        wl, ctx = self.wl, self.ctx
        r0, r1 = rows or (0, wl.H)
        tiles, records = ctx.plan_splits(wl.constants, self.d_pos, wl.W, wl.H, self.d_mask, light=wl.light, row_begin=r0, row_end=r1, **WHOLE, **kw)
        bx, by = ac.tiles_of(wl.W, r1 - r0)
        assert ctx.get_option("front_tiles") == bx * by and ctx.get_option("split_tiles") == 0, (tiles, records, bx, by)
        assert records == bx * by
        return bx, by, records

    def close(self):
        self.ctx.free(self.d_pos)
        self.ctx.free(self.d_mask)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:4].tolist())


class _Installed:
    """A context with the frame's stream installed, kernel 8 selected, the frame on the device."""

    def __init__(self, wl, positions=None, packed=None):
        self.wl, self.positions, self.packed = wl, positions, packed

    def __enter__(self):
        self.ctx = api.ShadowContext(0)
        try:
            self.ctx.set_bvh(self.wl.packed if self.packed is None else self.packed)
            self.ctx.set_option("kernel", 8)
            self.dev = _Dev(self.ctx, self.wl, self.positions)
        except BaseException:
            self.ctx.close()
            raise
        return self.ctx, self.dev

    def __exit__(self, *a):
        try:
            self.dev.close()
        finally:
            self.ctx.close()


# ----------------------------------------------------------------------------------------------------------------- a. both lights
@pytest.mark.parametrize("light", LIGHTS)
@pytest.mark.parametrize("f", ac.FRAMES, ids=ac.frame_id)
def test_both_lights_run_their_instantiation_on_every_frame(f, light):
    """light = directional: the first launches of the SEG = false ALLTABLE kernel in the suite.  The sky frame: waves of background
    texels only.  2064 x 8 and 8 x 2064: bx, by above 255 in a record's halves; 258 records, the map's last slots uneven."""
    wl = ac.frame(f, light)
    if f == ac.SKY:
        ac.assert_sky(wl.positions)
    with _Installed(wl) as (ctx, dev):
        _same(dev.trace(alltable=False), wl.want, "no table")
        for square, block in ((0, 0), (32, 16)):
            bx, by, records = dev.plan(xcd_square=square, life_block=block)
            if f in ac.LONG:
                assert max(bx, by) == 258 and records % 8 != 0
            _same(dev.trace(alltable=True), wl.want, ("whole-dispatch table", square, block))
        ctx.clear_splits()
        _same(dev.trace(alltable=False), wl.want, "table cleared")


# ------------------------------------------------------------------------------------------------------- b. dissolves inside ALLTABLE
@pytest.mark.parametrize("light", LIGHTS)
def test_dissolves_inside_the_walk(light):
    """wideDissolve makes the stream's buffer resource late in traverseWideScene.  "packet_budget" 1, 2 and 8 with "packet_share" 0 and
    at its default: the mask with the table is the oracle's.  That waves DO dissolve is read from the wave statistics of the plain wide
    kernel under the same options ("tile_splits" 0, "wave_stats" on), which shares wideDescend and the budget: the waves whose
    dissolved bit (o[2] & 1) is set.  Asserted above 0 at budget 1 with the default share, the case the walk checks its coherence at
    every node; the other counts are printed (with share 0 the rule's threshold budget * share is 0 and no member count lies below
    it: only a nearly full stack dissolves such a wave)."""
    f = ac.CORNELL[0]
    wl = ac.frame(f, light)
    bx, by = ac.tiles_of(wl.W, wl.H)
    with _Installed(wl) as (ctx, dev):
        default_share = ctx.get_option("packet_share")
        assert default_share > 0
        dev.plan(xcd_square=32, life_block=16)
        counts = {}
        for share in (0, default_share):
            for budget in (1, 2, 8):
                ctx.set_option("packet_share", share)
                ctx.set_option("packet_budget", budget)
                _same(dev.trace(alltable=True), wl.want, ("table", "budget", budget, "share", share))
                ctx.set_option("tile_splits", 0)
                ctx.set_option("wave_stats", bx * by)
                _same(dev.trace(alltable=False), wl.want, ("wave statistics", "budget", budget, "share", share))
                stats = ctx.read_wave_stats(bx * by)
                ctx.set_option("wave_stats", 0)
                ctx.set_option("tile_splits", 1)
                counts[(budget, share)] = int((stats[:, 2] & np.uint64(1)).sum())
        print(f"dissolved waves of {bx * by} ({ac.frame_id(f)}, {light}) by (budget, share): {counts}")
        n = counts[(1, default_share)]
        assert n > 0, f"{n} of {bx * by} waves dissolved at packet_budget 1, packet_share {default_share} ({light}): {counts}"


# -------------------------------------------------------------------------------------------------------------------- c. row ranges
@pytest.mark.parametrize("light", LIGHTS)
@pytest.mark.parametrize("f", ac.CORNELL, ids=ac.frame_id)
def test_row_ranges_run_alltable_and_leave_the_other_rows_alone(f, light):
    """The table is kept for its dispatch -- W, H and the row range (madeFor) -- and a range's grid is blocksX x ceil(rows / 8) records in
    as many rows, so allTableRule gives True for a trace of the planned range: the wave adds p.rowBegin to its tile's rows.  A trace of
    another range finds no table for its dispatch: the everyday kernel."""
    wl = ac.frame(f, light)
    with _Installed(wl) as (ctx, dev):
        for r0, r1 in ac.row_ranges(wl.H):
            assert 0 <= r0 < r1 <= wl.H
            bx, by, records = dev.plan(rows=(r0, r1), xcd_square=32, life_block=16)
            rule = ac.all_table_rule(bx, by, records, piece_rows=by)
            assert rule is True
            _same(dev.trace(alltable=rule, rows=(r0, r1)), ac.rows_of(wl.want, r0, r1), ("planned range", r0, r1))
            for o0, o1 in ((0, wl.H), (max(r0 - 3, 0), r1), (r0, min(r1 + 2, wl.H))):
                _same(dev.trace(alltable=False, rows=(o0, o1)), ac.rows_of(wl.want, o0, o1), ("table of", r0, r1, "trace of", o0, o1))
            _same(dev.trace(alltable=True, rows=(r0, r1)), ac.rows_of(wl.want, r0, r1), ("planned range again", r0, r1))


# ------------------------------------------------------------------------------------------------------------------- d. clock probe
@pytest.mark.parametrize("light", LIGHTS)
def test_the_clock_probe_changes_no_byte_and_stamps_every_row(light):
    wl = ac.frame(ac.CORNELL[1], light)
    with _Installed(wl) as (ctx, dev):
        bx, by, _ = dev.plan(xcd_square=32, life_block=16)
        _same(dev.trace(alltable=True), wl.want, "probe off")
        ctx.set_option("clock_probe", by)
        _same(dev.trace(alltable=True), wl.want, "probe on")
        mhz = ctx.clock_probe_mhz(by)
        o = ctx.last_clock_probe
        low48 = np.uint64(0x0000FFFFFFFFFFFF)
        clocks = (o[:, 1] - o[:, 0]) & low48                       # (the end stamp's top 16 bits carry the wave's hardware slot)
        assert (o[:, 3] > o[:, 2]).all(), ("100 MHz stamps", o[:, 2:].tolist())
        assert ((clocks > 0) & (clocks < np.uint64(1 << 40))).all(), ("shader clock stamps", clocks.tolist())
        assert mhz is None or mhz > 0
        ctx.set_option("clock_probe", 0)
        _same(dev.trace(alltable=True), wl.want, "probe off again")


# ------------------------------------------------------------------------------------------------- e. one context, several installs
@pytest.mark.parametrize("light", LIGHTS)
def test_one_context_through_several_installs(light):
    """The context's block of per-scene constants is one allocation, rewritten by every install that derives a private copy.  (The
    library has no other adopt entry point than the device builder's install.)"""
    wl = ac.frame(ac.CORNELL[0], light)
    A = wl.packed
    B = api.BVHBuilder().build(ac.moved(wl, ac.ROOTS[1]), 8, wl.indices, wl.prim_count).m_packedNodes
    assert B[1, 0:1].view(np.float32)[0] == np.float32(ac.ROOTS[1])          # node 0's bboxMax.x
    want_b = ac.want(wl, packed=B)
    with _Installed(wl) as (ctx, dev):
        plan = lambda: dev.plan(xcd_square=32, life_block=16)
        plan()
        _same(dev.trace(alltable=True), wl.want, "A installed and planned")
        ctx.set_bvh(B)
        _same(dev.trace(alltable=False), want_b, "B installed: the table is gone")
        plan()
        _same(dev.trace(alltable=True), want_b, "B planned")
        packed, _ = api.bvh_build_device(ctx, wl.vertices, 8, wl.indices, wl.prim_count, install=True, want_packed=True)
        want_built = ac.want(wl, packed=packed)
        _same(dev.trace(alltable=False), want_built, "the device builder's install: the table is gone")
        plan()
        _same(dev.trace(alltable=True), want_built, "the device builder's stream, planned")
        ctx.set_option("wide_copy", 0)
        ctx.set_bvh(B)
        assert ctx.get_option("wide_nodes") == 0
        _same(dev.trace(alltable=False), want_b, "B without a private copy")
        ctx.set_option("wide_copy", 1)
        ctx.set_bvh(A)
        assert ctx.get_option("wide_nodes") > 0
        _same(dev.trace(alltable=False), wl.want, "A again, before a plan")
        plan()
        _same(dev.trace(alltable=True), wl.want, "A again, planned")


# ------------------------------------------------------------------------------ f. what must de-select the instantiation, and its return
@pytest.mark.parametrize("light", LIGHTS)
def test_what_de_selects_alltable_and_its_return(light):
    """Each on its own, with the table installed: the host's count (rts_api.cpp) and the launcher's choice (launchWide) must agree on
    the grid, or the mask is wrong.  Afterwards the instantiation is back."""
    wl = ac.frame(ac.CORNELL[1], light)
    soft = ac.soft_light(wl, light, 4)
    want_soft = ac.want(wl, light=soft)
    assert want_soft.max() > 1                                                 # (counts of unoccluded samples, not a mask)
    with _Installed(wl) as (ctx, dev):
        bx, by, _ = dev.plan(xcd_square=32, life_block=16)
        _same(dev.trace(alltable=True), wl.want, "installed")
        for key, on, off in (("wide_lane", 1, 0), ("block_waves", 4, 1), ("wave_stats", bx * by, 0), ("tile_splits", 0, 1), ("kernel", 7, 8)):
            ctx.set_option(key, on)
            _same(dev.trace(alltable=False), wl.want, (key, on))
            ctx.set_option(key, off)
            _same(dev.trace(alltable=True), wl.want, (key, "restored"))
        _same(dev.trace(alltable=False, light=soft), want_soft, "4 light samples")
        _same(dev.trace(alltable=True), wl.want, "one sample again")
        _same(dev.trace(alltable=False, stripes=(8, 2)), wl.want, "two stripes of 8-row bands")
        _same(dev.trace(alltable=False, stripes=(16, 3)), wl.want, "three stripes of 16-row bands")
        _same(dev.trace(alltable=True), wl.want, "the whole frame again")


@pytest.mark.parametrize("light", LIGHTS)
def test_follow_mode_and_the_table(light):
    """include/rts.h: "an installed table ... always wins" -- with the table installed "follow" 1 records nothing and the trace runs the
    table, that is ALLTABLE.  Where no table applies, follow mode's planned order is a launch whose parameters look like a whole-dispatch
    table's (every tile a record, no pieces, a front map): the rule's `follow` term keeps ALLTABLE off it, in its own kernel."""
    wl = ac.frame(ac.CORNELL[1], light)
    with _Installed(wl) as (ctx, dev):
        dev.plan(xcd_square=32, life_block=16)
        ctx.set_option("follow", 1)
        recorded = ctx.get_option("follow_traces")
        _same(dev.trace(alltable=True), wl.want, "follow on, the table wins")
        assert ctx.get_option("follow_traces") == recorded
        ctx.set_option("tile_splits", 0)
        ordered = ctx.get_option("follow_ordered")
        for turn in range(3):                                                  # (the first records, the later ones run the planned order)
            _same(dev.trace(alltable=False), wl.want, ("follow mode", turn))
            assert ctx.last_kernel_name() == FOLLOW
        assert ctx.get_option("follow_ordered") == ordered + 2
        ctx.set_option("tile_splits", 1)
        _same(dev.trace(alltable=True), wl.want, "the table again, follow still on")
        ctx.set_option("follow", 0)
        _same(dev.trace(alltable=True), wl.want, "follow off")


# --------------------------------------------------------------------------------------------------- g. options that must not matter
@pytest.mark.parametrize("light", LIGHTS)
def test_options_that_must_not_change_a_byte(light):
    """What the code does, by the counter: "row_order" and "lds_pad" leave ALLTABLE selected (its waves run in record order; the pad is
    a launch parameter).  "xcd_swizzle" 1 and an installed tile order with "tile_order" on make the launch 1-D, where no table applies:
    the everyday kernel.  The mask is the same each time."""
    wl = ac.frame(ac.CORNELL[1], light)
    with _Installed(wl) as (ctx, dev):
        bx, by, _ = dev.plan(xcd_square=32, life_block=16)
        _same(dev.trace(alltable=True), wl.want, "installed")
        for key, value, runs in (("row_order", 1, True), ("row_order", 2, True), ("row_order", 0, True), ("xcd_swizzle", 1, False),
                                 ("xcd_swizzle", 0, True), ("lds_pad", 4096, True), ("lds_pad", 0, True)):
            ctx.set_option(key, value)
            _same(dev.trace(alltable=runs), wl.want, (key, value))
        ordered = ctx.plan_tile_order(wl.constants, dev.d_pos, wl.W, wl.H, dev.d_mask, light=wl.light)
        assert ordered == bx * by and ctx.get_option("tile_order_tiles") == bx * by
        assert ctx.get_option("front_tiles") == bx * by                       # (the table is still installed)
        _same(dev.trace(alltable=False), wl.want, "a planned tile order, on")
        ctx.set_option("tile_order", 0)
        _same(dev.trace(alltable=True), wl.want, "the tile order ignored")
        ctx.set_option("tile_order", 1)
        ctx.set_tile_order(None)
        _same(dev.trace(alltable=True), wl.want, "the tile order removed")


# ------------------------------------------------------------------------------------------------------------ h. capture, directional
def _captured(ctx, dev, stream):
    wl = dev.wl
    before = ctx.get_option("alltable_traces")
    g = hipgraph.capture(stream, lambda: ctx.trace_shadow_mask_device(wl.constants, dev.d_pos, wl.W, wl.H, dev.d_mask, light=wl.light, stream=stream))
    try:
        assert ctx.get_option("alltable_traces") == before + 1 and g.node_types() == [hipgraph.KERNEL], g.node_types()
    except BaseException:
        g.close()
        raise
    return g


def test_a_captured_directional_trace_replayed_after_refits():
    wl = ac.frame(ac.CORNELL[0], "directional")
    with _Installed(wl) as (ctx, dev):
        stream = ctx.stream_create()
        g = None
        try:
            dev.plan(xcd_square=32, life_block=16)
            _same(dev.trace(stream, alltable=True), wl.want, "first trace on the stream (the table's state for it)")
            g = _captured(ctx, dev, stream)
            dev.fill()
            g.launch(stream)
            _same(dev.read(stream), wl.want, "replay")
            for x in ac.ROOTS:
                packed, _, _ = api.bvh_refit_device(ctx, ac.moved(wl, x), 8, wl.indices, wl.prim_count, want_packed=True)
                assert packed[1, 0:1].view(np.float32)[0] == np.float32(x)
                dev.fill()
                g.launch(stream)
                _same(dev.read(stream), ac.want(wl, packed=packed), ("replay after a refit", x))
        finally:
            if g:
                g.close()
            ctx.synchronize(stream)
            ctx.stream_destroy(stream)


@pytest.mark.parametrize("light", LIGHTS)
def test_a_captured_trace_at_budget_one(light):
    wl = ac.frame(ac.CORNELL[0], light)
    with _Installed(wl) as (ctx, dev):
        stream = ctx.stream_create()
        g = None
        try:
            ctx.set_option("packet_budget", 1)
            dev.plan(xcd_square=32, life_block=16)
            _same(dev.trace(stream, alltable=True), wl.want, "first trace on the stream")
            g = _captured(ctx, dev, stream)
            for turn in range(2):
                dev.fill()
                g.launch(stream)
                _same(dev.read(stream), wl.want, ("replay", turn))
        finally:
            if g:
                g.close()
            ctx.synchronize(stream)
            ctx.stream_destroy(stream)


# ------------------------------------------------------------------------------------------- i. bad texels on sky and edge tiles
def _bad_frames():
    """(frame, where): one refused texel per tile of the sky frame -- so also in tiles of background only -- and of ragged cornell, whose
    partial edge tiles get theirs in the last column and the last row."""
    return [(ac.SKY, "every tile"), (ac.CORNELL[1], "every tile"), (ac.SKY, "one sky tile"), (ac.CORNELL[1], "the corner tile")]


@pytest.mark.parametrize("light", LIGHTS)
@pytest.mark.parametrize("case", _bad_frames(), ids=lambda c: f"{ac.frame_id(c[0])}-{c[1].replace(' ', '_')}")
def test_bad_texels_on_sky_and_edge_tiles(case, light):
    """0, a denormal and 1e38: the wave sets its rays up the general way and leaves through the inexact-ray exit, which opens the
    node stream inside the ALLTABLE instantiation -- in a wave that is otherwise all background, and in one with lanes off the frame."""
    f, where = case
    wl = ac.frame(f, light)
    W, H = wl.W, wl.H
    if where == "every tile":
        at = ac.one_per_tile(W, H)
    elif where == "one sky tile":
        sky, _, _ = ac.assert_sky(wl.positions)
        ty, tx = sky[len(sky) // 2]
        at = [(ty * 8 + 6, tx * 8 + 1)]
        assert ac.background(wl.positions)[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].all()
    else:
        assert W % 8 and H % 8                                               # (the corner tile is partial both ways)
        at = [(H - 1, W - 1), (H - 2, (W // 8) * 8)]
    pos = ac.bad_texels(wl, at)
    want = ac.want(wl, positions=pos)
    with _Installed(wl, positions=pos) as (ctx, dev):
        dev.plan(xcd_square=32, life_block=16)
        _same(dev.trace(alltable=True), want, ("bad texels", where))
