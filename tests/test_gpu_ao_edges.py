"""GPU: the ambient occlusion traces (rts_trace_ambient_occlusion*, rts_ao.inc) where their own suite never goes
(inputs: tests/ao_edge_cases.py): edge texels and wild normals behind the two wave-wide gates of the restated ray set-up, first live
lanes that are edge texels, lone pixels or lane 63, tiles that take the no-ray exit in all four waves, the streams the walk treats
specially, a refit that drops the private copy and a captured node replayed after a refit, frames of more than 65 535 block rows
(the 1-D grid), the default family's threshold, and the options the header promises to ignore and keep.

Everywhere the expected plane is the oracle's any-hit sum over the rays of the numpy rule (ao_edge_cases.want; on the tall frames
gathered with a numpy hash): no host twin stands in between -- tests/test_ao_edge_cases_host.py pins the twin and the rule to the
same values.  Counts are compared byte for byte on a plane preset to 0xAB inside a larger guarded block.  Every test asserts its
guards from the oracle's planes alone before its first trace, asserts the kernel's name, asserts that "ao_traces" moved and no other
trace counter did, and restores the options it sets."""
from contextlib import contextmanager

import numpy as np
import pytest

import ao_edge_cases as aec
import hipgraph
from raytracedshadows_amd import api
from test_gpu_ao import GUARD, SHARE, _name, _same
from test_gpu_edge_traces import _stream, _tall_height

pytestmark = pytest.mark.gpu

COUNTERS = ("ao_traces", "active_traces", "distance_traces", "soft_distance_traces", "light_list_traces", "adaptive_traces",
            "soft_list_adaptive_traces", "soft_list_jitter_traces", "soft_light_list_traces", "sparse_list_traces",
            "soft_list_distance_traces", "alltable_traces", "follow_traces")


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


def _reset(ctx):
    ctx.set_option("kernel", -1)
    ctx.set_option("soft_split", 1)


def _form(ctx, kernel, split):
    ctx.set_option("kernel", kernel)
    ctx.set_option("soft_split", split)


@contextmanager
def _counted(ctx, launches):
    """"ao_traces" moves by `launches` inside the block and no other trace counter moves."""
    before = [ctx.get_option(c) for c in COUNTERS]
    yield
    after = [ctx.get_option(c) for c in COUNTERS]
    assert after == [before[0] + launches] + before[1:], dict(zip(COUNTERS, zip(before, after)))


class _Dev:
    """Positions, normals and a map on the device; the counts live inside a larger guarded block (as _Dev of test_gpu_ao.py)."""
    PAD = 256

    def __init__(self, ctx, pos, nrm):
        self.ctx = ctx
        pos, nrm = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(nrm, np.float32)
        self.H, self.W = pos.shape[:2]
        n = self.W * self.H
        self.d_pos, self.d_nrm, self.d_act, self.d_block = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n), ctx.malloc(n + 2 * self.PAD)
        self.d_counts = self.d_block + self.PAD
        ctx.h2d(self.d_pos, pos)
        ctx.h2d(self.d_nrm, nrm)
        self._fill = np.full(n + 2 * self.PAD, GUARD, np.uint8)

    def set_map(self, m):
        self.ctx.h2d(self.d_act, np.ascontiguousarray(m, np.uint8))

    def guard(self):
        self.ctx.h2d(self.d_block, self._fill)

    def read(self, stream=None):
        self.ctx.synchronize(stream)
        block = np.empty(self.W * self.H + 2 * self.PAD, np.uint8)
        self.ctx.d2h(block, self.d_block)
        assert (block[:self.PAD] == GUARD).all() and (block[-self.PAD:] == GUARD).all(), "a byte outside the plane was written"
        return block[self.PAD:-self.PAD].reshape(self.H, self.W)

    def close(self):
        for d in (self.d_pos, self.d_nrm, self.d_act, self.d_block):
            self.ctx.free(d)


def _trace(ctx, dev, k, ao, plane, what, name, active=None, rows=None, stream=None):
    """`plane`: the oracle's plane WITHOUT a map.  One launch, counted, named; rows outside the range keep the fill."""
    if active is not None:
        dev.set_map(active)
        plane = aec.under(plane, active)
    if rows is not None:
        inside = (np.arange(dev.H) >= rows[0]) & (np.arange(dev.H) < rows[1])
        plane = np.where(inside[:, None], plane, GUARD).astype(np.uint8)
    dev.guard()
    kw = {} if rows is None else {"row_begin": rows[0], "row_end": rows[1]}
    with _counted(ctx, 1):
        ctx.trace_ambient_occlusion_device(k, ao, dev.d_pos, dev.d_nrm, dev.W, dev.H, dev.d_counts, stream=stream,
                                           d_active=dev.d_act if active is not None else None, **kw)
    got = dev.read(stream)
    _same(got, plane, what)
    assert ctx.last_kernel_name() == name, (what, ctx.last_kernel_name())
    return got


# ---- a. the gate frame --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", aec.GATE_SETS, ids=str)
@pytest.mark.parametrize("kernel,split", aec.FORMS)
def test_gate_frame_on_edge_texels_and_wild_normals(ctx, kernel, split, key):
    """Every radius without a map, under the maps a, b, c (the first walker is an edge texel / a later walker is / only edge texels
    walk), under the lone pixel (every other tile takes the no-ray exit in all four waves) and under lane63."""
    g = aec.gate()
    aec.guard_gate_all()
    nrm, maps = aec.gate_normals(), aec.gate_maps()
    ctx.set_bvh(g.packed)
    dev = _Dev(ctx, g.pos, nrm)
    try:
        _form(ctx, kernel, split)
        for rname in aec.GATE_RADII:
            ao, plane = aec.gate_ao(key, aec.gate_radius(key, rname)), aec.gate_want(key, rname)
            _trace(ctx, dev, g.k, ao, plane, (kernel, split, key, rname), _name(kernel, split))
            for mname, m in maps.items():
                got = _trace(ctx, dev, g.k, ao, plane, (kernel, split, key, rname, mname), _name(kernel, split), active=m)
                if mname == "lone":
                    assert not np.delete(got.ravel(), aec.ON_TEXEL[0] * g.W + aec.ON_TEXEL[1]).any()
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel,split", aec.FORMS)
def test_gate_host_form_rows_hash_the_full_frame_index(ctx, kernel, split):
    """Rows (5, 61) travel as a frame of their own; the start of a pixel must still be hashed from its index in the caller's frame."""
    g = aec.gate()
    nrm, (r0, r1) = aec.gate_normals(), aec.HOST_ROWS
    plane = aec.gate_want((5, 8), "ordinary")
    assert int((aec.gate_rows_wrong() != plane[r0:r1]).sum()) >= aec.LEAST
    ao = aec.gate_ao((5, 8), aec.gate_radius((5, 8), "ordinary"))
    ctx.set_bvh(g.packed)
    try:
        _form(ctx, kernel, split)
        rows = (np.arange(g.H) >= r0) & (np.arange(g.H) < r1)
        for mname, m in (("whole", None), ("a", aec.gate_maps()["a"])):
            out = np.full((g.H, g.W), GUARD, np.uint8)
            with _counted(ctx, 1):
                ctx.trace_ambient_occlusion(g.k, ao, g.pos, nrm, g.W, g.H, row_begin=r0, row_end=r1, active=m, out=out)
            want = plane if m is None else aec.under(plane, m)
            _same(out, np.where(rows[:, None], want, GUARD).astype(np.uint8), (kernel, split, mname))
            assert ctx.last_kernel_name() == _name(kernel, split), ctx.last_kernel_name()
    finally:
        _reset(ctx)


# ---- b. the awkward streams ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", aec.STREAMS)
def test_awkward_streams(ctx, name):
    pos, k, _, (nrm, wants) = _stream(ctx, name, lambda packed, pos, k, point: aec.stream_wants(packed, k, pos, point, name))
    H, W = pos.shape[:2]
    m = (np.random.RandomState(11).rand(H, W) < 0.5).astype(np.uint8)     # where the plane is n everywhere, the map mixes 0 and n
    for _, plane in wants.values():
        marked = aec.under(plane, m)[aec.live(nrm)]
        assert (marked == 0).any() and (marked != 0).any(), name
    dev = _Dev(ctx, pos, nrm)
    try:
        for kernel, split in aec.FORMS:
            _form(ctx, kernel, split)
            for key, (ao, plane) in wants.items():
                _trace(ctx, dev, k, ao, plane, (name, kernel, split, key), _name(kernel, split))
                _trace(ctx, dev, k, ao, plane, (name, kernel, split, key, "map"), _name(kernel, split), active=m)
                _trace(ctx, dev, k, ao, plane, (name, kernel, split, key, "rows"), _name(kernel, split), rows=(5, H - 7))
    finally:
        _reset(ctx)
        dev.close()


# ---- c. around a refit --------------------------------------------------------------------------------------------------------------
def test_around_a_refit_that_drops_the_copy(ctx):
    """The recipe of test_lists_and_soft_distance_around_a_refit_that_drops_the_copy: finite vertices whose edge overflows to +Inf,
    then back; the oracle's plane is recomputed from the stream each refit returns."""
    c = aec.refit_case()
    wl, k = c["wl"], c["k"]

    def check(packed, what):
        plane = aec.refit_want(packed, what)
        for kernel, split in aec.FORMS:
            _form(ctx, kernel, split)
            _trace(ctx, dev, k, c["ao"], plane, (what, kernel, split), _name(kernel, split))

    aec.refit_want(wl.packed, "refit, before")           # (from the oracle, before any device call)
    ctx.set_bvh(wl.packed)
    dev = _Dev(ctx, c["pos"], c["nrm"])
    try:
        assert ctx.get_option("bvh_finite") == 1 and ctx.get_option("wide_nodes") > 0
        check(wl.packed, "refit, before")
        w = wl.vertices.copy()
        w[0, 0], w[1, 0] = np.float32(-3e38), np.float32(3e38)           # finite vertices whose edge overflows: e0.x = +Inf
        got, _, _ = api.bvh_refit_device(ctx, w, 8, wl.indices, wl.prim_count, want_packed=True)
        assert np.isinf(got[:, :3].view(np.float32)).any()
        assert ctx.get_option("bvh_finite") == 0 and ctx.get_option("wide_nodes") == 0
        check(got, "refit, edge overflow")
        back, _, _ = api.bvh_refit_device(ctx, wl.vertices, 8, wl.indices, wl.prim_count, want_packed=True)
        assert ctx.get_option("bvh_finite") == 1 and ctx.get_option("wide_nodes") > 0
        check(back, "refit, back")
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel,split", aec.FORMS)
def test_a_captured_trace_replayed_after_a_refit_in_place(ctx, kernel, split):
    """One kernel node captured on a second stream; the installed tree is then refitted in place to finitely moved vertices, and the
    replay walks the refitted tree: the oracle's plane on the returned stream, which differs from the captured-time plane."""
    c = aec.refit_case()
    wl, k, ao = c["wl"], c["k"], c["ao"]
    before = aec.refit_want(wl.packed, "capture, before")
    ctx.set_bvh(wl.packed)
    dev = _Dev(ctx, c["pos"], c["nrm"])
    stream = ctx.stream_create()
    g = None
    try:
        _form(ctx, kernel, split)
        _trace(ctx, dev, k, ao, before, (kernel, split, "eager"), _name(kernel, split), stream=stream)
        with _counted(ctx, 1):
            g = hipgraph.capture(stream, lambda: ctx.trace_ambient_occlusion_device(k, ao, dev.d_pos, dev.d_nrm, dev.W, dev.H, dev.d_counts,
                                                                                     stream=stream))
        assert g.node_types() == [hipgraph.KERNEL], g.node_types()
        assert ctx.last_kernel_name() == _name(kernel, split), ctx.last_kernel_name()
        dev.guard()
        g.launch(stream)
        _same(dev.read(stream), before, (kernel, split, "replay, before"))
        moved, _, _ = api.bvh_refit_device(ctx, c["moved"], 8, wl.indices, wl.prim_count, want_packed=True)
        after = aec.refit_want(moved, "capture, after")
        assert int((after != before).sum()) >= aec.LEAST
        ctx.synchronize()
        dev.guard()
        g.launch(stream)
        _same(dev.read(stream), after, (kernel, split, "replay, after the refit"))
    finally:
        if g is not None:
            g.close()
        ctx.synchronize(stream)
        ctx.stream_destroy(stream)
        _reset(ctx)
        dev.close()


# ---- d. more than 65 535 block rows: the 1-D grid -----------------------------------------------------------------------------------
@pytest.mark.parametrize("table", (0, aec.TALL_TABLE))
@pytest.mark.parametrize("kernel,split", aec.FORMS)
def test_tall_frames_take_the_one_dimensional_grid(ctx, kernel, split, table):
    """Whole, on the row range (3, H - 2) and once under a random 50 % map.  With the table the expectation is gathered per pixel with
    start(y * W + x, 6) from the numpy hash: a kernel that ignored the table, or hashed the index inside the row range, writes
    another plane -- asserted before anything is traced."""
    t = aec.tall_case()
    H, W = _tall_height(kernel), 3
    plane = aec.tall_want(t, table, H)
    aec.guard_some(plane, 3, ("tall", table))
    if table:
        inside = slice(3, H - 2)
        assert int((plane[inside] != aec.tall_untabled(t, H)[inside]).sum()) >= aec.LEAST
        assert int((plane[inside] != aec.tall_want(t, table, H, wrong_base=3 * W)[inside]).sum()) >= aec.LEAST
    m = (np.random.RandomState(H + split).rand(H, W) < 0.5).astype(np.uint8)
    aec.guard_map(plane, m, ("tall, map", table))
    ao = t["ao6"] if table else t["ao0"]
    ctx.set_bvh(t["wl"].packed)
    dev = _Dev(ctx, aec.tall_positions(t["texels"], H), aec.tall_positions(t["nrm"], H))
    try:
        _form(ctx, kernel, split)
        name = _name(kernel, split, "general")
        _trace(ctx, dev, t["k"], ao, plane, ("tall", kernel, split, table), name)
        _trace(ctx, dev, t["k"], ao, plane, ("tall", kernel, split, table, "rows"), name, rows=(3, H - 2))
        _trace(ctx, dev, t["k"], ao, plane, ("tall", kernel, split, table, "map"), name, active=m)
    finally:
        _reset(ctx)
        dev.close()


# ---- e. the family threshold and wide frames ----------------------------------------------------------------------------------------
def _wide(ctx, W, H):
    t = aec.tall_case()
    plane = aec.tall_want(t, 0, H, W)
    aec.guard_some(plane, 3, ("wide", W, H))
    ctx.set_bvh(t["wl"].packed)
    return t, plane, _Dev(ctx, aec.tall_positions(t["texels"], H, W), aec.tall_positions(t["nrm"], H, W))


def test_default_family_switches_at_two_to_the_eighteen_pixels(ctx):
    """kernel = -1: 2064 x 128 = 264 192 pixels take the packet family (four waves, or one with soft_split 0), 2064 x 127 and the
    rows (0, 127) of the big frame -- rows * W below 2^18 -- the lane-per-ray family."""
    packet = "ambientOcclusionPacketKernel<%d,rows>"
    for H in (128, 127):
        t, plane, dev = _wide(ctx, 2064, H)
        try:
            _reset(ctx)
            assert (2064 * H >= 1 << 18) == (H == 128)
            _trace(ctx, dev, t["k"], t["ao0"], plane, ("threshold", H), packet % 4 if H == 128 else SHARE)
            if H == 128:
                _trace(ctx, dev, t["k"], t["ao0"], plane, ("threshold", H, "rows"), SHARE, rows=(0, 127))
                ctx.set_option("soft_split", 0)
                _trace(ctx, dev, t["k"], t["ao0"], plane, ("threshold", H, "one wave"), packet % 1)
        finally:
            _reset(ctx)
            dev.close()


@pytest.mark.parametrize("W,H", [(2064, 8), (8, 2064)])
def test_wide_and_narrow_frames(ctx, W, H):
    t, plane, dev = _wide(ctx, W, H)
    try:
        for kernel, split in aec.FORMS:
            _form(ctx, kernel, split)
            _trace(ctx, dev, t["k"], t["ao0"], plane, (W, H, kernel, split), _name(kernel, split))
    finally:
        _reset(ctx)
        dev.close()


# ---- f. options that must not matter, and must survive ------------------------------------------------------------------------------
def test_every_kernel_value_takes_the_family_blockFamily_documents(ctx):
    """Share for 7 and for the values below the packet kernels, packet for the rest, 8 and 9 included; -1 by the pixel count."""
    t, plane, dev = _wide(ctx, 61, 37)
    try:
        assert ctx.get_option("kernel_count") == 10
        for kernel in range(-1, ctx.get_option("kernel_count")):
            for split in (1, 0):
                _form(ctx, kernel, split)
                packet = kernel >= 3 and kernel != 7
                _trace(ctx, dev, t["k"], t["ao0"], plane, ("family", kernel, split), _name(3 if packet else 7, split))
        for bad in (-2, 10):
            with pytest.raises(api.RtsError):
                ctx.set_option("kernel", bad)
    finally:
        _reset(ctx)
        dev.close()


WHOLE = dict(min_life_us=1e9, piece_us=1e9, front_share=1.0)          # a whole-dispatch table without pieces (tests/test_gpu_alltable.py)
PIECES = dict(min_life_us=4.0, piece_us=2.0, max_pieces=8, front_share=1.0 / 3.0)
TABLE_KEYS = ("split_tiles", "front_tiles", "split_pieces", "tile_splits", "tile_order_tiles", "tile_order", "tile_order_planned")
OPTION_KEYS = ("xcd_swizzle", "packet_budget", "packet_share", "block_waves", "row_order", "wide_lane", "tile_splits", "tile_order", "follow")


class _Options:
    """The 256 x 256 cornell frame of the tall case on the device, the plain mask trace beside the AO trace."""

    def __init__(self, ctx):
        self.ctx, self.t = ctx, aec.tall_case()
        t = self.t
        self.wl, self.k, self.W, self.H = t["wl"], t["k"], 256, 256
        self.mask = aec.oracle.shadow_mask(self.wl.packed, self.k.as_array(), aec.oracle.light_from_product(self.wl.light, self.k), t["texels"],
                                           self.W, self.H)[0]
        assert 0 < int(self.mask.sum()) < self.mask.size
        ctx.set_bvh(self.wl.packed)
        assert ctx.get_option("wide_nodes") > 0
        self.dev = _Dev(ctx, t["texels"], t["nrm"])
        self.d_mask = ctx.malloc(self.W * self.H)
        self.defaults = dict({o: ctx.get_option(o) for o in OPTION_KEYS}, wave_stats=0, clock_probe=0)
        self.waves, self.rows = ((self.W + 7) // 8) * ((self.H + 7) // 8), (self.H + 7) // 8
        self.settings = (("row_order", 1), ("row_order", 2), ("xcd_swizzle", 1), ("block_waves", 4), ("wide_lane", 1), ("packet_budget", 1),
                         ("packet_budget", 4096), ("tile_splits", 0), ("follow", 1), ("wave_stats", self.waves), ("clock_probe", self.rows))

    def installed(self):
        """What is installed: the table's sizes, the order's, and the table's records themselves."""
        state = {o: self.ctx.get_option(o) for o in TABLE_KEYS}
        pieces = state["split_pieces"]
        records = self.ctx.read_piece_stats(pieces, clocks=False)[0].tobytes() if pieces else b""
        return state, records

    def ao_trace(self, what, plain_kernel, geom="rows"):
        """The three forms under the options as they stand: the oracle's bytes, and nothing installed dropped or altered."""
        before = self.installed(), {o: self.ctx.get_option(o) for o in OPTION_KEYS}
        for kernel, split in aec.FORMS:
            _form(self.ctx, kernel, split)
            _trace(self.ctx, self.dev, self.k, self.t["ao0"], self.t["plane0"], (what, kernel, split), _name(kernel, split, geom))
        _form(self.ctx, plain_kernel, 1)
        assert (self.installed(), {o: self.ctx.get_option(o) for o in OPTION_KEYS}) == before, what

    def plain_trace(self):
        """The plain mask trace: the oracle's bytes -> (kernel name, ALLTABLE launches it added)."""
        ctx = self.ctx
        n0 = ctx.get_option("alltable_traces")
        ctx.h2d(self.d_mask, np.full(self.W * self.H, GUARD, np.uint8))
        ctx.trace_shadow_mask_device(self.k, self.dev.d_pos, self.W, self.H, self.d_mask, light=self.wl.light)
        ctx.synchronize()
        got = np.empty((self.H, self.W), np.uint8)
        ctx.d2h(got, self.d_mask)
        _same(got, self.mask, "plain")
        return ctx.last_kernel_name(), ctx.get_option("alltable_traces") - n0

    def reads_back(self, o, v):
        if o == "wave_stats":                            # write-only: the records are there, and no AO trace wrote one
            assert not self.ctx.read_wave_stats(v).any()
        elif o == "clock_probe":
            self.ctx.clock_probe_mhz(v)
            assert not self.ctx.last_clock_probe.any()
        else:
            assert self.ctx.get_option(o) == v, (o, v)

    def close(self):
        ctx = self.ctx
        for o in ("wave_stats", "clock_probe", "follow"):
            ctx.set_option(o, 0)
        ctx.set_tile_order(None)
        ctx.clear_splits()
        for o in OPTION_KEYS:
            ctx.set_option(o, self.defaults[o])
        _reset(ctx)
        ctx.free(self.d_mask)
        self.dev.close()


@pytest.mark.parametrize("what", ["whole table", "table with pieces", "tile order"])
def test_options_are_ignored_and_what_is_installed_is_kept(ctx, what):
    """A whole-dispatch split table under kernel 8, a split table with pieces under kernel 3, or a caller's tile order (an order makes
    the grid one-dimensional, where no table applies: the two cannot be installed together) stays installed through EVERY setting.
    After each non-default option: the AO bytes are the oracle's in the three forms; the table's sizes and records and the order's
    size are unchanged and non-zero; the option reads back as set; the plain trace under the option still writes the oracle's mask;
    and with the option back at its default the plain trace takes the whole-dispatch table again -- "alltable_traces", which only a
    launch that reads that table moves, moves as it did before the AO calls.  (A table with pieces and a tile order have no such
    counter: their sizes and records are what is held.)"""
    o_ = _Options(ctx)
    try:
        kernel = 8 if what == "whole table" else 3
        _form(ctx, kernel, 1)
        if what == "tile order":
            order = np.arange(o_.waves, dtype=np.uint32)[::-1].copy()
            ctx.set_tile_order(order)
            assert ctx.get_option("tile_order_tiles") == order.size and ctx.get_option("tile_order") == 1
        else:
            tiles, records = ctx.plan_splits(o_.k, o_.dev.d_pos, o_.W, o_.H, o_.d_mask, light=o_.wl.light, **(WHOLE if kernel == 8 else PIECES))
            assert ctx.get_option("split_pieces") > 0
            if kernel == 8:
                assert ctx.get_option("front_tiles") == o_.waves and ctx.get_option("split_tiles") == 0     # every tile a record, no piece
            else:
                assert tiles > 0 and records > 0 and ctx.get_option("split_tiles") > 0
        uses = 1 if kernel == 8 else 0
        first = o_.installed()
        name_before, took = o_.plain_trace()
        assert took == uses
        o_.ao_trace(what, kernel)                        # (natural order on the 2-D grid, whatever order is installed)
        assert o_.plain_trace() == (name_before, uses)
        for o, v in o_.settings:
            ctx.set_option(o, v)
            o_.ao_trace((what, o, v), kernel, "general" if o == "xcd_swizzle" else "rows")         # (the swizzled grid is 1-D)
            o_.reads_back(o, v)
            o_.plain_trace()
            ctx.set_option(o, o_.defaults[o])
            assert o_.installed() == first, (what, o, v)
            assert o_.plain_trace() == (name_before, uses), (what, o, v)
    finally:
        o_.close()


def test_follow_mode_and_the_diagnostics_are_ignored_and_kept(ctx):
    """Nothing installed.  Follow mode: an AO trace moves neither "follow_traces" nor "follow_ordered", and the plain trace
    afterwards runs the followed kernel and moves the counter again.  Wave statistics and the clock probe: an AO trace leaves the
    records as it found them, the plain trace still fills them."""
    o_ = _Options(ctx)
    try:
        _form(ctx, 3, 1)
        ctx.set_option("follow", 1)
        o_.plain_trace()
        name_follow, _ = o_.plain_trace()
        assert name_follow.startswith("shadowMaskFollowKernel<")
        traces, ordered = ctx.get_option("follow_traces"), ctx.get_option("follow_ordered")
        o_.ao_trace("follow", 3)
        assert (ctx.get_option("follow_traces"), ctx.get_option("follow_ordered"), ctx.get_option("follow")) == (traces, ordered, 1)
        assert o_.plain_trace()[0] == name_follow and ctx.get_option("follow_traces") == traces + 1
        assert ctx.get_option("follow_ordered") == ordered + 1
        ctx.set_option("follow", 0)
        ctx.set_option("wave_stats", o_.waves)
        o_.ao_trace("wave_stats", 3)
        o_.reads_back("wave_stats", o_.waves)
        o_.plain_trace()
        assert ctx.read_wave_stats(o_.waves).any()
        ctx.set_option("wave_stats", 0)
        ctx.set_option("clock_probe", o_.rows)
        o_.ao_trace("clock_probe", 3)
        o_.reads_back("clock_probe", o_.rows)
        o_.plain_trace()
        ctx.clock_probe_mhz(o_.rows)
        assert ctx.last_clock_probe.any()
        ctx.set_option("clock_probe", 0)
    finally:
        o_.close()
