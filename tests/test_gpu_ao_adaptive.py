"""GPU: adaptive ambient occlusion traces (rts_trace_ambient_occlusion_adaptive*; include/rts.h) against the host twin
(rtsh_ambient_occlusion_adaptive, which tests/test_ao_adaptive_host.py pins to the oracle), byte for byte in counts AND refined on
guarded, preset buffers: the 67 x 45 and 40 x 24 frames of tests/ao_adaptive_cases.py in the lane-per-ray family ("kernel" 0) and the
packet family ("kernel" 3) with "soft_split" 0 and 1; every (n, k) pair with table 0 and 64; tiles without a ray, tiles whose probe is
unanimous, a tile whose only refining pixel is its last lane; a row range and stripes; refined = None; the host form; graph capture;
the counters and kernel names; an installed split table and tile order; every refusal."""
import ctypes as C

import numpy as np
import pytest

import ao_adaptive_cases as aa
import hipgraph
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = aa.GUARD
SHARE_NAME = "ambientOcclusionAdaptiveShareKernel"
FORMS = [(0, 1), (0, 0), (3, 1), (3, 0)]             # ("kernel", "soft_split")


def _name(kernel, split, geom="rows"):
    return SHARE_NAME if kernel == 0 else "ambientOcclusionAdaptivePacketKernel<%d,%s>" % (4 if split else 1, geom)


def _form(ctx, kernel, split):
    ctx.set_option("kernel", kernel)
    ctx.set_option("soft_split", split)


def _reset(ctx):
    ctx.set_option("kernel", -1)
    ctx.set_option("soft_split", 1)


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    _reset(c)
    c.close()


class _Dev:
    """The frame on the device; counts and refined live inside one larger guarded block."""
    PAD = 256

    def __init__(self, ctx, fr, active=None):
        self.ctx, self.W, self.H = ctx, fr.W, fr.H
        n = fr.W * fr.H
        self.size = 2 * n + 3 * self.PAD
        self.d_pos, self.d_nrm, self.d_block = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(self.size)
        self.d_act = ctx.malloc(n) if active is not None else None
        self.d_counts = self.d_block + self.PAD
        self.d_ref = self.d_block + 2 * self.PAD + n
        ctx.h2d(self.d_pos, np.ascontiguousarray(aa.dirty(fr, active)))
        ctx.h2d(self.d_nrm, np.ascontiguousarray(fr.nrm))
        if active is not None:
            ctx.h2d(self.d_act, np.ascontiguousarray(active))

    def guard(self):
        self.ctx.h2d(self.d_block, np.full(self.size, GUARD, np.uint8))

    def read(self, stream=None):
        self.ctx.synchronize(stream)
        block = np.empty(self.size, np.uint8)
        self.ctx.d2h(block, self.d_block)
        n, P = self.W * self.H, self.PAD
        assert (block[:P] == GUARD).all() and (block[P + n:2 * P + n] == GUARD).all() and (block[2 * P + 2 * n:] == GUARD).all(), \
            "a byte outside the planes was written"
        return block[P:P + n].reshape(self.H, self.W), block[2 * P + n:2 * P + 2 * n].reshape(self.H, self.W)

    def close(self):
        for d in (self.d_pos, self.d_nrm, self.d_block, self.d_act):
            if d is not None:
                self.ctx.free(d)


def _same(got, want, what, rows=None, refined=True):
    for name, g, w in (("counts", got[0], want[0]), ("refined", got[1], want[1])):
        if rows is not None:
            w = np.where(rows[:, None], w, GUARD).astype(np.uint8)
        if name == "refined" and not refined:
            w = np.full_like(w, GUARD)
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, name, bad.shape[0], bad[:4].tolist(), [int(g[tuple(b)]) for b in bad[:4]], [int(w[tuple(b)]) for b in bad[:4]])


def _trace(ctx, dev, fr, ao, k, want, what, rows=None, refined=True, **kw):
    dev.guard()
    ctx.trace_ambient_occlusion_adaptive_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts, k,
                                                d_refined=dev.d_ref if refined else None, d_active=dev.d_act, **kw)
    _same(dev.read(kw.get("stream")), want, what, rows, refined)


@pytest.fixture(scope="module", params=aa.FRAMES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}")
def fr(request):
    return aa.frame(*request.param)


def test_device_equals_the_twin_on_every_pair_in_every_form(ctx, fr):
    """Every (n, k) with table 0 and 64 at the main radius (all three branches: the guard of the host test), in both families and both
    splits; (2, 1), (3, 1), (5, 4) and (4, 3) leave waves of the four-wave form without a sample in one phase."""
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    try:
        for n, k in aa.PAIRS:
            for table in (0, 64):
                ao, want = fr.ao(n, table, aa.SHARE), aa.want(fr, n, k, table)
                for kernel, split in FORMS:
                    _form(ctx, kernel, split)
                    _trace(ctx, dev, fr, ao, k, want, (fr.name, fr.W, fr.H, n, k, table, kernel, split))
                    assert ctx.last_kernel_name() == _name(kernel, split), (kernel, split, ctx.last_kernel_name())
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("which", ["mixed", "dead", "lonely", "unanimous"])
def test_tiles_without_a_ray_unanimous_tiles_and_a_lonely_refining_lane(ctx, fr, which):
    """mixed: whole inactive tiles over NaN positions (the no-ray exit in all four waves).  dead: the 16 x 16 block at the origin.
    unanimous: a small radius, whole tiles end between the barriers.  lonely: one tile's only refining pixel is its last lane where
    such a tile exists -- the first refining lane, every other lane stands in for it."""
    n, k, table, share = (5, 4, 0, aa.SHARE) if which == "dead" else (16, 4, 64, 0.05 if which == "unanimous" else aa.SHARE)
    active = {"mixed": fr.active, "dead": aa.dead_block(fr), "lonely": aa.lonely(fr, n, k, table)[0] if which == "lonely" else None,
              "unanimous": None}[which]
    want = aa.want(fr, n, k, table, share, active, None if active is None else which)
    dead, unanimous, refining = aa.tile_classes(want[1], aa.live_of(fr, active))
    assert refining >= 1 and (which not in ("mixed", "dead") or dead >= 1) and (which != "unanimous" or unanimous >= 1)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr, active)
    try:
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            _trace(ctx, dev, fr, fr.ao(n, table, share), k, want, (which, fr.W, fr.H, kernel, split))
            _trace(ctx, dev, fr, fr.ao(n, table, share), k, want, (which, fr.W, fr.H, kernel, split, "no refined"), refined=False)
    finally:
        _reset(ctx)
        dev.close()


def test_rows_stripes_the_host_form_and_the_counters(ctx):
    fr = aa.frame("cornell_128", 67, 45)
    n, k, table = 16, 4, 64
    ao, want = fr.ao(n, table, aa.SHARE), aa.want(fr, n, k, table)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    counters = ("ao_adaptive_traces", "ao_traces", "adaptive_traces")
    try:
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            for r0, r1 in ((5, 37), (9, 10), (7, 7)):
                rows = (np.arange(fr.H) >= r0) & (np.arange(fr.H) < r1)
                before = [ctx.get_option(c) for c in counters]
                _trace(ctx, dev, fr, ao, k, want, (kernel, split, r0, r1), rows=rows, row_begin=r0, row_end=r1)
                assert [ctx.get_option(c) for c in counters] == [before[0] + (1 if r1 > r0 else 0), before[1], before[2]]
            band, geom = (16, None) if kernel == 0 else (8, "bands")
            total = [np.full((fr.H, fr.W), GUARD, np.uint8), np.full((fr.H, fr.W), GUARD, np.uint8)]
            for s in range(3):
                own = (np.arange(fr.H) // band) % 3 == s
                dev.guard()
                ctx.trace_ambient_occlusion_adaptive_stripes_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts, band, 3, s, k,
                                                                    d_refined=dev.d_ref)
                got = dev.read()
                _same(got, want, (kernel, split, band, s), rows=own)
                assert ctx.last_kernel_name() == _name(kernel, split, geom)
                total[0][own], total[1][own] = got[0][own], got[1][own]
            _same(total, want, (kernel, split, "all stripes"))
            # a stripe that owns no band launches nothing, writes nothing and returns RTS_OK
            before = ctx.get_option("ao_adaptive_traces")
            dev.guard()
            ctx.trace_ambient_occlusion_adaptive_stripes_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts, 32, 3, 2, k,
                                                                d_refined=dev.d_ref)
            got = dev.read()
            assert (got[0] == GUARD).all() and (got[1] == GUARD).all() and ctx.get_option("ao_adaptive_traces") == before
            # the host form stages rows 5..37 as a frame of their own: its pixel 0 is pixel 5 * W of the caller's frame
            out, ref = np.full((fr.H, fr.W), GUARD, np.uint8), np.full((fr.H, fr.W), GUARD, np.uint8)
            ctx.trace_ambient_occlusion_adaptive(fr.k, ao, fr.pos, fr.nrm, fr.W, fr.H, k, row_begin=5, row_end=37, out=out, refined=ref)
            _same((out, ref), want, (kernel, split, "host rows"), rows=(np.arange(fr.H) >= 5) & (np.arange(fr.H) < 37))
            alone, none = ctx.trace_ambient_occlusion_adaptive(fr.k, ao, fr.pos, fr.nrm, fr.W, fr.H, k, want_refined=False)
            assert none is None and np.array_equal(alone, want[0])
        with pytest.raises(api.RtsError):                                # a band that is no whole number of block rows
            ctx.trace_ambient_occlusion_adaptive_stripes_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts, 12, 2, 0, k)
        ctx.set_option("kernel", -1)
        _trace(ctx, dev, fr, ao, k, want, "defaults")
        assert ctx.last_kernel_name() == SHARE_NAME                      # below 256 K pixels: the lane-per-ray family
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel,split", [(0, 1), (3, 1), (3, 0)])
def test_capture_adds_one_kernel_node_and_replays_the_captured_parameters(ctx, kernel, split):
    fr = aa.frame("cornell_128", 40, 24)
    n, k, table = 16, 4, 64
    want = aa.want(fr, n, k, table)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    stream = ctx.stream_create()
    g = None
    try:
        _form(ctx, kernel, split)
        _trace(ctx, dev, fr, fr.ao(n, table, aa.SHARE), k, want, (kernel, split, "stream"), stream=stream)
        ao = fr.ao(n, table, aa.SHARE)
        before = ctx.get_option("ao_adaptive_traces")
        g = hipgraph.capture(stream, lambda: ctx.trace_ambient_occlusion_adaptive_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, fr.H,
                                                                                          dev.d_counts, k, d_refined=dev.d_ref, stream=stream))
        assert g.node_types() == [hipgraph.KERNEL]
        assert ctx.get_option("ao_adaptive_traces") == before + 1
        # the host struct is overwritten and the options changed: the graph holds what was captured
        C.memset(C.byref(ao), 0xFF, C.sizeof(ao))
        ctx.set_option("kernel", 3 if kernel == 0 else 0)
        for replay in range(2):
            dev.guard()
            g.launch(stream)
            _same(dev.read(stream), want, (kernel, split, "replay", replay))
    finally:
        if g is not None:
            g.close()
        ctx.stream_destroy(stream)
        _reset(ctx)
        dev.close()


def test_an_installed_split_table_and_tile_order_stay_and_change_no_byte(ctx):
    fr = aa.frame("cornell_128", 67, 45)
    n, k, table = 16, 4, 64
    ao, want = fr.ao(n, table, aa.SHARE), aa.want(fr, n, k, table)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    keys = ("split_tiles", "front_tiles", "split_pieces", "tile_splits", "tile_order_tiles", "tile_order", "tile_order_planned", "follow",
            "block_waves", "wide_lane", "ao_traces", "adaptive_traces")
    try:
        ctx.set_option("kernel", 8)
        ctx.plan_splits(fr.k, dev.d_pos, fr.W, fr.H, dev.d_counts, min_life_us=1e9, piece_us=1e9, front_share=1.0)   # every tile a record
        assert ctx.get_option("front_tiles") > 0
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            state = [ctx.get_option(key) for key in keys]
            _trace(ctx, dev, fr, ao, k, want, (kernel, split, "split table"))
            assert ctx.last_kernel_name() == _name(kernel, split) and [ctx.get_option(key) for key in keys] == state
        ctx.clear_splits()
        tiles = ((fr.W + 7) // 8) * ((fr.H + 7) // 8)
        ctx.set_tile_order(np.arange(tiles, dtype=np.uint32)[::-1].copy())
        assert ctx.get_option("tile_order_tiles") == tiles and ctx.get_option("tile_order") == 1
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            state = [ctx.get_option(key) for key in keys]
            _trace(ctx, dev, fr, ao, k, want, (kernel, split, "tile order"))
            assert ctx.last_kernel_name() == _name(kernel, split) and [ctx.get_option(key) for key in keys] == state
    finally:
        ctx.set_tile_order(None)
        ctx.clear_splits()
        _reset(ctx)
        dev.close()


def test_refusals_leave_the_buffers_and_the_counters_alone(ctx):
    fr = aa.frame("cornell_128", 40, 24)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    good = fr.ao(4, 0, 0.5)

    def bad(**fields):
        a = fr.ao(4, 0, 0.5)
        for name, v in fields.items():
            setattr(a, name, v)
        return a

    def call(K=fr.k, A=good, X=dev.d_pos, N=dev.d_nrm, O=dev.d_counts, W=fr.W, H=fr.H, r0=0, r1=fr.H, probe=2):
        return api._lib.rts_trace_ambient_occlusion_adaptive_device(ctx.handle, C.byref(K) if K is not None else None,
                                                                    C.byref(A) if A is not None else None, C.c_void_p(X), C.c_void_p(N), None,
                                                                    W, H, r0, r1, probe, C.c_void_p(O), C.c_void_p(dev.d_ref), None)

    counters = ("ao_adaptive_traces", "ao_traces", "adaptive_traces")
    try:
        dev.guard()
        before = [ctx.get_option(c) for c in counters]
        for kw in (dict(K=None), dict(A=None), dict(X=0), dict(N=0), dict(O=0), dict(W=0), dict(H=0), dict(r0=3, r1=2), dict(r1=fr.H + 1),
                   dict(A=bad(nsamples=49), probe=4), dict(A=bad(table=3)), dict(A=bad(table=65)), dict(A=bad(nsamples=1, table=1)),
                   dict(A=bad(radius=np.inf)), dict(A=bad(radius=np.nan)), dict(A=bad(nsamples=1), probe=1), dict(A=bad(nsamples=0), probe=1),
                   dict(probe=0), dict(probe=4), dict(probe=5), dict(A=bad(nsamples=48), probe=48)):
            assert call(**kw) == aa.INVALID, kw
        host, href = np.full((fr.H, fr.W), GUARD, np.uint8), np.full((fr.H, fr.W), GUARD, np.uint8)
        for a, probe in ((None, 2), (bad(nsamples=49), 2), (bad(radius=np.nan), 2), (good, 0), (good, 4), (bad(nsamples=1), 1)):
            with pytest.raises(api.RtsError):
                ctx.trace_ambient_occlusion_adaptive(fr.k, a, fr.pos, fr.nrm, fr.W, fr.H, probe, out=host, refined=href)
        with pytest.raises(api.RtsError):
            ctx.trace_ambient_occlusion_adaptive_stripes_device(fr.k, good, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts, 8, 2, 2, 2)
        got = dev.read()
        assert (host == GUARD).all() and (href == GUARD).all() and (got[0] == GUARD).all() and (got[1] == GUARD).all()
        assert [ctx.get_option(c) for c in counters] == before
        with pytest.raises(api.RtsError):
            ctx.set_option("ao_adaptive_traces", 0)                      # get-only
        assert call() == 0
        _same(dev.read(), aa.want(fr, 4, 2, 0, 0.5), "the good call")
        assert [ctx.get_option(c) for c in counters] == [before[0] + 1, before[1], before[2]]
    finally:
        dev.close()
