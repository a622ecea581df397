"""GPU: the ALLTABLE instantiation of the wide packet kernel -- a whole-dispatch table without pieces runs
the instantiation whose waves read their record and the context's per-scene constants (the root box and
the fast set-up's bounds from it) instead of deciding table forms and deriving the bounds per wave.

Every mask is compared with the oracle's on a pre-filled mask buffer: small and ragged frames, the table forms and the launches
that must keep their old kernels, refits that move the root box across powers of two (eager and as a replayed graph), texels that
fail the fast set-up, and two contexts with different streams traced alternately."""
import numpy as np
import pytest

import hipgraph
import oracle
from raytracedshadows_amd import api, workloads

pytestmark = pytest.mark.gpu

WIDE = "shadowMaskPacketKernel<1,wide>"       # every instantiation of kernel 8 reports this name; "alltable_traces" counts the new one's launches
SIZES = [(8, 8), (72, 40), (200, 120), (67, 45)]          # one tile; several blocks; more; ragged: edge lanes without a pixel
WHOLE = dict(min_life_us=1e9, piece_us=1e9, front_share=1.0)
FILL = 77


@pytest.fixture(scope="module")
def frames():
    """cornell (1024 triangles, point light) at every size, with the oracle's mask: computed once, never changed."""
    out = {}
    for W, H in SIZES:
        wl = workloads.prepare("cornell", W, H, via_obj=False)
        wl.want = _want(wl, wl.packed, wl.positions)
        out[(W, H)] = wl
    return out


def _want(wl, packed, positions):
    want, _, _ = oracle.shadow_mask(packed, wl.constants.as_array(), oracle.light_from_product(wl.light, wl.constants), positions, wl.W, wl.H)
    return want


class _Dev:
    def __init__(self, ctx, wl, positions=None):
        self.ctx, self.wl = ctx, wl
        pos = np.ascontiguousarray(wl.positions if positions is None else positions)
        self.d_pos, self.d_mask = ctx.malloc(pos.nbytes), ctx.malloc(wl.W * wl.H)
        ctx.h2d(self.d_pos, pos)

    def trace(self, stream=None, alltable=None):
        """One trace into the pre-filled mask; alltable True / False: it must (not) have run the ALLTABLE instantiation."""
        wl = self.wl
        before = self.ctx.get_option("alltable_traces")
        self.ctx.h2d(self.d_mask, np.full(wl.W * wl.H, FILL, np.uint8))
        self.ctx.trace_shadow_mask_device(wl.constants, self.d_pos, wl.W, wl.H, self.d_mask, light=wl.light, stream=stream)
        assert self.ctx.last_kernel_name() == WIDE
        if alltable is not None:
            assert self.ctx.get_option("alltable_traces") - before == (1 if alltable else 0), ("alltable", alltable)
        return self.read(stream)

    def read(self, stream=None):
        self.ctx.synchronize(stream)
        got = np.empty((self.wl.H, self.wl.W), np.uint8)
        self.ctx.d2h(got, self.d_mask)
        return got

    def plan(self, **kw):
        wl = self.wl
        return self.ctx.plan_splits(wl.constants, self.d_pos, wl.W, wl.H, self.d_mask, light=wl.light, **kw)

    def close(self):
        self.ctx.free(self.d_pos)
        self.ctx.free(self.d_mask)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:4].tolist())


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_whole_dispatch_tables_run_alltable_and_the_others_their_old_kernels(frames, size):
    wl = frames[size]
    tiles_all = ((wl.W + 7) // 8) * ((wl.H + 7) // 8)
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        ctx.set_option("kernel", 8)
        dev = _Dev(ctx, wl)
        try:
            _same(dev.trace(alltable=False), wl.want, "no table")
            for square in (0, 32):
                for block in (0, 16):
                    tiles, records = dev.plan(xcd_square=square, life_block=block, **WHOLE)
                    assert ctx.get_option("front_tiles") == tiles_all and ctx.get_option("split_tiles") == 0, (square, block, tiles, records)
                    _same(dev.trace(alltable=True), wl.want, ("whole-dispatch table", square, block))
            # a table with pieces: every tile long enough to be split in two
            dev.plan(min_life_us=1e-3, piece_us=5e-4, max_pieces=2, front_share=1.0)
            assert ctx.get_option("split_tiles") > 0
            _same(dev.trace(alltable=False), wl.want, "table with pieces")
            ctx.clear_splits()
            _same(dev.trace(alltable=False), wl.want, "table cleared")
        finally:
            dev.close()


def _moved(wl, x):
    """The scene's vertices with the one of largest x moved out to x: the root box's upper x bound becomes x."""
    w = wl.vertices.copy()
    w[int(np.argmax(w[:, 0])), 0] = np.float32(x)
    return w


# 3e7 lies in [2^24, 2^25) and 7e7 in [2^26, 2^27): the root crosses powers of two on x, in the range (beyond 2^22) where the
# fast set-up's bound on that axis follows the root's exponent
ROOTS = (3e7, 7e7)


def test_a_refit_that_moves_the_root_box_updates_the_constants(frames):
    wl = frames[(72, 40)]
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        ctx.set_option("kernel", 8)
        dev = _Dev(ctx, wl)
        try:
            dev.plan(xcd_square=32, life_block=16, **WHOLE)
            _same(dev.trace(alltable=True), wl.want, "installed")
            for x in ROOTS:
                packed, _, _ = api.bvh_refit_device(ctx, _moved(wl, x), 8, wl.indices, wl.prim_count, want_packed=True)
                assert packed[1, 0:1].view(np.float32)[0] == np.float32(x)          # node 0's bboxMax.x
                _same(dev.trace(alltable=True), _want(wl, packed, wl.positions), ("refit", x))
            packed, _, _ = api.bvh_refit_device(ctx, wl.vertices, 8, wl.indices, wl.prim_count, want_packed=True)
            _same(dev.trace(alltable=True), wl.want, "refit back")
        finally:
            dev.close()


def test_a_captured_trace_replayed_after_a_refit_sees_the_refitted_root(frames):
    """The constants live in device memory, like the stream: a graph captured before a refit traces the refitted geometry."""
    wl = frames[(72, 40)]
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        ctx.set_option("kernel", 8)
        dev = _Dev(ctx, wl)
        stream = ctx.stream_create()
        g = None
        try:
            dev.plan(xcd_square=32, life_block=16, **WHOLE)
            _same(dev.trace(stream, alltable=True), wl.want, "first trace on the stream (the table's state for it)")
            before = ctx.get_option("alltable_traces")
            g = hipgraph.capture(stream, lambda: ctx.trace_shadow_mask_device(wl.constants, dev.d_pos, wl.W, wl.H, dev.d_mask, light=wl.light,
                                                                              stream=stream))
            assert ctx.get_option("alltable_traces") == before + 1 and g.node_types() == [hipgraph.KERNEL]
            ctx.h2d(dev.d_mask, np.full(wl.W * wl.H, FILL, np.uint8))
            g.launch(stream)
            _same(dev.read(stream), wl.want, "replay")
            for x in ROOTS:
                packed, _, _ = api.bvh_refit_device(ctx, _moved(wl, x), 8, wl.indices, wl.prim_count, want_packed=True)
                ctx.h2d(dev.d_mask, np.full(wl.W * wl.H, FILL, np.uint8))
                g.launch(stream)
                _same(dev.read(stream), _want(wl, packed, wl.positions), ("replay after a refit", x))
        finally:
            if g:
                g.close()
            ctx.synchronize(stream)
            ctx.stream_destroy(stream)
            dev.close()


def test_texels_that_fail_the_fast_set_up_take_the_general_path(frames):
    """One texel per tile that the one-gate set-up refuses (0, a denormal, 1e38): the wave sets its rays up the general way and
    leaves through the inexact-ray exit, which opens the node stream inside the ALLTABLE instantiation."""
    wl = frames[(200, 120)]
    pos = wl.positions.copy()
    values = (np.float32(0.0), np.float32(1e-40), np.float32(1e38))
    n = 0
    for ty in range(0, wl.H, 8):
        for tx in range(0, wl.W, 8):
            y, x = min(ty + 3, wl.H - 1), min(tx + 5, wl.W - 1)
            pos[y, x, :3] = values[n % 3]
            n += 1
    want = _want(wl, wl.packed, pos)
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        ctx.set_option("kernel", 8)
        dev = _Dev(ctx, wl, positions=pos)
        try:
            dev.plan(xcd_square=32, life_block=16, **WHOLE)
            _same(dev.trace(alltable=True), want, "bad texels")
        finally:
            dev.close()


def test_two_contexts_keep_their_own_constants(frames):
    wl = frames[(67, 45)]
    far = api.BVHBuilder().build(_moved(wl, 7e7), 8, wl.indices, wl.prim_count).m_packedNodes
    wants = [wl.want, _want(wl, far, wl.positions)]                 # (the masks may agree; the constants differ either way)
    with api.ShadowContext(0) as a, api.ShadowContext(0) as b:
        devs = []
        try:
            for ctx, packed in ((a, wl.packed), (b, far)):
                ctx.set_bvh(packed)
                ctx.set_option("kernel", 8)
                devs.append(_Dev(ctx, wl))
                devs[-1].plan(xcd_square=0, life_block=0, **WHOLE)
            for turn in range(3):
                for i, (ctx, dev) in enumerate(zip((a, b), devs)):
                    _same(dev.trace(alltable=True), wants[i], ("context", i, "turn", turn))
        finally:
            for dev in devs:
                dev.close()
