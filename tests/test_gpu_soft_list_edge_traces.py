"""GPU: the soft light list traces in their three modes -- plain (rts_trace_soft_light_list*), adaptive and jittered -- where their own
suites never go (inputs: tests/soft_list_edge_cases.py): edge texels behind the wave-wide gates of the ray set-up, tiles in which
consecutive lights have different walkers, a penumbra that only edge texels own, lights at 3e19 and 1e38 with a radius, the streams
the walk treats specially, a refit that drops the private copy, frames of more than 65 535 block rows (the 1-D grid), and capture on
an awkward stream.

Everywhere the expected value is the oracle's definition computed here (soft_list_jitter_cases.definition; on the tall frames
gathered with a numpy hash): no host twin stands in between -- tests/test_soft_list_edge_cases_host.py pins the twins to the same
values.  Counts and the refined plane are compared byte for byte on buffers pre-filled with 0xAB; planes at or above the count, rows
outside the range and a refined plane that was not asked for must keep that fill.  Every test asserts its guards from the oracle's
planes alone before its first trace, asserts the kernel's name, and restores the options it sets."""
import numpy as np
import pytest

import hipgraph
import soft_list_edge_cases as sc
from raytracedshadows_amd import api, workloads
from test_gpu_edge_traces import _stream, _tall_height
from test_gpu_soft_light_list import _name as _plain_name
from test_gpu_soft_list_adaptive import GUARD, _Dev, _expect, _form, _reset, _same
from test_gpu_soft_list_adaptive import _name as _adaptive_name
from test_gpu_soft_list_jitter import _name as _jitter_name

pytestmark = pytest.mark.gpu

NAMES = {"plain": _plain_name, "adaptive": _adaptive_name, "jittered": _jitter_name}


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


def _rows(H, rows):
    return None if rows is None else (np.arange(H) >= rows[0]) & (np.arange(H) < rows[1])


def _call(ctx, dev, k, lights, probes, tables, mode, use_map, rows=None, refined=True, stream=None):
    kw = {"stream": stream, "d_lights_map": dev.d_map if use_map else None}
    if rows is not None:
        kw.update(row_begin=rows[0], row_end=rows[1])
    if mode == "plain":
        ctx.trace_soft_light_list_device(k, lights, dev.d_pos, dev.W, dev.H, dev.d_counts, **kw)
    else:
        ctx.trace_soft_light_list_adaptive_device(k, lights, probes, dev.d_pos, dev.W, dev.H, dev.d_counts, d_refined=dev.d_ref if refined else None,
                                                  tables=tables if mode == "jittered" else None, **kw)


def _trace(ctx, dev, k, lights, probes, tables, mode, want, what, lights_map=None, rows=None, refined=True):
    """`want`: the mode's definition without a map.  The plain call has no refined plane: its buffer keeps the fill."""
    if lights_map is not None:
        ctx.h2d(dev.d_map, np.ascontiguousarray(lights_map, np.uint8))
    dev.guard()
    _call(ctx, dev, k, lights, probes, tables, mode, lights_map is not None, rows, refined)
    c, r = _expect(want, lights_map, _rows(dev.H, rows))
    got = dev.read()
    _same(got, (c, r if refined and mode != "plain" else np.full_like(r, GUARD)), (what, mode))
    return got


# ---- 1. the gate list on edge texels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("kernel,split", sc.FORMS)
def test_gate_list_on_edge_texels(ctx, kernel, split, mode):
    """The whole list with and without the refined plane, the two per-light edge maps and the lone pixel; then the sub-lists of 1, 2
    and 5 entries with the same three maps, which leave waves of the four-wave form with few pairs or none in a phase."""
    g = sc.gate()
    sc.guard_gate(8)
    for n in sc.SUB_LISTS:
        sc.guard_gate(n)
        assert np.array_equal(sc.gate_want(mode, n)[0], sc.gate_want(mode)[0][:n])     # a plane is a function of its light alone
    name = NAMES[mode](kernel, split)
    ctx.set_bvh(g.packed)
    dev = _Dev(ctx, g.pos, g.W, g.H)
    try:
        _form(ctx, kernel, split)
        for n in (8,) + sc.SUB_LISTS:
            lights, probes, tables, want = sc.gate_soft_list(n), sc.GATE_PROBES[:n], sc.GATE_TABLES[:n], sc.gate_want(mode, n)
            _trace(ctx, dev, g.k, lights, probes, tables, mode, want, (kernel, split, n, "whole"))
            assert ctx.last_kernel_name() == name, ctx.last_kernel_name()
            if n == 8:
                _trace(ctx, dev, g.k, lights, probes, tables, mode, want, (kernel, split, n, "refined NULL"), refined=False)
            for what, m in sc.gate_maps(n).items():
                got = _trace(ctx, dev, g.k, lights, probes, tables, mode, want, (kernel, split, n, what), lights_map=m)
                assert ctx.last_kernel_name() == name, ctx.last_kernel_name()
                if what == "lone":
                    assert np.count_nonzero(got[0][0]) <= 1 and not got[0][1:n].any()
    finally:
        _reset(ctx)
        dev.close()


# ---- 2. a penumbra that only edge texels own ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", sc.FORMS)
def test_a_penumbra_that_only_edge_texels_own(ctx, kernel, split):
    """Under soft_list_edge_cases.penumbra_map only edge texels walk: every stand-in of the probe and of the refinement is an edge
    texel (under jitter with that texel's pixel index), and whether the four waves pass between the barriers is decided by the probe
    counts of NaN, Inf, denormal and 3e38 texels.  The oracle shows refined edge texels in both modes, so both kinds of tile are
    asserted: 18 tiles whose refined pixels are all edge texels (6 of them with a single marked lane) and 6 tiles with marked pixels
    of which none refines."""
    g = sc.gate()
    m = sc.penumbra_map()
    for mode in ("adaptive", "jittered"):
        owned, lone, idle = sc.penumbra_tiles(sc.gate_want(mode)[1], m)
        assert owned >= 1 and lone >= 1 and idle >= 1, (mode, owned, lone, idle)
    lights = sc.gate_soft_list()
    ctx.set_bvh(g.packed)
    dev = _Dev(ctx, g.pos, g.W, g.H)
    try:
        _form(ctx, kernel, split)
        for mode in ("adaptive", "jittered"):
            _trace(ctx, dev, g.k, lights, sc.GATE_PROBES, sc.GATE_TABLES, mode, sc.gate_want(mode), (kernel, split, "edge penumbra"), lights_map=m)
            assert ctx.last_kernel_name() == NAMES[mode](kernel, split), ctx.last_kernel_name()
    finally:
        _reset(ctx)
        dev.close()


# ---- 3. the definition on the device itself, on edges -------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", sc.FORMS)
def test_plane_l_is_the_devices_own_one_light_trace_on_edge_texels(ctx, kernel, split):
    """Jittered, under the `edges` map: plane l and bit l of refined = rts_trace_shadow_mask_adaptive for lights.light(l, table=T_l)
    with probe k_l and the map's bit l as its active byte; k_l == 0: the soft mask trace of that light, refined bit 0."""
    g = sc.gate()
    lights, want = sc.gate_soft_list(), sc.gate_want("jittered")
    m = sc.gate_maps()["edges"]
    sc.guard_map(want[0], m, "gate, edges")
    ctx.set_bvh(g.packed)
    dev = _Dev(ctx, g.pos, g.W, g.H)
    d_one, d_took, d_act = ctx.malloc(g.W * g.H), ctx.malloc(g.W * g.H), ctx.malloc(g.W * g.H)
    try:
        _form(ctx, kernel, split)
        c, r = _trace(ctx, dev, g.k, lights, sc.GATE_PROBES, sc.GATE_TABLES, "jittered", want, (kernel, split, "list"), lights_map=m)
        assert ctx.last_kernel_name() == _jitter_name(kernel, split), ctx.last_kernel_name()
        for l in range(lights.count):
            lt = lights.light(l, table=sc.GATE_TABLES[l])
            ctx.h2d(d_act, np.ascontiguousarray((m >> l) & 1, np.uint8))
            ctx.h2d(d_one, np.full(g.W * g.H, GUARD, np.uint8))
            ctx.h2d(d_took, np.zeros(g.W * g.H, np.uint8))
            if sc.GATE_PROBES[l]:
                ctx.trace_shadow_mask_adaptive_device(g.k, dev.d_pos, g.W, g.H, d_one, lt, sc.GATE_PROBES[l], d_refined=d_took, d_active=d_act)
            else:
                ctx.trace_shadow_mask_device(g.k, dev.d_pos, g.W, g.H, d_one, light=lt, d_active=d_act)
            _same(c[l], dev.read(what=d_one), (kernel, split, "light", l))
            _same((r >> l) & 1, dev.read(what=d_took), (kernel, split, "light", l, "refined"))
    finally:
        _reset(ctx)
        for d in (d_one, d_took, d_act):
            ctx.free(d)
        dev.close()


# ---- 4. packets that dissolve at once -----------------------------------------------------------------------------------------------
def test_gate_list_with_packets_that_dissolve(ctx):
    g = sc.gate()
    sc.guard_gate(8)
    lights, m = sc.gate_soft_list(), sc.gate_maps()["edges"]
    ctx.set_bvh(g.packed)
    dev = _Dev(ctx, g.pos, g.W, g.H)
    before = ctx.get_option("packet_budget")
    try:
        _form(ctx, 3, 1)
        ctx.set_option("packet_budget", 1)               # every packet dissolves at once
        for mode in sc.MODES:
            _trace(ctx, dev, g.k, lights, sc.GATE_PROBES, sc.GATE_TABLES, mode, sc.gate_want(mode), "dissolve")
            assert ctx.last_kernel_name() == NAMES[mode](3, 1), ctx.last_kernel_name()
            _trace(ctx, dev, g.k, lights, sc.GATE_PROBES, sc.GATE_TABLES, mode, sc.gate_want(mode), ("dissolve", "edges"), lights_map=m)
    finally:
        ctx.set_option("packet_budget", before)
        _reset(ctx)
        dev.close()


# ---- 5. awkward streams -------------------------------------------------------------------------------------------------------------
def _soft_stream(ctx, name):
    """test_gpu_edge_traces._stream (the definition and its guards before anything is installed; on `lbvh` and `ploc` again on the
    stream the device returns) -> (pos, k, lights, {mode: definition})."""
    def expect(packed, pos, k, point):
        lights = sc.stream_soft_list(pos, k, point)
        return lights, sc.stream_wants(packed, k, lights, pos, name)

    pos, k, _, (lights, wants) = _stream(ctx, name, expect)
    return pos, k, lights, wants


@pytest.mark.parametrize("name", sc.STREAMS)
def test_stream_soft_lists_on_awkward_streams(ctx, name):
    pos, k, lights, wants = _soft_stream(ctx, name)
    dev = _Dev(ctx, pos, pos.shape[1], pos.shape[0])
    try:
        for kernel, split in sc.FORMS:
            _form(ctx, kernel, split)
            for mode in sc.MODES:
                _trace(ctx, dev, k, lights, sc.STREAM_PROBES, sc.STREAM_TABLES, mode, wants[mode], (name, kernel, split))
                assert ctx.last_kernel_name() == NAMES[mode](kernel, split), ctx.last_kernel_name()
    finally:
        _reset(ctx)
        dev.close()


# ---- 6. around a refit that drops the private copy ----------------------------------------------------------------------------------
def test_stream_soft_list_around_a_refit_that_drops_the_copy(ctx):
    """The recipe of test_lists_and_soft_distance_around_a_refit_that_drops_the_copy: finite vertices whose edge overflows to +Inf,
    then back; the definition is recomputed from the stream each refit returns."""
    wl = workloads.prepare("cornell", 160, 160, via_obj=False)
    pos, k = np.ascontiguousarray(wl.positions, np.float32).reshape(wl.H, wl.W, 4), wl.constants
    lights = sc.stream_soft_list(pos, k, wl.light)

    def check(packed, what):
        wants = sc.stream_wants(packed, k, lights, pos, what)
        for kernel, split in sc.FORMS:
            _form(ctx, kernel, split)
            for mode in sc.MODES:
                _trace(ctx, dev, k, lights, sc.STREAM_PROBES, sc.STREAM_TABLES, mode, wants[mode], (what, kernel, split))
                assert ctx.last_kernel_name() == NAMES[mode](kernel, split), ctx.last_kernel_name()

    sc.stream_wants(wl.packed, k, lights, pos, "refit, before")          # (from the oracle, before any device call)
    ctx.set_bvh(wl.packed)
    dev = _Dev(ctx, pos, wl.W, wl.H)
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


# ---- 7. more than 65 535 block rows: the 1-D grid -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", sc.FORMS)
def test_tall_soft_lists_take_the_one_dimensional_grid(ctx, kernel, split):
    """The plain and the jittered mode, whole and on the row range (3, H - 2), with and without a random 50 % map, in the device
    form and, on the row range, in the host form (pixelBase = 9 on the `general` grid).  The jittered
    expectation is gathered per pixel with start(y * W + x, T) from the numpy hash: a kernel that ignored the table, or hashed the
    index inside the row range instead of the full frame's, writes another plane -- asserted below before anything is traced."""
    t = sc.tall_case()
    H, W = _tall_height(kernel), 3
    wants = {mode: sc.tall_want(t, mode, H) for mode in ("plain", "jittered")}
    inside = slice(3, H - 2)
    assert int((wants["jittered"][0][0][inside] != sc.tall_untabled(t, "jittered", H)[0][inside]).sum()) >= sc.LEAST
    assert int((wants["jittered"][0][0][inside] != sc.tall_want(t, "jittered", H, wrong_base=3 * W)[0][0][inside]).sum()) >= sc.LEAST
    assert not wants["plain"][1].any() and wants["jittered"][1].any()
    m = np.random.RandomState(H + split).randint(0, 256, (H, W)).astype(np.uint8)          # 50 % per bit
    for mode in wants:
        sc.guard_map(wants[mode][0], m, ("tall, map", mode))
    ctx.set_bvh(t["wl"].packed)
    dev = _Dev(ctx, sc.tall_positions(t["texels"], H), W, H)
    try:
        _form(ctx, kernel, split)
        for mode in ("plain", "jittered"):
            for rows in (None, (3, H - 2)):
                for lights_map in (None, m):
                    _trace(ctx, dev, t["k"], t["lights"], sc.TALL_PROBES, sc.TALL_TABLES, mode, wants[mode],
                           ("tall", kernel, split, rows, lights_map is not None), lights_map=lights_map, rows=rows)
                    assert ctx.last_kernel_name() == NAMES[mode](kernel, split, "general"), ctx.last_kernel_name()
        # The host forms on the row range.  A device-form row range hashes y * W + x with pixelBase 0; here the rows travel as a
        # frame of their own -- still more than 65 535 block rows -- and pixelBase = 3 * W must make the hash the caller's frame's.
        rows, pos = (3, H - 2), sc.tall_positions(t["texels"], H)
        for mode in ("plain", "jittered"):
            for lights_map in (None, m):
                out, ref = np.full((8, H, W), GUARD, np.uint8), np.full((H, W), GUARD, np.uint8)
                kw = dict(lights_map=lights_map, row_begin=rows[0], row_end=rows[1], out=out)
                if mode == "plain":
                    ctx.trace_soft_light_list(t["k"], t["lights"], pos, W, H, **kw)
                else:
                    ctx.trace_soft_light_list_adaptive(t["k"], t["lights"], sc.TALL_PROBES, pos, W, H, refined=ref, tables=sc.TALL_TABLES, **kw)
                assert ctx.last_kernel_name() == NAMES[mode](kernel, split, "general"), ctx.last_kernel_name()
                c, r = _expect(wants[mode], lights_map, _rows(H, rows))
                _same((out, ref), (c, r if mode != "plain" else np.full_like(r, GUARD)), ("tall", kernel, split, mode, "host rows", lights_map is not None))
    finally:
        _reset(ctx)
        dev.close()


# ---- 8. capture on an awkward stream ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["non_finite", "deep_bushy"])
def test_jittered_device_form_under_capture_on_an_awkward_stream(ctx, name):
    """One kernel node, replayed twice on guard-filled buffers; the second replay follows another map in the same buffer."""
    pos, k, lights, wants = _soft_stream(ctx, name)
    want = wants["jittered"]
    H, W = pos.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    m = ((x * 7 + y * 13 + (x >> 3) * 5) & 0xFF).astype(np.uint8)
    m[(x + y) % 5 == 0] = 0
    maps = (m, (255 - m).astype(np.uint8))
    for one in maps:
        sc.guard_map(want[0], one, (name, "capture"))
    dev = _Dev(ctx, pos, W, H)
    stream = ctx.stream_create()
    g = None
    try:
        _form(ctx, 3, 1)
        ctx.h2d(dev.d_map, maps[0])
        ctx.trace_shadow_mask_device(k, dev.d_pos, W, H, dev.d_counts, light=lights.light(0), stream=stream)     # a stream that has traced
        ctx.synchronize(stream)
        g = hipgraph.capture(stream, lambda: _call(ctx, dev, k, lights, sc.STREAM_PROBES, sc.STREAM_TABLES, "jittered", True, stream=stream))
        assert ctx.last_kernel_name() == _jitter_name(3, 1), ctx.last_kernel_name()
        assert g.node_types() == [hipgraph.KERNEL], g.node_types()
        for replay, one in enumerate(maps):
            ctx.h2d(dev.d_map, one)
            dev.guard()
            g.launch(stream)
            _same(dev.read(stream), _expect(want, one), (name, "replay", replay))
    finally:
        if g:
            g.close()
        ctx.synchronize(stream)
        ctx.stream_destroy(stream)
        _reset(ctx)
        dev.close()
