"""GPU: traces with an active map where the plain suite has a case and the active suite had none -- launch options, the 1-D grid
fallback, streams the walk treats specially, and edge texels in ACTIVE pixels (the stand-in of rts_packet_tile.inc).

Everywhere the expected mask is `oracle.shadow_mask(...) * (active != 0)` on a mask pre-filled with the guard, compared byte for
byte; and every (stream, light, map) case first shows, on the oracle's result alone, a zero and a non-zero byte among its active
pixels, so that a kernel that writes a constant cannot pass."""
import numpy as np
import pytest

import oracle
import streams
from raytracedshadows_amd import api, scenes, workloads
from test_gpu_active import GUARD, _Dev, _expect, _family, _maps, _stripe_rows
from test_gpu_ray_setup import EDGE, LIGHTS as GATE_LIGHTS, _frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


def _oracle(packed, k, light, pos):
    H, W = pos.shape[:2]
    m, _, _ = oracle.shadow_mask(packed, k.as_array(), oracle.light_from_product(light, k), pos, W, H)
    return m


def _nontrivial(full, active, what):
    """Among the active pixels the oracle's mask holds a zero and a non-zero byte."""
    on = full[active != 0]
    assert on.size and (on == 0).any() and (on != 0).any(), (what, int(on.size), int(np.count_nonzero(on)))


def _trace(ctx, dev, k, light, W, H, **kw):
    dev.guard()
    ctx.trace_shadow_mask_device(k, dev.d_pos, W, H, dev.d_mask, light=light, d_active=dev.d_act, **kw)
    return dev.mask()


# ---- 1. options ----------------------------------------------------------------------------------------------------------------
OPT_DEFAULTS = {"row_order": 0, "xcd_swizzle": 0, "packet_budget": None, "packet_share": None, "block_waves": 1, "wide_lane": 0}
PAIRS = ((1, 16), (1, 0), (2, 8), (8, 4), (64, 16), (64, 1))      # of test_tuning_options_never_change_the_mask


def _settings(kernel=3, soft=False):
    out = [{"row_order": r, "xcd_swizzle": s} for r in (0, 1, 2) for s in (0, 1)]
    for i, (budget, share) in enumerate(PAIRS):
        for s in (0, 1):
            out.append({"packet_budget": budget, "packet_share": share, "xcd_swizzle": s, "row_order": (i + s) % 3})
    out.append({"block_waves": 4})                                   # ignored by an active trace
    out.append({"wide_lane": 1})
    out.append({"block_waves": 4, "wide_lane": 1, "xcd_swizzle": 1})
    if kernel in (8, 9):
        # The wide walk takes 65 to 80 ms per trace of this frame (16 samples: 140 to 340 ms), the plain trace as much as the active
        # one, where the stackless packet takes 0.1 ms (measured on an MI355X; the plain suite never ran kernel 8 here with these
        # options).  The whole matrix would take eight minutes for the two kernels, so they get one setting per code path: row
        # orders 1 and 2, the swizzled 1-D grid, never-dissolve and always-dissolve pairs, the ignored options.
        out = [{"row_order": 1, "xcd_swizzle": 0}, {"row_order": 2, "xcd_swizzle": 1},
               {"packet_budget": 1, "packet_share": 0, "xcd_swizzle": 1, "row_order": 2},
               {"packet_budget": 64, "packet_share": 16, "xcd_swizzle": 0, "row_order": 1},
               {"block_waves": 4, "wide_lane": 1, "xcd_swizzle": 1}]
        if soft:
            out = [out[1], out[3], out[4]]
    return out


OPT_W, OPT_H = 333, 211
OPT_ROWS = (61, 150)
OPT_STRIPES = ((8, 2), (24, 4), (32, 8))             # band 24 = three tiles: not a power of two (<PLAIN=false, BANDS=false>)


@pytest.fixture(scope="module")
def atrium():
    wl = workloads.prepare("atrium", OPT_W, OPT_H, light="point")
    pos, nrm, _ = api.primary_gbuffer(wl.packed, wl.scene.eye, wl.scene.target, wl.scene.fovy, OPT_W, OPT_H)
    assert np.array_equal(pos.ravel(), np.asarray(wl.positions).ravel())
    lights = {"point": wl.light, "directional": None, "soft16pp": workloads.relight(wl, "point", 16, table=64).light}
    maps = _maps(OPT_W, OPT_H, seed=11)
    cases = {}
    for key, light in lights.items():
        full = _oracle(wl.packed, wl.constants, light, pos)
        todo = {m: maps[m] for m in ("random50", "one_active_per_tile", "tile_checker")}
        todo["facing"] = api.facing_active(wl.constants, light, pos, nrm)
        for mname, active in todo.items():
            _nontrivial(full, active, ("atrium", key, mname))
            cases[(key, mname)] = (light, full, active)
    return wl, cases


@pytest.mark.parametrize("kernel", [-1, 0, 3, 5, 7, 8, 9])
@pytest.mark.parametrize("key", ["point", "directional", "soft16pp"])
def test_options_never_change_an_active_mask(ctx, atrium, kernel, key):
    wl, cases = atrium
    W, H, k = OPT_W, OPT_H, wl.constants
    ctx.set_bvh(wl.packed)
    assert ctx.get_option("wide_nodes") > 0
    defaults = {o: ctx.get_option(o) for o in OPT_DEFAULTS}
    dev = _Dev(ctx, wl.positions, W, H)
    share = kernel in (-1, 0, 7)                     # 16 x 16 blocks: a band is a multiple of 16 rows
    rows = (np.arange(H) >= OPT_ROWS[0]) & (np.arange(H) < OPT_ROWS[1])
    try:
        ctx.set_option("kernel", kernel)
        soft = key.startswith("soft")
        for mname in ("random50", "facing") if (soft and kernel in (8, 9)) else ("random50", "one_active_per_tile", "tile_checker", "facing"):
            light, full, active = cases[(key, mname)]
            dev.set_map(active)
            for setting in _settings(kernel, soft):
                for o, v in defaults.items():
                    ctx.set_option(o, setting.get(o, v))
                what = (kernel, key, mname, setting)
                family = _family(ctx, kernel, W * H, soft)
                got = _trace(ctx, dev, k, light, W, H)
                assert int((got != _expect(full, active)).sum()) == 0, what
                assert ctx.last_kernel_name() == family, what
                got = _trace(ctx, dev, k, light, W, H, row_begin=OPT_ROWS[0], row_end=OPT_ROWS[1])
                assert int((got != _expect(full, active, rows)).sum()) == 0, (what, "rows")
                for band, n in OPT_STRIPES:
                    if share and band % 16:
                        band *= 2
                    whole = np.full((H, W), GUARD, np.uint8)
                    for stripe in range(n):
                        dev.guard()
                        ctx.trace_shadow_mask_stripes_device(k, dev.d_pos, W, H, dev.d_mask, band, n, stripe, light=light, d_active=dev.d_act)
                        own = _stripe_rows(H, band, n, stripe)
                        got = dev.mask()
                        assert int((got != _expect(full, active, own)).sum()) == 0, (what, band, n, stripe)   # (other rows keep the guard)
                        whole[own] = got[own]
                    assert np.array_equal(whole, _expect(full, active)), (what, band, n)
                    assert ctx.last_kernel_name() == family, what
    finally:
        for o, v in defaults.items():
            ctx.set_option(o, v)
        ctx.set_option("kernel", -1)
        dev.close()


# ---- 2. more than 65 535 block rows: the 1-D grid --------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,H", [(3, 8 * 65536 + 5), (8, 8 * 65536 + 5), (7, 16 * 65536 + 5)])
def test_tall_frame_takes_the_one_dimensional_grid(ctx, kernel, H):
    """W = 3: the texels of the cornell box's 256 x 256 G-buffer, in row-major order, repeated down the frame (a camera of this
    aspect would see one column of the room); the oracle traces the tall frame itself."""
    W, side = 3, 16 if kernel == 7 else 8
    assert (H + side - 1) // side > 65535
    wl = workloads.prepare_config("cornell_256", cache=True)
    ctx.set_bvh(wl.packed)
    pos = np.resize(np.asarray(wl.positions, np.float32).reshape(-1, 4), (H, W, 4))
    full = _oracle(wl.packed, wl.constants, wl.light, pos)
    active = (np.random.RandomState(H).rand(H, W) < 0.5).astype(np.uint8)
    _nontrivial(full, active, ("tall", kernel))
    _nontrivial(full, np.ones_like(active), ("tall, plain", kernel))
    dev = _Dev(ctx, pos, W, H)
    try:
        dev.set_map(active)
        ctx.set_option("kernel", kernel)
        got = _trace(ctx, dev, wl.constants, wl.light, W, H)
        assert int((got != _expect(full, active)).sum()) == 0
        assert ctx.last_kernel_name() == _family(ctx, kernel, W * H, False)
        a, b = 3, H - 2                              # a row range that still has more than 65 535 block rows
        rows = (np.arange(H) >= a) & (np.arange(H) < b)
        assert (b - a + side - 1) // side > 65535
        got = _trace(ctx, dev, wl.constants, wl.light, W, H, row_begin=a, row_end=b)
        assert int((got != _expect(full, active, rows)).sum()) == 0
        dev.guard()                                  # the plain call on the same frame
        ctx.trace_shadow_mask_device(wl.constants, dev.d_pos, W, H, dev.d_mask, light=wl.light)
        assert int((dev.mask() != full).sum()) == 0
    finally:
        ctx.set_option("kernel", -1)
        dev.close()


# ---- 3. streams the walk treats specially -------------------------------------------------------------------------------------------
def _grid(W, H, lo, hi, z):
    pos = np.zeros((H, W, 4), np.float32)
    pos[..., 0] = lo + (hi - lo) * (np.arange(W, dtype=np.float32)[None, :] + 0.5) / W
    pos[..., 1] = lo + (hi - lo) * (np.arange(H, dtype=np.float32)[:, None] + 0.5) / H
    pos[..., 2] = z
    return pos


def _aimed(packed, W=64, H=64, seed=3):
    """aimed_frame's texels with its point light and the directional light of the same direction."""
    pos, k, point = streams.aimed_frame(packed, 0, W, H, seed)
    d = np.array([7.0, 9.0, 11.0])
    k = api.RayTracingConstants.make([0, 0, 0], d / np.linalg.norm(d), W, H)
    return pos, k, point


def _built(tri, **kw):
    tri = np.ascontiguousarray(tri, np.float32)
    P = tri.shape[0]
    return api.BVHBuilder(**kw).build(tri.reshape(-1, 3), 3, np.arange(3 * P, dtype=np.uint32), P).m_packedNodes


def _soup_triangles(P=3000, seed=9):
    rs = np.random.RandomState(seed)
    return (rs.random_sample((P, 1, 3)) * 40 + (rs.random_sample((P, 3, 3)) - 0.5) * 1.5).astype(np.float32)


def _terrain(n, **kw):
    sc = scenes.terrain(n)
    v, idx = sc.flat()
    return api.BVHBuilder(**kw).build(v, 8, idx, sc.triangle_count).m_packedNodes


def _up_frame(W=64, H=64, lo=0.0, hi=10.0, point=(5.0, 5.0, 40.0)):
    """Texels on the plane z = 0 looking up: the directional light of the plain tests, and a point light above the triangles."""
    pos = _grid(W, H, lo, hi, 0.0)
    k = api.RayTracingConstants.make([0, 0, 0], [0.001, 0.002, 1.0], W, H)
    return pos, k, api.Light.make(api.Light.POINT, np.array(point, np.float32))


def _stream_case(name, ctx=None):
    """(packed or None when the device builds it, installer, positions, constants, point light, expected options)"""
    if name == "non_finite":
        packed = streams.infinite_root(_terrain(9))
        return (packed,) + _aimed(packed) + ({"bvh_finite": 0, "wide_nodes": 0},)
    if name == "unordered":
        wl = workloads.prepare("cornell", 160, 160, via_obj=False)
        return streams.swapped_boxes(wl.packed), wl.positions.reshape(160, 160, 4), wl.constants, wl.light, {"bvh_ordered": 0, "wide_nodes": 0}
    if name == "orphans":
        return (streams.orphan_streams()[1],) + _up_frame() + ({"bvh_enclosed": 0, "wide_nodes": 0},)
    if name == "degenerate":
        packed = _built(streams.degenerate_triangles()[0])
        return (packed,) + _aimed(packed) + ({},)
    if name in ("one_triangle", "two_triangles"):
        P = 1 if name == "one_triangle" else 2
        v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2], [1, 0, 2], [0, 1, 2]], np.float32)[:3 * P]
        pos, k, point = _up_frame(lo=-0.5, hi=1.5, point=(0.3, 0.3, 5.0))
        pos[..., 2] = -1.0
        return (_built(v.reshape(P, 3, 3)), pos, k, point, {"wide_nodes": 0} if P == 1 else {})
    if name == "median_split":
        packed = _terrain(40, sah_prim_limit=100)
        return (packed,) + _aimed(packed) + ({},)
    if name == "deep_bushy":
        return (streams.deep_bushy_stream(25),) + _up_frame(lo=0.2, hi=0.8, point=(0.45, 0.45, 1000.0)) + ({},)
    assert name in ("lbvh", "ploc"), name
    tri = _soup_triangles()
    if ctx is None:                                   # (CPU check of the frame: the same triangles in the host builder's tree)
        packed = _built(tri)
    else:
        packed, _ = api.bvh_build_device(ctx, tri.reshape(-1, 3), 3, np.arange(tri.shape[0] * 3, dtype=np.uint32), tri.shape[0], install=True,
                                         algorithm=name)
    return (packed,) + _aimed(packed) + ({},)


STREAMS = ["non_finite", "unordered", "orphans", "degenerate", "one_triangle", "two_triangles", "median_split", "deep_bushy", "lbvh", "ploc"]
STREAM_KERNELS = (0, 3, 7, 8)


def _active_traces_equal_oracle(ctx, packed, pos, k, lights, what, seed=5):
    H, W = pos.shape[:2]
    maps = _maps(W, H, seed=seed)
    dev = _Dev(ctx, pos, W, H)
    try:
        for lname, light in lights:
            full = _oracle(packed, k, light, pos)
            for mname in ("random50", "one_active_per_tile"):
                active = maps[mname]
                _nontrivial(full, active, (what, lname, mname))
                dev.set_map(active)
                for kernel in STREAM_KERNELS:
                    ctx.set_option("kernel", kernel)
                    got = _trace(ctx, dev, k, light, W, H)
                    bad = int((got != _expect(full, active)).sum())
                    assert bad == 0, (what, lname, mname, kernel, bad)
                    assert ctx.last_kernel_name() == _family(ctx, kernel, W * H, False), (what, kernel)
                    if kernel == 8 and ctx.get_option("wide_nodes") == 0:
                        assert ctx.last_kernel_name() == "shadowMaskActivePacketKernel<1>", what
    finally:
        ctx.set_option("kernel", -1)
        dev.close()


@pytest.mark.parametrize("name", STREAMS)
def test_active_traces_on_awkward_streams(ctx, name):
    packed, pos, k, point, options = _stream_case(name, ctx)
    if name not in ("lbvh", "ploc"):
        ctx.set_bvh(packed)
    for key, val in options.items():
        assert ctx.get_option(key) == val, (name, key)
    if name == "deep_bushy":
        assert ctx.get_option("wide_nodes") > 25
    if name in ("lbvh", "ploc", "median_split", "two_triangles"):
        assert ctx.get_option("wide_nodes") > 0, name
    _active_traces_equal_oracle(ctx, packed, pos, k, (("point", point), ("directional", None)), name)


def test_active_traces_around_a_refit_that_drops_the_copy(ctx):
    wl = workloads.prepare("cornell", 160, 160, via_obj=False)
    ctx.set_bvh(wl.packed)
    pos = wl.positions.reshape(wl.H, wl.W, 4)
    lights = (("point", wl.light), ("directional", None))
    assert ctx.get_option("wide_nodes") > 0
    w = wl.vertices.copy()
    w[0, 0], w[1, 0] = np.float32(-3e38), np.float32(3e38)               # finite vertices whose edge overflows: e0.x = +Inf
    got, _, _ = api.bvh_refit_device(ctx, w, 8, wl.indices, wl.prim_count, want_packed=True)
    assert np.isinf(got[:, :3].view(np.float32)).any()
    assert ctx.get_option("bvh_finite") == 0 and ctx.get_option("wide_nodes") == 0
    _active_traces_equal_oracle(ctx, got, pos, wl.constants, lights, "refit, edge overflow")
    back, _, _ = api.bvh_refit_device(ctx, wl.vertices, 8, wl.indices, wl.prim_count, want_packed=True)
    assert ctx.get_option("bvh_finite") == 1 and ctx.get_option("wide_nodes") > 0
    _active_traces_equal_oracle(ctx, back, pos, wl.constants, lights, "refit, back")


# ---- 4. edge texels in active pixels -------------------------------------------------------------------------------------------------
ON_LIGHT = len(EDGE)                                 # pseudo edge value: the texel the "on_texel" point light sits on


def _edge_ids(pos):
    """int[H, W, 3]: the index in EDGE of each coordinate's bit pattern, -1 for an ordinary one; the texel at (20, 40) counts as
    ON_LIGHT in all three."""
    bits = np.ascontiguousarray(pos[..., :3]).view(np.uint32)
    ids = np.full(bits.shape, -1, np.int64)
    for i, b in enumerate(EDGE.view(np.uint32)):
        ids[bits == b] = i
    assert (pos[20, 40, :3] == 0.5).all()
    ids[20, 40] = ON_LIGHT
    return ids


def _tiles(H, W):
    for ty in range(H // 8):
        for tx in range(W // 8):
            yield ty, tx, (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))


def _edge_maps(pos, seed=17):
    """The three maps of the stand-in's cases, over every tile that holds an edge texel (lane = 8 * row + column of the tile):
    a  the lowest active lane is an edge texel -- the first walker itself fails the gate;
    b  the lowest active lane is an ordinary texel and an edge texel is active later -- a later walker fails it;
    c  only the edge texels are active -- where a tile holds one, the first walker is the only edge texel.
    Tile t aims at edge value t mod (len(EDGE) + 1) when it holds it, so that every value gets a tile of every kind."""
    H, W = pos.shape[:2]
    ids = _edge_ids(pos)
    edge = (ids >= 0).any(-1)
    rnd = (np.random.RandomState(seed).rand(H, W) < 0.5)
    a, b, c = rnd.copy(), rnd.copy(), edge.copy()
    for t, (ty, tx, sl) in enumerate(_tiles(H, W)):
        e = edge[sl].ravel()
        if not e.any():
            continue
        has = (ids[sl] == (t % (len(EDGE) + 1))).any(-1).ravel()
        lanes = np.arange(64)
        # a
        first = int(np.flatnonzero(has)[0]) if has.any() else int(np.flatnonzero(e)[0])
        m = rnd[sl].ravel() & (lanes > first)
        m[first] = True
        a[sl] = m.reshape(8, 8)
        # b
        m = np.zeros(64, bool)
        if (~e).any():
            o = int(np.flatnonzero(~e)[0])
            later = np.flatnonzero((has if (has & (lanes > o)).any() else e) & (lanes > o))
            if later.size:
                m = rnd[sl].ravel() & (lanes > o)
                m[o] = True
                m[later[0]] = True
        b[sl] = m.reshape(8, 8)
    return {"a": a.astype(np.uint8), "b": b.astype(np.uint8), "c": c.astype(np.uint8)}, ids


def _check_edge_maps(maps, ids):
    """From the frame and the maps alone: each kind holds for at least one tile per edge value."""
    H, W = ids.shape[:2]
    edge = (ids >= 0).any(-1)
    seen = {"a": set(), "b": set(), "c": set()}
    for ty, tx, sl in _tiles(H, W):
        e, tid = edge[sl].ravel(), ids[sl].reshape(64, 3)
        for kind in "abc":
            act = np.flatnonzero(maps[kind][sl].ravel())
            if not act.size:
                continue
            if kind == "a" and e[act[0]]:
                seen["a"].update(int(v) for v in tid[act[0]] if v >= 0)
            if kind == "b" and not e[act[0]]:
                seen["b"].update(int(v) for lane in act[1:] for v in tid[lane] if v >= 0)
            if kind == "c":
                assert e[act].all()
                seen["c"].update(int(v) for lane in act for v in tid[lane] if v >= 0)
    everything = set(range(len(EDGE) + 1))
    for kind in "abc":
        assert seen[kind] == everything, (kind, sorted(everything - seen[kind]))
    assert any(np.count_nonzero(maps["c"][sl]) == 1 for _, _, sl in _tiles(H, W)), "c: a tile whose only active lane is an edge texel"


def _gate_lights():
    lights = {name: api.Light.make(kind, np.array(xyz, np.float32)) for name, (kind, xyz) in GATE_LIGHTS.items()}
    rng = np.random.RandomState(13)
    offsets = np.zeros((16, 4), np.float32)
    offsets[:, :3] = (rng.random_sample((16, 3)) * 2 - 1) * 0.05
    lights["soft16_on_texel"] = api.Light.make(api.Light.POINT, np.array([0.5, 0.5, 0.5], np.float32), offsets)
    return lights


@pytest.fixture(scope="module")
def gate():
    packed, tri = streams.gate_soup()
    pos = _frame(tri)
    maps, ids = _edge_maps(pos)
    _check_edge_maps(maps, ids)
    return packed, pos, maps


@pytest.mark.parametrize("name", sorted(GATE_LIGHTS) + ["soft16_on_texel"])
def test_edge_texels_in_active_pixels(ctx, gate, name):
    packed, pos, maps = gate
    H, W = pos.shape[:2]
    k = api.RayTracingConstants.make([0, 0, 0], [0.3, 0.8, 0.5], W, H)
    light = _gate_lights()[name]
    full = _oracle(packed, k, light, pos)
    ctx.set_bvh(packed)
    dev = _Dev(ctx, pos, W, H)
    try:
        for kind in "abc":
            active = maps[kind]
            _nontrivial(full, active, (name, kind))
            dev.set_map(active)
            for kernel in (3, 7, 8, 9):
                for soft_split in (0, 1):
                    ctx.set_option("kernel", kernel)
                    ctx.set_option("soft_split", soft_split)
                    got = _trace(ctx, dev, k, light, W, H)
                    bad = int((got != _expect(full, active)).sum())
                    assert bad == 0, (name, kind, kernel, soft_split, bad)
                    assert ctx.last_kernel_name() == _family(ctx, kernel, W * H, name.startswith("soft")), (name, kernel)
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()
