"""GPU: the occluder distance (rts_trace_shadow_distance*, rts_trace_rays_distance*; include/rts.h) against its host twin
(rtsh_shadow_distance / rtsh_rays_distance, which tests/test_distance_host.py pins to the oracle's any-hit), as uint32, on
guard-filled buffers: every kernel family, ragged frames, row ranges, stripes, both lights, active maps, dissolving packets, the
exact path's streams, generic rays, the 256 K-pixel switch, the counters, and the device forms under graph capture."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import streams
from distance_cases import (INF_BITS, bisect_distance, bits, far_before_near, far_before_near_frame, frame_rays, generic_rays)
from raytracedshadows_amd import api, workloads

pytestmark = pytest.mark.gpu

GUARD_F = np.float32(-123.25)
GUARD_B = 0xAB
SHARE, RAYS = "shadowDistanceShareKernel", "traceRaysDistanceKernel"
PACKET, PACKET_BANDS, PACKET_GENERAL = ("shadowDistancePacketKernel<%s>" % g for g in ("rows", "bands", "general"))


def _name(kernel, pixels):
    if kernel == -1:
        return SHARE if pixels < (1 << 18) else PACKET
    return SHARE if kernel in (0, 1, 2, 7) else PACKET


class _Frame:
    """A cornell frame (positions and normals from the library's host G-buffer pass), its lights, and the twin's values per light."""

    def __init__(self, W, H):
        self.wl = wl = workloads.prepare("cornell", W, H, light="point")
        self.W, self.H, self.k, self.packed = W, H, wl.constants, wl.packed
        sc = wl.scene
        self.pos, self.nrm, hits = api.primary_gbuffer(wl.packed, sc.eye, sc.target, sc.fovy, W, H)
        assert 0 < hits
        self.lights = {"point": wl.light, "directional": None}
        self._want = {}

    def want(self, key):
        if key not in self._want:
            d, m = api.shadow_distance(self.packed, self.k, self.lights[key], self.pos, self.W, self.H)
            assert 0 < int((bits(d) != INF_BITS).sum()) < d.size, key
            self._want[key] = (d, m)
        return self._want[key]


_FRAMES = {}


def frame(W, H):
    if (W, H) not in _FRAMES:
        _FRAMES[(W, H)] = _Frame(W, H)
    return _FRAMES[(W, H)]


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


class _Dev:
    def __init__(self, ctx, positions, W, H):
        self.ctx, self.W, self.H = ctx, W, H
        positions = np.ascontiguousarray(positions, np.float32)
        self.d_pos, self.d_act, self.d_mask, self.d_dist = ctx.malloc(positions.nbytes), ctx.malloc(W * H), ctx.malloc(W * H), ctx.malloc(W * H * 4)
        ctx.h2d(self.d_pos, positions)

    def guard(self):
        self.ctx.h2d(self.d_mask, np.full(self.W * self.H, GUARD_B, np.uint8))
        self.ctx.h2d(self.d_dist, np.full(self.W * self.H, GUARD_F, np.float32))

    def read(self, stream=None):
        d, m = np.empty((self.H, self.W), np.float32), np.empty((self.H, self.W), np.uint8)
        self.ctx.synchronize(stream)
        self.ctx.d2h(d, self.d_dist)
        self.ctx.d2h(m, self.d_mask)
        return d, m

    def close(self):
        for d in (self.d_pos, self.d_act, self.d_mask, self.d_dist):
            self.ctx.free(d)


def _expect(want, active=None, rows=None):
    d, m = want
    if active is not None:
        d, m = np.where(active != 0, d, np.float32(0.0)).astype(np.float32), (m * (active != 0)).astype(np.uint8)
    if rows is not None:
        d, m = np.where(rows[:, None], d, GUARD_F).astype(np.float32), np.where(rows[:, None], m, GUARD_B).astype(np.uint8)
    return d, m


def _same(got, want, what):
    for g, w, part in ((bits(got[0]), bits(want[0]), "distance"), (got[1], want[1], "mask")):
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, part, bad.shape[0], bad[:4].tolist(), [g[tuple(b)] for b in bad[:4]], [w[tuple(b)] for b in bad[:4]])


def _trace(ctx, dev, fr, key, what, active=None, rows=None, kernel=None, expect_name=True, **kw):
    if kernel is not None:
        ctx.set_option("kernel", kernel)
    if active is not None:
        ctx.h2d(dev.d_act, np.ascontiguousarray(active, np.uint8))
    dev.guard()
    ctx.trace_shadow_distance_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, d_mask=dev.d_mask, light=fr.lights[key],
                                     d_active=dev.d_act if active is not None else None, **kw)
    if expect_name and kernel is not None:
        assert ctx.last_kernel_name() == _name(kernel, fr.W * (kw.get("row_end", fr.H) - kw.get("row_begin", 0))), (what, ctx.last_kernel_name())
    _same(dev.read(), _expect(fr.want(key), active, rows), what)


@pytest.mark.parametrize("key", ["point", "directional"])
@pytest.mark.parametrize("size", [(64, 48), (61, 37)])
def test_every_family_equals_the_twin(ctx, size, key):
    fr = frame(*size)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        for kernel in (-1, 0, 3, 7, 8):
            _trace(ctx, dev, fr, key, (size, key, kernel), kernel=kernel)
            # a row range that cuts tiles and blocks at both ends
            rows = (np.arange(fr.H) >= 5) & (np.arange(fr.H) < fr.H - 6)
            _trace(ctx, dev, fr, key, (size, key, kernel, "rows"), rows=rows, kernel=kernel, row_begin=5, row_end=fr.H - 6)
    finally:
        ctx.set_option("kernel", -1)
        dev.close()


def test_smallest_case_equals_the_definition_directly(ctx):
    fr = frame(64, 48)
    want = bisect_distance(fr.packed, frame_rays(fr.k, fr.lights["point"], fr.pos)).reshape(fr.H, fr.W)
    assert np.array_equal(bits(want), bits(fr.want("point")[0]))
    ctx.set_bvh(fr.packed)
    for kernel in (3, 7):
        ctx.set_option("kernel", kernel)
        d, m = ctx.trace_shadow_distance(fr.k, fr.pos, fr.W, fr.H, light=fr.lights["point"])      # (the host-pointer form)
        assert np.array_equal(bits(d), bits(want)), kernel
        assert np.array_equal(m, (bits(want) == INF_BITS).astype(np.uint8)), kernel
    ctx.set_option("kernel", -1)


def _maps(fr, key):
    y, x = np.mgrid[0:fr.H, 0:fr.W]
    tile = np.ones((fr.H, fr.W), np.uint8)
    tile[8:16, 16:24] = 0                                # one 8 x 8 tile wholly inactive beside active ones
    return {"ones": np.ones((fr.H, fr.W), np.uint8), "zeros": np.zeros((fr.H, fr.W), np.uint8),
            "checker": (((x + y) & 1) * 255).astype(np.uint8), "tile": tile,
            "facing": api.facing_active(fr.k, fr.lights[key], fr.pos, fr.nrm)}


@pytest.mark.parametrize("key", ["point", "directional"])
@pytest.mark.parametrize("kernel", [3, 7])
def test_active_maps(ctx, kernel, key):
    fr = frame(64, 48)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    d_ref = ctx.malloc(fr.W * fr.H)
    try:
        _trace(ctx, dev, fr, key, (kernel, key, "no map"), kernel=kernel)
        for name, active in _maps(fr, key).items():
            if name == "facing":
                assert 0 < np.count_nonzero(active) < active.size
            dirty = fr.pos.copy()                        # inactive texels may hold anything
            dirty[active == 0] = np.array([np.nan, np.inf, 1e38, -np.inf], np.float32)
            ctx.h2d(dev.d_pos, dirty)
            _trace(ctx, dev, fr, key, (kernel, key, name), active=active, kernel=kernel)
            # the mask is the active mask trace's, byte for byte
            ctx.h2d(d_ref, np.full(fr.W * fr.H, GUARD_B, np.uint8))
            ctx.trace_shadow_mask_device(fr.k, dev.d_pos, fr.W, fr.H, d_ref, light=fr.lights[key], d_active=dev.d_act)
            ctx.synchronize()
            ref = np.empty((fr.H, fr.W), np.uint8)
            ctx.d2h(ref, d_ref)
            assert np.array_equal(dev.read()[1], ref), (kernel, key, name)
        # d_mask is optional: the distances alone
        ctx.h2d(dev.d_pos, fr.pos)
        dev.guard()
        ctx.trace_shadow_distance_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, light=fr.lights[key])
        d, m = dev.read()
        assert np.array_equal(bits(d), bits(fr.want(key)[0])) and (m == GUARD_B).all()
    finally:
        ctx.set_option("kernel", -1)
        ctx.free(d_ref)
        dev.close()


_HOST_ROWS = {}


def _host_rows_case():
    """Frame 61 x 37, the checker map (zero bytes and set bytes), and the twin's values under that map: computed once."""
    if not _HOST_ROWS:
        fr = frame(61, 37)
        active = _maps(fr, "point")["checker"]
        assert 0 < np.count_nonzero(active[3:30]) < active[3:30].size
        want = api.shadow_distance(fr.packed, fr.k, fr.lights["point"], fr.pos, fr.W, fr.H, active=active)
        for a in (active,) + want:
            a.setflags(write=False)
        _HOST_ROWS.update(fr=fr, active=active, want=want)
    return _HOST_ROWS["fr"], _HOST_ROWS["active"], _HOST_ROWS["want"]


@pytest.mark.parametrize("kernel", [7, 3])
def test_host_form_with_an_active_map_and_a_row_range(ctx, kernel):
    """The host-pointer form with a per-pixel map AND a row range: rows [3, 30) of the positions and of the map travel through the
    staging buffers as a frame of their own.  Inside the rows the twin's bits, outside them the guard the arrays were filled with."""
    fr, active, want = _host_rows_case()
    rows = (np.arange(fr.H) >= 3) & (np.arange(fr.H) < 30)
    ctx.set_bvh(fr.packed)
    try:
        ctx.set_option("kernel", kernel)
        out, om = np.full((fr.H, fr.W), GUARD_F, np.float32), np.full((fr.H, fr.W), GUARD_B, np.uint8)
        ctx.trace_shadow_distance(fr.k, fr.pos, fr.W, fr.H, light=fr.lights["point"], row_begin=3, row_end=30, active=active, out=out, mask=om)
        assert ctx.last_kernel_name() == _name(kernel, fr.W * 27), ctx.last_kernel_name()
        _same((out, om), _expect(want, None, rows), (kernel, "host rows with a map"))
        out = np.full((fr.H, fr.W), GUARD_F, np.float32)
        d, m = ctx.trace_shadow_distance(fr.k, fr.pos, fr.W, fr.H, light=fr.lights["point"], row_begin=3, row_end=30, active=active, out=out,
                                         want_mask=False)
        assert d is out and m is None
        assert np.array_equal(bits(out), bits(_expect(want, None, rows)[0])), (kernel, "distances alone")
    finally:
        ctx.set_option("kernel", -1)


@pytest.mark.parametrize("band", [8, 16, 24, 32])
def test_stripes(ctx, band):
    fr = frame(61, 37)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    active = _maps(fr, "point")["checker"]
    ctx.h2d(dev.d_act, active)
    try:
        for kernel in (3, 7, -1):
            ctx.set_option("kernel", kernel)
            for with_map in (False, True):
                for stripe in range(3):                  # (37 rows in bands of 16 or more: a stripe that owns no band)
                    dev.guard()
                    call = lambda: ctx.trace_shadow_distance_stripes_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, band, 3, stripe,
                                                                            d_mask=dev.d_mask, light=fr.lights["point"],
                                                                            d_active=dev.d_act if with_map else None)
                    rows = ((np.arange(fr.H) // band) % 3) == stripe
                    # lane per ray: a band is a multiple of 16 rows (include/rts.h) -- refused for every stripe that owns a band; one
                    # that owns none launches nothing and returns RTS_OK, as for the mask traces, and the buffers keep the guard
                    if kernel != 3 and band % 16 and rows.any():
                        with pytest.raises(api.RtsError):
                            call()
                        _same(dev.read(), _expect(fr.want("point"), None, np.zeros(fr.H, bool)), (band, kernel, with_map, stripe, "refused"))
                        continue
                    call()
                    if rows.any():                       # the instantiation: power-of-two bands (8, 16, 32 rows) or the general form (24)
                        want_name = SHARE if kernel != 3 else (PACKET_GENERAL if band == 24 else PACKET_BANDS)
                        assert ctx.last_kernel_name() == want_name, (band, kernel, stripe, ctx.last_kernel_name())
                    _same(dev.read(), _expect(fr.want("point"), active if with_map else None, rows), (band, kernel, with_map, stripe))
    finally:
        ctx.set_option("kernel", -1)
        dev.close()


@pytest.mark.parametrize("key", ["point", "directional"])
def test_dissolving_packets_keep_their_minimum(ctx, key):
    fr = frame(64, 48)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    before = (ctx.get_option("packet_budget"), ctx.get_option("packet_share"))
    try:
        ctx.set_option("packet_budget", 1)
        ctx.set_option("packet_share", 16)
        _trace(ctx, dev, fr, key, ("dissolve", key), kernel=3)
        _trace(ctx, dev, fr, key, ("dissolve", key, "map"), active=_maps(fr, key)["checker"], kernel=3)
    finally:
        ctx.set_option("packet_budget", before[0])
        ctx.set_option("packet_share", before[1])
        ctx.set_option("kernel", -1)
        dev.close()


def _soup(n=600):
    rng = np.random.RandomState(3)
    c = rng.random_sample((n, 1, 3))
    tri = (c + (rng.random_sample((n, 3, 3)) - 0.5) * 0.2).astype(np.float32)
    verts = np.zeros((n * 3, 8), np.float32)
    verts[:, :3] = tri.reshape(-1, 3)
    return verts, np.arange(n * 3, dtype=np.uint32), n


def _check_stream(ctx, packed, pos, k, light, what, kernels=(3, 7, 8), install=True):
    H, W = pos.shape[:2]
    want = api.shadow_distance(packed, k, light, pos, W, H)
    if install:
        ctx.set_bvh(packed)
    dev = _Dev(ctx, pos, W, H)
    try:
        for kernel in kernels:
            ctx.set_option("kernel", kernel)
            dev.guard()
            ctx.trace_shadow_distance_device(k, dev.d_pos, W, H, dev.d_dist, d_mask=dev.d_mask, light=light)
            _same(dev.read(), want, (what, kernel))
    finally:
        ctx.set_option("kernel", -1)
        dev.close()
    return want


def test_streams_of_the_exact_path(ctx):
    fr = frame(64, 48)
    for what, packed in (("infinite root", streams.infinite_root(fr.packed)), ("swapped boxes", streams.swapped_boxes(fr.packed))):
        _check_stream(ctx, packed, fr.pos, fr.k, fr.lights["point"], what)
        if what == "infinite root":
            assert ctx.get_option("bvh_finite") == 0
        else:
            assert ctx.get_option("bvh_ordered") == 0
    good, bad = streams.orphan_streams()
    pos, k = streams.orphan_frame(64, 48)
    w = _check_stream(ctx, bad, pos, k, None, "orphans")
    assert 0 < int((bits(w[0]) != INF_BITS).sum()) < w[0].size
    tri, _ = streams.degenerate_triangles()              # NaN contributions on the device: +0
    verts = np.zeros((tri.shape[0] * 3, 8), np.float32)
    verts[:, :3] = tri.reshape(-1, 3)
    packed = api.BVHBuilder().build(verts, 8, np.arange(tri.shape[0] * 3, dtype=np.uint32), tri.shape[0]).m_packedNodes
    pos, k, light = streams.aimed_frame(packed, 0, 48, 32)
    w = _check_stream(ctx, packed, pos, k, light, "degenerate triangles")
    assert int((bits(w[0]) == 0).sum()) > 0


def test_median_split_and_device_built_then_refitted_streams(ctx):
    verts, idx, n = _soup()
    packed = api.BVHBuilder(sah_prim_limit=32).build(verts, 8, idx, n).m_packedNodes       # median splits above 32 triangles
    pos, k, light = streams.aimed_frame(packed, 0, 48, 32)
    w = _check_stream(ctx, packed, pos, k, light, "median split")
    assert 0 < int((bits(w[0]) != INF_BITS).sum()) < w[0].size
    api.bvh_build_device(ctx, verts, 8, idx, n, install=True, want_packed=False)
    moved = verts.copy()
    moved[:, :3] += (np.random.RandomState(9).random_sample((n, 1, 3)).repeat(3, 0).reshape(-1, 3) * 0.05).astype(np.float32)
    refitted, _, _ = api.bvh_refit_device(ctx, moved, 8, idx, n, want_packed=True)
    _check_stream(ctx, refitted, pos, k, light, "device-built, refitted", install=False)


@pytest.mark.parametrize("kernel", list(range(-1, 10)))
def test_far_before_near_under_every_kernel(ctx, kernel):
    packed, k, pos = far_before_near_frame()
    H, W = pos.shape[:2]
    ctx.set_bvh(packed)
    try:
        ctx.set_option("kernel", kernel)
        d, m = ctx.trace_shadow_distance(k, pos, W, H)
        assert ctx.last_kernel_name() == _name(kernel, W * H)
        want = api.shadow_distance(packed, k, None, pos, W, H)
        assert np.array_equal(bits(d), bits(want[0])) and np.array_equal(m, want[1])
        assert (np.abs(d - 2.0) < 1e-3).all() and (m == 0).all()         # the near triangle's t (the walk meets the one at 5 first)
        _, rays, near = far_before_near()
        assert (ctx.trace_rays_distance(rays) == near).all()
    finally:
        ctx.set_option("kernel", -1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_generic_rays(ctx, n):
    fr = frame(64, 48)
    ctx.set_bvh(fr.packed)
    rays = generic_rays(fr.packed, 4096)[:n]
    want = api.rays_distance(fr.packed, rays)
    for kernel in (-1, 3):                               # generic rays always run lane per ray
        ctx.set_option("kernel", kernel)
        got = ctx.trace_rays_distance(rays)
        assert ctx.last_kernel_name() == RAYS
        assert np.array_equal(bits(got), bits(want)), (n, kernel, int((bits(got) != bits(want)).sum()))
    ctx.set_option("kernel", -1)
    if n == 4096:
        assert 0 < int((bits(want) != INF_BITS).sum()) < n


def test_auto_takes_the_packet_from_256k_pixels(ctx):
    fr = frame(640, 416)                                 # 266 240 pixels: just above 256 K
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        assert ctx.get_option("kernel") == -1
        _trace(ctx, dev, fr, "point", "640 x 416, defaults")
        assert ctx.last_kernel_name() == PACKET
        _trace(ctx, dev, fr, "point", "640 x 416, facing map", active=api.facing_active(fr.k, fr.lights["point"], fr.pos, fr.nrm))
        assert ctx.last_kernel_name() == PACKET
    finally:
        dev.close()


def test_counter_and_untouched_options(ctx):
    fr = frame(64, 48)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    keys = ["kernel", "xcd_swizzle", "packet_budget", "packet_share", "block_waves", "row_order", "wide_lane", "soft_split", "tile_splits",
            "follow", "tile_order", "tile_order_tiles", "active_traces", "follow_traces"]
    try:
        ctx.set_option("kernel", 3)
        order = np.arange(((fr.W + 7) // 8) * ((fr.H + 7) // 8), dtype=np.uint32)[::-1].copy()
        ctx.set_tile_order(order)
        before = {k: ctx.get_option(k) for k in keys}
        assert before["tile_order_tiles"] == order.size
        n0 = ctx.get_option("distance_traces")
        _trace(ctx, dev, fr, "point", "counter", kernel=3)
        ctx.trace_shadow_distance_stripes_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, 16, 2, 1, light=fr.lights["point"])
        ctx.trace_shadow_distance_stripes_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, 32, 3, 2, light=fr.lights["point"])   # owns no band: no launch
        ctx.trace_rays_distance(generic_rays(fr.packed, 64))
        ctx.synchronize()
        assert ctx.get_option("distance_traces") == n0 + 3
        assert {k: ctx.get_option(k) for k in keys} == before
        with pytest.raises(api.RtsError):                # read-only
            ctx.set_option("distance_traces", 0)
        soft = api.Light.make(api.Light.POINT, fr.lights["point"].xyz, np.zeros((4, 3), np.float32))
        with pytest.raises(api.RtsError):                # one sample in this version
            ctx.trace_shadow_distance_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, light=soft)
        # the installed order still drives the plain trace
        ctx.trace_shadow_mask_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_mask, light=fr.lights["point"])
        ctx.synchronize()
        assert np.array_equal(dev.read()[1], fr.want("point")[1])
    finally:
        ctx.set_tile_order(None)
        ctx.set_option("kernel", -1)
        dev.close()


def _copy(struct):
    return type(struct).from_buffer_copy(struct) if struct is not None else None


@pytest.mark.parametrize("form", ["whole", "rows", "stripe", "rays"])
@pytest.mark.parametrize("kernel", [3, 7])
def test_device_forms_under_capture(ctx, kernel, form):
    fr = frame(64, 48)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    active = _maps(fr, "point")["checker"]
    ctx.h2d(dev.d_act, active)
    stream = ctx.stream_create()
    k, light = _copy(fr.k), _copy(fr.lights["point"])
    n = 1000
    rays = generic_rays(fr.packed, n)
    d_rays, d_t = ctx.malloc(n * 32), ctx.malloc(n * 4)
    g = None
    try:
        ctx.set_option("kernel", kernel)
        ctx.trace_shadow_mask_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_mask, light=fr.lights["point"], stream=stream)   # a stream that has traced
        ctx.synchronize(stream)
        rows = None
        if form == "whole":
            record = lambda: ctx.trace_shadow_distance_device(k, dev.d_pos, fr.W, fr.H, dev.d_dist, d_mask=dev.d_mask, light=light,
                                                              stream=stream, d_active=dev.d_act)
        elif form == "rows":
            rows = (np.arange(fr.H) >= 5) & (np.arange(fr.H) < 41)
            record = lambda: ctx.trace_shadow_distance_device(k, dev.d_pos, fr.W, fr.H, dev.d_dist, d_mask=dev.d_mask, light=light,
                                                              stream=stream, d_active=dev.d_act, row_begin=5, row_end=41)
        elif form == "stripe":
            rows = ((np.arange(fr.H) // 16) % 2) == 1
            record = lambda: ctx.trace_shadow_distance_stripes_device(k, dev.d_pos, fr.W, fr.H, dev.d_dist, 16, 2, 1, d_mask=dev.d_mask,
                                                                      light=light, stream=stream, d_active=dev.d_act)
        else:
            record = lambda: ctx.trace_rays_distance_device(d_rays, n, d_t, stream=stream)
        n0 = ctx.get_option("distance_traces")
        g = hipgraph.capture(stream, record)
        assert ctx.get_option("distance_traces") == n0 + 1
        types = g.node_types()
        assert types == [hipgraph.KERNEL], (kernel, form, types)          # one kernel node; no memcpy, memset or allocation node
        for s in (k, light):                             # what a caller may do to its structs between capture and replay
            C.memset(C.byref(s), 0x7F, C.sizeof(s))
        for replay in range(2):
            if form == "rays":
                ctx.h2d(d_rays, rays)
                ctx.h2d(d_t, np.full(n, GUARD_F, np.float32))
                g.launch(stream)
                ctx.synchronize(stream)
                got = np.empty(n, np.float32)
                ctx.d2h(got, d_t)
                assert np.array_equal(bits(got), bits(api.rays_distance(fr.packed, rays))), (kernel, form, replay)
            else:
                dev.guard()
                g.launch(stream)
                _same(dev.read(stream), _expect(fr.want("point"), active, rows), (kernel, form, replay))
    finally:
        if g:
            g.close()
        ctx.synchronize(stream)
        ctx.stream_destroy(stream)
        ctx.set_option("kernel", -1)
        ctx.free(d_rays)
        ctx.free(d_t)
        dev.close()
