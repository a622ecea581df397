"""GPU: the light-list, distance and soft-distance traces where their own suites never go (inputs: tests/edge_cases.py) -- edge
texels behind the wave-wide gates of the ray set-up, a list whose lights have different walkers in one tile, the streams the walk
treats specially, a refit that drops the private copy, and frames of more than 65 535 block rows (the 1-D grid).

Everywhere the expected value is the oracle's definition computed here (light_list_cases.definition, the bisected any-hit of
distance_cases, soft_distance_cases.definition): no host twin stands in between.  Masks are compared byte for byte on buffers
pre-filled with 0xAB, distances bit for bit on buffers pre-filled with -123.25 (no definition is negative).  Every test asserts its
guard (tests/edge_cases.py) from the oracle's result alone before its first trace, so that a kernel that writes a constant, or a
light's bit into another position, cannot pass.  Every test restores the options it sets."""
import numpy as np
import pytest

import edge_cases as ec
from distance_cases import bits
from raytracedshadows_amd import api, workloads
from soft_distance_cases import RADIUS_FEW, point_light

pytestmark = pytest.mark.gpu

GUARD = 0xAB
GUARD_F = np.float32(-123.25)
LIST_SHARE, DIST_SHARE, SOFT_SHARE = "shadowLightListShareKernel", "shadowDistanceShareKernel", "shadowSoftDistanceShareKernel"


def _list_name(kernel, split, geom="rows"):
    return LIST_SHARE if kernel == 7 else "shadowLightListPacketKernel<%d,%s>" % (4 if split else 1, geom)


def _dist_name(kernel, geom="rows"):
    return DIST_SHARE if kernel == 7 else "shadowDistancePacketKernel<%s>" % geom


def _soft_name(kernel, split, geom="rows"):
    return SOFT_SHARE if kernel == 7 else "shadowSoftDistancePacketKernel<%d,%s>" % (4 if split else 1, geom)


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


def _reset(ctx):
    for key, v in (("kernel", -1), ("soft_split", 1), ("xcd_swizzle", 0), ("row_order", 0)):
        ctx.set_option(key, v)


def _form(ctx, kernel, split=1):
    ctx.set_option("kernel", kernel)
    ctx.set_option("soft_split", split)


class _Dev:
    """Device buffers of one frame: positions, a map, the mask and the distances."""

    def __init__(self, ctx, positions):
        self.ctx = ctx
        positions = np.ascontiguousarray(positions, np.float32)
        self.H, self.W = positions.shape[:2]
        n = self.W * self.H
        self.d_pos, self.d_map, self.d_mask, self.d_dist = ctx.malloc(positions.nbytes), ctx.malloc(n), ctx.malloc(n), ctx.malloc(n * 4)
        ctx.h2d(self.d_pos, positions)
        self._guard_b, self._guard_f = np.full(n, GUARD, np.uint8), np.full(n, GUARD_F, np.float32)

    def set_map(self, m):
        self.ctx.h2d(self.d_map, np.ascontiguousarray(m, np.uint8))

    def guard(self):
        self.ctx.h2d(self.d_mask, self._guard_b)
        self.ctx.h2d(self.d_dist, self._guard_f)

    def mask(self, what=None):
        m = np.empty((self.H, self.W), np.uint8)
        self.ctx.synchronize()
        self.ctx.d2h(m, self.d_mask if what is None else what)
        return m

    def both(self):
        d = np.empty((self.H, self.W), np.float32)
        m = self.mask()
        self.ctx.d2h(d, self.d_dist)
        return d, m

    def close(self):
        for d in (self.d_pos, self.d_map, self.d_mask, self.d_dist):
            self.ctx.free(d)


def _rows(H, rows):
    return None if rows is None else (np.arange(H) >= rows[0]) & (np.arange(H) < rows[1])


def _same_mask(got, want, what, rows=None):
    if rows is not None:
        want = np.where(rows[:, None], want, GUARD).astype(np.uint8)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (what, bad.size, bad[:4].tolist(), got.ravel()[bad[:4]].tolist(), want.ravel()[bad[:4]].tolist())


def _same_both(got, want, what, rows=None):
    d, m = want
    if rows is not None:
        d = np.where(rows[:, None], d, GUARD_F).astype(np.float32)
    g, w = bits(got[0]), bits(d)
    bad = np.flatnonzero(g.ravel() != w.ravel())
    assert bad.size == 0, (what, "distance", bad.size, bad[:4].tolist(), g.ravel()[bad[:4]].tolist(), w.ravel()[bad[:4]].tolist())
    _same_mask(got[1], m, (what, "mask"), rows)


def _trace_list(ctx, dev, k, lights, want, what, lights_map=None, rows=None):
    """`want`: the definition without a map."""
    if lights_map is not None:
        dev.set_map(lights_map)
    dev.guard()
    kw = {} if rows is None else {"row_begin": rows[0], "row_end": rows[1]}
    ctx.trace_light_list_device(k, lights, dev.d_pos, dev.W, dev.H, dev.d_mask, d_lights_map=dev.d_map if lights_map is not None else None, **kw)
    got = dev.mask()
    _same_mask(got, want if lights_map is None else want & lights_map, what, _rows(dev.H, rows))
    return got


def _trace_distance(ctx, dev, k, light, want, what, active=None, rows=None, soft=False):
    if active is not None:
        dev.set_map(active)
    dev.guard()
    kw = {} if rows is None else {"row_begin": rows[0], "row_end": rows[1]}
    call = ctx.trace_soft_distance_device if soft else ctx.trace_shadow_distance_device
    call(k, dev.d_pos, dev.W, dev.H, dev.d_dist, d_mask=dev.d_mask, light=light, d_active=dev.d_map if active is not None else None, **kw)
    _same_both(dev.both(), want if active is None else ec.under_map(want, active), what, _rows(dev.H, rows))


# ---- a. edge texels, light lists ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,split", ec.FORMS)
def test_gate_list_on_edge_texels(ctx, kernel, split):
    """The whole list, the two per-light edge maps and the lone pixel; then the sub-lists of 1, 2 and 5 lights, which leave waves of
    the four-wave form with one light, with two and with none.  (The lone map marks one pixel of one light, which cannot hold both
    values; the maps traced beside it carry the guard.)"""
    g = ec.gate()
    want = ec.gate_list_want()
    maps = dict(ec.list_maps(g.maps), lone=ec.lone_map(g.H, g.W))
    ec.guard_list(want, 8, "gate list")
    for name in ("edges", "complement"):
        ec.guard_list(want, 8, ("gate list", name), maps[name])
    subs = {}
    for n in (1, 2, 5):
        subs[n] = (ec.gate_list(n), ec.list_want(g.packed, g.k, ec.gate_list(n), g.pos), ec.list_maps(g.maps, n))
        assert np.array_equal(subs[n][1], want & ((1 << n) - 1))         # a bit is a function of its light alone
        ec.guard_list(subs[n][1], n, ("sub-list", n))
        for name in ("edges", "complement"):
            ec.guard_list(subs[n][1], n, ("sub-list", n, name), subs[n][2][name])
    ctx.set_bvh(g.packed)
    dev = _Dev(ctx, g.pos)
    try:
        _form(ctx, kernel, split)
        _trace_list(ctx, dev, g.k, ec.gate_list(), want, (kernel, split, "whole"))
        assert ctx.last_kernel_name() == _list_name(kernel, split), ctx.last_kernel_name()
        for name, m in maps.items():
            got = _trace_list(ctx, dev, g.k, ec.gate_list(), want, (kernel, split, name), lights_map=m)
            assert ctx.last_kernel_name() == _list_name(kernel, split), ctx.last_kernel_name()
            if name == "lone":
                assert np.count_nonzero(got) <= 1
        for n, (lights, sub, sub_maps) in subs.items():
            got = _trace_list(ctx, dev, g.k, lights, sub, (kernel, split, "sub-list", n))
            assert (got >> n == 0).all()
            for name, m in sub_maps.items():
                _trace_list(ctx, dev, g.k, lights, sub, (kernel, split, "sub-list", n, name), lights_map=m)
            assert ctx.last_kernel_name() == _list_name(kernel, split), ctx.last_kernel_name()
    finally:
        _reset(ctx)
        dev.close()


# ---- b. the definition on the device, on edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [3, 7])
def test_bit_l_is_the_active_trace_of_light_l_on_edge_texels(ctx, kernel):
    g = ec.gate()
    lights, want = ec.gate_list(), ec.gate_list_want()
    m = ec.list_maps(g.maps)["edges"]
    ec.guard_list(want, 8, "gate list, edges", m)
    ctx.set_bvh(g.packed)
    dev = _Dev(ctx, g.pos)
    d_one, d_act = ctx.malloc(g.W * g.H), ctx.malloc(g.W * g.H)
    try:
        _form(ctx, kernel)
        got = _trace_list(ctx, dev, g.k, lights, want, (kernel, "list"), lights_map=m)
        for l in range(8):
            ctx.h2d(d_act, np.ascontiguousarray((m >> l) & 1, np.uint8))
            ctx.h2d(d_one, np.full(g.W * g.H, GUARD, np.uint8))
            ctx.trace_shadow_mask_device(g.k, dev.d_pos, g.W, g.H, d_one, light=lights.light(l), d_active=d_act)
            _same_mask((got >> l) & 1, dev.mask(what=d_one), (kernel, "light", l))
    finally:
        _reset(ctx)
        ctx.free(d_one)
        ctx.free(d_act)
        dev.close()


# ---- c. edge texels, distance -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ec.LIGHTS))
def test_gate_distance_on_edge_texels(ctx, name):
    g = ec.gate()
    light, want, active = ec.gate_light(name), ec.gate_distance_want(name), g.maps["a"]
    ec.guard_distance(want[0], name)
    ec.guard_distance(want[0], (name, "a"), active)
    ctx.set_bvh(g.packed)
    dev = _Dev(ctx, g.pos)
    try:
        for kernel in (7, 3):
            ctx.set_option("kernel", kernel)
            _trace_distance(ctx, dev, g.k, light, want, (name, kernel))
            assert ctx.last_kernel_name() == _dist_name(kernel), ctx.last_kernel_name()
            _trace_distance(ctx, dev, g.k, light, want, (name, kernel, "a"), active=active)
            assert ctx.last_kernel_name() == _dist_name(kernel), ctx.last_kernel_name()
    finally:
        _reset(ctx)
        dev.close()


# ---- d. edge texels, soft distance --------------------------------------------------------------------------------------------------
def test_gate_soft_distance_on_edge_texels(ctx):
    g = ec.gate()
    light, want, active = ec.gate_light("soft16_on_texel"), ec.gate_soft_want(), g.maps["a"]
    ec.guard_soft(want[1], 16, "soft16_on_texel")
    ec.guard_soft(want[1], 16, "soft16_on_texel, a", active)
    ec.guard_distance(want[0], "soft16_on_texel", least=0)
    ctx.set_bvh(g.packed)
    dev = _Dev(ctx, g.pos)
    before = ctx.get_option("packet_budget")
    try:
        for kernel, split in ec.FORMS:
            _form(ctx, kernel, split)
            _trace_distance(ctx, dev, g.k, light, want, (kernel, split), soft=True)
            assert ctx.last_kernel_name() == _soft_name(kernel, split), ctx.last_kernel_name()
            _trace_distance(ctx, dev, g.k, light, want, (kernel, split, "a"), active=active, soft=True)
            assert ctx.last_kernel_name() == _soft_name(kernel, split), ctx.last_kernel_name()
        _form(ctx, 3, 1)
        ctx.set_option("packet_budget", 1)               # every packet dissolves at once
        _trace_distance(ctx, dev, g.k, light, want, "dissolve", soft=True)
        _trace_distance(ctx, dev, g.k, light, want, ("dissolve", "a"), active=active, soft=True)
    finally:
        ctx.set_option("packet_budget", before)
        _reset(ctx)
        dev.close()


# ---- e. awkward streams -------------------------------------------------------------------------------------------------------------
def _stream(ctx, name, expect):
    """Installs stream `name` and returns (pos, k, point, expect(packed, pos, k, point)); `expect` computes the oracle's definition
    and asserts its guard.  A host-built stream is installed only after that -- no device call comes first.  `lbvh` and `ploc` come
    from the device's builder, so there the guard is first asserted on the host builder's tree of the same triangles, and again on
    the stream the device returns before anything is traced in it."""
    if name in ("lbvh", "ploc"):
        expect(*ec.stream_case(name)[:4])
        packed, pos, k, point, options = ec.stream_case(name, ctx)       # (built and installed on the device)
        out = expect(packed, pos, k, point)
    else:
        packed, pos, k, point, options = ec.stream_case(name)
        out = expect(packed, pos, k, point)
        ctx.set_bvh(packed)
    for key, val in options.items():
        assert ctx.get_option(key) == val, (name, key)
    if name == "deep_bushy":
        assert ctx.get_option("wide_nodes") > 25
    if name in ("lbvh", "ploc", "median_split", "two_triangles"):
        assert ctx.get_option("wide_nodes") > 0, name
    return pos, k, point, out


@pytest.mark.parametrize("name", ec.STREAMS)
def test_stream_lists_on_awkward_streams(ctx, name):
    def expect(packed, pos, k, point):
        lights = ec.stream_list(pos, k, point)
        want = ec.list_want(packed, k, lights, pos)
        ec.guard_list(want, 3, name)
        return lights, want

    pos, k, point, (lights, want) = _stream(ctx, name, expect)
    dev = _Dev(ctx, pos)
    try:
        for kernel, split in ec.FORMS:
            _form(ctx, kernel, split)
            _trace_list(ctx, dev, k, lights, want, (name, kernel, split))
            assert ctx.last_kernel_name() == _list_name(kernel, split), ctx.last_kernel_name()
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("name", [s for s in ec.STREAMS if s not in ("non_finite", "unordered")])
def test_soft_distance_on_awkward_streams(ctx, name):
    def expect(packed, pos, k, point):
        light = ec.stream_soft_light(pos, point)
        want = ec.soft_want(packed, k, light, pos)
        ec.guard_soft(want[1], 4, name, least=0)
        ec.guard_distance(want[0], name, least=0)
        return light, want

    pos, k, point, (light, want) = _stream(ctx, name, expect)
    dev = _Dev(ctx, pos)
    try:
        for kernel, split in ((7, 1), (3, 1)):
            _form(ctx, kernel, split)
            _trace_distance(ctx, dev, k, light, want, (name, kernel, split), soft=True)
            assert ctx.last_kernel_name() == _soft_name(kernel, split), ctx.last_kernel_name()
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("name", ["one_triangle", "two_triangles", "deep_bushy"])
def test_distance_on_the_smallest_and_the_deepest_stream(ctx, name):
    def expect(packed, pos, k, point):
        wants = {}
        for lname, light in (("point", point), ("directional", None)):
            wants[lname] = (light, ec.distance_want(packed, k, light, pos))
            ec.guard_distance(wants[lname][1][0], (name, lname), least=0)
        return wants

    pos, k, point, wants = _stream(ctx, name, expect)
    dev = _Dev(ctx, pos)
    try:
        for kernel in (7, 3):
            ctx.set_option("kernel", kernel)
            for lname, (light, want) in wants.items():
                _trace_distance(ctx, dev, k, light, want, (name, lname, kernel))
                assert ctx.last_kernel_name() == _dist_name(kernel), ctx.last_kernel_name()
    finally:
        _reset(ctx)
        dev.close()


# ---- f. around a refit that drops the private copy ----------------------------------------------------------------------------------
def test_lists_and_soft_distance_around_a_refit_that_drops_the_copy(ctx):
    """The recipe of test_active_traces_around_a_refit_that_drops_the_copy: finite vertices whose edge overflows to +Inf, then back."""
    wl = workloads.prepare("cornell", 160, 160, via_obj=False)
    pos, k = np.ascontiguousarray(wl.positions, np.float32).reshape(wl.H, wl.W, 4), wl.constants
    lights = api.LightList.make([wl.light, (api.Light.DIRECTIONAL, list(k.lightDirection)[:3]), (api.Light.POINT, (2.0, 8.0, 6.0))])
    soft = point_light(wl, 4, 0, RADIUS_FEW)
    assert soft.nsamples == 4 and soft.table == 0

    def check(packed, what):
        want = ec.list_want(packed, k, lights, pos)
        ec.guard_list(want, 3, what)
        swant = ec.soft_want(packed, k, soft, pos)
        ec.guard_soft(swant[1], 4, what, least=0)
        for kernel, split in ec.FORMS:
            _form(ctx, kernel, split)
            _trace_list(ctx, dev, k, lights, want, (what, kernel, split))
            assert ctx.last_kernel_name() == _list_name(kernel, split), ctx.last_kernel_name()
            _trace_distance(ctx, dev, k, soft, swant, (what, kernel, split, "soft"), soft=True)
            assert ctx.last_kernel_name() == _soft_name(kernel, split), ctx.last_kernel_name()

    ec.guard_list(ec.list_want(wl.packed, k, lights, pos), 3, "refit, before")     # (from the oracle, before any device call)
    ctx.set_bvh(wl.packed)
    dev = _Dev(ctx, pos)
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


# ---- g. more than 65 535 block rows: the 1-D grid -----------------------------------------------------------------------------------
_TALL = {}


def _tall_case():
    """The 65 536 texels of cornell_256 and, per family, the definition on them -- computed once; a tall frame repeats them in
    row-major order, and every expected value is a function of the texel alone (the soft light has no table)."""
    if not _TALL:
        wl = workloads.prepare_config("cornell_256", cache=True)
        k = wl.constants
        texels = np.ascontiguousarray(wl.positions, np.float32).reshape(256, 256, 4)
        lights = api.LightList.make([wl.light, (api.Light.DIRECTIONAL, list(k.lightDirection)[:3]), (api.Light.POINT, (2.0, 8.0, 6.0))])
        soft = workloads.relight(wl, "point", 4, RADIUS_FEW).light
        assert soft.nsamples == 4 and soft.table == 0
        _TALL.update(wl=wl, k=k, texels=texels, lights=lights, soft_light=soft, point=workloads.relight(wl, "point", 1).light,
                     list=ec.list_want(wl.packed, k, lights, texels))
        _TALL["distance"] = ec.distance_want(wl.packed, k, _TALL["point"], texels)
        _TALL["soft"] = ec.soft_want(wl.packed, k, soft, texels)
    return _TALL


def _tall_height(kernel):
    side = 16 if kernel == 7 else 8
    H = side * 65536 + 5
    assert (H + side - 1) // side > 65535 and (H - 2 - 3 + side - 1) // side > 65535     # the row range (3, H - 2) too
    return H


@pytest.mark.parametrize("kernel,split", ec.FORMS)
def test_tall_light_list_takes_the_one_dimensional_grid(ctx, kernel, split):
    t = _tall_case()
    H, W = _tall_height(kernel), 3
    want = ec.tall(t["list"], H)
    m = np.random.RandomState(H + split).randint(0, 256, (H, W)).astype(np.uint8)          # 50 % per bit
    ec.guard_list(t["list"], 3, "tall")
    ec.guard_list(want, 3, "tall, map", m)
    ctx.set_bvh(t["wl"].packed)
    dev = _Dev(ctx, ec.tall_positions(t["texels"], H))
    try:
        _form(ctx, kernel, split)
        for rows in (None, (3, H - 2)):
            _trace_list(ctx, dev, t["k"], t["lights"], want, ("tall", kernel, split, rows), rows=rows)
            assert ctx.last_kernel_name() == _list_name(kernel, split, "general"), ctx.last_kernel_name()
            _trace_list(ctx, dev, t["k"], t["lights"], want, ("tall", kernel, split, rows, "map"), lights_map=m, rows=rows)
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel", [7, 3])
def test_tall_distance_takes_the_one_dimensional_grid(ctx, kernel):
    t = _tall_case()
    H = _tall_height(kernel)
    ec.guard_distance(t["distance"][0], "tall", least=0)
    want = (ec.tall(t["distance"][0], H), ec.tall(t["distance"][1], H))
    ctx.set_bvh(t["wl"].packed)
    dev = _Dev(ctx, ec.tall_positions(t["texels"], H))
    try:
        ctx.set_option("kernel", kernel)
        for rows in (None, (3, H - 2)):
            _trace_distance(ctx, dev, t["k"], t["point"], want, ("tall", kernel, rows), rows=rows)
            assert ctx.last_kernel_name() == _dist_name(kernel, "general"), ctx.last_kernel_name()
    finally:
        _reset(ctx)
        dev.close()


@pytest.mark.parametrize("kernel,split", ec.FORMS)
def test_tall_soft_distance_takes_the_one_dimensional_grid(ctx, kernel, split):
    t = _tall_case()
    H = _tall_height(kernel)
    ec.guard_soft(t["soft"][1], 4, "tall", least=0)
    ec.guard_distance(t["soft"][0], "tall", least=0)
    want = (ec.tall(t["soft"][0], H), ec.tall(t["soft"][1], H))
    ctx.set_bvh(t["wl"].packed)
    dev = _Dev(ctx, ec.tall_positions(t["texels"], H))
    try:
        _form(ctx, kernel, split)
        for rows in (None, (3, H - 2)):
            _trace_distance(ctx, dev, t["k"], t["soft_light"], want, ("tall", kernel, split, rows), rows=rows, soft=True)
            assert ctx.last_kernel_name() == _soft_name(kernel, split, "general"), ctx.last_kernel_name()
    finally:
        _reset(ctx)
        dev.close()
