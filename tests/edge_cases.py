"""Shared by tests/test_edge_cases_host.py (CPU) and tests/test_gpu_edge_traces.py (GPU): the inputs on which the light-list, distance
and soft-distance kernels could part from the mask traces without the cornell suites noticing, the expected values from the oracle's
definitions alone, and the guards that keep every case from degenerating.  No test lives here.

Nothing is restated: the gate frame, its lights and its edge maps are those of tests/test_gpu_ray_setup.py and section 4 of
tests/test_gpu_active_edges.py, the awkward streams are `_stream_case` of the latter, and the definitions are
light_list_cases.definition, soft_distance_cases.definition and distance_cases.bisect_distance.

* The gate frame: streams.gate_soup under `_frame` (96 x 64; texels at 0, -0, denormal, 2^-114..2^-112, 1e30, 3e38, +-Inf, NaN, one
  bad lane in a good tile, whole tiles of edge values, and the texel at (20, 40) the light `on_texel` sits on).
* The gate list: eight lights, bits 0..5 the six of test_gpu_ray_setup.LIGHTS in the order of GATE_LIST, bit 6 an ordinary point
  light, bit 7 light 1 with a negative zero -- a list light is taken as given, and the oracle tells the two apart by one pixel.
* The per-light edge maps: the maps a, b, c of `_edge_maps` (the first walker is an edge texel / a later walker is / only edge texels
  walk) packed as a | b<<1 | c<<2 | a<<3 | b<<4 | c<<5 | a<<6 | c<<7, so that in one tile consecutive lights have different walkers,
  and the complement of that byte below the count.
* The stream lists: per stream of STREAMS its point light, the directional light of its constants and the point light moved sideways
  by a tenth of its distance from the mean texel.

The guards are computed from the oracle's result alone and never lowered: without a map every light of a list has at least LEAST = 32
lit and 32 occluded pixels, with a map a 0 and a 1 among its marked pixels; a distance on the gate frame holds 32 pixels of each of
+Inf, +0 and finite positive; the soft light on the gate frame 32 of each of all-lit, all-occluded and penumbra.  On the awkward
streams and the refitted stream, where nothing was measured beforehand, a distance or soft distance must show a blocked and an
unblocked pixel (one pixel of each class the oracle can be asked for there), so that no constant passes.  No seed and no radius had
to be changed to meet them."""
import numpy as np

import streams
from distance_cases import INF_BITS, bisect_distance, bits, frame_rays
from light_list_cases import definition as list_definition
from raytracedshadows_amd import api
from soft_distance_cases import classes, definition as soft_definition
from test_gpu_active_edges import STREAMS, _check_edge_maps, _edge_maps, _gate_lights, _stream_case
from test_gpu_ray_setup import EDGE, LIGHTS, _frame

LEAST = 32
GATE_LIST = ("on_texel", "directional_axis", "above", "far", "huge", "directional")
GATE_EXTRA = ((api.Light.POINT, (0.2, 0.9, 0.7)), (api.Light.DIRECTIONAL, (-0.0, 1.0, 0.0)))
ON_TEXEL = (20, 40)                                      # (row, column) of the texel the light `on_texel` sits on
HOST_STREAMS = [s for s in STREAMS if s not in ("lbvh", "ploc")]
FORMS = [(7, 1), (3, 1), (3, 0)]                         # ("kernel", "soft_split") of the list and soft-distance traces

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


# ---- the gate frame ---------------------------------------------------------------------------------------------------------------
class Gate:
    """packed, pos[64, 96, 4], k, maps {"a", "b", "c"} (checked by _check_edge_maps), ids (the edge value of each coordinate, -1: none)."""

    def __init__(self):
        self.packed, tri = streams.gate_soup()
        self.pos = _frozen(_frame(tri))
        self.H, self.W = self.pos.shape[:2]
        self.k = api.RayTracingConstants.make([0, 0, 0], [0.3, 0.8, 0.5], self.W, self.H)
        self.maps, self.ids = _edge_maps(self.pos)
        _check_edge_maps(self.maps, self.ids)
        assert (self.pos[ON_TEXEL][:3] == 0.5).all()


def gate():
    return _once("gate", Gate)


def gate_list(count=8):
    """The first `count` lights of the gate list."""
    entries = [(LIGHTS[n][0], LIGHTS[n][1]) for n in GATE_LIST] + list(GATE_EXTRA)
    lights = api.LightList.make(entries[:count])
    if count == 8:                                       # the negative zero travels
        assert bits(np.float32(lights.lights[7].xyz[0])) == 0x80000000 and bits(np.float32(lights.lights[1].xyz[0])) == 0
    return lights


def gate_light(name):
    """A one-light entry: one of LIGHTS, or "soft16_on_texel"."""
    return _gate_lights()[name]


def list_maps(maps, count=8):
    """{"edges", "complement"}: the per-light packing of the maps a, b, c, and its complement below the count."""
    a, b, c = (maps[kind].astype(np.uint8) & 1 for kind in "abc")
    below = np.uint8((1 << count) - 1)
    m = (a | b << 1 | c << 2 | a << 3 | b << 4 | c << 5 | a << 6 | c << 7).astype(np.uint8)
    return {"edges": _frozen(m & below), "complement": _frozen(~m & below)}


def lone_map(H, W):
    """One marked pixel of one light in the whole frame: bit 0 (`on_texel`) of the texel that light sits on."""
    m = np.zeros((H, W), np.uint8)
    m[ON_TEXEL] = 1
    return m


# ---- the guards, from the oracle's result alone -----------------------------------------------------------------------------------
def lit_counts(want, count):
    return [int(((want >> l) & 1).sum()) for l in range(count)]


def guard_list(want, count, what, lights_map=None):
    """`want`: the definition WITHOUT a map.  No map: every light has LEAST lit and LEAST occluded pixels; with one: a 0 and a 1 among
    the pixels marked for it.  Bits from the count up are clear."""
    assert (want >> count == 0).all(), what
    for l in range(count):
        bit = (want >> l) & 1
        if lights_map is None:
            lit = int(bit.sum())
            assert lit >= LEAST and bit.size - lit >= LEAST, (what, l, lit, bit.size)
        else:
            on = bit[((lights_map >> l) & 1) != 0]
            assert on.size and (on == 0).any() and (on == 1).any(), (what, l, int(on.size), int(on.sum()))


def distance_classes(d):
    """(+Inf, +0, finite positive) pixel counts; a definition takes no other value."""
    b = bits(d)
    inf, zero = int((b == INF_BITS).sum()), int((b == 0).sum())
    positive = int(((b > 0) & (b < INF_BITS)).sum())
    assert inf + zero + positive == b.size
    return inf, zero, positive


def guard_distance(d, what, active=None, least=LEAST):
    """least = LEAST: the gate frame's three classes.  least = 0: an awkward stream -- a blocked and an unblocked pixel."""
    got = distance_classes(d if active is None else d[active != 0])
    if least:
        assert min(got) >= (least if active is None else 1), (what, got)
    else:
        assert got[0] >= 1 and got[1] + got[2] >= 1, (what, got)
    return got


def guard_soft(m, n, what, active=None, least=LEAST):
    """(all lit, all occluded, penumbra) of a count mask: LEAST of each on the gate frame, else one all-lit and one blocked pixel."""
    got = classes(m if active is None else m[active != 0], n)
    if least:
        assert min(got) >= (least if active is None else 1), (what, got)
    else:
        assert got[0] >= 1 and got[1] + got[2] >= 1, (what, got)
    return got


# ---- the definitions --------------------------------------------------------------------------------------------------------------
def list_want(packed, k, lights, pos):
    return _frozen(list_definition(packed, k, lights, pos))


def distance_want(packed, k, light, pos):
    """(float32[H, W], uint8[H, W]): the bisected any-hit, and the mask byte beside it (1 where the ray is lit)."""
    H, W = pos.shape[:2]
    d = bisect_distance(packed, frame_rays(k, light, pos)).reshape(H, W)
    return _frozen(d, (bits(d) == INF_BITS).astype(np.uint8))


def soft_want(packed, k, light, pos):
    return _frozen(*soft_definition(packed, k, light, pos))


def under_map(want, active):
    """What a distance or soft-distance trace leaves under an active map: +0 and 0 where the pixel is not active."""
    d, m = want
    return np.where(active != 0, d, np.float32(0.0)).astype(np.float32), (m * (active != 0)).astype(np.uint8)


def gate_list_want():
    g = gate()
    return _once("gate list", lambda: list_want(g.packed, g.k, gate_list(), g.pos))


def gate_distance_want(name):
    g = gate()
    return _once(("gate distance", name), lambda: distance_want(g.packed, g.k, gate_light(name), g.pos))


def gate_soft_want():
    g = gate()
    return _once("gate soft", lambda: soft_want(g.packed, g.k, gate_light("soft16_on_texel"), g.pos))


# ---- the stream lists -------------------------------------------------------------------------------------------------------------
def stream_list(pos, k, point):
    """The case's point light, the directional light of k.lightDirection, and the point light moved sideways by a tenth of its
    distance from the mean texel, along cross(p - c, (0.3, -0.2, 0.9))."""
    p = np.array(list(point.xyz), np.float64)
    c = np.asarray(pos, np.float64).reshape(-1, 4)[:, :3].mean(0)
    side = np.cross(p - c, np.array([0.3, -0.2, 0.9]))
    moved = p + 0.1 * np.linalg.norm(p - c) * side / np.linalg.norm(side)
    return api.LightList.make([point, (api.Light.DIRECTIONAL, list(k.lightDirection)[:3]), (api.Light.POINT, moved.astype(np.float32))])


def stream_soft_light(pos, point, n=4, seed=29):
    """A point light of `n` samples and no table, of radius 0.05 times the light's distance from the mean texel."""
    p = np.array(list(point.xyz), np.float64)
    c = np.asarray(pos, np.float64).reshape(-1, 4)[:, :3].mean(0)
    offsets = np.zeros((n, 4), np.float32)
    offsets[:, :3] = (np.random.RandomState(seed).random_sample((n, 3)) * 2 - 1) * 0.05 * np.linalg.norm(p - c)
    light = api.Light.make(api.Light.POINT, list(point.xyz), offsets)
    assert light.nsamples == n and light.table == 0
    return light


def stream_case(name, ctx=None):
    """_stream_case with positions as [H, W, 4]; with a context, `lbvh` and `ploc` are built and installed on the device."""
    packed, pos, k, point, options = _stream_case(name, ctx)
    side = 160 if name == "unordered" else 64
    return packed, np.ascontiguousarray(pos, np.float32).reshape(side, side, 4), k, point, options


# ---- the tall frames of the 1-D grid ----------------------------------------------------------------------------------------------
def tall_positions(texels, H, W=3):
    """The texels repeated down a W x H frame in row-major order: pixel i holds texel i mod len(texels)."""
    return np.resize(np.asarray(texels, np.float32).reshape(-1, 4), (H, W, 4))


def tall(per_texel, H, W=3):
    """A per-texel result repeated the same way."""
    return np.resize(np.asarray(per_texel).ravel(), (H, W))
