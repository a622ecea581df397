"""Shared by tests/test_ao_edge_cases_host.py (CPU) and tests/test_gpu_ao_edges.py (GPU): the inputs of tests/edge_cases.py -- the
gate frame and its edge maps, the awkward streams, a refit, the tall frames of the 1-D grid -- under ambient occlusion
(rts_trace_ambient_occlusion*, include/rts.h), the expected count planes from the oracle alone, and the guards that keep
every case from degenerating.  No test lives here.

Everywhere want[p] = sum over j of oracle.trace_rays(packed, rays)[p, j], the rays from ao_cases.rays_rule (the numpy float32
restatement of the header's text); 0 where the pixel is background or inactive.  No host twin stands in between.

* The gate frame: edge_cases.gate() with normals made here.  Pixel (x, y) takes entry (x + 3 y) mod 8 of NORMALS; the background is
  (5 x + 11 y) mod 37 == 9, written as (0, -0, 0) where x + y is even; the WILD normals ((0, 2, 0), (0, 1e-30, 0), (0, 1e30, 0), one
  with a NaN and one with an Inf component) sit on ordinary texels; the tile NONUNIT_TILE holds the list's normals times 3 and times
  0.25.  Direction sets: AoParams.make (seed 3) with (n, table) of GATE_SETS and the exact axis set AXIS (n = 3, table 0).  Radii:
  GATE_RADII -- the ordinary one, 0, a negative one, the denormal 1e-40 and 3e38.  Maps: a, b, c of Gate.maps, the lone pixel and
  lane63_map (the only marked pixel of every other tile is its lane 63, edge tiles included).
* The streams: the ten of edge_cases.STREAMS; the normal is the unit vector from the texel (camera + rel, float64, rounded once)
  towards the stream's point light, all-zero where the texel is not finite; (n, table) of STREAM_SETS.
* The refit: cornell 160 x 160, geometric normals (ao_cases.geometric_normals), n = 4, and vertices moved by a smooth finite field.
* The tall and the wide frames: the 65 536 texels of cornell_256 with geometric normals, repeated in row-major order, n = 3.  With
  table 0 a count is a function of the texel alone; with table 6 of (texel, start), so the plane is gathered from six planes of
  explicit rotated directions without a table, start(y * W + x, 6) from the numpy hash32 of soft_list_edge_cases.py.

The guards are computed from the oracle's planes alone, before the first device call, and never lowered.  Gate frame, ordinary
radius, without a map: LEAST = 32 pixels at 0, at n and strictly between, counted over the pixels whose texel and normal are both
ordinary.  Streams, the refit, the tall texels: a pixel with count < n and one with count > 0.  Under a map: a zero and a non-zero
count among the marked pixels (the lone map marks one pixel: the maps traced beside it carry that guard).

Ladder picks and class counts (at 0 / at n / between; tests/test_ao_edge_cases_host.py pins them):
* Gate frame, 5244 ordinary pixels, ladder 0.02, 0.05, 0.1, 0.2, 0.5 of the soup's diagonal (4.3745), picked per direction set:
    (4, 0)   0.02: 39 / 2894 / 2311      (5, 8)   0.02: 40 / 2719 / 2485      axis     0.02: 52 / 3175 / 2017
    (16, 16) 0.2:  46 / 85 / 5113   (0.02: 4 / 1098 / 4142, 0.05: 5 / 196 / 5043, 0.1: 13 / 108 / 5123)
    (48, 64) NO entry meets the guard: 5 / 424 / 4815, 5 / 68 / 5171, 6 / 50 / 5188, 10 / 36 / 5198, 15 / 28 / 5201.  The set is kept at
             0.5, the entry whose smallest class is largest, under the guard that entry meets: a pixel at 0, one at n, LEAST between.
  Set (5, 8) over the 5979 live pixels at the other radii: zero 0 / 5979 / 0 (every ray is NaN and unoccluded), negative
  91 / 3251 / 2637, denormal 1 / 5978 / 0, huge 5214 / 337 / 428.  Marked pixels at 0 / not at 0 under the maps (set (5, 8)):
  a 101 / 2676, b 104 / 2909, c 18 / 667, lane63 2 / 46; the lone pixel's count is 4 of 5.
* Streams, ladder 0.25, 0.5, 1.0 of the light's distance, sets (4, 0) and (5, 8) over the live pixels: `unordered` 0.25:
  0 / 23347 / 2253 and 0 / 23691 / 1909; `orphans` 0.25: 0 / 3233 / 863, 0 / 2828 / 1268; `one_triangle` and `two_triangles` 0.25:
  0 / 3342 / 754, 0 / 3139 / 957; `deep_bushy` 0.25: 0 / 1863 / 2233, 0 / 1370 / 2726.  On `non_finite`, `degenerate`, `median_split`,
  `lbvh` and `ploc` NO entry meets the guard: with the normal towards the light every segment is free (0 / 4096 / 0 at all three),
  and so is every segment with the radius negated.  They are kept at 1.0 under the guard that meets: a pixel with count > 0.
* The refit, 0.1 of the texels' diagonal: 0 / 20299 / 1694.  The tall texels, 0.1: table 0 5 / 53460 / 3106; start 0 of table 6
  39 / 54474 / 2058."""
import numpy as np

import ao_cases as ac
import oracle
import streams
from edge_cases import FORMS, LEAST, ON_TEXEL, STREAMS, gate, lone_map, stream_case, tall, tall_positions  # noqa: F401  (re-exported to the tests)
from raytracedshadows_amd import api, workloads
from soft_list_edge_cases import start

f32 = np.float32
GUARD = ac.GUARD
SEED = 3

#: ---- the gate frame
NORMALS = ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.6, 0.8, 0.0), (0.6, 0.8, -0.0), (1.0, 0.0, 0.0), (-0.48, 0.6, 0.64),
           tuple(np.array([0.3, 0.8, 0.5]) / np.linalg.norm([0.3, 0.8, 0.5])))
WILD = {(25, 9): (0.0, 2.0, 0.0), (33, 50): (0.0, 1e-30, 0.0), (41, 77): (0.0, 1e30, 0.0), (49, 14): (np.nan, 0.5, 0.5),
        (57, 90): (np.inf, 0.0, 1.0)}                     # (row, column) -> normal
NONUNIT_TILE = (4, 2)                                     # (tile row, tile column): rows 32..39, columns 16..23
GATE_SETS = ((4, 0), (5, 8), (16, 16), (48, 64), "axis")
AXIS = np.array([(0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, -1.0, 0.0)], f32)
GATE_LADDER = (0.02, 0.05, 0.1, 0.2, 0.5)                 # of the soup's diagonal
#: per set the first entry of the ladder that meets the guard; none does for GATE_UNMET, which keeps the entry whose smallest class is
#: largest under the guard that entry meets: a pixel at 0, one at n and LEAST between
GATE_SHARES = {(4, 0): 0.02, (5, 8): 0.02, (16, 16): 0.2, (48, 64): 0.5, "axis": 0.02}
GATE_UNMET = ((48, 64),)
GATE_RADII = ("ordinary", "zero", "negative", "denormal", "huge")
GATE_MAPS = ("a", "b", "c", "lone", "lane63")
HOST_ROWS = (5, 61)                                       # the host-form call, with set (5, 8)

#: ---- the streams
STREAM_SETS = ((4, 0), (5, 8))
STREAM_LADDER = (0.25, 0.5, 1.0)                          # of the light's distance from the mean texel
#: per stream the first entry that meets the guard in both sets; on STREAM_UNMET no entry does (every segment towards the light is
#: free: the planes are n on all 4096 pixels at 0.25, 0.5 and 1.0), so they keep the longest one under the guard it meets: a pixel
#: with count > 0
STREAM_UNMET = ("non_finite", "degenerate", "median_split", "lbvh", "ploc")
STREAM_SHARE = {name: (1.0 if name in STREAM_UNMET else 0.25) for name in STREAMS}

#: ---- the refit, the tall frames, the options frame
REFIT_SHARE = 0.1                                         # of the diagonal of the texels
TALL_SHARE = 0.1
TALL_TABLE = 6

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- the expectation: the oracle's sum over the rule's rays -----------------------------------------------------------------------
def live(nrm, active=None):
    on = ~(np.asarray(nrm)[..., :3] == 0).all(-1)
    return on if active is None else on & (np.asarray(active) != 0)


def want(packed, k, ao, pos, nrm):
    """uint8[H, W] WITHOUT a map: per pixel the sum of the oracle's any-hit bytes over the rule's rays; 0 on the background."""
    H, W = pos.shape[:2]
    unoccluded, _, _ = oracle.trace_rays(packed, ac.rays_rule(k, ao, pos, nrm))
    return _frozen(np.where(live(nrm), unoccluded.reshape(H, W, ao.samples).sum(-1), 0).astype(np.uint8))


def under(plane, active):
    """What an AO trace leaves under an active map: 0 where the pixel is not marked."""
    return np.where(np.asarray(active) != 0, plane, 0).astype(np.uint8)


def classes(plane, n, where=None):
    """(at 0, at n, strictly between) over the pixels of `where`."""
    v = plane[where] if where is not None else plane.ravel()
    at0, atn = int((v == 0).sum()), int((v == n).sum())
    return at0, atn, int(v.size) - at0 - atn


def guard_gate(plane, n, what, unmet=False):
    """LEAST ordinary pixels at 0, at n and between; a set of GATE_UNMET: one at 0, one at n and LEAST between."""
    got = classes(plane, n, gate_ordinary())
    assert (min(got[:2]) >= 1 and got[2] >= LEAST) if unmet else min(got) >= LEAST, (what, got)
    return got


def guard_some(plane, n, what, where=None):
    """A pixel with count < n and one with count > 0 among the live ones: no constant passes."""
    v = plane[where] if where is not None else plane.ravel()
    assert (v < n).any() and (v > 0).any(), (what, classes(plane, n, where))


def guard_map(plane, active, what):
    on = plane[np.asarray(active) != 0]
    assert on.size and (on == 0).any() and (on != 0).any(), (what, int(on.size), int((on != 0).sum()))


def first_of(ladder, meets):
    """The first entry of the ladder that meets the guard, else None."""
    for share in ladder:
        if meets(share):
            return share
    return None


# ---- the gate frame ---------------------------------------------------------------------------------------------------------------
def gate_diagonal():
    tri = _once("soup", lambda: streams.gate_soup()[1]).reshape(-1, 3).astype(np.float64)
    return float(np.linalg.norm(tri.max(0) - tri.min(0)))


def _gate_planes():
    def make():
        g = gate()
        y, x = np.mgrid[0:g.H, 0:g.W]
        nrm = np.zeros((g.H, g.W, 4), f32)
        nrm[..., :3] = np.array(NORMALS, np.float64).astype(f32)[(x + 3 * y) % 8]
        ty, tx = NONUNIT_TILE
        tile = (y >> 3 == ty) & (x >> 3 == tx)
        nrm[tile, :3] *= np.where((x + y) % 2 == 0, f32(3.0), f32(0.25))[tile][:, None]
        wild = np.zeros((g.H, g.W), bool)
        for at, v in WILD.items():
            nrm[at][:3] = np.array(v, f32)
            wild[at] = True
        background = (5 * x + 11 * y) % 37 == 9
        nrm[background] = 0
        nrm[background & ((x + y) % 2 == 0), 1] = f32(-0.0)              # a negative zero is still background
        plain_texel = (g.ids < 0).all(-1)
        assert not (wild & background).any() and plain_texel[wild].all() and not (wild & tile).any()
        assert np.signbit(nrm[..., 1][background]).sum() >= 8 and (~np.signbit(nrm[..., 1][background])).sum() >= 8
        assert not background[ON_TEXEL]
        return _frozen(nrm), _frozen(background), _frozen(wild), _frozen(plain_texel & ~background & ~wild & ~tile)
    return _once("gate planes", make)


def gate_normals():
    return _gate_planes()[0]


def gate_wild():
    return _gate_planes()[2]


def gate_ordinary():
    """bool[H, W]: the texel and the normal are both ordinary (no edge value, not background, not wild, not in the non-unit tile)."""
    return _gate_planes()[3]


def gate_radius(key, name):
    r = GATE_SHARES[key] * gate_diagonal()
    return {"ordinary": r, "zero": 0.0, "negative": -r, "denormal": 1e-40, "huge": 3e38}[name]


def gate_ao(key, radius):
    """`key`: (n, table) of AoParams.make, or "axis"."""
    if key == "axis":
        return api.AoParams.make(3, radius, table=0, dirs=AXIS)
    return api.AoParams.make(key[0], radius, table=key[1], seed=SEED)


def gate_want(key, rname, share=None):
    """The oracle's plane of a direction set at a named radius (or, with `share`, at that share of the diagonal)."""
    g = gate()
    radius = gate_radius(key, rname) if share is None else share * gate_diagonal()
    return _once(("gate", key, rname, share), lambda: want(g.packed, g.k, gate_ao(key, radius), g.pos, gate_normals()))


def gate_rows_wrong():
    """What a kernel that hashed the index inside the rows HOST_ROWS would write there under set (5, 8): those rows as a frame of
    their own."""
    g = gate()
    r0, r1 = HOST_ROWS
    ao = gate_ao((5, 8), gate_radius((5, 8), "ordinary"))
    return _once("gate rows", lambda: want(g.packed, g.k, ao, g.pos[r0:r1], gate_normals()[r0:r1]))


def lane63_map():
    """The only marked pixel of every other tile is its lane 63 (the tile's bottom-right pixel); the other tiles hold none."""
    g = gate()
    y, x = np.mgrid[0:g.H, 0:g.W]
    m = ((y & 7) == 7) & ((x & 7) == 7) & (((y >> 3) + (x >> 3)) % 2 == 0)
    return _frozen(m.astype(np.uint8))


def gate_maps():
    g = gate()
    return _once("gate maps", lambda: dict({kind: g.maps[kind] for kind in "abc"}, lone=_frozen(lone_map(g.H, g.W)), lane63=lane63_map()))


def first_walkers(active):
    """Per tile with a live pixel under the map: (tile, lane, (row, column)) of the first live lane -- the one every other lane of the
    wave stands in for."""
    g = gate()
    on = live(gate_normals(), active)
    out = []
    for ty in range(g.H // 8):
        for tx in range(g.W // 8):
            lanes = np.flatnonzero(on[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].ravel())
            if lanes.size:
                out.append(((ty, tx), int(lanes[0]), (8 * ty + int(lanes[0]) // 8, 8 * tx + int(lanes[0]) % 8)))
    return out


def walker_tiles(active):
    """Over the tiles with a live pixel under the map: (tiles whose first live lane is an edge texel, tiles whose first live lane is an
    ordinary texel with a live edge texel after it, tiles whose live lanes are all edge texels, tiles with one live lane)."""
    g = gate()
    on, edge = live(gate_normals(), active), (g.ids >= 0).any(-1)
    first = later = only = lone = 0
    for ty in range(g.H // 8):
        for tx in range(g.W // 8):
            sl = (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))
            lanes = np.flatnonzero(on[sl].ravel())
            if lanes.size:
                e = edge[sl].ravel()[lanes]
                first += bool(e[0])
                later += bool(not e[0] and e[1:].any())
                only += bool(e.all())
                lone += lanes.size == 1
    return first, later, only, lone


def guard_gate_all():
    """Every guard of the gate frame: the ordinary radius without a map in every set, and a zero and a non-zero count under every map
    but the lone one (whose pixel is non-zero)."""
    maps = gate_maps()
    for key in GATE_SETS:
        n = gate_ao(key, 1.0).samples
        plane = gate_want(key, "ordinary")
        guard_gate(plane, n, ("gate", key), key in GATE_UNMET)
        for name in GATE_MAPS:
            if name == "lone":
                assert plane[ON_TEXEL] != 0, ("gate", key, "lone")
            else:
                guard_map(plane, maps[name], ("gate", key, name))


# ---- the streams ------------------------------------------------------------------------------------------------------------------
def towards(pos, k, point):
    """float32[H, W, 4]: the unit vector from the texel towards the point light, float64 rounded once; all-zero where the texel is not
    finite (or is the light itself)."""
    cam = np.array([k.cameraPosition[i] for i in range(3)], np.float64)
    v = np.array(list(point.xyz), np.float64) - (cam + np.asarray(pos, np.float64)[..., :3])
    with np.errstate(all="ignore"):
        N = v / np.linalg.norm(v, axis=-1, keepdims=True)
    N[~np.isfinite(N).all(-1) | ~np.isfinite(np.asarray(pos)[..., :3]).all(-1)] = 0
    out = np.zeros(N.shape[:2] + (4,), f32)
    out[..., :3] = N
    return out


def light_distance(pos, k, point):
    """The point light's distance from the mean texel (camera + rel)."""
    cam = np.array([k.cameraPosition[i] for i in range(3)], np.float64)
    c = cam + np.asarray(pos, np.float64).reshape(-1, 4)[:, :3].mean(0)
    return float(np.linalg.norm(np.array(list(point.xyz), np.float64) - c))


def stream_wants(packed, k, pos, point, what):
    """(normals, {(n, table): (ao, plane)}) of a stream at its recorded share of the light's distance, the guard asserted."""
    nrm = towards(pos, k, point)
    radius = STREAM_SHARE[what] * light_distance(pos, k, point)
    out = {}
    for n, table in STREAM_SETS:
        ao = api.AoParams.make(n, radius, table=table, seed=SEED)
        plane = want(packed, k, ao, pos, nrm)
        if what in STREAM_UNMET:
            assert (plane[live(nrm)] > 0).any(), (what, n, table)
        else:
            guard_some(plane, n, (what, n, table), live(nrm))
        out[(n, table)] = (ao, plane)
    return nrm, out


# ---- the refit --------------------------------------------------------------------------------------------------------------------
def normals4(pos):
    nrm = np.zeros(pos.shape[:2] + (4,), f32)
    nrm[..., :3] = ac.geometric_normals(pos)
    return nrm


def texel_diagonal(pos):
    p3 = np.asarray(pos, np.float64)[..., :3].reshape(-1, 3)
    seen = p3[~ac.empty_texels(p3)]
    return float(np.linalg.norm(seen.max(0) - seen.min(0)))


def refit_case():
    """wl (cornell 160 x 160), pos, nrm, k, ao (n = 4, table 0), and `moved`: every vertex displaced by a smooth finite field of its own
    position, so that shared corners stay shared."""
    def make():
        wl = workloads.prepare("cornell", 160, 160, via_obj=False)
        pos = _frozen(np.ascontiguousarray(wl.positions, f32).reshape(wl.H, wl.W, 4).copy())
        nrm = _frozen(normals4(pos))
        ao = api.AoParams.make(4, REFIT_SHARE * texel_diagonal(pos), table=0, seed=SEED)
        moved = wl.vertices.copy()
        v = wl.vertices[:, :3].astype(np.float64)
        moved[:, :3] = (v + 0.2 * np.sin(2.0 * v[:, [1, 2, 0]] + 1.0)).astype(f32)
        return {"wl": wl, "pos": pos, "nrm": nrm, "k": wl.constants, "ao": ao, "moved": _frozen(moved)}
    return _once("refit", make)


def refit_want(packed, what):
    c = refit_case()
    plane = want(packed, c["k"], c["ao"], c["pos"], c["nrm"])
    guard_some(plane, 4, what, live(c["nrm"]))
    return plane


# ---- the tall and the wide frames -------------------------------------------------------------------------------------------------
def tall_case():
    """wl, k, texels and normals [256, 256, 4], ao0 (table 0), ao6 (table 6), `plane0` uint8[256, 256] and `planes6` uint8[6, 256, 256]:
    plane s of the explicit directions dirs[(s + j) mod 6], j < 3, and no table."""
    def make():
        wl = workloads.prepare_config("cornell_256", cache=True)
        texels = _frozen(np.ascontiguousarray(wl.positions, f32).reshape(256, 256, 4).copy())
        nrm = _frozen(normals4(texels))
        radius = TALL_SHARE * texel_diagonal(texels)
        ao0 = api.AoParams.make(3, radius, table=0, seed=SEED)
        ao6 = api.AoParams.make(3, radius, table=TALL_TABLE, seed=SEED)
        dirs = ao6.dirs_array()[:TALL_TABLE, :3]
        plane0 = want(wl.packed, wl.constants, ao0, texels, nrm)
        guard_some(plane0, 3, "tall, table 0", live(nrm))
        planes6 = []
        for s in range(TALL_TABLE):
            rotated = api.AoParams.make(3, radius, table=0, dirs=dirs[[(s + j) % TALL_TABLE for j in range(3)]])
            planes6.append(want(wl.packed, wl.constants, rotated, texels, nrm))
            guard_some(planes6[-1], 3, ("tall, start", s), live(nrm))
        return {"wl": wl, "k": wl.constants, "texels": texels, "nrm": nrm, "ao0": ao0, "ao6": ao6, "plane0": plane0,
                "planes6": _frozen(np.stack(planes6))}
    return _once("tall", make)


def tall_want(t, table, H, W=3, wrong_base=0):
    """uint8[H, W] of the frame that repeats the texels: texel (i mod 65536) at pixel i; with the table the byte is gathered from the
    plane of start(i, 6).  wrong_base != 0: what a kernel that hashed i - wrong_base -- the index inside a row range -- would write."""
    if not table:
        return tall(t["plane0"], H, W)
    index = np.arange(H * W, dtype=np.uint64)
    texel = (index % np.uint64(65536)).astype(np.int64)
    s = start((index - np.uint64(wrong_base)) & np.uint64(0xFFFFFFFF), table).astype(np.int64)
    return t["planes6"].reshape(table, -1)[s, texel].reshape(H, W)


def tall_untabled(t, H, W=3):
    """What a kernel that never looked at the table would write under ao6: the plane of start 0 everywhere."""
    return tall(t["planes6"][0], H, W)
