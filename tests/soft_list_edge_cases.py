"""Shared by tests/test_soft_list_edge_cases_host.py (CPU) and tests/test_gpu_soft_list_edge_traces.py (GPU): the inputs of
tests/edge_cases.py -- the gate frame and its per-light edge maps, the awkward streams, the tall frames of the 1-D grid -- under soft
light lists in their three modes, the expected planes from the oracle's definition alone, and the guards that keep every case from
degenerating.  No test lives here.

A mode is one of MODES: `plain` (the soft list call; as a definition, every probe and table 0), `adaptive` (the probes, no table) and
`jittered` (the probes and the tables).  The expected (counts, refined) of every mode is soft_list_jitter_cases.definition, which
reduces to the adaptive definition with all tables 0 and to the plain list with all probes 0; soft_list_adaptive_cases.under gives the
values under a map.

* The gate soft list: the eight lights of edge_cases.gate_list in its plane order, as GATE_SOFT makes them soft -- `on_texel` with 16
  samples under a probe of 4 and a table of 16, the axis directional light, a hard light, the lights at 3e19 and 1e38 with radii of
  1e19 and 3e37 (radius * offset is rounded on its own and added to a huge position), a soft directional light traced in full, a
  16-sample light of radius 0 under a probe and a table (every sample is the light itself), and the hard directional light with the
  negative zero.  Its sub-lists of 1, 2 and 5 entries leave waves of the four-wave form with few pairs or none in a phase.
* The stream soft list: edge_cases.stream_list made soft -- the point light (4, 8, 0.05 d), the directional light (6, 42, 0.1), the
  moved point light (5, 20, 0.08 d), d the point light's distance from the mean texel; probes (2, 0, 2), tables (8, 6, 0).
* The tall case: the 65 536 texels of cornell_256 under three lights, of which the first has a table of 6.  Without a table a byte is
  a function of the texel alone; with one it is a function of (texel, start), so the expected tall plane is gathered from T planes of
  the definition -- plane s: the derived light with the explicit offsets offsets[(s + j) mod T], j < n, and no table -- with
  start(y * W + x, T) from the numpy hash32 below, written from the text of include/rts.h.  Neither the oracle's hash nor the host
  twin's is asked about a tall frame.

The guards are computed from the oracle's planes alone, before the first device call, and never lowered.  On the gate frame without a
map: a soft light of radius > 0 has LEAST = 32 pixels at 0, at n and strictly between, and with a probe >= 2 LEAST refined pixels; a
hard or radius-0 light has LEAST pixels at 0, LEAST at n and none between.  Under a map every light has a 0 and a non-zero byte among
the pixels marked for it.  In jittered mode one tabled light with a probe differs somewhere from the adaptive mode's plane.  On the
streams and the tall texels, where classes are thinner, every soft light has a pixel in each of the three classes and every refining
light a refined pixel (least = 1), in each of the three modes.

One radius was changed to meet them.  The moved point light of the stream list was specified with a radius of 0.1 d.  At that radius
its plain plane -- the full count c_n of 5 samples -- has no all-occluded pixel on `non_finite` and `median_split` (pixels at 0 / at
n / between: 0 / 1524 / 2572 and 0 / 1555 / 2541), though the planes its probe gives hold all three classes.  At 0.08 d
(STREAM_MOVED_RADIUS) every mode holds them on all ten streams (the plain plane: 30 / 1614 / 2452 and 7 / 1660 / 2429); at 0.06 d
and below the probe of `one_triangle` no longer refines.  No other radius and no seed was changed.  The tall case's third light,
whose radius was left open, takes TALL_RADIUS = 0.9, the radius the cornell lists of tests/soft_list_cases.py give a light of
5 samples from slot 20."""
import numpy as np

import adaptive_cases
import edge_cases as ec
import soft_list_jitter_cases as sjc
from edge_cases import FORMS, HOST_STREAMS, LEAST, STREAMS, gate, list_maps, lone_map, stream_case, tall, tall_positions  # noqa: F401
from raytracedshadows_amd import api, workloads
from soft_distance_cases import RADIUS_FEW
from soft_list_adaptive_cases import under  # noqa: F401  (re-exported to the tests)
from soft_list_cases import TABLE, samples

MODES = ("plain", "adaptive", "jittered")

#: per entry of the gate list: (samples, first, radius), None: hard
GATE_SOFT = ((16, 8, 0.05), (6, 42, 0.1), None, (5, 20, 1e19), (3, 45, 3e37), (4, 0, 0.2), (16, 8, 0.0), None)
GATE_PROBES = (4, 2, 0, 2, 2, 0, 4, 0)
GATE_TABLES = (16, 6, 0, 12, 3, 0, 16, 0)
SUB_LISTS = (1, 2, 5)

STREAM_MOVED_RADIUS = 0.08                                # of d; 0.1 leaves the plain plane without a pixel at 0 on two streams
STREAM_PROBES = (2, 0, 2)
STREAM_TABLES = (8, 6, 0)

TALL_RADIUS = 0.9
TALL_PROBES = (2, 0, 2)
TALL_TABLES = (6, 0, 0)

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the hash of include/rts.h, in numpy ------------------------------------------------------------------------------------------
def hash32(v):
    """v ^= v >> 16; v *= 0x7feb352d; v ^= v >> 15; v *= 0x846ca68b; v ^= v >> 16, in uint32 arithmetic."""
    v = np.array(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(16)
    v = (v * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(16)
    return v.astype(np.uint32)


def start(p, T):
    """(hash32(p) * T) >> 32: the entry of a table of T at which the pixel of index p in the full frame begins."""
    return ((hash32(p).astype(np.uint64) * np.uint64(T)) >> np.uint64(32)).astype(np.uint32)


# ---- modes and definitions --------------------------------------------------------------------------------------------------------
def vectors(mode, probes, tables):
    """(probes, tables) of a mode, as the definition takes them."""
    zeros = (0,) * len(probes)
    return {"plain": (zeros, zeros), "adaptive": (tuple(probes), zeros), "jittered": (tuple(probes), tuple(tables))}[mode]


def want(packed, k, lights, probes, tables, pos, mode):
    """(uint8[count, H, W] counts, uint8[H, W] refined) of a mode without a map, from the oracle alone."""
    pr, tb = vectors(mode, probes, tables)
    counts, refined, _ = sjc.definition(packed, k, lights, pr, tb, pos)
    return _frozen(counts, refined)


def classes(plane, n):
    """(at 0, at n, strictly between)"""
    at0, atn = int((plane == 0).sum()), int((plane == n).sum())
    return at0, atn, plane.size - at0 - atn


def guard_planes(counts, refined, lights, probes, what, least=LEAST):
    """`counts`, `refined`: a definition WITHOUT a map, `probes` those of its mode."""
    assert counts.shape[0] == lights.count and (refined >> lights.count == 0).all(), what
    for l in range(lights.count):
        e, n = lights.lights[l], samples(lights, l)
        got = classes(counts[l], n)
        took = int(((refined >> l) & 1).sum())
        if n > 1 and e.radius > 0:
            assert min(got) >= least, (what, l, got)
            if probes[l] >= 2:
                assert took >= least, (what, l, "refined", took)
        else:
            assert min(got[:2]) >= least and got[2] == 0 and took == 0, (what, l, got, took)
        if probes[l] == 0:
            assert took == 0, (what, l, took)


def guard_map(counts, lights_map, what):
    """Among the pixels the map marks for each light there is a 0 and a non-zero byte."""
    for l in range(counts.shape[0]):
        on = counts[l][((lights_map >> l) & 1) != 0]
        assert on.size and (on == 0).any() and (on != 0).any(), (what, l, int(on.size))


def guard_jitter(jittered, adaptive, probes, tables, what):
    """One tabled light with a probe differs somewhere from the adaptive mode's plane."""
    assert any(probes[l] and tables[l] and not np.array_equal(jittered[l], adaptive[l]) for l in range(len(probes))), what


# ---- the gate soft list -----------------------------------------------------------------------------------------------------------
def gate_soft_list(count=8):
    """The first `count` entries of the gate soft list."""
    hard = ec.gate_list(8)
    entries = []
    for l in range(count):
        e = (hard.lights[l].type, list(hard.lights[l].xyz))
        entries.append(e if GATE_SOFT[l] is None else e + GATE_SOFT[l])
    lights = api.SoftLightList.make(entries, TABLE)
    if count == 8:                                       # the negative zero travels
        assert np.float32(lights.lights[7].xyz[0]).view(np.uint32) == 0x80000000
    return lights


def gate_want(mode, count=8):
    g = gate()
    return _once(("gate", mode, count), lambda: want(g.packed, g.k, gate_soft_list(count), GATE_PROBES[:count], GATE_TABLES[:count],
                                                     g.pos, mode))


def gate_maps(count=8):
    """{"edges", "complement", "lone"} of the first `count` lights."""
    g = gate()
    return dict(list_maps(g.maps, count), lone=lone_map(g.H, g.W))


def guard_gate(count=8):
    """Every guard of the gate list of `count` entries, in the three modes and under its two edge maps."""
    lights, maps = gate_soft_list(count), gate_maps(count)
    for mode in MODES:
        counts, refined = gate_want(mode, count)
        guard_planes(counts, refined, lights, vectors(mode, GATE_PROBES[:count], GATE_TABLES[:count])[0], ("gate", count, mode))
        for name in ("edges", "complement"):
            guard_map(counts, maps[name], ("gate", count, mode, name))
    guard_jitter(gate_want("jittered", count)[0], gate_want("adaptive", count)[0], GATE_PROBES[:count], GATE_TABLES[:count], ("gate", count))


# ---- the stream soft list ---------------------------------------------------------------------------------------------------------
def stream_soft_list(pos, k, point):
    """edge_cases.stream_list made soft (see the module's text)."""
    hard = ec.stream_list(pos, k, point)
    p = np.array(list(point.xyz), np.float64)
    c = np.asarray(pos, np.float64).reshape(-1, 4)[:, :3].mean(0)
    d = np.linalg.norm(p - c)
    soft = ((4, 8, 0.05 * d), (6, 42, 0.1), (5, 20, STREAM_MOVED_RADIUS * d))
    return api.SoftLightList.make([(hard.lights[l].type, list(hard.lights[l].xyz)) + soft[l] for l in range(3)], TABLE)


def stream_wants(packed, k, lights, pos, what, probes=STREAM_PROBES, tables=STREAM_TABLES):
    """{mode: (counts, refined)} on a stream, every guard asserted (least = 1)."""
    wants = {mode: want(packed, k, lights, probes, tables, pos, mode) for mode in MODES}
    for mode in MODES:
        guard_planes(wants[mode][0], wants[mode][1], lights, vectors(mode, probes, tables)[0], (what, mode), least=1)
    guard_jitter(wants["jittered"][0], wants["adaptive"][0], probes, tables, what)
    return wants


# ---- the tall frames of the 1-D grid ----------------------------------------------------------------------------------------------
def rotated(lights, l, s, T):
    """The derived light of entry l with the explicit offsets offsets[(s + j) mod T], j < n, and no table."""
    whole = lights.light(l, table=T)
    rows = np.array([[whole.offsets[(s + j) % T][i] for i in range(3)] for j in range(whole.nsamples)], np.float32)
    lt = api.Light.make(whole.type, list(whole.xyz), rows)
    assert lt.nsamples == whole.nsamples and lt.table == 0
    return lt


def tall_case():
    """wl, k, texels[256, 256, 4], lights, and per mode of ("plain", "jittered") the per-texel planes: `counts[l]` / `refined_bit[l]`
    are uint8[256, 256] for a light without a table and uint8[T, 256, 256] -- one plane per start -- for the tabled one."""
    def make():
        wl = workloads.prepare_config("cornell_256", cache=True)
        k = wl.constants
        texels = np.ascontiguousarray(wl.positions, np.float32).reshape(256, 256, 4)
        lights = api.SoftLightList.make([(wl.light.type, list(wl.light.xyz), 4, 8, RADIUS_FEW),
                                         (api.Light.DIRECTIONAL, list(k.lightDirection)[:3]),
                                         (api.Light.POINT, (2.0, 8.0, 6.0), 5, 20, TALL_RADIUS)], TABLE)
        out = {"wl": wl, "k": k, "texels": texels, "lights": lights}
        for mode in ("plain", "jittered"):
            probes, tables = vectors(mode, TALL_PROBES, TALL_TABLES)
            counts, refined, _ = sjc.definition(wl.packed, k, lights, probes, (0,) * 3, texels)        # every table 0: the texel alone
            guard_planes(counts, refined, lights, probes, ("tall", mode), least=1)
            per_counts, per_bit = [counts[l] for l in range(3)], [(refined >> l) & 1 for l in range(3)]
            for l in range(3):
                T = tables[l]
                if T:
                    planes = [adaptive_cases.definition(wl.packed, k, rotated(lights, l, s, T), texels, max(1, probes[l])) for s in range(T)]
                    assert probes[l] != 0
                    assert np.array_equal(planes[0][0], counts[l]) and np.array_equal(planes[0][1], per_bit[l])   # start 0: the untabled light
                    per_counts[l], per_bit[l] = np.stack([m for m, _, _ in planes]), np.stack([r for _, r, _ in planes])
            out[mode] = {"counts": _frozen(*per_counts), "refined_bit": _frozen(*per_bit), "probes": probes, "tables": tables}
        return out
    return _once("tall", make)


def tall_want(t, mode, H, W=3, wrong_base=0):
    """(counts[3, H, W], refined[H, W]) of the tall frame: texel (i mod 65536) at pixel i; a tabled light's byte gathered from the plane
    of start(i, T).  wrong_base != 0: what a kernel that hashed i - wrong_base -- the index inside a row range -- would write."""
    case = t[mode]
    index = np.arange(H * W, dtype=np.uint64)
    texel = (index % np.uint64(65536)).astype(np.int64)
    counts, refined = np.zeros((3, H, W), np.uint8), np.zeros((H, W), np.uint8)
    for l in range(3):
        T = case["tables"][l]
        if T:
            s = start((index - np.uint64(wrong_base)) & np.uint64(0xFFFFFFFF), T).astype(np.int64)
            c, r = case["counts"][l].reshape(T, -1)[s, texel], case["refined_bit"][l].reshape(T, -1)[s, texel]
        else:
            c, r = case["counts"][l].ravel()[texel], case["refined_bit"][l].ravel()[texel]
        counts[l] = c.reshape(H, W)
        refined |= (r.reshape(H, W) << l).astype(np.uint8)
    return counts, refined


def tall_untabled(t, mode, H, W=3):
    """tall_want with every table ignored: what a kernel that never looked at the table would write."""
    case = t[mode]
    return np.stack([tall(case["counts"][l][0] if case["tables"][l] else case["counts"][l], H, W) for l in range(3)])


# ---- a penumbra that only edge texels own -----------------------------------------------------------------------------------------
def penumbra_map():
    """Every light's bit on the edge texels of the first two tile rows of the gate frame and nowhere else: in the first tile row the
    one edge texel of each tile, in the second, which holds whole tiles of edge values, every texel with an edge coordinate.  So a
    pixel that refines under this map is an edge texel, and so is the stand-in of every tile."""
    g = gate()
    edge = (g.ids >= 0).any(-1)
    m = np.where(edge & (np.arange(g.H)[:, None] < 16), 0xFF, 0).astype(np.uint8)
    assert all(np.count_nonzero(m[0:8, 8 * i:8 * i + 8]) >= 1 for i in range(g.W // 8)) and m[3, 5] == 0xFF
    return m


def penumbra_tiles(refined, lights_map):
    """From a definition's `refined` WITHOUT a map: (tiles whose refined pixels under the map are all edge texels, and exist; of those,
    tiles with a single marked lane; tiles with marked pixels and no refined one)."""
    g = gate()
    edge = (g.ids >= 0).any(-1)
    took = (refined & lights_map) != 0
    owned = lone = idle = 0
    for ty in range(g.H // 8):
        for tx in range(g.W // 8):
            sl = (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))
            marked = lights_map[sl] != 0
            if not marked.any():
                continue
            if took[sl].any():
                if edge[sl][took[sl]].all():
                    owned += 1
                    lone += int(marked.sum() == 1)
            else:
                idle += 1
    return owned, lone, idle
