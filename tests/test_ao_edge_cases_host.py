"""CPU: what tests/test_gpu_ao_edges.py expects, pinned before any device sees it (inputs: tests/ao_edge_cases.py).  The expectation
is the oracle's any-hit sum over the rays of the numpy rule; here the host twin (api.ambient_occlusion) is held against that sum on
every case but the tall frames, and the rule's ray against the oracle's own ray (oracle.gen_rays for the hard point light at
aim_rule's L) bit for bit on a subsample of every edge-value class and every wild normal.  When a GPU case fails, this tells a wrong
twin or a wrong rule from a wrong kernel; it also pins the inputs themselves -- ladder picks and class counts -- so that a change to a
shared helper that empties a case shows here first."""
import numpy as np
import pytest

import ao_cases as ac
import ao_edge_cases as aec
import edge_cases as ec
import oracle
from raytracedshadows_amd import api

GUARD = aec.GUARD
#: the gate frame without a map, per set at its ordinary radius: (at 0, at n, between) over the 5244 ordinary pixels
GATE_ORDINARY = {(4, 0): (39, 2894, 2311), (5, 8): (40, 2719, 2485), (16, 16): (46, 85, 5113), (48, 64): (15, 28, 5201),
                 "axis": (52, 3175, 2017)}
#: ... and of set (5, 8) over the 5979 live pixels at the other radii
GATE_OTHER = {"zero": (0, 5979, 0), "negative": (91, 3251, 2637), "denormal": (1, 5978, 0), "huge": (5214, 337, 428)}
#: stream -> (at 0, at n, between) over the live pixels, sets (4, 0) and (5, 8), at the recorded share
STREAM_CLASSES = {"non_finite": [(0, 4096, 0), (0, 4096, 0)], "unordered": [(0, 23347, 2253), (0, 23691, 1909)],
                  "orphans": [(0, 3233, 863), (0, 2828, 1268)], "degenerate": [(0, 4096, 0), (0, 4096, 0)],
                  "one_triangle": [(0, 3342, 754), (0, 3139, 957)], "two_triangles": [(0, 3342, 754), (0, 3139, 957)],
                  "median_split": [(0, 4096, 0), (0, 4096, 0)], "deep_bushy": [(0, 1863, 2233), (0, 1370, 2726)],
                  "lbvh": [(0, 4096, 0), (0, 4096, 0)], "ploc": [(0, 4096, 0), (0, 4096, 0)]}


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:4].tolist())


def _bits(a):
    """Bit patterns with every NaN as one value: a NaN equals a NaN."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def _twin(packed, k, ao, pos, nrm, **kw):
    return api.ambient_occlusion(packed, k, ao, pos, nrm, pos.shape[1], pos.shape[0], **kw)


# ---- the gate frame ---------------------------------------------------------------------------------------------------------------
def test_gate_inputs_are_pinned_and_guarded():
    g = aec.gate()
    assert int(aec.gate_ordinary().sum()) == 5244 and int(aec.live(aec.gate_normals()).sum()) == 5979
    aec.guard_gate_all()
    for key in aec.GATE_SETS:
        n = aec.gate_ao(key, 1.0).samples
        assert aec.classes(aec.gate_want(key, "ordinary"), n, aec.gate_ordinary()) == GATE_ORDINARY[key], key
        # the recorded share is the first entry of the ladder that meets the guard -- or, where none does, the one whose smallest class is largest
        meets = lambda s: min(aec.classes(aec.gate_want(key, "ordinary", share=s), n, aec.gate_ordinary())) >= aec.LEAST
        first = aec.first_of(aec.GATE_LADDER, meets)
        if first is None:
            assert key in aec.GATE_UNMET
            first = max(aec.GATE_LADDER, key=lambda s: min(aec.classes(aec.gate_want(key, "ordinary", share=s), n, aec.gate_ordinary())))
        else:
            assert key not in aec.GATE_UNMET
        assert first == aec.GATE_SHARES[key], (key, first)
    for rname, got in GATE_OTHER.items():
        assert aec.classes(aec.gate_want((5, 8), rname), 5, aec.live(aec.gate_normals())) == got, rname
    # the stand-in's cases: under map c every first walker is an edge texel; under lane63 the first live lane of a tile is lane 63
    # (on edge tiles too); under the lone map one tile has a walker, and it is a lone pixel
    # AFTER the background rule has taken its pixels.  Of the 27 tiles that hold an edge texel, per map (tiles whose first live lane
    # is an edge texel, tiles whose first live lane is ordinary with a live edge texel after it, tiles whose live lanes are all edge
    # texels, tiles with one live lane); the texel the light `on_texel` sits on counts as an edge texel
    maps = aec.gate_maps()
    assert {name: aec.walker_tiles(m) for name, m in maps.items()} == {"a": (27, 0, 0, 0), "b": (0, 27, 0, 0), "c": (27, 0, 27, 15),
                                                                       "lone": (1, 0, 1, 1), "lane63": (6, 0, 6, 46)}
    assert aec.walker_tiles(None) == (12, 15, 0, 0)
    walkers = aec.first_walkers(maps["lane63"])
    assert len(walkers) == 46 and all(lane == 63 for _, lane, _ in walkers)
    assert [(lane, at) for _, lane, at in aec.first_walkers(maps["lone"])] == [(8 * (aec.ON_TEXEL[0] % 8) + aec.ON_TEXEL[1] % 8, aec.ON_TEXEL)]
    on = aec.live(aec.gate_normals())
    assert all(on[at] and aec.gate_wild()[at] for at in aec.WILD) and int(aec.gate_wild().sum()) == len(aec.WILD)


@pytest.mark.parametrize("key", aec.GATE_SETS, ids=str)
def test_gate_twin_equals_the_oracles_sum(key):
    g = aec.gate()
    nrm = aec.gate_normals()
    for rname in aec.GATE_RADII:
        ao, plane = aec.gate_ao(key, aec.gate_radius(key, rname)), aec.gate_want(key, rname)
        _same(_twin(g.packed, g.k, ao, g.pos, nrm), plane, (key, rname))
        for name, m in aec.gate_maps().items():
            _same(_twin(g.packed, g.k, ao, g.pos, nrm, active=m), aec.under(plane, m), (key, rname, name))


def test_gate_host_rows_hash_the_full_frame_index():
    g = aec.gate()
    nrm, (r0, r1) = aec.gate_normals(), aec.HOST_ROWS
    plane = aec.gate_want((5, 8), "ordinary")
    ao = aec.gate_ao((5, 8), aec.gate_radius((5, 8), "ordinary"))
    out = np.full((g.H, g.W), GUARD, np.uint8)
    _twin(g.packed, g.k, ao, g.pos, nrm, row_begin=r0, row_end=r1, out=out)
    rows = (np.arange(g.H) >= r0) & (np.arange(g.H) < r1)
    _same(out, np.where(rows[:, None], plane, GUARD), "rows")
    assert int((aec.gate_rows_wrong() != plane[r0:r1]).sum()) >= aec.LEAST       # a start hashed inside the rows shows


@pytest.mark.parametrize("key", aec.GATE_SETS, ids=str)
def test_rule_ray_is_the_oracles_ray_for_the_point_light_at_L(key):
    """Per radius a subsample with a pixel of every edge-value class of Gate.ids (in every coordinate it occurs in), every wild
    normal, the pixels of the non-unit tile's first row and a few ordinary ones: rays_rule's ray of (pixel, j) is oracle.gen_rays
    for make_light(POINT, aim_rule(...)) at that texel, bit for bit (a NaN equals a NaN)."""
    g = aec.gate()
    nrm = aec.gate_normals()
    on = aec.live(nrm)
    picks, seen = [], set()
    for v in sorted(set(g.ids[on].ravel().tolist()) - {-1}):
        for c in range(3):
            ys, xs = np.nonzero(on & (g.ids[..., c] == v))
            if ys.size:
                picks.append((int(ys[0]), int(xs[0])))
                seen.add(v)
    assert seen == set(range(len(ec.EDGE) + 1)), sorted(seen)
    picks += list(aec.WILD) + [(32, x) for x in range(16, 24) if on[32, x]]
    ys, xs = np.nonzero(aec.gate_ordinary())
    picks += [(int(ys[i]), int(xs[i])) for i in range(0, ys.size, ys.size // 8)]
    for rname in aec.GATE_RADII:
        ao = aec.gate_ao(key, aec.gate_radius(key, rname))
        n = ao.samples
        rays = ac.rays_rule(g.k, ao, g.pos, nrm).reshape(g.H, g.W, n, 8)
        for y, x in picks:
            for j in sorted({0, 1, n - 1}):
                with np.errstate(all="ignore"):
                    L = ac.aim_rule(g.k, ao, g.pos, nrm, y, x, j)
                ray = oracle.gen_rays(g.k.as_array(), oracle.make_light(1, L), g.pos[y:y + 1, x:x + 1]).reshape(-1, 8)[0]
                assert np.array_equal(_bits(ray[:7]), _bits(rays[y, x, j][:7])), (key, rname, y, x, j, ray[:7].tolist(), rays[y, x, j][:7].tolist())


# ---- the streams ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", aec.STREAMS)
def test_stream_twins_equal_the_oracle_and_the_share_is_the_ladders_first(name):
    """On `lbvh` and `ploc` the same triangles in the host builder's tree: the frame the GPU test traces in the device's tree."""
    packed, pos, k, point, _ = aec.stream_case(name)
    nrm, wants = aec.stream_wants(packed, k, pos, point, name)
    assert [aec.classes(wants[key][1], key[0], aec.live(nrm)) for key in aec.STREAM_SETS] == STREAM_CLASSES[name], name
    for key, (ao, plane) in wants.items():
        _same(_twin(packed, k, ao, pos, nrm), plane, (name, key))

    def meets(share):
        d = aec.light_distance(pos, k, point)
        planes = [aec.want(packed, k, api.AoParams.make(n, share * d, table=t, seed=aec.SEED), pos, nrm) for n, t in aec.STREAM_SETS]
        return all((p[aec.live(nrm)] < n).any() and (p[aec.live(nrm)] > 0).any() for p, (n, _) in zip(planes, aec.STREAM_SETS))

    first = aec.first_of(aec.STREAM_LADDER, meets)
    assert (first is None) == (name in aec.STREAM_UNMET), (name, first)
    assert aec.STREAM_SHARE[name] == (first if first is not None else aec.STREAM_LADDER[-1])


# ---- the refit --------------------------------------------------------------------------------------------------------------------
def test_refit_frame_meets_its_guard_and_the_twin_the_oracle():
    c = aec.refit_case()
    plane = aec.refit_want(c["wl"].packed, "before")
    assert aec.classes(plane, 4, aec.live(c["nrm"])) == (0, 20299, 1694)
    _same(_twin(c["wl"].packed, c["k"], c["ao"], c["pos"], c["nrm"]), plane, "refit, before")
    assert np.isfinite(c["moved"]).all() and (c["moved"][:, :3] != c["wl"].vertices[:, :3]).any()
    assert np.array_equal(c["moved"][:, 3:], c["wl"].vertices[:, 3:])


# ---- the tall and the wide frames -------------------------------------------------------------------------------------------------
def test_tall_planes_are_pinned_and_the_table_shows():
    t = aec.tall_case()
    on = aec.live(t["nrm"])
    assert aec.classes(t["plane0"], 3, on) == (5, 53460, 3106)
    assert aec.classes(t["planes6"][0], 3, on) == (39, 54474, 2058)
    _same(_twin(t["wl"].packed, t["k"], t["ao0"], t["texels"], t["nrm"]), t["plane0"], "texels, table 0")
    for side in (8, 16):
        H = side * 65536 + 5
        tabled = aec.tall_want(t, aec.TALL_TABLE, H)
        assert int((tabled[3:H - 2] != aec.tall_untabled(t, H)[3:H - 2]).sum()) >= aec.LEAST, side
        assert int((tabled[3:H - 2] != aec.tall_want(t, aec.TALL_TABLE, H, wrong_base=9)[3:H - 2]).sum()) >= aec.LEAST, side


def test_tall_slice_gathered_with_the_numpy_hash_equals_the_twin():
    """A 3 x 2053 frame of the tall case's texels, rows (3, 2051): the twin hashes the pixel's index in the frame it is given, the
    expectation is gathered from the six per-start planes with the numpy hash."""
    t = aec.tall_case()
    H, W, rows = 2053, 3, (3, 2051)
    pos, nrm = aec.tall_positions(t["texels"], H), aec.tall_positions(t["nrm"], H)
    inside = (np.arange(H) >= rows[0]) & (np.arange(H) < rows[1])
    for table, ao in ((0, t["ao0"]), (aec.TALL_TABLE, t["ao6"])):
        out = np.full((H, W), GUARD, np.uint8)
        _twin(t["wl"].packed, t["k"], ao, pos, nrm, row_begin=rows[0], row_end=rows[1], out=out)
        _same(out, np.where(inside[:, None], aec.tall_want(t, table, H), GUARD), ("tall slice", table))
