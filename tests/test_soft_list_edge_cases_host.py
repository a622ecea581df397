"""CPU: the host twins (api.soft_light_list, api.soft_light_list_adaptive with and without `tables=`) against the oracle's definition
on the inputs of tests/soft_list_edge_cases.py, byte for byte -- the gate soft list and its sub-lists under the per-light edge maps,
the lone pixel and the map that leaves the penumbra to edge texels, the stream soft list on every host-built awkward stream, and a
slice of the tall frame, where the expectation is gathered with the numpy hash.  When a case of
tests/test_gpu_soft_list_edge_traces.py fails, this tells a wrong twin from a wrong kernel; it also pins the inputs themselves (class
sizes, refined pixels), so that a change to a shared helper that empties a case shows here first."""
import numpy as np
import pytest

import soft_list_edge_cases as sc
import soft_list_jitter_cases as sjc
from raytracedshadows_amd import api

GUARD = 0xAB
#: the gate list without a map, per light (at 0, at n, between) of 6144 pixels, and the refined pixels: adaptive, then jittered
GATE_ADAPTIVE = [(1755, 858, 3531), (2546, 2456, 1142), (3624, 2520, 0), (3961, 1351, 832), (5480, 374, 290), (1365, 1876, 2903),
                 (4168, 1976, 0), (3192, 2952, 0)]
GATE_ADAPTIVE_REFINED = [3531, 1142, 0, 832, 290, 0, 0, 0]
GATE_JITTERED_REFINED = [3481, 1401, 0, 955, 298, 0, 0, 0]
#: stream -> the jittered mode's refined pixels per light of the stream soft list
STREAM_REFINED = {"non_finite": [1469, 0, 694], "unordered": [8276, 0, 545], "orphans": [128, 0, 61], "degenerate": [1494, 0, 985],
                  "one_triangle": [120, 0, 78], "two_triangles": [818, 0, 269], "median_split": [1456, 0, 681],
                  "deep_bushy": [129, 0, 68], "lbvh": [1210, 0, 763], "ploc": [1210, 0, 763]}
#: the plain plane of the moved point light, (at 0, at n, between), on the two streams that decided its radius
STREAM_PLAIN_MOVED = {"non_finite": (30, 1614, 2452), "median_split": (7, 1660, 2429)}


def _twin(packed, k, lights, probes, tables, pos, mode, **kw):
    """(counts, refined) of the host twin in a mode; the plain twin has no refined plane: zeros stand for it."""
    H, W = pos.shape[:2]
    if mode == "plain":
        c = api.soft_light_list(packed, k, lights, pos, W, H, **kw)
        return c, np.zeros((H, W), np.uint8)
    return api.soft_light_list_adaptive(packed, k, lights, probes, pos, W, H, tables=tables if mode == "jittered" else None, **kw)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("counts", "refined")):
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())


def _refined_counts(refined, count):
    return [int(((refined >> l) & 1).sum()) for l in range(count)]


def test_numpy_hash_known_answers():
    """The six values tests/test_oracle_golden.py pins, and start() against Python's integers."""
    values = [0, 1, 2, 12345, 0xFFFFFFFF, 3840 * 2160 - 1]
    want = [0, 1753845952, 3507691905, 2435775735, 1734902346, 3873009951]
    assert sc.hash32(values).tolist() == want
    assert int(sc.hash32(12345)) == want[3]
    for T in (3, 6, 16, 48):
        assert sc.start(values, T).tolist() == [(h * T) >> 32 for h in want]
        s = sc.start(np.arange(100000), T)
        assert s.min() == 0 and s.max() == T - 1


def test_gate_inputs_are_pinned_and_guarded():
    lights = sc.gate_soft_list()
    sc.guard_gate(8)
    c, r = sc.gate_want("adaptive")
    assert [sc.classes(c[l], sc.samples(lights, l)) for l in range(8)] == GATE_ADAPTIVE
    assert _refined_counts(r, 8) == GATE_ADAPTIVE_REFINED
    assert _refined_counts(sc.gate_want("jittered")[1], 8) == GATE_JITTERED_REFINED
    plain = sc.gate_want("plain")
    assert not plain[1].any() and sc.classes(plain[0][5], 4) == GATE_ADAPTIVE[5]
    for n in sc.SUB_LISTS:                               # a plane is a function of its light alone
        sc.guard_gate(n)
        for mode in sc.MODES:
            sub, whole = sc.gate_want(mode, n), sc.gate_want(mode)
            assert np.array_equal(sub[0], whole[0][:n]) and np.array_equal(sub[1], whole[1] & ((1 << n) - 1)), (n, mode)


@pytest.mark.parametrize("mode", sc.MODES)
@pytest.mark.parametrize("count", (8,) + sc.SUB_LISTS)
def test_gate_list_twins_equal_the_oracle_with_and_without_the_edge_maps(count, mode):
    g = sc.gate()
    lights, probes, tables = sc.gate_soft_list(count), sc.GATE_PROBES[:count], sc.GATE_TABLES[:count]
    want = sc.gate_want(mode, count)
    _same(_twin(g.packed, g.k, lights, probes, tables, g.pos, mode), want, (count, mode))
    pr, tb = sc.vectors(mode, probes, tables)
    for name, m in sc.gate_maps(count).items():
        marked = sc.under(want[0], want[1], m)
        c, r, _ = sjc.definition(g.packed, g.k, lights, pr, tb, g.pos, m)       # the definition under the map is `under`
        _same((c, r), marked, (count, mode, name, "definition"))
        _same(_twin(g.packed, g.k, lights, probes, tables, g.pos, mode, lights_map=m), marked, (count, mode, name))
        if name == "lone":
            assert np.count_nonzero(marked[0][0]) <= 1 and not marked[0][1:].any()


@pytest.mark.parametrize("mode", ("adaptive", "jittered"))
def test_twins_under_the_map_that_leaves_the_penumbra_to_edge_texels(mode):
    g = sc.gate()
    m = sc.penumbra_map()
    assert (np.count_nonzero(m), np.count_nonzero(m[:8])) == (682, 12)
    want = sc.gate_want(mode)
    assert sc.penumbra_tiles(want[1], m) == (18, 6, 6)
    _same(_twin(g.packed, g.k, sc.gate_soft_list(), sc.GATE_PROBES, sc.GATE_TABLES, g.pos, mode, lights_map=m), sc.under(want[0], want[1], m), mode)


@pytest.mark.parametrize("name", sc.HOST_STREAMS)
def test_stream_soft_list_twins_equal_the_oracle(name):
    packed, pos, k, point, _ = sc.stream_case(name)
    lights = sc.stream_soft_list(pos, k, point)
    wants = sc.stream_wants(packed, k, lights, pos, name)
    assert _refined_counts(wants["jittered"][1], 3) == STREAM_REFINED[name], name
    if name in STREAM_PLAIN_MOVED:
        assert sc.classes(wants["plain"][0][2], 5) == STREAM_PLAIN_MOVED[name], name
    for mode in sc.MODES:
        _same(_twin(packed, k, lights, sc.STREAM_PROBES, sc.STREAM_TABLES, pos, mode), wants[mode], (name, mode))


@pytest.mark.parametrize("name", ["lbvh", "ploc"])
def test_the_device_built_streams_frame_is_usable(name):
    """The same triangles in the host builder's tree: the frame the GPU test traces in the device's tree meets the guard."""
    packed, pos, k, point, _ = sc.stream_case(name)
    wants = sc.stream_wants(packed, k, sc.stream_soft_list(pos, k, point), pos, name)
    assert _refined_counts(wants["jittered"][1], 3) == STREAM_REFINED[name], name


def test_smallest_stream_class_is_the_directional_lights_zero_on_degenerate():
    packed, pos, k, point, _ = sc.stream_case("degenerate")
    lights = sc.stream_soft_list(pos, k, point)
    c, _ = sc.want(packed, k, lights, sc.STREAM_PROBES, sc.STREAM_TABLES, pos, "adaptive")
    assert sc.classes(c[1], 6)[0] == 5


def test_tall_slice_gathered_with_the_numpy_hash_equals_the_twin():
    """A 3 x 2053 frame of the tall case's texels, rows (3, 2051): the twin hashes the pixel's index in the frame it is given, the
    expectation is gathered from per-start planes with the numpy hash -- two routes that share nothing but the oracle's rays."""
    t = sc.tall_case()
    H, W, rows = 2053, 3, (3, 2051)
    pos = sc.tall_positions(t["texels"], H)
    inside = (np.arange(H) >= rows[0]) & (np.arange(H) < rows[1])
    for mode in ("plain", "jittered"):
        c, r = sc.tall_want(t, mode, H)
        out, ref = np.full((3, H, W), GUARD, np.uint8), np.full((H, W), GUARD, np.uint8)
        kw = dict(lights_map=None, row_begin=rows[0], row_end=rows[1], out=out)
        if mode == "plain":
            api.soft_light_list(t["wl"].packed, t["k"], t["lights"], pos, W, H, **kw)
            r = ref
        else:
            api.soft_light_list_adaptive(t["wl"].packed, t["k"], t["lights"], sc.TALL_PROBES, pos, W, H, tables=sc.TALL_TABLES, refined=ref, **kw)
        _same((out, ref), (np.where(inside[None, :, None], c, GUARD), np.where(inside[:, None], r, GUARD)), ("tall slice", mode))


def test_the_tabled_light_shows_on_the_tall_frames():
    """On both tall heights the tabled light's gathered plane differs from its untabled plane, inside the row range too -- else a kernel
    that ignored the table could pass; and from the plane gathered with the index inside the row range."""
    t = sc.tall_case()
    for side in (8, 16):
        H = side * 65536 + 5
        c, _ = sc.tall_want(t, "jittered", H)
        plain = sc.tall_untabled(t, "jittered", H)
        assert int((c[0][3:H - 2] != plain[0][3:H - 2]).sum()) >= sc.LEAST, side
        assert np.array_equal(c[1:], plain[1:])
        wrong, _ = sc.tall_want(t, "jittered", H, wrong_base=9)            # the hash of the index inside the row range (3, H - 2)
        assert int((c[0][3:H - 2] != wrong[0][3:H - 2]).sum()) >= sc.LEAST, side
