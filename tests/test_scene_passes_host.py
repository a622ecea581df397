"""CPU: the host twins of the four scene passes (rtsh_primary_gbuffer, rtsh_combine, rtsh_facing_active, rtsh_facing_lights) on the
awkward inputs of tests/scene_pass_cases.py -- against the oracle, against float32 numpy restatements of the per-pixel rules, and,
for rts_closest_hit.h alone, in a host program of its own under the address and UB sanitizers.  Every comparison is bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import scene_pass_cases as sp
from raytracedshadows_amd import api

bits = sp.bits


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = (bits(got), bits(want)) if got.dtype == np.float32 else (got, want)
    bad = np.argwhere(g != w)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


@pytest.mark.parametrize("name", sp.gbuffer_names())
def test_gbuffer_equals_the_oracle_and_brute_force(name):
    _, packed, eye, target, fovy, W, H, _ = sp.gbuffer_case(name)
    want_pos, want_nrm, want_hits = sp.oracle_gbuffer(name)
    pos, nrm, hits = api.primary_gbuffer(packed, eye, target, fovy, W, H)
    _same(pos, want_pos, name + " positions")
    _same(nrm, want_nrm, name + " normals")
    assert hits == want_hits
    only_pos, only_hits = api.primary_positions(packed, eye, target, fovy, W, H)
    _same(only_pos, want_pos, name + " positions alone")
    assert only_hits == want_hits
    assert sp.prim_count(packed) <= 1000
    brute_pos, brute_nrm, brute_hits = oracle.primary_gbuffer(packed, eye, target, fovy, W, H, cull=False)
    _same(pos, brute_pos, name + " positions, brute force")
    _same(nrm, brute_nrm, name + " normals, brute force")
    assert hits == brute_hits


def test_tall_frame_equals_the_oracle_on_the_host():
    name, packed, eye, target, fovy, W, H, _ = sp.tall_case()
    want_pos, want_nrm, want_hits = oracle.primary_gbuffer(packed, eye, target, fovy, W, H)
    pos, nrm, hits = api.primary_gbuffer(packed, eye, target, fovy, W, H)
    _same(pos, want_pos, name)
    _same(nrm, want_nrm, name)
    assert 0 < hits == want_hits < W * H


@pytest.mark.parametrize("name", sp.gbuffer_names())
def test_each_gbuffer_case_reaches_its_edge(name):
    """On the oracle's output alone."""
    _, packed, eye, target, fovy, W, H, expect = sp.gbuffer_case(name)
    pos, nrm, hits = sp.oracle_gbuffer(name)
    assert hits == int((pos[..., 3] != 0).sum())
    if expect == "mixed":
        assert 0 < hits < W * H, hits
    elif expect == "hit":
        assert hits > 0
    elif expect == "tiny":
        tiny = (pos[..., 3] == 1) & (nrm[..., :3] == 0).all(axis=-1)
        assert tiny.any()
        assert np.isfinite(pos[tiny]).all()
    elif expect == "axis":
        assert hits == 1 and pos[0, 0, 0] == 0 and pos[0, 0, 1] == 0 and pos[0, 0, 2] < 0 and pos[0, 0, 3] == 1
    else:
        assert expect is None


def test_odd_frames_carry_exact_zeros_in_the_centre_column_and_row():
    pos, _, _ = sp.oracle_gbuffer("tri_odd_7x5")
    hit = pos[..., 3] == 1
    assert hit[2, 3] and (pos[hit[:, 3], 3, 0] == 0).all() and (pos[2, hit[2], 1] == 0).all()
    assert (pos[hit][:, 0] != 0).any() and (pos[hit][:, 1] != 0).any()


def test_tie_cases_are_ties_and_the_stream_order_shows_in_the_normal():
    """Both orders see the same positions (every texel both triangles cover is a tie in t), and where both cover a texel the normal is
    the first leaf's: (+0, +0, 1) from A, (-0, -0, 1) from B."""
    for kind in ("coincident", "coplanar"):
        pab, nab, hab = sp.oracle_gbuffer(f"tie_{kind}_ab")
        pba, nba, hba = sp.oracle_gbuffer(f"tie_{kind}_ba")
        assert hab == hba > 0
        _same(pab, pba, kind)
        differ = (bits(nab) != bits(nba)).any(axis=-1)
        assert differ.any(), kind
        assert (bits(nab[differ]) == bits(np.array([0.0, 0.0, 1.0, 0.0], np.float32))).all()
        assert (bits(nba[differ]) == bits(np.array([-0.0, -0.0, 1.0, 0.0], np.float32))).all()
        if kind == "coincident":
            assert differ.sum() == hab


# ------------------------------------------------------------------------------------------------------------ per-pixel passes
def _describe(shape, run, bad, nrm, pos, mask, got, want):
    H, W = shape
    lines = [f"{shape} {run}: {bad.shape[0]} texels differ"]
    for y, x in bad[:12].tolist():
        lines.append(f"  normal {nrm[y, x, :3].tolist()} position {pos[y, x, :3].tolist()} mask {int(mask[y, x])}: got {int(got[y, x, 0])}, want {int(want[y, x, 0])}")
    return "\n".join(lines)


@pytest.mark.parametrize("shape", sp.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_combine_equals_the_oracle_and_the_written_out_rule(shape):
    nrm, pos, mask = sp.texels(shape)
    lights = sp.lights()
    for run in sp.pass_runs():
        kind, name, with_pos = run
        k, light = sp.constants(kind), lights[name]
        p = pos if with_pos else None
        rule = sp.combine_rule(k, light, p, nrm, mask)
        want = sp.oracle_combine(k, light, p, nrm, mask)
        assert np.array_equal(want, rule), _describe(shape, run, np.argwhere((want != rule).any(axis=-1)), nrm, pos, mask, want, rule)
        got = api.combine(k, light, p, nrm, mask)
        bad = np.argwhere((got != want).any(axis=-1))
        assert bad.shape[0] == 0, _describe(shape, run, bad, nrm, pos, mask, got, want)


def test_combine_saturates_large_normals_and_takes_a_nan_as_zero():
    """The two findings by value: a normal (0, y, 0) under the sun (0, 1, 0) with mask 1 is 255 for every y >= 1, +Inf included, and a
    NaN N.L leaves the ambient term alone: 0.15 + 0.05 = 0.2 -> 51."""
    k = sp.constants("unit")
    ys = [1, 1e5, 1e7, 1e8, 1e30, 3e38, np.inf]
    nrm = np.zeros((1, len(ys) + 1, 4), np.float32)
    nrm[0, :len(ys), 1] = ys
    nrm[0, len(ys), :3] = (np.nan, 0, 0)
    mask = np.ones((1, len(ys) + 1), np.uint8)
    want = [255] * len(ys) + [51]
    assert sp.combine_rule(k, None, None, nrm, mask)[0, :, 0].tolist() == want
    assert sp.oracle_combine(k, None, None, nrm, mask)[0, :, 0].tolist() == want
    assert api.combine(k, None, None, nrm, mask)[0, :, 0].tolist() == want


def test_a_mask_above_the_sample_count_saturates():
    k = sp.constants("unit")
    nrm = np.zeros((1, 3, 4), np.float32)
    nrm[..., 1] = 1
    mask = np.array([[16, 64, 255]], np.uint8)
    for name in ("sun", "directional1", "directional16"):
        light = sp.lights()[name]
        if light is not None:
            light.xyz[0], light.xyz[1], light.xyz[2] = 0, 1, 0
        got = api.combine(k, light, None, nrm, mask)[0, :, 0].tolist()
        assert got == sp.oracle_combine(k, light, None, nrm, mask)[0, :, 0].tolist()
        assert got == ([255, 255, 255]), (name, got)


@pytest.mark.parametrize("shape", sp.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_facing_marks_equal_the_rule(shape):
    nrm, pos, mask = sp.texels(shape)
    lights = sp.lights()
    for kind, name, with_pos in sp.pass_runs():
        k, light = sp.constants(kind), lights[name]
        p = pos if with_pos else None
        got = api.facing_active(k, light, p, nrm)
        want = sp.facing_rule(k, light, p, nrm)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (shape, kind, name, np.argwhere(got != want)[:8].tolist())
        assert set(np.unique(got).tolist()) <= {0, 1}
        with np.errstate(all="ignore"):
            ndl = sp.ndl_rule(k, light, p, nrm)
        background = (nrm[..., :3] == 0).all(axis=-1)
        assert got[np.isnan(ndl) & ~background].all()                        # a NaN is traced
        assert not got[background].any()
    for name, (lst, has_point) in sp.light_lists().items():
        k = sp.constants("unit")
        for p in ((pos,) if has_point else (pos, None)):
            got = api.facing_lights(k, lst, p, nrm)
            assert np.array_equal(got, sp.facing_lights_rule(k, lst, p, nrm)), (shape, name)
            assert not (got >> lst.count).any()
            for l in range(lst.count):
                assert np.array_equal((got >> l) & 1, api.facing_active(k, lst.light(l), p, nrm)), (shape, name, l)


def test_the_tables_reach_their_edges():
    """On the rules alone: the 999-texel table holds every normal with every mask, a denormal N.L that is traced, both marks, lit
    bytes of 0, 255 and in between, and a point light met exactly at the pixel."""
    nrm, pos, mask = sp.texels((3, 333))
    k = sp.constants("unit")
    pairs = {(bits(n[:3]).tobytes(), int(m)) for n, m in zip(nrm.reshape(-1, 4), mask.reshape(-1))}
    assert len(pairs) == len(sp.NORMALS) * len(sp.MASKS)
    with np.errstate(all="ignore"):
        ndl = sp.ndl_rule(k, None, None, nrm)
    denormal = (ndl > 0) & (ndl < np.finfo(np.float32).tiny)
    assert denormal.any() and sp.facing_rule(k, None, None, nrm)[denormal].all()
    mark = sp.facing_rule(k, sp.lights()["point1"], pos, nrm)
    assert 0 < int(mark.sum()) < mark.size
    rgb = sp.combine_rule(k, None, None, nrm, mask)[..., 0]
    assert (rgb == 0).any() and (rgb == 255).any() and ((rgb > 0) & (rgb < 255)).any()
    at_light = (pos[..., :3] == sp.POSITIONS[6]).all(axis=-1)
    assert at_light.any()
    unit = at_light & np.isfinite(nrm).all(axis=-1)
    with np.errstate(all="ignore"):
        assert (sp.ndl_rule(k, sp.lights()["point1"], pos, nrm)[unit] == 0).all()


@pytest.mark.parametrize("shape", sp.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_culling_by_the_mark_changes_no_byte_of_the_image(shape):
    """The mark never culls a pixel the combine pass would light: the image over the full mask equals the image over the mask zeroed
    where the mark is 0 -- by the oracle's combine pass and by the product's, NaN, Inf and huge normals included (the mask over the
    sample count is finite, so 1.25 * 0 * mask is 0 wherever N.L <= 0)."""
    nrm, pos, mask = sp.texels(shape)
    lights = sp.lights()
    culled_any = False
    for kind, name, with_pos in sp.pass_runs():
        k, light = sp.constants(kind), lights[name]
        p = pos if with_pos else None
        mark = api.facing_active(k, light, p, nrm)
        culled = (mask * (mark != 0)).astype(np.uint8)
        culled_any |= bool((culled != mask).any())
        a, b = sp.oracle_combine(k, light, p, nrm, mask), sp.oracle_combine(k, light, p, nrm, culled)
        assert np.array_equal(a, b), (shape, kind, name, np.argwhere((a != b).any(axis=-1))[:8].tolist())
        a, b = api.combine(k, light, p, nrm, mask), api.combine(k, light, p, nrm, culled)
        assert np.array_equal(a, b), (shape, kind, name, np.argwhere((a != b).any(axis=-1))[:8].tolist())
    assert culled_any or shape == (1, 1)


def test_refusals_of_the_host_passes_write_nothing():
    lib, k = api._lib, sp.constants("unit")
    nrm, pos, mask = (np.array(a) for a in sp.texels((16, 16)))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rgb = np.full((16, 16, 3), 0xAB, np.uint8)
    out = np.full((16, 16), 0xAB, np.uint8)
    point = sp.lights()["point1"]
    lst3, lst2 = sp.light_lists()["3"][0], sp.light_lists()["2_directional"][0]
    INVALID = 1
    assert lib.rtsh_combine(None, None, p(pos), p(nrm), p(mask), 16, 16, p(rgb)) == INVALID
    assert lib.rtsh_combine(C.byref(k), None, p(pos), None, p(mask), 16, 16, p(rgb)) == INVALID
    assert lib.rtsh_combine(C.byref(k), None, p(pos), p(nrm), None, 16, 16, p(rgb)) == INVALID
    assert lib.rtsh_combine(C.byref(k), None, p(pos), p(nrm), p(mask), 0, 16, p(rgb)) == INVALID
    assert lib.rtsh_combine(C.byref(k), None, p(pos), p(nrm), p(mask), 16, 0, p(rgb)) == INVALID
    assert lib.rtsh_combine(C.byref(k), C.byref(point), None, p(nrm), p(mask), 16, 16, p(rgb)) == INVALID
    assert lib.rtsh_facing_lights(C.byref(k), None, p(pos), p(nrm), 16, 16, p(out)) == INVALID
    assert lib.rtsh_facing_lights(None, C.byref(lst2), p(pos), p(nrm), 16, 16, p(out)) == INVALID
    assert lib.rtsh_facing_lights(C.byref(k), C.byref(lst3), None, p(nrm), 16, 16, p(out)) == INVALID          # a point light in the list
    assert lib.rtsh_facing_lights(C.byref(k), C.byref(lst2), p(pos), p(nrm), 0, 16, p(out)) == INVALID
    assert (rgb == 0xAB).all() and (out == 0xAB).all()


def test_closest_hit_header_under_address_and_ub_sanitizers(tmp_path):
    """rts_closest_hit.h alone in a host program of its own (tests/cpp/closest_hit_host.cpp, -fsanitize=address,undefined,
    float-cast-overflow): combinePixel, facingPixel, facingLightsPixel, leafTest, boxTest and writeTexel over NaN, +-Inf, denormal,
    huge and zero operands, every light kind and mask byte.  float-cast-overflow is named because `undefined` does not include it: it
    is the check that catches a float converted to int out of range."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "closest_hit_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(root, "tests", "cpp", "closest_hit_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100000, run.stdout[-2000:]
