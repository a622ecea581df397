"""CPU: the host twin of the jittered soft light list trace (rtsh_soft_light_list_jittered, include/rts_scene.h;
api.soft_light_list_adaptive(tables=...)) against the definition taken from the untouched oracle (tests/soft_list_jitter_cases.py),
byte for byte in the count planes and in the refined plane, with and without the facing map and over a row range; tables None and all
zeros against the adaptive list's twin; the refusals; the derived light; and the argument rule as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

from raytracedshadows_amd import api
from soft_list_jitter_cases import CASES, FRAMES, case_id, definition, jitter_list_frame, light_map, make_list, samples, under
from test_soft_light_list_host import bad_lists
from test_soft_list_adaptive_host import bad_probes

GUARD = 0xAB
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("name,probes,tables", CASES, ids=case_id)
def test_twin_equals_the_oracle(name, probes, tables, W, H):
    fr = jitter_list_frame(W, H)
    lights = make_list(name)
    want_c, want_r, _ = fr.oracle_planes(name, probes, tables)   # (asserts that the case does not degenerate)
    got_c, got_r = fr.want(name, probes, tables)
    assert got_c.shape == (lights.count, H, W) and got_r.shape == (H, W)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_r, want_r), (name, probes, tables)
    # with the facing map and with a map of every bit pattern: the oracle's bytes under the map's bits
    for m in (fr.facing(name), light_map(fr, lights.count)):
        map_c, map_r = under(want_c, want_r, m)
        got_c, got_r = api.soft_light_list_adaptive(fr.packed, fr.k, lights, probes, fr.pos, W, H, lights_map=m, tables=tables)
        assert np.array_equal(got_c, map_c) and np.array_equal(got_r, map_r), (name, probes, tables)
    # a row range leaves the other rows, and the planes from the count up, alone; the hash stays the full frame's
    rows = (np.arange(H) >= 8) & (np.arange(H) < 29)
    for lm, (c, r) in ((m, (map_c, map_r)), (None, (want_c, want_r))):
        out, ref = np.full((8, H, W), GUARD, np.uint8), np.full((H, W), GUARD, np.uint8)
        api.soft_light_list_adaptive(fr.packed, fr.k, lights, probes, fr.pos, W, H, lights_map=lm, row_begin=8, row_end=29, out=out,
                                     refined=ref, tables=tables)
        assert np.array_equal(out[:lights.count], np.where(rows[None, :, None], c, GUARD)), name
        assert (out[lights.count:] == GUARD).all() and np.array_equal(ref, np.where(rows[:, None], r, GUARD)), name


def test_under_a_map_the_oracle_itself_gives_the_same():
    fr = jitter_list_frame(61, 37)
    name, probes, tables = "mixed", (0, 2, 2, 0, 2), (0, 6, 12, 0, 3)
    m = light_map(fr, 5)
    map_c, map_r, _ = definition(fr.packed, fr.k, make_list(name), probes, tables, fr.pos, m)
    want_c, want_r, _ = fr.oracle_planes(name, probes, tables)
    uc, ur = under(want_c, want_r, m)
    assert np.array_equal(map_c, uc) and np.array_equal(map_r, ur)


@pytest.mark.parametrize("name,probes", [("mixed", (0, 2, 2, 0, 2)), ("overlap", (3, 4, 2)), ("48", (4,))], ids=case_id)
def test_no_table_is_the_adaptive_list(name, probes):
    for W, H in FRAMES:
        fr = jitter_list_frame(W, H)
        lights = make_list(name)
        c0, r0 = api.soft_light_list_adaptive(fr.packed, fr.k, lights, probes, fr.pos, W, H)
        for tables in ((0,) * lights.count,):
            c, r = api.soft_light_list_adaptive(fr.packed, fr.k, lights, probes, fr.pos, W, H, tables=tables)
            assert np.array_equal(c, c0) and np.array_equal(r, r0), (W, H, name)
        # tables == NULL through the new entry point itself
        c, r = np.zeros_like(c0), np.zeros_like(r0)
        assert api._lib.rtsh_soft_light_list_jittered(api._ptr(fr.packed), fr.packed.shape[0], api.C.byref(fr.k), api.C.byref(lights),
                                                      api._ptr(fr.pos), None, W, H, 0, H, api._ptr(c), api._probes(lights, probes), None,
                                                      api._ptr(r), 0) == 0
        assert np.array_equal(c, c0) and np.array_equal(r, r0), (W, H, name)


def test_planes_are_the_one_light_twins_of_the_derived_lights():
    fr = jitter_list_frame(61, 37)
    name, probes, tables = "mixed", (0, 2, 2, 0, 2), (0, 6, 12, 0, 3)
    lights = make_list(name)
    m = light_map(fr, lights.count)
    got_c, got_r = api.soft_light_list_adaptive(fr.packed, fr.k, lights, probes, fr.pos, fr.W, fr.H, lights_map=m, tables=tables)
    for l in range(lights.count):
        act = ((m >> l) & 1).astype(np.uint8)
        lt = lights.light(l, table=tables[l])
        if probes[l] == 0:
            _, mask = api.soft_distance(fr.packed, fr.k, lt, fr.pos, fr.W, fr.H, active=act)
            took = np.zeros_like(act)
        else:
            mask, took = api.shadow_mask_adaptive(fr.packed, fr.k, lt, fr.pos, fr.W, fr.H, probes[l], active=act)
        assert np.array_equal(got_c[l], mask) and np.array_equal((got_r >> l) & 1, took), l


def test_unmarked_pixels_may_hold_anything():
    fr = jitter_list_frame(64, 48)
    name, probes, tables = "mixed", (0, 2, 2, 0, 2), (0, 6, 12, 0, 3)
    lights = make_list(name)
    m = light_map(fr, 5)
    dead = (m & 31) == 0
    dirty = fr.pos.copy()
    dirty[dead] = np.array([np.nan, np.inf, 1e38, -np.inf], np.float32)
    got_c, got_r = api.soft_light_list_adaptive(fr.packed, fr.k, lights, probes, dirty, fr.W, fr.H, lights_map=m, tables=tables)
    want_c, want_r = under(*fr.want(name, probes, tables), m)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_r, want_r)
    assert (got_c[:, dead] == 0).all() and (got_r[dead] == 0).all() and dead.sum() > 100


def bad_tables(good):
    """(probes, tables) pairs the rule refuses although list and probes are accepted (good: the `mixed` list -- hard, 6 from 42,
    5 from 20, hard, 3 from 45)."""
    assert [(samples(good, l), good.lights[l].first) for l in (1, 2, 4)] == [(6, 42), (5, 20), (3, 45)]
    p = (0, 2, 2, 0, 2)
    return [(p, (1, 0, 0, 0, 0)), (p, (0, 0, 0, 2, 0)),                  # a table on a hard entry
            (p, (0, 5, 0, 0, 0)), (p, (0, 0, 4, 0, 0)), (p, (0, 0, 1, 0, 0)),   # below the samples
            (p, (0, 7, 0, 0, 0)), (p, (0, 0, 29, 0, 0)), (p, (0, 0, 0, 0, 4)), (p, (0, 0, 0xFFFFFFFF, 0, 0)),   # past slot 48
            (p, (0, 0, 0xFFFFFFFF - 19, 0, 0))]                          # first + table wraps in 32 bits


def test_refusals_without_a_device():
    fr = jitter_list_frame(64, 48)
    W, H, packed, k = fr.W, fr.H, fr.packed, fr.k
    lib, kp = api._lib, api.C.byref(k)
    out, ref = np.full((8, H, W), GUARD, np.uint8), np.full((H, W), GUARD, np.uint8)
    P, M, R = api._ptr(fr.pos), api._ptr(out), api._ptr(ref)
    pk, n = api._ptr(packed), packed.shape[0]
    good = make_list("mixed")
    gp, pr0, tb0 = api.C.byref(good), api._probes(good, (0, 2, 2, 0, 2)), api._probes(good, (0, 6, 12, 0, 3))
    assert lib.rtsh_soft_light_list_jittered(pk, n, kp, gp, P, None, W, H, 0, 0, M, pr0, tb0, R, 1) == 0
    # the edge that is still accepted: first + table == 48 and table == nsamples
    assert lib.rtsh_soft_light_list_jittered(pk, n, kp, gp, P, None, W, H, 0, 0, M, pr0, api._probes(good, (0, 6, 28, 0, 3)), R, 1) == 0
    cases = [(bad, api._probes(None, (0,) * 8), api._probes(None, (0,) * 8)) for bad in bad_lists(good)]
    cases += [(l, api._probes(l, pr), tb0) for l, pr in bad_probes(good)]
    cases += [(good, api._probes(good, pr), api._probes(good, tb)) for pr, tb in bad_tables(good)]
    for bad, pr, tb in cases:
        bp = api.C.byref(bad) if bad is not None else None
        assert lib.rtsh_soft_light_list_jittered(pk, n, kp, bp, P, None, W, H, 0, H, M, pr, tb, R, 1) == 1
        # the device entry points refuse the arguments before any device call (no context is needed to be told so)
        assert lib.rts_trace_soft_light_list_jittered(None, kp, bp, P, None, W, H, 0, H, M, pr, tb, R) == 1
        assert lib.rts_trace_soft_light_list_jittered_device(None, kp, bp, P, None, W, H, 0, H, M, pr, tb, R, None) == 1
        assert lib.rts_trace_soft_light_list_jittered_stripes_device(None, kp, bp, P, None, W, H, 8, 2, 0, M, pr, tb, R, None) == 1
    assert lib.rtsh_soft_light_list_jittered(None, n, kp, gp, P, None, W, H, 0, H, M, pr0, tb0, R, 1) == 1
    assert lib.rtsh_soft_light_list_jittered(pk, n, None, gp, P, None, W, H, 0, H, M, pr0, tb0, R, 1) == 1
    assert lib.rtsh_soft_light_list_jittered(pk, n, kp, gp, None, None, W, H, 0, H, M, pr0, tb0, R, 1) == 1
    assert lib.rtsh_soft_light_list_jittered(pk, n, kp, gp, P, None, W, H, 0, H, None, pr0, tb0, R, 1) == 1
    assert lib.rtsh_soft_light_list_jittered(pk, n, kp, gp, P, None, W, H, 9, 8, M, pr0, tb0, R, 1) == 1
    assert lib.rtsh_soft_light_list_jittered(pk, n, kp, gp, P, None, W, H, 0, H + 1, M, pr0, tb0, R, 1) == 1
    assert lib.rts_trace_soft_light_list_jittered_stripes_device(None, kp, gp, P, None, W, H, 8, 2, 2, M, pr0, tb0, R, None) == 1   # stripe >= n_stripes
    assert (out == GUARD).all() and (ref == GUARD).all()     # nothing was written
    # tables from the count up are not read, and the wrapper wants one integer per light
    three = make_list("overlap")
    long_probes = (api.C.c_uint32 * 8)(0, 4, 0, 99, 99, 99, 99, 99)
    long_tables = (api.C.c_uint32 * 8)(20, 0, 12, 1, 99, 0xFFFFFFFF, 49, 7)
    c = np.zeros((3, H, W), np.uint8)
    assert lib.rtsh_soft_light_list_jittered(pk, n, kp, api.C.byref(three), P, None, W, H, 0, H, api._ptr(c), long_probes, long_tables, None, 0) == 0
    assert np.array_equal(c, fr.want("overlap", (0, 4, 0), (20, 0, 12))[0])
    with pytest.raises(api.RtsError):
        api.soft_light_list_adaptive(packed, k, three, (0, 4, 0), fr.pos, W, H, tables=(20, 0))
    with pytest.raises(api.RtsError):
        api.soft_light_list_adaptive(packed, k, three, (0, 4, 0), fr.pos, W, H, tables=(20, 0, -1))


def test_the_derived_light_is_the_hand_built_one():
    lights = make_list("mixed")
    table = np.array([[lights.offsets[j][i] for i in range(3)] for j in range(48)], np.float32)
    for l, T in ((1, 6), (2, 12), (2, 28), (4, 3), (2, 0)):
        e = lights.lights[l]
        rows = np.float32(e.radius) * table[e.first:e.first + (T or e.nsamples)]
        want = api.Light.make(e.type, list(e.xyz), rows)
        want.nsamples, want.table = e.nsamples, T
        got = lights.light(l, table=T)
        assert bytes(got) == bytes(want), (l, T)
        assert got.table == T and got.nsamples == e.nsamples
    assert bytes(lights.light(2)) == bytes(lights.light(2, table=0))
    for l, T in ((0, 1), (2, 4), (2, 29), (4, 4)):
        with pytest.raises(api.RtsError):
            lights.light(l, table=T)


def test_the_argument_rule_over_its_boundary_values(tmp_path):
    """tests/cpp/soft_list_tables_host.cpp: softListTablesOk against a slow restatement, built with the host sanitizers."""
    exe = str(tmp_path / "soft_list_tables_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "cpp", "soft_list_tables_host.cpp"), "-o", exe], check=True)
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "ok" in done.stdout
