"""CPU: the host twin of the light list trace (rtsh_light_list, include/rts_scene.h; api.light_list) against the definition taken from
the untouched oracle (tests/light_list_cases.py: definition), byte for byte; the light map (rtsh_facing_lights) against the one-light
facing mark; the argument checks that need no device; and the layouts of rts_light_entry and rts_light_list as gcc sees them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from light_list_cases import FRAMES, LISTS, definition, list_frame, make_list
from raytracedshadows_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xAB


def _map(fr, count):
    """A map that mixes every bit pattern below `count` with bits above it, whole zero bytes included."""
    y, x = np.mgrid[0:fr.H, 0:fr.W]
    m = ((x * 7 + y * 13 + (x >> 3) * 5) & 0xFF).astype(np.uint8)
    m[(x + y) % 5 == 0] = 0
    assert ((m & ((1 << count) - 1)) == 0).any() and (m != 0).any()
    return m


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("name", list(LISTS))
def test_twin_equals_the_oracle(name, W, H):
    fr = list_frame(W, H)
    lights = make_list(name)
    assert lights.count == len(LISTS[name])
    want = fr.oracle_bits(name)                          # (asserts that no light of the list degenerates)
    assert np.array_equal(fr.want(name), want), name
    assert (want >> lights.count == 0).all()
    # with a map: the oracle's byte and'ed with the map's bit, over a row range that leaves the other rows alone
    m = _map(fr, lights.count)
    with_map = definition(fr.packed, fr.k, lights, fr.pos, m)
    assert np.array_equal(with_map, want & m)
    got = api.light_list(fr.packed, fr.k, lights, fr.pos, fr.W, fr.H, lights_map=m)
    assert np.array_equal(got, with_map), name
    out = np.full((fr.H, fr.W), GUARD, np.uint8)
    api.light_list(fr.packed, fr.k, lights, fr.pos, fr.W, fr.H, lights_map=m, row_begin=8, row_end=29, out=out)
    rows = (np.arange(fr.H) >= 8) & (np.arange(fr.H) < 29)
    assert np.array_equal(out, np.where(rows[:, None], with_map, GUARD)), name
    out = np.full((fr.H, fr.W), GUARD, np.uint8)
    api.light_list(fr.packed, fr.k, lights, fr.pos, fr.W, fr.H, row_begin=8, row_end=29, out=out)
    assert np.array_equal(out, np.where(rows[:, None], want, GUARD)), name


def test_unmarked_pixels_may_hold_anything():
    fr = list_frame(64, 48)
    lights, want = make_list("5"), fr.want("5")
    m = _map(fr, 5)
    dead = (m & 31) == 0
    dirty = fr.pos.copy()
    dirty[dead] = np.array([np.nan, np.inf, 1e38, -np.inf], np.float32)
    got = api.light_list(fr.packed, fr.k, lights, dirty, fr.W, fr.H, lights_map=m)
    assert np.array_equal(got, want & m) and (got[dead] == 0).all() and dead.sum() > 100


def test_bits_from_the_count_up_are_zero():
    fr = list_frame(61, 37)
    for name in ("1", "3", "5"):
        full = np.full((fr.H, fr.W), 0xFF, np.uint8)
        got = api.light_list(fr.packed, fr.k, make_list(name), fr.pos, fr.W, fr.H, lights_map=full)
        assert np.array_equal(got, fr.want(name)) and (got >> len(LISTS[name]) == 0).all()
    # reserved_ is ignored
    lights = make_list("3")
    for i in range(3):
        lights.reserved_[i] = 0xDEADBEEF
    assert np.array_equal(api.light_list(fr.packed, fr.k, lights, fr.pos, fr.W, fr.H), fr.want("3"))


@pytest.mark.parametrize("W,H", FRAMES)
def test_facing_lights_is_the_facing_mark_per_light(W, H):
    fr = list_frame(W, H)
    for name in ("1", "4", "8"):
        lights = make_list(name)
        got = fr.facing(name)
        for l in range(lights.count):
            one = api.facing_active(fr.k, lights.light(l), fr.pos, fr.nrm)
            assert np.array_equal((got >> l) & 1, one), (name, l)
            assert 0 < int(one.sum()) < one.size
        assert (got >> lights.count == 0).all()
    # directional lights alone need no positions; a point light does
    dirs = api.LightList.make([make_list("2").lights[0]])
    assert np.array_equal(api.facing_lights(fr.k, dirs, None, fr.nrm), api.facing_active(fr.k, dirs.light(0), None, fr.nrm))
    with pytest.raises(api.RtsError):
        api.facing_lights(fr.k, make_list("2"), None, fr.nrm)


def _copy(lights, **fields):
    c = type(lights).from_buffer_copy(lights)
    for f, v in fields.items():
        setattr(c, f, v)
    return c


def test_refusals_without_a_device():
    fr = list_frame(64, 48)
    W, H, packed, k = fr.W, fr.H, fr.packed, fr.k
    lib, kp = api._lib, api.C.byref(k)
    out = np.full((H, W), GUARD, np.uint8)
    P, M, N = api._ptr(fr.pos), api._ptr(out), api._ptr(fr.nrm)
    pk, n = api._ptr(packed), packed.shape[0]
    good = make_list("4")
    gp = api.C.byref(good)
    badtype = _copy(good)
    badtype.lights[2].type = 2
    beyond = _copy(good)
    beyond.lights[5].type = 7                            # an entry at or above count is not looked at
    assert lib.rtsh_light_list(pk, n, kp, api.C.byref(beyond), P, None, W, H, 0, 0, M, 1) == 0
    for bad in (None, _copy(good, count=0), _copy(good, count=9), badtype):
        bp = api.C.byref(bad) if bad is not None else None
        assert lib.rtsh_light_list(pk, n, kp, bp, P, None, W, H, 0, H, M, 1) == 1
        assert lib.rtsh_facing_lights(kp, bp, P, N, W, H, M) == 1
        # the device entry points refuse the list before any device call (no context is needed to be told so)
        assert lib.rts_trace_light_list(None, kp, bp, P, None, W, H, 0, H, M) == 1
        assert lib.rts_trace_light_list_device(None, kp, bp, P, None, W, H, 0, H, M, None) == 1
        assert lib.rts_trace_light_list_stripes_device(None, kp, bp, P, None, W, H, 8, 2, 0, M, None) == 1
        assert lib.rtsh_facing_lights_device(None, kp, bp, P, N, W, H, M, None) == 1
    assert lib.rtsh_light_list(None, n, kp, gp, P, None, W, H, 0, H, M, 1) == 1
    assert lib.rtsh_light_list(pk, n, None, gp, P, None, W, H, 0, H, M, 1) == 1
    assert lib.rtsh_light_list(pk, n, kp, gp, None, None, W, H, 0, H, M, 1) == 1
    assert lib.rtsh_light_list(pk, n, kp, gp, P, None, W, H, 0, H, None, 1) == 1
    assert lib.rtsh_light_list(pk, n, kp, gp, P, None, W, H, 9, 8, M, 1) == 1
    assert lib.rtsh_light_list(pk, n, kp, gp, P, None, W, H, 0, H + 1, M, 1) == 1
    assert lib.rts_trace_light_list_device(None, kp, gp, P, None, W, H, 0, H, M, None) == 1
    assert lib.rts_trace_light_list_stripes_device(None, kp, gp, P, None, W, H, 8, 2, 2, M, None) == 1      # stripe >= n_stripes
    assert (out == GUARD).all()                          # nothing was written
    with pytest.raises(api.RtsError):
        api.LightList.make([(0, (0, 0, 1))] * 9)


def test_layouts_are_what_the_compiler_lays_out(tmp_path):
    """rts_light_entry is 16 bytes and rts_light_list 144, and gcc lays both out from include/rts.h as the ctypes mirrors do."""
    assert ctypes.sizeof(api.LightEntry) == 16 and ctypes.sizeof(api.LightList) == 144
    assert api.LightList.MAX == 8
    pairs = (("rts_light_entry", api.LightEntry), ("rts_light_list", api.LightList))
    body = '  printf("%d\\n", (int)RTS_MAX_LIST_LIGHTS);\n'
    for cname, mirror in pairs:
        body += f'  printf("%zu", sizeof({cname}));\n'
        body += "".join(f'  printf(" %zu", offsetof({cname}, {f}));\n' for f, _ in mirror._fields_) + '  printf("\\n");\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rts.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert int(lines[0]) == 8
    for (cname, mirror), line in zip(pairs, lines[1:]):
        got = [int(v) for v in line.split()]
        assert got[0] == ctypes.sizeof(mirror), cname
        assert got[1:] == [getattr(mirror, f).offset for f, _ in mirror._fields_], cname
