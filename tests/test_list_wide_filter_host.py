"""CPU: the host twins of the wide (a-trous) filter of a light list's planes (rtsh_wide_filter_light_list,
rtsh_wide_filter_soft_light_list) against the numpy rule of tests/list_wide_filter_cases.py, bit for bit -- and what pins the rule: the
three anchors, the clamp of a byte to n_l, NaN and Inf in the G-buffer, the planes that are never touched, every refusal, the struct's
layout, and the host twins under the address and UB sanitizers (tests/cpp/list_wide_filter_host.cpp, a program of its own)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import list_combine_cases as lc
import list_filter_cases as fc
import list_wide_filter_cases as wc
import scene_pass_cases as sp
from raytracedshadows_amd import api

f32 = np.float32
INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _twin(form, lst, p, pos, nrm, planes, mask, lights_map, threads=0):
    if form == "hard":
        return api.wide_filter_light_list(lst, p, pos, nrm, mask, lights_map, threads)
    return api.wide_filter_soft_light_list(lst, p, pos, nrm, planes, lights_map, threads)


@pytest.mark.parametrize("wh", wc.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twins_equal_the_numpy_rule(wh):
    """Awkward, geometric and (at the sizes this filter adds) flat frames; hard and soft lists of 1, 4 and 8 lights with n_l of 1, 4, 16 and 48 in every entry; with and
    without the map; passes 0 .. 5."""
    for kind in wc.kinds(wh):
        nrm, pos, planes, mask, lights_map, _ = wc.frame(kind, wh)
        for form, count, rotation in wc.lists():
            lst = wc.the_list(form, count, rotation)
            for with_map in (False, True):
                m = lights_map if with_map else None
                want = wc.wide_filter_rule(lst, wc.params(0, kind), pos, nrm, mask if form == "hard" else planes, m)
                for passes in wc.PASSES:
                    got = _twin(form, lst, wc.params(passes, kind), pos, nrm, planes, mask, m)
                    wc.same_bits(got, want[passes], (kind, wh, form, count, rotation, with_map, passes))


def test_the_72_frame_reaches_both_far_taps_and_every_pass_changes_it():
    """On the geometric 72 x 72 frame every pass accepts some taps and rejects some, a step-16 pass accepts its -32 and +32 taps (both
    at one pixel on the flat frame), and each pass changes the planes: the filter is no identity and no pass is idle."""
    nrm, pos, planes, mask, lights_map, _ = wc.frame("geometric", (72, 72))
    lst = wc.the_list("soft", 8, 1)
    census = {}
    outs = wc.wide_filter_rule(lst, wc.params(0), pos, nrm, planes, lights_map, census=census)
    for k in range(5):
        assert census[k][0] > 50 and census[k][1] > 50, (k, census)
        assert (outs[k] != outs[k + 1]).any(), k
    # the far taps of the step-16 pass: each accepted somewhere on this frame (its crease and its depth step lie between the -32 and the
    # +32 tap of every pixel that has both), and BOTH accepted at some pixels of the flat frame, in x and in y
    taps = {(dx, dy): geom for _, _, _, geom, dx, dy in wc._taps(pos, nrm, wc.params(0).normal_cos_min, wc.params(0).plane_eps, 16)[1]}
    assert all(taps[t].any() for t in ((-2, 0), (2, 0), (0, -2), (0, 2)))
    f_nrm, f_pos = wc.frame("flat", (72, 72))[:2]
    taps = {(dx, dy): geom for _, _, _, geom, dx, dy in wc._taps(f_pos, f_nrm, wc.params(0).normal_cos_min, wc.params(0).plane_eps, 16)[1]}
    assert (taps[(-2, 0)] & taps[(2, 0)]).any() and (taps[(0, -2)] & taps[(0, 2)]).any() and (taps[(-2, -2)] & taps[(2, 2)]).any()
    assert ((outs[5] > 0) & (outs[5] < 1)).any()


def test_threads_change_nothing():
    nrm, pos, planes, mask, lights_map, _ = wc.frame("geometric", (72, 40))
    lst = wc.the_list("soft", 8, 2)
    one = _twin("soft", lst, wc.params(4), pos, nrm, planes, mask, lights_map, threads=1)
    wc.same_bits(_twin("soft", lst, wc.params(4), pos, nrm, planes, mask, lights_map, threads=7), one, "7 threads")


@pytest.mark.parametrize("kind", ["awkward", "geometric"])
def test_anchor_no_neighbour_gives_the_centre_quotient(kind):
    """Anchor 1: passes == 0 -- or thresholds no neighbour passes at any pass (a negative plane distance; a cosine above any) -- gives
    (float)min(c, n_l) / (float)n_l where the pixel is active and +0 elsewhere; where c <= n_l that is the R = 0 filter's plane."""
    for wh in ((17, 15), (40, 72)):
        nrm, pos, planes, mask, lights_map, _ = wc.frame(kind, wh)
        for form, count, rotation in (("hard", 8, 0), ("soft", 8, 0), ("soft", 8, 3), ("soft", 1, 1)):
            lst = wc.the_list(form, count, rotation)
            for with_map in (False, True):
                m = lights_map if with_map else None
                want = wc.centre_quotient(lst, mask if form == "hard" else planes, nrm, m)
                closed = [api.WideFilterParams.make(0, 0.9, 0.02), api.WideFilterParams.make(5, 3e38, -1.0),
                          api.WideFilterParams.make(3, -1e30, -1e-30)]
                for p in closed:
                    wc.same_bits(_twin(form, lst, p, pos, nrm, planes, mask, m), want, (kind, wh, form, count, rotation, with_map, p.passes))
                # ... and the R = 0 filter's plane wherever the byte does not exceed n_l
                n_l = np.array(wc.samples_of(lst)).reshape(-1, 1, 1)
                if form == "soft":
                    tame = np.minimum(planes[:count], n_l).astype(np.uint8)
                    r0 = api.filter_soft_light_list(lst, fc.params(0), pos, nrm, tame, m)
                    wc.same_bits(api.wide_filter_soft_light_list(lst, wc.params(0, kind), pos, nrm, tame, m), r0, "R = 0, soft")
                else:
                    r0 = api.filter_light_list(lst, fc.params(0), pos, nrm, mask, m)
                    wc.same_bits(api.wide_filter_light_list(lst, wc.params(0, kind), pos, nrm, mask, m), r0, "R = 0, hard")


def test_anchor_equal_values_give_the_centre_quotient():
    """Anchor 2: where every tap that can be accepted carries the same byte, every pass returns it: the rounded mean of equal values."""
    nrm, pos, planes, mask, lights_map, _ = wc.frame("geometric", (72, 72))
    lst = wc.the_list("soft", 8, 0)                                    # n_l = 1, 4, 16, 48, 1, 4, 16, 48
    flat = np.stack([np.full((72, 72), b, np.uint8) for b in (1, 3, 7, 47, 0, 4, 16, 255)])
    want = wc.centre_quotient(lst, flat, nrm, lights_map)
    for passes in (1, 3, 5):
        wc.same_bits(api.wide_filter_soft_light_list(lst, wc.params(passes), pos, nrm, flat, lights_map), want, passes)
    hard = wc.the_list("hard", 8)
    got = api.wide_filter_light_list(hard, wc.params(5), pos, nrm, np.full((72, 72), 0xA5, np.uint8), lights_map)
    wc.same_bits(got, wc.centre_quotient(hard, np.full((72, 72), 0xA5, np.uint8), nrm, lights_map), "hard")


def test_anchor_range():
    """Anchor 3: visibility stays inside [0, 1], and inside the range of the input quotients of the light: a mean leaves no range."""
    for kind in ("awkward", "geometric"):
        nrm, pos, planes, mask, lights_map, _ = wc.frame(kind, (72, 72))
        lst = wc.the_list("soft", 8, 1)
        lo_hi = wc.centre_quotient(lst, planes, nrm, lights_map)
        for passes in wc.PASSES:
            got = api.wide_filter_soft_light_list(lst, wc.params(passes, kind), pos, nrm, planes, lights_map)
            assert (got >= 0).all() and (got <= 1).all(), (kind, passes)
            for l in range(8):
                on = lo_hi[l] > -1 if lights_map is None else (((lights_map >> l) & 1) != 0) & ~(nrm[..., :3] == 0).all(axis=-1)
                if on.any():
                    # one 16-bit step of slack: V is rounded to nearest, the bound is on V, not on the quotient's float
                    assert got[l][on].min() >= lo_hi[l][on].min() and got[l][on].max() <= lo_hi[l][on].max(), (kind, passes, l)


def test_bytes_above_the_sample_count_behave_as_the_sample_count():
    nrm, pos, planes, mask, lights_map, _ = wc.frame("geometric", (40, 72))
    lst = wc.the_list("soft", 8, 1)
    n_l = np.array(wc.samples_of(lst)).reshape(-1, 1, 1)
    assert (planes > n_l).any()
    clamped = np.minimum(planes, n_l).astype(np.uint8)
    for passes in (0, 2, 5):
        p = wc.params(passes)
        wc.same_bits(api.wide_filter_soft_light_list(lst, p, pos, nrm, planes, lights_map),
                     api.wide_filter_soft_light_list(lst, p, pos, nrm, clamped, lights_map), passes)


def test_nan_and_inf_in_the_gbuffer_reject_taps():
    """NaN and Inf in positions and normals: a tap whose comparison meets a NaN is rejected, the centre stays accepted; the twin
    equals the rule and every value stays in [0, 1]."""
    nrm, pos, planes, mask, lights_map, _ = (a.copy() for a in wc.frame("geometric", (72, 40)))
    rs = np.random.RandomState(7)
    for a in (nrm, pos):
        for value in (np.nan, np.inf, -np.inf, 3e38):
            idx = rs.randint(0, 72 * 40, 60)
            a.reshape(-1, 4)[idx, rs.randint(0, 3, 60)] = value
    lst = wc.the_list("soft", 4, 1)
    want = wc.wide_filter_rule(lst, wc.params(0), pos, nrm, planes, lights_map)
    for passes in wc.PASSES:
        got = api.wide_filter_soft_light_list(lst, wc.params(passes), pos, nrm, planes, lights_map)
        wc.same_bits(got, want[passes], passes)
        assert (got >= 0).all() and (got <= 1).all()


def test_visibility_combine_over_a_passes_0_plane_is_the_list_combine():
    """combine_visibility_list over a passes == 0 plane gives combine_soft_light_list's bytes over the clamped counts (the traces
    write no more than n_l), and combine_light_list's for a hard list."""
    k = sp.constants("unit")
    for kind in ("awkward", "geometric"):
        nrm, pos, planes, mask, lights_map, _ = wc.frame(kind, (17, 15))
        soft, hard = wc.the_list("soft", 8, 1), wc.the_list("hard", 8)
        tame = np.minimum(planes, np.array(wc.samples_of(soft)).reshape(-1, 1, 1)).astype(np.uint8)
        for m in (None, lights_map):
            vis = api.wide_filter_soft_light_list(soft, wc.params(0, kind), pos, nrm, tame, m)
            assert (api.combine_visibility_list(k, soft.hard_list(), pos, nrm, vis, m) == api.combine_soft_light_list(k, soft, pos, nrm, tame, m)).all()
            vis = api.wide_filter_light_list(hard, wc.params(0, kind), pos, nrm, mask, m)
            assert (api.combine_visibility_list(k, hard, pos, nrm, vis, m) == api.combine_light_list(k, hard, pos, nrm, mask, m)).all()


def test_planes_from_the_count_up_are_never_touched():
    """Exactly `count` planes of counts and visibility are used; a background pixel's position, map byte and count bytes, and the bytes
    of a light whose map bit is clear, are never looked at."""
    nrm, pos, planes, mask, lights_map, _ = wc.frame("geometric", (17, 15))
    lst = wc.the_list("soft", 4, 1)
    p = wc.params(3)
    want = wc.wide_filter_rule(lst, p, pos, nrm, planes, lights_map)[3]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    counts = np.ascontiguousarray(planes[:4])                            # a block of exactly four planes
    vis = np.full((8, 15, 17), 7.5, f32)
    assert api._lib.rtsh_wide_filter_soft_light_list(C.byref(lst), C.byref(p), ptr(np.ascontiguousarray(pos)), ptr(np.ascontiguousarray(nrm)),
                                                     ptr(np.ascontiguousarray(lights_map)), ptr(counts), 17, 15, ptr(vis), 0) == 0
    wc.same_bits(vis[:4], want, "planes below the count")
    assert (vis[4:] == 7.5).all()
    background = (nrm[..., :3] == 0).all(axis=-1)
    counts, map2 = planes.copy(), lights_map.copy()
    for l in range(4):
        counts[l][((lights_map >> l) & 1) == 0] ^= 0xFF
    counts[:, background] ^= 0xFF
    map2[background] ^= 0xFF
    wc.same_bits(api.wide_filter_soft_light_list(lst, p, pos, nrm, counts, map2), want, "poisoned unread bytes")


def test_refusals_write_nothing():
    lib = api._lib
    nrm, pos, planes, mask, lights_map, _ = (np.ascontiguousarray(a) for a in wc.frame("geometric", (16, 16)))
    vis = np.full((8, 16, 16), 7.5, f32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ref = lambda s: C.byref(s) if s is not None else None
    good = wc.params(3)
    hard_bad, soft_bad = lc.bad_lists()
    hard, soft = wc.the_list("hard", 4), wc.the_list("soft", 4, 1)

    def call(form, lst, p, pos_=pos, nrm_=nrm, plane=True, W=16, H=16, out=vis):
        fn = lib.rtsh_wide_filter_light_list if form == "hard" else lib.rtsh_wide_filter_soft_light_list
        return fn(ref(lst), ref(p), ptr(pos_), ptr(nrm_), ptr(lights_map), ptr((mask if form == "hard" else planes) if plane else None), W, H,
                  ptr(out), 0)

    def bad_params():
        out = [None]
        for field, value in (("passes", 6), ("passes", 0xFFFFFFFF), ("normal_cos_min", np.nan), ("normal_cos_min", np.inf),
                             ("plane_eps", -np.inf), ("plane_eps", np.nan)):
            p = wc.params(3)
            setattr(p, field, value)
            out.append(p)
        return out

    for form, lst, bad in (("hard", hard, hard_bad), ("soft", soft, soft_bad)):
        assert call(form, lst, good) == 0
        vis[:] = 7.5
        for b in bad:
            assert call(form, b, good) == INVALID, form
        for p in bad_params():
            assert call(form, lst, p) == INVALID, form
        assert call(form, lst, good, pos_=None) == INVALID
        assert call(form, lst, good, nrm_=None) == INVALID
        assert call(form, lst, good, plane=False) == INVALID
        assert call(form, lst, good, out=None) == INVALID
        assert call(form, lst, good, W=0) == INVALID
        assert call(form, lst, good, H=0) == INVALID
        assert call(form, lst, good, W=0x7FFFFFF1, H=1) == INVALID
        assert call(form, lst, good, W=1, H=0x7FFFFFF1) == INVALID
        assert (vis == 7.5).all(), form
    p = wc.params(3)
    p.reserved_[0] = 0xFFFFFFFF                                          # (ignored)
    assert call("soft", soft, p) == 0
    with pytest.raises(api.RtsError):
        api.wide_filter_soft_light_list(soft, good, None, nrm, planes)


def test_scratch_bytes():
    assert api.wide_filter_scratch_bytes(4, 3840, 2160) == 2 * 4 * 3840 * 2160 * 2
    assert api.wide_filter_scratch_bytes(8, 65536, 65536) == 2 * 8 * 65536 * 65536 * 2
    assert api.wide_filter_scratch_bytes(0, 16, 16) == 0 and api.wide_filter_scratch_bytes(9, 16, 16) == 0
    assert api.wide_filter_scratch_bytes(1, 0, 16) == 0 and api.wide_filter_scratch_bytes(1, 16, 0) == 0


def test_params_layout_is_what_the_compiler_lays_out(tmp_path):
    """rtsh_wide_filter_params is 32 bytes, and gcc lays out its fields where the ctypes mirror has them (tests/test_abi.py's way)."""
    mirror = api.WideFilterParams
    assert C.sizeof(mirror) == 32 and mirror.MAX_PASSES == 5
    body = '  printf("%zu", sizeof(rtsh_wide_filter_params));\n'
    body += "".join(f'  printf(" %zu", offsetof(rtsh_wide_filter_params, {f}));\n' for f, _ in mirror._fields_)
    body += '  printf(" %d\\n", (int)RTSH_WIDE_FILTER_MAX_PASSES);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rts_scene.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == 32
    assert got[1:-1] == [getattr(mirror, f).offset for f, _ in mirror._fields_]
    assert got[-1] == 5


def test_list_wide_filter_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/list_wide_filter_host.cpp: the host twins themselves (rts_scene.cpp and the shared per-pixel source, compiled into the
    program -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow, over every refusal and
    over the tiny and the 72 x 72 frames, whose buffers are heap blocks of exactly the size the header states."""
    exe = str(tmp_path / "list_wide_filter_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "list_wide_filter_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 1000, run.stdout[-2000:]
