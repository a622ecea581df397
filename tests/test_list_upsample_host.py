"""CPU: half-resolution light lists on the host (include/rts_scene.h: rtsh_subsample_gbuffer, rtsh_upsample_retrace_map,
rtsh_upsample_soft_light_list, rtsh_upsample_light_list).  The host twins against the numpy rules of
tests/list_upsample_cases.py byte for byte, over every shape and phase of the cases, lists of 1 and 8 lights, soft and hard, maps and
keep present and absent, on the synthetic frames (NaN, Inf and zero normals planted) and on a cornell G-buffer; the five anchors of the
header; every refusal with its outputs shown untouched; and the twins on tiny frames under the sanitizers
(tests/cpp/list_upsample_host.cpp).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import list_combine_cases as lc
import list_upsample_cases as uc
from raytracedshadows_amd import api
from soft_list_cases import make_list, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
POISON = 0xA5
CASES = [(kind, wh, phase) for kind in ("planes", "random") for wh in uc.SHAPES for phase in uc.PHASES if uc.valid(wh, phase)]
ids = lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2][0]}{c[2][1]}"


def low(kind, wh, phase, with_map):
    pos, nrm, m = uc.gbuffer(kind, wh)
    return uc.subsample_rule(phase, pos, nrm, m if with_map else None)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_subsample_equals_the_rule(case):
    kind, wh, phase = case
    pos, nrm, m = uc.gbuffer(kind, wh)
    w, h = uc.size(wh[0], wh[1], *phase)
    assert api.subsampled_size(wh[0], wh[1], *phase) == (w, h)
    for with_map in (False, True):
        got = api.subsample_gbuffer(uc.params(phase), pos, nrm, m if with_map else None)
        want = uc.subsample_rule(phase, pos, nrm, m if with_map else None)
        assert got[0].shape == (h, w, 4) and got[0].view(np.uint32).tolist() == want[0].view(np.uint32).tolist()
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        assert (got[2] is None and want[2] is None) if not with_map else np.array_equal(got[2], want[2])


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_retrace_map_equals_the_rule(case):
    """Anchor 5: for ordinary thresholds the map is "active, not sampled, no accepted tap" as the numpy rule computes it."""
    kind, wh, phase = case
    pos, nrm, m = uc.gbuffer(kind, wh)
    p = uc.params(phase)
    for count in uc.COUNTS:
        for with_map, own_low_map in ((False, False), (True, False), (True, True)):
            lo_pos, lo_nrm, lo_map = low(kind, wh, phase, with_map)
            if own_low_map:
                lo_map = uc.low_planes(wh, phase)[2]
            fm = m if with_map else None
            got = api.upsample_retrace_map(count, p, pos, nrm, lo_pos, lo_nrm, fm, lo_map)
            assert np.array_equal(got, uc.retrace_rule(count, p, pos, nrm, lo_pos, lo_nrm, fm, lo_map)), (count, with_map, own_low_map)
            assert (got >> count == 0).all()


def test_retrace_map_census():
    """The frames exercise both sides: pixels with an accepted tap and pixels to retrace, per phase, on both kinds."""
    for kind in ("planes", "random"):
        for phase in uc.PHASES:
            pos, nrm, m = uc.gbuffer(kind, (64, 40))
            lo_pos, lo_nrm, _ = low(kind, (64, 40), phase, False)
            r = uc.retrace_rule(1, uc.params(phase), pos, nrm, lo_pos, lo_nrm)
            active_unsampled = int((uc.retrace_rule(1, uc.params(phase, uc.NONE_ACCEPTED), pos, nrm, lo_pos, lo_nrm) != 0).sum())
            assert 50 <= int((r != 0).sum()) <= active_unsampled - 50, (kind, phase, int((r != 0).sum()), active_unsampled)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_upsample_equals_the_rule(case):
    kind, wh, phase = case
    pos, nrm, m = uc.gbuffer(kind, wh)
    p = uc.params(phase)
    planes, mask, own_map = uc.low_planes(wh, phase)
    keep = uc.keep_map(wh)
    H, W = nrm.shape[:2]
    for count in uc.COUNTS:
        soft, hard = uc.soft_list(count), uc.hard_list(count)
        for with_map, own_low_map in ((False, False), (True, False), (True, True)):
            lo_pos, lo_nrm, lo_map = low(kind, wh, phase, with_map)
            lo_map = own_map if own_low_map else lo_map
            fm = m if with_map else None
            for with_keep in (False, True):
                k = keep if with_keep else None
                what = (count, with_map, own_low_map, with_keep)
                before = np.full((8, H, W), POISON, np.uint8)
                want, _ = uc.upsample_rule(count, False, p, pos, nrm, lo_pos, lo_nrm, planes, fm, lo_map, k, before if with_keep else None)
                got = api.upsample_soft_light_list(soft, p, pos, nrm, lo_pos, lo_nrm, planes, fm, lo_map, k, out=before.copy())
                assert np.array_equal(got[:count], want), ("soft",) + what
                assert (got[count:] == POISON).all(), "a plane from the count up was written"
                if with_keep:
                    for l in range(count):
                        assert (got[l][(keep >> l) & 1 != 0] == POISON).all(), "a kept byte was touched"
                before = np.full((H, W), POISON, np.uint8)
                want, _ = uc.upsample_rule(count, True, p, pos, nrm, lo_pos, lo_nrm, mask, fm, lo_map, k, before if with_keep else None)
                got = api.upsample_light_list(hard, p, pos, nrm, lo_pos, lo_nrm, mask, fm, lo_map, k, out=before.copy())
                assert np.array_equal(got, want), ("hard",) + what


def test_one_thread_and_three_agree():
    pos, nrm, m = uc.gbuffer("planes", (33, 19))
    p = uc.params((1, 0))
    lo_pos, lo_nrm, lo_map = low("planes", (33, 19), (1, 0), True)
    planes = uc.low_planes((33, 19), (1, 0))[0]
    a = api.upsample_soft_light_list(uc.soft_list(8), p, pos, nrm, lo_pos, lo_nrm, planes, m, lo_map, threads=1)
    b = api.upsample_soft_light_list(uc.soft_list(8), p, pos, nrm, lo_pos, lo_nrm, planes, m, lo_map, threads=3)
    assert np.array_equal(a, b)
    assert np.array_equal(api.upsample_retrace_map(8, p, pos, nrm, lo_pos, lo_nrm, m, lo_map, threads=1),
                          api.upsample_retrace_map(8, p, pos, nrm, lo_pos, lo_nrm, m, lo_map, threads=3))


@pytest.mark.parametrize("phase", uc.PHASES, ids=str)
def test_anchor_sampled_pixels_get_their_low_resolution_byte(phase):
    """Anchor 1, with a low-resolution map of its own whose bits are clear at some sampled pixels: the tap that is the pixel itself
    does not look at its map bit."""
    for kind in ("planes", "random"):
        wh = (33, 19)
        pos, nrm, m = uc.gbuffer(kind, wh)
        lo_pos, lo_nrm, _ = low(kind, wh, phase, True)
        planes, mask, own_map = uc.low_planes(wh, phase)
        p = uc.params(phase)
        got = api.upsample_soft_light_list(uc.soft_list(8), p, pos, nrm, lo_pos, lo_nrm, planes, m, own_map)
        bits = api.upsample_light_list(uc.hard_list(8), p, pos, nrm, lo_pos, lo_nrm, mask, m, own_map)
        px, py = phase
        active = uc._active(8, nrm, m)[py::2, px::2]
        assert (active != 0).sum() > 20
        for l in range(8):
            on = (active >> l) & 1 != 0
            assert np.array_equal(got[l][py::2, px::2][on], planes[l][on]), (kind, l)
            assert (got[l][py::2, px::2][~on] == 0).all()
        assert np.array_equal(bits[py::2, px::2], mask & active)


def test_anchor_uniform_taps_give_their_byte():
    """Anchor 2: planes that hold one byte c give c at every active pixel that has an on tap -- accepted or through the fallback --
    and 0 elsewhere, for every c that a rounding slip would move."""
    wh, phase = (33, 19), (1, 1)
    pos, nrm, m = uc.gbuffer("planes", wh)
    lo_pos, lo_nrm, lo_map = low("planes", wh, phase, True)
    p = uc.params(phase)
    for c in (0, 1, 2, 3, 127, 128, 254, 255):
        planes = uc.low_planes(wh, phase, uniform=c)[0]
        got = api.upsample_soft_light_list(uc.soft_list(8), p, pos, nrm, lo_pos, lo_nrm, planes, m, lo_map)
        assert set(np.unique(got).tolist()) <= {0, c}, c
        want, _ = uc.upsample_rule(8, False, p, pos, nrm, lo_pos, lo_nrm, planes, m, lo_map)
        assert np.array_equal(got, want)
    assert (got == 255).sum() > 500


@pytest.mark.parametrize("kind", ["planes", "random"])
def test_anchor_no_fallback_under_the_retrace_map(kind):
    """Anchor 3: with keep = the retrace map of the same params and maps, the rule's fallback census is empty over the written bytes --
    and it is not without keep, so the census looks at something."""
    wh = (64, 40)
    pos, nrm, m = uc.gbuffer(kind, wh)
    for phase in uc.PHASES:
        p = uc.params(phase)
        lo_pos, lo_nrm, lo_map = low(kind, wh, phase, True)
        planes = uc.low_planes(wh, phase)[0]
        keep = api.upsample_retrace_map(8, p, pos, nrm, lo_pos, lo_nrm, m, lo_map)
        before = np.full((8, wh[1], wh[0]), POISON, np.uint8)
        want, fell = uc.upsample_rule(8, False, p, pos, nrm, lo_pos, lo_nrm, planes, m, lo_map, keep, before)
        assert not fell.any(), (kind, phase)
        _, fell_without = uc.upsample_rule(8, False, p, pos, nrm, lo_pos, lo_nrm, planes, m, lo_map)
        assert np.array_equal(fell_without, keep), "the fallback is taken exactly where the retrace map asks for a trace"
        assert (fell_without != 0).sum() > 50
        got = api.upsample_soft_light_list(uc.soft_list(8), p, pos, nrm, lo_pos, lo_nrm, planes, m, lo_map, keep, out=before.copy())
        assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def cornell():
    return workload(33, 21)


@pytest.mark.parametrize("phase", uc.PHASES, ids=str)
def test_anchor_end_to_end_equals_the_full_resolution_trace(cornell, phase):
    """Anchor 4 on cornell at 33 x 21 with the host traces: plane_eps = -1 accepts no neighbour, so every active pixel is sampled or
    retraced, and subsample -> trace at w x h -> retrace map -> masked trace at W x H -> upsample with keep equals the plain trace
    byte for byte, for a soft list (no jitter tables) and for a hard one, with the facing map and without a map."""
    wl = cornell
    W, H, k = 33, 21, wl.constants
    p = uc.params(phase, uc.NONE_ACCEPTED)
    w, h = api.subsampled_size(W, H, *phase)
    soft = make_list("mixed")
    hard = soft.hard_list()
    facing = api.facing_lights(k, hard, wl.pos, wl.nrm)
    bg = uc._bg(wl.nrm)
    for fm in (None, facing):
        lo_pos, lo_nrm, lo_map = api.subsample_gbuffer(p, wl.pos, wl.nrm, fm)
        keep = api.upsample_retrace_map(soft.count, p, wl.pos, wl.nrm, lo_pos, lo_nrm, fm, lo_map)
        assert (keep != 0).sum() > W * H // 3
        want = api.soft_light_list(wl.packed, k, soft, wl.pos, W, H, lights_map=fm)
        lo = api.soft_light_list(wl.packed, k, soft, lo_pos, w, h, lights_map=lo_map)
        planes = api.soft_light_list(wl.packed, k, soft, wl.pos, W, H, lights_map=keep)
        got = api.upsample_soft_light_list(soft, p, wl.pos, wl.nrm, lo_pos, lo_nrm, lo, fm, lo_map, keep, out=planes)
        if fm is None:        # the INACTIVE rule gives a background pixel 0; a trace WITHOUT a map traces its cleared texel like any other
            assert bg.sum() > 20 and (got[:, bg] == 0).all()
            want = np.where(bg, 0, want)
        assert np.array_equal(got, want), ("soft", fm is not None)
        assert len(np.unique(want)) > 3
        want = api.light_list(wl.packed, k, hard, wl.pos, W, H, lights_map=fm)
        if fm is None:
            want = np.where(bg, 0, want)
        lo = api.light_list(wl.packed, k, hard, lo_pos, w, h, lights_map=lo_map)
        mask = api.light_list(wl.packed, k, hard, wl.pos, W, H, lights_map=keep)
        got = api.upsample_light_list(hard, p, wl.pos, wl.nrm, lo_pos, lo_nrm, lo, fm, lo_map, keep, out=mask)
        assert np.array_equal(got, want), ("hard", fm is not None)


@pytest.mark.parametrize("phase", uc.PHASES, ids=str)
def test_a_golden_scene_gbuffer_equals_the_rule(cornell, phase):
    """The three passes over cornell's own G-buffer and traced planes at the ordinary thresholds, against the numpy rules."""
    wl = cornell
    W, H, k = 33, 21, wl.constants
    p = uc.params(phase, (0.9, 0.05))
    soft = make_list("mixed")
    facing = api.facing_lights(k, soft.hard_list(), wl.pos, wl.nrm)
    lo_pos, lo_nrm, lo_map = api.subsample_gbuffer(p, wl.pos, wl.nrm, facing)
    lo = api.soft_light_list(wl.packed, k, soft, lo_pos, lo_map.shape[1], lo_map.shape[0], lights_map=lo_map)
    keep = api.upsample_retrace_map(soft.count, p, wl.pos, wl.nrm, lo_pos, lo_nrm, facing, lo_map)
    assert np.array_equal(keep, uc.retrace_rule(soft.count, p, wl.pos, wl.nrm, lo_pos, lo_nrm, facing, lo_map))
    assert 0 < (keep != 0).sum() < W * H // 2
    for kk in (None, keep):
        before = np.full((soft.count, H, W), POISON, np.uint8)
        want, _ = uc.upsample_rule(soft.count, False, p, wl.pos, wl.nrm, lo_pos, lo_nrm, lo, facing, lo_map, kk, before if kk is not None else None)
        got = api.upsample_soft_light_list(soft, p, wl.pos, wl.nrm, lo_pos, lo_nrm, lo, facing, lo_map, kk, out=before.copy())
        assert np.array_equal(got, want)


def test_refusals_write_nothing():
    """Every refusal of the header: RTS_ERR_INVALID_ARG and not a byte of any output."""
    lib, v = api._lib, C.c_void_p
    W, H, phase = 9, 7, (1, 0)
    pos, nrm, m = uc.gbuffer("planes", (W, H))
    lo_pos, lo_nrm, lo_map = low("planes", (W, H), phase, True)
    planes, mask, _ = uc.low_planes((W, H), phase)
    ptr = lambda a: a.ctypes.data_as(v) if a is not None else None
    ref = lambda s: C.byref(s) if s is not None else None
    good = uc.params(phase)
    outs = {n: np.full(s, POISON, t) for n, (s, t) in dict(lp=((H, W, 4), np.float32), ln=((H, W, 4), np.float32), lm=((H, W), np.uint8),
                                                            re=((H, W), np.uint8), so=((8, H, W), np.uint8), ha=((H, W), np.uint8)).items()}
    pristine = {n: a.copy() for n, a in outs.items()}

    def bad_params():
        out = [None]
        for field, value in (("phase_x", 2), ("phase_y", 2), ("phase_x", 0xFFFFFFFF), ("normal_cos_min", np.nan), ("normal_cos_min", np.inf),
                             ("plane_eps", -np.inf), ("plane_eps", np.nan)):
            q = uc.params(phase)
            setattr(q, field, value)
            out.append(q)
        return out

    def sub(p=good, P=pos, N=nrm, M=m, W_=W, H_=H, a="lp", b="ln", c="lm"):
        return lib.rtsh_subsample_gbuffer(ref(p), ptr(P), ptr(N), ptr(M), W_, H_, ptr(outs.get(a)), ptr(outs.get(b)), ptr(outs.get(c)))

    def ret(count=3, p=good, P=pos, N=nrm, LP=lo_pos, LN=lo_nrm, W_=W, H_=H, out="re"):
        return lib.rtsh_upsample_retrace_map(count, ref(p), ptr(P), ptr(N), ptr(m), ptr(LP), ptr(LN), ptr(lo_map), W_, H_, ptr(outs.get(out)), 0)

    def up(form, lst, p=good, P=pos, N=nrm, LP=lo_pos, LN=lo_nrm, LC=True, W_=W, H_=H, out=True, alias=False):
        fn = lib.rtsh_upsample_soft_light_list if form == "soft" else lib.rtsh_upsample_light_list
        lo_c = planes if form == "soft" else mask
        o = outs["so" if form == "soft" else "ha"]
        return fn(ref(lst), ref(p), ptr(P), ptr(N), ptr(m), ptr(LP), ptr(LN), ptr(lo_map), ptr(lo_c if LC else None), None, W_, H_,
                  ptr(o) if alias is False and out else (ptr(lo_c) if alias else None), 0)

    for p in bad_params():
        assert sub(p=p) == INVALID and ret(p=p) == INVALID
    for kw in (dict(P=None), dict(N=None), dict(a=None), dict(b=None), dict(c=None), dict(W_=0), dict(H_=0)):
        assert sub(**kw) == INVALID, kw
    for kw in (dict(count=0), dict(count=9), dict(P=None), dict(N=None), dict(LP=None), dict(LN=None), dict(W_=0), dict(H_=0), dict(out=None)):
        assert ret(**kw) == INVALID, kw
    hard_bad, soft_bad = lc.bad_lists()
    for form, lst, bad in (("soft", uc.soft_list(3), soft_bad), ("hard", uc.hard_list(3), hard_bad)):
        for b in bad:
            assert up(form, b) == INVALID, form
        for p in bad_params():
            assert up(form, lst, p=p) == INVALID, form
        for kw in (dict(P=None), dict(N=None), dict(LP=None), dict(LN=None), dict(LC=False), dict(W_=0), dict(H_=0), dict(out=False),
                   dict(alias=True)):
            assert up(form, lst, **kw) == INVALID, (form, kw)
    # phase 1 on a frame one pixel wide or tall: w or h is 0
    for wh, ph in (((1, 5), (1, 0)), ((5, 1), (0, 1)), ((1, 1), (1, 1))):
        q = uc.params(ph)
        assert sub(p=q, W_=wh[0], H_=wh[1]) == INVALID and ret(p=q, W_=wh[0], H_=wh[1]) == INVALID
        assert up("soft", uc.soft_list(3), p=q, W_=wh[0], H_=wh[1]) == INVALID and up("hard", uc.hard_list(3), p=q, W_=wh[0], H_=wh[1]) == INVALID
        with pytest.raises(api.RtsError):
            api.subsampled_size(wh[0], wh[1], *ph)
    for n, a in outs.items():
        assert np.array_equal(a.view(np.uint8), pristine[n].view(np.uint8)), n
    assert sub() == 0 and ret() == 0 and up("soft", uc.soft_list(3)) == 0 and up("hard", uc.hard_list(3)) == 0      # (the calls were good ones)


def test_on_tiny_frames_under_the_sanitizers(tmp_path):
    """tests/cpp/list_upsample_host.cpp: the host twins (rts_scene.cpp and the shared per-pixel source, compiled into the program --
    nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow over 1 x 1, 1 x 5, 5 x 1, 2 x 2 and
    3 x 3 frames in exact-size heap blocks, in all four phases."""
    exe = str(tmp_path / "list_upsample_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "list_upsample_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100, run.stdout[-2000:]
