"""CPU: the host twins of the wide filters fed from the accumulated mean (rtsh_wide_filter_mean_soft_light_list,
rtsh_wide_filter_guided_temporal_mean_soft_light_list) against the numpy rules of tests/list_mean_filter_cases.py, bit for bit -- and
what pins the rules: every anchor of include/rts_scene.h (anchor 1 against the SHIPPED count-input entry points), the planes that are
never touched, every refusal, and both twins under the address and UB sanitizers (tests/cpp/list_mean_filter_host.cpp, a program of its
own)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import list_combine_cases as lc
import list_mean_filter_cases as mf
import list_wide_guided_cases as gc
from raytracedshadows_amd import api

f32 = np.float32
INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
ref = lambda s: C.byref(s) if s is not None else None


def _unguided(lst, p, pos, nrm, mean, lights_map, threads=0):
    return api.wide_filter_mean_soft_light_list(lst, p, pos, nrm, mean, lights_map, threads)


def _guided(lst, p, pos, nrm, planes, moments, lights_map, threads=0):
    return api.wide_filter_guided_temporal_mean_soft_light_list(lst, p, pos, nrm, planes, moments, lights_map, threads)


@pytest.mark.parametrize("wh", mf.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unguided_twin_equals_the_numpy_rule(wh):
    """Awkward, geometric and (at the wide sizes) flat frames; every list (1, 4 and 8 lights, n_l of 1, 4, 16 and 48 in every entry);
    with the map and without in turn; every kind of mean plane; passes 0 .. 5."""
    for kind in mf.kinds(wh):
        nrm, pos, lights_map = mf.frame(kind, wh)
        for i, (count, rotation) in enumerate(mf.lists()):
            lst = mf.the_list(count, rotation)
            for j, kind_of_mean in enumerate(mf.KINDS_OF_MEAN):
                mean = mf.moments_of(kind_of_mean, kind, wh, lst)[0]
                m = lights_map if (i + j) % 2 == 0 else None
                want = mf.mean_filter_rule(lst, mf.filter_params(0, kind), pos, nrm, mean, m, kind=kind, wh=wh)
                for passes in mf.PASSES:
                    mf.same_bits(_unguided(lst, mf.filter_params(passes, kind), pos, nrm, mean, m), want[passes],
                                 (kind, wh, count, rotation, kind_of_mean, passes))


@pytest.mark.parametrize("wh", mf.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_guided_twin_equals_the_numpy_rule(wh):
    """The same frames and lists; every kind of mean plane at guide_k4 12 and one kind at guide_k4 0, 1, 8 and 255 (the hashed
    kind on a frame at least 40 pixels wide, for the census; else the kinds in turn); min_history 1, 2, 255 in turn; passes 0 .. 5.  On a frame at least 40 pixels wide the rule meets
    list_mean_filter_cases.census_ok with the hashed planes, for every list."""
    for kind in mf.kinds(wh):
        nrm, pos, lights_map = mf.frame(kind, wh)
        for i, (count, rotation) in enumerate(mf.lists()):
            lst = mf.the_list(count, rotation)
            m = lights_map if i % 2 == 0 else None
            for j, k4 in enumerate(mf.K4):
                some = set(mf.KINDS_OF_MEAN) if k4 == 12 else ({"hashed"} if wh[0] >= 40 else {mf.KINDS_OF_MEAN[(i + j) % 4]})
                for kind_of_mean in sorted(some):
                    planes, moments = mf.counts_for(kind_of_mean, wh, lst), mf.moments_of(kind_of_mean, kind, wh, lst)
                    min_history = mf.MIN_HISTORY[(i + j) % 3] if kind_of_mean != "hashed" else 2
                    census = {}
                    p = mf.guide_params(0, k4, min_history, kind)
                    want, _ = mf.guided_mean_rule(lst, p, pos, nrm, planes, moments, m, census=census, kind=kind, wh=wh)
                    if wh[0] >= 40 and kind_of_mean == "hashed":
                        mf.census_ok(lst, census, k4, (kind, wh, count, rotation, k4))
                    for passes in mf.PASSES:
                        p.passes = passes
                        mf.same_bits(_guided(lst, p, pos, nrm, planes, moments, m), want[passes],
                                     (kind, wh, count, rotation, kind_of_mean, k4, min_history, passes))


def test_threads_change_nothing():
    wh = (40, 72)
    nrm, pos, lights_map = mf.frame("geometric", wh)
    lst = mf.the_list(8, 1)
    moments, planes = mf.moments_of("hashed", "geometric", wh, lst), mf.counts(wh, lst)
    for threads in (1, 7):
        mf.same_bits(_unguided(lst, mf.filter_params(3), pos, nrm, moments[0], lights_map, threads),
                     _unguided(lst, mf.filter_params(3), pos, nrm, moments[0], lights_map), ("unguided", threads))
        mf.same_bits(_guided(lst, mf.guide_params(3, 12, 2), pos, nrm, planes, moments, lights_map, threads),
                     _guided(lst, mf.guide_params(3, 12, 2), pos, nrm, planes, moments, lights_map), ("guided", threads))


def test_anchor_1_a_mean_that_is_v0_gives_the_count_input_filters_bits():
    """mean == min(c, n_l) * S_l at every active pixel -- written out, from first-frame moments and from max_length 1 --: both functions
    give the planes of the SHIPPED rtsh_wide_filter_soft_light_list and rtsh_wide_filter_guided_temporal_soft_light_list, whatever square
    and lengths hold."""
    import list_wide_filter_cases as wc
    for kind in ("geometric", "flat", "awkward"):
        wh = (72, 40)
        nrm, pos, lights_map = mf.frame(kind, wh)
        lst = mf.the_list(8, 1)
        planes = mf.counts(wh, lst)
        exact = mf.moments_of("exact", kind, wh, lst)
        tp, delta = mf.overhead_camera(wh, max_length=1)
        first = api.accumulate_moments_soft_light_list(lst, tp, pos, nrm, planes, None, lights_map)
        prev_pos = np.ascontiguousarray(pos, f32).copy()
        with np.errstate(all="ignore"):
            prev_pos[..., :3] += delta
        hashed = mf.moments_of("hashed", kind, wh, lst)
        one = api.accumulate_moments_soft_light_list(lst, tp, pos, nrm, planes, (prev_pos, nrm) + tuple(a for a in hashed), lights_map)
        active = mf._active(lst, nrm, lights_map)
        for moments in (first, one):
            assert (moments[0].astype(np.int64)[active] == mf.v0_of_counts(lst, planes)[active]).all()
        for passes in mf.PASSES:
            shipped = api.wide_filter_soft_light_list(lst, wc.params(passes, kind), pos, nrm, planes, lights_map)
            for name, moments in (("exact", exact), ("first frame", first), ("max_length 1", one)):
                mf.same_bits(_unguided(lst, mf.filter_params(passes, kind), pos, nrm, moments[0], lights_map), shipped,
                             ("unguided", kind, passes, name))
            for k4 in (8, 255):
                for min_history in (2, 255):
                    for name, moments in (("exact", exact), ("first frame", first), ("max_length 1", one)):
                        p = mf.guide_params(passes, k4, min_history, kind)
                        counterpart = api.wide_filter_guided_temporal_soft_light_list(lst, p, pos, nrm, planes, moments, lights_map)
                        mf.same_bits(_guided(lst, p, pos, nrm, planes, moments, lights_map), counterpart,
                                     ("guided", kind, passes, k4, min_history, name))


def test_anchors_2_3_4_and_5():
    """(2) passes == 0: (float)min(mean, n S) / (float)(n S).  (3) A constant plane: that value's quotient after every pass.  (4) RANGE:
    visibility in [0, 1] from planes whose values exceed n S (the rule asserts the range per pass, and the twin equals the rule).
    (5) guide_k4 == 0: the passes == 0 plane for every light of two samples or more; a light of one sample: the unguided mean filter's
    plane; every counted length below min_history and a mean that is V_0: rtsh_wide_filter_guided_soft_light_list's bits."""
    for kind in ("geometric", "flat"):
        wh = (72, 40)
        nrm, pos, lights_map = mf.frame(kind, wh)
        lst = mf.the_list(8, 1)
        planes = mf.counts(wh, lst)
        hashed, constant, exact = (mf.moments_of(k, kind, wh, lst) for k in ("hashed", "constant", "exact"))
        raw = mf.centre_quotient(lst, hashed[0], nrm, lights_map)
        n_l, S_l = mf._nS(lst)
        flat_value = np.where(mf._active(lst, nrm, lights_map), (np.minimum(mf.CONSTANT, n_l * S_l)).astype(f32) / (n_l * S_l).astype(f32),
                              f32(0)).astype(f32)
        assert (hashed[0][:8].astype(np.int64) > n_l * S_l).any()
        short = np.minimum(hashed[2], 2)
        for passes in mf.PASSES:
            fp = mf.filter_params(passes, kind)
            unguided = _unguided(lst, fp, pos, nrm, hashed[0], lights_map)
            assert (unguided >= 0).all() and (unguided <= 1).all()
            mf.same_bits(_unguided(lst, fp, pos, nrm, constant[0], lights_map), flat_value, ("anchor 3, unguided", kind, passes))
            mf.same_bits(_guided(lst, mf.guide_params(passes, 12, 2, kind), pos, nrm, planes, constant, lights_map), flat_value,
                         ("anchor 3, guided", kind, passes))
            a5 = _guided(lst, mf.guide_params(passes, 0, 2, kind), pos, nrm, planes, hashed, lights_map)
            for l, n in enumerate(mf.samples_of(lst)):
                if n >= 2:
                    mf.same_bits(a5[l], raw[l], ("anchor 5, guide_k4 0", kind, passes, l))
            g = _guided(lst, mf.guide_params(passes, 12, 2, kind), pos, nrm, planes, hashed, lights_map)
            assert (g >= 0).all() and (g <= 1).all()
            for l, n in enumerate(mf.samples_of(lst)):
                if n < 2:
                    mf.same_bits(g[l], unguided[l], ("anchor 5, one sample", kind, passes, l))
            shipped = api.wide_filter_guided_soft_light_list(lst, gc.params(passes, 12, kind), pos, nrm, planes, lights_map)
            mf.same_bits(_guided(lst, mf.guide_params(passes, 12, 3, kind), pos, nrm, planes, (exact[0], exact[1], short), lights_map),
                         shipped, ("anchor 5, short history", kind, passes))
        mf.same_bits(_unguided(lst, mf.filter_params(0, kind), pos, nrm, hashed[0], lights_map), raw, ("anchor 2", kind))
        mf.same_bits(_guided(lst, mf.guide_params(0, 12, 2, kind), pos, nrm, planes, hashed, lights_map), raw, ("anchor 2, guided", kind))
        if kind == "flat":                                               # the input does something: it differs from the count-input form
            p = mf.guide_params(3, 12, 2, kind)
            chained, last = mf.moments_of("chained", kind, wh, lst), mf.chained_counts(wh, lst)
            assert (chained[2][:8] > 1).any()                            # the camera did reproject: histories grew
            assert (_guided(lst, p, pos, nrm, last, chained, lights_map) !=
                    api.wide_filter_guided_temporal_soft_light_list(lst, p, pos, nrm, last, chained, lights_map)).any()


def test_planes_from_the_count_up_are_never_touched():
    """Exactly `count` planes of mean, counts, square, lengths and visibility are used; the mean and the moments of a pixel that is not
    counted (background, or the light's map bit clear) and a count byte outside the fallback are never looked at."""
    wh = (17, 15)
    nrm, pos, lights_map = (np.ascontiguousarray(a) for a in mf.frame("geometric", wh))
    lst = mf.the_list(4, 1)
    planes, moments = mf.counts(wh, lst), mf.moments_of("hashed", "geometric", wh, lst)
    p, fp = mf.guide_params(3, 12, 2), mf.filter_params(3)
    want = mf.guided_mean_rule(lst, p, pos, nrm, planes, moments, lights_map)[0][3]
    want_unguided = mf.mean_filter_rule(lst, fp, pos, nrm, moments[0], lights_map)[3]
    four = [np.ascontiguousarray(a[:4]) for a in (planes,) + moments]
    vis = np.full((8, 15, 17), 7.5, f32)
    assert api._lib.rtsh_wide_filter_guided_temporal_mean_soft_light_list(ref(lst), ref(p), ptr(pos), ptr(nrm), ptr(lights_map),
                                                                          *(ptr(a) for a in four), 17, 15, ptr(vis), 0) == 0
    mf.same_bits(vis[:4], want, "guided: planes below the count")
    assert (vis[4:] == 7.5).all()
    vis[:] = 7.5
    assert api._lib.rtsh_wide_filter_mean_soft_light_list(ref(lst), ref(fp), ptr(pos), ptr(nrm), ptr(lights_map), ptr(four[1]), 17, 15,
                                                          ptr(vis), 0) == 0
    mf.same_bits(vis[:4], want_unguided, "unguided: planes below the count")
    assert (vis[4:] == 7.5).all()
    background = (nrm[..., :3] == 0).all(axis=-1)
    poisoned = [a.copy() for a in moments]
    for a in poisoned:
        for l in range(4):
            a[l][(((lights_map >> l) & 1) == 0) | background] ^= 0xFF
    poisoned_counts = planes.copy()
    for l in range(4):
        poisoned_counts[l][(((lights_map >> l) & 1) == 0) | background | (moments[2][l] >= 2)] ^= 0xFF
    mf.same_bits(_guided(lst, p, pos, nrm, poisoned_counts, tuple(poisoned), lights_map), want, "poisoned unread planes")
    mf.same_bits(_unguided(lst, fp, pos, nrm, poisoned[0], lights_map), want_unguided, "poisoned unread mean")


def test_refusals_write_nothing():
    lib = api._lib
    nrm, pos, lights_map = (np.ascontiguousarray(a) for a in mf.frame("geometric", (16, 16)))
    soft = mf.the_list(4, 1)
    planes = np.ascontiguousarray(mf.counts((16, 16), soft))
    moments = [np.ascontiguousarray(a) for a in mf.moments_of("hashed", "geometric", (16, 16), soft)]
    vis = np.full((8, 16, 16), 7.5, f32)
    _, soft_bad = lc.bad_lists()

    def guided(lst=soft, p=mf.guide_params(3, 12, 2), pos_=pos, nrm_=nrm, cnt=planes, mom=moments, W=16, H=16, out=vis):
        return lib.rtsh_wide_filter_guided_temporal_mean_soft_light_list(ref(lst), ref(p), ptr(pos_), ptr(nrm_), ptr(lights_map), ptr(cnt),
                                                                         *(ptr(a) for a in mom), W, H, ptr(out), 0)

    def unguided(lst=soft, p=mf.filter_params(3), pos_=pos, nrm_=nrm, mean=moments[0], W=16, H=16, out=vis):
        return lib.rtsh_wide_filter_mean_soft_light_list(ref(lst), ref(p), ptr(pos_), ptr(nrm_), ptr(lights_map), ptr(mean), W, H, ptr(out), 0)

    def bad(make, fields):
        out = [None]
        for field, value in fields:
            p = make()
            setattr(p, field, value)
            out.append(p)
        return out

    common = [("passes", 6), ("passes", 0xFFFFFFFF), ("normal_cos_min", np.nan), ("normal_cos_min", np.inf), ("plane_eps", -np.inf),
              ("plane_eps", np.nan)]
    assert guided() == 0 and unguided() == 0
    vis[:] = 7.5
    for call in (guided, unguided):
        for b in soft_bad:
            assert call(lst=b) == INVALID
        assert call(pos_=None) == INVALID and call(nrm_=None) == INVALID and call(out=None) == INVALID
        assert call(W=0) == INVALID and call(H=0) == INVALID and call(W=0x7FFFFFF1, H=1) == INVALID and call(W=1, H=0x7FFFFFF1) == INVALID
    for p in bad(lambda: mf.filter_params(3), common):
        assert unguided(p=p) == INVALID
    for p in bad(lambda: mf.guide_params(3, 12, 2), common + [("guide_k4", 256), ("guide_k4", 0xFFFFFFFF), ("min_history", 0),
                                                              ("min_history", 256), ("min_history", 0xFFFFFFFF)]):
        assert guided(p=p) == INVALID
    assert unguided(mean=None) == INVALID and guided(cnt=None) == INVALID
    for i in range(3):
        assert guided(mom=[None if j == i else a for j, a in enumerate(moments)]) == INVALID
    assert (vis == 7.5).all()
    p = mf.guide_params(3, 255, 255)
    p.reserved_[0] = p.reserved_[2] = 0xFFFFFFFF                         # (ignored)
    assert guided(p=p) == 0
    with pytest.raises(api.RtsError):
        api.wide_filter_mean_soft_light_list(soft, mf.filter_params(1), pos, nrm, moments[0][:2])
    with pytest.raises(api.RtsError):
        api.wide_filter_guided_temporal_mean_soft_light_list(soft, mf.guide_params(1, 12, 2), pos, nrm, planes, [a[:2] for a in moments])


def test_list_mean_filter_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/list_mean_filter_host.cpp: both host twins themselves (rts_scene.cpp and the shared per-pixel source, compiled into the
    program -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow, over every refusal and
    small frames with guard bytes behind every output."""
    exe = str(tmp_path / "list_mean_filter_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "list_mean_filter_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 1000, run.stdout[-2000:]
