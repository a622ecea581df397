"""CPU: the host twins of the count moments (rtsh_accumulate_moments_soft_light_list) and of the guided wide filter with a temporal
threshold (rtsh_wide_filter_guided_temporal_soft_light_list) against the numpy rules of tests/list_moments_cases.py, bit for bit -- and
what pins the rules: every anchor of include/rts_scene.h for both stages, the still-camera chain against the integer recurrence, the
threshold function against math.isqrt at G up to 2^42, the planes that are never touched, every refusal, both structs' layouts, the
guided filter's own entry point against its own rule, and both twins under the address and UB sanitizers
(tests/cpp/list_moments_host.cpp, a program of its own)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import list_combine_cases as lc
import list_moments_cases as mc
import list_temporal_cases as tc
import list_wide_guided_cases as gc
from raytracedshadows_amd import api

f32 = np.float32
INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
ref = lambda s: C.byref(s) if s is not None else None


def _moments(lst, c, p=None, with_map=True, first=False, threads=0):
    return api.accumulate_moments_soft_light_list(lst, p or c["params"], c["pos"], c["nrm"], c["counts"], None if first else c["prev"],
                                                  c["map"] if with_map else None, threads)


def _rule(lst, c, p=None, with_map=True, first=False, census=None):
    return mc.moments_rule(lst, p or c["params"], c["pos"], c["nrm"], c["counts"], None if first else c["prev"],
                           c["map"] if with_map else None, census)


# ------------------------------------------------------------------------------------------------------------------ stage 1
@pytest.mark.parametrize("motion", mc.MOTIONS)
@pytest.mark.parametrize("wh", tc.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_twin_equals_the_numpy_rule(wh, motion):
    """The geometric pairs of all four motions; lists of 1, 4 and 8 lights in two rotations, with and without the map; max_length 1, 2,
    5 and 255; reset_lights 0, 0b101 and all ones; the first frame.  On the 40 x 40 pair the rule must have blended a pixel from two
    or more taps and one with a rejected tap (every motion but "away")."""
    for i, (count, rotation) in enumerate([(8, 1), (4, 0), (1, 1), (8, 3)]):
        lst = mc.the_list(count, rotation)
        c = mc.moments_case(motion, wh, lst)
        for j, max_length in enumerate(mc.MAX_LENGTHS):
            for reset in mc.RESETS:
                p = tc.with_params(c["params"], max_length, reset)
                with_map = (i + j) % 2 == 0
                census = {}
                want = _rule(lst, c, p, with_map, census=census)
                if wh[0] >= 40 and max_length > 1 and reset == 0:
                    mc.moments_census_ok(motion, census, (motion, wh, count, max_length))
                mc.same_moments(_moments(lst, c, p, with_map), want, (motion, wh, count, rotation, max_length, reset, with_map))
        mc.same_moments(_moments(lst, c, first=True), _rule(lst, c, first=True), (motion, wh, count, "first frame"))


def test_moments_on_awkward_gbuffers_and_threads():
    """NaN, Inf and huge normals and positions in both frames (list_temporal_cases' awkward pair): the twin equals the rule; and the
    number of threads changes nothing."""
    for wh in ((17, 15), (33, 18)):
        lst = mc.the_list(8, 1)
        a = tc.awkward(wh)
        mean, square = mc.history(wh, lst, 1)
        c = dict(a, counts=gc.counts(wh, lst), prev=(a["prev_pos"], a["prev_nrm"], mean, square, a["prev_len"]))
        mc.same_moments(_moments(lst, c, threads=1), _rule(lst, c), ("awkward", wh))
        mc.same_moments(_moments(lst, c, threads=7), _rule(lst, c), ("awkward, 7 threads", wh))


def test_anchor_1_lengths_are_the_visibility_pass_s_bytes():
    for motion in mc.MOTIONS:
        for wh in ((17, 15), (40, 40)):
            lst = mc.the_list(8, 1)
            c = mc.moments_case(motion, wh, lst)
            for max_length in mc.MAX_LENGTHS:
                for reset in mc.RESETS:
                    p = tc.with_params(c["params"], max_length, reset)
                    got = _moments(lst, c, p)[2]
                    want = api.accumulate_visibility_list(lst.hard_list(), p, c["pos"], c["nrm"], c["vis"],
                                                          (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"]), c["map"])[1]
                    assert (got == want).all(), (motion, wh, max_length, reset)
            assert (_moments(lst, c, first=True)[2] ==
                    api.accumulate_visibility_list(lst.hard_list(), c["params"], c["pos"], c["nrm"], c["vis"], None, c["map"])[1]).all()


def _still(wh):
    """A G-buffer of list_temporal_cases' world and the params of a camera that did not move."""
    W, H = wh
    cam = tc._camera((0.2, 1.4, -1.6), (0.7, 0.1, 0.8), 0.9, W, H)
    nrm, pos = tc._gbuffer(cam, W, H)
    p = api.TemporalParams.make((0, 0, 0), cam["right"], cam["up"], cam["fwd"], cam["scale_x"], cam["scale_y"], 0.9, 1e-3, 4, 0)
    return nrm, pos, p


def test_anchor_2_six_still_frames_equal_the_integer_recurrence():
    """A still camera, max_length 4, six chained frames of changing counts: h_k = (2 * ((n - 1) * h_(k-1) + cur) + n) // (2 * n) with
    n = min(k, 4), per pixel, for both moments; every solid pixel keeps its history (length min(k, 4))."""
    wh = (40, 40)
    nrm, pos, p = _still(wh)
    lst = mc.the_list(4, 1)                                              # n_l = 4, 16, 48, 1
    solid = (nrm[..., :3] != 0).any(axis=-1)
    assert solid.sum() > 500
    n_l = np.array(mc.samples_of(lst), np.int64).reshape(-1, 1, 1)
    rs = np.random.RandomState(11)
    prev, want1, want2 = None, None, None
    for k in range(1, 7):
        counts = rs.randint(0, 50, (4, 40, 40)).astype(np.uint8)
        got = api.accumulate_moments_soft_light_list(lst, p, pos, nrm, counts, prev)
        cur1 = np.minimum(counts.astype(np.int64), n_l) * (65535 // n_l)
        cur2 = cur1 * cur1
        n = min(k, 4)
        if k == 1:
            want1, want2 = cur1, cur2
        else:
            want1 = (2 * ((n - 1) * want1 + cur1) + n) // (2 * n)
            want2 = (2 * ((n - 1) * want2 + cur2) + n) // (2 * n)
        assert (got[2][:, solid] == n).all() and (got[2][:, ~solid] == 0).all(), k
        assert (got[0][:, solid] == want1[:, solid]).all() and (got[1][:, solid] == want2[:, solid]).all(), k
        prev = (pos, nrm) + got


def test_anchor_3_a_constant_history_passes_through_for_any_weights():
    """Where history and current value agree the output is that value whatever the weights: on a moving camera ("turn": four weights)
    with a constant count, prev_mean = V_0 and prev_square = V_0^2 everywhere, the outputs are V_0 and V_0^2 exactly at every active
    pixel -- so square == mean * mean."""
    wh = (40, 40)
    lst = mc.the_list(8, 1)
    c = tc.geometric("turn", wh)
    n_l = np.array(mc.samples_of(lst), np.int64).reshape(-1, 1, 1)
    counts = np.broadcast_to(np.array([3, 7, 29, 1, 0, 16, 48, 0], np.uint8).reshape(-1, 1, 1), (8, 40, 40))
    v0 = np.minimum(counts.astype(np.int64), n_l) * (65535 // n_l)
    prev = (c["prev_pos"], c["prev_nrm"], v0.astype(np.uint16), (v0 * v0).astype(np.uint32), c["prev_len"])
    mean, square, lengths = api.accumulate_moments_soft_light_list(lst, tc.with_params(c["params"], 255, 0), c["pos"], c["nrm"], counts, prev, c["map"])
    active = lengths != 0
    assert (lengths > 1).sum() > 1000
    assert (mean[active] == v0[active]).all() and (square[active] == (v0 * v0)[active]).all()
    assert (square.astype(np.int64) == mean.astype(np.int64) ** 2).all()


def test_anchor_4_nothing_to_blend_gives_the_current_moments():
    lst = mc.the_list(8, 1)
    c = mc.moments_case("subpixel", (33, 18), lst)
    n_l = np.array(mc.samples_of(lst), np.int64).reshape(-1, 1, 1)
    cur1 = np.minimum(c["counts"].astype(np.int64), n_l) * (65535 // n_l)
    bg = (c["nrm"][..., :3] == 0).all(axis=-1)
    on = np.stack([~bg & (((c["map"] >> l) & 1) != 0) for l in range(8)])
    for got in (_moments(lst, c, tc.with_params(c["params"], 1, 0)), _moments(lst, c, tc.with_params(c["params"], 5, 0xFF)),
                _moments(lst, c, first=True)):
        assert (got[0] == np.where(on, cur1, 0)).all() and (got[1] == np.where(on, cur1 * cur1, 0)).all() and (got[2] == on).all()
    partly = _moments(lst, c, tc.with_params(c["params"], 5, 0b101))
    for l in (0, 2):
        assert (partly[0][l] == np.where(on[l], cur1[l], 0)).all() and (partly[2][l] == on[l]).all()
    assert (partly[2][1] > 1).any()


def test_anchor_5_range():
    """Every output lies between the smallest and the largest of its accepted history values and the current one (restated with the
    rule's own taps)."""
    for motion in ("subpixel", "turn"):
        lst = mc.the_list(8, 1)
        c = mc.moments_case(motion, (40, 40), lst)
        p = tc.with_params(c["params"], 255, 0)
        mean, square, lengths = _moments(lst, c, p)
        taps = mc._taps(p, c["pos"], c["nrm"], c["prev_pos"], c["prev_nrm"])[1]
        n_l = mc.samples_of(lst)
        for l in range(8):
            cur1 = np.minimum(c["counts"][l].astype(np.int64), n_l[l]) * (65535 // n_l[l])
            for out, cur, hist in ((mean[l], cur1, c["prev"][2][l]), (square[l], cur1 * cur1, c["prev"][3][l])):
                lo, hi = cur.copy(), cur.copy()
                for geom, w, cy, cx, _ in taps:
                    acc = geom & (c["prev"][4][l][cy, cx] != 0)
                    h = hist[cy, cx].astype(np.int64)
                    lo, hi = np.where(acc, np.minimum(lo, h), lo), np.where(acc, np.maximum(hi, h), hi)
                active = lengths[l] != 0
                assert ((out >= lo) & (out <= hi))[active].all(), (motion, l)


def test_moments_planes_from_the_count_up_are_never_touched():
    lst = mc.the_list(4, 1)
    c = mc.moments_case("turn", (17, 15), lst)
    want = _rule(lst, c)
    n = 17 * 15
    prev = tuple(np.ascontiguousarray(a[:4]) if a.ndim == 3 and a.shape[0] == 8 else np.ascontiguousarray(a) for a in c["prev"])   # exactly four planes
    counts = np.ascontiguousarray(c["counts"][:4])
    mean, square, lengths = np.full((8, 15, 17), 0xABAB, np.uint16), np.full((8, 15, 17), 0xABABABAB, np.uint32), np.full((8, 15, 17), 0xAB, np.uint8)
    assert api._lib.rtsh_accumulate_moments_soft_light_list(ref(lst), ref(c["params"]), ptr(np.ascontiguousarray(c["pos"])),
                                                            ptr(np.ascontiguousarray(c["nrm"])), ptr(np.ascontiguousarray(c["map"])),
                                                            ptr(counts), *(ptr(a) for a in prev), 17, 15, ptr(mean), ptr(square), ptr(lengths), 0) == 0
    mc.same_moments((mean[:4], square[:4], lengths[:4]), want, "planes below the count")
    assert (mean[4:] == 0xABAB).all() and (square[4:] == 0xABABABAB).all() and (lengths[4:] == 0xAB).all() and n


def test_moments_refusals_write_nothing():
    lib = api._lib
    lst = mc.the_list(4, 1)
    c = mc.moments_case("turn", (16, 16), lst)
    pos, nrm, lights_map, counts = (np.ascontiguousarray(c[k]) for k in ("pos", "nrm", "map", "counts"))
    prev = [np.ascontiguousarray(a) for a in c["prev"]]
    outs = [np.full((8, 16, 16), 0xABAB, np.uint16), np.full((8, 16, 16), 0xABABABAB, np.uint32), np.full((8, 16, 16), 0xAB, np.uint8)]
    good = c["params"]
    _, soft_bad = lc.bad_lists()

    def call(lst_=lst, p=good, pos_=pos, nrm_=nrm, cnt=counts, prev_=prev, W=16, H=16, out=outs):
        return lib.rtsh_accumulate_moments_soft_light_list(ref(lst_), ref(p), ptr(pos_), ptr(nrm_), ptr(lights_map), ptr(cnt),
                                                           *(ptr(a) for a in prev_), W, H, *(ptr(a) for a in out), 0)

    def bad_params():
        out = [None]
        for field, value in (("max_length", 0), ("max_length", 256), ("normal_cos_min", np.nan), ("plane_eps", np.inf), ("prev_scale_x", 0.0),
                             ("prev_scale_y", -1.0), ("prev_scale_x", np.nan)):
            p = tc.with_params(good)
            setattr(p, field, value)
            out.append(p)
        for field in ("eye_delta", "prev_right", "prev_up", "prev_fwd"):
            p = tc.with_params(good)
            getattr(p, field)[1] = np.nan
            out.append(p)
        return out

    assert call() == 0
    for a, fill in zip(outs, (0xABAB, 0xABABABAB, 0xAB)):
        a[:] = fill
    for b in soft_bad:
        assert call(lst_=b) == INVALID
    for p in bad_params():
        assert call(p=p) == INVALID
    assert call(pos_=None) == INVALID and call(nrm_=None) == INVALID and call(cnt=None) == INVALID
    for i in range(3):
        assert call(out=[None if j == i else a for j, a in enumerate(outs)]) == INVALID
    for i in range(5):                                                   # some but not all of the five prev_*
        assert call(prev_=[None if j == i else a for j, a in enumerate(prev)]) == INVALID
        assert call(prev_=[a if j == i else None for j, a in enumerate(prev)]) == INVALID
    for i in range(3):                                                   # an output equal to the history it gathers from
        assert call(prev_=prev[:2] + [outs[j] if j == i else prev[2 + j] for j in range(3)]) == INVALID
    assert call(W=0) == INVALID and call(H=0) == INVALID and call(W=65537, H=1) == INVALID and call(W=1, H=65537) == INVALID
    assert (outs[0] == 0xABAB).all() and (outs[1] == 0xABABABAB).all() and (outs[2] == 0xAB).all()
    assert call(prev_=[None] * 5) == 0                                   # the first frame
    with pytest.raises(api.RtsError):
        api.accumulate_moments_soft_light_list(lst, good, pos, nrm, counts[:2], None)


# ------------------------------------------------------------------------------------------------------------------ stage 2
def _filter(lst, p, pos, nrm, planes, moments, lights_map, threads=0):
    return api.wide_filter_guided_temporal_soft_light_list(lst, p, pos, nrm, planes, moments, lights_map, threads)


def _moments_of(wh, lst):
    return mc.history(wh, lst) + (mc.filter_lengths(wh),)


@pytest.mark.parametrize("wh", gc.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_twin_equals_the_numpy_rule(wh):
    """Awkward, geometric and (at the wide sizes) flat frames; lists of 1, 4 and 8 lights with n_l of 1, 4, 16 and 48 in every entry;
    with the map and without in turn; passes 0 .. 5; guide_k4 0, 1, 8, 12, 255; min_history 1, 2, 255 in turn.  On a frame at least 40
    pixels wide the rule meets the census of list_moments_cases.filter_census_ok."""
    for kind in gc.kinds(wh):
        nrm, pos, lights_map = gc.frame(kind, wh)
        for i, (count, rotation) in enumerate(gc.lists()):
            lst = mc.the_list(count, rotation)
            planes, moments = gc.counts(wh, lst), _moments_of(wh, lst)
            m = lights_map if i % 2 == 0 else None
            for j, k4 in enumerate(gc.K4):
                for min_history in (mc.MIN_HISTORY if wh[0] >= 40 and count == 8 and k4 == 12 else [mc.MIN_HISTORY[(i + j) % 3]]):
                    census = {}
                    p = mc.params(0, k4, min_history, kind)
                    want = mc.guided_temporal_rule(lst, p, pos, nrm, planes, moments, m, census=census, kind=kind, wh=wh)
                    if wh[0] >= 40:
                        mc.filter_census_ok(lst, census, k4, (kind, wh, count, rotation, k4, min_history))
                    for passes in gc.PASSES:
                        p.passes = passes
                        gc.same_bits(_filter(lst, p, pos, nrm, planes, moments, m), want[passes],
                                     (kind, wh, count, rotation, i % 2 == 0, k4, min_history, passes))


def test_filter_anchor_1_a_short_history_gives_the_guided_filter_s_bits():
    """Every counted length below min_history: bit for bit rtsh_wide_filter_guided_soft_light_list, whatever mean and square hold; and
    that entry point itself still equals ITS rule (list_wide_guided_cases.guided_rule), the plane its parent commit gave."""
    for kind in ("geometric", "flat"):
        wh = (72, 40)
        nrm, pos, lights_map = gc.frame(kind, wh)
        lst = mc.the_list(8, 1)
        planes = gc.counts(wh, lst)
        mean, square = mc.history(wh, lst)
        short = np.minimum(mc.filter_lengths(wh), 2)
        for k4 in (8, 255):
            recorded = gc.guided_rule(lst, gc.params(0, k4, kind), pos, nrm, planes, lights_map, kind=kind, wh=wh)
            for passes in gc.PASSES:
                parent = api.wide_filter_guided_soft_light_list(lst, gc.params(passes, k4, kind), pos, nrm, planes, lights_map)
                gc.same_bits(parent, recorded[passes], ("the guided filter's own bits", kind, k4, passes))
                for min_history, lengths in ((3, short), (255, np.minimum(mc.filter_lengths(wh), 254)), (1, np.zeros_like(short))):
                    got = _filter(lst, mc.params(passes, k4, min_history, kind), pos, nrm, planes, (mean, square, lengths), lights_map)
                    gc.same_bits(got, parent, (kind, k4, passes, min_history))


def test_filter_anchors_2_3_4_and_5():
    """(2) First-frame moments with min_history 1: the passes == 0 plane for every light of two samples or more.  (3) guide_k4 == 0:
    the same.  (4) A light of one sample: the unguided filter's plane.  (5) visibility stays in [0, 1] (the rule asserts RANGE per
    pass, and the twin equals the rule)."""
    import list_wide_filter_cases as wc
    for kind in ("geometric", "flat"):
        wh = (72, 40)
        nrm, pos, lights_map = gc.frame(kind, wh)
        lst = mc.the_list(8, 1)
        planes = gc.counts(wh, lst)
        raw = gc.centre_quotient(lst, planes, nrm, lights_map)
        tp = api.TemporalParams.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, -1), 1.0, 1.0)
        first = api.accumulate_moments_soft_light_list(lst, tp, pos, nrm, planes, None, lights_map)
        assert (first[1].astype(np.int64) == first[0].astype(np.int64) ** 2).all()
        awkward = _moments_of(wh, lst)
        for passes in gc.PASSES:
            unguided = api.wide_filter_soft_light_list(lst, wc.params(passes, kind), pos, nrm, planes, lights_map)
            a2 = _filter(lst, mc.params(passes, 255, 1, kind), pos, nrm, planes, first, lights_map)
            a3 = _filter(lst, mc.params(passes, 0, 2, kind), pos, nrm, planes, awkward, lights_map)
            a4 = _filter(lst, mc.params(passes, 12, 2, kind), pos, nrm, planes, awkward, lights_map)
            assert (a4 >= 0).all() and (a4 <= 1).all()
            for l, n in enumerate(mc.samples_of(lst)):
                if n >= 2:
                    gc.same_bits(a2[l], raw[l], ("anchor 2", kind, passes, l))
                    gc.same_bits(a3[l], raw[l], ("anchor 3", kind, passes, l))
                else:
                    for got in (a2, a3, a4):
                        gc.same_bits(got[l], unguided[l], ("anchor 4", kind, passes, l))
        if kind == "flat":                                               # the temporal guide does something: it differs from 4.26's
            guided = api.wide_filter_guided_soft_light_list(lst, gc.params(3, 12, kind), pos, nrm, planes, lights_map)
            assert (_filter(lst, mc.params(3, 12, 2, kind), pos, nrm, planes, awkward, lights_map) != guided).any()


def test_threshold_function_equals_isqrt_up_to_two_to_the_42():
    """rtsh_wide_guide_threshold -- unchanged, and what the temporal threshold evaluates -- against min(65535, isqrt(k4^2 * G // (16 * D
    * n))) at the new extremes: G up to 2^42, D 4 and 16, n 2 and 48, guide_k4 1 and 255, and around perfect squares of the quotient."""
    want = lambda G, D, n, k4: min(65535, math.isqrt((k4 * k4 * G) // (16 * D * n)))
    rs = np.random.RandomState(9)
    checked = 0
    for n in (2, 48):
        for D in (4, 16):
            for k4 in (1, 255):
                d = 16 * D * n
                values = {0, 1, (1 << 42) - 1, 1 << 41, (1 << 35) - 1, 1 << 35, 16 * 48 * ((1 << 32) - 1), D * n * ((1 << 32) - 1)}
                values.update(int(a) * int(b) for a, b in zip(rs.randint(0, 1 << 21, 40), rs.randint(0, 1 << 21, 40)))
                for r in (1, 2, 255, 4095, 32768, 65534, 65535, 65536, int(rs.randint(1, 65536)), int(rs.randint(1, 65536))):
                    g = -(-(r * r * d) // (k4 * k4))                      # the smallest G whose quotient reaches r * r
                    values.update(v for v in (g - 1, g, g + 1) if 0 <= v < 1 << 42)
                for G in values:
                    assert G < 1 << 42
                    assert api.wide_guide_threshold(G, D, n, k4) == want(G, D, n, k4), (G, D, n, k4)
                    checked += 1
    assert checked > 400
    assert api.wide_guide_threshold((1 << 42) - 1, 4, 2, 255) == 65535 and api.wide_guide_threshold((1 << 42) - 1, 16, 48, 1) == want((1 << 42) - 1, 16, 48, 1)


def test_filter_planes_from_the_count_up_are_never_touched():
    """Exactly `count` planes of counts, mean, square, lengths and visibility are used; the moments of a pixel that is not counted
    (background, or the light's map bit clear) are never looked at."""
    wh = (17, 15)
    nrm, pos, lights_map = gc.frame("geometric", wh)
    lst = mc.the_list(4, 1)
    planes, moments = gc.counts(wh, lst), _moments_of(wh, lst)
    p = mc.params(3, 12, 2)
    want = mc.guided_temporal_rule(lst, p, pos, nrm, planes, moments, lights_map)[3]
    four = [np.ascontiguousarray(a[:4]) for a in (planes,) + moments]
    vis = np.full((8, 15, 17), 7.5, f32)
    assert api._lib.rtsh_wide_filter_guided_temporal_soft_light_list(ref(lst), ref(p), ptr(np.ascontiguousarray(pos)), ptr(np.ascontiguousarray(nrm)),
                                                                     ptr(np.ascontiguousarray(lights_map)), *(ptr(a) for a in four), 17, 15,
                                                                     ptr(vis), 0) == 0
    gc.same_bits(vis[:4], want, "planes below the count")
    assert (vis[4:] == 7.5).all()
    background = (nrm[..., :3] == 0).all(axis=-1)
    poisoned = [a.copy() for a in moments]
    for a in poisoned:
        for l in range(4):
            a[l][(((lights_map >> l) & 1) == 0) | background] ^= 0xFF
    gc.same_bits(_filter(lst, p, pos, nrm, planes, tuple(poisoned), lights_map), want, "poisoned unread moments")


def test_filter_refusals_write_nothing():
    lib = api._lib
    nrm, pos, lights_map = (np.ascontiguousarray(a) for a in gc.frame("geometric", (16, 16)))
    soft = mc.the_list(4, 1)
    planes = np.ascontiguousarray(gc.counts((16, 16), soft))
    moments = [np.ascontiguousarray(a) for a in _moments_of((16, 16), soft)]
    vis = np.full((8, 16, 16), 7.5, f32)
    good = mc.params(3, 12, 2)
    _, soft_bad = lc.bad_lists()

    def call(lst=soft, p=good, pos_=pos, nrm_=nrm, cnt=planes, mom=moments, W=16, H=16, out=vis):
        return lib.rtsh_wide_filter_guided_temporal_soft_light_list(ref(lst), ref(p), ptr(pos_), ptr(nrm_), ptr(lights_map), ptr(cnt),
                                                                    *(ptr(a) for a in mom), W, H, ptr(out), 0)

    def bad_params():
        out = [None]
        for field, value in (("passes", 6), ("passes", 0xFFFFFFFF), ("normal_cos_min", np.nan), ("normal_cos_min", np.inf),
                             ("plane_eps", -np.inf), ("plane_eps", np.nan), ("guide_k4", 256), ("guide_k4", 0xFFFFFFFF),
                             ("min_history", 0), ("min_history", 256), ("min_history", 0xFFFFFFFF)):
            p = mc.params(3, 12, 2)
            setattr(p, field, value)
            out.append(p)
        return out

    assert call() == 0
    vis[:] = 7.5
    for b in soft_bad:
        assert call(lst=b) == INVALID
    for p in bad_params():
        assert call(p=p) == INVALID
    assert call(pos_=None) == INVALID and call(nrm_=None) == INVALID and call(cnt=None) == INVALID and call(out=None) == INVALID
    for i in range(3):
        assert call(mom=[None if j == i else a for j, a in enumerate(moments)]) == INVALID
    assert call(W=0) == INVALID and call(H=0) == INVALID and call(W=0x7FFFFFF1, H=1) == INVALID and call(W=1, H=0x7FFFFFF1) == INVALID
    assert (vis == 7.5).all()
    p = mc.params(3, 255, 255)
    p.reserved_[0] = p.reserved_[2] = 0xFFFFFFFF                         # (ignored)
    assert call(p=p) == 0


def test_struct_layouts_are_what_the_compiler_lays_out(tmp_path):
    """rtsh_wide_guide_temporal_params is 32 bytes and rtsh_temporal_params 80, and gcc lays out their fields where the ctypes mirrors
    have them."""
    assert C.sizeof(api.WideGuideTemporalParams) == 32 and C.sizeof(api.TemporalParams) == 80
    body = ""
    for name, mirror in (("rtsh_wide_guide_temporal_params", api.WideGuideTemporalParams), ("rtsh_temporal_params", api.TemporalParams)):
        body += f'  printf("%zu", sizeof({name}));\n'
        body += "".join(f'  printf(" %zu", offsetof({name}, {f}));\n' for f, _ in mirror._fields_) + '  printf("\\n");\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rts_scene.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (size, mirror) in zip(lines, ((32, api.WideGuideTemporalParams), (80, api.TemporalParams))):
        got = [int(v) for v in line.split()]
        assert got[0] == size and got[1:] == [getattr(mirror, f).offset for f, _ in mirror._fields_]


def test_list_moments_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/list_moments_host.cpp: both host twins themselves (rts_scene.cpp and the shared per-pixel source, compiled into the
    program -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow, over every refusal and
    small frames with guard bytes behind every output."""
    exe = str(tmp_path / "list_moments_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "list_moments_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 1000, run.stdout[-2000:]
