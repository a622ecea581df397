"""The clamped forms of the moments pass on the host (include/rts_scene.h's last section):
rtsh_accumulate_moments_soft_light_list_clamped and ..._clamped_motion against the numpy rule of tests/list_moments_clamp_cases.py bit
for bit over every frame of list_temporal_cases.FRAMES, every kind, 1, 3 and 8 lights and a walk through radius 0..4 x sigma_k4
{0, 8, 36, 255} x margin {0, 1, 65535}; the census; the six anchors of the header; rtsh_moments_clamp_bounds against a big-integer
restatement at its extremes; every refusal with canaries; the struct's layout.  No GPU.  The twins run under the sanitizers in
tests/cpp/list_moments_clamp_host.cpp."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import list_combine_cases as lc
import list_moments_cases as mc
import list_moments_clamp_cases as cc
import list_motion_edge_cases as ec
import list_temporal_cases as tc
from raytracedshadows_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
f32 = np.float32
ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
ref = lambda s: C.byref(s) if s is not None else None


def twin(lst, p, c, clamp, with_map=True, motion=None, first=False, threads=0):
    return api.accumulate_moments_soft_light_list(lst, p, c["pos"], c["nrm"], c["counts"], None if first else c["prev"],
                                                  c["map"] if with_map else None, threads, motion=motion,
                                                  clamp=None if clamp is None else api.MomentsClamp.make(*clamp))


def rule(lst, p, c, clamp, with_map=True, motion=None, first=False):
    lights_map = c["map"] if with_map else None
    prev = None if first else c["prev"]
    if motion is not None:
        return cc.clamped_motion_rule(lst, p, c["nrm"], c["counts"], prev, lights_map, motion, clamp)
    return cc.clamped_rule(lst, p, c["pos"], c["nrm"], c["counts"], prev, lights_map, clamp)


# ------------------------------------------------------------------------------------------------------------ twin == rule
def test_fifteen_runs_walk_the_whole_grid():
    seen = {s for run in range(15) for s in cc.selections(run)}
    assert seen == set(cc.GRID) and len(cc.GRID) == 60


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("wh", tc.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_clamped_twins_equal_the_numpy_rule(wh, kind):
    """Per frame: five kinds x three lists = fifteen runs, four selections each: all sixty; with and without a map; plain and motion;
    max_length and reset_lights in turn."""
    fi, ki = tc.FRAMES.index(wh), tc.KINDS.index(kind)
    for ci, count in enumerate((1, 3, 8)):
        run = ki * 3 + ci
        lst = mc.the_list(count, run % 4)
        c = cc.case(kind, wh, lst)
        motion = ec.motion_planes(c, wh, run % 8)
        for j, clamp in enumerate(cc.selections(run)):
            p = tc.with_params(c["params"], mc.MAX_LENGTHS[(run + j + fi) % 4], mc.RESETS[(run + 2 * j) % 3])
            with_map = (run + j + fi) % 2 == 0
            mc.same_moments(twin(lst, p, c, clamp, with_map), rule(lst, p, c, clamp, with_map), (wh, kind, count, clamp, "plain"))
            if j % 2 == 0:
                mc.same_moments(twin(lst, p, c, clamp, with_map, motion), rule(lst, p, c, clamp, with_map, motion),
                                (wh, kind, count, clamp, "motion"))


def test_the_stale_history_and_threads():
    """The history a moved shadow leaves, every radius, sigma_k4 8 and 36, on the 40 x 40 and 33 x 18 pairs; one thread and three agree."""
    lst = mc.the_list(8, 1)
    for wh in ((40, 40), (33, 18)):
        c = cc.stale_case("turn", wh, lst)
        p = tc.with_params(c["params"], 32, 0b100)
        for r in cc.RADII:
            for k4 in (8, 36):
                want = rule(lst, p, c, (r, k4, 0))
                mc.same_moments(twin(lst, p, c, (r, k4, 0), threads=1), want, (wh, r, k4, "one thread"))
                mc.same_moments(twin(lst, p, c, (r, k4, 0), threads=3), want, (wh, r, k4, "three threads"))


@pytest.mark.parametrize("radius", (1, 4))
def test_census_of_the_40_x_40_pair(radius):
    """From the numpy rule alone: blended pairs clamped from above, from below and left alone, windows cut by the frame, windows with a
    tap that does not contribute, and at sigma_k4 8 pairs where the sigma bound and not the range binds: 20 or more of each."""
    out = cc.census(radius, 8)
    for what in ("above", "below", "alone", "cut", "hole", "sigma"):
        assert out[what] >= 20, (radius, what, out)
    wide = cc.census(radius, 36)
    assert wide["sigma"] == 0 and wide["above"] >= 20 and wide["below"] >= 20, (radius, wide)


# ------------------------------------------------------------------------------------------------------------ the anchors
def _pairs():
    lst = mc.the_list(8, 1)
    return lst, [cc.case(kind, (40, 40), lst) for kind in ("pixels", "turn")] + [cc.stale_case("subpixel", (33, 18), lst)]


def test_anchor_1_margin_65535_is_the_unclamped_pass():
    """Over histories whose squares are at most 65535^2 -- every plane the pass itself wrote is (RANGE) --; list_moments_cases' awkward
    squares above that (2^32 - 1) are cut to it here: the box of margin 65535 is [0, 65535] and its square side ends at 65535^2."""
    lst, cases = _pairs()
    for c in cases:
        prev = c["prev"]
        c = dict(c, prev=prev[:3] + (np.minimum(prev[3], np.uint32(65535 * 65535)),) + prev[4:])
        motion = ec.motion_planes(c, c["nrm"].shape[1::-1])
        for r in cc.RADII:
            for k4 in cc.SIGMA_K4:
                for m in (None, motion):
                    want = twin(lst, c["params"], c, None, motion=m)
                    mc.same_moments(twin(lst, c["params"], c, (r, k4, 65535), motion=m), want, (r, k4, m is not None))
        # ... and the unedited numpy rule of the unclamped pass says the same
        mc.same_moments(twin(lst, c["params"], c, (2, 8, 65535)),
                        mc.moments_rule(lst, c["params"], c["pos"], c["nrm"], c["counts"], c["prev"], c["map"]), "the unclamped rule")


def test_anchor_2_radius_0_gives_the_current_moments_at_blended_pairs():
    lst, cases = _pairs()
    n_l = np.array(mc.samples_of(lst), np.int64).reshape(-1, 1, 1)
    for c in cases:
        for k4 in cc.SIGMA_K4:
            p = tc.with_params(c["params"], 32, 0)
            mean, square, lengths = twin(lst, p, c, (0, k4, 0))
            plain = twin(lst, p, c, None)
            cur1 = np.minimum(c["counts"][:8].astype(np.int64), n_l) * (65535 // n_l)
            blended = plain[2] > 1
            assert blended.sum() > 1000 and (plain[0][blended] != cur1[blended]).any()
            assert (mean[blended] == cur1[blended]).all() and (square[blended] == (cur1 * cur1)[blended]).all()
            assert (lengths == plain[2]).all()


def test_anchor_3_pass_through_and_inactive_pairs_are_the_unclamped_bits():
    lst, cases = _pairs()
    for c in cases:
        motion = ec.motion_planes(c, c["nrm"].shape[1::-1])
        for clamp in ((1, 8, 0), (4, 0, 0)):
            for p, first in ((tc.with_params(c["params"], 1, 0), False), (tc.with_params(c["params"], 5, 0xFF), False), (c["params"], True)):
                for m in (None, motion):
                    mc.same_moments(twin(lst, p, c, clamp, motion=m, first=first), twin(lst, p, c, None, motion=m, first=first),
                                    (clamp, p.max_length, p.reset_lights, first))
            # a reset light in the middle of the list, and every pair that does not blend
            p = tc.with_params(c["params"], 5, 0b1000)
            got, plain = twin(lst, p, c, clamp), twin(lst, p, c, None)
            mc.same_moments(tuple(a[3:4] for a in got), tuple(a[3:4] for a in plain), "the reset light")
            rest = plain[2] <= 1
            assert rest.any() and all((g[rest] == w[rest]).all() for g, w in zip(got, plain))
            assert (got[2] == plain[2]).all(), "the clamp shortens no history"


def test_anchor_4_the_step():
    """History mean 65535 and square 65535^2 of any length, current counts all 0, a still camera, margin 0: 0 and 0 exactly at any
    radius, sigma_k4 and max_length, where the unclamped pass gives round(65535 (n - 1) / n)."""
    W, H = 24, 20
    lst = mc.the_list(4, 0)
    cam = tc._camera((0.6, 1.5, 1.1), (0.6, 0.0, 1.1), 2.0 * np.arctan(1.0 / 1.5), W, H)
    nrm, pos = tc._gbuffer(cam, W, H)
    p = api.TemporalParams.make((0, 0, 0), cam["right"], cam["up"], cam["fwd"], cam["scale_x"], cam["scale_y"], 0.9, 0.02, 32, 0)
    lengths = tc.lengths((W, H), 2)[[1, 2, 3, 5, 6, 7, 1, 2]]
    lengths = np.where(lengths == 0, 1, lengths).astype(np.uint8)
    prev = (pos, nrm, np.full((8, H, W), 65535, np.uint16), np.full((8, H, W), 65535 * 65535, np.uint32), lengths)
    c = dict(pos=pos, nrm=nrm, counts=np.zeros((8, H, W), np.uint8), prev=prev, map=None)
    active = ~(nrm[..., :3] == 0).all(-1)
    assert active.sum() > 300
    for max_length in (2, 5, 32, 255):
        q = tc.with_params(p, max_length, 0)
        plain = twin(lst, q, c, None, with_map=False)
        n = np.minimum(lengths[:4].astype(np.int64) + 1, max_length)
        assert (plain[2][:, active] == n[:, active]).all(), "a still camera keeps every history"
        assert (plain[0][:, active] == ((2 * 65535 * (n - 1) + n) // (2 * n))[:, active]).all()
        for r in cc.RADII:
            for k4 in cc.SIGMA_K4:
                mean, square, got_len = twin(lst, q, c, (r, k4, 0), with_map=False)
                assert (mean == 0).all() and (square == 0).all() and (got_len == plain[2]).all(), (max_length, r, k4)


def test_anchor_5_sigma_k4_36_is_the_range_box_alone():
    lst, cases = _pairs()
    for c in cases:
        motion = ec.motion_planes(c, c["nrm"].shape[1::-1])
        p = tc.with_params(c["params"], 32, 0)
        for r in cc.RADII:
            for margin in (0, 1):
                for m in (None, motion):
                    a, b = twin(lst, p, c, (r, 36, margin), motion=m), twin(lst, p, c, (r, 255, margin), motion=m)
                    mc.same_moments(a, b, (r, margin, "36 == 255"))
        assert any((x != y).any() for x, y in zip(twin(lst, p, c, (4, 8, 0)), twin(lst, p, c, (4, 36, 0)))), "sigma_k4 8 never bound"


def test_anchor_6_range():
    lst, cases = _pairs()
    n_l = np.array(mc.samples_of(lst), np.int64).reshape(-1, 1, 1)
    for c in cases:
        p = tc.with_params(c["params"], 32, 0)
        cur1 = np.minimum(c["counts"][:8].astype(np.int64), n_l) * (65535 // n_l)
        for clamp in ((1, 8, 0), (4, 4, 3), (2, 36, 0)):
            mean, square, lengths = (a.astype(np.int64) for a in twin(lst, p, c, clamp))
            on, m, S1, S2, lo, hi, _ = cc.window_rule(lst, c["nrm"], c["counts"], c["map"], clamp[0])
            blended = lengths > 1
            Lv, Hv = cc.bounds_rule(np.where(blended, m, 1), np.where(blended, S1, 0), np.where(blended, S2, 0), np.where(blended, lo, 0),
                                    np.where(blended, hi, 0), clamp[1], clamp[2])
            assert ((mean >= np.minimum(Lv, cur1)) & (mean <= np.maximum(Hv, cur1)))[blended].all()
            assert ((square >= np.minimum(Lv * Lv, cur1 * cur1)) & (square <= np.maximum(Hv * Hv, cur1 * cur1)))[blended].all()


# ------------------------------------------------------------------------------------------------------------ the bounds function
def big_bounds(m, S1, S2, lo, hi, k4, margin):
    """The header's BOX in Python integers."""
    D = m * S2 - S1 * S1
    x = k4 * k4 * D
    R = math.isqrt(x)
    R += 1 if R * R < x else 0
    Rc = (R + 3) // 4
    A, B = max(S1 - Rc, 0), S1 + Rc
    Lm, Hm = max(m * lo, A), min(m * hi, B)
    return max(Lm // m - margin, 0), min(65535, (Hm + m - 1) // m + margin)


def test_bounds_function_at_its_extremes():
    windows = []
    for m in (1, 2, 9, 25, 80, 81):
        windows += [[0] * m, [65535] * m, [0] * (m // 2) + [65535] * (m - m // 2), [65535] + [0] * (m - 1), [0] + [65535] * (m - 1),
                    [30000] * (m - 1) + [30001], list(range(100, 100 + m)), [(i * 40503) % 65536 for i in range(m)]]
    checked = 0
    for v in windows:
        m, S1, S2, lo, hi = len(v), sum(v), sum(a * a for a in v), min(v), max(v)
        for k4 in (0, 1, 4, 8, 35, 36, 255):
            for margin in (0, 1, 65535):
                want = big_bounds(m, S1, S2, lo, hi, k4, margin)
                assert api.moments_clamp_bounds(m, S1, S2, lo, hi, k4, margin) == want, (v[:4], m, k4, margin)
                checked += 1
            L, Hh = big_bounds(m, S1, S2, lo, hi, k4, 0)
            assert lo <= L <= Hh <= hi and (k4 < 36 or (L, Hh) == (lo, hi)) and (k4 != 0 or Hh - L <= 1), (v[:4], k4)
    # x around perfect squares: S1 = 0 makes D = m S2, so x = k4^2 m S2 is chosen freely; R must be the exact ceiling of its root
    for root in (1, 2, 3, 1000, 65535, 65536, (1 << 19) + 7, 11863283):
        for d in (-1, 0, 1):
            S2 = root * root + d
            if not 0 < S2 < 1 << 39:
                continue
            for m, k4 in ((1, 1), (1, 4), (81, 255), (7, 3)):
                want = big_bounds(m, 0, S2, 0, 65535, k4, 0)
                assert api.moments_clamp_bounds(m, 0, S2, 0, 65535, k4, 0) == want, (root, d, m, k4)
                checked += 1
    # x at its largest inside the widths
    assert api.moments_clamp_bounds(81, 0, (1 << 39) - 1, 0, 65535, 255, 0) == big_bounds(81, 0, (1 << 39) - 1, 0, 65535, 255, 0)
    # outside the widths: no box
    for args in ((0, 0, 0, 0, 0, 8, 0), (82, 0, 0, 0, 0, 8, 0), (1, 5, 25, 5, 5, 256, 0), (1, 5, 25, 6, 5, 8, 0), (1, 5, 25, 5, 65536, 8, 0),
                 (2, 10, 49, 5, 5, 8, 0), (1, 1 << 23, 1 << 38, 0, 65535, 8, 0), (1, 0, 1 << 39, 0, 65535, 8, 0)):
        assert api.moments_clamp_bounds(*args) == (0, 65535), args
    assert checked > 1000


def test_bounds_function_over_random_windows():
    rs = np.random.RandomState(35)
    for _ in range(3000):
        m = int(rs.randint(1, 82))
        kind = rs.randint(0, 4)
        v = rs.randint(0, 65536, m) if kind == 0 else rs.choice([0, 65535], m) if kind == 1 else \
            np.clip(rs.randint(0, 65536) + rs.randint(-40, 41, m), 0, 65535) if kind == 2 else rs.choice([0, 21845, 43690, 65535], m)
        v = [int(a) for a in v]
        k4, margin = int(rs.choice([0, 1, 4, 8, 12, 36, 255])), int(rs.choice([0, 0, 1, 300]))
        args = (m, sum(v), sum(a * a for a in v), min(v), max(v), k4, margin)
        assert api.moments_clamp_bounds(*args) == big_bounds(*args), args


# ------------------------------------------------------------------------------------------------------------ refusals, layout
def test_planes_from_the_count_up_are_never_touched_or_read():
    lst = mc.the_list(3, 1)
    c = cc.case("turn", (17, 15), lst)
    base = twin(lst, c["params"], c, (4, 8, 0))
    other = dict(c, counts=np.ascontiguousarray(np.where(np.arange(8).reshape(8, 1, 1) >= 3, 7, c["counts"]).astype(np.uint8)))
    mc.same_moments(twin(lst, c["params"], other, (4, 8, 0)), base, "count planes from the count up")
    assert all(a.shape[0] == 3 for a in base)


@pytest.mark.parametrize("form", ("plain", "motion"))
def test_refusals_write_nothing(form):
    lib = api._lib
    lst = mc.the_list(4, 1)
    c = mc.moments_case("turn", (16, 16), lst)
    pos, nrm, lights_map, counts = (np.ascontiguousarray(c[k]) for k in ("pos", "nrm", "map", "counts"))
    prev = [np.ascontiguousarray(a) for a in c["prev"]]
    mot = [np.ascontiguousarray(a) for a in ec.motion_planes(c, (16, 16))]
    outs = [np.full((8, 16, 16), 0xABAB, np.uint16), np.full((8, 16, 16), 0xABABABAB, np.uint32), np.full((8, 16, 16), 0xAB, np.uint8)]
    good, clamp = c["params"], api.MomentsClamp.make(2, 8, 0)
    _, soft_bad = lc.bad_lists()

    def call(lst_=lst, p=good, pos_=pos, nrm_=nrm, cnt=counts, prev_=prev, mot_=mot, W=16, H=16, out=outs, clamp_=clamp):
        if form == "motion":
            return lib.rtsh_accumulate_moments_soft_light_list_clamped_motion(
                ref(lst_), ref(p), ptr(pos_), ptr(nrm_), ptr(lights_map), ptr(cnt), *(ptr(a) for a in prev_), *(ptr(a) for a in mot_), W, H,
                *(ptr(a) for a in out), ref(clamp_), 0)
        return lib.rtsh_accumulate_moments_soft_light_list_clamped(ref(lst_), ref(p), ptr(pos_), ptr(nrm_), ptr(lights_map), ptr(cnt),
                                                                   *(ptr(a) for a in prev_), W, H, *(ptr(a) for a in out), ref(clamp_), 0)

    assert call() == 0
    assert (outs[0][:4] != 0xABAB).any()
    for a, fill in zip(outs, (0xABAB, 0xABABABAB, 0xAB)):
        a[:] = fill
    # the clamp's own
    assert call(clamp_=None) == INVALID
    for field, value in (("radius", 5), ("radius", 0xFFFFFFFF), ("sigma_k4", 256), ("margin", 65536), ("margin", 0xFFFFFFFF)):
        bad = api.MomentsClamp.make(2, 8, 0)
        setattr(bad, field, value)
        assert call(clamp_=bad) == INVALID, (field, value)
    # everything the unclamped form refuses
    for b in soft_bad:
        assert call(lst_=b) == INVALID
    for field, value in (("max_length", 0), ("max_length", 256), ("normal_cos_min", np.nan), ("plane_eps", np.inf), ("prev_scale_x", 0.0),
                         ("prev_scale_y", -1.0)):
        p = tc.with_params(good)
        setattr(p, field, value)
        assert call(p=p) == INVALID
    for field in ("eye_delta", "prev_right", "prev_up", "prev_fwd"):
        p = tc.with_params(good)
        getattr(p, field)[1] = np.nan
        assert call(p=p) == INVALID
    assert call(p=None) == INVALID and call(nrm_=None) == INVALID and call(cnt=None) == INVALID
    if form == "plain":
        assert call(pos_=None) == INVALID
    for i in range(3):
        assert call(out=[None if j == i else a for j, a in enumerate(outs)]) == INVALID
        assert call(prev_=prev[:2] + [outs[j] if j == i else prev[2 + j] for j in range(3)]) == INVALID
    for i in range(5):
        assert call(prev_=[None if j == i else a for j, a in enumerate(prev)]) == INVALID
    assert call(W=0) == INVALID and call(H=0) == INVALID and call(W=65537, H=1) == INVALID and call(W=1, H=65537) == INVALID
    if form == "motion":
        assert call(mot_=[None, mot[1]]) == INVALID and call(mot_=[mot[0], None]) == INVALID
    assert (outs[0] == 0xABAB).all() and (outs[1] == 0xABABABAB).all() and (outs[2] == 0xAB).all()
    reserved = api.MomentsClamp.make(2, 8, 0)
    reserved.reserved_ = 0xDEADBEEF                                        # ignored
    assert call(clamp_=reserved) == 0
    assert call(prev_=[None] * 5, mot_=[None, None]) == 0                  # the first frame reads neither motion plane
    with pytest.raises(api.RtsError):
        api.accumulate_moments_soft_light_list(lst, good, pos, nrm, counts[:2], None, clamp=clamp)


def test_struct_layout_is_what_the_compiler_lays_out(tmp_path):
    assert C.sizeof(api.MomentsClamp) == 16
    name, mirror = "rtsh_moments_clamp", api.MomentsClamp
    body = f'  printf("%zu", sizeof({name}));\n' + "".join(f'  printf(" %zu", offsetof({name}, {f}));\n' for f, _ in mirror._fields_)
    body += '  printf(" %d\\n", (int)RTSH_MOMENTS_CLAMP_MAX_RADIUS);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rts_scene.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [16, 0, 4, 8, 12, 4] and [getattr(mirror, f).offset for f, _ in mirror._fields_] == [0, 4, 8, 12]


def test_clamped_twins_on_tiny_frames_under_the_sanitizers(tmp_path):
    """tests/cpp/list_moments_clamp_host.cpp: the host twins (rts_scene.cpp and the shared per-pixel source, compiled into the program --
    nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow over 1 x 1, 1 x 5 and 5 x 1 frames in
    exact-size heap blocks at radius 4, and the bounds function at its extremes."""
    exe = str(tmp_path / "list_moments_clamp_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "list_moments_clamp_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 300, run.stdout[-2000:]
