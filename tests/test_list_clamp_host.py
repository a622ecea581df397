"""CPU: the host twin of the clamped temporal accumulation (rtsh_accumulate_visibility_list_clamped) against the numpy rule of
tests/list_clamp_cases.py, bit for bit -- and what pins the rule: its four anchors with no tolerance, every refusal, the ignored
reserved words, clamp=None, the struct's layout and a sanitized stand-alone host program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import list_clamp_cases as cc
import list_combine_cases as lc
import list_temporal_cases as tc
from raytracedshadows_amd import api

f32, u32 = np.float32, np.uint32
INVALID = 1


def _prev(c):
    return (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"])


def _twin(c, count, radius, margin=0.0, p=None, with_map=True, first=False, threads=0):
    return api.accumulate_visibility_list(cc.the_list(count), p or c["params"], c["pos"], c["nrm"], c["vis"], None if first else _prev(c),
                                          c["map"] if with_map else None, threads, clamp=cc.clamp_of(radius, margin))


def _plain(c, count, p=None, with_map=True, first=False):
    return api.accumulate_visibility_list(cc.the_list(count), p or c["params"], c["pos"], c["nrm"], c["vis"], None if first else _prev(c),
                                          c["map"] if with_map else None)


def test_the_numpy_rule_itself():
    """With a huge margin the restatement equals list_temporal_cases.accumulate_rule on the finite pairs, and the census of the biting
    40 x 40 "pixels" pair holds at r = 1 and r = 4 (both asserted inside)."""
    cc.check_huge_margin()
    out = cc.census()
    assert set(out) == {1, 4}


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("wh", cc.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_equals_the_numpy_rule(wh, kind):
    """Every case and frame: radii 0, 1, 2, 4 x margins 0, 0.125, 3.0e38 x lists of 1, 3, 8 lights with the map; without a map; the first
    frame; max_length 1, 2, 5, 255 and reset_lights 0, 0b101, all ones."""
    c = cc.case(kind, wh)
    for radius in cc.RADII:
        for margin in cc.MARGINS:
            for count in (1, 3, 8):
                cc.same_bits(_twin(c, count, radius, margin), cc.rule_of(c, count, radius, margin), (kind, wh, radius, margin, count))
        cc.same_bits(_twin(c, 8, radius, 0.125, with_map=False), cc.rule_of(c, 8, radius, 0.125, with_map=False), (kind, wh, radius, "no map"))
        cc.same_bits(_twin(c, 3, radius, first=True), cc.rule_of(c, 3, radius, 0.0, first=True), (kind, wh, radius, "first frame"))
    for max_length in tc.MAX_LENGTHS:
        for reset in tc.RESETS:
            p = tc.with_params(c["params"], max_length, reset)
            radius = 1 if reset else 4
            cc.same_bits(_twin(c, 8, radius, 0.0, p), cc.rule_of(c, 8, radius, 0.0, p), (kind, wh, radius, max_length, reset))


def test_threads_change_nothing():
    c = cc.case("bite-turn", (40, 40))
    cc.same_bits(_twin(c, 8, 2, threads=7), _twin(c, 8, 2, threads=1), "7 threads")


def test_anchor_1_a_huge_margin_is_the_unclamped_pass():
    """Finite planes, margin 3.0e38: the bits of rtsh_accumulate_visibility_list, at every radius."""
    for motion in tc.MOTIONS:
        for wh in ((17, 15), (40, 40)):
            c = tc.geometric(motion, wh)
            for radius in cc.RADII:
                for with_map in (True, False):
                    cc.same_bits(_twin(c, 8, radius, 3.0e38, with_map=with_map), _plain(c, 8, with_map=with_map), (motion, wh, radius, with_map))


def test_anchor_2_radius_0_margin_0_gives_the_current_plane():
    """visibility_out == visibility at every blended pixel whose current value is finite and not -0 (the history of the geometric pairs
    is finite); and the unclamped pass does differ there."""
    for motion in ("subpixel", "pixels", "turn"):
        c = dict(tc.geometric(motion, (40, 40)))
        vis = c["vis"].copy()
        vis[:, ::5, ::3] = f32(1e-41)                                    # denormals, +0 and huge values among the current ones
        vis[:, 1::7, ::4] = f32(0.0)
        vis[:, 2::7, 1::4] = f32(-3e38)
        vis[:, 3::6, 2::5] = f32(-0.0)                                   # ... and the excepted ones
        vis[:, 4::6, 3::5] = np.inf
        c["vis"] = vis
        got, plain = _twin(c, 8, 0, 0.0), _plain(c, 8)
        blended = got[1] > 1
        covered = blended & np.isfinite(vis) & (vis.view(u32) != 0x80000000)
        assert covered.sum() > 1000 and (blended & ~covered).sum() > 50
        assert (got[0].view(u32)[covered] == vis.view(u32)[covered]).all()
        assert (plain[0].view(u32)[covered] != vis.view(u32)[covered]).sum() > 1000
        assert (got[1] == plain[1]).all()
        minus_zero = blended & (vis.view(u32) == 0x80000000)             # why -0 is excepted: -0 + 0 is +0
        assert (got[0].view(u32)[minus_zero] == 0).any()
        assert (got[0].view(u32)[blended & np.isinf(vis)] == 0x7FC00000).all()


@pytest.mark.parametrize("kind", ["awkward", "bite-pixels", "bite-turn"])
def test_anchor_3_the_pass_through_cases_keep_the_current_bits(kind):
    """The first frame, max_length 1, a light in reset_lights: the unclamped pass's bits, which are the current plane's; a pixel with
    no accepted tap likewise (length 1 in the unclamped result)."""
    c = cc.case(kind, (40, 40))
    for radius in (0, 4):
        closed = [(tc.with_params(c["params"], 1, 0), False), (tc.with_params(c["params"], 255, 0xFF), False), (c["params"], True)]
        for p, first in closed:
            cc.same_bits(_twin(c, 8, radius, 0.0, p, first=first), _plain(c, 8, p, first=first), (kind, radius, first))
        p = tc.with_params(c["params"], 255, 0b101)
        got, plain = _twin(c, 8, radius, 0.0, p), _plain(c, 8, p)
        for l in (0, 2):
            cc.same_bits((got[0][l], got[1][l]), (plain[0][l], plain[1][l]), (kind, radius, "reset light", l))
        got, plain = _twin(c, 8, radius), _plain(c, 8)
        assert (got[1] == plain[1]).all()                                # the clamp does not shorten a history
        through = plain[1] <= 1
        assert (got[0].view(u32)[through] == plain[0].view(u32)[through]).all()
        if kind != "awkward":
            assert (got[0].view(u32) != plain[0].view(u32)).sum() > 1000


@pytest.mark.parametrize("wh", [(17, 15), (40, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_anchor_4_the_step(wh):
    """History 1.0 of length >= 1 everywhere, current 0.0 everywhere, a still camera, margin 0: exactly +0.0 at any radius and any
    max_length, where the unclamped pass gives 1 - 1/n."""
    W, H = wh
    cur_cam, _ = tc.cameras("turn", wh)
    nrm, pos = tc._gbuffer(cur_cam, W, H)
    p0 = api.TemporalParams.make((0, 0, 0), cur_cam["right"], cur_cam["up"], cur_cam["fwd"], cur_cam["scale_x"], cur_cam["scale_y"], 0.9, 0.02, 5, 0)
    vis, hist = np.zeros((8, H, W), f32), np.ones((8, H, W), f32)
    lengths = np.ascontiguousarray(np.maximum(tc.lengths(wh), 1))
    lst = cc.the_list(8)
    for max_length in (2, 5, 32, 255):
        p = tc.with_params(p0, max_length, 0)
        plain = api.accumulate_visibility_list(lst, p, pos, nrm, vis, (pos, nrm, hist, lengths))
        n = plain[1].astype(f32)
        blended = plain[1] > 1
        assert blended.sum() > 100
        assert (plain[0][blended] == (f32(1) + (f32(0) - f32(1)) * (f32(1) / n[blended]))).all()
        for radius in cc.RADII:
            got = api.accumulate_visibility_list(lst, p, pos, nrm, vis, (pos, nrm, hist, lengths), clamp=cc.clamp_of(radius))
            assert (got[0].view(u32) == 0).all() and (got[1] == plain[1]).all(), (max_length, radius)


def test_reserved_words_are_ignored_and_none_is_the_existing_call():
    c = cc.case("bite-turn", (33, 18))
    clamp = cc.clamp_of(2, 0.125)
    want = api.accumulate_visibility_list(cc.the_list(8), c["params"], c["pos"], c["nrm"], c["vis"], _prev(c), c["map"], clamp=clamp)
    clamp.reserved_[0], clamp.reserved_[1] = 0xDEADBEEF, 0xFFFFFFFF
    p = tc.with_params(c["params"])
    p.reserved_[0], p.reserved_[1] = 0xFFFFFFFF, 0x12345678
    cc.same_bits(api.accumulate_visibility_list(cc.the_list(8), p, c["pos"], c["nrm"], c["vis"], _prev(c), c["map"], clamp=clamp), want, "reserved_")
    none = api.accumulate_visibility_list(cc.the_list(8), c["params"], c["pos"], c["nrm"], c["vis"], _prev(c), c["map"], 0, clamp=None)
    cc.same_bits(none, tc.rule_of(c, 8), "clamp=None")
    cc.same_bits(none, _plain(c, 8), "clamp=None against the call without the keyword")


def test_the_struct_is_16_bytes():
    assert C.sizeof(api.HistoryClamp) == 16 and C.alignment(api.HistoryClamp) == 4
    assert (api.HistoryClamp.radius.offset, api.HistoryClamp.margin.offset, api.HistoryClamp.reserved_.offset) == (0, 4, 8)
    k = api.HistoryClamp.make(3, 0.1)
    assert k.radius == 3 and k.margin == f32(0.1) and list(k.reserved_) == [0, 0] and api.HistoryClamp.make(1).margin == 0.0


def test_refusals_write_nothing():
    lib = api._lib
    c = tc.geometric("turn", (16, 16))
    a = {k: np.ascontiguousarray(c[k]).copy() for k in ("pos", "nrm", "map", "vis", "prev_pos", "prev_nrm", "prev_vis", "prev_len")}
    out, out_len = np.full((8, 16, 16), 7.5, f32), np.full((8, 16, 16), 0xAB, np.uint8)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    ref = lambda s: C.byref(s) if s is not None else None
    good, lst, box = c["params"], cc.the_list(3), cc.clamp_of(2, 0.125)

    def call(lst_=lst, p=good, W=16, H=16, o=out, ol=out_len, k=box, **swap):
        b = dict(a, **swap)
        return lib.rtsh_accumulate_visibility_list_clamped(ref(lst_), ref(p), ptr(b["pos"]), ptr(b["nrm"]), ptr(b["map"]), ptr(b["vis"]),
                                                           ptr(b["prev_pos"]), ptr(b["prev_nrm"]), ptr(b["prev_vis"]), ptr(b["prev_len"]), W, H,
                                                           ptr(o), ptr(ol), ref(k), 0)

    assert call() == 0 and call(map=None) == 0
    assert call(prev_pos=None, prev_nrm=None, prev_vis=None, prev_len=None) == 0
    out[:], out_len[:] = 7.5, 0xAB
    # the clamp's own
    assert call(k=None) == INVALID
    for radius in (5, 6, 0x80000000, 0xFFFFFFFF):
        assert call(k=cc.clamp_of(radius)) == INVALID, radius
    for margin in (-1.0, -1e-45, np.nan, np.inf, -np.inf):
        assert call(k=cc.clamp_of(1, margin)) == INVALID, margin
    assert call(k=cc.clamp_of(4, 0.0)) == 0 and call(k=cc.clamp_of(0, 3.0e38)) == 0 and call(k=cc.clamp_of(0, -0.0)) == 0
    out[:], out_len[:] = 7.5, 0xAB
    vis_before = a["vis"].copy()
    assert call(o=a["vis"]) == INVALID                                   # visibility_out == visibility
    assert (a["vis"].view(u32) == vis_before.view(u32)).all()
    # everything the unclamped form refuses
    for bad in lc.bad_lists()[0]:
        assert call(lst_=bad) == INVALID
    bad_params = [None]
    for field, value in (("max_length", 0), ("max_length", 256), ("normal_cos_min", np.nan), ("plane_eps", -np.inf), ("prev_scale_x", 0.0),
                         ("prev_scale_x", np.inf), ("prev_scale_y", np.nan), ("prev_scale_y", -0.0)):
        p = tc.with_params(good)
        setattr(p, field, value)
        bad_params.append(p)
    for field in ("eye_delta", "prev_right", "prev_up", "prev_fwd"):
        for i, value in ((0, np.nan), (1, np.inf), (2, -np.inf)):
            p = tc.with_params(good)
            getattr(p, field)[i] = value
            bad_params.append(p)
    for p in bad_params:
        assert call(p=p) == INVALID
    for name in ("pos", "nrm", "vis"):
        assert call(**{name: None}) == INVALID, name
    assert call(o=None) == INVALID and call(ol=None) == INVALID
    prevs = ("prev_pos", "prev_nrm", "prev_vis", "prev_len")
    for keep in range(1, 15):
        assert call(**{name: None for i, name in enumerate(prevs) if not (keep >> i) & 1}) == INVALID, keep
    for W, H in ((0, 16), (16, 0), (65537, 1), (1, 65537), (0xFFFFFFFF, 1)):
        assert call(W=W, H=H) == INVALID, (W, H)
    assert call(prev_vis=out) == INVALID and call(prev_len=out_len) == INVALID
    assert (out == 7.5).all() and (out_len == 0xAB).all()
    with pytest.raises(api.RtsError):
        api.accumulate_visibility_list(lst, good, a["pos"], a["nrm"], a["vis"], clamp=cc.clamp_of(5))


def test_planes_from_the_count_up_are_never_touched():
    c = cc.case("bite-turn", (17, 15))
    got = np.full((8, 15, 17), 7.5, f32), np.full((8, 15, 17), 0xAB, np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    vis, pvis, plen = c["vis"].copy(), c["prev_vis"].copy(), c["prev_len"].copy()
    vis[3:], pvis[3:], plen[3:] = np.nan, np.nan, 0
    a = [np.ascontiguousarray(c[k]) for k in ("pos", "nrm", "map", "prev_pos", "prev_nrm")]
    lst, box = cc.the_list(3), cc.clamp_of(4)
    assert api._lib.rtsh_accumulate_visibility_list_clamped(C.byref(lst), C.byref(c["params"]), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(vis),
                                                            ptr(a[3]), ptr(a[4]), ptr(pvis), ptr(plen), 17, 15, ptr(got[0]), ptr(got[1]),
                                                            C.byref(box), 0) == 0
    cc.same_bits((got[0][:3], got[1][:3]), cc.rule_of(c, 3, 4, 0.0), "planes below the count")
    assert (got[0][3:] == 7.5).all() and (got[1][3:] == 0xAB).all()


def test_list_clamp_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/list_clamp_host.cpp: the clamped host twin itself (rts_scene.cpp and the shared per-pixel source, compiled into the
    program -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow, over every refusal and
    over small frames whose buffers are heap blocks of exactly the size the header states."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "list_clamp_host")
    csrc = os.path.join(root, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(root, "tests", "cpp", "list_clamp_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 1000, run.stdout[-2000:]
