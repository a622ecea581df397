"""The motion forms of the three temporal passes and the motion G-buffer pass on awkward inputs, on the host (include/rts_scene.h's last
section): the synthetic motion planes, small streams and poisoned previous streams of tests/list_motion_edge_cases.py.
The host twins against the numpy rules of tests/list_motion_cases.py bit for bit over every frame of list_temporal_cases.FRAMES, every
kind, 1, 3 and 8 lights and a walk through MAX_LENGTHS, RESETS, RADII and MARGINS; the census; the properties the header states; the
G-buffer twin on a root-leaf stream, cameras that miss everything or sit inside the moved part, and poisoned previous streams.  No
GPU.  The twins run under the sanitizers in tests/cpp/list_motion_edges_host.cpp."""
import os
import subprocess

import numpy as np
import pytest

import list_moments_cases as mc
import list_motion_cases as ms
import list_motion_edge_cases as ec
import list_temporal_cases as tc
from raytracedshadows_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32


def salts(wh):
    """A frame of fewer than 64 pixels sees every group of the planes through eight salts."""
    return range(8) if wh[0] * wh[1] < 64 else (0,)


def host_forms(c, wh, count, sel, motion, positions=None, threads=0, forms=("plain", "clamped", "moments")):
    """dict form -> the host twin's planes for one selection of parameters."""
    pos = c["pos"] if positions is None else positions
    lights_map = c["map"] if sel["with_map"] else None
    out = {}
    if "plain" in forms:
        p = tc.with_params(c["params"], sel["max_length"], sel["reset"])
        out["plain"] = api.accumulate_visibility_list(tc.the_list(count), p, pos, c["nrm"], c["vis"],
                                                      (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"]), lights_map, threads, motion=motion)
    if "clamped" in forms:
        p = tc.with_params(c["params"], sel["clamp_max_length"], sel["clamp_reset"])
        out["clamped"] = api.accumulate_visibility_list(tc.the_list(count), p, pos, c["nrm"], c["vis"],
                                                        (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"]), lights_map, threads,
                                                        clamp=api.HistoryClamp.make(sel["radius"], sel["margin"]), motion=motion)
    if "moments" in forms:
        p = tc.with_params(c["params"], sel["max_length"], sel["reset"])
        soft = mc.the_list(count)
        pm, ps = mc.history(wh, soft)
        out["moments"] = api.accumulate_moments_soft_light_list(soft, p, pos, c["nrm"], ms.planes(wh, 1)[1],
                                                                (c["prev_pos"], c["prev_nrm"], pm, ps, c["prev_len"]), lights_map, threads, motion=motion)
    return out


def rule_forms(c, wh, count, sel, motion):
    lights_map = c["map"] if sel["with_map"] else None
    prev = (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"])
    p = tc.with_params(c["params"], sel["max_length"], sel["reset"])
    pc = tc.with_params(c["params"], sel["clamp_max_length"], sel["clamp_reset"])
    soft = mc.the_list(count)
    pm, ps = mc.history(wh, soft)
    return dict(plain=ms.accumulate_motion_rule(count, p, c["nrm"], c["vis"], prev, lights_map, motion),
                clamped=ms.accumulate_motion_rule(count, pc, c["nrm"], c["vis"], prev, lights_map, motion, (sel["radius"], sel["margin"])),
                moments=ms.moments_motion_rule(soft, p, c["nrm"], ms.planes(wh, 1)[1], (c["prev_pos"], c["prev_nrm"], pm, ps, c["prev_len"]),
                                               lights_map, motion))


# ------------------------------------------------------------------------------------------------------------ the three passes
def test_the_selection_walks_every_value_with_every_frame():
    for fi in range(len(tc.FRAMES)):
        runs = [ec.selection(fi, k) for k in range(len(tc.KINDS) * 3)]
        assert {(s["max_length"], s["reset"]) for s in runs} == {(m, r) for m in ec.MAX_LENGTHS for r in ec.RESETS}
        assert {(s["radius"], s["margin"]) for s in runs} == {(r, m) for r in ec.RADII for m in ec.MARGINS}
        assert {s["clamp_max_length"] for s in runs} == set(ec.MAX_LENGTHS) and {s["clamp_reset"] for s in runs} == set(ec.RESETS)
        assert {s["with_map"] for s in runs} == {True, False}
        assert any(s["radius"] == 4 and (s["clamp_max_length"] == 1 or s["clamp_reset"] == 0xFF) for s in runs)


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("wh", tc.FRAMES)
def test_motion_forms_match_the_rule_on_awkward_planes(wh, kind):
    fi, ki = tc.FRAMES.index(wh), tc.KINDS.index(kind)
    c = tc.case(kind, wh)
    for ci, count in enumerate((1, 3, 8)):
        sel = ec.selection(fi, ki * 3 + ci)
        for salt in salts(wh):
            motion = ec.motion_planes(c, wh, salt)
            got, want = host_forms(c, wh, count, sel, motion), rule_forms(c, wh, count, sel, motion)
            for form in ("plain", "clamped", "moments"):
                ms.same_planes(got[form], want[form], (wh, kind, count, salt, sorted(sel.items()), form))


def test_one_thread_and_three_agree():
    wh = (33, 18)
    for kind in ("awkward", "pixels"):
        c = tc.case(kind, wh)
        motion = ec.motion_planes(c, wh)
        sel = dict(ec.selection(0, 2), radius=4, clamp_max_length=5, clamp_reset=0)
        one, three = host_forms(c, wh, 8, sel, motion, threads=1), host_forms(c, wh, 8, sel, motion, threads=3)
        for form in one:
            ms.same_planes(one[form], three[form], (kind, form, "threads"))


def test_census_of_the_awkward_planes():
    """Both outcomes of the replaced groups occur, the shifted group blends, the zero groups never do: from the numpy rules alone."""
    out = ec.census()
    assert out["q_replaced"][0] >= 20 and out["q_replaced"][1] >= 20 and out["m_replaced"][0] >= 20 and out["m_replaced"][1] >= 20, out
    assert out["shifted"][0] >= 20 and out["m_zero"][0] == 0, out


def test_every_bound_is_probed_from_both_sides_on_every_frame():
    """bounds_points asserts the side of each comparison itself; here: it does so for every frame and kind, and the points differ."""
    for wh in tc.FRAMES:
        for kind in tc.KINDS:
            pts, exact = ec.bounds_points(tc.case(kind, wh)["params"], wh)
            assert pts.shape == (len(ec.BOUNDS), 3) and np.isfinite(pts).all() and exact >= 2, (wh, kind, exact)
            for lo in (3, 5, 7, 9):                                      # the accepted and the rejected point of one bound are neighbours
                assert (pts[lo] != pts[lo + 1]).any() and np.abs(pts[lo] - pts[lo + 1]).max() < 1e-3, (wh, kind, lo)


# ------------------------------------------------------------------------------------------------------------ the header's properties
@pytest.mark.parametrize("wh", [(1, 1), (17, 15), (40, 40)])
def test_positions_and_w_lanes_are_never_read(wh):
    """With a history, no motion form reads `positions` -- a plane of NaN changes no bit --, nor the .w lane of any texel plane."""
    for kind in ("awkward", "pixels"):
        c = tc.case(kind, wh)
        motion = ec.motion_planes(c, wh, 3)
        sel = ec.selection(1, 5)
        want = host_forms(c, wh, 8, sel, motion)
        nan_positions = host_forms(c, wh, 8, sel, motion, positions=np.full((wh[1], wh[0], 4), np.nan, f32))
        lanes = dict(c, nrm=ec.garbage_w(c["nrm"], 1), prev_nrm=ec.garbage_w(c["prev_nrm"], 2), prev_pos=ec.garbage_w(c["prev_pos"], 3))
        w_lanes = host_forms(lanes, wh, 8, sel, (ec.garbage_w(motion[0], 4), ec.garbage_w(motion[1], 5)), positions=ec.garbage_w(c["pos"], 6))
        for form in want:
            ms.same_planes(nan_positions[form], want[form], (wh, kind, form, "NaN positions"))
            ms.same_planes(w_lanes[form], want[form], (wh, kind, form, ".w lanes"))


@pytest.mark.parametrize("wh", [(7, 9), (40, 40)])
def test_background_pixels_give_zero_whatever_the_motion_texel_holds(wh):
    W, H = wh
    for kind in ("awkward", "pixels"):
        c = tc.case(kind, wh)
        bg = (c["nrm"][..., :3] == 0).all(-1)
        assert bg.any() and not bg.all()
        sel = dict(ec.selection(0, 8), with_map=False)
        base = host_forms(c, wh, 8, sel, ec.motion_planes(c, wh, 0))
        for salt in range(8):                                            # every group's texel comes to lie on the background pixels
            pts, pnr = ec.motion_planes(c, wh, salt)
            got = host_forms(c, wh, 8, sel, (pts, pnr))
            for form, planes in got.items():
                for plane in planes:
                    assert (plane.view(u32 if plane.dtype == f32 else plane.dtype)[:, bg] == 0).all(), (wh, kind, salt, form)
            # ... and a background pixel's texel reaches no other pixel: with the active pixels' texels restored, nothing else changes
            base_pts, base_pnr = ec.motion_planes(c, wh, 0)
            mixed = (np.where(bg[..., None], pts, base_pts), np.where(bg[..., None], pnr, base_pnr))
            again = host_forms(c, wh, 8, sel, mixed)
            for form in base:
                ms.same_planes(again[form], base[form], (wh, kind, salt, form, "background texels"))


def loose_case(wh, cos_min):
    """The "pixels" pair with a normal_cos_min of 0 or below and whole histories: a zero M_p would PASS both geometric tests
    (0 >= cos_min, |0| <= plane_eps), so only the header's own sentence -- M_p all zero: no tap is accepted -- makes the pixel restart."""
    c = dict(tc.geometric("pixels", wh))
    q = api.TemporalParams.from_buffer_copy(c["params"])
    q.normal_cos_min = cos_min
    c["params"], c["prev_len"] = q, np.full((8, wh[1], wh[0]), 7, np.uint8)
    return c


@pytest.mark.parametrize("cos_min", (0.0, -1.0))
def test_zero_previous_normal_restarts_where_the_normal_test_would_pass(cos_min):
    wh = (40, 40)
    c = loose_case(wh, cos_min)
    motion = ec.motion_planes(c, wh)
    sel = dict(ec.selection(0, 2), with_map=False, max_length=5, reset=0, clamp_max_length=5, clamp_reset=0)
    got, want = host_forms(c, wh, 3, sel, motion), rule_forms(c, wh, 3, sel, motion)
    g, j = ec.groups(wh)
    zero = (g == 5) & ~(c["nrm"][..., :3] == 0).all(-1)
    parent = tc.accumulate_rule(3, c["params"], c["pos"], c["nrm"], c["vis"], (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"]))[1]
    assert (parent[0][zero] > 1).sum() >= 20 and (j[zero] % 2 == 0).any() and (j[zero] % 2 == 1).any()
    for form in got:
        ms.same_planes(got[form], want[form], (cos_min, form))
        assert (got[form][-1][:, zero] == 1).all(), (cos_min, form, "a zero M_p, +0 or -0, must restart")


# ------------------------------------------------------------------------------------------------------------ the G-buffer pass
def gbuffer(s, cam, wh, prev=None, **kw):
    _, eye, prev_eye, target, fovy = cam
    return api.primary_gbuffer_motion(s["packed"], s["prev_packed"] if prev is None else prev, eye, prev_eye, target, fovy, wh[0], wh[1], **kw)


def rule(s, cam, wh, out, prev=None):
    _, eye, prev_eye, target, fovy = cam
    d = ms.directions(api.camera_basis(eye, target, fovy, wh[0], wh[1]), wh[0], wh[1])
    return ms.motion_texel_rule(out[4], s["packed"], s["prev_packed"] if prev is None else prev, eye, prev_eye, d, out[0], out[1])


@pytest.mark.parametrize("wh", ec.GBUFFER_FRAMES)
@pytest.mark.parametrize("name", ("one", "quad", "cornell"))
def test_gbuffer_motion_on_small_streams_matches_the_rule(name, wh):
    W, H = wh
    s = ec.small_streams(name)
    assert (name == "one") == (ec.leaf_nodes(s["packed"]).tolist() == [0]), "the root of `one` is a leaf"
    for cam in ec.cameras_of(name):
        out = gbuffer(s, cam, wh)
        parent = api.primary_gbuffer(s["packed"], cam[1], cam[3], cam[4], W, H)
        ms.same_planes(out[:2], parent[:2], (name, cam[0], wh, "parent planes"))
        ms.same_planes(out[2:4], rule(s, cam, wh, out), (name, cam[0], wh, "motion texels"))
        ms.same_planes(gbuffer(s, cam, wh, threads=3)[:5], out[:5], (name, cam[0], wh, "threads"))
        if cam[0] == "all_miss":
            assert out[5] == 0 and (out[4] == ec.END).all()
            assert all((a.view(u32) == 0).all() for a in out[:4])
        elif cam[0] == "eye_inside_the_moved_box":
            assert out[5] == W * H and (out[2][..., 3] == 2).all(), "inside the box every pixel sees a moved face"
        elif cam[0] == "front":
            assert (out[2][..., 3] == 2).any()
            if wh == (1, 1):
                d = ms.directions(api.camera_basis(cam[1], cam[3], cam[4], 1, 1), 1, 1)
                assert d[0, 0, 0] == 0 and d[0, 0, 1] == 0 and d[0, 0, 2] == -1, "the only direction has exact zero components"
                assert out[5] == 1
        elif cam[0] == "still" and name == "quad" and W * H >= 63:
            assert (out[2][..., 3] == 1).any() and (out[2][..., 3] == 2).any(), "one triangle moved, the other did not"


@pytest.mark.parametrize("wh", ec.GBUFFER_FRAMES)
@pytest.mark.parametrize("name", ("one", "quad", "cornell"))
def test_gbuffer_motion_with_a_poisoned_previous_stream(name, wh):
    s = ec.small_streams(name)
    cam = ec.cameras_of(name)[0]
    clean = gbuffer(s, cam, wh)
    # words the pass never reads in prev: not one output bit changes
    never, _ = ec.poison(s["packed"], s["prev_packed"], "never_read")
    assert (never != s["prev_packed"]).any()
    ms.same_planes(gbuffer(s, cam, wh, prev=never)[:5], clean[:5], (name, wh, "never-read words"))
    for kind in ("leaf_words", "sign"):
        poisoned, touched = ec.poison(s["packed"], s["prev_packed"], kind)
        assert len(touched) > 0
        out = gbuffer(s, cam, wh, prev=poisoned)                         # (RTS_OK: api raises otherwise)
        ms.same_planes(out[:2] + (out[4],), clean[:2] + (clean[4],), (name, wh, kind, "parent planes and leaves"))
        seen = np.isin(out[4], touched)
        assert seen.any() or name == "cornell", (name, wh, kind, "no touched leaf is seen")
        assert (out[2][..., 3][seen] == 2).all(), (name, wh, kind, "a touched leaf must be MOVED")
        ec.nan_aware_same(out[2:4], rule(s, cam, wh, out, prev=poisoned), (name, wh, kind, "motion texels"))
        if kind == "sign":                                               # equal values, other bits: MOVED, and the texel a finite one
            assert np.isfinite(out[2][seen]).all() and np.isfinite(out[3][seen]).all()
    if name == "cornell" and wh == (17, 15):
        for kind in ("leaf_words", "sign"):
            out = gbuffer(s, cam, wh, prev=ec.poison(s["packed"], s["prev_packed"], kind)[0])
            assert np.isin(out[4], ec.poison(s["packed"], s["prev_packed"], kind)[1]).sum() >= 20


# ------------------------------------------------------------------------------------------------------------ the sanitizers
def test_motion_forms_on_tiny_frames_under_the_sanitizers(tmp_path):
    """tests/cpp/list_motion_edges_host.cpp: the host twins (rts_scene.cpp and the shared per-pixel source, compiled into the program --
    nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow over 1 x 1, 1 x 5 and 5 x 1 frames
    in exact-size heap blocks, with texels on the on-screen bounds and clamp radius 4."""
    exe = str(tmp_path / "list_motion_edges_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "list_motion_edges_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 300, run.stdout[-2000:]
