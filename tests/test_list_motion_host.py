"""The motion G-buffer pass and the motion forms of the three temporal passes on the host (include/rts_scene.h's last section,
DESIGN.md 4.29): the host twins against the numpy rules of tests/list_motion_cases.py bit for bit, the anchors of the header, and every
refusal with canary-filled outputs.  No GPU.  The twins themselves run under the sanitizers in tests/cpp/list_motion_host.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import list_moments_cases as mc
import list_motion_cases as ms
import list_temporal_cases as tc
from raytracedshadows_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
MOVES = ("static", "translate", "rotate")
_FRAMES = {}


def pair(name, move, wh, camera):
    """Two frames of a moved scene: frame 0 from the previous stream and eye, frame 1 the motion G-buffer pass.  Shared, read-only."""
    key = (name, move, wh, camera)
    if key not in _FRAMES:
        s = ms.streams(name, move)
        W, H = wh
        eye, prev_eye = ms.cameras(s, camera)
        p0, n0, _, _, leaves0, _ = api.primary_gbuffer_motion(s["prev_packed"], s["prev_packed"], prev_eye, prev_eye, s["target"], s["fovy"], W, H)
        pos, nrm, pts, pnr, leaves, hits = api.primary_gbuffer_motion(s["packed"], s["prev_packed"], eye, prev_eye, s["target"], s["fovy"], W, H)
        f = dict(s=s, eye=eye, prev_eye=prev_eye, prev_pos=p0, prev_nrm=n0, prev_leaves=leaves0, pos=pos, nrm=nrm, pts=pts, pnr=pnr,
                 leaves=leaves, hits=hits, params=ms.params_of(s, wh, eye, prev_eye))
        for v in f.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FRAMES[key] = f
    return _FRAMES[key]


def history(wh, count):
    """Awkward history of the three passes for a frame size: visibility and lengths, and the moments' planes."""
    W, H = wh
    vis, counts, lights_map = ms.planes(wh, 1)
    prev_vis = np.random.RandomState(W * 31 + H).randint(0, 1 << 20, (8, H, W)).astype(f32) / f32(1 << 20)
    return vis, counts, lights_map, prev_vis, tc.lengths(wh, 1)


# ------------------------------------------------------------------------------------------------------------ the G-buffer pass
@pytest.mark.parametrize("wh", ms.FRAMES)
@pytest.mark.parametrize("move", MOVES + ("degenerate",))
@pytest.mark.parametrize("name", ("cornell", "terrain"))
def test_gbuffer_motion_matches_the_rule(name, move, wh):
    W, H = wh
    for camera in ("still", "moved"):
        f = pair(name, move, wh, camera)
        s = f["s"]
        pos, nrm, hits = api.primary_gbuffer(s["packed"], f["eye"], s["target"], s["fovy"], W, H)
        ms.same_planes((f["pos"], f["nrm"]), (pos, nrm), (name, move, wh, camera, "parent planes"))
        assert f["hits"] == hits
        d = ms.directions(api.camera_basis(f["eye"], s["target"], s["fovy"], W, H), W, H)
        want = ms.motion_texel_rule(f["leaves"], s["packed"], s["prev_packed"], f["eye"], f["prev_eye"], d, f["pos"], f["nrm"])
        ms.same_planes((f["pts"], f["pnr"]), want, (name, move, wh, camera, "motion texels"))
        # the leaves plane: background exactly where the position's w is 0, and the point lies on the leaf's triangle
        assert ((f["leaves"] == ms.END) == (f["pos"][..., 3] == 0)).all()
        assert ms.on_triangle(f["leaves"], s["packed"], f["eye"], f["pos"]).all()
        moved = int((f["pts"][..., 3] == 2).sum())
        assert (moved == 0) == (move == "static"), (name, move, wh, moved)
        bg = f["leaves"] == ms.END
        assert (f["pts"].view(u32)[bg] == 0).all() and (f["pnr"].view(u32)[bg] == 0).all()


def test_gbuffer_motion_without_normals_or_leaves_and_across_threads():
    s = ms.streams("terrain", "translate")
    W, H = 37, 19
    eye, prev_eye = ms.cameras(s, "moved")
    want = api.primary_gbuffer_motion(s["packed"], s["prev_packed"], eye, prev_eye, s["target"], s["fovy"], W, H, threads=1)
    got = api.primary_gbuffer_motion(s["packed"], s["prev_packed"], eye, prev_eye, s["target"], s["fovy"], W, H, threads=3, want_leaves=False)
    assert got[4] is None and got[5] == want[5]
    ms.same_planes(got[:4], want[:4], "threads, no leaves")
    pos, pts, pnr = (np.full((H, W, 4), 7.5, f32) for _ in range(3))
    e, pe, t = api._f3(eye), api._f3(prev_eye), api._f3(s["target"])
    st = api._lib.rtsh_primary_gbuffer_motion(api._ptr(s["packed"]), s["packed"].shape[0], api._ptr(s["prev_packed"]), s["packed"].shape[0], e, pe,
                                              t, s["fovy"], W, H, api._ptr(pos), None, api._ptr(pts), api._ptr(pnr), None, None, 1)
    assert st == 0
    ms.same_planes((pos, pts, pnr), (want[0], want[2], want[3]), "NULL normals, leaves and hit count")


# ------------------------------------------------------------------------------------------------------------ the three passes
def run_forms(f, wh, count, motion=True, p=None, prev_vis_len=None, lights_map="hashed", threads=0, motion_planes=None):
    """(plain, clamped, moments) outputs of the host twins over a pair; motion=False: the parents."""
    vis, counts, hashed_map, prev_vis, prev_len = history(wh, count)
    lights_map = hashed_map if isinstance(lights_map, str) else lights_map
    if prev_vis_len is not None:
        prev_vis, prev_len = prev_vis_len
    p = p or f["params"]
    hard, soft = tc.the_list(count), mc.the_list(count)
    pm, ps = mc.history(wh, soft)
    mo = (motion_planes or (f["pts"], f["pnr"])) if motion else None
    prev = (f["prev_pos"], f["prev_nrm"], prev_vis, prev_len)
    plain = api.accumulate_visibility_list(hard, p, f["pos"], f["nrm"], vis, prev, lights_map, threads, motion=mo)
    clamped = api.accumulate_visibility_list(hard, p, f["pos"], f["nrm"], vis, prev, lights_map, threads, clamp=api.HistoryClamp.make(2, 0.05), motion=mo)
    moments = api.accumulate_moments_soft_light_list(soft, p, f["pos"], f["nrm"], counts, (f["prev_pos"], f["prev_nrm"], pm, ps, prev_len),
                                                     lights_map, threads, motion=mo)
    return plain, clamped, moments


def rule_forms(f, wh, count, p=None, use_current_normal=False):
    vis, counts, lights_map, prev_vis, prev_len = history(wh, count)
    p = p or f["params"]
    soft = mc.the_list(count)
    pm, ps = mc.history(wh, soft)
    prev = (f["prev_pos"], f["prev_nrm"], prev_vis, prev_len)
    mo = (f["pts"], f["pnr"])
    plain = ms.accumulate_motion_rule(count, p, f["nrm"], vis, prev, lights_map, mo, None, use_current_normal)
    clamped = ms.accumulate_motion_rule(count, p, f["nrm"], vis, prev, lights_map, mo, (2, 0.05), use_current_normal)
    moments = ms.moments_motion_rule(soft, p, f["nrm"], counts, (f["prev_pos"], f["prev_nrm"], pm, ps, prev_len), lights_map, mo)
    return plain, clamped, moments


@pytest.mark.parametrize("count", ms.COUNTS)
@pytest.mark.parametrize("wh", ms.FRAMES)
@pytest.mark.parametrize("move", MOVES + ("degenerate",))
def test_motion_forms_match_the_rule(move, wh, count):
    for name, camera in (("cornell", "moved"), ("terrain", "still")):
        f = pair(name, move, wh, camera)
        got, want = run_forms(f, wh, count), rule_forms(f, wh, count)
        for g, w, form in zip(got, want, ("plain", "clamped", "moments")):
            ms.same_planes(g, w, (name, move, wh, count, form))
        if count == 3:
            one = run_forms(f, wh, count, threads=1)
            for g, w, form in zip(got, one, ("plain", "clamped", "moments")):
                ms.same_planes(g, w, (name, move, wh, "threads", form))


@pytest.mark.parametrize("camera", ("still", "moved"))
@pytest.mark.parametrize("wh", ms.FRAMES)
def test_anchor_a_static_streams_give_the_parents_bits(wh, camera):
    """prev_packed == packed: every hit is STATIC (w == 1), and each motion accumulate equals its parent with eye_delta = eye - prev_eye."""
    for name in ("cornell", "terrain"):
        f = pair(name, "static", wh, camera)
        hit = f["leaves"] != ms.END
        assert (f["pts"][..., 3][hit] == 1).all() and hit.any()
        ms.same_planes((f["pnr"],), (f["nrm"],), "STATIC normal")
        for count in ms.COUNTS:
            got, want = run_forms(f, wh, count), run_forms(f, wh, count, motion=False)
            for g, w, form in zip(got, want, ("plain", "clamped", "moments")):
                ms.same_planes(g, w, (name, wh, camera, count, form))
            assert (got[0][1] > 1).any(), "the anchor must blend somewhere"


def reprojection(p, Q, W, H):
    """(x0, y0, on screen) of REPROJECT for the points Q, float32 as the header states it."""
    dot3 = lambda v: (Q[..., 0] * f32(v[0]) + Q[..., 1] * f32(v[1])) + Q[..., 2] * f32(v[2])
    with np.errstate(all="ignore"):
        z = dot3(p.prev_fwd)
        a, b = dot3(p.prev_right) / z, dot3(p.prev_up) / z
        fx = (a / f32(p.prev_scale_x) + f32(1.0)) * (f32(0.5) * f32(W)) - f32(0.5)
        fy = (f32(1.0) - b / f32(p.prev_scale_y)) * (f32(0.5) * f32(H)) - f32(0.5)
        gx, gy = fx * f32(32.0) + f32(0.5), fy * f32(32.0) + f32(0.5)
        on = (z > 0) & (gx >= f32(-32.0)) & (gx < f32(W) * f32(32.0)) & (gy >= f32(-32.0)) & (gy < f32(H) * f32(32.0))
    ix, iy = np.floor(np.where(on, gx, 0)).astype(np.int64), np.floor(np.where(on, gy, 0)).astype(np.int64)
    return ix >> 5, iy >> 5, on


def plane_keys(packed):
    """Per node index, a key of the plane its triangle lies in (unit normal and offset, rounded): equal for the triangles of one face."""
    w = np.ascontiguousarray(packed, u32).reshape(-1)
    keys = {}
    for node in range((w.size // 4 + 2) // 5 * 2 - 1):                     # the 2P - 1 nodes of a stream of 5P - 2 vec4
        if w[node * 8 + 3] == ms.END:
            continue
        e0, e1 = w[node * 8:node * 8 + 3].view(f32).astype(np.float64), w[node * 8 + 4:node * 8 + 7].view(f32).astype(np.float64)
        v0 = w[int(w[node * 8 + 3]) * 4:int(w[node * 8 + 3]) * 4 + 3].view(f32).astype(np.float64)
        n = np.cross(e0, e1)
        if not (n * n).sum() > 0:
            continue
        n = n / np.sqrt((n * n).sum())
        if n[np.argmax(np.abs(n))] < 0:
            n = -n
        keys[node] = tuple(np.round(np.append(n, n @ v0), 3) + 0.0)
    return keys


@pytest.mark.parametrize("wh", ms.FRAMES)
def test_anchor_b_tracking_a_translated_box(wh):
    """The tall cornell box moves by T, |N . T| >= 0.25 > plane_eps on its faces: the parent pass restarts on it, the motion pass follows."""
    W, H = wh
    f = pair("cornell", "translate", wh, "still")
    p = f["params"]
    hard = tc.the_list(1)
    vis = np.full((1, H, W), 0.25, f32)
    first = api.accumulate_visibility_list(hard, p, f["prev_pos"], f["prev_nrm"], np.ones((1, H, W), f32))      # frame 0: lengths 1
    prev = (f["prev_pos"], f["prev_nrm"], first[0], first[1])
    assert (first[1] == 1).all()
    parent = api.accumulate_visibility_list(hard, p, f["pos"], f["nrm"], vis, prev)
    motion = api.accumulate_visibility_list(hard, p, f["pos"], f["nrm"], vis, prev, motion=(f["pts"], f["pnr"]))
    x0, y0, on = reprojection(p, f["pts"], W, H)
    moved = f["pts"][..., 3] == 2
    keys = plane_keys(f["s"]["prev_packed"])
    tracked, whole = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for y, x in np.argwhere(moved & on):
        taps = [(y0[y, x] + (k >> 1), x0[y, x] + (k & 1)) for k in range(4)]
        inside = [(ty, tx) for ty, tx in taps if 0 <= ty < H and 0 <= tx < W]
        leaf = int(f["leaves"][y, x])
        tracked[y, x] = any(int(f["prev_leaves"][t]) == leaf for t in inside)
        whole[y, x] = len(inside) == 4 and all(keys.get(int(f["prev_leaves"][t])) == keys[leaf] for t in inside)
    assert tracked.sum() >= 20 and whole.sum() >= 10, (wh, int(tracked.sum()), int(whole.sum()))     # (a non-empty set at both sizes)
    assert (parent[1][0][tracked] == 1).all(), "the parent pass must restart on the moved box"
    assert (motion[1][0][tracked] == 2).any()
    assert (motion[1][0][whole] == 2).all(), np.argwhere(whole & (motion[1][0] != 2))[:6].tolist()
    want = np.float32(1.0) + (np.float32(0.25) - np.float32(1.0)) * (np.float32(1.0) / np.float32(2.0))
    assert (motion[0][0][whole] == want).all()


@pytest.mark.parametrize("wh", ms.FRAMES)
def test_rotation_keeps_history_through_the_previous_normal(wh):
    """normal_cos_min tighter than cos(ANGLE): M_p, the previous frame's orientation, passes where the current normal would not."""
    W, H = wh
    f = pair("cornell", "rotate", wh, "still")
    assert np.cos(ms.ANGLE) < ms.TIGHT_COS_MIN
    p = ms.params_of(f["s"], wh, f["eye"], f["prev_eye"], normal_cos_min=ms.TIGHT_COS_MIN)
    got = run_forms(f, wh, 3, p=p)
    with_m, with_n = rule_forms(f, wh, 3, p=p), rule_forms(f, wh, 3, p=p, use_current_normal=True)
    for g, w, form in zip(got, with_m, ("plain", "clamped", "moments")):
        ms.same_planes(g, w, (wh, form))
    moved = f["pts"][..., 3] == 2
    kept = (with_m[0][1][0] > 1) & moved
    assert kept.sum() >= 10 and not ((with_n[0][1][0] > 1) & moved).any(), (int(kept.sum()), int(((with_n[0][1][0] > 1) & moved).sum()))
    assert (got[0][1][0][kept] > 1).all()


@pytest.mark.parametrize("wh", ms.FRAMES)
def test_degenerate_previous_triangle_and_nan_point_restart(wh):
    W, H = wh
    f = pair("cornell", "degenerate", wh, "still")
    hit = f["leaves"] != ms.END
    zero = hit & (f["pnr"][..., :3] == 0).all(-1)
    assert zero.sum() >= 10 and (f["pts"][..., 3][zero] == 2).all()
    vis, counts, _, _, _ = history(wh, 3)
    full = np.full((8, H, W), 7, np.uint8)
    got = run_forms(f, wh, 3, lights_map=None, prev_vis_len=(np.full((8, H, W), 0.5, f32), full))
    for l in range(3):
        assert (got[0][1][l][zero] == 1).all() and (got[1][1][l][zero] == 1).all() and (got[2][2][l][zero] == 1).all()
        assert (got[0][0][l].view(u32)[zero] == vis[l].view(u32)[zero]).all()
    assert (got[0][1][0][hit & ~zero] > 1).any()
    # a NaN anywhere in a pixel's prev_points texel: every comparison fails, the pixel restarts
    still = pair("cornell", "static", wh, "still")
    pts = still["pts"].copy()
    blended = run_forms(still, wh, 3, lights_map=None, prev_vis_len=(np.full((8, H, W), 0.5, f32), full))
    assert (blended[0][1][0] > 1).all(), "the precondition: with whole texels every pixel of the static frame blends"
    for k, (y, x) in enumerate(((0, 0), (H // 2, W // 2), (H - 1, W - 1))):
        pts[y, x, k] = np.nan
    got = run_forms(still, wh, 3, lights_map=None, prev_vis_len=(np.full((8, H, W), 0.5, f32), full), motion_planes=(pts, still["pnr"]))
    for y, x in ((0, 0), (H // 2, W // 2), (H - 1, W - 1)):
        assert got[0][1][0][y, x] == 1 and got[1][1][0][y, x] == 1 and got[2][2][0][y, x] == 1
    untouched = np.ones((H, W), bool)
    untouched[[0, H // 2, H - 1], [0, W // 2, W - 1]] = False
    assert (got[0][1][0][untouched] == blended[0][1][0][untouched]).all()


# ------------------------------------------------------------------------------------------------------------ refusals
CANARY = 0xA5


def test_gbuffer_motion_refusals_write_nothing():
    s = ms.streams("terrain", "translate")
    W, H = 37, 19
    packed, prev = s["packed"], s["prev_packed"]
    n = packed.shape[0]
    outs = [np.full(H * W * 16, CANARY, np.uint8) for _ in range(4)] + [np.full(H * W * 4, CANARY, np.uint8)]
    hits = C.c_uint64(0x5A5A)
    eye, prev_eye, target = (np.asarray(v, f32) for v in (s["eye"], s["eye"] + f32(0.1), s["target"]))
    other = np.array(prev)
    other[3, 3] ^= 1                                                   # node 1's tag word (an inner node or a leaf: either way it differs)
    short = np.ascontiguousarray(prev[:-5])

    def call(packed=packed, count=n, prev=prev, prev_count=n, eye=eye, prev_eye=prev_eye, target=target, W=W, H=H, skip=()):
        o = [None if i in skip else api._ptr(a) for i, a in enumerate(outs)]
        return api._lib.rtsh_primary_gbuffer_motion(api._ptr_or_none(packed), count, api._ptr_or_none(prev), prev_count, api._f3(eye), api._f3(prev_eye),
                                                    api._f3(target), f32(s["fovy"]), W, H, o[0], o[1], o[2], o[3], o[4], C.byref(hits), 1)

    INVALID, BAD_BVH = 1, 5
    nan_eye, inf_eye = np.array([0, np.nan, 0], f32), np.array([np.inf, 0, 0], f32)
    cases = [(dict(packed=None), INVALID), (dict(prev=None), INVALID), (dict(eye=None), INVALID), (dict(prev_eye=None), INVALID),
             (dict(target=None), INVALID), (dict(W=0), INVALID), (dict(H=0), INVALID), (dict(skip=(0,)), INVALID), (dict(skip=(2,)), INVALID),
             (dict(skip=(3,)), INVALID), (dict(prev_eye=nan_eye), INVALID), (dict(prev_eye=inf_eye), INVALID),
             (dict(prev=short, prev_count=n - 5), INVALID), (dict(prev_count=n + 5), INVALID), (dict(prev=other), BAD_BVH),
             (dict(packed=packed[:-1], count=n - 1, prev=prev[:-1], prev_count=n - 1), BAD_BVH)]
    for kw, want in cases:
        got = call(**kw)
        assert got == want, (list(kw), got, want)
        assert all((a == CANARY).all() for a in outs) and hits.value == 0x5A5A, list(kw)
    assert call() == 0 and not any((a == CANARY).all() for a in outs)


def test_accumulate_motion_refusals_write_nothing():
    wh = (37, 19)
    W, H = wh
    f = pair("terrain", "translate", wh, "moved")
    vis, counts, lights_map, prev_vis, prev_len = history(wh, 3)
    hard, soft = tc.the_list(3), mc.the_list(3)
    pm, ps = mc.history(wh, soft)
    out_f, out_l = np.full((3, H, W), 7.5, f32), np.full((3, H, W), CANARY, np.uint8)
    out_m, out_s = np.full((3, H, W), 0xA5A5, np.uint16), np.full((3, H, W), 0xA5A5A5A5, np.uint32)
    clamp = api.HistoryClamp.make(2, 0.0)
    P = api._ptr

    def forms(pts, pnr, p=f["params"], history=True):
        h = [P(f["prev_pos"]), P(f["prev_nrm"])] if history else [None, None]
        hv = [P(prev_vis), P(prev_len)] if history else [None, None]
        hm = [P(pm), P(ps), P(prev_len)] if history else [None, None, None]
        a = api._lib.rtsh_accumulate_visibility_list_motion(api._ref(hard), api._ref(p), P(f["pos"]), P(f["nrm"]), P(lights_map), P(vis), *h, *hv,
                                                            pts, pnr, W, H, P(out_f), P(out_l), 1)
        b = api._lib.rtsh_accumulate_visibility_list_clamped_motion(api._ref(hard), api._ref(p), P(f["pos"]), P(f["nrm"]), P(lights_map), P(vis), *h,
                                                                    *hv, pts, pnr, W, H, P(out_f), P(out_l), api._ref(clamp), 1)
        c = api._lib.rtsh_accumulate_moments_soft_light_list_motion(api._ref(soft), api._ref(p), P(f["pos"]), P(f["nrm"]), P(lights_map), P(counts),
                                                                    *h, *hm, pts, pnr, W, H, P(out_m), P(out_s), P(out_l), 1)
        return a, b, c

    def untouched():
        return (out_f == 7.5).all() and (out_l == CANARY).all() and (out_m == 0xA5A5).all() and (out_s == 0xA5A5A5A5).all()

    bad_delta = tc.with_params(f["params"])
    bad_delta.eye_delta[1] = np.inf                                    # not used by the motion forms, but must still be finite
    bad_length = tc.with_params(f["params"], max_length=0)
    for what, got in (("NULL prev_points", forms(None, P(f["pnr"]))), ("NULL prev_point_normals", forms(P(f["pts"]), None)),
                      ("both NULL with a history", forms(None, None)), ("eye_delta", forms(P(f["pts"]), P(f["pnr"]), p=bad_delta)),
                      ("max_length", forms(P(f["pts"]), P(f["pnr"]), p=bad_length))):
        assert got == (1, 1, 1), (what, got)
        assert untouched(), what
    # the first frame: both planes may be NULL, and the result is the parents'
    assert forms(None, None, history=False) == (0, 0, 0)
    want = api.accumulate_moments_soft_light_list(soft, f["params"], f["pos"], f["nrm"], counts, None, lights_map)
    ms.same_planes((out_m, out_s, out_l), want, "first frame")


def test_motion_forms_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/list_motion_host.cpp: the host twins themselves (rts_scene.cpp and the shared per-pixel source, compiled into the program --
    nothing sanitized is loaded into Python) under -fsanitize=address,undefined, over the refusals and small frames in exact-size blocks."""
    exe = str(tmp_path / "list_motion_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "list_motion_host.cpp"), os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100, run.stdout[-2000:]
