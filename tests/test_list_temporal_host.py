"""CPU: the host twin of the temporal accumulation of a light list's visibility (rtsh_accumulate_visibility_list) against the numpy
rule of tests/list_temporal_cases.py, bit for bit -- and what pins the rule: the three anchors (the still-camera one on real
G-buffers), the ping-pong chain, the in-place form, every refusal, the camera basis and a sanitized stand-alone host program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import list_combine_cases as lc
import list_temporal_cases as tc
from raytracedshadows_amd import api, scenes

f32, u32 = np.float32, np.uint32
INVALID = 1


def _prev(c):
    return (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"])


def _twin(c, count, p=None, with_map=True, first=False, threads=0):
    return api.accumulate_visibility_list(tc.the_list(count), p or c["params"], c["pos"], c["nrm"], c["vis"], None if first else _prev(c),
                                          c["map"] if with_map else None, threads)


@pytest.mark.parametrize("kind", tc.KINDS)
@pytest.mark.parametrize("wh", tc.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_equals_the_numpy_rule(wh, kind):
    """Awkward and geometric pairs; lists of 1, 3 and 8 lights, with and without a map; max_length 1, 2, 5 and 255; reset_lights 0,
    0b101 and all ones; and the first frame."""
    c = tc.case(kind, wh)
    for count in (1, 3, 8):
        for with_map in (True, False):
            for max_length in tc.MAX_LENGTHS:
                for reset in tc.RESETS:
                    if not with_map and (max_length, reset) not in ((5, 0), (255, 0b101)):
                        continue
                    p = tc.with_params(c["params"], max_length, reset)
                    tc.same_bits(_twin(c, count, p, with_map), tc.rule_of(c, count, p, with_map), (kind, wh, count, with_map, max_length, reset))
        tc.same_bits(_twin(c, count, first=True), tc.rule_of(c, count, first=True), (kind, wh, count, "first frame"))


def test_the_census_of_the_largest_pair():
    """Every test of the rule accepts and rejects at least 50 taps, pixels of one, two and four weights occur (asserted in census()),
    the "away" pair has pixels off the previous screen and behind the previous camera -- and the pass is no identity there."""
    out = tc.census()
    assert out["weights"][1] > 0 and out["weights"][2] > 0 and out["weights"][4] > 0
    c = tc.geometric("pixels", (40, 40))
    got = _twin(c, 8)
    assert (got[0] != c["vis"]).any() and set(np.unique(got[1])) >= {0, 1, 2, 3, 5}
    a = tc.geometric("away", (40, 40))
    p = a["params"]
    q = a["pos"][..., :3] + np.array(list(p.eye_delta), f32)
    z = q @ np.array(list(p.prev_fwd), f32)
    solid = (a["nrm"][..., :3] != 0).any(axis=-1)
    assert (z[solid] <= 0).sum() >= 50 and (z[solid] > 0).sum() >= 50


def test_threads_change_nothing():
    c = tc.geometric("turn", (40, 40))
    tc.same_bits(_twin(c, 8, threads=7), _twin(c, 8, threads=1), "7 threads")


@pytest.mark.parametrize("kind", ["awkward", "pixels", "turn"])
def test_anchor_no_history_gives_the_current_bits(kind):
    """Anchors 1 and 3: max_length 1, all-ones reset_lights or the first frame give visibility's bits and length 1 at active pixels
    (+0 and 0 elsewhere); a light whose reset bit is set gets that whatever the others do."""
    for wh in ((17, 15), (40, 40)):
        c = tc.case(kind, wh)
        background = (c["nrm"][..., :3] == 0).all(axis=-1)
        for with_map in (True, False):
            on = [~background & ((((c["map"] >> l) & 1) != 0) if with_map else True) for l in range(8)]
            want = np.stack([np.where(on[l], c["vis"][l].view(u32), u32(0)) for l in range(8)]).view(f32)
            want_len = np.stack([on[l].astype(np.uint8) for l in range(8)])
            closed = [("max_length 1", tc.with_params(c["params"], 1, 0), False), ("all reset", tc.with_params(c["params"], 255, 0xFF), False),
                      ("all reset, high bits too", tc.with_params(c["params"], 255, 0xFFFFFFFF), False), ("first frame", c["params"], True)]
            for what, p, first in closed:
                tc.same_bits(_twin(c, 8, p, with_map, first), (want, want_len), (kind, wh, with_map, what))
            p = tc.with_params(c["params"], 255, 0b101)
            got, free = _twin(c, 8, p, with_map), _twin(c, 8, tc.with_params(c["params"], 255, 0), with_map)
            for l in range(8):
                if l in (0, 2):
                    tc.same_bits((got[0][l], got[1][l]), (want[l], want_len[l]), (kind, wh, with_map, "reset light", l))
                else:
                    tc.same_bits((got[0][l], got[1][l]), (free[0][l], free[1][l]), (kind, wh, with_map, "free light", l))
            if kind != "awkward":
                assert (free[1][0] > 1).any() and (free[0][0] != want[0]).any()


_GBUFFERS = {}


def _real_gbuffer(name, wh):
    if (name, wh) not in _GBUFFERS:
        sc = scenes.cornell() if name == "cornell" else scenes.terrain(23)
        verts, idx = sc.flat()
        packed = api.BVHBuilder().build(verts, 8, idx, sc.triangle_count).m_packedNodes
        pos, nrm, _ = api.primary_gbuffer(packed, sc.eye, sc.target, sc.fovy, wh[0], wh[1])
        _GBUFFERS[(name, wh)] = (sc, pos, nrm)
    return _GBUFFERS[(name, wh)]


@pytest.mark.parametrize("wh", [(128, 128), (1920, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["cornell", "terrain"])
def test_anchor_still_camera_on_real_gbuffers(name, wh):
    """Anchor 2: params from api.camera_basis of the camera the G-buffer was made with, eye_delta 0.  EVERY non-background pixel has
    ax == ay == 0 and lands on itself, and six chained frames with max_length 4 equal the per-pixel recurrence bit for bit."""
    W, H = wh
    sc, pos, nrm = _real_gbuffer(name, wh)
    cam = (sc.eye, sc.target, sc.fovy)
    p = api.TemporalParams.from_cameras(cam, cam, W, H, 0.9, 1e-3, 4, 0)
    assert list(p.eye_delta) == [0.0, 0.0, 0.0]
    solid = (nrm[..., :3] != 0).any(axis=-1)
    assert solid.sum() > 30                                             # (at 1920 x 8 the scene is a sliver of the strip)
    # the landing, restated: the header's float32 steps
    b = api.camera_basis(*cam, W, H)
    dot3 = lambda v: (pos[..., 0] * v[0] + pos[..., 1] * v[1]) + pos[..., 2] * v[2]
    with np.errstate(all="ignore"):
        z = dot3(b["fwd"])
        fx = ((dot3(b["right"]) / z) / f32(p.prev_scale_x) + f32(1)) * (f32(0.5) * f32(W)) - f32(0.5)
        fy = (f32(1) - (dot3(b["up"]) / z) / f32(p.prev_scale_y)) * (f32(0.5) * f32(H)) - f32(0.5)
        ix = np.floor(fx * f32(32) + f32(0.5)).astype(np.int64)
        iy = np.floor(fy * f32(32) + f32(0.5)).astype(np.int64)
    assert fx.dtype == f32 and fy.dtype == f32
    yy, xx = np.mgrid[0:H, 0:W]
    assert (ix[solid] == xx[solid] * 32).all() and (iy[solid] == yy[solid] * 32).all(), "a pixel does not land on itself"
    lst = tc.the_list(3)
    rs = np.random.RandomState(5)
    history = lengths = None
    want = None
    for k in range(1, 7):
        cur = (rs.randint(0, 5, (3, H, W)).astype(f32) / f32(4)) if k != 3 else rs.randint(0, 1 << 16, (3, H, W)).astype(f32) / f32(3 << 14)
        prev = None if k == 1 else (pos, nrm, history, lengths)
        history, lengths = api.accumulate_visibility_list(lst, p, pos, nrm, cur, prev)
        n = min(k, 4)
        want = cur if k == 1 else want + (cur - want) * (f32(1.0) / f32(n))
        assert want.dtype == f32
        for l in range(3):
            tc.same_bits((history[l], lengths[l]), (np.where(solid, want[l], f32(0)), np.where(solid, n, 0).astype(np.uint8)), (name, wh, k, l))


def _plane_gbuffer(cam, W, H):
    """A G-buffer that fills the frame, made as the primary pass makes one -- the pixel's direction in float32, operation for
    operation, times a ray parameter -- over a tilted plane: t varies from 2 to 9 along the strip and from row to row."""
    b = api.camera_basis(*cam, W, H)
    y, x = np.mgrid[0:H, 0:W]
    sx = (((x.astype(f32) + f32(0.5)) / f32(W) * f32(2) - f32(1)) * b["tan_half"]) * b["aspect"]
    sy = (f32(1) - (y.astype(f32) + f32(0.5)) / f32(H) * f32(2)) * b["tan_half"]
    assert sx.dtype == f32 and sy.dtype == f32
    t = (f32(2) + f32(7) * ((x * 37 + y * 11) % 101).astype(f32) / f32(100)).astype(f32)
    pos, nrm = np.ones((H, W, 4), f32), np.zeros((H, W, 4), f32)
    for i in range(3):
        d = (b["fwd"][i] + b["right"][i] * sx) + b["up"][i] * sy
        pos[..., i] = d * t
    nrm[..., :3] = -b["fwd"]
    return pos, nrm


def test_anchor_still_camera_across_the_whole_width():
    """Anchor 2 where the real scenes leave the 1920 x 8 strip empty: a synthetic plane that fills every column, depths from 2 to 9,
    under a camera turned off the axes.  EVERY pixel, columns 0 and 1919 included, keeps its history: after four chained frames every
    length is 4 and the planes equal the per-pixel recurrence bit for bit.  (The strip's aspect of 240 is about as far as the anchor
    reaches: the float32 inverse misses a centre by up to 0.0084 pixel here, against 0.0004 at 1920 x 1080, and the miss grows with
    W / H -- DESIGN.md 4.23.)"""
    wh = W, H = 1920, 8
    cam = ((1.5, 2.0, -3.0), (0.25, 0.5, 1.0), 0.9)
    pos, nrm = _plane_gbuffer(cam, W, H)
    p = api.TemporalParams.from_cameras(cam, cam, W, H, 0.9, 1e-3, 8, 0)
    lst = tc.the_list(1)
    rs = np.random.RandomState(W)
    history = lengths = want = None
    for k in range(1, 5):
        cur = rs.randint(0, 5, (1, H, W)).astype(f32) / f32(4)
        history, lengths = api.accumulate_visibility_list(lst, p, pos, nrm, cur, None if k == 1 else (pos, nrm, history, lengths))
        want = cur if k == 1 else want + (cur - want) * (f32(1.0) / f32(k))
        assert (lengths == k).all(), (wh, k, np.argwhere(lengths != k)[:6].tolist())
        tc.same_bits((history, lengths), (want, np.full((1, H, W), k, np.uint8)), (wh, k))


def test_chain_of_four_frames():
    """Four frames ping-ponged through the twin equal four through the rule: this frame's output is the next frame's history, and the
    cameras alternate between the pair's two."""
    for kind in ("subpixel", "turn"):
        c = tc.geometric(kind, (40, 40))
        back = tc.reverse_params(kind, (40, 40))
        lst = tc.the_list(3)
        frames = [(c["pos"], c["nrm"]), (c["prev_pos"], c["prev_nrm"])]
        got = want = None
        for k in range(4):
            pos, nrm = frames[(k + 1) % 2]
            ppos, pnrm = frames[k % 2]
            p = tc.with_params(c["params"] if k % 2 else back, 3, 0b010 if k == 2 else 0)
            vis = np.ascontiguousarray(np.roll(c["vis"], k, axis=2))
            got = api.accumulate_visibility_list(lst, p, pos, nrm, vis, None if k == 0 else (ppos, pnrm) + got, c["map"])
            want = tc.accumulate_rule(3, p, pos, nrm, vis, None if k == 0 else (ppos, pnrm) + want, c["map"])
            tc.same_bits(got, want, (kind, "frame", k))
        assert got[1].max() == 3


def test_in_place_equals_out_of_place():
    """visibility_out == visibility is allowed: a pixel reads only its own current value, before it writes."""
    lib = api._lib
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for kind in ("awkward", "turn"):
        c = tc.case(kind, (33, 18))
        lst = tc.the_list(8)
        want = _twin(c, 8)
        vis, lengths = c["vis"].copy(), np.zeros((8, 18, 33), np.uint8)
        arrays = [np.ascontiguousarray(c[k]) for k in ("pos", "nrm", "map", "prev_pos", "prev_nrm", "prev_vis", "prev_len")]
        assert lib.rtsh_accumulate_visibility_list(C.byref(lst), C.byref(c["params"]), ptr(arrays[0]), ptr(arrays[1]), ptr(arrays[2]), ptr(vis),
                                                   ptr(arrays[3]), ptr(arrays[4]), ptr(arrays[5]), ptr(arrays[6]), 33, 18, ptr(vis),
                                                   ptr(lengths), 3) == 0
        tc.same_bits((vis, lengths), want, (kind, "in place"))


def test_planes_from_the_count_up_are_never_touched():
    c = tc.geometric("turn", (17, 15))
    got = np.full((8, 15, 17), 7.5, f32), np.full((8, 15, 17), 0xAB, np.uint8)
    lst = tc.the_list(3)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    vis, pvis, plen = c["vis"].copy(), c["prev_vis"].copy(), c["prev_len"].copy()
    vis[3:], pvis[3:], plen[3:] = np.nan, np.nan, 0
    a = [np.ascontiguousarray(c[k]) for k in ("pos", "nrm", "map", "prev_pos", "prev_nrm")]
    assert api._lib.rtsh_accumulate_visibility_list(C.byref(lst), C.byref(c["params"]), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(vis), ptr(a[3]),
                                                    ptr(a[4]), ptr(pvis), ptr(plen), 17, 15, ptr(got[0]), ptr(got[1]), 0) == 0
    tc.same_bits((got[0][:3], got[1][:3]), tc.rule_of(c, 3), "planes below the count")
    assert (got[0][3:] == 7.5).all() and (got[1][3:] == 0xAB).all()


def _bad_params(good):
    out = [None]
    for field, value in (("max_length", 0), ("max_length", 256), ("max_length", 0xFFFFFFFF), ("normal_cos_min", np.nan),
                         ("normal_cos_min", np.inf), ("plane_eps", -np.inf), ("plane_eps", np.nan), ("prev_scale_x", 0.0),
                         ("prev_scale_x", -1.0), ("prev_scale_x", np.inf), ("prev_scale_y", np.nan), ("prev_scale_y", -0.0)):
        p = tc.with_params(good)
        setattr(p, field, value)
        out.append(p)
    for field in ("eye_delta", "prev_right", "prev_up", "prev_fwd"):
        for i, value in ((0, np.nan), (1, np.inf), (2, -np.inf)):
            p = tc.with_params(good)
            getattr(p, field)[i] = value
            out.append(p)
    return out


def test_refusals_write_nothing():
    lib = api._lib
    c = tc.geometric("turn", (16, 16))
    a = {k: np.ascontiguousarray(c[k]) for k in ("pos", "nrm", "map", "vis", "prev_pos", "prev_nrm", "prev_vis", "prev_len")}
    out, out_len = np.full((8, 16, 16), 7.5, f32), np.full((8, 16, 16), 0xAB, np.uint8)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    ref = lambda s: C.byref(s) if s is not None else None
    good, lst = c["params"], tc.the_list(3)

    def call(lst_=lst, p=good, W=16, H=16, o=out, ol=out_len, **swap):
        b = dict(a, **swap)
        return lib.rtsh_accumulate_visibility_list(ref(lst_), ref(p), ptr(b["pos"]), ptr(b["nrm"]), ptr(b["map"]), ptr(b["vis"]), ptr(b["prev_pos"]),
                                                   ptr(b["prev_nrm"]), ptr(b["prev_vis"]), ptr(b["prev_len"]), W, H, ptr(o), ptr(ol), 0)

    assert call() == 0 and call(map=None) == 0
    assert call(prev_pos=None, prev_nrm=None, prev_vis=None, prev_len=None) == 0
    out[:], out_len[:] = 7.5, 0xAB
    for bad in lc.bad_lists()[0]:
        assert call(lst_=bad) == INVALID
    for p in _bad_params(good):
        assert call(p=p) == INVALID, p and [p.max_length, p.normal_cos_min, p.plane_eps, p.prev_scale_x, p.prev_scale_y]
    for name in ("pos", "nrm", "vis"):
        assert call(**{name: None}) == INVALID, name
    assert call(o=None) == INVALID and call(ol=None) == INVALID
    prevs = ("prev_pos", "prev_nrm", "prev_vis", "prev_len")
    for keep in range(1, 15):                                           # some but not all of the four
        assert call(**{name: None for i, name in enumerate(prevs) if not (keep >> i) & 1}) == INVALID, keep
    for W, H in ((0, 16), (16, 0), (65537, 1), (1, 65537), (0xFFFFFFFF, 1)):
        assert call(W=W, H=H) == INVALID, (W, H)
    assert call(prev_vis=out) == INVALID and call(prev_len=out_len) == INVALID      # history must ping-pong
    assert (out == 7.5).all() and (out_len == 0xAB).all()
    with pytest.raises(api.RtsError):
        api.accumulate_visibility_list(lst, good, None, a["nrm"], a["vis"])
    with pytest.raises(api.RtsError):
        api.accumulate_visibility_list(lst, good, a["pos"], a["nrm"], a["vis"][:2])


def test_camera_basis():
    """rtsh_camera_basis: an orthonormal basis, tanHalf and aspect of the camera; the straight-down fallback; its refusals; and
    TemporalParams.from_cameras built on it."""
    b = api.camera_basis((1, 2, 3), (0, 0, 0), 0.8, 64, 32)
    for u in ("fwd", "right", "up"):
        assert abs(float(b[u] @ b[u]) - 1) < 1e-6
    assert abs(float(b["fwd"] @ b["right"])) < 1e-6 and abs(float(b["fwd"] @ b["up"])) < 1e-6 and b["aspect"] == 2.0
    assert abs(float(b["tan_half"]) - np.tan(0.4)) < 1e-6 and (b["eye"] == np.array([1, 2, 3], f32)).all()
    down = api.camera_basis((0, 5, 0), (0, 0, 0), 0.8, 8, 8)
    assert list(down["right"]) == [1, 0, 0] and list(down["fwd"]) == [0, -1, 0] and list(down["up"]) == [0, 0, 1]
    p = api.TemporalParams.from_cameras(((1, 2, 3), (0, 0, 0), 0.8), ((0.5, 2, 3), (0, 0, 0), 0.7), 64, 32, max_length=9, reset_lights=5)
    q = api.camera_basis((0.5, 2, 3), (0, 0, 0), 0.7, 64, 32)
    assert list(p.eye_delta) == [0.5, 0, 0] and list(p.prev_fwd) == list(q["fwd"]) and p.prev_scale_y == q["tan_half"]
    assert p.prev_scale_x == f32(q["tan_half"] * q["aspect"]) and p.max_length == 9 and p.reset_lights == 5
    assert C.sizeof(api.TemporalParams) == 80
    out = np.zeros(14, f32)
    e = np.zeros(3, f32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    lib = api._lib
    assert lib.rtsh_camera_basis(None, ptr(e), 0.8, 8, 8, ptr(out)) == INVALID and lib.rtsh_camera_basis(ptr(e), None, 0.8, 8, 8, ptr(out)) == INVALID
    assert lib.rtsh_camera_basis(ptr(e), ptr(e), 0.8, 8, 8, None) == INVALID and lib.rtsh_camera_basis(ptr(e), ptr(e), 0.8, 0, 8, ptr(out)) == INVALID
    assert lib.rtsh_camera_basis(ptr(e), ptr(e), 0.8, 8, 0, ptr(out)) == INVALID and (out == 0).all()


def test_list_temporal_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/list_temporal_host.cpp: the host twin itself (rts_scene.cpp and the shared per-pixel source, compiled into the program
    -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow, over every refusal and over
    small frames of awkward texels whose buffers are heap blocks of exactly the size the header states."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "list_temporal_host")
    csrc = os.path.join(root, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(root, "tests", "cpp", "list_temporal_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 1000, run.stdout[-2000:]
