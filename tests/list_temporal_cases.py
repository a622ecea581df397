"""Shared by the temporal accumulation tests (tests/test_list_temporal_host.py, tests/test_gpu_list_temporal.py): pairs of frames for
rtsh_accumulate_visibility_list* (include/rts_scene.h) and the expected planes from a float32 / uint32 / int32 numpy restatement of its
per-pixel rule, written here from the header's text and independently of the C++.  No GPU code is touched here.

A case is a dict: cur and prev G-buffers (normals, positions), lights_map, visibility, prev_visibility, prev_lengths and params.
  "awkward"    list_filter_cases.awkward as BOTH frames (NaN, Inf and huge normals and positions), wild visibility and history (NaN, Inf,
               negative, huge, denormal), lengths cycling through 0, 1, 2, 254, 255, a camera that puts some of the few finite positions
               on screen, some off it and some behind it.
  "geometric"  the world of list_filter_cases.geometric -- a floor (normal +y) that creases into a tilted wall (N.N' = 0.8), a second
               floor half a unit higher behind a step, holes of background fixed in the world -- seen from two cameras; positions are
               made analytically (ray against plane; the step has a riser), not traced.  Motions:
                 "subpixel"  the eye moves by a fraction of a pixel's footprint;
                 "pixels"    a camera looking straight down moves by (3, 8) pixels of the floor's depth: the floor lands on pixel centres
                             (one weight), the upper floor, at 2/3 of the depth, on (4.5, 12) (two weights), the wall anywhere (four);
                 "turn"      a shift of a few pixels with a small rotation;
                 "away"      the previous camera turned so far that part of the frame is off its screen and part behind it (z <= 0).
               census() asserts on the 40 x 40 "pixels" pair that each of the on-screen, normal, plane and length tests accepts at least
               50 taps and rejects at least 50 and that pixels of one, two and four non-zero weights all occur.
The cameras of the geometric pairs are built in numpy (float64, then rounded to float32), so the frames are the same bits everywhere.
Floats are compared through a uint32 view: bit for bit."""
import numpy as np

import list_filter_cases as fc
from raytracedshadows_amd import api

f32, u32, i32 = np.float32, np.uint32, np.int32
NAN, INF = np.nan, np.inf

#: W x H: list_filter_cases.FRAMES and 40 x 40 (several 16 x 16 blocks in both directions, taps crossing their edges, a partial last one)
FRAMES = fc.FRAMES + [(40, 40)]
LENGTHS = np.array([0, 1, 2, 254, 255], np.uint8)
MOTIONS = ("subpixel", "pixels", "turn", "away")
MAX_LENGTHS = (1, 2, 5, 255)
RESETS = (0, 0b101, 0xFF)
#: the world of the geometric pairs: the crease at x = XC, the step at z = ZS, holes on a lattice of HOLE units
XC, ZS, HOLE = 0.7, 0.9, 0.11

_CASES = {}


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def lengths(wh, salt=0):
    W, H = wh
    i = np.arange(H * W) + salt
    return np.ascontiguousarray(np.stack([LENGTHS[(i * (l + 1) + 3 * l) % len(LENGTHS)] for l in range(8)]).reshape(8, H, W))


def awkward(wh):
    if ("awkward", wh) not in _CASES:
        nrm, pos, _, _, lights_map, _ = fc.awkward(wh)
        wild = fc.wild_visibility(wh)
        p = api.TemporalParams.make((0.1, 0.05, 1.5), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1.0, 1.3, 0.5, 10.0, 5, 0)
        _CASES[("awkward", wh)] = _freeze(dict(nrm=nrm, pos=pos, prev_nrm=nrm, prev_pos=pos, map=lights_map, vis=wild,
                                               prev_vis=np.ascontiguousarray(wild[::-1]), prev_len=lengths(wh), params=p))
    return _CASES[("awkward", wh)]


# ------------------------------------------------------------------------------------------------- the geometric pairs
def _camera(eye, target, fovy, W, H):
    """The pinhole camera of the primary pass (vertical fov, look-at, +Y up), in float64 and rounded to float32."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = target - eye
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross([0.0, 1.0, 0.0], fwd)
    right = right / np.linalg.norm(right) if np.linalg.norm(right) > 0 else np.array([1.0, 0.0, 0.0])
    up = np.cross(fwd, right)
    tan_half = f32(np.tan(fovy * 0.5))
    return dict(eye=eye.astype(f32), fwd=fwd.astype(f32), right=right.astype(f32), up=up.astype(f32), tan_half=tan_half,
                scale_x=f32(tan_half * (f32(W) / f32(H))), scale_y=tan_half)


def _gbuffer(cam, W, H):
    """(normals, positions) of the world seen by `cam`: per pixel the nearest of floor, upper floor, wall and upper wall; positions are
    relative to the eye."""
    y, x = np.mgrid[0:H, 0:W]
    sx = ((x + 0.5) / W * 2.0 - 1.0) * np.float64(cam["scale_x"])
    sy = (1.0 - (y + 0.5) / H * 2.0) * np.float64(cam["scale_y"])
    d = cam["fwd"].astype(np.float64) + sx[..., None] * cam["right"].astype(np.float64) + sy[..., None] * cam["up"].astype(np.float64)
    o = cam["eye"].astype(np.float64)
    best = np.full((H, W), np.inf)
    nrm = np.zeros((H, W, 4), f32)
    pos = np.zeros((H, W, 4), f32)
    wall_n = np.array([-0.6, 0.8, 0.0])
    for lift, upper in ((0.0, False), (0.5, True)):
        for n, anchor, is_wall in ((np.array([0.0, 1.0, 0.0]), np.array([0.0, lift, 0.0]), False), (wall_n, np.array([XC, lift, 0.0]), True)):
            with np.errstate(all="ignore"):
                t = ((anchor - o) @ n) / (d @ n)
            hit = o + t[..., None] * d
            ok = (t > 0) & np.isfinite(t) & ((hit[..., 2] >= ZS) == upper) & ((hit[..., 0] >= XC) == is_wall) & (t < best)
            hole = (np.floor(hit[..., 0] / HOLE) + 2 * np.floor(hit[..., 2] / HOLE)) % 23 == 7
            ok = ok & (np.abs(hit[..., 0]) < 50) & (np.abs(hit[..., 2]) < 50)
            best = np.where(ok, t, best)
            facing = np.where(((d @ n) > 0)[..., None], -n, n)
            nrm[..., :3] = np.where((ok & ~hole)[..., None], facing, np.where(ok[..., None], 0, nrm[..., :3]))
            pos[..., :3] = np.where((ok & ~hole)[..., None], t[..., None] * d, np.where(ok[..., None], NAN, pos[..., :3]))
            pos[..., 3] = np.where(ok, np.where(hole, NAN, 1.0), pos[..., 3])
    n = np.array([0.0, 0.0, -1.0])                                      # the riser of the step: the plane z = ZS, half a unit high
    with np.errstate(all="ignore"):
        t = ((np.array([0.0, 0.0, ZS]) - o) @ n) / (d @ n)
    t = np.where(np.isfinite(t), t, -1.0)
    hit = o + t[..., None] * d
    foot = np.where(hit[..., 0] >= XC, 0.75 * (hit[..., 0] - XC), 0.0)
    ok = (t > 0) & np.isfinite(t) & (hit[..., 1] >= foot) & (hit[..., 1] <= foot + 0.5) & (np.abs(hit[..., 0]) < 50) & (t < best)
    facing = np.where(((d @ n) > 0)[..., None], -n, n)
    nrm[..., :3] = np.where(ok[..., None], facing, nrm[..., :3])
    pos[..., :3] = np.where(ok[..., None], t[..., None] * d, pos[..., :3])
    pos[..., 3] = np.where(ok, 1.0, pos[..., 3])
    return np.ascontiguousarray(nrm), np.ascontiguousarray(pos)


def cameras(motion, wh):
    """(current, previous) camera of a motion."""
    W, H = wh
    if motion == "pixels":                                              # straight down from 1.5 above the floor, 2 x 2 units in view
        fovy = 2.0 * np.arctan(1.0 / 1.5)
        pitch = 2.0 / H                                                 # a pixel's footprint on the floor, both axes
        cur = ((0.6, 1.5, 1.1), (0.6, 0.0, 1.1), fovy)
        # right = +x and up = +z for this camera: the previous eye 3 pixels to the left and 8 pixels up puts the floor at (+3, +8);
        # the eye is over the upper floor, so the step's riser is hidden and the lower floor next to it was covered in the previous frame
        prev = ((0.6 - 3 * pitch, 1.5, 1.1 + 8 * pitch), (0.6 - 3 * pitch, 0.0, 1.1 + 8 * pitch), fovy)
    else:
        cur = ((0.2, 1.4, -1.6), (0.7, 0.1, 0.8), 0.9)
        if motion == "subpixel":
            prev = ((0.2025, 1.401, -1.6), (0.7025, 0.101, 0.8), 0.9)
        elif motion == "turn":
            prev = ((0.33, 1.36, -1.55), (0.74, 0.12, 0.8), 0.9)
        else:
            prev = ((0.9, 0.45, 0.4), (-2.0, 0.2, -1.2), 0.9)
    return _camera(*cur, W, H), _camera(*prev, W, H)


def geometric(motion, wh):
    if (motion, wh) not in _CASES:
        W, H = wh
        cur, prev = cameras(motion, wh)
        nrm, pos = _gbuffer(cur, W, H)
        prev_nrm, prev_pos = _gbuffer(prev, W, H)
        rs = np.random.RandomState(7000 * W + H + len(motion))
        lights_map = rs.randint(0, 256, (H, W)).astype(np.uint8) | np.uint8(0x13)
        vis = rs.randint(0, 5, (8, H, W)).astype(f32) / f32(4)
        prev_vis = rs.randint(0, 1 << 20, (8, H, W)).astype(f32) / f32(1 << 20)
        p = api.TemporalParams.make(cur["eye"] - prev["eye"], prev["right"], prev["up"], prev["fwd"], prev["scale_x"], prev["scale_y"],
                                    0.9, 0.02, 5, 0)
        _CASES[(motion, wh)] = _freeze(dict(nrm=nrm, pos=pos, prev_nrm=prev_nrm, prev_pos=prev_pos, map=lights_map, vis=vis,
                                            prev_vis=prev_vis, prev_len=lengths(wh, 1), params=p))
    return _CASES[(motion, wh)]


def reverse_params(motion, wh):
    """The params of a geometric pair taken the other way round: its previous frame as the current one."""
    cur, prev = cameras(motion, wh)
    return api.TemporalParams.make(prev["eye"] - cur["eye"], cur["right"], cur["up"], cur["fwd"], cur["scale_x"], cur["scale_y"], 0.9, 0.02, 5, 0)


def case(kind, wh):
    return awkward(wh) if kind == "awkward" else geometric(kind, wh)


KINDS = ("awkward",) + MOTIONS


def with_params(p, max_length=None, reset_lights=None):
    """A copy of a TemporalParams with another max_length / reset_lights."""
    q = api.TemporalParams.from_buffer_copy(p)
    if max_length is not None:
        q.max_length = max_length
    if reset_lights is not None:
        q.reset_lights = reset_lights
    return q


# --------------------------------------------------------------------------------------- the rule, written out in float32 / uint32 / int32
def _dot3(ax, ay, az, bx, by, bz):
    out = (ax * bx + ay * by) + az * bz
    assert out.dtype == f32
    return out


def accumulate_rule(count, p, positions, normals, visibility, prev=None, lights_map=None, census=None):
    """(float32[count, H, W], uint8[count, H, W]) of the accumulation, from the header's text.  ``prev``: None (the first frame) or
    (prev_positions, prev_normals, prev_visibility, prev_lengths).  ``census``: a dict that receives [accepted, rejected] of the
    on-screen test (pixels) and of the normal, plane and length tests (taps that reached them), and the number of pixels by their count
    of non-zero weights."""
    n = np.ascontiguousarray(normals, f32)
    P = np.ascontiguousarray(positions, f32)
    H, W = n.shape[:2]
    vis = np.ascontiguousarray(visibility, f32)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    bg = (nx == 0) & (ny == 0) & (nz == 0)
    on = [~bg & (True if lights_map is None else ((np.asarray(lights_map, np.uint8) >> l) & 1) != 0) for l in range(count)]
    out = np.zeros((count, H, W), f32)
    out_len = np.zeros((count, H, W), np.uint8)
    for l in range(count):                                               # no accepted tap: the current value's bits, length 1
        out[l].view(u32)[...] = np.where(on[l], vis[l].view(u32), u32(0))
        out_len[l] = np.where(on[l], 1, 0)
    if prev is None:
        return out, out_len
    pP, pn, pvis, plen = (np.ascontiguousarray(a) for a in prev)
    assert pP.dtype == f32 and pn.dtype == f32 and pvis.dtype == f32 and plen.dtype == np.uint8
    e = [f32(p.eye_delta[i]) for i in range(3)]
    with np.errstate(all="ignore"):
        qx, qy, qz = P[..., 0] + e[0], P[..., 1] + e[1], P[..., 2] + e[2]
        z = _dot3(qx, qy, qz, *(f32(v) for v in p.prev_fwd))
        a = _dot3(qx, qy, qz, *(f32(v) for v in p.prev_right)) / z
        b = _dot3(qx, qy, qz, *(f32(v) for v in p.prev_up)) / z
        fx = (a / f32(p.prev_scale_x) + f32(1.0)) * (f32(0.5) * f32(W)) - f32(0.5)
        fy = (f32(1.0) - b / f32(p.prev_scale_y)) * (f32(0.5) * f32(H)) - f32(0.5)
        gx, gy = fx * f32(32.0) + f32(0.5), fy * f32(32.0) + f32(0.5)
        assert gx.dtype == f32 and gy.dtype == f32
        onscreen = (z > 0) & (gx >= f32(-32.0)) & (gx < f32(W) * f32(32.0)) & (gy >= f32(-32.0)) & (gy < f32(H) * f32(32.0))
        ix = np.floor(np.where(onscreen, gx, f32(0))).astype(i32)
        iy = np.floor(np.where(onscreen, gy, f32(0))).astype(i32)
        x0, y0, ax, ay = ix >> 5, iy >> 5, (ix & 31).astype(u32), (iy & 31).astype(u32)
        if census is not None:
            census.update({"onscreen": [int((onscreen & ~bg).sum()), int((~onscreen & ~bg).sum())], "normal": [0, 0], "plane": [0, 0],
                           "length": [0, 0], "weights": {}})
            nonzero = (np.where(ax == 0, 1, 2) * np.where(ay == 0, 1, 2))[onscreen & ~bg]
            for k in (1, 2, 4):
                census["weights"][k] = int((nonzero == k).sum())
        taps = []
        for k in range(4):
            tx, ty = x0 + (k & 1), y0 + (k >> 1)
            w = np.where(k & 1, ax, u32(32) - ax) * np.where(k >> 1, ay, u32(32) - ay)
            inside = onscreen & ~bg & (w != 0) & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            cx, cy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
            tn, tp = pn[cy, cx], pP[cy, cx]
            reach = inside & ~((tn[..., 0] == 0) & (tn[..., 1] == 0) & (tn[..., 2] == 0))
            normal_ok = _dot3(nx, ny, nz, tn[..., 0], tn[..., 1], tn[..., 2]) >= f32(p.normal_cos_min)
            h = _dot3(nx, ny, nz, tp[..., 0] - qx, tp[..., 1] - qy, tp[..., 2] - qz)
            plane_ok = np.abs(h) <= f32(p.plane_eps)
            geom = reach & normal_ok & plane_ok
            if census is not None:
                census["normal"][0] += int((reach & normal_ok).sum())
                census["normal"][1] += int((reach & ~normal_ok).sum())
                census["plane"][0] += int((reach & normal_ok & plane_ok).sum())
                census["plane"][1] += int((reach & normal_ok & ~plane_ok).sum())
            taps.append((geom, w.astype(u32), cy, cx))
        for l in range(count):
            if (int(p.reset_lights) >> l) & 1:
                continue
            sw = np.zeros((H, W), u32)
            sv = np.zeros((H, W), f32)
            m = np.full((H, W), 255, u32)
            for geom, w, cy, cx in taps:
                length = plen[l][cy, cx].astype(u32)
                acc = geom & on[l] & (length != 0)
                if census is not None:
                    census["length"][0] += int((geom & on[l] & (length != 0)).sum())
                    census["length"][1] += int((geom & on[l] & (length == 0)).sum())
                sw = np.where(acc, sw + w, sw).astype(u32)
                sv = np.where(acc, sv + w.astype(f32) * pvis[l][cy, cx], sv)
                assert sv.dtype == f32
                m = np.where(acc, np.minimum(m, length), m)
            nl = np.minimum(m + u32(1), u32(p.max_length))
            blend = on[l] & (sw != 0) & (nl != 1)
            before = sv / sw.astype(f32)
            cur = vis[l]
            value = before + (cur - before) * (f32(1.0) / nl.astype(f32))
            assert value.dtype == f32
            bits = np.where(np.isnan(value), u32(0x7FC00000), value.view(u32))              # a blended NaN is the canonical quiet NaN
            out[l].view(u32)[...] = np.where(blend, bits, out[l].view(u32))
            out_len[l] = np.where(on[l] & (sw != 0), nl, out_len[l]).astype(np.uint8)
    return out, out_len


def rule_of(c, count, p=None, with_map=True, first=False):
    """accumulate_rule over a case."""
    prev = None if first else (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"])
    return accumulate_rule(count, p or c["params"], c["pos"], c["nrm"], c["vis"], prev, c["map"] if with_map else None)


def census():
    """The census of the 40 x 40 "pixels" pair, asserted: every test accepts and rejects, every number of weights occurs."""
    c = geometric("pixels", (40, 40))
    out = {}
    accumulate_rule(8, c["params"], c["pos"], c["nrm"], c["vis"], (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"]), c["map"], out)
    for test in ("onscreen", "normal", "plane", "length"):
        assert out[test][0] >= 50 and out[test][1] >= 50, (test, out)
    assert all(out["weights"][k] > 0 for k in (1, 2, 4)), out
    return out


def the_list(count):
    return fc.the_list("hard", {1: "1", 3: "3", 8: "8"}[count])


def same_bits(got, want, what):
    fc.same_bits(got[0], want[0], (what, "visibility"))
    assert got[1].dtype == np.uint8 and (got[1] == want[1]).all(), (what, "lengths", np.argwhere(got[1] != want[1])[:6].tolist())
