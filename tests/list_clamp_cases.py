"""Shared by the clamped temporal accumulation tests (tests/test_list_clamp_host.py, tests/test_gpu_list_clamp.py): the cases for
rtsh_accumulate_visibility_list_clamped* (include/rts_scene.h) and the expected planes from a float32 / uint32 / int64 numpy restatement
of the WHOLE clamped rule, written here from the header's text and independently of the C++.  No GPU code is touched here.

Cases: the pairs of tests/list_temporal_cases.py as they are (the "awkward" pair and the four motions, every frame of its FRAMES), and
"biting" variants of the geometric pairs, kind "bite-<motion>":
  * the history is the CURRENT plane plus an offset of +-3, the sign alternating in cells of 4 x 4 pixels and from light to light: the
    current planes lie in [0, 1], so the history lies outside any window's range and the clamp bites from above and from below;
  * about one history value in six is the current plane's own (inside most boxes: left alone);
  * NaN, +Inf, -Inf and -0 are sprinkled into current and history, a few per cent each;
  * a 9 x 9 patch of NaN in every current plane (where the frame has room), so that some blended pixel's box is EMPTY at every radius;
  * the background holes and the map holes of the geometric pair lie inside the windows as they are.
check_huge_margin() asserts that with a margin of 3.0e38 the rule here equals list_temporal_cases.accumulate_rule on the finite
geometric pairs; census() asserts on the biting 40 x 40 "pixels" pair, for r = 1 and r = 4 and from the numpy rule alone, that every
branch of the clamp is taken often enough.  Floats are compared through a uint32 view: bit for bit."""
import numpy as np

import list_temporal_cases as tc
from raytracedshadows_amd import api

f32, u32, i32, i64 = np.float32, np.uint32, np.int32, np.int64

FRAMES = tc.FRAMES
RADII = (0, 1, 2, 4)
MARGINS = (0.0, 0.125, 3.0e38)
BITE_KINDS = tuple("bite-" + m for m in tc.MOTIONS)
KINDS = tc.KINDS + BITE_KINDS

_CASES = {}


def biting(motion, wh):
    if (motion, wh) not in _CASES:
        W, H = wh
        c = dict(tc.geometric(motion, wh))
        rs = np.random.RandomState(31 * W + H + len(motion))
        vis = c["vis"].copy()
        y, x = np.mgrid[0:H, 0:W]
        sign = np.stack([np.where(((x // 4 + y // 4 + l) & 1) != 0, f32(3), f32(-3)) for l in range(8)]).astype(f32)
        hist = (vis + sign).astype(f32)
        own = rs.randint(0, 6, vis.shape) == 0
        hist[own] = vis[own]
        for plane in (vis, hist):
            pick = rs.randint(0, 100, plane.shape)
            plane[pick == 0] = np.nan
            plane[pick == 1] = np.inf
            plane[pick == 2] = -np.inf
            plane[pick == 3] = f32(-0.0)
        if W >= 9 and H >= 9:
            cx, cy = min(12, W - 5), min(12, H - 5)
            vis[:, cy - 4:cy + 5, cx - 4:cx + 5] = np.nan
        c["vis"], c["prev_vis"] = vis, hist
        _CASES[(motion, wh)] = tc._freeze(c)
    return _CASES[(motion, wh)]


def case(kind, wh):
    return biting(kind[5:], wh) if kind.startswith("bite-") else tc.case(kind, wh)


def clamp_of(radius, margin=0.0):
    return api.HistoryClamp.make(radius, margin)


# --------------------------------------------------------------------------------------- the rule, written out in float32 / uint32 / int64
def _dot3(ax, ay, az, bx, by, bz):
    out = (ax * bx + ay * by) + az * bz
    assert out.dtype == f32
    return out


def box_rule(on_l, vis_l, radius):
    """(any, lo, hi, cut, dull) of one light: any = the window has a contributing tap; lo, hi = float32 of the smallest and largest key
    (arbitrary where not any); cut = the window leaves the frame; dull = it holds a tap inside the frame that does not contribute."""
    H, W = vis_l.shape
    u = vis_l.view(u32).astype(i64)
    key = np.where((u >> 31) != 0, u ^ 0xFFFFFFFF, u ^ 0x80000000)                      # ORDER
    contributes = on_l & ~(vis_l != vis_l)
    r = radius
    pad = lambda a, fill: np.pad(a, r, constant_values=fill) if r else a
    small, large, there = pad(np.where(contributes, key, 1 << 40), 1 << 40), pad(np.where(contributes, key, -1), -1), pad(contributes, False)
    inside = pad(np.ones((H, W), bool), False)
    lo, hi = np.full((H, W), 1 << 40, i64), np.full((H, W), -1, i64)
    cut, dull = np.zeros((H, W), bool), np.zeros((H, W), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            s = (slice(dy, dy + H), slice(dx, dx + W))
            lo, hi = np.minimum(lo, small[s]), np.maximum(hi, large[s])
            cut |= ~inside[s]
            dull |= inside[s] & ~there[s]
    some = hi >= 0
    unkey = lambda k: np.where((k >> 31) != 0, k ^ 0x80000000, k ^ 0xFFFFFFFF).astype(u32).view(f32)
    return some, unkey(np.where(some, lo, 0x80000000)), unkey(np.where(some, hi, 0x80000000)), cut, dull


def accumulate_rule_clamped(count, p, positions, normals, visibility, prev, lights_map, radius, margin, census=None):
    """(float32[count, H, W], uint8[count, H, W]) of the clamped accumulation, from the header's text.  ``prev``: None (the first frame)
    or (prev_positions, prev_normals, prev_visibility, prev_lengths).  ``census``: a dict that receives, over the blended (pixel, light)
    pairs, how many were clamped from above and from below, left alone, had a window cut by the frame edge, had a window with a tap
    inside the frame that does not contribute, and had an empty box."""
    n = np.ascontiguousarray(normals, f32)
    P = np.ascontiguousarray(positions, f32)
    H, W = n.shape[:2]
    vis = np.ascontiguousarray(visibility, f32)
    margin = f32(margin)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    bg = (nx == 0) & (ny == 0) & (nz == 0)
    on = [~bg & (np.ones((H, W), bool) if lights_map is None else ((np.asarray(lights_map, np.uint8) >> l) & 1) != 0) for l in range(count)]
    out = np.zeros((count, H, W), f32)
    out_len = np.zeros((count, H, W), np.uint8)
    for l in range(count):                                               # INACTIVE, and the pass-through: the current bits, length 1
        out[l].view(u32)[...] = np.where(on[l], vis[l].view(u32), u32(0))
        out_len[l] = np.where(on[l], 1, 0)
    if census is not None:
        census.update(blended=0, above=0, below=0, alone=0, cut=0, dull=0, empty=0)
    if prev is None:
        return out, out_len
    pP, pn, pvis, plen = (np.ascontiguousarray(a) for a in prev)
    assert pP.dtype == f32 and pn.dtype == f32 and pvis.dtype == f32 and plen.dtype == np.uint8
    e = [f32(p.eye_delta[i]) for i in range(3)]
    with np.errstate(all="ignore"):
        qx, qy, qz = P[..., 0] + e[0], P[..., 1] + e[1], P[..., 2] + e[2]                 # REPROJECT
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
        taps = []
        for k in range(4):                                               # the four taps in their order; the geometry of a tap
            tx, ty = x0 + (k & 1), y0 + (k >> 1)
            w = np.where(k & 1, ax, u32(32) - ax) * np.where(k >> 1, ay, u32(32) - ay)
            inside = onscreen & ~bg & (w != 0) & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            cx, cy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
            tn, tp = pn[cy, cx], pP[cy, cx]
            reach = inside & ~((tn[..., 0] == 0) & (tn[..., 1] == 0) & (tn[..., 2] == 0))
            normal_ok = _dot3(nx, ny, nz, tn[..., 0], tn[..., 1], tn[..., 2]) >= f32(p.normal_cos_min)
            plane_ok = np.abs(_dot3(nx, ny, nz, tp[..., 0] - qx, tp[..., 1] - qy, tp[..., 2] - qz)) <= f32(p.plane_eps)
            taps.append((reach & normal_ok & plane_ok, w.astype(u32), cy, cx))
        for l in range(count):
            if (int(p.reset_lights) >> l) & 1:
                continue
            sw = np.zeros((H, W), u32)
            sv = np.zeros((H, W), f32)
            m = np.full((H, W), 255, u32)
            for geom, w, cy, cx in taps:                                 # BLEND
                length = plen[l][cy, cx].astype(u32)
                acc = geom & on[l] & (length != 0)
                sw = np.where(acc, sw + w, sw).astype(u32)
                sv = np.where(acc, sv + w.astype(f32) * pvis[l][cy, cx], sv)
                assert sv.dtype == f32
                m = np.where(acc, np.minimum(m, length), m)
            nl = np.minimum(m + u32(1), u32(p.max_length))
            blend = on[l] & (sw != 0) & (nl != 1)
            before = sv / sw.astype(f32)
            some, lo, hi, cut, dull = box_rule(on[l], vis[l], radius)    # BOX
            lo_m, hi_m = lo - margin, hi + margin                       # CLAMP
            assert lo_m.dtype == f32 and hi_m.dtype == f32
            below, above = some & (before < lo_m), some & ~(before < lo_m) & (before > hi_m)
            clamped = np.where(below, lo_m, np.where(above, hi_m, before))
            cur = vis[l]
            value = clamped + (cur - clamped) * (f32(1.0) / nl.astype(f32))
            assert value.dtype == f32
            bits = np.where(value != value, u32(0x7FC00000), value.view(u32))                # a blended NaN is the canonical quiet NaN
            out[l].view(u32)[...] = np.where(blend, bits, out[l].view(u32))
            out_len[l] = np.where(on[l] & (sw != 0), nl, out_len[l]).astype(np.uint8)
            if census is not None:
                for name, mask in (("blended", blend), ("above", blend & above), ("below", blend & below),
                                   ("alone", blend & some & ~above & ~below), ("cut", blend & cut), ("dull", blend & dull),
                                   ("empty", blend & ~some)):
                    census[name] += int(mask.sum())
    return out, out_len


def rule_of(c, count, radius, margin, p=None, with_map=True, first=False, census=None):
    """accumulate_rule_clamped over a case."""
    prev = None if first else (c["prev_pos"], c["prev_nrm"], c["prev_vis"], c["prev_len"])
    return accumulate_rule_clamped(count, p or c["params"], c["pos"], c["nrm"], c["vis"], prev, c["map"] if with_map else None, radius, margin,
                                   census)


def check_huge_margin():
    """Anchor 1 of the numpy rule itself: a margin of 3.0e38 over the finite geometric pairs gives list_temporal_cases.accumulate_rule."""
    for motion in tc.MOTIONS:
        for wh in ((7, 9), (33, 18), (40, 40)):
            c = tc.geometric(motion, wh)
            assert np.isfinite(c["vis"]).all() and np.isfinite(c["prev_vis"]).all()
            for radius in RADII:
                for with_map in (True, False):
                    tc.same_bits(rule_of(c, 8, radius, 3.0e38, with_map=with_map), tc.rule_of(c, 8, with_map=with_map), (motion, wh, radius, with_map))


def census():
    """The census of the biting 40 x 40 "pixels" pair for r = 1 and r = 4, asserted: among the blended (pixel, light) pairs at least a
    quarter are clamped from above, at least a quarter from below, at least 50 are left alone, at least 50 have a window cut by the
    frame edge, at least 50 a window with a non-contributing tap, and at least one an empty box."""
    out = {}
    c = biting("pixels", (40, 40))
    for radius in (1, 4):
        got = {}
        rule_of(c, 8, radius, 0.0, census=got)
        assert got["blended"] >= 1000, got
        assert 4 * got["above"] >= got["blended"] and 4 * got["below"] >= got["blended"], (radius, got)
        assert got["alone"] >= 50 and got["cut"] >= 50 and got["dull"] >= 50 and got["empty"] >= 1, (radius, got)
        out[radius] = got
    return out


the_list = tc.the_list
same_bits = tc.same_bits
