"""Shared by the list filter tests (tests/test_list_filter_host.py, tests/test_gpu_list_filter.py): frames for the filter of a light
list's planes (include/rts_scene.h, rtsh_filter_light_list* / rtsh_filter_soft_light_list*) and for the visibility combine
(rtsh_combine_visibility_list*), and the expected floats and bytes from float32 / uint32 numpy restatements of their per-pixel rules,
written here from the header's text and independently of the C++.  No GPU code is touched here.

Two kinds of frame, each (normals, positions, planes[8], mask, lights_map, distances[8]) and read-only:
  "awkward"    list_combine_cases.frame: NaN, Inf and huge normals and positions, bytes above the sample counts, arbitrary maps and
               masks; its distance planes cycle through +Inf, +0, finite values, NaN, -0, a negative and a denormal.
  "geometric"  a floor (normal +y) that creases into a tilted wall (N.N' = 0.8) along a column, with a depth step (a second floor, half
               a unit higher) along a row, a band of background, and planes that are uniform per light over some 16 x 16 blocks'
               windows and not over their neighbours' (the device form's shortcut).  With PARAMS the normal test rejects the taps
               across the crease, the plane test those across the step, and the spread test (distances of +Inf, +0, 0.15 and 3)
               the far taps of a near blocker; geometric() asserts on its largest frame that each of the three tests accepts some taps
               and rejects some, so that a frame where a test never fires cannot pass unnoticed.
Floats are compared through a uint32 view: bit for bit."""
import numpy as np

import list_combine_cases as lc
import scene_pass_cases as sp
from raytracedshadows_amd import api

f32, u32 = np.float32, np.uint32
NAN, INF = np.nan, np.inf

#: W x H: one pixel, one row, one column, odd sizes, exactly one block, just over and under one, several blocks, a tall sliver
FRAMES = [(1, 1), (1, 5), (5, 1), (7, 9), (16, 16), (17, 15), (33, 18), (3, 333)]
#: R = 8 is wider than several of the frames
RADII = [0, 1, 2, 8]
#: distance words of the awkward frames
DISTANCES = np.array([INF, 0.0, 0.5, 3.0, NAN, -0.0, -1.0, 1e30, 1e-41, 0.125], f32)
#: pixel pitch of the geometric frames in world units
STEP = 0.1


def params(radius, kind="geometric"):
    """The FilterParams of a run: thresholds that split the geometric frame's taps; for the awkward frames a wide plane test (their
    positions are units apart) and spreads from 0 to large."""
    if kind == "geometric":
        return api.FilterParams.make(radius, 0.9, 0.02, [0.5, 0.25, 1.0, 0.0, 0.5, 2.0, 0.125, 0.75])
    return api.FilterParams.make(radius, 0.5, 10.0, [0.5, 0.0, 3.0, 1e30, 1e-3, 2.0, 1.0, 0.25])


_FRAMES = {}


def _freeze(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def awkward(wh):
    if ("awkward", wh) not in _FRAMES:
        W, H = wh
        nrm, pos, planes, mask, lights_map = lc.frame(wh)
        i = np.arange(H * W) + 3 * W + H
        dist = np.stack([DISTANCES[(i * (l + 2) + l) % len(DISTANCES)] for l in range(8)]).reshape(8, H, W)
        _FRAMES[("awkward", wh)] = (nrm, pos, planes, mask, lights_map) + _freeze((np.ascontiguousarray(dist, f32),))
    return _FRAMES[("awkward", wh)]


def geometric(wh):
    if ("geometric", wh) not in _FRAMES:
        W, H = wh
        y, x = np.mgrid[0:H, 0:W]
        xc, ys = max(1, (2 * W) // 3), max(1, (3 * H) // 4)              # the crease's column, the step's row
        s = (x - xc) * STEP
        wall = x >= xc
        nrm = np.zeros((H, W, 4), f32)
        pos = np.ones((H, W, 4), f32)
        nrm[..., 0] = np.where(wall, -0.6, 0.0)
        nrm[..., 1] = np.where(wall, 0.8, 1.0)
        pos[..., 0] = np.where(wall, xc * STEP + 0.8 * s, x * STEP)
        pos[..., 1] = np.where(wall, 0.6 * s, 0.0) + np.where(y >= ys, 0.5, 0.0)
        pos[..., 2] = y * STEP
        background = ((x + 2 * y) % 23 == 7) | ((y == H // 2) & (x % 5 < 2) & (H > 8))
        nrm[background] = 0
        pos[background] = NAN                                            # (a background texel's position is never looked at)
        rs = np.random.RandomState(1000 * W + H)
        lights_map = rs.randint(0, 256, (H, W)).astype(np.uint8) | np.uint8(0x11)
        lights_map[(x * 7 + y * 3) % 11 == 0] &= np.uint8(0xF6)          # (lights 0 and 3 off here and there)
        mask = rs.randint(0, 256, (H, W)).astype(np.uint8)
        planes = np.stack([rs.randint(0, max(1, lc.NSAMPLES[l]) + 1, (H, W)) for l in range(8)]).astype(np.uint8)
        planes[0] = 9                                                    # light 0: one byte everywhere
        planes[1][(x < 19) & (y < 19)] = 2                               # light 1: one byte over the first block's window (R <= 2)
        planes[3] = 31                                                   # light 3: one byte wherever a tap can be accepted ...
        off3 = ((lights_map >> 3) & 1) == 0
        planes[3][off3 | background] = rs.randint(0, 256, (H, W)).astype(np.uint8)[off3 | background]     # ... and noise elsewhere
        mask[(x < 19) & (y < 19)] |= 0x05                                # hard: bits 0 and 2 uniform over the first block's window
        near = np.array([INF, 0.0, 0.15, 3.0], f32)
        dist = np.stack([near[(x * 3 + y * 5 + l) % 4] for l in range(8)]).astype(f32)
        _FRAMES[("geometric", wh)] = _freeze((nrm, pos, np.ascontiguousarray(planes), mask, lights_map, np.ascontiguousarray(dist)))
        if wh == (33, 18):
            census = {}
            filter_rule(lc.the_list("soft", "8"), params(2), pos, nrm, planes, lights_map, dist, census)
            for test in ("normal", "plane", "spread"):
                assert census[test][0] > 50 and census[test][1] > 50, (test, census)
    return _FRAMES[("geometric", wh)]


def frame(kind, wh):
    return awkward(wh) if kind == "awkward" else geometric(wh)


# ------------------------------------------------------------------------------------------- the rules, written out in float32 / uint32
def _bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def filter_rule(lst, p, positions, normals, planes, lights_map=None, distances=None, census=None):
    """float32[count, H, W] of the filter, from the header's text: integer tent weights, integer sums, float32 comparisons that a NaN
    fails, one float32 division.  ``lst`` a ``LightList``: ``planes`` is the mask, c_l = its bit l, n_l = 1; a ``SoftLightList``:
    c_l = planes[l], n_l = max(1, nsamples_l).  ``census``: a dict that receives, per test, [taps accepted, taps rejected] among the
    taps that reached it."""
    hard = isinstance(lst, api.LightList)
    count, R = lst.count, int(p.radius)
    cos_min, eps = f32(p.normal_cos_min), f32(p.plane_eps)
    n = np.ascontiguousarray(normals, f32)
    P = np.ascontiguousarray(positions, f32)
    H, W = n.shape[:2]
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    bg = (nx == 0) & (ny == 0) & (nz == 0)
    planes = np.ascontiguousarray(planes, np.uint8)
    on = [np.ones((H, W), bool) if lights_map is None else ((np.asarray(lights_map, np.uint8) >> l) & 1) != 0 for l in range(count)]
    c = [(((planes >> l) & 1) if hard else planes[l]).astype(u32) for l in range(count)]
    n_l = [u32(1) if hard else u32(max(1, lst.lights[l].nsamples)) for l in range(count)]
    num = [np.zeros((H, W), u32) for _ in range(count)]
    den = [np.zeros((H, W), u32) for _ in range(count)]
    yy, xx = np.mgrid[0:H, 0:W]
    if census is not None:
        census.update({"normal": [0, 0], "plane": [0, 0], "spread": [0, 0]})
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                w = u32((R + 1 - abs(dx)) * (R + 1 - abs(dy)))
                qy, qx = yy + dy, xx + dx
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                centre = dx == 0 and dy == 0
                if not centre:
                    cos = (nx * nx[qy, qx] + ny * ny[qy, qx]) + nz * nz[qy, qx]
                    Dx, Dy, Dz = P[qy, qx, 0] - P[..., 0], P[qy, qx, 1] - P[..., 1], P[qy, qx, 2] - P[..., 2]
                    h = (nx * Dx + ny * Dy) + nz * Dz
                    d2 = (Dx * Dx + Dy * Dy) + Dz * Dz
                    assert cos.dtype == f32 and h.dtype == f32 and d2.dtype == f32
                    reach = inside & ~bg & ~bg[qy, qx]
                    normal_ok, plane_ok = cos >= cos_min, np.abs(h) <= eps
                    geom = reach & normal_ok & plane_ok
                    if census is not None:
                        census["normal"][0] += int((reach & normal_ok).sum())
                        census["normal"][1] += int((reach & ~normal_ok).sum())
                        census["plane"][0] += int((reach & normal_ok & plane_ok).sum())
                        census["plane"][1] += int((reach & normal_ok & ~plane_ok).sum())
                for l in range(count):
                    if centre:
                        acc = np.ones((H, W), bool)
                    else:
                        acc = geom & on[l][qy, qx]
                        if distances is not None:
                            d = _bits(distances[l])
                            m = np.minimum(d, d[qy, qx])
                            sm = f32(p.spread[l]) * m.view(f32)
                            near = (m == u32(0x7F800000)) | (d2 <= sm * sm)
                            if census is not None:
                                census["spread"][0] += int((acc & on[l] & near).sum())
                                census["spread"][1] += int((acc & on[l] & ~near).sum())
                            acc = acc & near
                    num[l] += np.where(acc, w * c[l][qy, qx], u32(0)).astype(u32)
                    den[l] += np.where(acc, w * n_l[l], u32(0)).astype(u32)
        out = np.zeros((count, H, W), f32)
        for l in range(count):
            assert int(num[l].max()) < 1 << 24 and int(den[l].max()) < 1 << 24
            out[l] = np.where(~bg & on[l], num[l].astype(f32) / den[l].astype(f32), f32(0.0))
        return out


def visibility_combine_rule(k, lst, positions, normals, visibility, lights_map=None, colors=None):
    """uint8[H, W, 3] of the visibility combine: list_combine_cases.list_combine_rule with visibility[l] in place of byte_l / samples_l."""
    with np.errstate(all="ignore"):
        n = np.ascontiguousarray(normals, f32)
        nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
        cx, cy, cz = (f32(k.cameraDirection[i]) for i in range(3))
        cl = np.sqrt((cx * cx + cy * cy) + cz * cz)
        if cl > 0:
            inv = f32(1.0) / cl
            cx, cy, cz = cx * inv, cy * inv, cz * inv
        ndv = (nx * (cx * f32(-1.0)) + ny * (cy * f32(-1.0))) + nz * (cz * f32(-1.0))
        ndv = np.where(ndv > 0, ndv, f32(0))
        ambient = f32(0.15) + f32(0.05) * (f32(1.0) - ndv)
        vis = np.ascontiguousarray(visibility, f32)
        sums = [np.zeros(nx.shape, f32) for _ in range(3)]
        for l in range(lst.count):
            e = lst.lights[l]
            ndl = sp.ndl_rule(k, api.Light.make(e.type, list(e.xyz)), positions, normals)
            ndl = np.where(ndl > 0, ndl, f32(0))
            direct = (f32(1.25) * ndl) * vis[l]
            on = np.ones(nx.shape, bool) if lights_map is None else ((np.asarray(lights_map, np.uint8) >> l) & 1) != 0
            for ch in range(3):
                color = f32(1.0) if colors is None else f32(np.asarray(colors, f32)[l, ch])
                sums[ch] = np.where(on, sums[ch] + (direct * color).astype(f32), sums[ch]).astype(f32)
        background = (nx == 0) & (ny == 0) & (nz == 0)
        out = np.zeros(nx.shape + (3,), np.uint8)
        for ch in range(3):
            scaled = (sums[ch] + ambient) * f32(255.0) + f32(0.5)
            assert scaled.dtype == f32
            inside = (scaled > 0) & (scaled < 255)
            byte = np.where(scaled >= 255, 255, np.where(inside, np.where(inside, scaled, 0).astype(np.int32), 0))
            out[..., ch] = np.where(background, 0, byte).astype(np.uint8)
        return out


def wild_visibility(wh):
    """float32[8, H, W]: arbitrary finite values, negatives, values above 1, +-Inf and NaN."""
    W, H = wh
    table = np.array([0.0, 1.0, 0.25, 0.6875, -0.5, 2.5, 1e-41, 3e38, INF, -INF, NAN, -0.0, 0.333333343], f32)
    i = np.arange(H * W)
    return np.ascontiguousarray(np.stack([table[(i * (2 * l + 1) + 5 * l) % len(table)] for l in range(8)]).reshape(8, H, W))


def runs(radius):
    """(form, list name, with map, with distances) of the runs over a frame at a radius: the wide lists at the small radii only."""
    out = [("soft", "3", True, True), ("hard", "3", True, False), ("soft", "2_directional", False, False)]
    if radius <= 2:
        out += [("soft", "8", True, True), ("soft", "8", False, True), ("hard", "8", False, False), ("soft", "1", True, False)]
    return out


def the_list(form, name):
    return lc.the_list(form, name)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(u32) != want.view(u32))
    assert bad.shape[0] == 0, (what, bad.shape[0], [(tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:6].tolist()])
