"""Shared by the clamped count-moment tests (tests/test_list_moments_clamp_host.py, tests/test_gpu_list_moments_clamp.py): the rule of
include/rts_scene.h's last section -- rtsh_accumulate_moments_soft_light_list_clamped* -- restated in numpy from the header's text and
independently of the C++: int64 arrays, ``//`` and ``math.isqrt``.  The geometry of the four taps is list_moments_cases' own (``_taps``,
imported and not edited); the window, the box, the clamp and the quotient are written out here, and ``moments_rule`` of
list_moments_cases -- not edited either -- is what anchor 1 compares against.  No GPU code is touched here.

Frames, motions, length planes and history planes are list_moments_cases' (mean 0 / 65535 / hashed, squares below, equal to and above
mean^2).  ``stale_case`` is this file's own: the history of a frame that was lit everywhere (mean 65535, square 65535^2) or dark
everywhere, in stripes, over this frame's counts -- what a shadow that moved leaves behind.  The census (``census``) counts, from the
numpy rule alone, what the tests need to occur on the 40 x 40 "pixels" pair."""
import math

import numpy as np

import list_moments_cases as mc
import list_motion_cases as ms
import list_temporal_cases as tc

i64 = np.int64
RADII = (0, 1, 2, 3, 4)
SIGMA_K4 = (0, 8, 36, 255)
MARGINS = (0, 1, 65535)
#: every (radius, sigma_k4, margin): 60 selections, walked four at a time
GRID = [(r, k, m) for r in RADII for k in SIGMA_K4 for m in MARGINS]


def bounds_rule(m, S1, S2, lo, hi, k4, margin):
    """(Lv', Hv') int64 arrays from the header's BOX, element for element (m >= 1 everywhere)."""
    m, S1, S2, lo, hi = (np.asarray(a, i64) for a in (m, S1, S2, lo, hi))
    D = m * S2 - S1 * S1
    assert (D >= 0).all() and int(D.max(initial=0)) < 1 << 43
    x = int(k4) * int(k4) * D
    assert int(x.max(initial=0)) < 1 << 59
    flat = x.reshape(-1).tolist()
    R = np.array([math.isqrt(v) + (1 if math.isqrt(v) ** 2 < v else 0) for v in flat], i64).reshape(x.shape)
    Rc = (R + 3) // 4
    A, B = np.maximum(S1 - Rc, 0), S1 + Rc
    Lm, Hm = np.maximum(m * lo, A), np.minimum(m * hi, B)
    Lv, Hv = Lm // m, (Hm + m - 1) // m
    return np.maximum(Lv - int(margin), 0), np.minimum(65535, Hv + int(margin))


def window_rule(lst, normals, counts, lights_map, radius):
    """Per light over the (2r+1)^2 window: (contributes bool, m, S1, S2, lo, hi) as [count, H, W] arrays, and ``cut`` bool[H, W]: the
    window reaches outside the frame.  lo = 65535 and hi = 0 where m == 0."""
    count = lst.count
    nrm = np.ascontiguousarray(normals, np.float32)
    H, W = nrm.shape[:2]
    bg = (nrm[..., 0] == 0) & (nrm[..., 1] == 0) & (nrm[..., 2] == 0)
    r = int(radius)
    y, x = np.mgrid[0:H, 0:W]
    cut = (x - r < 0) | (x + r >= W) | (y - r < 0) | (y + r >= H)
    on = np.zeros((count, H, W), bool)
    m, S1, S2 = (np.zeros((count, H, W), i64) for _ in range(3))
    lo, hi = np.full((count, H, W), 65535, i64), np.zeros((count, H, W), i64)
    for l, n_l in enumerate(mc.samples_of(lst)):
        on[l] = ~bg & (True if lights_map is None else ((np.asarray(lights_map, np.uint8) >> l) & 1) != 0)
        v = np.minimum(np.asarray(counts)[l].astype(i64), n_l) * (65535 // n_l)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H + min(0, -dy))
                xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W + min(0, -dx))
                if ys.start >= ys.stop or xs.start >= xs.stop:
                    continue
                c, q = on[l][ys, xs], v[ys, xs]
                m[l][yd, xd] += c
                S1[l][yd, xd] += np.where(c, q, 0)
                S2[l][yd, xd] += np.where(c, q * q, 0)
                lo[l][yd, xd] = np.where(c, np.minimum(lo[l][yd, xd], q), lo[l][yd, xd])
                hi[l][yd, xd] = np.where(c, np.maximum(hi[l][yd, xd], q), hi[l][yd, xd])
    assert int(m.max()) <= 81 and int(S1.max()) < 1 << 23 and int(S2.max()) < 1 << 39
    return on, m, S1, S2, lo, hi, cut


def clamped_rule(lst, p, positions, normals, counts, prev, lights_map, clamp, census=None):
    """(uint16 mean, uint32 square, uint8 lengths)[count, H, W] of the clamped pass from the header's text.  ``clamp`` = (radius,
    sigma_k4, margin).  ``census``: a dict that receives, summed over the lights, the numbers of blended pairs "above" (s1 clamped from
    above), "below", "alone" (neither sum moved), "cut" (blended, window cut by the frame), "hole" (blended, a tap inside the frame
    that does not contribute) and "sigma" (blended, the sigma bound and not the range binds: Lv > lo or Hv < hi at margin 0)."""
    radius, k4, margin = clamp
    count = lst.count
    nrm = np.ascontiguousarray(normals, np.float32)
    H, W = nrm.shape[:2]
    on, wm, S1, S2, wlo, whi, cut = window_rule(lst, nrm, counts, lights_map, radius)
    mean, square, lengths = (np.zeros((count, H, W), i64) for _ in range(3))
    taps = None if prev is None else mc._taps(p, positions, normals, prev[0], prev[1])[1]
    if census is not None:
        census.update(above=0, below=0, alone=0, cut=0, hole=0, sigma=0, blended=0)
    y, x = np.mgrid[0:H, 0:W]
    inside = (np.minimum(x + radius, W - 1) - np.maximum(x - radius, 0) + 1) * (np.minimum(y + radius, H - 1) - np.maximum(y - radius, 0) + 1)
    for l, n_l in enumerate(mc.samples_of(lst)):
        cur1 = np.minimum(np.asarray(counts)[l].astype(i64), n_l) * (65535 // n_l)
        cur2 = cur1 * cur1
        out1, out2, out_len = np.where(on[l], cur1, 0), np.where(on[l], cur2, 0), np.where(on[l], 1, 0)
        if taps is not None and not (int(p.reset_lights) >> l) & 1:
            pm, ps, pl = (np.asarray(a)[l].astype(i64) for a in prev[2:])
            sw, s1, s2, m = np.zeros((H, W), i64), np.zeros((H, W), i64), np.zeros((H, W), i64), np.full((H, W), 255, i64)
            for geom, w, cy, cx, _ in taps:
                acc = geom & on[l] & (pl[cy, cx] != 0)
                sw += np.where(acc, w, 0)
                s1 += np.where(acc, w * pm[cy, cx], 0)
                s2 += np.where(acc, w * ps[cy, cx], 0)
                m = np.where(acc, np.minimum(m, pl[cy, cx]), m)
            n = np.minimum(m + 1, int(p.max_length))
            blend = on[l] & (sw != 0) & (n != 1)
            assert (wm[l][blend] >= 1).all()                             # the centre of a blended pair contributes
            safe = np.where(blend, wm[l], 1)
            Lv, Hv = bounds_rule(safe, np.where(blend, S1[l], 0), np.where(blend, S2[l], 0), np.where(blend, wlo[l], 0),
                                 np.where(blend, whi[l], 0), k4, margin)
            assert (Lv <= Hv)[blend].all()
            if int(margin) == 0:
                assert ((wlo[l] <= Lv) & (Hv <= whi[l]))[blend].all()
            c1 = np.minimum(np.maximum(s1, sw * Lv), sw * Hv)
            c2 = np.minimum(np.maximum(s2, sw * Lv * Lv), sw * Hv * Hv)
            den = np.where(blend, n * sw, 1)
            assert int(c2.max()) <= 1 << 42 and int(den.max()) < 1 << 18
            for cur, s, out in ((cur1, c1, out1), (cur2, c2, out2)):
                num = (n - 1) * s + sw * cur
                assert int((2 * num + den).max()) < 1 << 52
                out[...] = np.where(blend, (2 * num + den) // (2 * den), out)
            # RANGE (anchor 6), in the rule itself
            assert ((out1 >= np.minimum(Lv, cur1)) & (out1 <= np.maximum(Hv, cur1)))[blend].all()
            assert ((out2 >= np.minimum(Lv * Lv, cur2)) & (out2 <= np.maximum(Hv * Hv, cur2)))[blend].all()
            out_len = np.where(on[l] & (sw != 0), n, out_len)
            if census is not None:
                L0, H0 = bounds_rule(safe, np.where(blend, S1[l], 0), np.where(blend, S2[l], 0), np.where(blend, wlo[l], 0),
                                     np.where(blend, whi[l], 0), k4, 0)
                census["blended"] += int(blend.sum())
                census["above"] += int((blend & (s1 > sw * Hv)).sum())
                census["below"] += int((blend & (s1 < sw * Lv)).sum())
                census["alone"] += int((blend & (c1 == s1) & (c2 == s2)).sum())
                census["cut"] += int((blend & cut).sum())
                census["hole"] += int((blend & (wm[l] < inside)).sum())
                census["sigma"] += int((blend & ((L0 > wlo[l]) | (H0 < whi[l]))).sum())
        mean[l], square[l], lengths[l] = out1, out2, out_len
    assert int(mean.max()) <= 65535 and int(square.max()) < 1 << 32
    return mean.astype(np.uint16), square.astype(np.uint32), lengths.astype(np.uint8)


def clamped_motion_rule(lst, p, normals, counts, prev, lights_map, motion, clamp):
    """The motion form: list_motion_cases' reprojection (Q and M_p handed over as positions and normals; a background pixel keeps its
    zero normal, so INACTIVE and the window's activity stay the CURRENT normal's decision) in front of the rule above."""
    if prev is None:
        q, P, n = p, np.zeros(np.shape(normals), np.float32), np.ascontiguousarray(normals, np.float32)
    else:
        q, P, n = ms.reproject_inputs(p, normals, motion[0], motion[1])
    return clamped_rule(lst, q, P, n, counts, prev, lights_map, clamp)


def case(kind, wh, lst):
    """A frame pair of list_temporal_cases ("awkward" included) with list_moments_cases' counts and history planes."""
    if kind != "awkward":
        return mc.moments_case(kind, wh, lst)
    c = tc.case(kind, wh)
    mean, square = mc.history(wh, lst, 3)
    return dict(c, counts=mc.gc.counts(wh, lst), prev=(c["prev_pos"], c["prev_nrm"], mean, square, c["prev_len"]))


def stale_case(motion, wh, lst):
    """``case`` with the history a moved shadow leaves: stripes of 7 columns of all lit (65535, 65535^2) and all dark (0, 0), every
    length 9."""
    c = dict(mc.moments_case(motion, wh, lst))
    W, H = wh
    y, x = np.mgrid[0:H, 0:W]
    lit = ((x // 7 + y // 11) % 2 == 0)
    mean = np.full((8, H, W), 0xEEEE, np.uint16)
    square = np.full((8, H, W), 0xEEEEEEEE, np.uint32)
    for l in range(lst.count):
        mean[l] = np.where(lit, 65535, 0)
        square[l] = np.where(lit, 65535 * 65535, 0)
    c["prev"] = (c["prev_pos"], c["prev_nrm"], mean, square, np.full((8, H, W), 9, np.uint8))
    return c


def census(radius, k4=8, make=None):
    """The census of the 40 x 40 "pixels" pair with eight lights at a radius, margin 0."""
    lst = mc.the_list(8, 1)
    c = (make or stale_case)("pixels", (40, 40), lst)
    out = {}
    clamped_rule(lst, tc.with_params(c["params"], 32, 0), c["pos"], c["nrm"], c["counts"], c["prev"], c["map"], (radius, k4, 0), out)
    return out


def selections(run):
    """The four selections of GRID that run number ``run`` takes: fifteen runs walk all sixty."""
    return [GRID[(4 * run + j) % len(GRID)] for j in range(4)]
