"""Shared by the propagated-variance filter tests (tests/test_list_propagated_host.py, tests/test_gpu_list_propagated.py): the rule of
include/rts_scene.h's rtsh_wide_filter_propagated_mean_soft_light_list* restated in numpy from the header's text and independently of
the C++: float32 for the geometry of a tap (list_wide_guided_cases' ``_geom``), int64 arrays with every bound asserted (numQ < 2^45,
2 * numQ + den^2 < 2^46, guide_k4^2 * G < 2^58: all exact in 64 bits), ``//``, and ``math.isqrt`` over Python integers for every root.
No GPU code is touched here.

Frames, lists, count planes and the mean-plane material are the existing case modules' (imported, not copied).  FRAMES are the smallest
at which each kernel form can go wrong: 3 x 2 and 17 x 1 (every far tap outside; NaN and Inf in the awkward G-buffer), 40 x 72 and
72 x 40 (partial blocks on one side), 72 x 72 geometric and 72 x 72 flat (the step-16 taps accepted on both sides).  MOMENTS come in
four kinds (``moments_of``), each (mean, square, lengths) of 8 planes:
  "zero"       square == mean^2 and a long history everywhere: Q = 0, T = 0 (anchor 6);
  "saturated"  square 0xFFFFFFFF everywhere, mean and lengths hashed: the largest R, Q and G the planes can give;
  "short"      every length 1, mean and square hashed (anchor 7; with min_history >= 2 every pair takes the Bernoulli branch);
  "mixed"      list_mean_filter_cases' "hashed" planes: mean 0, 65535 or hashed, square below, at and above mean^2, lengths 0, 1, 2,
               254, 255 in turn.
The census (``census_ok``) is a condition on the RULE alone, asserted with the "mixed" planes at guide_k4 8 and 12 on every frame at
least 40 pixels wide: pixels with T_k != T_0 for some k >= 1, taps accepted under T_0 but rejected under T_k, accepted taps of a
value other than the centre's (in a pass k >= 1 as well), and pixels where by_length changes T_0 -- all non-zero."""
import math

import numpy as np

import list_mean_filter_cases as mf
import list_moments_cases as mc
import list_wide_guided_cases as gc
from raytracedshadows_amd import api

f32, i64 = np.float32, np.int64

#: (kind of frame, (W, H))
FRAMES = [("geometric", (3, 2)), ("awkward", (3, 2)), ("awkward", (17, 1)), ("geometric", (40, 72)), ("awkward", (72, 40)),
          ("flat", (72, 40)), ("geometric", (72, 72)), ("flat", (72, 72))]
PASSES = [0, 1, 2, 3, 4, 5]
K4 = [0, 1, 8, 12, 255]
CENSUS_K4 = [8, 12]
MIN_HISTORY = [1, 4, 255]
KINDS_OF_MOMENTS = ["zero", "saturated", "short", "mixed"]
same_bits = mf.same_bits
samples_of = mf.samples_of
the_list = mf.the_list
lists = mf.lists
frame = mf.frame
counts = mf.counts


def frame_id(f):
    return f"{f[0]}-{f[1][0]}x{f[1][1]}"


def params(passes, k4, min_history, by_length, kind="geometric"):
    if kind in ("geometric", "flat"):
        return api.WideGuidePropagatedParams.make(passes, k4, min_history, by_length, 0.9, 0.02)
    return api.WideGuidePropagatedParams.make(passes, k4, min_history, by_length, 0.5, 10.0)


_MOMENTS = {}


def moments_of(kind_of_moments, kind, wh, lst):
    key = (kind_of_moments, kind, wh, tuple(samples_of(lst)))
    if key not in _MOMENTS:
        mean, square, lengths = (a.copy() for a in mf.moments_of("hashed", kind, wh, lst))
        count = lst.count
        if kind_of_moments == "zero":
            square[:count] = (mean[:count].astype(i64) ** 2).astype(np.uint32)
            lengths[:count] = 255
        elif kind_of_moments == "saturated":
            square[:count] = 0xFFFFFFFF
        elif kind_of_moments == "short":
            lengths[:count] = 1
        else:
            assert kind_of_moments == "mixed"
        out = (mean, square, lengths)
        for a in out:
            a.setflags(write=False)
        _MOMENTS[key] = out
    return _MOMENTS[key]


def isqrt_array(q):
    """math.isqrt over an array of non-negative integers, through Python integers."""
    values, inverse = np.unique(q, return_inverse=True)
    roots = np.array([math.isqrt(int(v)) for v in values], i64)
    return roots[inverse].reshape(q.shape)


def _sum3(E, active):
    """G, D: the 3 x 3 sums of w * E and of w over the counted pixels, weights {1, 2, 1} x {1, 2, 1} (E is 0 where not counted)."""
    count, H, W = active.shape
    G, D = np.zeros((count, H, W), i64), np.zeros((count, H, W), i64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            w = (2 - abs(dx)) * (2 - abs(dy))
            ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H + min(0, -dy))
            xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W + min(0, -dx))
            G[:, yd, xd] += w * E[:, ys, xs]
            D[:, yd, xd] += w * active[:, ys, xs]
    return G, D


def _threshold(G, D, n, k4, n_l, active):
    assert int(G.max()) < 1 << 42 and int(k4) * int(k4) * int(G.max()) < 1 << 58
    T = np.minimum(65535, isqrt_array((int(k4) * int(k4) * G) // (16 * np.maximum(D, 1) * n)))
    return np.where(active, np.where(n_l <= 1, 65535, T), 0)


def first_variance_and_threshold(lst, k4, min_history, by_length, planes, moments, active):
    """(Q_0, T_0), int64[count, H, W] each: R, Q_0 and T_0 of the header."""
    count = lst.count
    n_l, S_l = mf._nS(lst)
    V0 = mf.v0_of_counts(lst, planes)
    mean, square, lengths = (np.asarray(a)[:count].astype(i64) for a in moments)
    temporal = lengths >= int(min_history)
    R = np.maximum(0, square - mean * mean)
    Qt = R // np.maximum(lengths, 1) if by_length else R
    bernoulli = V0 * (n_l * S_l - V0)
    Q = np.where(active, np.where(temporal, Qt, bernoulli // n_l), 0)
    assert int(Q.max()) < 1 << 32
    E = np.where(active, np.where(temporal, n_l * Qt, bernoulli), 0)
    G, D = _sum3(E, active)
    return Q, _threshold(G, D, n_l, k4, n_l, active)


def propagated_rule(lst, p, positions, normals, planes, moments, lights_map=None, max_passes=5, census=None, kind=None, wh=None):
    """([float32[count, H, W] for passes = 0 .. max_passes], [int64 Q_0, Q_1, ...], [int64 T_0, T_1, ...]) of the propagated filter
    (p.passes is not looked at; guide_k4, min_history and by_length are).  ``planes``: this frame's counts.  Anchors 4 and 5 are
    asserted per pass."""
    count = lst.count
    n_l, S_l = mf._nS(lst)
    k4 = int(p.guide_k4)
    active = mf._active(lst, normals, lights_map)
    guided = active & (n_l >= 2)
    V = mf.mean_input(lst, moments[0], active)
    Q, T0 = first_variance_and_threshold(lst, k4, p.min_history, int(p.by_length), planes, moments, active)
    Q = np.where(guided, Q, 0)
    outs, Qs, Ts = [mf._output(lst, V, active)], [Q], []
    tally = {"T_changed": 0, "tightened": 0, "moved": 0, "moved_later": 0}
    for k in range(max_passes):
        if k == 0:
            T = T0
        else:
            G, D = _sum3(Q, active)
            assert int(G.max()) < 1 << 36
            T = _threshold(G, D, 1, k4, n_l, active)
            tally["T_changed"] += int((guided & (T != T0)).sum())
        Ts.append(T)
        taps = gc._geom(kind, wh, positions, normals, p.normal_cos_min, p.plane_eps, 1 << k)[1]
        num, den, numQ = 36 * V, np.full(V.shape, 36, i64), 1296 * Q
        lo, hi, hiQ = V.copy(), V.copy(), Q.copy()
        for w, qy, qx, geom in taps:
            q, qq = V[:, qy, qx], Q[:, qy, qx]
            reach = geom[None] & active[:, qy, qx] & active
            diff = np.abs(q - V)
            acc = reach & (diff <= T)
            num += np.where(acc, w * q, 0)
            den += np.where(acc, w, 0)
            numQ += np.where(acc, w * w * qq, 0)
            lo, hi = np.where(acc, np.minimum(lo, q), lo), np.where(acc, np.maximum(hi, q), hi)
            hiQ = np.where(acc, np.maximum(hiQ, qq), hiQ)
            moved = int((acc & guided & (diff != 0)).sum())
            tally["moved"] += moved
            if k >= 1:
                tally["moved_later"] += moved
                tally["tightened"] += int((reach & guided & (diff <= T0) & ~acc).sum())
        assert int(num.max()) < 1 << 24 and int(den.max()) <= 256 and int(numQ.max()) < 1 << 45
        V = np.where(active, (2 * num + den) // (2 * den), 0)
        newQ = np.where(guided, (2 * numQ + den * den) // (2 * den * den), 0)
        assert ((V >= lo) & (V <= hi))[active].all()                      # anchor 4
        assert (newQ <= hiQ).all()                                        # anchor 5: at most the largest accepted Q_k
        assert (newQ == Q)[guided & (den == 36)].all()                    # ... and kept exactly by a pixel that accepts only its centre
        Q = newQ
        outs.append(mf._output(lst, V, active))
        Qs.append(Q)
    if census is not None:
        census.update(tally)
        other = first_variance_and_threshold(lst, k4, p.min_history, 1 - int(p.by_length), planes, moments, active)[1]
        census["by_length"] = int((guided & (other != T0)).sum())
    return outs, Qs, Ts


def census_ok(census, what):
    for name in ("T_changed", "tightened", "moved", "moved_later", "by_length"):
        assert census[name] > 0, (what, name, census)
