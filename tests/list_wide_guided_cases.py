"""Shared by the guided wide filter tests (tests/test_list_wide_guided_host.py, tests/test_gpu_list_wide_guided.py): lists, frames,
count planes and the expected floats of the variance-guided wide filter of a soft light list's planes (include/rts_scene.h,
rtsh_wide_filter_guided_soft_light_list*) from a numpy restatement of its rule, written here from the header's text and independently
of the C++ and of tests/list_wide_filter_cases.py's rule: integer arrays, ``//``, ``math.isqrt``, float32 comparisons that a NaN fails,
one float32 division.  Of list_wide_filter_cases only the frame and list generators are used.  No GPU code is touched here.

The count planes are this file's own (``counts``): per light a pattern, 32 columns long, of ten columns where no sample sees the light,
twelve of a ramp with a hash on top and ten where every sample does -- so T is 0 in the unanimous stretches, in between inside the
ramp, and 65535 for the lights of one sample --, drifting by a column every 16 rows.  ``guided_rule`` counts, per pass and light, the
taps that geom and the map accept and the guide rejects, and the accepted taps whose value differs from the centre's; ``census_ok``
asserts both on every frame at least 40 pixels wide, so that a guide that never fires, or fires always, cannot pass unnoticed."""
import math

import numpy as np

import list_wide_filter_cases as wc
from raytracedshadows_amd import api

f32, u32, u64 = np.float32, np.uint32, np.uint64

FRAMES = wc.FRAMES
PASSES = [0, 1, 2, 3, 4, 5]
COUNTS = [1, 4, 8]
K4 = [0, 1, 8, 12, 255]
#: the values of guide_k4 at which the census must see both kinds of tap
CENSUS_K4 = [8, 12]
B5 = {0: 6, 1: 4, 2: 1}

same_bits = wc.same_bits
kinds = wc.kinds
samples_of = wc.samples_of


def the_list(count, rotation=0):
    """A ``SoftLightList`` of ``count`` lights; entry l has wc.SAMPLES[(l + rotation) % 4] = 1, 4, 16 or 48 samples."""
    return wc.the_list("soft", count, rotation)


def lists():
    """(count, rotation) of every list: 1, 4 and 8 lights, every n_l in every entry."""
    return [(c, r) for c in COUNTS for r in range(4)]


def params(passes, k4, kind="geometric"):
    if kind in ("geometric", "flat"):
        return api.WideGuideParams.make(passes, k4, 0.9, 0.02)
    return api.WideGuideParams.make(passes, k4, 0.5, 10.0)


_COUNTS = {}


def counts(wh, lst):
    """uint8[8, H, W]: the count planes of a frame for a list (planes from its count up: 0xEE, never to be read)."""
    key = (wh, tuple(samples_of(lst)))
    if key not in _COUNTS:
        W, H = wh
        y, x = np.mgrid[0:H, 0:W]
        planes = np.full((8, H, W), 0xEE, np.uint8)
        for l, n in enumerate(samples_of(lst)):
            u = (x + y // 16 + 5 * l) % 32
            ramp = np.clip((u - 9) / 12.0, 0.0, 1.0)
            noise = ((x * 7 + y * 13 + l * 3 + (x * y) % 5) % 3) - 1
            c = np.rint(n * ramp).astype(np.int64) + np.where((u >= 10) & (u < 22), noise, 0)
            c = np.clip(c, 0, n)
            c[(u < 10)] = 0
            c[(u >= 22)] = n
            planes[l] = c
        planes.setflags(write=False)
        _COUNTS[key] = planes
    return _COUNTS[key]


def frame(kind, wh):
    """(normals, positions, lights_map) of wc.frame."""
    nrm, pos, _, _, lights_map, _ = wc.frame(kind, wh)
    return nrm, pos, lights_map


_GEOM = {}


def _geom(kind, wh, positions, normals, cos_min, eps, step):
    """bg, and [(weight, qy, qx, geom)] of the 24 taps of a pass beside the centre: geom = inside the frame, not bg(q), the normal test,
    the plane test.  Cached per named frame (kind not None)."""
    key = (kind, wh, float(cos_min), float(eps), step)
    if kind is None or key not in _GEOM:
        n = np.ascontiguousarray(normals, f32)
        P = np.ascontiguousarray(positions, f32)
        H, W = n.shape[:2]
        nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
        bg = (nx == 0) & (ny == 0) & (nz == 0)
        yy, xx = np.mgrid[0:H, 0:W]
        taps = []
        with np.errstate(all="ignore"):
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        continue
                    qy, qx = yy + dy * step, xx + dx * step
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    if not inside.any():
                        continue
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    cos = (nx * nx[qy, qx] + ny * ny[qy, qx]) + nz * nz[qy, qx]
                    h = (nx * (P[qy, qx, 0] - P[..., 0]) + ny * (P[qy, qx, 1] - P[..., 1])) + nz * (P[qy, qx, 2] - P[..., 2])
                    assert cos.dtype == f32 and h.dtype == f32
                    taps.append((B5[abs(dx)] * B5[abs(dy)], qy, qx, inside & ~bg[qy, qx] & (cos >= f32(cos_min)) & (np.abs(h) <= f32(eps))))
        if kind is None:
            return bg, taps
        _GEOM[key] = (bg, taps)
    return _GEOM[key]


def isqrt_array(q):
    """math.isqrt over an array of non-negative integers."""
    values, inverse = np.unique(q, return_inverse=True)
    roots = np.array([math.isqrt(int(v)) for v in values], np.int64)
    return roots[inverse].reshape(q.shape)


def thresholds(lst, k4, normals, planes, lights_map=None):
    """int64[count, H, W]: T(p, l) of the header (0 at an inactive pixel), and the active mask bool[count, H, W]."""
    count = lst.count
    n = np.ascontiguousarray(normals, f32)
    H, W = n.shape[:2]
    bg = (n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0)
    n_l = np.array(samples_of(lst), np.int64).reshape(-1, 1, 1)
    S_l = 65535 // n_l
    on = np.ones((count, H, W), bool) if lights_map is None else \
        np.stack([((np.asarray(lights_map, np.uint8) >> l) & 1) != 0 for l in range(count)])
    counted = on & ~bg                                                           # inside the frame by construction
    V0 = np.minimum(np.asarray(planes)[:count].astype(np.int64), n_l) * S_l
    E = np.where(counted, V0 * (n_l * S_l - V0), 0)
    assert int(E.max()) < 1 << 30
    G = np.zeros((count, H, W), np.int64)
    D = np.zeros((count, H, W), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            w = (2 - abs(dx)) * (2 - abs(dy))
            ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H + min(0, -dy))
            xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W + min(0, -dx))
            G[:, yd, xd] += w * E[:, ys, xs]
            D[:, yd, xd] += w * counted[:, ys, xs]
    assert int(G.max()) < 1 << 35
    T = np.minimum(65535, isqrt_array((int(k4) * int(k4) * G) // (16 * np.maximum(D, 1) * n_l)))
    T = np.where(n_l <= 1, 65535, T)
    return np.where(counted, T, 0), counted


def guided_rule(lst, p, positions, normals, planes, lights_map=None, max_passes=5, census=None, kind=None, wh=None):
    """[float32[count, H, W] for passes = 0 .. max_passes] of the guided wide filter, from the header's text (p.passes is not looked
    at; p.guide_k4 is).  ``census``: a dict that receives, per (pass, light), [taps that geom and the map accept and the guide
    rejects, accepted taps whose value differs from the centre's]."""
    count = lst.count
    n_l = np.array(samples_of(lst), np.int64).reshape(-1, 1, 1)
    S_l = 65535 // n_l
    T, active = thresholds(lst, p.guide_k4, normals, planes, lights_map)
    on = active                                                                  # on(q, l) of a tap that geom accepts: geom has bg(q)
    V = np.where(active, np.minimum(np.asarray(planes)[:count].astype(np.int64), n_l) * S_l, 0)

    def output():
        assert int(V.max()) <= 65535 and int(V.min()) >= 0
        return np.where(active, V.astype(f32) / (n_l * S_l).astype(f32), f32(0.0)).astype(f32)

    outs = [output()]
    for k in range(max_passes):
        taps = _geom(kind, wh, positions, normals, p.normal_cos_min, p.plane_eps, 1 << k)[1]
        num, den = 36 * V, np.full(V.shape, 36, np.int64)
        lo, hi = V.copy(), V.copy()
        rejected, moved = np.zeros(count, np.int64), np.zeros(count, np.int64)
        for w, qy, qx, geom in taps:
            q = V[:, qy, qx]
            reach = geom[None] & on[:, qy, qx] & active
            diff = np.abs(q - V)
            acc = reach & (diff <= T)
            num += np.where(acc, w * q, 0)
            den += np.where(acc, w, 0)
            lo, hi = np.where(acc, np.minimum(lo, q), lo), np.where(acc, np.maximum(hi, q), hi)
            rejected += (reach & ~acc).sum(axis=(1, 2))
            moved += (acc & (diff != 0)).sum(axis=(1, 2))
        assert int(num.max()) < 1 << 24 and int(den.max()) <= 256
        V = np.where(active, (2 * num + den) // (2 * den), 0)
        assert ((V >= lo) & (V <= hi))[active].all()                              # anchor 4, in the rule itself
        if census is not None:
            for l in range(count):
                census[(k, l)] = [int(rejected[l]), int(moved[l])]
        outs.append(output())
    return outs


def census_ok(lst, census, what):
    """Every pass and every light of two samples or more saw a tap the guide rejected and an accepted tap of another value."""
    for (k, l), (rejected, moved) in census.items():
        if samples_of(lst)[l] >= 2:
            assert rejected > 0 and moved > 0, (what, "pass", k, "light", l, rejected, moved)


def centre_quotient(lst, planes, normals, lights_map=None):
    """float32[count, H, W]: (float)min(c, n_l) / (float)n_l where the pixel is active, +0 elsewhere: the passes == 0 plane."""
    nrm = np.asarray(normals, f32)
    bg = (nrm[..., :3] == 0).all(axis=-1)
    out = np.zeros((lst.count,) + bg.shape, f32)
    for l, n in enumerate(samples_of(lst)):
        on = ~bg & ((((np.asarray(lights_map) >> l) & 1) != 0) if lights_map is not None else True)
        out[l] = np.where(on, np.minimum(np.asarray(planes)[l], n).astype(f32) / f32(n), f32(0))
    return out
