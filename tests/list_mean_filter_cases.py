"""Shared by the mean-input wide filter tests (tests/test_list_mean_filter_host.py, tests/test_gpu_list_mean_filter.py): the two rules
of include/rts_scene.h -- rtsh_wide_filter_mean_soft_light_list* and rtsh_wide_filter_guided_temporal_mean_soft_light_list* -- restated
in numpy from the header's text and independently of the C++: float32 for the geometry of a tap (list_wide_guided_cases' ``_geom``,
every comparison fails on a NaN), int64 arrays, ``//`` and ``math.isqrt`` for everything that is summed; the input V_0', the threshold
with its two branches of E* and both passes are written out here.  No GPU code is touched here.

Frames, lists, count planes and PASSES / K4 are list_wide_guided_cases'; length planes, the awkward history planes and ``moments_rule``
are list_moments_cases'.  MEAN PLANES come in four kinds (``moments_of``), each a triple (mean, square, lengths) of 8 planes:
  "exact"    mean == min(c, n_l) * S_l of the count planes (anchor 1); square and lengths awkward (list_moments_cases.history), so both
             branches of E* are taken while the passes see the count-input filter's own values;
  "chained"  ``moments_rule`` chained over 3 frames of differing counts through a camera that maps every pixel of the flat frame onto
             itself (on other frames: onto whatever the rule says), max_length 4;
  "hashed"   list_moments_cases.history: mean 0, 65535 or hashed over 0 .. 65535 -- the clamp bites for every n_l with n_l * S_l < 65535
             (4: 65532, 16 and 48: 65520) --, square below, at and above mean^2, lengths 0, 1, 2, 254, 255 in turn;
  "constant" mean 30000 everywhere (anchor 3), square and lengths as in "hashed".
The census (``census_ok``) holds conditions on the RULE alone and is asserted with the "hashed" planes on every frame at least 40
pixels wide, for every list: a pixel where V_0' differs from V_0 of the counts inside the temporal branch of E* and one inside the
fallback; a clamped value; at guide_k4 8 and 12 a guide-rejected tap and an accepted tap of another value; T = 0 and T in between (8,
12), T = 65535 (255) -- each for every light of two samples or more (the clamp: for the frame)."""
import numpy as np

import list_filter_cases as fc
import list_moments_cases as mc
import list_wide_guided_cases as gc
from raytracedshadows_amd import api

f32, i64 = np.float32, np.int64

FRAMES = gc.FRAMES
PASSES = gc.PASSES
K4 = gc.K4
KINDS_OF_MEAN = ["exact", "chained", "hashed", "constant"]
MIN_HISTORY = mc.MIN_HISTORY
CONSTANT = 30000
same_bits = gc.same_bits
samples_of = gc.samples_of
the_list = gc.the_list
lists = gc.lists
kinds = gc.kinds
frame = gc.frame
counts = gc.counts


def filter_params(passes, kind="geometric"):
    if kind in ("geometric", "flat"):
        return api.WideFilterParams.make(passes, 0.9, 0.02)
    return api.WideFilterParams.make(passes, 0.5, 10.0)


guide_params = mc.params


def _nS(lst):
    n_l = np.array(samples_of(lst), i64).reshape(-1, 1, 1)
    return n_l, 65535 // n_l


def v0_of_counts(lst, planes):
    """int64[count, H, W]: V_0 = min(c, n_l) * S_l."""
    n_l, S_l = _nS(lst)
    return np.minimum(np.asarray(planes)[:lst.count].astype(i64), n_l) * S_l


def overhead_camera(wh, max_length=4):
    """(TemporalParams, eye_delta float32[3]) of a camera above the flat frame's floor that reprojects pixel (x, y) of that frame onto
    (x, y): positions there are (x, 0, y) * STEP, so with the eye one unit above, forward = down, scale = STEP * size / 2 the header's
    REPROJECT gives fx = x up to rounding, which the 1/32-pixel grid absorbs."""
    W, H = wh
    sx, sy = fc.STEP * W / 2.0, fc.STEP * H / 2.0
    eye = (sx * (1.0 - 1.0 / W), 1.0, sy * (1.0 - 1.0 / H))
    delta = tuple(-v for v in eye)
    return api.TemporalParams.make(delta, (1, 0, 0), (0, 0, -1), (0, -1, 0), sx, sy, 0.9, 1e-3, max_length, 0), np.array(delta, f32)


_MOMENTS = {}


def moments_of(kind_of_mean, kind, wh, lst):
    """(uint16[8, H, W] mean, uint32[8, H, W] square, uint8[8, H, W] lengths) of a kind (planes from the count up: 0xEE.., never to be
    read); cached and read-only."""
    key = (kind_of_mean, kind, wh, tuple(samples_of(lst)))
    if key in _MOMENTS:
        return _MOMENTS[key]
    W, H = wh
    count = lst.count
    mean, square = (a.copy() for a in mc.history(wh, lst))
    lengths = mc.filter_lengths(wh).copy()
    if kind_of_mean == "exact":
        mean[:count] = v0_of_counts(lst, counts(wh, lst)).astype(np.uint16)
    elif kind_of_mean == "constant":
        mean[:count] = CONSTANT
    elif kind_of_mean == "chained":
        nrm, pos, lights_map = frame(kind, wh)
        p, delta = overhead_camera(wh)
        with np.errstate(all="ignore"):
            prev_pos = np.ascontiguousarray(pos, f32).copy()
            prev_pos[..., :3] = prev_pos[..., :3] + delta
        prev = None
        for k in range(3):
            c = np.ascontiguousarray(np.roll(counts(wh, lst), 5 * k, axis=2))
            m = mc.moments_rule(lst, p, pos, nrm, c, prev, lights_map)
            prev = (prev_pos, nrm) + m
        mean[:count], square[:count], lengths[:count] = prev[2:]
    else:
        assert kind_of_mean == "hashed"
    out = (mean, square, lengths)
    for a in out:
        a.setflags(write=False)
    _MOMENTS[key] = out
    return out


def chained_counts(wh, lst):
    """The count planes of the LAST frame of the "chained" kind: what that frame's guided filter takes as `counts`."""
    return np.ascontiguousarray(np.roll(counts(wh, lst), 10, axis=2))


def counts_for(kind_of_mean, wh, lst):
    return chained_counts(wh, lst) if kind_of_mean == "chained" else counts(wh, lst)


def _active(lst, normals, lights_map):
    n = np.ascontiguousarray(normals, f32)
    H, W = n.shape[:2]
    bg = (n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0)
    on = np.ones((lst.count, H, W), bool) if lights_map is None else \
        np.stack([((np.asarray(lights_map, np.uint8) >> l) & 1) != 0 for l in range(lst.count)])
    return on & ~bg


def mean_input(lst, mean, active):
    """INPUT: V_0' = min(mean, n_l * S_l) at an active (pixel, light), 0 elsewhere."""
    n_l, S_l = _nS(lst)
    return np.where(active, np.minimum(np.asarray(mean)[:lst.count].astype(i64), n_l * S_l), 0)


def _output(lst, V, active):
    n_l, S_l = _nS(lst)
    assert int(V.min()) >= 0 and (V <= n_l * S_l).all()
    return np.where(active, V.astype(f32) / (n_l * S_l).astype(f32), f32(0.0)).astype(f32)


def _passes(lst, p, positions, normals, V, active, T, max_passes, kind, wh, census=None):
    """[float32 planes for passes = 0 .. max_passes]; T None: the unguided pass.  RANGE is asserted per pass."""
    count = lst.count
    outs = [_output(lst, V, active)]
    rejected, moved = np.zeros(count, i64), np.zeros(count, i64)
    for k in range(max_passes):
        taps = gc._geom(kind, wh, positions, normals, p.normal_cos_min, p.plane_eps, 1 << k)[1]
        num, den = 36 * V, np.full(V.shape, 36, i64)
        lo, hi = V.copy(), V.copy()
        for w, qy, qx, geom in taps:
            q = V[:, qy, qx]
            reach = geom[None] & active[:, qy, qx] & active
            diff = np.abs(q - V)
            acc = reach if T is None else reach & (diff <= T)
            num += np.where(acc, w * q, 0)
            den += np.where(acc, w, 0)
            lo, hi = np.where(acc, np.minimum(lo, q), lo), np.where(acc, np.maximum(hi, q), hi)
            rejected += (reach & ~acc).sum(axis=(1, 2))
            moved += (acc & (diff != 0)).sum(axis=(1, 2))
        assert int(num.max()) < 1 << 24 and int(den.max()) <= 256
        V = np.where(active, (2 * num + den) // (2 * den), 0)
        assert ((V >= lo) & (V <= hi))[active].all()                      # anchor 4, in the rule itself
        outs.append(_output(lst, V, active))
    if census is not None:
        census["taps"] = {l: [int(rejected[l]), int(moved[l])] for l in range(count)}
    return outs


def mean_filter_rule(lst, p, positions, normals, mean, lights_map=None, max_passes=5, kind=None, wh=None):
    """[float32[count, H, W] for passes = 0 .. max_passes] of rtsh_wide_filter_mean_soft_light_list (p.passes is not looked at)."""
    active = _active(lst, normals, lights_map)
    return _passes(lst, p, positions, normals, mean_input(lst, mean, active), active, None, max_passes, kind, wh)


def thresholds(lst, k4, min_history, planes, moments, active, census=None):
    """int64[count, H, W]: T(p, l), 0 at an inactive pixel.  E* from the UNCLAMPED moments where lengths >= min_history, from this
    frame's count elsewhere; G, D over the 3 x 3 of counted pixels, no geom test."""
    count = lst.count
    n_l, S_l = _nS(lst)
    H, W = active.shape[1:]
    V0 = v0_of_counts(lst, planes)
    mean, square, lengths = (np.asarray(a)[:count].astype(i64) for a in moments)
    temporal = lengths >= int(min_history)
    E = np.where(temporal, n_l * np.maximum(0, square - mean * mean), V0 * (n_l * S_l - V0))
    E = np.where(active, E, 0)
    G, D = np.zeros((count, H, W), i64), np.zeros((count, H, W), i64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            w = (2 - abs(dx)) * (2 - abs(dy))
            ys, yd = slice(max(0, dy), H + min(0, dy)), slice(max(0, -dy), H + min(0, -dy))
            xs, xd = slice(max(0, dx), W + min(0, dx)), slice(max(0, -dx), W + min(0, -dx))
            G[:, yd, xd] += w * E[:, ys, xs]
            D[:, yd, xd] += w * active[:, ys, xs]
    assert int(G.max()) < 1 << 42 and int(k4) * int(k4) * int(G.max()) < 1 << 58
    T = np.minimum(65535, gc.isqrt_array((int(k4) * int(k4) * G) // (16 * np.maximum(D, 1) * n_l)))
    T = np.where(active, np.where(n_l <= 1, 65535, T), 0)
    if census is not None:
        differs = active & (mean_input(lst, moments[0], active) != V0)
        census["differs"] = {l: [int((differs[l] & temporal[l]).sum()), int((differs[l] & ~temporal[l]).sum())] for l in range(count)}
        census["clamped"] = int((active & (mean > n_l * S_l)).sum())
        census["T"] = {l: (bool((T[l][active[l]] == 0).any()), bool(((T[l][active[l]] > 0) & (T[l][active[l]] < 65535)).any()),
                           bool((T[l][active[l]] == 65535).any())) for l in range(count)}
    return T


def guided_mean_rule(lst, p, positions, normals, planes, moments, lights_map=None, max_passes=5, census=None, kind=None, wh=None):
    """([float32[count, H, W] for passes = 0 .. max_passes], int64 T) of rtsh_wide_filter_guided_temporal_mean_soft_light_list
    (p.passes is not looked at; p.guide_k4 and p.min_history are).  ``planes``: this frame's counts."""
    active = _active(lst, normals, lights_map)
    T = thresholds(lst, p.guide_k4, p.min_history, planes, moments, active, census)
    return _passes(lst, p, positions, normals, mean_input(lst, moments[0], active), active, T, max_passes, kind, wh, census), T


def census_ok(lst, census, k4, what):
    assert census["clamped"] > 0 or max(samples_of(lst)) < 2, (what, "clamped")
    for l, n in enumerate(samples_of(lst)):
        if n < 2:
            continue
        assert census["differs"][l][0] > 0 and census["differs"][l][1] > 0, (what, "differs", l, census["differs"][l])
        zero, mid, top = census["T"][l]
        if k4 in (8, 12):
            assert zero and mid, (what, "T", l, census["T"][l])
            assert census["taps"][l][0] > 0 and census["taps"][l][1] > 0, (what, "taps", l, census["taps"][l])
        if k4 == 255:
            assert top, (what, "T", l, census["T"][l])


def centre_quotient(lst, mean, normals, lights_map=None):
    """Anchor 2: (float)min(mean, n S) / (float)(n S) at an active pixel, +0 elsewhere."""
    active = _active(lst, normals, lights_map)
    return _output(lst, mean_input(lst, mean, active), active)
