"""Shared by the wide filter tests (tests/test_list_wide_filter_host.py, tests/test_gpu_list_wide_filter.py): lists, frames and the
expected floats of the wide (a-trous) filter of a light list's planes (include/rts_scene.h, rtsh_wide_filter_light_list* /
rtsh_wide_filter_soft_light_list*) from a numpy restatement of its rule, written here from the header's text and independently of the
C++: integer arrays, ``//``, float32 comparisons that a NaN fails, one float32 division.  No GPU code is touched here.

The frames are those of tests/list_filter_cases.py (its generators, imported), at its sizes and at the sizes this filter adds:
3 x 2 and 17 x 1 (at large steps every tap but the centre is outside), 72 x 72 (the smallest frame in which a step-16 pass has pixels
with both the -32 and the +32 tap inside), 40 x 72 and 72 x 40 (partial blocks on one side).  Floats are compared bit for bit."""
import numpy as np

import list_filter_cases as fc
from raytracedshadows_amd import api

f32, u32 = np.float32, np.uint32

#: the filter's own frames, both kinds
SMALL = list(fc.FRAMES)
#: the sizes this filter adds
WIDE = [(3, 2), (17, 1), (72, 72), (40, 72), (72, 40)]
FRAMES = SMALL + WIDE
PASSES = [0, 1, 2, 3, 4, 5]
COUNTS = [1, 4, 8]
#: n_l of a soft list's entries: entry l has SAMPLES[(l + rotation) % 4]
SAMPLES = [1, 4, 16, 48]
WEIGHT = {0: 6, 1: 4, 2: 1}

same_bits = fc.same_bits
#: kinds of frame: list_filter_cases' two, and "flat" at the sizes this filter adds
KINDS = ["awkward", "geometric", "flat"]

_FLAT = {}


def flat(wh):
    """One floor without a crease or a step (and a sprinkle of background): every tap inside the frame passes geom, so the far taps of
    the step-8 and step-16 passes are accepted on both sides of a pixel -- which the geometric frame's crease and step prevent.  Planes
    of random bytes (some above n_l), a random map."""
    if wh not in _FLAT:
        W, H = wh
        y, x = np.mgrid[0:H, 0:W]
        nrm = np.zeros((H, W, 4), f32)
        pos = np.ones((H, W, 4), f32)
        nrm[..., 1] = 1.0
        pos[..., 0], pos[..., 1], pos[..., 2] = x * fc.STEP, 0.0, y * fc.STEP
        background = (3 * x + 5 * y) % 41 == 9
        nrm[background] = 0
        pos[background] = np.nan
        rs = np.random.RandomState(77 * W + H)
        lights_map = rs.randint(0, 256, (H, W)).astype(np.uint8) | np.uint8(0x42)
        mask = rs.randint(0, 256, (H, W)).astype(np.uint8)
        planes = np.stack([rs.randint(0, SAMPLES[l % 4] + 2, (H, W)) for l in range(8)]).astype(np.uint8)
        arrays = (nrm, pos, np.ascontiguousarray(planes), mask, lights_map, np.zeros((8, H, W), f32))
        for a in arrays:
            a.setflags(write=False)
        _FLAT[wh] = arrays
    return _FLAT[wh]


def frame(kind, wh):
    return flat(wh) if kind == "flat" else fc.frame(kind, wh)


def kinds(wh):
    return KINDS if wh in WIDE else KINDS[:2]


def params(passes, kind="geometric"):
    """The thresholds of list_filter_cases.params for the kind of frame."""
    if kind in ("geometric", "flat"):
        return api.WideFilterParams.make(passes, 0.9, 0.02)
    return api.WideFilterParams.make(passes, 0.5, 10.0)


_LISTS = {}


def the_list(form, count, rotation=0):
    """A hard (``LightList``) or soft (``SoftLightList``) list of ``count`` lights, directional and point in turn; soft entry l has
    SAMPLES[(l + rotation) % 4] samples."""
    key = (form, count, rotation)
    if key not in _LISTS:
        where = [(api.Light.POINT if l & 1 else api.Light.DIRECTIONAL, [0.6 - 0.3 * l, 0.64, 0.48 + l]) for l in range(count)]
        if form == "hard":
            _LISTS[key] = api.LightList.make(where)
        else:
            entries = []
            for l, (kind, xyz) in enumerate(where):
                n = SAMPLES[(l + rotation) % 4]
                entries.append((kind, xyz, n, 0 if n < 2 else 48 - n, 0.25))
            _LISTS[key] = api.SoftLightList.make(entries, np.zeros((48, 3), f32))
    return _LISTS[key]


def lists():
    """(form, count, rotation) of every list: hard and soft, 1, 4 and 8 lights, every n_l of SAMPLES in every entry."""
    return [("hard", c, 0) for c in COUNTS] + [("soft", c, r) for c in COUNTS for r in range(4)]


def samples_of(lst):
    hard = isinstance(lst, api.LightList)
    return [1 if hard else max(1, int(lst.lights[l].nsamples)) for l in range(lst.count)]


_GEOM = {}


def _taps(positions, normals, cos_min, eps, step):
    """[(weight, qy, qx, geom, dx, dy)] of the 24 taps of a pass beside the centre: geom = inside the frame, not bg(q), the normal test, the
    plane test; evaluated once per (frame, thresholds, step) -- it does not depend on the light."""
    key = (hash(np.ascontiguousarray(positions, f32).tobytes()), hash(np.ascontiguousarray(normals, f32).tobytes()), np.shape(normals), float(cos_min),
           float(eps), step)
    if key not in _GEOM:
        n = np.ascontiguousarray(normals, f32)
        P = np.ascontiguousarray(positions, f32)
        H, W = n.shape[:2]
        nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
        bg = (nx == 0) & (ny == 0) & (nz == 0)
        yy, xx = np.mgrid[0:H, 0:W]
        out = []
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
                    Dx, Dy, Dz = P[qy, qx, 0] - P[..., 0], P[qy, qx, 1] - P[..., 1], P[qy, qx, 2] - P[..., 2]
                    h = (nx * Dx + ny * Dy) + nz * Dz
                    assert cos.dtype == f32 and h.dtype == f32
                    geom = inside & ~bg[qy, qx] & (cos >= f32(cos_min)) & (np.abs(h) <= f32(eps))
                    out.append((u32(WEIGHT[abs(dx)] * WEIGHT[abs(dy)]), qy, qx, geom, dx, dy))
        _GEOM[key] = (bg, out)
    return _GEOM[key]


def wide_filter_rule(lst, p, positions, normals, planes, lights_map=None, max_passes=5, census=None):
    """[float32[count, H, W] for passes = 0 .. max_passes] of the wide filter, from the header's text (p.passes is not looked at).
    ``lst`` a ``LightList``: ``planes`` is the mask, c_l = its bit l, n_l = 1; a ``SoftLightList``: c_l = planes[l].  ``census``: a
    dict that receives, per pass, [taps accepted, taps rejected by geom] among the taps inside the frame of active pixels."""
    hard = isinstance(lst, api.LightList)
    count = lst.count
    planes = np.ascontiguousarray(planes, np.uint8)
    H, W = np.asarray(normals).shape[:2]
    n_l = samples_of(lst)
    S_l = [65535 // n for n in n_l]
    bg = _taps(positions, normals, p.normal_cos_min, p.plane_eps, 1)[0]
    on = [np.ones((H, W), bool) if lights_map is None else ((np.asarray(lights_map, np.uint8) >> l) & 1) != 0 for l in range(count)]
    active = [~bg & on[l] for l in range(count)]
    V = []
    for l in range(count):
        c = (((planes >> l) & 1) if hard else planes[l]).astype(u32)
        V.append(np.where(active[l], np.minimum(c, u32(n_l[l])) * u32(S_l[l]), u32(0)).astype(u32))

    def output():
        out = np.zeros((count, H, W), f32)
        for l in range(count):
            assert int(V[l].max()) <= n_l[l] * S_l[l] <= 65535
            out[l] = np.where(active[l], V[l].astype(f32) / f32(n_l[l] * S_l[l]), f32(0.0))
        return out

    outs = [output()]
    for k in range(max_passes):
        taps = _taps(positions, normals, p.normal_cos_min, p.plane_eps, 1 << k)[1]
        if census is not None:
            census[k] = [0, 0]
        nxt = []
        for l in range(count):
            num, den = u32(36) * V[l], np.full((H, W), 36, u32)
            for w, qy, qx, geom, _, _ in taps:
                acc = geom & on[l][qy, qx]
                num = num + np.where(acc, w * V[l][qy, qx], u32(0)).astype(u32)
                den = den + np.where(acc, w, u32(0)).astype(u32)
                if census is not None and l == 0:
                    census[k][0] += int((geom & ~bg).sum())
                    census[k][1] += int((~geom & ~bg).sum())
            assert int(num.max()) < 1 << 24 and int(den.max()) <= 256
            nxt.append(np.where(active[l], (u32(2) * num + den) // (u32(2) * den), u32(0)).astype(u32))
        V = nxt
        outs.append(output())
    return outs


def centre_quotient(lst, planes, normals, lights_map=None):
    """float32[count, H, W]: (float)min(c, n_l) / (float)n_l where the pixel is active, +0 elsewhere -- anchor 1."""
    hard = isinstance(lst, api.LightList)
    nrm = np.asarray(normals, f32)
    bg = (nrm[..., :3] == 0).all(axis=-1)
    out = np.zeros((lst.count,) + bg.shape, f32)
    for l, n in enumerate(samples_of(lst)):
        on = ~bg & ((((np.asarray(lights_map) >> l) & 1) != 0) if lights_map is not None else True)
        c = ((np.asarray(planes) >> l) & 1) if hard else np.asarray(planes)[l]
        out[l] = np.where(on, np.minimum(c, n).astype(f32) / f32(n), f32(0))
    return out
