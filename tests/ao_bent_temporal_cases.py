"""Shared by the bent temporal tests (tests/test_ao_bent_temporal_host.py, tests/test_gpu_ao_bent_temporal.py): the numpy rules of
include/rts_scene.h's rtsh_accumulate_bent* and rtsh_wide_filter_bent_mean* (DESIGN.md 4.39), restated from the header's text and
independently of the C++ -- float32 for the geometry, int64 sums, ``//`` -- and the planes the tests feed them.  Reused, none of them
edited: ``list_moments_cases._taps`` (REPROJECT and the acceptance of a tap), ``list_motion_cases.reproject_inputs`` (the motion form
put in front of the same blend), ``ao_bent_filter_cases`` (quantise, output, the synthetic float planes), ``list_temporal_cases``
(the geometric pairs of the four motions, the length planes).  The twin and the kernels are compared only with these rules, as bits.

THE GUARDS (``accumulate_census_ok``, ``mean_census_ok``) are conditions on the RULE alone, asserted on every frame at least 40 pixels
wide and every motion but "away".  Every frame of the grid meets every one of them with the history of salt 3 (``case``): no frame
needed a salt of its own."""
import numpy as np

import ao_bent_filter_cases as bf
import list_moments_cases as mc
import list_motion_cases as ms
import list_temporal_cases as tc
import list_wide_filter_cases as wc
from raytracedshadows_amd import api

f32, u32, u64, i64 = np.float32, np.uint32, np.uint64, np.int64

MOTIONS = tc.MOTIONS
FRAMES = [(72, 40), (40, 40), (17, 1), (3, 2)]
MAX_LENGTHS = (1, 2, 5, 255)
SAMPLES = (1, 4, 48)
PASSES = bf.PASSES


# ------------------------------------------------------------------------------------------------------------------- the texel
def pack(X):
    """uint64[H, W] from int64[H, W, 4]: int16 x, y, z then uint16 V, lowest bits first."""
    X = np.asarray(X, i64)
    assert (X[..., :3] >= -32768).all() and (X[..., :3] <= 32767).all() and (X[..., 3] >= 0).all() and (X[..., 3] <= 65535).all()
    w = (X & 0xFFFF).astype(u64)
    return np.ascontiguousarray(w[..., 0] | (w[..., 1] << u64(16)) | (w[..., 2] << u64(32)) | (w[..., 3] << u64(48)))


def unpack(texels):
    """int64[H, W, 4] from uint64[H, W]: the three signed components and V."""
    t = np.ascontiguousarray(texels, u64)
    c = np.stack([((t >> u64(s)) & u64(0xFFFF)).astype(i64) for s in (0, 16, 32, 48)], -1)
    c[..., :3] = np.where(c[..., :3] >= 32768, c[..., :3] - 65536, c[..., :3])
    return c


def same_texels(got, want, what):
    for g, w, name, dtype in zip(got, want, ("texels", "lengths"), (u64, np.uint8)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, name, bad.shape[0], [(tuple(i), hex(int(g[tuple(i)])), hex(int(w[tuple(i)]))) for i in bad[:4].tolist()])


# ------------------------------------------------------------------------------------------------------------------- the planes
def active_plane(wh, salt=0):
    """uint8[H, W]: a fifth of the bytes 0, the others 1, 2, 0x80 or 255 -- any non-zero byte is active."""
    W, H = wh
    y, x = np.mgrid[0:H, 0:W].astype(i64)
    h = (x * 7919 + y * 104729 + salt * 31 + (x * y) % 11) % 65536
    return np.ascontiguousarray(np.where(h % 5 == 0, 0, np.array([1, 2, 0x80, 255], np.uint8)[h % 4]).astype(np.uint8))


def history(wh, salt=3, symmetric=False):
    """(uint64[H, W] texels, uint8[H, W] lengths): a hashed awkward history -- components 0x8000 (-32768) and 0x7FFF, small values of
    both signs, V = 65535, 0 and hashed; lengths 0, 1, 2, 254, 255 in turn (list_temporal_cases.lengths, plane 0).  ``symmetric``:
    no component is -32768 (the negation anchor: that value has no negative)."""
    W, H = wh
    y, x = np.mgrid[0:H, 0:W].astype(i64)
    X = np.zeros((H, W, 4), i64)
    for c in range(3):
        h = (x * 2654435761 + y * 40503 + (c + salt) * 977 + (x * y) % 7) % 65536
        v = np.where(h % 6 == 0, -32768, np.where(h % 6 == 1, 32767, np.where(h % 6 == 2, (h % 5) - 2, h - 32768)))
        X[..., c] = np.where((v == -32768) & symmetric, -32767, v)
    h = (x * 40503 + y * 2654435761 + salt * 131) % 65536
    X[..., 3] = np.where(h % 4 == 0, 65535, np.where(h % 4 == 1, 0, h))
    return pack(X), np.ascontiguousarray(tc.lengths(wh, salt)[0])


_CASES = {}


def case(motion, wh, nsamples):
    """list_temporal_cases' geometric pair of a motion with this file's planes: params, G-buffers, ``active``, the synthetic float plane
    of ao_bent_filter_cases and the four prev_*.  Shared, read-only."""
    key = (motion, wh, nsamples)
    if key not in _CASES:
        c = tc.geometric(motion, wh)
        texels, lengths = history(wh)
        d = dict(params=c["params"], pos=c["pos"], nrm=c["nrm"], active=active_plane(wh), bent=bf.synthetic_bent(wh, nsamples),
                 prev=(c["prev_pos"], c["prev_nrm"], texels, lengths))
        for v in (d["active"], texels, lengths):
            v.setflags(write=False)
        _CASES[key] = d
    return _CASES[key]


def counted_bent(wh, nsamples, salt=0):
    """(counts uint8[H, W], bent float32[H, W, 4]) as a trace gives them: the synthetic vectors with .w = the integer count <= n."""
    W, H = wh
    n = max(1, nsamples)
    counts = np.random.RandomState(77 * W + H + n + salt).randint(0, n + 1, (H, W)).astype(np.uint8)
    bent = np.array(bf.synthetic_bent(wh, nsamples))
    bent[..., 3] = counts
    return counts, bent


_PAIRS = {}


def pair(name, move, wh, camera):
    """Two frames of a moved scene (list_motion_cases): frame 0 from the previous stream and eye, frame 1 the motion G-buffer pass."""
    key = (name, move, wh, camera)
    if key not in _PAIRS:
        s = ms.streams(name, move)
        W, H = wh
        eye, prev_eye = ms.cameras(s, camera)
        p0, n0, _, _, _, _ = api.primary_gbuffer_motion(s["prev_packed"], s["prev_packed"], prev_eye, prev_eye, s["target"], s["fovy"], W, H)
        pos, nrm, pts, pnr, _, _ = api.primary_gbuffer_motion(s["packed"], s["prev_packed"], eye, prev_eye, s["target"], s["fovy"], W, H)
        _PAIRS[key] = dict(prev_pos=p0, prev_nrm=n0, pos=pos, nrm=nrm, pts=pts, pnr=pnr, params=ms.params_of(s, wh, eye, prev_eye, max_length=255))
    return _PAIRS[key]


# --------------------------------------------------------------------------------------------------------- stage 1: the accumulate
def accumulate_rule(p, nsamples, positions, normals, bent, prev=None, active=None, census=None, parts=None):
    """(uint64[H, W] texels, uint8[H, W] lengths) from the header's text.  ``prev``: None or (prev_positions, prev_normals, prev_texels,
    prev_lengths).  ``census``: a dict that receives the number of blended pixels with two or more accepted taps ("shared"), with a tap
    of non-zero weight that was not accepted ("rejected") and with a negative num in some component ("negative").  ``parts``: a dict
    that receives X_0, the output as int64[H, W, 4], the blend mask and, per component, the smallest and largest value among the
    accepted history values and the current one ("lo", "hi")."""
    act = bf.active_of(normals, active)
    H, W = act.shape
    X0 = bf.quantise_rule(bent, nsamples, act)
    out, out_len = X0.copy(), np.where(act, 1, 0).astype(i64)
    blend = np.zeros((H, W), bool)
    lo, hi = X0.copy(), X0.copy()
    if census is not None:
        census.update(shared=0, rejected=0, negative=0)
    if prev is not None and not int(p.reset_lights) & 1:
        taps = mc._taps(p, positions, normals, prev[0], prev[1])[1]
        hist, pl = unpack(prev[2]), np.asarray(prev[3]).astype(i64)
        sw, s, m = np.zeros((H, W), i64), np.zeros((H, W, 4), i64), np.full((H, W), 255, i64)
        accepted, refused = np.zeros((H, W), i64), np.zeros((H, W), bool)
        for geom, w, cy, cx, nonzero in taps:
            acc = geom & act & (pl[cy, cx] != 0)
            sw += np.where(acc, w, 0)
            s += np.where(acc[..., None], w[..., None] * hist[cy, cx], 0)
            m = np.where(acc, np.minimum(m, pl[cy, cx]), m)
            lo = np.where(acc[..., None], np.minimum(lo, hist[cy, cx]), lo)
            hi = np.where(acc[..., None], np.maximum(hi, hist[cy, cx]), hi)
            accepted += acc
            refused |= nonzero & act & ~acc
        nf = np.minimum(m + 1, int(p.max_length))
        blend = act & (sw != 0) & (nf != 1)
        den = np.where(blend, nf * sw, 1)[..., None]
        num = (nf - 1)[..., None] * s + sw[..., None] * X0
        assert int(np.abs(s).max()) <= 1 << 26 and int(np.abs(num).max()) < 1 << 35 and int(den.max()) < 1 << 18
        assert (num[..., 3] >= 0).all()
        mean = np.sign(num) * ((2 * np.abs(num) + den) // (2 * den))        # the rounded mean, half away from zero
        out = np.where(blend[..., None], mean, out)
        out_len = np.where(act & (sw != 0), nf, out_len)
        if census is not None:
            census["shared"] = int((blend & (accepted >= 2)).sum())
            census["rejected"] = int((blend & refused).sum())
            census["negative"] = int((blend & (num[..., :3] < 0).any(-1)).sum())
    if parts is not None:
        parts.update(X0=X0, out=out, blend=blend, lo=lo, hi=hi, act=act)
    return pack(out), out_len.astype(np.uint8)


def accumulate_motion_rule(p, nsamples, normals, bent, prev, active, motion, census=None, parts=None):
    """The motion form: list_motion_cases' REPROJECT in front of the same blend."""
    if prev is None:                                                       # the first frame reads neither motion plane
        q, P, n = p, np.zeros(np.shape(normals), f32), np.ascontiguousarray(normals, f32)
    else:
        q, P, n = ms.reproject_inputs(p, normals, motion[0], motion[1])
    return accumulate_rule(q, nsamples, P, n, bent, prev, active, census, parts)


def accumulate_census_ok(motion, wh, census, what):
    if motion != "away" and wh[0] >= 40:
        assert census["shared"] > 0 and census["rejected"] > 0 and census["negative"] > 0, (what, census)


# ------------------------------------------------------------------------------------------- stage 2: the filter over the texels
def mean_input_rule(texels, nsamples, act):
    """int64[H, W, 4]: X_0' and V_0' of the header -- the clamped texel; four zeros where the pixel is inactive."""
    n, S_b, S_l = bf.scales(nsamples)
    X = unpack(texels)
    X[..., :3] = np.clip(X[..., :3], -(n * S_b), n * S_b)
    X[..., 3] = np.minimum(X[..., 3], n * S_l)
    return np.where(act[..., None], X, 0)


def mean_filter_rule(p, nsamples, positions, normals, texels, active=None, max_passes=5, census=None):
    """[float32[H, W, 4] for passes = 0 .. max_passes] (p.passes is not looked at): rtsh_wide_filter_bent's passes, restated, over the
    clamped texel.  ``census``: a dict that receives "clamped", the number of active pixels at which the clamp changes a component."""
    H, W = np.asarray(normals).shape[:2]
    act = bf.active_of(normals, active)
    X = mean_input_rule(texels, nsamples, act)
    if census is not None:
        census["clamped"] = int((act & (X != unpack(texels)).any(-1)).sum())
    outs = [bf.output_rule(X, nsamples, act)]
    for k in range(max_passes):
        taps = wc._taps(positions, normals, p.normal_cos_min, p.plane_eps, 1 << k)[1]
        num, den = 36 * X, np.full((H, W), 36, i64)
        lo, hi = X.copy(), X.copy()
        for w, qy, qx, geom, dx, dy in taps:
            acc = geom & act[qy, qx] & act
            num = num + np.where(acc[..., None], int(w) * X[qy, qx], 0)
            den = den + np.where(acc, int(w), 0)
            lo = np.where(acc[..., None], np.minimum(lo, X[qy, qx]), lo)
            hi = np.where(acc[..., None], np.maximum(hi, X[qy, qx]), hi)
        d = den[..., None]
        nxt = np.sign(num) * ((2 * np.abs(num) + d) // (2 * d))
        assert ((nxt >= lo) & (nxt <= hi))[act].all()                       # RANGE, in the rule itself
        X = np.where(act[..., None], nxt, 0)
        outs.append(bf.output_rule(X, nsamples, act))
    return outs


def mean_census_ok(wh, census, what):
    if wh[0] >= 40:
        assert census["clamped"] > 0, (what, census)
