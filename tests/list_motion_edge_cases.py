"""Shared by the awkward-input tests of the motion family (tests/test_list_motion_edges_host.py, tests/test_gpu_list_motion_edges.py):
synthetic motion planes laid over the pairs of tests/list_temporal_cases.py, a census of them, small streams for the motion G-buffer
pass and a helper that poisons a previous stream.  The expected values are the numpy rules of tests/list_motion_cases.py, unedited.
No GPU code is touched here.

  motion_planes(case, wh, salt)   (prev_points, prev_point_normals) float32[H, W, 4] for a case of list_temporal_cases.  Every texel
      starts as the STATIC one -- positions + eye_delta with .w = 1, and the current normal -- and the pixels are then dealt into eight
      groups by (pixel index + salt) % 8, j = (pixel index + salt) // 8 choosing within a group; nothing is random:
        0, 7  untouched: STATIC.
        1     Q, one component (j % 3) replaced by Q_VALUES[(j // 3) % 10]: NaN, +-Inf, +-1e-41 (denormal), +-3e38, +-0 and 1e-20.
        2     Q shifted by OFFSETS[j % 8], a hundredth of a unit: the four taps and their weights fall elsewhere.
        3     Q constructed for one bound of the on-screen test, BOUNDS[j % 11] (bounds_points below).
        4     M_p, one component (j % 3) replaced by M_VALUES[(j // 3) % 8]: 0, -0.0, NaN, Inf, 1e30, 1e-41, -1 and 0.6 (non-unit).
        5     M_p all +0 (j even) or all -0.0 (j odd): both must restart.
        6     garbage in the .w lane of both texels, NaN included: the rule reads three components only.
      A frame of fewer than 8 pixels sees every group through `salt`.
  bounds_points(p, wh)   the eleven points of group 3, built in float64 from the previous camera's basis in `p`, searched over a few
      hundred float32 neighbours for the one that sits ON the bound, and confirmed -- asserted here, on the CPU -- with the float32
      `reprojection` expression of tests/test_list_motion_host.py: the intended side of the intended comparison is taken and every
      other comparison of the on-screen test holds, so the bound alone decides.
  census()   on the 40 x 40 "pixels" pair with a map of all ones and prev_lengths all 7, from the numpy rules alone: in groups 1 and 4
      at least 20 pixels blend and at least 20 restart that the non-motion parent blends; in group 2 at least 20 blend; in group 5 none.
  small_streams() / cameras_of()   "one" (a single triangle: the root is a leaf), "quad" (two triangles, one of them moves) and
      "cornell" with its moved box (list_motion_cases.streams), each with its cameras: the eye inside the moved box and a camera that
      misses everything among them.
  poison(prev_packed, kind)   a copy of a previous stream with words overwritten; tag and link words (3 and 7 of a node) stay.
        "leaf_words"  in every second leaf, one of its nine words -- and in every sixth all nine -- takes NaN, +Inf or 1e-41 in turn;
        "sign"        the sign bit of every zero word among the leaves' nine words is flipped: -0.0 against +0.0 is MOVED by the
                      header's bit comparison although the values are equal;
        "never_read"  0x7FC00001 in the words the header says the pass never reads in prev: the six box words of every inner node and
                      the fourth word of every tail.
Floats are compared through a uint32 view: bit for bit."""
import numpy as np

import list_motion_cases as ms
import list_temporal_cases as tc
from raytracedshadows_amd import api

f32, u32 = np.float32, np.uint32
END = ms.END
NAN, INF = np.nan, np.inf

GROUPS = ("static", "q_replaced", "shifted", "bounds", "m_replaced", "m_zero", "w_garbage", "static")
Q_VALUES = np.array([NAN, INF, -INF, 1e-41, -1e-41, 3e38, -3e38, 0.0, -0.0, 1e-20], f32)
M_VALUES = np.array([0.0, -0.0, NAN, INF, 1e30, 1e-41, -1.0, 0.6], f32)
W_VALUES = np.array([NAN, INF, -1.0, 0.0, 3e38, 1e-41, 2.0, -0.0], f32)
OFFSETS = np.array([[0.01, 0, 0], [-0.01, 0, 0], [0, 0, 0.01], [0, 0, -0.01], [0.01, 0, 0.01], [-0.01, 0, -0.01], [0, 0.01, 0],
                    [0.007, -0.004, 0.009]], f32)
#: name -> is the point ON SCREEN.  z: the `z > 0` test; lo / hi: the `>= -32` and `< 32 * size` tests of gx and gy, from both sides
BOUNDS = (("z_tiny", True), ("z_zero", False), ("z_negative", False), ("gx_lo_on", True), ("gx_lo_off", False), ("gx_hi_on", True),
          ("gx_hi_off", False), ("gy_lo_on", True), ("gy_lo_off", False), ("gy_hi_on", True), ("gy_hi_off", False))
MAX_LENGTHS, RESETS = tc.MAX_LENGTHS, tc.RESETS
RADII, MARGINS = (0, 1, 2, 4), (0.0, 0.125, 3.0e38)
#: frames of the G-buffer pass on the small streams
GBUFFER_FRAMES = [(1, 1), (1, 5), (5, 1), (7, 9), (17, 15), (3, 333)]

_CACHE = {}


def groups(wh, salt=0):
    """(group int[H, W], j int[H, W]) of a frame."""
    W, H = wh
    i = np.arange(H * W, dtype=np.int64).reshape(H, W) + salt
    return i % 8, i // 8


# ------------------------------------------------------------------------------------------------------------ the bounds
def _reprojection(p, Q, W, H):
    import test_list_motion_host as host                                 # its float32 REPROJECT expression, as it stands
    return host.reprojection(p, Q, W, H)


def _g(p, Q, W, H):
    """(z, gx, gy) float32 of REPROJECT for the points Q, the header's expression."""
    dot3 = lambda v: (Q[..., 0] * f32(v[0]) + Q[..., 1] * f32(v[1])) + Q[..., 2] * f32(v[2])
    with np.errstate(all="ignore"):
        z = dot3(p.prev_fwd)
        a, b = dot3(p.prev_right) / z, dot3(p.prev_up) / z
        fx = (a / f32(p.prev_scale_x) + f32(1.0)) * (f32(0.5) * f32(W)) - f32(0.5)
        fy = (f32(1.0) - b / f32(p.prev_scale_y)) * (f32(0.5) * f32(H)) - f32(0.5)
        return z, fx * f32(32.0) + f32(0.5), fy * f32(32.0) + f32(0.5)


def _neighbours(q, axes, reach):
    """float32[n, 3]: q with the components `axes` moved by -reach .. reach units in the last place, every combination."""
    steps = np.arange(-reach, reach + 1, dtype=np.int64)
    out = np.repeat(q[None, :], len(steps) ** len(axes), 0).copy()
    grid = np.stack(np.meshgrid(*([steps] * len(axes)), indexing="ij"), -1).reshape(-1, len(axes))
    for k, axis in enumerate(axes):
        bits = out[:, axis].view(np.int32).astype(np.int64)
        moved = np.where(bits >= 0, bits + grid[:, k], bits - grid[:, k])   # (the sign never changes: |q| is far above `reach` ulps)
        out[:, axis] = moved.astype(np.int32).view(f32)
    return out


def bounds_points(p, wh):
    """float32[11, 3] in the order of BOUNDS, and the number of them that sit exactly on their bound."""
    key = ("bounds", bytes(p), wh)
    if key in _CACHE:
        return _CACHE[key]
    W, H = wh
    r, u, f = (np.array([float(v) for v in b], np.float64) for b in (p.prev_right, p.prev_up, p.prev_fwd))
    sx, sy = float(p.prev_scale_x), float(p.prev_scale_y)

    def point(gx, gy, z=2.0):                                             # float64: the inverse of REPROJECT for an orthonormal basis
        a = (((gx - 0.5) / 32.0 + 0.5) / (0.5 * W) - 1.0) * sx
        b = (1.0 - ((gy - 0.5) / 32.0 + 0.5) / (0.5 * H)) * sy
        return z * (f + a * r + b * u)

    mid_x, mid_y = 16.0 * W, 16.0 * H
    out, exact = np.zeros((len(BOUNDS), 3), f32), 0
    below = lambda v: float(np.nextafter(f32(v), f32(-INF)))
    targets = {"gx_lo_on": (0, -32.0), "gx_lo_off": (0, below(-32.0)), "gx_hi_on": (0, below(32.0 * W)), "gx_hi_off": (0, 32.0 * W),
               "gy_lo_on": (1, -32.0), "gy_lo_off": (1, below(-32.0)), "gy_hi_on": (1, below(32.0 * H)), "gy_hi_off": (1, 32.0 * H)}
    for k, (name, on) in enumerate(BOUNDS):
        if name == "z_tiny":
            q = (f * 1e-30).astype(f32)                                   # a normal float: z > 0 by 1e-30, a = b = 0, the frame's centre
        elif name == "z_negative":
            q = (-point(mid_x, mid_y)).astype(f32)                        # the mirror of the frame's centre: only `z > 0` rejects it
        elif name == "z_zero":
            start = (r * 0.75).astype(f32)
            cand = np.concatenate([start[None], _neighbours(start, [int(np.argmax(np.abs(f)))], 2000), np.zeros((1, 3), f32)])
            z = _g(p, cand, W, H)[0]
            q = cand[np.argmax(z == 0)]                                   # (the zero vector, the last candidate, always qualifies)
        else:
            axis, target = targets[name]
            g64 = [mid_x, mid_y]
            g64[axis] = target
            for _ in range(8):                                            # the float32 basis is not exactly orthonormal: close in on it
                start = point(*g64).astype(f32)
                g64[axis] -= float(_g(p, start[None], W, H)[1 + axis][0]) - target
            moving = r if axis == 0 else u
            axes = sorted({int(np.argmax(np.abs(moving))), int(np.argmax(np.abs(f)))})
            cand = _neighbours(start, axes, 300 if len(axes) == 1 else 40)
            z, gx, gy = _g(p, cand, W, H)
            g, other, size = (gx, gy, H) if axis == 0 else (gy, gx, W)
            with np.errstate(all="ignore"):
                ok = (z > 0) & (other >= 0) & (other < f32(size) * f32(32.0) - f32(1.0))
                lower = name.endswith(("lo_on", "lo_off"))
                limit = f32(-32.0) if lower else f32(W if axis == 0 else H) * f32(32.0)
                side = ok & ((g >= limit) if (lower == on) else (g < limit))
                assert side.any(), (name, wh, "no float32 neighbour on the intended side")
                dist = np.where(side, np.abs(g.astype(np.float64) - float(limit)), INF)
            q = cand[np.argmin(dist)]
            exact += int(_g(p, q[None], W, H)[1 + axis][0] == f32(target))
        out[k] = q
    # the confirmation: the intended side of the intended comparison, and every other comparison holds
    _, _, on_screen = _reprojection(p, out, W, H)
    z, gx, gy = _g(p, out, W, H)
    for k, (name, on) in enumerate(BOUNDS):
        assert bool(on_screen[k]) == on, (name, wh, float(z[k]), float(gx[k]), float(gy[k]))
        inside_x, inside_y = f32(-32.0) <= gx[k] < f32(W) * f32(32.0), f32(-32.0) <= gy[k] < f32(H) * f32(32.0)
        if name == "z_zero":
            assert z[k] == 0, (name, wh, float(z[k]))
        elif name == "z_negative":
            assert z[k] < 0 and inside_x and inside_y, (name, wh, float(z[k]), float(gx[k]), float(gy[k]))
        elif name == "z_tiny":
            assert 0 < z[k] < 1e-29 and inside_x and inside_y, (name, wh, float(z[k]))
        else:
            assert z[k] > 0 and (inside_y if name.startswith("gx") else inside_x), (name, wh)
    out.setflags(write=False)
    _CACHE[key] = (out, exact)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ the planes
def motion_planes(case, wh, salt=0):
    """(prev_points, prev_point_normals) float32[H, W, 4]: see the module text."""
    W, H = wh
    p = case["params"]
    pos, nrm = np.ascontiguousarray(case["pos"], f32), np.ascontiguousarray(case["nrm"], f32)
    pts, pnr = np.zeros((H, W, 4), f32), nrm.copy()
    with np.errstate(all="ignore"):
        for k in range(3):
            pts[..., k] = pos[..., k] + f32(p.eye_delta[k])
    pts[..., 3] = 1.0
    g, j = groups(wh, salt)
    comp = j % 3
    for k in range(3):                                                    # groups 1 and 4: one component replaced
        pick = (g == 1) & (comp == k)
        pts[..., k][pick] = Q_VALUES[(j[pick] // 3) % len(Q_VALUES)]
        pick = (g == 4) & (comp == k)
        pnr[..., k][pick] = M_VALUES[(j[pick] // 3) % len(M_VALUES)]
    pick = g == 2
    with np.errstate(all="ignore"):
        pts[pick, :3] = pts[pick, :3] + OFFSETS[j[pick] % len(OFFSETS)]
    pick = g == 3
    pts[pick, :3] = bounds_points(p, wh)[0][j[pick] % len(BOUNDS)]
    pick = g == 5
    pnr[pick, :3] = np.where((j[pick] % 2 == 0)[:, None], f32(0.0), f32(-0.0))
    pick = g == 6
    pts[..., 3][pick] = W_VALUES[j[pick] % len(W_VALUES)]
    pnr[..., 3][pick] = W_VALUES[(j[pick] + 3) % len(W_VALUES)]
    return np.ascontiguousarray(pts), np.ascontiguousarray(pnr)


def garbage_w(plane, salt=0):
    """A copy of a texel plane with every .w lane replaced by W_VALUES in turn."""
    out = np.array(plane, f32)
    H, W = out.shape[:2]
    out[..., 3] = W_VALUES[(np.arange(H * W).reshape(H, W) + salt) % len(W_VALUES)]
    return out


def selection(fi, k):
    """The parameters of run k of frame number fi: dict(max_length, reset, with_map, radius, margin, clamp_max_length, clamp_reset).
    j = (k + fi) % 12 walks all twelve (max_length, reset) pairs and all twelve (radius, margin) pairs (4 and 3 are coprime), so with
    twelve runs or more every value -- and every pair of those two tables -- occurs with every frame; the clamped run's max_length
    and reset are taken at 7 j + fi, another walk of the twelve, so that radius and max_length are not tied."""
    j, jc = (k + fi) % 12, (7 * (k + fi) + fi) % 12
    return dict(max_length=MAX_LENGTHS[j % 4], reset=RESETS[j % 3], with_map=(k // 4) % 2 == 0, radius=RADII[j % 4], margin=MARGINS[j % 3],
                clamp_max_length=MAX_LENGTHS[jc % 4], clamp_reset=RESETS[jc % 3])


# ------------------------------------------------------------------------------------------------------------ the census
def census():
    """dict group -> [pixels that blend, pixels that restart although the non-motion parent blends], asserted: see the module text."""
    wh = (40, 40)
    c = tc.geometric("pixels", wh)
    pts, pnr = motion_planes(c, wh)
    ones, sevens = np.full((40, 40), 0xFF, np.uint8), np.full((8, 40, 40), 7, np.uint8)
    prev = (c["prev_pos"], c["prev_nrm"], c["prev_vis"], sevens)
    motion = ms.accumulate_motion_rule(1, c["params"], c["nrm"], c["vis"], prev, ones, (pts, pnr))[1][0]
    parent = tc.accumulate_rule(1, c["params"], c["pos"], c["nrm"], c["vis"], prev, ones)[1][0]
    g, _ = groups(wh)
    out = {GROUPS[k]: [int(((g == k) & (motion > 1)).sum()), int(((g == k) & (motion == 1) & (parent > 1)).sum())] for k in (1, 2, 3, 4, 5, 6)}
    out["exact_bounds"] = bounds_points(c["params"], wh)[1]
    for name in ("q_replaced", "m_replaced"):
        assert out[name][0] >= 20 and out[name][1] >= 20, (name, out)
    assert out["shifted"][0] >= 20 and out["m_zero"][0] == 0, out
    assert out["m_zero"][1] >= 20, out                                    # (the zero groups restart where the parent blends)
    active = ~((c["nrm"][..., :3] == 0).all(-1))
    same = (motion == parent) | ~active
    assert same[(g == 0) | (g == 6) | (g == 7)].all(), "STATIC texels and garbage .w lanes must give the parent's lengths"
    return out


# ------------------------------------------------------------------------------------------------------------ small streams
def _refit_pair(old, new, faces):
    old32, new32 = np.ascontiguousarray(old, f32), np.ascontiguousarray(new, f32)
    idx, P = np.ascontiguousarray(faces.reshape(-1), np.uint32), faces.shape[0]
    built = api.BVHBuilder().build(new32, 3, idx, P).m_packedNodes
    cur, prev = api.bvh_refit(built, new32, 3, idx, P), api.bvh_refit(built, old32, 3, idx, P)
    for a in (cur, prev):
        a.setflags(write=False)
    return cur, prev


def small_streams(name):
    """dict(packed, prev_packed) of "one", "quad" or "cornell"."""
    if ("stream", name) not in _CACHE:
        if name == "cornell":
            s = ms.streams("cornell", "translate")
            _CACHE[("stream", name)] = dict(packed=s["packed"], prev_packed=s["prev_packed"])
        else:
            # a tilted triangle that covers the -z axis; "quad" adds its neighbour across the long edge, which stays where it was
            old = np.array([[-1, -1, -3], [1, -1, -2.5], [0, 1, -3.5], [1.5, 1.2, -3.0]], np.float64)
            faces = np.array([[0, 1, 2]] if name == "one" else [[0, 1, 2], [1, 3, 2]], np.uint32)
            new = old.copy()
            new[0] += [0.25, -0.125, 0.5]                                 # vertex 0 belongs to the first triangle alone
            if name == "one":
                old, new = old[:3], new[:3]
            cur, prev = _refit_pair(old, new, faces)
            _CACHE[("stream", name)] = dict(packed=cur, prev_packed=prev)
    return _CACHE[("stream", name)]


def cameras_of(name):
    """[(tag, eye, prev_eye, target, fovy)] of a small stream."""
    if name == "cornell":
        sc = ms._scene("cornell")
        box = sc["verts"][np.unique(sc["faces"][sc["part"]])] + ms.T
        inside = box.mean(0).astype(f32)                                  # the centre of the moved box
        return [("eye_inside_the_moved_box", inside, (inside + f32(0.05)).astype(f32), sc["target"], 1.4),
                ("all_miss", np.array([5.0, 30.0, 5.0], f32), np.array([5.0, 30.0, 5.5], f32), np.array([5.0, 60.0, 5.0], f32), 0.9)]
    origin = np.zeros(3, f32)
    return [("front", origin, np.array([0.05, -0.02, 0.1], f32), np.array([0, 0, -1], f32), 1.0),
            ("still", origin, origin, np.array([0, 0, -1], f32), 1.0),
            ("all_miss", origin, np.array([0.05, 0.0, 0.0], f32), np.array([0, 0, 1], f32), 1.0)]


def leaf_nodes(packed):
    """The node indices of the leaves of a stream of 5P - 2 vec4."""
    w = np.ascontiguousarray(packed, u32).reshape(-1)
    nodes = np.arange((w.size // 4 + 2) // 5 * 2 - 1)
    return nodes[w[nodes * 8 + 3] != END]


def nine_word_indices(packed, leaf):
    w = np.ascontiguousarray(packed, u32).reshape(-1)
    return [leaf * 8 + k for k in (0, 1, 2, 4, 5, 6)] + [int(w[leaf * 8 + 3]) * 4 + k for k in (0, 1, 2)]


def poison(packed, prev_packed, kind):
    """(poisoned copy of prev_packed, the leaves whose nine words were touched): see the module text."""
    w = np.array(prev_packed, u32).reshape(-1)
    cur = np.ascontiguousarray(packed, u32).reshape(-1)
    leaves = leaf_nodes(packed)
    values = np.array([NAN, INF, 1e-41], f32).view(u32)
    touched = []
    if kind == "leaf_words":
        for n, leaf in enumerate(leaves[::2]):
            words = nine_word_indices(packed, int(leaf))
            for k in (range(9) if n % 3 == 2 else [n % 9]):
                w[words[k]] = values[(n + k) % 3]
            touched.append(int(leaf))
    elif kind == "sign":
        for leaf in leaves:
            hit = False
            for i in nine_word_indices(packed, int(leaf)):
                if w[i] == 0:
                    w[i], hit = 0x80000000, True
            if hit:
                touched.append(int(leaf))
    elif kind == "never_read":
        nodes = np.arange((w.size // 4 + 2) // 5 * 2 - 1)
        for node in nodes[cur[nodes * 8 + 3] == END]:
            w[[node * 8 + k for k in (0, 1, 2, 4, 5, 6)]] = 0x7FC00001
        for leaf in leaves:
            w[int(cur[leaf * 8 + 3]) * 4 + 3] = 0x7FC00001
    else:
        raise ValueError(kind)
    out = w.reshape(-1, 4)
    out.setflags(write=False)
    return out, np.array(touched, np.int64)


def nan_aware_same(got, want, what):
    """Bit for bit wherever the expected float is not a NaN; where it is, a NaN of any payload (include/rts_scene.h: which NaN an
    operation returns is not defined for the motion G-buffer pass's MOVED texels)."""
    for g, w, name in zip(got, want, ("first", "second", "third", "fourth", "fifth")):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == f32:
            nan = w != w
            if nan.any():                                                 # (measured: shown with pytest -s)
                print(what, name, "NaN components:", int(nan.sum()), "of other bits:", int((nan & (g.view(u32) != w.view(u32))).sum()))
            assert ((g != g) == nan).all(), (what, name, "NaNs elsewhere", np.argwhere((g != g) != nan)[:6].tolist())
            g, w = np.where(nan, u32(0), g.view(u32)), np.where(nan, u32(0), w.view(u32))
        assert (g == w).all(), (what, name, int((g != w).sum()), np.argwhere(g != w)[:6].tolist())
