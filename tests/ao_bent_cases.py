"""Shared by the bent-normal tests (include/rts.h: rts_trace_ambient_occlusion_bent*; include/rts_scene.h: rtsh_ambient_occlusion_bent,
rtsh_combine_visibility_list_ao_bent): tests/ao_cases.py's frames, rays_rule, frame_rule and sample_index as they are,
and a numpy rule written from the header's text and from nothing of the library's --
  u_j from the ORACLE's any-hit over ao_cases.rays_rule's rays, Q with numpy.rint, the sums in int64, the frame from
  ao_cases.frame_rule, float32 operations in the written order.
The twin and the kernels are only ever compared with this rule (and through it with the oracle), never with each other alone.
The combine's numpy restatement lives here too."""
import numpy as np

import ao_cases as ac
import oracle
import scene_pass_cases as sp
from raytracedshadows_amd import api

f32, u32 = np.float32, np.uint32
GUARD = ac.GUARD
INVALID = ac.INVALID
GUARD_F32 = np.frombuffer(bytes([GUARD] * 4), f32)[0]


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def quantise_rule(v):
    """Q of the header: 0 for a NaN, else rint(clamp(v, -1, 1) * 16384) as an integer (numpy.rint: ties to even)."""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        c = np.minimum(np.maximum(v, f32(-1.0)), f32(1.0)).astype(f32)
        q = np.rint((c * f32(16384.0)).astype(f32))
    return np.where(np.isnan(v), 0, q).astype(np.int64)


def free_bytes(fr_packed, k, ao, positions, normals, active=None):
    """u[H, W, n]: the oracle's any-hit byte (1 = unoccluded) of every ray of the numpy rule; 0 for a pixel that sends none."""
    H, W = np.asarray(positions).shape[:2]
    n = max(1, int(ao.nsamples))
    rays = ac.rays_rule(k, ao, positions, normals, active)
    unoccluded, _, _ = oracle.trace_rays(fr_packed, rays)
    live = live_of(normals, active)
    return np.where(live[..., None], np.asarray(unoccluded).reshape(H, W, n), 0).astype(np.int64)


def live_of(normals, active=None):
    N = np.asarray(normals, f32)[..., :3]
    live = ~((N[..., 0] == 0) & (N[..., 1] == 0) & (N[..., 2] == 0))
    if active is not None:
        live &= np.asarray(active) != 0
    return live


def bent_from_sum(normals, S, c, live):
    """float32[H, W, 4]: the frame applied to the integer sum S[H, W, 3], (float)c in .w; (+0, +0, +0, +0) where not live."""
    N = np.ascontiguousarray(normals, f32)[..., :3]
    with np.errstate(all="ignore"):
        T, B = ac.frame_rule(N)
        f = S.astype(f32) * f32(2.0 ** -14)
        assert (f.astype(np.float64) * 16384.0 == S).all()              # both steps exact
        v = ((T * f[..., 0:1]) + (B * f[..., 1:2])) + (N * f[..., 2:3])
    assert v.dtype == f32
    out = np.zeros(N.shape[:2] + (4,), f32)
    out[..., :3] = np.where(live[..., None], v, f32(0.0))
    out[..., 3] = np.where(live, c.astype(f32), f32(0.0))
    return out


def bent_rule(fr_packed, k, ao, positions, normals, active=None):
    """(uint8[H, W] counts, float32[H, W, 4] bent, int64[H, W, 3] S) of the header."""
    pos = np.ascontiguousarray(positions, f32)
    H, W = pos.shape[:2]
    n = max(1, int(ao.nsamples))
    u = free_bytes(fr_packed, k, ao, positions, normals, active)
    q = quantise_rule(ao.dirs_array()[:, :3])                            # [64, 3]
    px = np.arange(H * W)
    S = np.zeros((H * W, 3), np.int64)
    for j in range(n):
        S += u.reshape(-1, n)[:, j:j + 1] * q[ac.sample_index(int(ao.table), j, px)]
    S = S.reshape(H, W, 3)
    c = u.sum(-1)
    live = live_of(normals, active)
    assert (np.abs(S) <= 48 * 16384).all()
    return np.where(live, c, 0).astype(np.uint8), bent_from_sum(normals, S, c, live), S


_WANT = {}


def want(fr, n, table, share, masked=False, dirs_key=None):
    """The rule's (counts, bent, S) on a frame of ao_cases, computed once per case and read-only."""
    key = (fr.name, fr.W, fr.H, n, table, share, masked, dirs_key)
    if key not in _WANT:
        ao = fr.ao(n, table, share, dirs=None if dirs_key is None else ac.below_horizon_dirs())
        w = bent_rule(fr.packed, fr.k, ao, fr.dirty if masked else fr.pos, fr.nrm, fr.active if masked else None)
        for a in w:
            a.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def same_bent(got, rule, what):
    bad = np.argwhere(bits(got) != bits(rule))
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:4].tolist(), [np.asarray(got)[tuple(b[:2])].tolist() for b in bad[:2]],
                               [np.asarray(rule)[tuple(b[:2])].tolist() for b in bad[:2]])


def guard_radius():
    """The first radius of ao_cases.RADII at which ("cornell_128", 48, 40) with n = 16 shows, by the ORACLE alone, at least 32 pixels
    with 0 < c < n and at least 32 with c == n -> (share, partly, full); the best one (most partly free pixels) if none does."""
    fr = ac.frame("cornell_128", 48, 40)
    best = None
    for share in ac.RADII:
        u = free_bytes(fr.packed, fr.k, fr.ao(16, 0, share), fr.pos, fr.nrm)
        c = u.sum(-1)[~fr.background]
        partly, full = int(((c > 0) & (c < 16)).sum()), int((c == 16).sum())
        if partly >= 32 and full >= 32:
            return share, partly, full
        if best is None or min(partly, full) > min(best[1], best[2]):
            best = (share, partly, full)
    return best


# ------------------------------------------------------------------------------------------------------------------ the bent combine
def sky_tint_rule(sky, bent):
    """float32[H, W, 3]: tint of the header from bent[H, W, 4], one rounded float32 operation per step."""
    b = np.ascontiguousarray(bent, f32)
    up, hi, lo = (np.array([v[i] for i in range(3)], f32) for v in (sky.up, sky.sky, sky.ground))
    with np.errstate(all="ignore"):
        bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
        l2 = ((bx * bx) + (by * by)) + (bz * bz)
        ln = np.sqrt(l2)
        dot = ((bx * up[0]) + (by * up[1])) + (bz * up[2])
        ok = (ln > 0) & np.isfinite(ln)
        u = np.where(ok, dot / np.where(ok, ln, f32(1.0)), f32(0.0)).astype(f32)
        h = f32(0.5) + f32(0.5) * u
        h = np.where(h > 0, np.where(h < 1, h, f32(1.0)), f32(0.0)).astype(f32)
        tint = np.stack([lo[c] + (hi[c] - lo[c]) * h for c in range(3)], -1)
    assert tint.dtype == f32
    return tint


def combine_ao_bent_rule(k, lst, positions, normals, visibility, ao_plane, bent, sky, lights_map=None, colors=None):
    """uint8[H, W, 3]: ao_cases.combine_ao_rule with channel c's ambient term (ambient * ao[p]) * tint_c."""
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
        ambient = (f32(0.15) + f32(0.05) * (f32(1.0) - ndv)) * np.ascontiguousarray(ao_plane, f32)
        tint = sky_tint_rule(sky, bent)
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
            term = (ambient * tint[..., ch]).astype(f32)
            scaled = (sums[ch] + term) * f32(255.0) + f32(0.5)
            inside = (scaled > 0) & (scaled < 255)
            byte = np.where(scaled >= 255, 255, np.where(inside, np.where(inside, scaled, 0).astype(np.int32), 0))
            out[..., ch] = np.where(background, 0, byte).astype(np.uint8)
        return out


def combine_case(W=33, H=18):
    """ao_cases.combine_case's frame (or the 48 x 40 one of the GPU test) with a random bent plane -- long, short, all-zero, NaN and
    infinite texels, garbage on the background -- and a sky whose up is a tilted unit vector."""
    import list_filter_cases as fc
    nrm, pos, planes, mask, lights_map, _ = fc.frame("geometric", (W, H))
    H, W = nrm.shape[:2]
    lst = api.LightList.make([(api.Light.POINT, (1.0, 3.0, 0.5)), (api.Light.DIRECTIONAL, (0.3, 0.8, 0.2))])
    k = api.RayTracingConstants.make((0.5, 2.0, 4.0), (0.3, 0.8, 0.2), W, H, camera_direction=(0.1, -0.5, -1.0))
    rs = np.random.RandomState(43)
    vis = rs.random_sample((2, H, W)).astype(f32)
    plane = (rs.random_sample((H, W)) * 1.5).astype(f32)
    plane[rs.random_sample((H, W)) < 0.05] = np.nan
    plane[rs.random_sample((H, W)) < 0.05] = -0.25
    bent = np.zeros((H, W, 4), f32)
    bent[..., :3] = rs.standard_normal((H, W, 3)) * 9.0
    bent[..., 3] = rs.randint(0, 17, (H, W))
    pick = rs.random_sample((H, W))
    bent[pick < 0.10, :3] = 0.0
    bent[(pick >= 0.10) & (pick < 0.13), 0] = np.nan
    bent[(pick >= 0.13) & (pick < 0.16), 1] = np.inf
    bent[(pick >= 0.16) & (pick < 0.19), :3] = 1e-30                    # l2 underflows to a denormal or 0
    bent[(pick >= 0.19) & (pick < 0.22), :3] = 3e19                     # l2 overflows: len = +Inf
    background = (nrm[..., :3] == 0).all(-1)
    plane[background] = np.nan
    bent[background] = np.nan
    colors = np.array([[1.0, 0.8, 0.6], [0.2, 0.4, 1.0]], f32)
    up = np.array([0.2, 0.9, -0.3], np.float64)
    sky = api.SkyAmbient.make(up=(up / np.linalg.norm(up)).astype(f32), sky=(0.4, 0.6, 1.0), ground=(0.5, 0.35, 0.2))
    return k, lst, pos, nrm, vis, plane, bent, sky, lights_map, colors
