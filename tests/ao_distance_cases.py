"""Shared by the AO distance tests (include/rts.h: rts_trace_ambient_occlusion_distance*; include/rts_scene.h:
rtsh_ambient_occlusion_distance): tests/ao_cases.py's frames, rays_rule and sample_index as they are, and a numpy rule
written from the header's text --
  d_j from api.rays_distance (rtsh_rays_distance, which tests/test_distance_host.py pins to the oracle) over ao_cases.rays_rule's rays;
  the minimum over uint32 views, the bins with float32 products truncated, weights, A and the quotient in numpy integers.
On every frame the rule also checks (d_j == +Inf) against the ORACLE's any-hit byte of the same ray.  The twin and the kernels are only
ever compared with this rule, never with each other alone."""
import numpy as np

import ao_cases as ac
import oracle
from raytracedshadows_amd import api

f32, u32 = np.float32, np.uint32
GUARD = ac.GUARD
INVALID = ac.INVALID
INF_BITS = 0x7F800000
RADII = (0.05, 0.10, 0.20, 0.50)                      # the guard's ladder, of the scene's diagonal
NS = (1, 3, 4, 5, 16, 48)
SHARES = {1: 0.05, 3: 0.5, 4: 0.5, 5: 10.0, 16: 0.5, 48: 0.05}


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def non_monotone():
    """A falloff that is no falloff: any bytes are legal."""
    return api.AoFalloff.make(((np.arange(64) * 37 + 11) % 256).astype(np.uint8))


FALLOFFS = {"zeros": api.AoFalloff.zeros, "full": lambda: api.AoFalloff.make(np.full(64, 255, np.uint8)), "linear": api.AoFalloff.linear,
            "saw": non_monotone}


def falloff(name):
    return FALLOFFS[name]()


def live_of(normals, active=None):
    N = np.asarray(normals, f32)[..., :3]
    live = ~((N[..., 0] == 0) & (N[..., 1] == 0) & (N[..., 2] == 0))
    if active is not None:
        live &= np.asarray(active) != 0
    return live


def bin_rule(d_bits):
    """b of the header for blocked samples' distances (uint32 bit patterns below +Inf): min(63, (uint32)(min(d, 1.0f) * 64.0f))."""
    d = np.ascontiguousarray(d_bits, u32).view(f32)
    with np.errstate(all="ignore"):
        c = np.where(d < f32(1.0), d, f32(1.0)).astype(f32)
        prod = (c * f32(64.0)).astype(f32)
        assert (prod.astype(np.float64) == c.astype(np.float64) * 64.0).all()   # the product is exact
    return np.minimum(63, np.trunc(prod).astype(np.int64))


def sample_distances(fr_packed, k, ao, positions, normals, active=None):
    """uint32[H, W, n]: the bit pattern of d_j of every ray of the numpy rule (+Inf for a pixel that sends none), checked against the
    oracle's any-hit byte of the same ray."""
    H, W = np.asarray(positions).shape[:2]
    n = max(1, int(ao.nsamples))
    rays = ac.rays_rule(k, ao, positions, normals, active)
    live = live_of(normals, active)
    d = bits(api.rays_distance(fr_packed, rays)).reshape(H, W, n)
    assert (d[live] <= INF_BITS).all()                                    # every d_j is a bit pattern >= +0, +Inf at most
    unoccluded, _, _ = oracle.trace_rays(fr_packed, rays)
    free = np.asarray(unoccluded).reshape(H, W, n) != 0
    assert np.array_equal((d == INF_BITS)[live], free[live]), "(d_j == +Inf) is not the oracle's any-hit byte"
    return np.where(live[..., None], d, u32(INF_BITS))


def rule_from_distances(d, n, weights, live):
    """(uint8 counts, float32 distance, uint16 obscurance, int64 A) of the header from d = uint32[H, W, n]."""
    free = d == INF_BITS
    c = free.sum(-1).astype(np.int64)
    best = d.min(-1).astype(u32)
    w = np.asarray(weights, np.int64)
    a = np.where(free, 255, w[bin_rule(np.where(free, u32(0), d))])
    A = a.sum(-1).astype(np.int64)
    S = 65535 // n
    assert (A <= 48 * 255).all() and (2 * A * S + 255 < 2 ** 26).all()
    obs = (2 * A * S + 255) // 510
    assert (obs <= n * S).all()
    counts = np.where(live, c, 0).astype(np.uint8)
    distance = np.where(live, best, u32(0)).astype(u32).view(f32)
    return counts, distance, np.where(live, obs, 0).astype(np.uint16), A


def distance_rule(fr_packed, k, ao, fall, positions, normals, active=None):
    """(counts, distance, obscurance, d) of the header; d = the per-sample bit patterns, uint32[H, W, n]."""
    n = max(1, int(ao.nsamples))
    d = sample_distances(fr_packed, k, ao, positions, normals, active)
    live = live_of(normals, active)
    counts, distance, obs, _ = rule_from_distances(d, n, fall.weights(), live)
    return counts, distance, obs, d


_D = {}


def distances(fr, n, table, share, masked=False, dirs_key=None):
    """The rule's per-sample bit patterns on a frame of ao_cases, computed once per case and read-only."""
    key = (fr.name, fr.W, fr.H, n, table, share, masked, dirs_key)
    if key not in _D:
        ao = fr.ao(n, table, share, dirs=None if dirs_key is None else ac.below_horizon_dirs())
        d = sample_distances(fr.packed, fr.k, ao, fr.dirty if masked else fr.pos, fr.nrm, fr.active if masked else None)
        d.setflags(write=False)
        _D[key] = d
    return _D[key]


def want(fr, n, table, share, fall_name, masked=False, dirs_key=None):
    """The rule's (counts, distance, obscurance) on a frame of ao_cases for a named falloff; the walks are shared among the falloffs."""
    d = distances(fr, n, table, share, masked, dirs_key)
    live = live_of(fr.nrm, fr.active if masked else None)
    return rule_from_distances(d, n, falloff(fall_name).weights(), live)[:3]


def same_planes(got, rule, what):
    """(counts, distance, obscurance) against the rule's, distance as uint32 views; a None plane is skipped."""
    for name, g, w in zip(("counts", "distance", "obscurance"), got, rule):
        if g is None:
            continue
        g, w = (bits(g), bits(w)) if name == "distance" else (np.asarray(g), np.asarray(w))
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, name, bad.shape[0], bad[:4].tolist(), [int(g[tuple(b)]) for b in bad[:4]],
                                   [int(w[tuple(b)]) for b in bad[:4]])


def guard_radius():
    """The first radius of the ladder 5, 10, 20, 50 % of the diagonal at which ("cornell_128", 48, 40) with n = 16 shows, by the rule
    alone, blocked samples in at least 8 different bins and at least 32 pixels with 0 < c < n -> (share, bins, partly); the last rung's
    figures if none does."""
    fr = ac.frame("cornell_128", 48, 40)
    found = None
    for share in RADII:
        d = distances(fr, 16, 0, share)
        live = ~fr.background
        blocked = d[live][d[live] != INF_BITS]
        nbins = int(np.unique(bin_rule(blocked)).size) if blocked.size else 0
        c = (d[live] == INF_BITS).sum(-1)
        partly = int(((c > 0) & (c < 16)).sum())
        found = (share, nbins, partly)
        if nbins >= 8 and partly >= 32:
            break
    return found


def zero_distance_case():
    """(packed, constants, positions, normals, at_origin): a 9 x 8 frame over one large quad in the plane y = 0, the camera AT the
    world's origin.  Where the position is (0, 0, 0) the surface point is the origin itself: the bias of the ray set-up is 0, the ray
    starts in the quad's plane and the triangle test accepts t = +-0 -- d_j is exactly +0 for every direction.  (The quad is off centre,
    so that the origin lies inside one triangle and not on the diagonal.)  Everywhere else the bias lifts the origin off the plane and
    every upward segment is free."""
    from raytracedshadows_amd.api import BVHBuilder
    s = f32(1000.0)
    verts = np.array([[-s, 0, -s, 0, 1, 0, 0, 0], [3 * s, 0, -s, 0, 1, 0, 0, 0], [3 * s, 0, s, 0, 1, 0, 0, 0], [-s, 0, s, 0, 1, 0, 0, 0]], f32)
    idx = np.array([0, 1, 2, 0, 2, 3], u32)
    packed = BVHBuilder().build(verts, 8, idx, 2).m_packedNodes
    W, H = 9, 8
    k = api.RayTracingConstants.make((0.0, 0.0, 0.0), (0.0, -1.0, 0.0), W, H)
    y, x = np.mgrid[0:H, 0:W]
    at_origin = (x + 2 * y) % 3 == 0
    pos = np.zeros((H, W, 4), f32)
    pos[..., 0] = np.where(at_origin, 0.0, (x + 1) * 0.5)
    pos[..., 2] = np.where(at_origin, 0.0, (y + 1) * 0.25)
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., 1] = 1.0
    nrm[2, 3] = 0
    at_origin = at_origin & (nrm[..., 1] != 0)
    return np.ascontiguousarray(packed), k, pos, nrm, at_origin
