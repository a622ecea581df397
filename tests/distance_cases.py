"""Shared by the occluder-distance tests: the expected value from the CPU oracle's any-hit alone, and the small scenes.

The distance of a ray (include/rts.h) is the smallest T >= +0 for which the reference's any-hit with tmax = min(T, the ray's tmax)
reports a hit, +Inf if the ray is lit at its own tmax.  occluded(T) is monotone in T (a triangle accepted at T is accepted at every
larger T up to the ray's tmax, and the leaves visited do not depend on T), so the value is found by bisection over the bit patterns
of the non-negative floats: 31 traces of `oracle.trace_rays`, whatever the rays."""
import os

import numpy as np

import oracle
import streams
from raytracedshadows_amd import api

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF_BITS = 0x7F800000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bisect_distance(packed, rays):
    """float32[n]: the definition, from oracle.trace_rays alone."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = rays.shape[0]
    out = np.full(n, INF_BITS, np.uint32)
    lit, _, _ = oracle.trace_rays(packed, rays)
    occ = np.flatnonzero(lit == 0)
    if occ.size == 0:
        return out.view(np.float32)
    tb = bits(rays[occ, 3]).astype(np.int64)
    negative = (tb >> 31) != 0                          # an occluded ray with a negative tmax (-0 included): only +-0 / NaN hits -> +0
    nan = ~negative & (tb > INF_BITS)
    hi = np.where(nan, INF_BITS, tb)
    hi[negative] = 0
    lo = np.zeros_like(hi)
    sub = rays[occ].copy()
    for _ in range(31):                                 # 2^31 > INF_BITS + 1 candidates
        mid = (lo + hi) >> 1
        sub[:, 3] = mid.astype(np.uint32).view(np.float32)
        hit = oracle.trace_rays(packed, sub)[0] == 0
        hit |= negative
        hi = np.where(hit, mid, hi)
        lo = np.where(hit, lo, np.minimum(mid + 1, hi))
    assert (lo == hi).all()
    out[occ] = hi.astype(np.uint32)
    return out.view(np.float32)


def constants_from(array):
    return api.RayTracingConstants.from_buffer_copy(np.ascontiguousarray(array, np.float32).tobytes())


def frame_rays(constants, light, positions):
    """The rays of a frame as the oracle sets them up (one per pixel, row-major)."""
    return oracle.gen_rays(constants.as_array(), oracle.light_from_product(light, constants), positions)


def golden_frame(name, W=None, H=None):
    """(packed, constants, point light, positions[H, W, 4]) of a golden scene, cut to its bottom-right W x H (in the cornell box
    the part both lights throw shadows into)."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    pos = g["positions"]
    H = pos.shape[0] if H is None else H
    W = pos.shape[1] if W is None else W
    return (np.ascontiguousarray(g["packed"]), constants_from(g["constants"]), api.Light.make(api.Light.POINT, g["light_point"]),
            np.ascontiguousarray(pos[pos.shape[0] - H:, pos.shape[1] - W:]))


def generic_rays(packed, n=4096, seed=11):
    """Seeded incoherent rays through the stream's vertices' box, tmax cycling over {1, 1e9, +Inf, 0, negative, NaN}."""
    t = streams.triangles_of(packed).reshape(-1, 3).astype(np.float64)
    t = t[np.isfinite(t).all(1)]
    lo, ext = t.min(0), np.maximum(t.max(0) - t.min(0), 1e-6)
    rs = np.random.RandomState(seed)
    r = np.zeros((n, 8), np.float32)
    a = lo + rs.random_sample((n, 3)) * ext
    b = lo + rs.random_sample((n, 3)) * ext
    r[:, 0:3] = a
    r[:, 4:7] = b - a                                   # t = 1 is the second point
    tmax = np.array([1.0, 1e9, np.inf, 0.0, -0.5, np.nan], np.float32)
    r[:, 3] = tmax[np.arange(n) % tmax.size]
    v0 = streams.triangles_of(packed)[:, 0]             # every sixth ray starts ON a vertex: t = +-0 exactly, inside tmax = 0 too
    r[3::6, 0:3] = v0[rs.randint(0, v0.shape[0], r[3::6].shape[0])]
    return r


def far_before_near():
    """(packed, rays, near t): two big triangles across the +z axis, the FAR one first in depth-first order -- the any-hit walk
    stops at it; the distance is the near one's t."""
    tris = np.array([[[-4, -4, 5], [8, -4, 5], [-4, 8, 5]],
                     [[-4, -4, 2], [8, -4, 2], [-4, 8, 2]]], np.float32)
    packed = streams.stream_from_tree((0, 1), tris)
    rays = np.zeros((64, 8), np.float32)
    rays[:, 0] = (np.arange(64) % 8) * 0.25
    rays[:, 1] = (np.arange(64) // 8) * 0.25
    rays[:, 3] = 1e9
    rays[:, 6] = 1.0
    return packed, rays, np.float32(2.0)


def far_before_near_frame(W=24, H=16):
    """The same stream under a directional light along +z: a frame whose every pixel looks up at both triangles."""
    packed, _, near = far_before_near()
    pos = np.zeros((H, W, 4), np.float32)
    pos[..., 0] = np.arange(W, dtype=np.float32)[None, :] * 0.0625
    pos[..., 1] = np.arange(H, dtype=np.float32)[:, None] * 0.0625
    pos[..., 3] = 1.0
    return packed, api.RayTracingConstants.make([0, 0, 0], [0, 0, 1], W, H), pos


def origin_and_degenerate():
    """(packed, rays): triangle 0 lies in the plane z = 0 through the ray origins (t = +-0), triangle 1 is a point (v0 = v1 = v2:
    det = 0, every quantity NaN, accepted by the reference's test -- contribution +0), triangle 2 is an ordinary one at z = 3."""
    tris = np.array([[[-1, -1, 0], [3, -1, 0], [-1, 3, 0]],
                     [[0.5, 0.5, 1], [0.5, 0.5, 1], [0.5, 0.5, 1]],
                     [[-1, -1, 3], [3, -1, 3], [-1, 3, 3]]], np.float32)
    rays = np.zeros((6, 8), np.float32)
    rays[:, 3] = 10.0
    rays[0, 0:3], rays[0, 4:7] = (0.25, 0.25, 0.0), (0, 0, 1)        # starts ON triangle 0: t = +0
    rays[1, 0:3], rays[1, 4:7] = (0.25, 0.25, 0.0), (0, 0, -1)       # ... looking away: t = -0, accepted (-0 < 0 is false)
    rays[2, 0:3], rays[2, 4:7] = (0.25, 0.25, 0.5), (0, 0, 1)        # above it: the NaN triangle counts as +0
    rays[3, 0:3], rays[3, 4:7] = (0.25, 0.25, -1.0), (0, 0, 1)       # below all three
    rays[4, 0:3], rays[4, 4:7] = (9.0, 9.0, 0.5), (0, 0, 1)          # beside the boxes ...
    rays[5, 0:3], rays[5, 4:7] = (2.5, 2.5, 0.5), (0, 0, 1)          # ... and inside them, past the hypotenuse of 0 and 2
    return streams.stream_from_tree(((0, 1), 2), tris), rays
