"""Shared by the ambient occlusion tests (include/rts.h: rts_trace_ambient_occlusion*; include/rts_scene.h: rtsh_ambient_occlusion,
rtsh_ao_rays, rtsh_combine_visibility_list_ao): a numpy float32 restatement of the frame, L and the ray, written from
the header's text and from nothing of the library's; the frames and the parameter cases.

Frames: the bottom-right 48 x 40 of cornell_128 and 40 x 36 of terrain_96 (tests/golden/), and 1 x 1, 17 x 5 and 61 x 37 of cornell_128
(32 texels in from that corner, which is background) for partial tiles.  The golden files hold positions only, so the normals are made here: the normalised cross product of the position
differences to the right and below, turned towards the camera; where that is not finite the pixel is background.  Four pixels carry
normals with N.z of +0, -0, exactly -1 and exactly +1; every background pixel's position is NaN, and so is every inactive one's in
`dirty` (neither may be read).  nsamples 1, 2, 3, 4, 5, 16, 48: waves of the four-wave form own no sample, one, or an uneven share.
table 0, n and 64.  Radii of 5 %, 50 % and 1000 % of the scene's diagonal.  A direction set with z < 0 entries.  An active map
that mixes whole zero tiles, single pixels and all-set tiles."""
import numpy as np

import list_filter_cases as fc
import scene_pass_cases as sp
from distance_cases import golden_frame
from raytracedshadows_amd import api

f32, u32 = np.float32, np.uint32
FRAMES = [("cornell_128", 48, 40), ("terrain_96", 40, 36), ("cornell_128", 1, 1), ("cornell_128", 17, 5), ("cornell_128", 61, 37)]
NSAMPLES = (1, 2, 3, 4, 5, 16, 48)
RADII = (0.05, 0.5, 10.0)                            # of the scene's diagonal
GUARD = 0xAB
INVALID = 1                                          # RTS_ERR_INVALID_ARG


def tables(n):
    """table 0, n and 64 -- a table needs at least two samples."""
    return (0,) if n < 2 else (0, n, 64)


def param_cases():
    """(nsamples, table, radius share): every sample count with every table it may have and every radius."""
    return [(n, t, r) for n in NSAMPLES for t in tables(n) for r in RADII]


# ----------------------------------------------------------------------------------------------------- the rule, from the header's text
def hash32(v):
    v = np.asarray(v, np.uint64)
    v ^= v >> np.uint64(16); v = (v * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15); v = (v * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(16)
    return v


def sample_index(table, j, pixels):
    """idx of sample j at the pixels (frame indices): j, or (start(p) + j) mod table with start(p) = (hash32(p) * table) >> 32."""
    if table == 0:
        return np.full(np.shape(pixels), j, np.int64)
    start = (hash32(pixels) * np.uint64(table)) >> np.uint64(32)
    return ((start + np.uint64(j)) % np.uint64(table)).astype(np.int64)


def _epsilon_for(x):
    u = np.ascontiguousarray(x, f32).view(u32)
    e = (u >> u32(23)) & u32(0xFF)
    e = e - np.minimum(u32(13), e)
    return ((u & ~u32(0xFF << 23)) | (e << u32(23))).view(f32)


def _gmax(x, y):
    return np.where(x < y, y, x).astype(f32)             # GLSL max


def frame_rule(N):
    """T, B of the header, N = float32[..., 3]."""
    nx, ny, nz = N[..., 0], N[..., 1], N[..., 2]
    with np.errstate(all="ignore"):
        sg = np.where(np.signbit(nz), f32(-1.0), f32(1.0)).astype(f32)
        a = f32(-1.0) / (sg + nz)
        b = (nx * ny) * a
        T = np.stack([f32(1.0) + (sg * (nx * nx)) * a, sg * b, -(sg * nx)], -1)
        B = np.stack([b, sg + (ny * ny) * a, -ny], -1)
    assert T.dtype == f32 and B.dtype == f32
    return T, B


def rays_rule(k, ao, positions, normals, active=None):
    """float32[H * W * n, 8]: what rtsh_ao_rays must write, every step one rounded float32 operation."""
    pos = np.ascontiguousarray(positions, f32)
    nrm = np.ascontiguousarray(normals, f32)
    H, W = pos.shape[:2]
    n = max(1, int(ao.nsamples))
    dirs = ao.dirs_array()
    radius = f32(ao.radius)
    cam = np.array([k.cameraPosition[i] for i in range(3)], f32)
    N = nrm[..., :3].reshape(-1, 3)
    rel = pos[..., :3].reshape(-1, 3)
    live = ~((N[:, 0] == 0) & (N[:, 1] == 0) & (N[:, 2] == 0))
    if active is not None:
        live &= np.asarray(active).reshape(-1) != 0
    out = np.zeros((H * W, n, 8), f32)
    px = np.nonzero(live)[0]
    N, rel = N[px], rel[px]
    with np.errstate(all="ignore"):
        T, B = frame_rule(N)
        o0 = cam[None, :] + rel
        absmax = lambda v: _gmax(_gmax(np.abs(v[:, 0]), np.abs(v[:, 1])), np.abs(v[:, 2]))
        bias = _gmax(_epsilon_for(absmax(o0)), _epsilon_for(absmax(rel)))
        for j in range(n):
            s = dirs[sample_index(int(ao.table), j, px)]
            d = ((T * s[:, 0:1]) + (B * s[:, 1:2])) + (N * s[:, 2:3])
            L = o0 + (radius * d)
            d0 = L - o0
            inv = f32(1.0) / np.sqrt((d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]) + d0[:, 2] * d0[:, 2])
            o = o0 + (d0 * inv[:, None]) * bias[:, None]
            assert o.dtype == f32 and L.dtype == f32
            out[px, j, 0:3] = o
            out[px, j, 3] = 1.0
            out[px, j, 4:7] = L - o
    return out.reshape(-1, 8)


def aim_rule(k, ao, positions, normals, y, x, j):
    """float32[3]: the header's L of sample j at pixel (x, y) -- the position of the hard point light whose shadow ray the sample is."""
    W = positions.shape[1]
    cam = np.array([k.cameraPosition[i] for i in range(3)], f32)
    N = np.ascontiguousarray(normals[y, x, :3], f32)[None]
    T, B = frame_rule(N)
    s = ao.dirs_array()[sample_index(int(ao.table), j, np.array([y * W + x]))][0]
    d = ((T[0] * s[0]) + (B[0] * s[1])) + (N[0] * s[2])
    L = (cam + np.ascontiguousarray(positions[y, x, :3], f32)) + (f32(ao.radius) * d)
    assert L.dtype == f32
    return L


# ---------------------------------------------------------------------------------------------------------------------------- the frames
_FRAMES = {}


def empty_texels(q):
    """A frame's background: a zero texel (or one that is not finite)."""
    return (q == 0).all(-1) | ~np.isfinite(q).all(-1)


def geometric_normals(positions):
    """float64[H, W, 3] of positions[H, W, 3 or 4]: the normalised cross product of the position differences to the right and below,
    turned towards the camera; all-zero (background) where that is not finite, where one of the three texels is background, and in
    the last row and column."""
    p3 = np.asarray(positions)[..., :3].astype(np.float64)
    cross = np.cross(p3[:-1, 1:] - p3[:-1, :-1], p3[1:, :-1] - p3[:-1, :-1])
    with np.errstate(all="ignore"):
        N = cross / np.linalg.norm(cross, axis=-1, keepdims=True)
    N = np.where((np.einsum("ijk,ijk->ij", N, p3[:-1, :-1]) > 0)[..., None], -N, N)      # towards the camera
    bad = ~np.isfinite(N).all(-1) | empty_texels(p3[:-1, :-1]) | empty_texels(p3[:-1, 1:]) | empty_texels(p3[1:, :-1])
    N[bad] = 0
    return np.pad(N, ((0, 1), (0, 1), (0, 0)))                           # (the last row and column: background)


class AoFrame:
    """A golden crop (read-only arrays): positions (background NaN), normals, the mixed active map, `dirty` (inactive NaN too)."""

    def __init__(self, name, W, H, inset=0):
        self.name, self.W, self.H = name, W, H
        self.packed, self.k, _, pos = golden_frame(name)                 # (the whole frame: the differences need a texel more)
        pos = np.ascontiguousarray(pos, f32)
        p3 = pos[..., :3].astype(np.float64)
        N = geometric_normals(pos)
        y1, x1 = pos.shape[0] - inset, pos.shape[1] - inset
        sl = (slice(y1 - H, y1), slice(x1 - W, x1))
        nrm = np.zeros((H, W, 4), f32)
        nrm[..., :3] = N[sl]
        pos = pos[sl].copy()
        y, x = np.mgrid[0:H, 0:W]
        if W * H > 1:
            nrm[(x * 5 + y * 11) % 37 == 9] = 0                          # some background inside every frame
        special = [(0.6, 0.8, 0.0), (0.6, 0.8, -0.0), (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)]
        self.special = []
        ys, xs = np.nonzero((nrm[..., :3] != 0).any(-1))
        if ys.size >= 16:
            for i, v in enumerate(special):                              # on pixels that have a surface
                at = (int(ys[(2 * i + 1) * ys.size // 8]), int(xs[(2 * i + 1) * ys.size // 8]))
                nrm[at][:3] = v
                self.special.append(at)
        self.background = (nrm[..., :3] == 0).all(-1)
        pos[self.background] = np.nan                                    # (a background position is never read)
        tile = (y >> 3) * ((W + 7) // 8) + (x >> 3)
        self.active = np.where(tile % 3 == 0, 0, np.where(tile % 3 == 1, 1, (x + 3 * y) % 5 == 0)).astype(np.uint8)
        if W * H == 1:
            self.active[:] = 1
        self.dirty = pos.copy()
        self.dirty[self.active == 0] = np.nan                            # (nor an inactive one)
        seen = p3[~empty_texels(p3)]
        self.diagonal = float(np.linalg.norm(seen.max(0) - seen.min(0)))  # of the scene as the whole golden frame sees it
        assert self.diagonal > 0 and (~self.background).any()
        self.pos, self.nrm = pos, nrm
        for a in (self.pos, self.nrm, self.active, self.dirty, self.background):
            a.setflags(write=False)
        self._want = {}

    def ao(self, n, table, share, dirs=None, seed=3):
        return api.AoParams.make(n, self.diagonal * share, table=table, seed=seed, dirs=dirs)

    def want(self, n, table, share, masked=False, dirs_key=None):
        """The twin's counts (computed once per case, read-only)."""
        key = (n, table, share, masked, dirs_key)
        if key not in self._want:
            ao = self.ao(n, table, share, dirs=None if dirs_key is None else below_horizon_dirs())
            w = api.ambient_occlusion(self.packed, self.k, ao, self.dirty if masked else self.pos, self.nrm, self.W, self.H,
                                      active=self.active if masked else None)
            w.setflags(write=False)
            self._want[key] = w
        return self._want[key]


def frame(name, W, H):
    """The two crops of the sparse list tests sit in the frame's bottom-right corner; the three small frames 32 texels further in,
    where the corner's background does not reach."""
    if (name, W, H) not in _FRAMES:
        _FRAMES[(name, W, H)] = AoFrame(name, W, H, 0 if (name, W, H) in FRAMES[:2] else 32)
    return _FRAMES[(name, W, H)]


def below_horizon_dirs():
    """64 directions, every third one with z < 0, some of length 0 and some long: any float is legal."""
    rs = np.random.RandomState(17)
    d = rs.standard_normal((64, 3)).astype(f32)
    d[::3, 2] = -np.abs(d[::3, 2])
    d[5] = 0
    d[9] *= f32(7.0)
    return d


def ground_quad():
    """(packed, constants, positions, normals): a 12 x 9 frame looking down at one large quad in the plane y = 0 -- every segment that
    leaves the surface upwards is unoccluded, whatever the table."""
    from raytracedshadows_amd.api import BVHBuilder
    s = f32(1000.0)
    verts = np.array([[-s, 0, -s, 0, 1, 0, 0, 0], [s, 0, -s, 0, 1, 0, 0, 0], [s, 0, s, 0, 1, 0, 0, 0], [-s, 0, s, 0, 1, 0, 0, 0]], f32)
    idx = np.array([0, 1, 2, 0, 2, 3], u32)
    packed = BVHBuilder().build(verts, 8, idx, 2).m_packedNodes
    W, H = 12, 9
    k = api.RayTracingConstants.make((0.0, 5.0, 0.0), (0.0, -1.0, 0.0), W, H)
    y, x = np.mgrid[0:H, 0:W]
    pos = np.zeros((H, W, 4), f32)
    pos[..., 0] = (x - W / 2) * 0.5
    pos[..., 1] = -5.0                                                   # camera-relative: the plane y = 0
    pos[..., 2] = (y - H / 2) * 0.5
    nrm = np.zeros((H, W, 4), f32)
    nrm[..., 1] = 1.0
    nrm[2, 3] = 0
    return np.ascontiguousarray(packed), k, pos, nrm


# ------------------------------------------------------------------------------------------------------------------- the AO combine
def combine_ao_rule(k, lst, positions, normals, visibility, ao_plane, lights_map=None, colors=None):
    """uint8[H, W, 3]: list_filter_cases.visibility_combine_rule with ambient' = ambient * ao[p], one rounded multiply."""
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
        assert ambient.dtype == f32
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
            scaled = (sums[ch] + ambient) * f32(255.0) + f32(0.5)
            inside = (scaled > 0) & (scaled < 255)
            byte = np.where(scaled >= 255, 255, np.where(inside, np.where(inside, scaled, 0).astype(np.int32), 0))
            out[..., ch] = np.where(background, 0, byte).astype(np.uint8)
        return out


def combine_case():
    """A geometric frame of the filter tests with a two-light list, random visibility and a random AO plane with NaN, values above 1,
    negative ones and NaN on the background."""
    nrm, pos, planes, mask, lights_map, _ = fc.frame("geometric", (33, 18))
    H, W = nrm.shape[:2]
    lst = api.LightList.make([(api.Light.POINT, (1.0, 3.0, 0.5)), (api.Light.DIRECTIONAL, (0.3, 0.8, 0.2))])
    k = api.RayTracingConstants.make((0.5, 2.0, 4.0), (0.3, 0.8, 0.2), W, H, camera_direction=(0.1, -0.5, -1.0))
    rs = np.random.RandomState(41)
    vis = rs.random_sample((2, H, W)).astype(f32)
    plane = (rs.random_sample((H, W)) * 1.5).astype(f32)
    plane[rs.random_sample((H, W)) < 0.05] = np.nan
    plane[rs.random_sample((H, W)) < 0.05] = -0.25
    plane[rs.random_sample((H, W)) < 0.03] = 40.0
    plane[(nrm[..., :3] == 0).all(-1)] = np.nan
    colors = np.array([[1.0, 0.8, 0.6], [0.2, 0.4, 1.0]], f32)
    return k, lst, pos, nrm, vis, plane, lights_map, colors
