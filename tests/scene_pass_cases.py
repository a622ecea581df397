"""Shared by the scene-pass tests (tests/test_scene_passes_host.py, tests/test_gpu_scene_passes.py): awkward inputs for the four passes
of raytracedshadows_amd/csrc/rts_primary.hip -- the G-buffer pass, the combine pass, the facing mark and the light map -- and the
expected values from the oracle and from float32 numpy restatements of the per-pixel rules.  No GPU code is touched here.

G-buffer cases are (name, packed stream, eye, target, fovy, W, H, expect); `expect` names the edge the case is meant to reach, which
the host tests assert on the ORACLE's output alone (so a case that degenerates fails loudly):
    "mixed"     0 < hits < W*H
    "hit"       at least one hit texel
    "tiny"      a texel with w == 1 and an all-zero normal (the normal's squared length underflows)
    "axis"      a hit whose position has two exact zeros (the direction is axis-parallel: 1/d is infinite, the slab product 0 * Inf)
    None        nothing beyond equality (a camera that may see nothing at all)

Texel tables are explicit (normals, positions, mask) frames: every pixel takes one entry of NORMALS, POSITIONS and MASKS, the three
lists cycling with pairwise coprime lengths (29, 8, 5) from a start that differs per frame, so that the 3 x 333 frame holds 999 of
the 1160 combinations.  Everything is compared bit for bit; floats through a uint32 view."""
import numpy as np

import oracle
import streams
from raytracedshadows_amd import api

f32 = np.float32
NAN, INF = np.nan, np.inf


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- streams
def _built(tris):
    tris = np.ascontiguousarray(tris, f32).reshape(-1, 3, 3)
    verts = np.zeros((tris.shape[0] * 3, 8), f32)
    verts[:, :3] = tris.reshape(-1, 3)
    return api.BVHBuilder().build(verts, 8, np.arange(tris.shape[0] * 3, dtype=np.uint32), tris.shape[0]).m_packedNodes


#: the triangle of the camera cases: tilted, so that it is seen from the front, from above and from below; it covers x = y = 0
TRI = np.array([[[-1, -1, -3], [1, -1, -2.5], [0, 1, -3.5]]], f32)
#: a triangle in the plane z = -3 (power-of-two edges: every product of the ray-triangle test is exact)
FLAT = np.array([[[-1, -1, -3], [1, -1, -3], [-1, 1, -3]]], f32)


def one_triangle(tris=TRI):
    return streams.stream_from_tree(0, tris)


def soup(n=80, seed=3):
    """(n, 3, 3): small triangles in the box [-1, 1]^2 x [-4, -2] -- the box the camera cases look at."""
    rs = np.random.RandomState(seed)
    c = rs.random_sample((n, 1, 3)) * 2 - 1 + np.array([0, 0, -3.0])
    return (c + (rs.random_sample((n, 3, 3)) - 0.5) * 0.7).astype(f32)


def chain(P=300):
    """A left-deep chain: (((0, 1), 2), ...), P leaves, a strip of small triangles along x."""
    tris = np.zeros((P, 3, 3), f32)
    x = (np.arange(P, dtype=np.float64) / P * 4 - 2)
    tris[:, 0] = np.stack([x, -0.5 + 0.3 * np.sin(x * 9), -3 + 0.2 * np.cos(x * 5)], 1)
    tris[:, 1] = tris[:, 0] + np.array([0.05, 0, 0], f32)
    tris[:, 2] = tris[:, 0] + np.array([0, 0.9, 0.1], f32)
    tree = 0
    for i in range(1, P):
        tree = (tree, i)
    return streams.stream_from_tree(tree, tris)


def degenerate():
    """streams.degenerate_triangles() plus one triangle around the origin with edges of 3e-13 and 5e-13: its determinant (1.5e-25 |d|)
    is an ordinary number, so it is hit, but its normal's squared length (2.25e-50) underflows to 0 -- the position is written with
    w = 1 and the normal as zeros.  (The 1e-41 triangles of degenerate_triangles are never hit: their determinant underflows.)  The
    origin lies inside the triangle, not on its corner: a ray down the z axis from an eye ON a face plane of the leaf's box has the
    slab bounds Inf and 0 * Inf = NaN, the compare-select then takes Inf for the near bound, and the culled walk -- the oracle's and
    the product's alike -- skips a triangle that brute force hits."""
    tri, _ = streams.degenerate_triangles()
    tiny = np.zeros((1, 3, 3), f32)
    tiny[0, :, :2] = -1e-13
    tiny[0, 1, 0] += 3e-13
    tiny[0, 2, 1] += 5e-13
    return _built(np.concatenate([tri, tiny]))


def nan_vertex():
    """Three triangles, the middle one with a NaN vertex; the boxes are the min / max unions written by stream_from_tree, so the
    NaN reaches the boxes above it (a NaN slab is ignored: the box is entered)."""
    tris = np.array([[[-1, -1, -3], [1, -1, -3], [-1, 1, -3]],
                     [[NAN, 0, -2.5], [1, 1, -2.5], [0, 1, -2.5]],
                     [[0.2, 0.2, -4], [1, 0.2, -4], [0.2, 1, -4]]], f32)
    return streams.stream_from_tree(((0, 1), 2), tris)


def tie_pairs():
    """name -> stream.  A and B lie in z = -3 with power-of-two edges, so t is exact and every texel both cover is a tie in t; B is
    wound the other way, so its normal, turned towards the viewer, is (-0, -0, 1) where A's is (+0, +0, 1): the leaf the strict `<`
    keeps shows in the sign bits.  `coincident`: the same three vertices; `coplanar`: B is twice A's size."""
    A = np.array([[-1, -1, -3], [1, -1, -3], [-1, 1, -3]], f32)
    same = A[[0, 2, 1]]
    big = np.array([[-1, -1, -3], [-1, 3, -3], [3, -1, -3]], f32)
    out = {}
    for name, B in (("coincident", same), ("coplanar", big)):
        out[name + "_ab"] = streams.stream_from_tree((0, 1), np.stack([A, B]))
        out[name + "_ba"] = streams.stream_from_tree((0, 1), np.stack([B, A]))
    return out


# ---------------------------------------------------------------------------------------------------------- G-buffer cases
FRONT = ((0, 0, 0), (0, 0, -1))                        # looking down -z from the origin


def _camera_cases(tag, packed, is_tri):
    e, t = FRONT
    hit = "hit" if is_tri else None
    return [
        (tag + "_1x1_minus_z", packed, e, t, 1.0, 1, 1, "axis" if is_tri else None),
        (tag + "_odd_7x5", packed, e, t, 1.0, 7, 5, "mixed" if is_tri else None),          # centre column and row: exact zeros
        (tag + "_eye_is_target", packed, e, e, 1.0, 9, 9, "mixed" if is_tri else None),    # forward falls back to -z
        (tag + "_straight_down", packed, (0, 3, -3), (0, -5, -3), 1.0, 12, 10, hit),       # `right` falls back to +x
        (tag + "_straight_up", packed, (0, -5, -3), (0, 5, -3), 1.0, 10, 12, hit),
        (tag + "_fovy_1e-4", packed, e, t, 1e-4, 9, 9, hit),
        (tag + "_fovy_3.1415", packed, e, t, 3.1415, 16, 16, None),
        (tag + "_eye_in_root_box", packed, (0.0, -0.5, -2.8), (0, -0.5, -4), 1.0, 16, 16, None),
        (tag + "_eye_far", packed, (0, 0, 3e6), (0, 0, -3), 2e-6, 15, 15, "mixed" if is_tri else None),
    ]


_GBUFFER = []


def gbuffer_cases():
    """The list of cases, built once."""
    if _GBUFFER:
        return _GBUFFER
    e, t = FRONT
    tri, sp = one_triangle(), _built(soup())
    two = streams.stream_from_tree((0, 1), np.concatenate([TRI, FLAT - np.array([0, 0, 1], f32)]))
    good, bad = streams.orphan_streams()
    deg = degenerate()
    c = _GBUFFER
    c += [("one_triangle", tri, e, t, 1.0, 16, 16, "mixed"),
          ("two_triangles", two, e, t, 1.0, 24, 16, "mixed"),
          ("orphans_good", good, (4.5, 4.5, -6), (4.5, 4.5, 0), 1.2, 33, 31, "mixed"),
          ("orphans_bad", bad, (4.5, 4.5, -6), (4.5, 4.5, 0), 1.2, 33, 31, "mixed"),
          ("deep_bushy_6", streams.deep_bushy_stream(6), (0.5, 0.5, -1.5), (0.5, 0.5, 1), 0.8, 64, 64, "mixed"),
          ("chain_300", chain(), e, t, 1.4, 64, 40, "mixed"),
          ("degenerate_view", deg, (5, 5, -9), (5, 5, 5), 1.0, 48, 40, "mixed"),
          ("degenerate_tiny", deg, (0, 0, 1), (0, 0, 0), 1.0, 9, 9, "tiny"),
          ("infinite_root", streams.infinite_root(sp), e, t, 1.0, 40, 40, "mixed"),
          ("swapped_boxes", streams.swapped_boxes(sp), e, t, 1.0, 40, 40, "mixed"),
          ("nan_vertex", nan_vertex(), e, t, 1.0, 32, 32, "mixed")]
    for name, packed in tie_pairs().items():
        c.append(("tie_" + name, packed, e, t, 1.0, 32, 24, "hit"))
    c += _camera_cases("tri", tri, True)
    # the eye exactly in the triangle's plane: t is +-0 or the determinant is 0, and `t > 0` is strict
    c += [("flat_eye_on_plane", one_triangle(FLAT), (0.25, -0.25, -3), (0, 0, -4), 1.0, 16, 16, None),
          ("flat_eye_on_plane_along", one_triangle(FLAT), (-3, 0, -3), (0, 0, -3), 1.0, 16, 16, None)]
    c += _camera_cases("soup", sp, False)
    for W, H in ((1, 1), (7, 9), (8, 8), (9, 7), (65, 3), (1, 200)):
        c.append((f"soup_{W}x{H}", sp, e, t, 1.0, W, H, "mixed" if W * H > 1 else None))
    assert len({x[0] for x in c}) == len(c)
    return c


def gbuffer_names():
    return [x[0] for x in gbuffer_cases()]


def gbuffer_case(name):
    return next(x for x in gbuffer_cases() if x[0] == name)


def prim_count(packed):
    return (np.asarray(packed).reshape(-1, 4).shape[0] + 2) // 5


_ORACLE_GB = {}


def oracle_gbuffer(name):
    """(positions, normals, hits) of a case from the oracle: computed once, shared, never written to."""
    if name not in _ORACLE_GB:
        _, packed, eye, target, fovy, W, H, _ = gbuffer_case(name)
        pos, nrm, hits = oracle.primary_gbuffer(packed, eye, target, fovy, W, H)
        pos.setflags(write=False)
        nrm.setflags(write=False)
        _ORACLE_GB[name] = (pos, nrm, hits)
    return _ORACLE_GB[name]


#: the tall frame: the tallest the two-dimensional grid of the device pass takes (8 rows per block, 65535 blocks), and one row more
TALL_H = 8 * 65535


def tall_case():
    return ("tall_1x524280", one_triangle(), FRONT[0], FRONT[1], 1.0, 1, TALL_H, "mixed")


# ------------------------------------------------------------------------------------------------------------ texel tables
NORMALS = np.array([
    (0, 1, 0), (0, -1, 0), (0.6, 0.8, 0), (-0.48, 0.6, 0.64), (0, 0, 1), (0.57735026, 0.57735026, 0.57735026),    # unit
    (0, 0, 0), (-0.0, 0, -0.0), (-0.0, -0.0, -0.0),                                                                # background
    (0, 1e-41, 0), (1e-41, 0, 0), (0, 0, -1e-41),                                                                  # denormal: not background
    (NAN, 0, 0), (0, NAN, 0), (0, 0, NAN), (NAN, 1, 0),
    (INF, 0, 0), (0, INF, 0), (0, -INF, 0), (0, 0, INF), (-INF, 1, 0),
    (0, 1e5, 0), (0, 1e7, 0), (0, 1e8, 0), (0, 1e30, 0), (0, 3e38, 0), (0, -1e30, 0), (1e30, 1e30, 0), (3e38, 3e38, 3e38),
], f32)
CAMERA = (1.0, 2.0, 3.0)
POINT = (1.0, 5.0, 3.0)
POSITIONS = np.array([
    (0, 0, 0), (0.5, -1, 2), (-3, 0.25, -7),
    (NAN, 0, 0), (INF, 0, 0), (0, -INF, 0),
    (0, 3, 0),                                           # CAMERA + this == POINT exactly: the length is 0 and L stays unnormalised
    (1e30, 1e30, -1e30),
], f32)
MASKS = np.array([0, 1, 16, 64, 255], np.uint8)
assert (np.asarray(CAMERA, f32) + POSITIONS[6] == np.asarray(POINT, f32)).all()

#: (H, W) of the tables: 1, 255, 256, 257 and 3 x 333 pixels -- the last block of 256 lanes is partial or absent
SHAPES = [(1, 1), (1, 255), (16, 16), (1, 257), (3, 333)]


def texels(shape):
    """(normals[H, W, 4], positions[H, W, 4], mask[H, W]) of a table, read-only."""
    H, W = shape
    i = np.arange(H * W) + 31 * SHAPES.index(shape)
    nrm = np.zeros((H * W, 4), f32)
    pos = np.ones((H * W, 4), f32)
    nrm[:, :3] = NORMALS[i % len(NORMALS)]
    pos[:, :3] = POSITIONS[i % len(POSITIONS)]
    mask = MASKS[i % len(MASKS)]
    out = nrm.reshape(H, W, 4), pos.reshape(H, W, 4), np.ascontiguousarray(mask.reshape(H, W))
    for a in out:
        a.setflags(write=False)
    return out


def _offsets(n):
    return np.stack([np.cos(np.arange(n)), np.sin(np.arange(n)), np.cos(2.0 * np.arange(n))], 1).astype(f32) * f32(0.05)


SLANT = (0.6, 0.64, 0.48)


def lights():
    """name -> Light or None.  The combine pass takes a jittered light by its centre and divides the mask by the sample count."""
    D, P = api.Light.DIRECTIONAL, api.Light.POINT
    out = {"sun": None}
    for n in (1, 16, 64):
        off = _offsets(n) if n > 1 else None
        out[f"directional{n}"] = api.Light.make(D, np.array(SLANT, f32), off)
        out[f"point{n}"] = api.Light.make(P, np.array(POINT, f32), off)
    return out


def constants(kind="unit"):
    """The constants of the tables: camera at CAMERA, the sun straight up; cameraDirection unit, zero or unnormalised."""
    direction = {"unit": (0, 0, -1), "zero": (0, 0, 0), "long": (0, -3, -4)}[kind]
    return api.RayTracingConstants.make(np.array(CAMERA, f32), np.array([0, 1, 0], f32), 4, 4, np.array(direction, f32))


def light_lists():
    """name -> (LightList, whether it holds a point light): 1, 3 and 8 mixed lights."""
    D, P = api.Light.DIRECTIONAL, api.Light.POINT
    pool = [(D, SLANT), (P, POINT), (D, (0, 1, 0)), (P, (-2.0, 0.5, 9.0)), (D, (0, -1, 0)), (P, (1.0, 2.0, 3.0)), (D, (-0.6, 0, 0.8)),
            (P, (1e30, 0, 0))]
    return {"1": (api.LightList.make(pool[:1]), False), "3": (api.LightList.make(pool[:3]), True),
            "8": (api.LightList.make(pool), True), "2_directional": (api.LightList.make([pool[0], pool[4]]), False)}


def pass_runs():
    """(constants kind, light name, with positions) of every run of the combine and facing passes on a table."""
    runs = [("unit", name, True) for name in lights()]
    runs += [("unit", "sun", False), ("unit", "directional16", False)]
    runs += [(kind, name, True) for kind in ("zero", "long") for name in ("sun", "point16")]
    return runs


# -------------------------------------------------------------------------------------- the per-pixel rules, written out in float32
def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def ndl_rule(k, light, positions, normals):
    """N.L before the clamp, operation for operation in float32 (numpy has no fused multiply-add): Combine.frag:24-28 with the point
    light's L = normalize(light - (camera + P)), left unnormalised where its length is not > 0."""
    n = np.ascontiguousarray(normals, f32)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    if light is not None and light.type == api.Light.POINT:
        P = np.ascontiguousarray(positions, f32)
        px, py, pz = (f32(k.cameraPosition[i]) + P[..., i] for i in range(3))
        lx, ly, lz = f32(light.xyz[0]) - px, f32(light.xyz[1]) - py, f32(light.xyz[2]) - pz
        ll = np.sqrt(_dot(lx, ly, lz, lx, ly, lz))
        inv = f32(1.0) / ll
        ok = ll > 0
        lx, ly, lz = np.where(ok, lx * inv, lx), np.where(ok, ly * inv, ly), np.where(ok, lz * inv, lz)
    else:
        src = light.xyz if light is not None else k.lightDirection
        lx, ly, lz = f32(src[0]), f32(src[1]), f32(src[2])
    return _dot(nx, ny, nz, lx, ly, lz)


def _background(normals):
    n = np.ascontiguousarray(normals, f32)
    return (n[..., 0] == 0) & (n[..., 1] == 0) & (n[..., 2] == 0)


def facing_rule(k, light, positions, normals):
    """uint8[H, W]: 0 for the background and where N.L <= 0 (false for a NaN: a NaN is traced), 1 elsewhere."""
    with np.errstate(all="ignore"):
        ndl = ndl_rule(k, light, positions, normals)
        return np.where(_background(normals) | (ndl <= 0), 0, 1).astype(np.uint8)


def facing_lights_rule(k, lights_list, positions, normals):
    out = np.zeros(np.asarray(normals).shape[:2], np.uint8)
    for l in range(lights_list.count):
        out |= (facing_rule(k, lights_list.light(l), positions, normals) << l).astype(np.uint8)
    return out


def combine_rule(k, light, positions, normals, mask):
    """uint8[H, W, 3]: Combine.frag:24-32 with baseColor = 1, in float32, with the conversion spelled out --
        max(0, x)   = x if x > 0 else 0            (GLSL's max: 0 for a NaN)
        byte        = 255 where scaled >= 255, int(scaled) where 0 < scaled < 255, 0 otherwise (a NaN included)
    where scaled = (direct + ambient) * 255 + 0.5."""
    with np.errstate(all="ignore"):
        n = np.ascontiguousarray(normals, f32)
        nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
        ndl = ndl_rule(k, light, positions, normals)
        ndl = np.where(ndl > 0, ndl, f32(0))
        cx, cy, cz = (f32(k.cameraDirection[i]) for i in range(3))
        cl = np.sqrt(_dot(cx, cy, cz, cx, cy, cz))
        if cl > 0:
            inv = f32(1.0) / cl
            cx, cy, cz = cx * inv, cy * inv, cz * inv
        ndv = _dot(nx, ny, nz, cx * f32(-1.0), cy * f32(-1.0), cz * f32(-1.0))
        ndv = np.where(ndv > 0, ndv, f32(0))
        samples = f32(light.nsamples) if light is not None and light.nsamples > 1 else f32(1.0)
        direct = (f32(1.25) * ndl) * (np.ascontiguousarray(mask, np.uint8).astype(f32) / samples)      # frag:29
        ambient = f32(0.15) + f32(0.05) * (f32(1.0) - ndv)                                             # frag:30
        scaled = (direct + ambient) * f32(255.0) + f32(0.5)                                            # frag:32, UNORM8
        assert scaled.dtype == f32
        inside = (scaled > 0) & (scaled < 255)
        byte = np.where(scaled >= 255, 255, np.where(inside, np.where(inside, scaled, 0).astype(np.int32), 0)).astype(np.uint8)
        byte = np.where(_background(normals), 0, byte).astype(np.uint8)
        return np.repeat(byte[..., None], 3, axis=-1)


def oracle_combine(k, light, positions, normals, mask):
    """The oracle's combine pass for the product's (light | None); positions None: zeros (the oracle reads them for a point light only)."""
    olight = oracle.light_from_product(light, k) if light is not None else None
    if positions is None:
        positions = np.zeros(np.asarray(normals).shape, f32)
    return oracle.combine(k.as_array(), olight, positions, normals, mask)
