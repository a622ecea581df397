"""Hand-made packed streams (SURVEY.md Appendix A layout) for tests that need a tree SHAPE no builder would produce.

A tree is nested 2-tuples; an int is a leaf holding that triangle.  Boxes are the exact float32 min/max union of the
children's (what BVHBuilder.cpp:53-76 computes), nodes are numbered in pre-order, miss links follow BVHBuilder.cpp:222-244."""
import numpy as np

END = 0xFFFFFFFF


def stream_from_tree(tree, tris):
    """tris: (P, 3, 3) float32 vertices.  Returns the packed (5P-2, 4) uint32 stream."""
    tris = np.ascontiguousarray(tris, np.float32)
    P = tris.shape[0]
    N = 2 * P - 1
    nodes = []                                         # (kind, payload, size, lo, hi) in pre-order

    def walk(t):
        at = len(nodes)
        nodes.append(None)
        if isinstance(t, tuple):
            l, r = walk(t[0]), walk(t[1])
            lo = np.minimum(nodes[l][3], nodes[r][3])
            hi = np.maximum(nodes[l][4], nodes[r][4])
            nodes[at] = ("inner", None, nodes[l][2] + nodes[r][2] + 1, lo, hi)
        else:
            v = tris[t]
            nodes[at] = ("leaf", int(t), 1, v.min(0), v.max(0))
        return at

    import sys
    sys.setrecursionlimit(max(10000, sys.getrecursionlimit()))
    walk(tree)
    assert len(nodes) == N, (len(nodes), N)
    out = np.zeros((5 * P - 2, 4), np.uint32)
    f = out.view(np.float32)
    seen = set()
    for i, (kind, prim, size, lo, hi) in enumerate(nodes):
        nxt = i + size if i + size < N else END
        if kind == "inner":
            f[2 * i, :3] = lo
            out[2 * i, 3] = END
            f[2 * i + 1, :3] = hi
        else:
            v0, v1, v2 = tris[prim]
            f[2 * i, :3] = v1 - v0
            out[2 * i, 3] = 2 * N + prim
            f[2 * i + 1, :3] = v2 - v0
            f[2 * N + prim, :3] = v0
            seen.add(prim)
        out[2 * i + 1, 3] = nxt
    assert len(seen) == P
    return out


def deep_bushy_stream(levels):
    """A tree whose wide walk keeps three subtrees pending per level: node(l) = ((node(l-1), small), (small, small)), small =
    two tiny triangles in opposite corners of the unit square (its box covers the middle, where every ray passes; the
    triangles are hit by nobody).  Level 0 holds two real occluders."""
    tris, z = [], [0.0]

    def tiny(x, y):
        tris.append([[x, y, z[0]], [x + 1e-3, y, z[0]], [x, y + 1e-3, z[0]]])
        return len(tris) - 1

    def small():
        z[0] += 0.25
        a = tiny(0.05, 0.05)
        z[0] += 0.25
        return (a, tiny(0.95, 0.95))

    def node(l):
        if l == 0:
            z[0] += 0.5
            tris.append([[0.0, 0.0, z[0]], [0.55, 0.0, z[0]], [0.0, 0.9, z[0]]])          # occludes the rays of one corner
            tris.append([[0.6, 0.6, z[0] + 0.1], [0.9, 0.6, z[0] + 0.1], [0.6, 0.9, z[0] + 0.1]])
            return (len(tris) - 2, len(tris) - 1)
        return ((node(l - 1), small()), (small(), small()))

    tree = node(levels)
    return stream_from_tree(tree, np.array(tris, np.float32))


def shrink_boxes(packed, boxes):
    """A copy of `packed` in which inner nodes whose two children are both leaves get smaller boxes: `boxes` maps a node index
    to (bboxMin, bboxMax).  Each new box must lie inside the node's old one, so every ancestor still encloses it (the stream
    stays "enclosed") while the node's triangles stick out of it -- or miss it altogether."""
    out = np.array(packed, np.uint32).reshape(-1, 4)
    f = out.view(np.float32)
    for node, (lo, hi) in boxes.items():
        assert out[2 * node, 3] == END, f"node {node} is a leaf"
        left = node + 1
        right = out[2 * left + 1, 3]
        assert out[2 * left, 3] != END and out[2 * right, 3] != END, f"node {node}: both children must be leaves"
        lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
        assert (f[2 * node, :3] <= lo).all() and (hi <= f[2 * node + 1, :3]).all() and (lo <= hi).all(), node
        f[2 * node, :3] = lo
        f[2 * node + 1, :3] = hi
    return out


def triangles_of(packed):
    """(P, 3, 3) triangles of a stream, in tail order: v0, v0 + e0, v0 + e1."""
    packed = np.asarray(packed, np.uint32).reshape(-1, 4)
    P = (packed.shape[0] + 2) // 5
    N = 2 * P - 1
    nodes = packed[:2 * N].reshape(N, 8)
    f = nodes.view(np.float32)
    leaves = np.flatnonzero(nodes[:, 3] != END)
    prim = nodes[leaves, 3].astype(np.int64) - 2 * N
    t = np.zeros((P, 3, 3), np.float32)
    v0 = packed[2 * N:].view(np.float32)[:, :3]
    t[prim, 0] = v0[prim]
    t[prim, 1] = v0[prim] + f[leaves, 0:3]
    t[prim, 2] = v0[prim] + f[leaves, 4:7]
    return t


def aimed_frame(packed, target, W=32, H=32, seed=0):
    """Positions, constants and a point light such that every ray passes through the box of node `target` (or, when that box is
    not a finite ordered one, through the box of the stream's finite vertices)."""
    from raytracedshadows_amd import api
    packed = np.asarray(packed, np.uint32).reshape(-1, 4)
    f = packed.view(np.float32)
    lo, hi = f[2 * target, :3].astype(np.float64), f[2 * target + 1, :3].astype(np.float64)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        t = triangles_of(packed).reshape(-1, 3).astype(np.float64)
        t = t[np.isfinite(t).all(1)]
        lo, hi = t.min(0), t.max(0)
    ext = max(float((hi - lo).max()), 1e-30)
    c = (lo + hi) / 2
    light = c + ext * np.array([7.0, 9.0, 11.0])
    rs = np.random.RandomState(seed)
    T = lo - 0.05 * ext + rs.random_sample((H * W, 3)) * ((hi - lo) + 0.1 * ext)
    pos = np.zeros((H, W, 4), np.float32)
    pos[..., :3] = (T - 0.3 * (light - T)).reshape(H, W, 3)
    k = api.RayTracingConstants.make([0, 0, 0], [0.3, 0.8, 0.5], W, H)
    return pos, k, api.Light.make(api.Light.POINT, light.astype(np.float32))


def orphan_streams():
    """(good, bad): a three-triangle tree, and the same triangles in a stream rts_bvh_validate accepts although a leaf's miss link
    skips two nodes -- the skipped nodes are orphans no walk reaches, so the stream is not a pre-order tree (no private copy)."""
    tris = np.zeros((3, 3, 3), np.float32)
    tris[0] = [[0, 0, 5], [4, 0, 5], [0, 4, 5]]
    tris[1] = [[6, 6, 7], [9, 6, 7], [6, 9, 7]]
    tris[2] = [[2, 2, 3], [3, 2, 3], [2, 3, 3]]                       # only the stray leaves point at it
    good = stream_from_tree(((0, 1), 2), tris)                        # N = 5: 0 inner, 1 inner, 2 leaf, 3 leaf, 4 leaf
    N = 5
    bad = good.copy()
    # root 0 -> children: leaf 1 (link 4) and leaf 4; nodes 2 and 3 are stray leaves
    f = bad.view(np.float32)
    f[2, :3] = tris[0, 1] - tris[0, 0]; bad[2, 3] = 2 * N + 0
    f[3, :3] = tris[0, 2] - tris[0, 0]; bad[3, 3] = 4
    for i in (2, 3):
        f[2 * i, :3] = tris[2, 1] - tris[2, 0]; bad[2 * i, 3] = 2 * N + 2
        f[2 * i + 1, :3] = tris[2, 2] - tris[2, 0]; bad[2 * i + 1, 3] = i + 1
    f[8, :3] = tris[1, 1] - tris[1, 0]; bad[8, 3] = 2 * N + 1
    f[9, :3] = tris[1, 2] - tris[1, 0]; bad[9, 3] = END
    return good, bad


def orphan_frame(W=64, H=64):
    """The grid of texels below orphan_streams' triangles and the constants whose directional light looks up at them."""
    from raytracedshadows_amd import api
    pos = np.zeros((H, W, 4), np.float32)
    pos[..., 0] = 10.0 * (np.arange(W, dtype=np.float32)[None, :] + 0.5) / W
    pos[..., 1] = 10.0 * (np.arange(H, dtype=np.float32)[:, None] + 0.5) / H
    return pos, api.RayTracingConstants.make([0, 0, 0], [0.001, 0.002, 1.0], W, H)


def degenerate_triangles(P=400, seed=5):
    """(P, 3, 3): random triangles of which the first 250 are zero-area ('hit' through the all-NaN rule)
    or have denormal edges (which must not be flushed).  Returns (triangles, the RandomState for the caller's rays)."""
    rs = np.random.RandomState(seed)
    c = rs.random_sample((P, 1, 3)) * 10
    tri = (c + (rs.random_sample((P, 3, 3)) - 0.5)).astype(np.float32)
    tri[0:50, 1] = tri[0:50, 0]                                                    # v1 == v0
    tri[50:100, 2] = tri[50:100, 1]                                                # v2 == v1 (sliver to a line)
    tri[100:150] = tri[100:150, 0:1]                                               # all three equal (a point)
    tiny = np.float32(1e-41)
    tri[150:200, 1] = tri[150:200, 0] + np.array([tiny, 0, 0], np.float32)         # denormal-ish edge lengths
    base = np.zeros((50, 3, 3), np.float32)
    base[:, 1, 0] = tiny * 3
    base[:, 2, 1] = tiny * 5
    tri[200:250] = base                                                            # denormal triangles at the origin
    return tri, rs


def infinite_root(packed):
    """A copy of `packed` whose root box is everything (-Inf .. +Inf), as another producer may write it."""
    out = np.array(packed, np.uint32).reshape(-1, 4).copy()
    f = out.view(np.float32)
    f[0, 0:3] = -np.inf
    f[1, 0:3] = np.inf
    return out


def swapped_boxes(packed, first=5, last=40):
    """A copy of `packed` in which the inner nodes first..last (counted among the inner nodes) have bboxMin.x and bboxMax.x swapped."""
    out = np.array(packed, np.uint32).reshape(-1, 4).copy()
    P = (out.shape[0] + 2) // 5
    N = 2 * P - 1
    inner = np.nonzero(out[0:2 * N:2, 3] == END)[0][first:last]
    for i in inner:
        out[2 * i, 0], out[2 * i + 1, 0] = out[2 * i + 1, 0], out[2 * i, 0]
    return out


def gate_soup(seed=21, n=4000):
    """(packed, triangles): small random triangles in the unit cube over a two-triangle floor at y = 0 -- the scene of the ray
    set-up's gate tests (tests/test_gpu_ray_setup.py)."""
    from raytracedshadows_amd import api
    rng = np.random.RandomState(seed)
    c = rng.random_sample((n, 1, 3))
    tri = c + (rng.random_sample((n, 3, 3)) - 0.5) * 0.08
    floor = np.array([[[-1, 0, -1], [2, 0, -1], [2, 0, 2]], [[-1, 0, -1], [2, 0, 2], [-1, 0, 2]]], np.float64)
    tri = np.concatenate([tri, floor]).astype(np.float32)
    verts = np.zeros((tri.shape[0] * 3, 8), np.float32)
    verts[:, :3] = tri.reshape(-1, 3)
    idx = np.arange(tri.shape[0] * 3, dtype=np.uint32)
    return api.BVHBuilder().build(verts, 8, idx, tri.shape[0]).m_packedNodes, tri
