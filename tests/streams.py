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
