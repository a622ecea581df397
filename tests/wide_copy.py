"""numpy restatement of what rts_wide.hip derives from a packed stream: the device verdict and the private copy of the wide
packet kernels (variants 8 and 9), written from the documented contract (the header of rts_wide.hip, DESIGN.md 4.4, the
option text of include/rts.h), not from the kernels.

* verdict bits (validateKernel): 0 structure (the rules of rts_bvh_validate), 1 a non-finite float in a node or tail vec4,
  2 an inner node with !(min <= max), 3 not a pre-order binary tree with the reference's miss links, or an inner child's box
  not inside its parent's.  Bit 3 is checked GLOBALLY here: the tree is read from (left = i + 1, right = link(left)), every
  node but the root must be the child of exactly one inner node, the pre-order numbering of that tree must be the stream's
  own and every link must be the first node after the subtree (END after the last node).
* the copy: wide node i = the i-th inner node of even depth in stream order (32 dwords); triangle record j = the j-th leaf
  in stream order (16 dwords); then the parent of every node (END for the root).

Also the mutation corpus shared by tests/test_wide_copy.py and tests/test_gpu_wide_copy.py."""
import numpy as np

import streams

END = 0xFFFFFFFF
FLT_MAX_BITS = 0x7F7FFFFF
NEG_FLT_MAX_BITS = 0xFF7FFFFF
MAX_DEPTH = 512                       # deeper trees keep the stackless kernels (rts_api.cpp, finishInstall)
MAX_WIDE_P = 1 << 24                  # 32-bit byte offsets inside the copy: 192 bytes per triangle

STRUCTURE, NONFINITE, UNORDERED, NOT_ENCLOSED = 1, 2, 4, 8


def _view(packed):
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    P = (packed.shape[0] + 2) // 5
    N = 2 * P - 1
    nodes = packed[:2 * N].reshape(N, 8)
    return packed, P, N, nodes


def _boxes(nodes):
    f = nodes.view(np.float32)
    return f[:, 0:3], f[:, 4:7]


def structure_ok(packed):
    """rts_bvh_validate's rules: 5P - 2 vec4; links strictly forward or END; an inner node has a successor; a leaf's tail
    pointer lies in [2N, 2N + P)."""
    packed = np.asarray(packed, np.uint32).reshape(-1, 4)
    n = packed.shape[0]
    if n < 3 or (n + 2) % 5 != 0:
        return False
    packed, P, N, nodes = _view(packed)
    i = np.arange(N, dtype=np.int64)
    tag, link = nodes[:, 3].astype(np.int64), nodes[:, 7].astype(np.int64)
    inner = tag == END
    ok_link = (link == END) | ((link > i) & (link < N))
    ok_inner = ~inner | (i + 1 < N)
    ok_leaf = inner | ((tag >= 2 * N) & (tag < 2 * N + P))
    return bool(ok_link.all() and ok_inner.all() and ok_leaf.all())


def tree_of(packed):
    """(parent, depth) of a stream whose bit 3 is clear, or None when the links do not describe a pre-order binary tree
    with the reference's miss links.  parent: END for the root; depth by pointer doubling."""
    packed, P, N, nodes = _view(packed)
    tag, link = nodes[:, 3].astype(np.int64), nodes[:, 7].astype(np.int64)
    inner = np.flatnonzero(tag == END)
    if (inner + 1 >= N).any():
        return None
    left = inner + 1
    right = link[left]
    if ((right == END) | (right <= left) | (right >= N)).any():
        return None
    parent = np.full(N, -1, np.int64)
    indeg = np.zeros(N, np.int64)
    np.add.at(indeg, left, 1)
    np.add.at(indeg, right, 1)
    if indeg[0] != 0 or (indeg[1:] != 1).any():
        return None
    parent[left] = inner
    parent[right] = inner
    # every child has a larger index than its parent and every node but 0 has exactly one parent: a tree rooted at 0.
    # depth by pointer doubling
    depth = (parent >= 0).astype(np.int64)
    anc = np.where(parent >= 0, parent, 0)
    while (anc != 0).any():
        depth = depth + depth[anc]
        anc = anc[anc]
    # subtree sizes bottom-up, level by level
    size = np.ones(N, np.int64)
    order = np.argsort(-depth, kind="stable")
    d_sorted = depth[order]
    cuts = np.flatnonzero(np.diff(d_sorted)) + 1
    for grp in np.split(order, cuts):
        if depth[grp[0]] == 0:
            break
        np.add.at(size, parent[grp], size[grp])
    # pre-order numbering of that tree, top-down: pre(left) = pre(i) + 1, pre(right) = pre(i) + 1 + size(left)
    pre = np.zeros(N, np.int64)
    order = np.argsort(depth, kind="stable")
    d_sorted = depth[order]
    cuts = np.flatnonzero(np.diff(d_sorted)) + 1
    is_inner = tag == END
    for grp in np.split(order, cuts):
        g = grp[is_inner[grp]]
        if g.size == 0:
            continue
        l, r = g + 1, link[g + 1]
        pre[l] = pre[g] + 1
        pre[r] = pre[g] + 1 + size[l]
    if (pre != np.arange(N)).any():
        return None
    want = np.arange(N) + size
    want = np.where(want >= N, END, want)
    if (link != want).any():
        return None
    parent = np.where(parent >= 0, parent, END).astype(np.int64)
    return parent, depth


def verdict(packed):
    """The four flag bits of validateKernel for `packed` (bits 1..3 only mean something when bit 0 is clear)."""
    if not structure_ok(packed):
        return STRUCTURE
    packed, P, N, nodes = _view(packed)
    bits = 0
    f = packed.view(np.float32)
    node_f = nodes.view(np.float32)[:, [0, 1, 2, 4, 5, 6]]
    tail_f = f[2 * N:, :3]
    if not (np.isfinite(node_f).all() and np.isfinite(tail_f).all()):
        bits |= NONFINITE
    lo, hi = _boxes(nodes)
    inner = nodes[:, 3] == END
    with np.errstate(invalid="ignore"):
        if (~(lo[inner] <= hi[inner])).any():
            bits |= UNORDERED
    tree = tree_of(packed)
    if tree is None:
        return bits | NOT_ENCLOSED
    parent = tree[0]
    child = np.flatnonzero(inner & (parent != END))            # inner children: their parent's box holds theirs
    p = parent[child]
    with np.errstate(invalid="ignore"):
        ok = (lo[p] <= lo[child]) & (hi[child] <= hi[p])
    if (~ok).any():
        bits |= NOT_ENCLOSED
    return bits


def restate(packed, max_depth=MAX_DEPTH):
    """dict: bits, allowed, levels, wide_nodes, and (when allowed) wide (W, 32), tris (P, 16), parents (N,) as uint32 and
    copy = the bytes rtsh_ctx_read_private_copy returns (empty without a copy)."""
    bits = verdict(packed)
    out = {"bits": bits, "allowed": False, "levels": 0, "wide_nodes": 0, "copy": np.zeros(0, np.uint8)}
    if bits:
        return out
    packed, P, N, nodes = _view(packed)
    if not (2 <= P <= MAX_WIDE_P):
        return out
    parent, depth = tree_of(packed)
    tag, link = nodes[:, 3].astype(np.int64), nodes[:, 7].astype(np.int64)
    leaf = tag != END
    deepest = int(depth[leaf].max())
    if deepest > max_depth:
        return out
    wroot = ~leaf & (depth % 2 == 0)
    wide_rank = np.cumsum(wroot) - 1
    leaf_rank = np.cumsum(leaf) - 1
    roots = np.flatnonzero(wroot)
    W = roots.size
    # four candidate slots per wide node in child / grandchild order: (box node, reference, slot node, filled)
    left = roots + 1
    right = link[left]
    cand_box = np.zeros((W, 4), np.int64)
    cand_ref = np.zeros((W, 4), np.int64)
    cand_node = np.zeros((W, 4), np.int64)
    filled = np.zeros((W, 4), bool)
    for c, col in ((left, 0), (right, 2)):
        cl = leaf[c]
        # the child itself a leaf: one slot, the wide node's own box
        cand_box[:, col] = np.where(cl, roots, 0)
        cand_node[:, col] = np.where(cl, c, 0)
        cand_ref[:, col] = np.where(cl, leaf_rank[c] * 64 + 1, 0)
        filled[:, col] = cl
        # an inner child: its two children, a leaf carrying the child's box, an inner node its own
        gl = np.where(cl, 0, c + 1)
        gr = np.where(cl, 0, link[np.minimum(c + 1, N - 1)])
        for g, k in ((gl, col), (gr, col + 1)):
            gleaf = leaf[g]
            box = np.where(gleaf, c, g)
            ref = np.where(gleaf, leaf_rank[g] * 64 + 1, wide_rank[g] * 128)
            cand_box[:, k] = np.where(cl, cand_box[:, k], box)
            cand_node[:, k] = np.where(cl, cand_node[:, k], g)
            cand_ref[:, k] = np.where(cl, cand_ref[:, k], ref)
            filled[:, k] = np.where(cl, filled[:, k], True)
    order = np.argsort(~filled, axis=1, kind="stable")       # filled slots first, in their order
    take = lambda a: np.take_along_axis(a, order, axis=1)
    cand_box, cand_ref, cand_node, filled = take(cand_box), take(cand_ref), take(cand_node), take(filled)
    wide = np.zeros((W, 32), np.uint32)
    for k in range(4):
        b = nodes[cand_box[:, k]]
        f = filled[:, k]
        wide[:, 6 * k + 0:6 * k + 3] = np.where(f[:, None], b[:, 0:3], FLT_MAX_BITS)
        wide[:, 6 * k + 3:6 * k + 6] = np.where(f[:, None], b[:, 4:7], NEG_FLT_MAX_BITS)
        wide[:, 24 + k] = np.where(f, cand_ref[:, k], END)
        if k:
            wide[:, 28 + k] = np.where(f, cand_node[:, k], END)
    wide[:, 28] = roots
    leaves = np.flatnonzero(leaf)
    tris = np.zeros((P, 16), np.uint32)
    tris[:, 0:3] = packed[tag[leaves], 0:3]
    tris[:, 3:6] = nodes[leaves, 0:3]
    tris[:, 6:9] = nodes[leaves, 4:7]
    tris[:, 9] = leaves
    pb = nodes[parent[leaves]]
    tris[:, 10:13] = pb[:, 0:3]
    tris[:, 13:16] = pb[:, 4:7]
    parents = parent.astype(np.uint32)
    copy = np.concatenate([wide.reshape(-1).view(np.uint8), tris.reshape(-1).view(np.uint8), parents.view(np.uint8)])
    out.update(allowed=True, levels=deepest // 2 + 1, wide_nodes=W, wide=wide, tris=tris, parents=parents, copy=copy,
               slot_nodes=np.where(filled, cand_node, END), depth=depth)
    return out


def first_difference(got, rs, P):
    """A readable description of the first dword in which `got` (bytes of read_private_copy) differs from the restatement."""
    want = rs["copy"]
    if got.size != want.size:
        return f"size {got.size} bytes, restated {want.size}"
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero(g != w)
    if bad.size == 0:
        return None
    d = int(bad[0])
    nw = rs["wide_nodes"] * 32
    if d < nw:
        where = f"wide node {d // 32} (stream node {int(w[(d // 32) * 32 + 28])}) dword {d % 32}"
    elif d < nw + P * 16:
        where = f"triangle record {(d - nw) // 16} dword {(d - nw) % 16}"
    else:
        where = f"parents[{d - nw - P * 16}]"
    return f"{bad.size} dwords differ; first: {where}: got {int(g[d]):#010x}, restated {int(w[d]):#010x}"


# ---- tree shapes -------------------------------------------------------------------------------------------------------------
def complete(lo, hi):
    return lo if hi - lo == 1 else (complete(lo, (lo + hi) // 2), complete((lo + hi) // 2, hi))


def chain(P):
    """A chain: one leaf off every inner node; the deepest leaves sit at depth P - 1."""
    tree = P - 1
    for i in range(P - 2, -1, -1):
        tree = (i, tree)
    return tree


# ---- the mutation corpus -----------------------------------------------------------------------------------------------------
def _tris(P, seed, scale=1.0, offset=0.0):
    """P tilted triangles spread along a diagonal, each in its own cell of a 2 x 2 x P/2 grid."""
    rs = np.random.RandomState(seed)
    c = np.stack([np.arange(P) % 2 * 3.0, np.arange(P) // 2 % 2 * 3.0, np.arange(P) * 1.5], 1)[:, None, :]
    t = c + 0.2 + rs.random_sample((P, 3, 3)) * 2.0
    return (t * scale).astype(np.float32) + np.asarray(offset, np.float32)


BASE_TREE = ((((0, 1), (2, 3)), ((4, 5), 6)), (7, ((8, 9), 10)))      # inner children at depths 1..3, leaves at 2..4


def _base(scale=1.0, offset=0.0, seed=1):
    tris = _tris(11, seed, scale, offset)
    return streams.stream_from_tree(BASE_TREE, tris), tris


def _inner_children(packed):
    _, P, N, nodes = _view(packed)
    parent, _ = tree_of(packed)
    inner = nodes[:, 3] == END
    return [int(i) for i in np.flatnonzero(inner & (parent != END))], parent


def _fset(packed, node, dword, value):
    f = packed.view(np.float32)
    f.reshape(-1)[node * 8 + dword] = np.float32(value)


def _fget(packed, node, dword):
    return packed.view(np.float32).reshape(-1)[node * 8 + dword]


def corpus():
    """[(name, packed, expected bits, compared bits, target node)]: small valid streams and mutations of them.  The verdict of
    each is known by hand (expected & compared); `target` is the node whose (original) box the rays of the GPU test aim at."""
    out = []
    base, tris = _base()
    P = tris.shape[0]
    N = 2 * P - 1
    kids, parent = _inner_children(base)
    out.append(("base", base, 0, 0xF, 0))
    # a child box grown by one ulp past its parent's, on each face; the child chosen among those sharing that face
    for face in range(6):
        dw = face if face < 3 else face + 1                     # dwords 0..2 min, 4..6 max
        outward = -np.inf if face < 3 else np.inf
        shared = [c for c in kids if _fget(base, c, dw) == _fget(base, int(parent[c]), dw)]
        c = shared[-1] if shared else kids[-1]
        m = base.copy()
        _fset(m, c, dw, np.nextafter(_fget(base, int(parent[c]), dw), np.float32(outward)))
        out.append((f"grown_face{face}_node{c}", m, NOT_ENCLOSED, 0xF, c))
    # a child's box equal to its parent's: still inside it
    c = kids[1]
    m = base.copy()
    for dw in (0, 1, 2, 4, 5, 6):
        _fset(m, c, dw, _fget(base, int(parent[c]), dw))
    out.append((f"child_equals_parent_node{c}", m, 0, 0xF, c))
    # -0 against +0 on a shared face, both ways, min and max side: IEEE -0 <= +0 and +0 <= -0 both hold
    zb, ztris = _base(offset=-_tris(11, 1).reshape(-1, 3).min(0))                           # the scene's minimum corner at exactly 0 on every axis
    zkids, zparent = _inner_children(zb)
    for axis in range(3):
        c = [k for k in zkids if _fget(zb, k, axis) == 0.0 and _fget(zb, int(zparent[k]), axis) == 0.0][0]
        for pz, cz in ((-0.0, 0.0), (0.0, -0.0)):
            m = zb.copy()
            _fset(m, int(zparent[c]), axis, pz)
            _fset(m, c, axis, cz)
            out.append((f"signed_zero_min{axis}_parent{pz:+}_child{cz:+}", m, 0, 0xF, c))
    neg = _base(offset=-_tris(11, 1).reshape(-1, 3).max(0))[0]     # maximum corner at 0
    nkids, nparent = _inner_children(neg)
    for axis in range(3):
        cs = [k for k in nkids if _fget(neg, k, 4 + axis) == 0.0 and _fget(neg, int(nparent[k]), 4 + axis) == 0.0]
        if not cs:
            continue
        c = cs[0]
        m = neg.copy()
        _fset(m, int(nparent[c]), 4 + axis, -0.0)
        _fset(m, c, 4 + axis, 0.0)
        out.append((f"signed_zero_max{axis}_parent-0_child+0", m, 0, 0xF, c))
    # non-finite values: an inner box (NaN fails every comparison, +-inf leaves its parent), a leaf edge, a tail v0
    c = kids[0]
    for what, val, dw, bits in (("nan_min", np.nan, 0, NONFINITE | UNORDERED | NOT_ENCLOSED),
                                ("nan_max", np.nan, 5, NONFINITE | UNORDERED | NOT_ENCLOSED),
                                ("neg_inf_min", -np.inf, 1, NONFINITE | NOT_ENCLOSED),
                                ("pos_inf_max", np.inf, 6, NONFINITE | NOT_ENCLOSED)):
        m = base.copy()
        _fset(m, c, dw, val)
        out.append((f"{what}_node{c}", m, bits, 0xF, c))
    m = base.copy()
    _fset(m, 0, 4, np.nan)                                      # the root itself
    out.append(("nan_root_max", m, NONFINITE | UNORDERED | NOT_ENCLOSED, 0xF, 0))
    leaves = [i for i in range(N) if base[2 * i, 3] != END]
    for what, val, dw in (("nan_leaf_e0", np.nan, 1), ("inf_leaf_e1", np.inf, 6), ("neg_inf_leaf_e0", -np.inf, 2)):
        m = base.copy()
        _fset(m, leaves[3], dw, val)
        out.append((f"{what}_node{leaves[3]}", m, NONFINITE, 0xF, int(parent[leaves[3]])))
    for what, val in (("nan_tail_v0", np.nan), ("inf_tail_v0", np.inf)):
        m = base.copy()
        m.view(np.float32)[2 * N + 4, 1] = val
        out.append((what, m, NONFINITE, 0xF, 0))
    m = base.copy()
    m.view(np.float32)[2 * N + 4, 3] = np.nan                   # the tail's w is not part of the stream's geometry
    out.append(("nan_tail_w", m, 0, 0xF, 0))
    # denormal geometry, and one ulp past a denormal face
    den, dtris = _base(scale=np.float32(1e-40))
    assert (np.abs(dtris) < np.finfo(np.float32).tiny).all()
    out.append(("denormal", den, 0, 0xF, 0))
    dkids, dparent = _inner_children(den)
    c = dkids[2]
    m = den.copy()
    _fset(m, c, 4, np.nextafter(_fget(den, int(dparent[c]), 4), np.float32(np.inf)))
    out.append((f"denormal_grown_node{c}", m, NOT_ENCLOSED, 0xF, c))
    # min > max on one axis of an inner node whose children are leaves (nothing below it to enclose)
    pairs = [k for k in kids if base[2 * (k + 1), 3] != END and base[2 * int(base[2 * (k + 1) + 1, 3]), 3] != END]
    c = pairs[0]
    m = base.copy()
    lo, hi = _fget(base, c, 1), _fget(base, c, 5)
    _fset(m, c, 1, hi)
    _fset(m, c, 5, lo)
    out.append((f"swapped_min_max_node{c}", m, UNORDERED, 0xF, c))
    # a right child whose miss link differs from its parent's
    rights = [int(base[2 * (p + 1) + 1, 3]) for p in range(N) if base[2 * p, 3] == END]
    r = [x for x in rights if base[2 * x, 3] == END and base[2 * x + 1, 3] != END][0]
    m = base.copy()
    m[2 * r + 1, 3] = END
    out.append((f"right_child_link_node{r}", m, NOT_ENCLOSED, 0xF, r))
    # an orphaned subtree: an inner node turned into a leaf that links past its former children
    c = pairs[0]
    m = base.copy()
    m[2 * c, 3] = base[2 * (c + 1), 3]                          # a tail pointer of one of its children
    out.append((f"orphans_under_node{c}", m, NOT_ENCLOSED, 0xF, int(parent[c])))
    # an orphaned leaf: a leaf whose link skips the next node (a forward link, so the structure rules still pass)
    lf = [x for x in leaves if x + 2 < N][0]
    m = base.copy()
    m[2 * lf + 1, 3] = lf + 2
    out.append((f"leaf_link_skips_node{lf}", m, NOT_ENCLOSED, 0xF, int(parent[lf])))
    # structure: backward and self links, a missing successor, tail pointers out of range
    for what, node, val in (("backward_link", leaves[4], leaves[4] - 1), ("self_link", leaves[4], leaves[4]),
                            ("link_past_end", leaves[4], N)):
        m = base.copy()
        m[2 * node + 1, 3] = val
        out.append((f"{what}_node{node}", m, STRUCTURE, STRUCTURE, 0))
    for what, val in (("tail_below", 2 * N - 1), ("tail_past_end", 2 * N + P), ("tail_far", 0x7FFFFFFF)):
        m = base.copy()
        m[2 * leaves[2], 3] = val
        out.append((f"{what}_node{leaves[2]}", m, STRUCTURE, STRUCTURE, 0))
    m = base.copy()
    m[2 * (N - 1), 3] = END                                     # the last node made inner: no i + 1
    out.append(("last_node_inner", m, STRUCTURE, STRUCTURE, 0))
    # two leaves that share one tail pointer: a valid stream (the other tail vec4 is unused, but still checked for finiteness)
    m = base.copy()
    m[2 * leaves[5], 3] = m[2 * leaves[6], 3]
    out.append((f"shared_tail_nodes{leaves[5]}_{leaves[6]}", m, 0, 0xF, int(parent[leaves[5]])))
    m2 = m.copy()
    m2.view(np.float32)[int(base[2 * leaves[5], 3]), 0] = np.inf  # ... the unused one non-finite
    out.append(("shared_tail_unused_inf", m2, NONFINITE, 0xF, 0))
    return out


# ---- confirmation at its edge: boxes shrunk so that triangles stick out ------------------------------------------------------
SIGMA = np.array([1.0, -1.0, 1.0])             # the sign of every ray direction in the frame (all components far from 0)
K_RANGE = np.arange(-4, 68)                    # crossing points, in ulps outward of the shrunk face (72 columns)
LATERAL = 12                                   # rows per face


def _ulps(f, k):
    """float32 value k ulps above f (k may be negative); f and the result keep one sign."""
    b = np.float32(f).view(np.int32).astype(np.int64)
    step = np.where(np.float32(f) >= 0, k, -k)
    return (b + step).astype(np.int32).view(np.float32)


# (kind, shrunk axis a, entry axis b): the face of a on the side rays leave by is shrunk; rays enter the box's region through
# the face of b they come from, at a crossing point that sweeps a's new face.  kind "zero": the box is flat on axis a;
# "apart": a small box inside the old one that meets neither triangle.
CONFIRM_PAIRS = (("face", 0, 1), ("face", 1, 2), ("face", 2, 0), ("face", 0, 2), ("zero", 1, 0), ("apart", 2, 1))
# pairs at odd depths (1, 3) and even depths (4): a leaf slot then carries the box of an odd-depth child or the wide node's own
CONFIRM_TREE = ((0, 1), ((((2, 3), (4, 5)), (6, 7)), ((8, 9), (10, 11))))


def confirmation_scene():
    """dict: packed (the shrunk stream), plain (the same tree with true unions), tris, pairs [(node, depth, kind, box lo, hi)],
    positions (H, W, 4) with camera at the origin, light (a point), k (H, W) nominal ulps past the face, pair_of (H, W)."""
    canon = np.array([[[0.0, 1.0, 0.0], [2.0, 0.95, 0.0], [0.0, 0.95, 1.2]],           # the big one: sticks out past x = 1.25
                      [[0.1, 0.1, 0.1], [0.4, 0.2, 0.1], [0.1, 0.3, 0.4]]], np.float64)
    canon_box = {"face": ([0.0, 0.1, 0.0], [1.25, 1.0, 1.2]), "zero": ([1.25, 0.1, 0.0], [1.25, 1.0, 1.2]),
                 "apart": ([1.5, 0.1, 0.9], [1.9, 0.3, 1.1])}
    tris = np.zeros((12, 3, 3), np.float32)
    maps = []
    for p, (kind, a, b) in enumerate(CONFIRM_PAIRS):
        c = 3 - a - b
        perm = np.zeros((3, 3))
        perm[a, 0] = SIGMA[a]                                   # canonical x (leaving +) -> axis a
        perm[b, 1] = -SIGMA[b]                                  # canonical y (entered from above, going -) -> axis b
        perm[c, 2] = SIGMA[c]                                   # canonical z (going +) -> axis c
        offset = np.array([3.0 + 4.0 * p, 5.0 - 3.0 * p, 2.0 + 4.5 * p])
        maps.append((perm, offset))
        tris[2 * p:2 * p + 2] = (canon @ perm.T + offset).astype(np.float32)
    plain = streams.stream_from_tree(CONFIRM_TREE, tris)
    parent, depth = tree_of(plain)
    edits, pairs = {}, []
    for p, (kind, a, b) in enumerate(CONFIRM_PAIRS):
        perm, offset = maps[p]
        node = int(parent[np.flatnonzero(plain[:2 * (2 * len(tris) - 1):2, 3] == 2 * (2 * len(tris) - 1) + 2 * p)[0]])
        lo_c, hi_c = (np.array(x, np.float64) for x in canon_box[kind])
        corners = np.stack([lo_c, hi_c]) @ perm.T + offset
        lo, hi = corners.min(0).astype(np.float32), corners.max(0).astype(np.float32)
        f = plain.view(np.float32)
        lo, hi = np.maximum(lo, f[2 * node, :3]), np.minimum(hi, f[2 * node + 1, :3])
        if kind == "zero":
            lo[a] = hi[a]
        edits[node] = (lo, hi)
        pairs.append((node, int(depth[node]), kind, lo, hi))
    packed = streams.shrink_boxes(plain, edits)
    light = np.array([80.0, -60.0, 110.0], np.float32)         # far along SIGMA from every pair
    H, W = LATERAL * len(CONFIRM_PAIRS), K_RANGE.size
    positions = np.zeros((H, W, 4), np.float32)
    kk = np.zeros((H, W), np.int64)
    pair_of = np.zeros((H, W), np.int64)
    for p, (kind, a, b) in enumerate(CONFIRM_PAIRS):
        node, _, _, lo, hi = pairs[p]
        if kind == "apart":                                     # the rays of a "face" pair: they hit the big triangle
            perm, offset = maps[p]
            corners = np.stack([np.array(x, np.float64) for x in canon_box["face"]]) @ perm.T + offset
            lo, hi = corners.min(0).astype(np.float32), corners.max(0).astype(np.float32)
        c = 3 - a - b
        face = hi[a] if SIGMA[a] > 0 else lo[a]
        entry = hi[b] if SIGMA[b] < 0 else lo[b]
        for row in range(LATERAL):
            X = np.zeros((W, 3), np.float64)
            X[:, a] = _ulps(face, K_RANGE * int(SIGMA[a]))
            X[:, b] = entry
            t = 0.05 + 0.2 * row / (LATERAL - 1)                # across axis c, inside the box, from its entry side
            X[:, c] = lo[c] + t * (hi[c] - lo[c]) if SIGMA[c] > 0 else hi[c] - t * (hi[c] - lo[c])
            d = light.astype(np.float64) - X
            pos = X - 0.01 * d                                  # behind the crossing point, away from the light
            r = p * LATERAL + row
            positions[r, :, :3] = pos.astype(np.float32)
            kk[r] = K_RANGE
            pair_of[r] = p
    return {"packed": packed, "plain": plain, "tris": tris, "pairs": pairs, "positions": positions, "light": light, "k": kk,
            "pair_of": pair_of}


def confirmation_rays(s, offsets=None):
    """Counts over the confirmation frame (one sample, or `offsets` as the light's samples): rays that hit a triangle of a
    shrunk pair outside its exact box, 1..16 ulps past the face, and are lit (teeth), split by the parity of the pair's depth."""
    import oracle
    from raytracedshadows_amd import api
    H, W = s["k"].shape
    k = api.RayTracingConstants.make([0, 0, 0], [0, 1, 0], W, H)
    light = api.Light.make(api.Light.POINT, s["light"], offsets)
    rays = oracle.gen_rays(k.as_array(), oracle.light_from_product(light, k), s["positions"])
    ns = rays.shape[0] // (H * W)
    occluded = oracle.trace_rays(s["packed"], rays)[0] == 0
    brute = oracle.brute_force_rays(s["packed"], s["tris"].shape[0], rays) == 0
    assert (brute | ~occluded).all(), "the walk found a hit brute force did not"
    kk = np.repeat(s["k"].reshape(-1), ns)
    pair = np.repeat(s["pair_of"].reshape(-1), ns)
    teeth = np.zeros(rays.shape[0], bool)
    parity = [0, 0]
    inv = (np.float32(1.0) / rays[:, 4:7]).astype(np.float32)
    for p, (node, depth, kind, lo, hi) in enumerate(s["pairs"]):
        sel = pair == p
        tri = np.zeros(rays.shape[0], bool)
        for t in (2 * p, 2 * p + 1):
            tri |= oracle.trace_rays(streams.stream_from_tree(0, s["tris"][t:t + 1]), rays)[0] == 0
        inbox = np.array([oracle.ray_box(rays[i, :3], inv[i], lo, hi) if sel[i] else False for i in range(rays.shape[0])])
        t = sel & tri & ~inbox & (kk > 0) & (kk <= 16) & ~occluded
        assert brute[t].all()
        teeth |= t
        parity[depth % 2] += int(t.sum())
    return {"rays": rays.shape[0], "teeth": int(teeth.sum()), "by_depth_parity": parity, "occluded": int(occluded.sum())}
