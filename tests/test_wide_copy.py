"""CPU: the numpy restatement of kernel 8's private copy and of the device verdict (tests/wide_copy.py), pinned by hand-derived
known answers, by structural properties on builder streams and by rts_bvh_validate on a mutation corpus; and the frame of the
confirmation test (tests/test_gpu_wide_copy.py) checked for teeth."""
import numpy as np
import pytest

import oracle
import streams
import wide_copy as wc
from raytracedshadows_amd import api

END = wc.END
FMAX = float(np.finfo(np.float32).max)
EMPTY = [FMAX, FMAX, FMAX, -FMAX, -FMAX, -FMAX]


def _tris(P):
    """t_i = (i, 0, 0), (i + 1, 0, 0.5), (i, 1 + i, 0.25): v0 = (i, 0, 0), e0 = (1, 0, 0.5), e1 = (0, 1 + i, 0.25)."""
    t = np.zeros((P, 3, 3), np.float32)
    for i in range(P):
        t[i] = [[i, 0, 0], [i + 1, 0, 0.5], [i, 1 + i, 0.25]]
    return t


def box(i, j):
    """The box of triangles i..j: (i, 0, 0) .. (j + 1, j + 1, 0.5)."""
    return [float(i), 0.0, 0.0, float(j + 1), float(j + 1), 0.5]


def rec(i, node, parent_box):
    return [float(i), 0.0, 0.0, 1.0, 0.0, 0.5, 0.0, float(1 + i), 0.25, node] + parent_box


def dwords(*rows):
    """Python floats -> float32 bits, Python ints -> uint32; one flat uint32 array."""
    out = []
    for row in rows:
        for v in row:
            out.append(np.float32(v).view(np.uint32) if isinstance(v, float) else np.uint32(v))
    return np.array(out, np.uint32)


KNOWN = {
    # one wide node: two leaf slots carrying the root's box, two empty slots
    "P2": ((0, 1), 1, [
        box(0, 1) + box(0, 1) + EMPTY + EMPTY + [1, 65, END, END] + [0, 2, END, END],
        rec(0, 1, box(0, 1)), rec(1, 2, box(0, 1)),
        [END, 0, 0]]),
    # ((0, 1), 2): nodes 0 root, 1 inner (odd depth: folded), 2 leaf, 3 leaf, 4 leaf
    "P3_left": (((0, 1), 2), 2, [
        box(0, 1) + box(0, 1) + box(0, 2) + EMPTY + [1, 65, 129, END] + [0, 3, 4, END],
        rec(0, 2, box(0, 1)), rec(1, 3, box(0, 1)), rec(2, 4, box(0, 2)),
        [END, 0, 1, 1, 0]]),
    # (0, (1, 2)): nodes 0 root, 1 leaf, 2 inner, 3 leaf, 4 leaf
    "P3_right": ((0, (1, 2)), 2, [
        box(0, 2) + box(1, 2) + box(1, 2) + EMPTY + [1, 65, 129, END] + [0, 3, 4, END],
        rec(0, 1, box(0, 2)), rec(1, 3, box(1, 2)), rec(2, 4, box(1, 2)),
        [END, 0, 0, 2, 2]]),
    # ((0, 1), (2, 3)): four leaf slots, two boxes
    "complete4": (((0, 1), (2, 3)), 2, [
        box(0, 1) + box(0, 1) + box(2, 3) + box(2, 3) + [1, 65, 129, 193] + [0, 3, 5, 6],
        rec(0, 2, box(0, 1)), rec(1, 3, box(0, 1)), rec(2, 5, box(2, 3)), rec(3, 6, box(2, 3)),
        [END, 0, 1, 1, 0, 4, 4]]),
    # (0, (1, (2, (3, 4)))): nodes 0 root, 1 leaf, 2 inner, 3 leaf, 4 inner (even: wide node 1), 5 leaf, 6 inner, 7, 8 leaves
    "chain5": ((0, (1, (2, (3, 4)))), 3, [
        box(0, 4) + box(1, 4) + box(2, 4) + EMPTY + [1, 65, 128, END] + [0, 3, 4, END],
        box(2, 4) + box(3, 4) + box(3, 4) + EMPTY + [129, 193, 257, END] + [4, 7, 8, END],
        rec(0, 1, box(0, 4)), rec(1, 3, box(1, 4)), rec(2, 5, box(2, 4)), rec(3, 7, box(3, 4)), rec(4, 8, box(3, 4)),
        [END, 0, 0, 2, 2, 4, 4, 6, 6]]),
}


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    tree, levels, rows = KNOWN[name]
    P = len(rows[-1]) // 2 + 1
    packed = streams.stream_from_tree(tree, _tris(P))
    want = dwords(*rows).view(np.uint8)
    rs = wc.restate(packed)
    assert rs["bits"] == 0 and rs["allowed"] and rs["levels"] == levels
    assert rs["wide_nodes"] == sum(1 for r in rows if len(r) == 32)
    assert wc.first_difference(want, rs, P) is None, wc.first_difference(want, rs, P)
    assert np.array_equal(rs["copy"], want)
    # the comparison helper names what differs: one parent-box float of the last triangle record
    bad = want.copy().view(np.uint32)
    bad[rs["wide_nodes"] * 32 + (P - 1) * 16 + 13] ^= 1
    msg = wc.first_difference(bad.view(np.uint8), rs, P)
    assert msg is not None and f"triangle record {P - 1} dword 13" in msg, msg


def test_no_copy_for_one_triangle_and_for_deep_chains():
    one = streams.stream_from_tree(0, _tris(1))
    assert wc.verdict(one) == 0 and not wc.restate(one)["allowed"]
    rs = np.random.RandomState(0)
    for P, levels in ((512, 256), (513, 257), (514, 0)):
        t = (rs.random_sample((P, 1, 3)) * 10 + rs.random_sample((P, 3, 3))).astype(np.float32)
        r = wc.restate(streams.stream_from_tree(wc.chain(P), t))
        assert r["bits"] == 0 and r["levels"] == levels and r["allowed"] == (levels > 0), P
        assert (r["wide_nodes"] > 0) == (levels > 0)


def _soup(n, seed):
    rs = np.random.RandomState(seed)
    c = rs.random_sample((n, 1, 3)) * 30
    return (c + (rs.random_sample((n, 3, 3)) - 0.5) * 2).astype(np.float32)


def _builder_streams():
    t = _soup(3001, 3)
    v, idx = t.reshape(-1, 3), np.arange(3 * 3001, dtype=np.uint32)
    out = {"host_sah": api.BVHBuilder().build(v, 3, idx, 3001).m_packedNodes,
           "host_median": api.BVHBuilder(sah_prim_limit=1).build(v, 3, idx, 3001).m_packedNodes,
           "oracle": oracle.bvh_build(v, 3, idx, 3001),
           "oracle_ties": oracle.bvh_build(v, 3, idx, 3001, ties_by_prim=True),
           "complete1024": streams.stream_from_tree(wc.complete(0, 1024), _soup(1024, 4)),
           "complete777": streams.stream_from_tree(wc.complete(0, 777), _soup(777, 5)),
           "chain300": streams.stream_from_tree(wc.chain(300), _soup(300, 6)),
           "deep_bushy": streams.deep_bushy_stream(25)}
    return out


@pytest.fixture(scope="module")
def builder_streams():
    return _builder_streams()


@pytest.mark.parametrize("name", ["host_sah", "host_median", "oracle", "oracle_ties", "complete1024", "complete777", "chain300",
                                  "deep_bushy"])
def test_structure_of_the_copy(builder_streams, name):
    packed = builder_streams[name]
    _, P, N, nodes = wc._view(packed)
    rs = wc.restate(packed)
    assert rs["bits"] == 0 and rs["allowed"]
    wide, tris, parents, slot = rs["wide"], rs["tris"], rs["parents"], rs["slot_nodes"]
    tag, link = nodes[:, 3], nodes[:, 7].astype(np.int64)
    end = np.where(link == END, N, link)
    leaf = tag != END
    depth = rs["depth"]
    filled = wide[:, 24:28] != END
    # every leaf in exactly one slot, every even-depth inner node but the root in exactly one slot, nothing else in a slot
    used = slot[filled]
    counts = np.bincount(used.astype(np.int64), minlength=N)
    want = (leaf | (depth % 2 == 0)).astype(np.int64)
    want[0] = 0
    assert np.array_equal(counts, want)
    for w in range(wide.shape[0]):
        n = int(wide[w, 28])
        k = int(filled[w].sum())
        assert filled[w, :k].all() and not filled[w, k:].any(), w
        idx = [int(slot[w, j]) for j in range(k)]
        assert idx[0] in (n + 1, n + 2) and list(wide[w, 29:29 + k - 1]) == idx[1:]
        assert all(x == END for x in wide[w, 28 + k:32]) and all(x == END for x in wide[w, 24 + k:28])
        assert idx == sorted(idx) and len(set(idx)) == k
        ranges = idx[1:] + [int(end[n])]
        for j, s in enumerate(idx):
            assert s < int(end[s]) <= ranges[j], (w, j)       # slot j's subtree lies in [idx_j, idx_j+1) (an odd-depth inner
            ref = int(wide[w, 24 + j])
            if ref & 1:
                assert leaf[s] and int(tris[(ref - 1) // 64, 9]) == s
                boxnode = int(parents[s])
            else:
                assert not leaf[s] and ref % 128 == 0 and int(wide[ref // 128, 28]) == s
                boxnode = s
            assert list(wide[w, 6 * j:6 * j + 6]) == list(nodes[boxnode, [0, 1, 2, 4, 5, 6]]), (w, j)
        assert int(end[idx[-1]]) == int(end[n]), w            # node may lie between); the last one ends at n's miss link
    # triangle records in stream order of the leaves; parents as the tree says
    assert np.array_equal(tris[:, 9], np.flatnonzero(leaf))
    for i in np.flatnonzero(~leaf):
        assert parents[i + 1] == i and parents[int(link[i + 1])] == i
    assert parents[0] == END


def test_restated_verdict_on_builder_streams_is_clean(builder_streams):
    for name, packed in builder_streams.items():
        assert wc.verdict(packed) == 0, name


@pytest.mark.parametrize("case", wc.corpus(), ids=lambda c: c[0])
def test_mutation_corpus_verdict(case):
    name, packed, expected, compared, _ = case
    bits = wc.verdict(packed)
    assert bits & compared == expected, (name, bits, expected)
    try:
        accepted = api.bvh_validate(packed) > 0
    except api.RtsError as e:
        assert e.status == 5, name
        accepted = False
    assert accepted == (not bits & wc.STRUCTURE), name


def test_confirmation_frame_has_teeth():
    """A sizeable share of the frame's rays hit a triangle sticking out of its exact parent box, within 16 ulps of the box's
    face, and are lit: only the confirmation against the parent's box gives them the right answer."""
    s = wc.confirmation_scene()
    counted = wc.confirmation_rays(s)
    assert counted["teeth"] >= 0.03 * counted["rays"], counted
    assert counted["by_depth_parity"][0] > 0 and counted["by_depth_parity"][1] > 0, counted
