"""Follow mode's planner: the independent restatement of its order and the chosen lives it is tested on (plain numpy, no device).

deal_reference() restates include/rts.h's bands and DEAL rule without looking at the library's planner code; the CPU tests hold
the host twin (rtsh_follow_order) against it, the GPU tests hold the device planner (rtsh_follow_plan_device) against the twin,
both on every (geometry, setting, distribution) triple listed here.  Every distribution says what it is for with a predicate
over deal_reference's own band statistics (REACH), asserted at the triples of REACH_AT -- never from the code under test.

The band of a life is float64 floor(log2(max(ticks * 0.01, 0.25)) * 2).  The library's rule is the float32 one of rts.h
("ticks * 0.01f us"), and within a few float32 roundings of a half-octave edge the two can disagree (from 2.3 million ticks
up a neighbouring tick is that close; above 2^24 a float32 cannot even tell the ticks around an edge apart).  pin() finds those ticks with rtsh_split_front_order -- the split planner, which the planner under test
does not call -- by sorting each tick between two tiles from the middle of a band, and records the band the split planner
gives them; deal_reference() then takes a pinned tick's band from that table.  A tick that cannot be pinned to its float64 band
or a neighbour of it is dropped by the generators and counted (edge_ticks())."""
import numpy as np

from raytracedshadows_amd import api

GEOMETRIES = [(1, 1), (7, 1), (1, 9), (8, 1), (3, 3), (9, 17), (64, 16), (41, 25), (1, 1500), (2000, 1), (240, 135), (257, 259)]
SETTINGS = [(0, 1), (1, 1), (2, 1), (3, 2), (5, 3), (32, 8), (32, 1), (0, 64), (65535, 1), (4, 64), (1, 64)]
DISTRIBUTIONS = ["equal", "zeros", "ones", "edges", "wrap", "one_xcd_long", "one_xcd_short", "two_xcds", "one_per_band",
                 "chunk_one_key", "mix"]
BAND_LOW, BAND_HIGH = -4, 50                           # 55 bands: 0.25 us and less .. 2^32 - 1 ticks
CHUNK = 1024                                           # tiles per workgroup of the device's rank pass


def tile_ids(bx, by):
    t = np.arange(bx * by, dtype=np.uint32)
    return (t % bx) | ((t // bx) << 16)


def edge_ticks_all():
    """Tick counts at every half-octave edge of life (0.25 us .. 2^25 us) and around it."""
    out = [0, 1, 2, 24, 25, 26]
    for b in range(-4, 51):
        e = int(round(2.0 ** (b / 2.0) * 100.0))
        out += [e + d for d in (-2, -1, 0, 1, 2) if 0 <= e + d < 2 ** 32]
    return np.array(out, np.uint64).astype(np.uint32)


def mid_band(b):
    return int(round(2.0 ** (b / 2.0 + 0.25) * 100.0))          # well inside band b: its band is not in doubt


def band64(ticks):
    return np.floor(np.log2(np.maximum(np.asarray(ticks).astype(np.float64) * 0.01, 0.25)) * 2).astype(np.int64)


def xcd_of(t, bx, S):
    return ((t % bx) // S + (t // bx) // S * 3) & 7


# ---- ticks whose band float32 and float64 disagree about -------------------------------------------------------------------------
_checked = np.zeros(0, np.uint32)                      # sorted: ticks pin() has seen
_pin_ticks = np.zeros(0, np.uint32)                    # sorted: ticks whose band is not band64's ...
_pin_bands = np.zeros(0, np.int64)                     # ... and the band rtsh_split_front_order sorts them into
_unpinnable = np.zeros(0, np.uint32)                   # neither band64 nor a neighbour: dropped by the generators


def _sorts_into(ticks, bands):
    """True where the split planner sorts tick[i] between two tiles from the middle of bands[i] that enclose it in image order
    (band, longest first, then image order: the three stay adjacent exactly when they share a band)."""
    n = ticks.size
    life = np.empty(3 * n, np.float32)
    anchor = np.array([mid_band(int(b)) for b in bands], np.float64).astype(np.float32) * np.float32(0.01)
    life[0::3] = anchor
    life[1::3] = ticks.astype(np.float32) * np.float32(0.01)
    life[2::3] = anchor
    t = np.arange(3 * n, dtype=np.uint32)
    order = api.split_front_order(life, (t & 0xFFFF) | ((t >> 16) << 16))
    pos = np.empty(3 * n, np.int64)
    pos[order] = np.arange(3 * n)
    return (pos[1::3] == pos[0::3] + 1) & (pos[2::3] == pos[0::3] + 2)


def pin(ticks):
    """Checks every tick not seen before against the split planner and records the ones band64 gets wrong."""
    global _checked, _pin_ticks, _pin_bands, _unpinnable
    new = np.setdiff1d(np.unique(np.asarray(ticks, np.uint32)), _checked)
    if not new.size:
        return
    b = band64(new)
    doubt = new[~_sorts_into(new, b)]
    found_t, found_b, lost = [], [], []
    if doubt.size:
        b = band64(doubt)
        lower = np.zeros(doubt.size, bool)
        upper = np.zeros(doubt.size, bool)
        can = b - 1 >= BAND_LOW
        lower[can] = _sorts_into(doubt[can], b[can] - 1)
        can = b + 1 <= BAND_HIGH
        upper[can] = _sorts_into(doubt[can], b[can] + 1)
        for t, bb, lo, up in zip(doubt.tolist(), b.tolist(), lower.tolist(), upper.tolist()):
            if lo != up:
                found_t.append(t)
                found_b.append(bb - 1 if lo else bb + 1)
            else:
                lost.append(t)
    # A pinned band is believed only where float32 can be in doubt, so that band64 stays the check everywhere else: (float)ticks, 0.01f
    # and their product are each within 2^-24 of exact, relatively, and log2f's result -- below 32, one ulp 2^-19 -- within 1.5 ulp,
    # i.e. ticks within 1.5 * 2^-19 * ln 2 = 2.0e-6: together less than 2^-18 of an edge.  A wrong lifeBand would be a band off far from it.
    if found_t:
        x = np.log2(np.array(found_t, np.float64) * 0.01) * 2
        off = np.abs(x - np.round(x)) / 2 * np.log(2)                          # relative distance to the nearest half-octave edge
        assert (off < 2.0 ** -18).all(), ("the split planner disagrees with float64 far from an edge", found_t, off.max())
    keys = np.concatenate([_pin_ticks, np.array(found_t, np.uint32)])
    vals = np.concatenate([_pin_bands, np.array(found_b, np.int64)])
    at = np.argsort(keys)
    _pin_ticks, _pin_bands = keys[at], vals[at]
    _unpinnable = np.union1d(_unpinnable, np.array(lost, np.uint32))
    _checked = np.union1d(_checked, new)


def pinned_count():
    return int(_pin_ticks.size)


def band_of(life):
    """band64, except for the ticks pin() recorded."""
    life = np.asarray(life, np.uint32)
    b = band64(life)
    if _pin_ticks.size:
        at = np.minimum(np.searchsorted(_pin_ticks, life), _pin_ticks.size - 1)
        hit = _pin_ticks[at] == life
        b[hit] = _pin_bands[at[hit]]
    return b


def edge_ticks():
    """(the edge ticks the reference can place, how many were dropped, how many took their band from the split planner)"""
    e = edge_ticks_all()
    pin(e)
    keep = ~np.isin(e, _unpinnable)
    return e[keep], int((~keep).sum()), int(np.isin(e, _pin_ticks).sum())


def _placeable(ticks, instead=0):
    """The ticks with those the reference cannot place replaced (a random tick on an edge both ways: none in the seeds used)."""
    pin(ticks)
    return np.where(np.isin(ticks, _unpinnable), np.uint32(instead), ticks).astype(np.uint32)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def block_lives(ticks, bx, by, B):
    """life_block: a tile as long as the longest of its B x B block."""
    ticks = np.asarray(ticks, np.uint32)
    if B <= 1:
        return ticks.copy()
    t = np.arange(bx * by)
    blk = (t // bx) // B * ((bx + B - 1) // B) + (t % bx) // B
    m = np.zeros(int(blk.max()) + 1, np.uint64)
    np.maximum.at(m, blk, ticks.astype(np.uint64))
    return m[blk].astype(np.uint32)


def deal_bands(ticks, bx, by, first, S, B):
    """(order, bands): the whole order, and per band -- longest first -- a dict of its band number b, first record R, length L, the
    tiles per XCD c[8], each XCD's positions m[8] and the number of leftovers."""
    n = bx * by
    band = band_of(block_lives(ticks, bx, by, B))
    order = np.argsort(-band, kind="stable")                                   # longest first, image order inside a band
    sb = band[order]
    cuts = np.concatenate([[0], np.flatnonzero(np.diff(sb)) + 1, [n]])
    out = order.copy()
    stats = []
    for i, j in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
        R, L = first + i, j - i
        seg = order[i:j]
        x = xcd_of(seg, bx, S) if S else np.zeros(L, np.int64)
        placed = np.full(L, -1, np.int64)
        left, c, m = [], [], []
        for y in range(8):
            own = seg[x == y]
            off = (y - R) & 7
            slots = (L - 1 - off) // 8 + 1 if L > off else 0
            k = min(own.size, slots)
            placed[off + 8 * np.arange(k)] = own[:k]                           # record r from XCD (first + r) mod 8 while it has tiles
            left.append(own[k:])                                               # leftovers: XCD order, then image order ...
            c.append(int(own.size))
            m.append(slots)
        left = np.concatenate(left)
        placed[placed < 0] = left                                              # ... into the vacant positions, in increasing order
        if S:
            out[i:j] = placed
        stats.append({"b": int(sb[i]), "R": R, "L": L, "c": c, "m": m, "leftovers": int(left.size) if S else 0})
    return out.astype(np.uint32), stats


def deal_reference(ticks, bx, by, first, S, B):
    """rts.h's order of follow mode: half-octave bands of (block) life, longest first, row-major inside a band; with S > 0 each
    band dealt by the DEAL rule.  order[r] = tile id of record first + r."""
    return deal_bands(ticks, bx, by, first, S, B)[0]


# ---- the lives --------------------------------------------------------------------------------------------------------------------
def _mix(bx, by, seed):
    """The random mix of test_without_deal_equals_the_split_front_order."""
    n = bx * by
    rng = np.random.default_rng(seed)
    edges = edge_ticks()[0]
    ticks = np.where(rng.random(n) < 0.5, rng.choice(edges, n), rng.integers(0, 2 ** 32, n, dtype=np.uint64)).astype(np.uint32)
    ticks[rng.random(n) < 0.3] = rng.integers(0, 5000, 1)[0]
    return _placeable(ticks)


_LIVES = {}


def lives(dist, bx, by, S, B):
    """(life_ticks, start_ticks or None) of one triple; cached, and never written to."""
    key = (dist, bx, by, S, B)
    if key not in _LIVES:
        ticks, start = _make(dist, bx, by, S, B)
        ticks.setflags(write=False)
        _LIVES[key] = (ticks, start)
    return _LIVES[key]


def _make(dist, bx, by, S, B):
    n = bx * by
    t = np.arange(n, dtype=np.int64)
    Sx = S if S else 1                                                         # (the pattern of the XCD cases without a deal: S = 1)
    x = xcd_of(t, bx, Sx)
    long_, short = mid_band(20), mid_band(2)
    if dist == "equal":
        return np.full(n, mid_band(9), np.uint32), None
    if dist == "zeros":
        return np.zeros(n, np.uint32), None
    if dist == "ones":
        return np.full(n, 0xFFFFFFFF, np.uint32), None
    if dist == "edges":
        return np.resize(edge_ticks()[0], n).astype(np.uint32), None
    if dist == "wrap":                                                         # stamps that wrap: the end below the start
        return _mix(bx, by, 7 + bx * 1000 + by), ((0xFFFFFF00 + t) & 0xFFFFFFFF).astype(np.uint32)
    if dist == "one_xcd_long":
        return np.where(x == 0, long_, short).astype(np.uint32), None
    if dist == "one_xcd_short":
        return np.where(x == 0, short, long_).astype(np.uint32), None
    if dist == "two_xcds":                                                     # the squares of XCD 2 and 5 long: a lattice of S-squares
        return np.where((x == 2) | (x == 5), long_, short).astype(np.uint32), None
    if dist == "one_per_band":
        ticks = np.full(n, mid_band(BAND_LOW), np.uint32)
        gx, gy = (bx + B - 1) // B, (by + B - 1) // B
        k = np.arange(min(55, n))
        if B > 1 and gx * gy >= 55:                                            # one block per band: the tile in the block's corner
            at = (k // gx) * B * bx + (k % gx) * B
        else:
            at = k
        ticks[at] = [mid_band(BAND_LOW + int(i)) for i in k]
        return ticks, None
    if dist == "chunk_one_key":
        ticks = _mix(bx, by, 11 + bx * 1000 + by).copy()
        c = 1 if n >= 2 * CHUNK else 0
        ticks[c * CHUNK:(c + 1) * CHUNK] = mid_band(12)
        return ticks, None
    if dist == "mix":
        return _mix(bx, by, bx * 1000 + by), None
    raise KeyError(dist)


# ---- what each distribution is for ------------------------------------------------------------------------------------------------
def _leftovers(s):
    return sum(b["leftovers"] for b in s)


def _one_key_chunk(ticks, bx, by, S, B):
    """A whole chunk of the rank pass in which every tile has the same band and the same XCD."""
    n = bx * by
    band = band_of(block_lives(ticks, bx, by, B))
    x = xcd_of(np.arange(n), bx, S) if S else np.zeros(n, np.int64)
    key = band * 8 + x
    return any(np.unique(key[c:c + CHUNK]).size == 1 for c in range(0, n - CHUNK + 1, CHUNK))


REACH = {
    "equal": lambda s, *a: len(s) == 1 and _leftovers(s) > 0 and s[0]["c"][0] == s[0]["L"],
    "zeros": lambda s, *a: len(s) == 1 and s[0]["b"] == BAND_LOW,
    "ones": lambda s, *a: len(s) == 1 and s[0]["b"] == BAND_HIGH,
    "edges": lambda s, *a: len(s) == 55,
    "wrap": lambda s, ticks, start, *a: 2 * int(((start.astype(np.uint64) + ticks) >= 2 ** 32).sum()) > ticks.size,
    "one_xcd_long": lambda s, *a: any(max(c) > 2 * m and m > 0 for b in s for c, m in [(b["c"], b["m"][int(np.argmax(b["c"]))])]),
    "one_xcd_short": lambda s, *a: any(max(c) > 2 * m and m > 0 for b in s for c, m in [(b["c"], b["m"][int(np.argmax(b["c"]))])]),
    "two_xcds": lambda s, *a: any(sum(1 for v in b["c"] if v == 0) >= 3 and sum(1 for v in b["c"] if v) == 2 and b["leftovers"] > 0
                                  for b in s),
    "one_per_band": lambda s, *a: len(s) == 55 and sum(1 for b in s if b["L"] < 8) >= 50,
    "chunk_one_key": lambda s, ticks, start, bx, by, S, B: _one_key_chunk(ticks, bx, by, S, B),
    "mix": lambda s, *a: len(s) >= 10 and (a[4] == 0 or _leftovers(s) > 0),
}

# (geometry, setting) at which each distribution must reach what it is for
REACH_AT = {
    "equal": [((9, 17), (32, 1)), ((64, 16), (65535, 1)), ((41, 25), (65535, 1)), ((240, 135), (65535, 1)), ((3, 3), (5, 3))],
    "zeros": [((9, 17), (3, 2)), ((257, 259), (32, 8))],
    "ones": [((9, 17), (3, 2)), ((257, 259), (32, 8))],
    "edges": [((41, 25), (0, 1)), ((41, 25), (1, 1)), ((240, 135), (32, 1)), ((257, 259), (2, 1))],
    "wrap": [((7, 1), (1, 1)), ((9, 17), (2, 1)), ((3, 3), (0, 1))],
    "one_xcd_long": [((9, 17), (1, 1)), ((64, 16), (2, 1)), ((240, 135), (32, 1)), ((257, 259), (32, 8)), ((2000, 1), (5, 3))],
    "one_xcd_short": [((9, 17), (1, 1)), ((64, 16), (2, 1)), ((240, 135), (32, 1)), ((257, 259), (32, 8)), ((2000, 1), (5, 3))],
    "two_xcds": [((9, 17), (1, 1)), ((64, 16), (2, 1)), ((41, 25), (1, 1)), ((240, 135), (32, 1)), ((257, 259), (32, 8))],
    "one_per_band": [((64, 16), (1, 1)), ((41, 25), (2, 1)), ((1, 1500), (32, 1)), ((240, 135), (3, 2)), ((257, 259), (1, 1)),
                     ((2000, 1), (0, 1))],
    "chunk_one_key": [((64, 16), (0, 1)), ((41, 25), (65535, 1)), ((240, 135), (0, 1)), ((257, 259), (65535, 1)), ((2000, 1), (0, 1))],
    "mix": [((9, 17), (1, 1)), ((240, 135), (32, 1)), ((257, 259), (0, 1)), ((257, 259), (2, 1))],
}


def reaches(dist, bx, by, S, B):
    ticks, start = lives(dist, bx, by, S, B)
    _, stats = deal_bands(ticks, bx, by, 0, S, B)
    return bool(REACH[dist](stats, ticks, start, bx, by, S, B))
