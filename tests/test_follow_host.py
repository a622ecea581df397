"""CPU: follow mode's order on the host (rtsh_follow_order), the checker of the device planner (rts_follow.hip).

With xcd_square 0 it is rts_ctx_plan_splits' front order (rtsh_split_front_order) of the same lives; with S > 0 each band is dealt
over the XCDs by the DEAL rule of include/rts.h."""
import numpy as np
import pytest

from raytracedshadows_amd import api


def _tiles(bx, by):
    t = np.arange(bx * by, dtype=np.uint32)
    return (t % bx) | ((t // bx) << 16)


def _edge_ticks():
    """Tick counts at every half-octave edge of life (0.25 us .. 2^25 us) and around it."""
    out = [0, 1, 2, 24, 25, 26]
    for b in range(-4, 51):
        e = int(round(2.0 ** (b / 2.0) * 100.0))
        out += [e + d for d in (-2, -1, 0, 1, 2) if 0 <= e + d < 2 ** 32]
    return np.array(out, np.uint64).astype(np.uint32)


def _mid_band(b):
    return int(round(2.0 ** (b / 2.0 + 0.25) * 100.0))          # well inside band b: its band is not in doubt


def _band(ticks):
    return np.floor(np.log2(np.maximum(ticks.astype(np.float64) * 0.01, 0.25)) * 2).astype(np.int64)


def _xcd(t, bx, S):
    return ((t % bx) // S + (t // bx) // S * 3) & 7


@pytest.mark.parametrize("B", [1, 2, 8])
@pytest.mark.parametrize("dims", [(37, 23), (1, 50), (64, 1), (9, 17), (240, 135)])
def test_without_deal_equals_the_split_front_order(B, dims):
    bx, by = dims
    rng = np.random.default_rng(bx * 1000 + by + B)
    edges = _edge_ticks()
    ticks = np.where(rng.random(bx * by) < 0.5, rng.choice(edges, bx * by), rng.integers(0, 2 ** 32, bx * by, dtype=np.uint64)).astype(np.uint32)
    ticks[rng.random(bx * by) < 0.3] = rng.integers(0, 5000, 1)[0]
    for first in (0, 5):
        got = api.follow_order(ticks, bx, by, first_record=first, xcd_square=0, life_block=B)
        want = api.split_front_order(ticks.astype(np.float32) * np.float32(0.01), _tiles(bx, by), first, 0, B)
        assert np.array_equal(got, want)


def test_every_edge_tick_sorts_as_the_split_planner_does():
    edges = _edge_ticks()
    n = edges.size
    got = api.follow_order(edges[::-1].copy(), n, 1)
    want = api.split_front_order(edges[::-1].astype(np.float32) * np.float32(0.01), _tiles(n, 1))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("S,B,first", [(1, 1, 0), (2, 1, 3), (4, 2, 7), (32, 1, 0), (3, 4, 13)])
def test_deal_rule(S, B, first):
    bx, by = 45, 31
    rng = np.random.default_rng(S * 100 + B + first)
    ticks = np.array([_mid_band(b) for b in rng.choice([2, 3, 7, 12, 20], bx * by, p=[0.5, 0.2, 0.15, 0.1, 0.05])], np.uint32)
    order = api.follow_order(ticks, bx, by, first_record=first, xcd_square=S, life_block=B)
    n = bx * by
    assert sorted(order.tolist()) == list(range(n))                            # a permutation
    life = ticks.copy()
    if B > 1:                                                                  # (a tile as long as the longest of its block)
        t = np.arange(n)
        blk = (t // bx) // B * ((bx + B - 1) // B) + (t % bx) // B
        m = np.zeros(blk.max() + 1, np.uint64)
        np.maximum.at(m, blk, ticks.astype(np.uint64))
        life = m[blk].astype(np.uint32)
    band = _band(life)[order]
    assert (np.diff(band) <= 0).all()                                          # longest first
    i = 0
    while i < n:
        j = i
        while j < n and band[j] == band[i]:
            j += 1
        R, L = first + i, j - i
        seg = order[i:j]
        own = {y: sorted(t for t in seg.tolist() if _xcd(t, bx, S) == y) for y in range(8)}
        placed, left = [None] * L, []
        for y in range(8):
            off = (y - R) & 7
            slots = (L - 1 - off) // 8 + 1 if L > off else 0
            for k, t in enumerate(own[y]):
                if k < slots:
                    placed[off + 8 * k] = t                                     # record r from XCD (first + r) mod 8 while it has tiles
                else:
                    left.append(t)                                              # leftovers: XCD order, then image order ...
        it = iter(left)
        placed = [p if p is not None else next(it) for p in placed]             # ... into the vacant positions, in increasing order
        assert placed == seg.tolist(), f"band at record {R}"
        i = j


def test_deal_equals_the_split_front_order_when_no_xcd_runs_out():
    bx, by = 8, 8                                                               # S 1: every row holds each XCD once
    ticks = np.array([_mid_band(9) if y < 4 else _mid_band(3) for y in range(by) for _ in range(bx)], np.uint32)
    for first in (0, 8, 16):
        got = api.follow_order(ticks, bx, by, first_record=first, xcd_square=1)
        want = api.split_front_order(ticks.astype(np.float32) * np.float32(0.01), _tiles(bx, by), first, 1, 0)
        assert np.array_equal(got, want)


def test_arguments():
    ticks = np.ones(12, np.uint32)
    with pytest.raises(api.RtsError):
        api.follow_order(ticks, 4, 3, life_block=65)
    with pytest.raises(api.RtsError):
        api.follow_order(ticks, 4, 3, xcd_square=65536)
    with pytest.raises(api.RtsError):
        api.follow_order(ticks, 5, 3)
    assert sorted(api.follow_order(ticks, 4, 3, life_block=64, xcd_square=65535).tolist()) == list(range(12))
