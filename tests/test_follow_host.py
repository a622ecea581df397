"""CPU: follow mode's order on the host (rtsh_follow_order), the checker of the device planner (rts_follow.hip).

With xcd_square 0 it is rts_ctx_plan_splits' front order (rtsh_split_front_order) of the same lives; with S > 0 each band is dealt
over the XCDs by the DEAL rule of include/rts.h."""
import numpy as np
import pytest

import follow_cases as fc
from raytracedshadows_amd import api


_tiles = fc.tile_ids
_edge_ticks = fc.edge_ticks_all
_mid_band = fc.mid_band


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
    band = fc.band64(fc.block_lives(ticks, bx, by, B))[order]
    assert (np.diff(band) <= 0).all()                                          # longest first
    want, bands = fc.deal_bands(ticks, bx, by, first, S, B)                    # the independent restatement of rts.h's rule
    assert sum(b["leftovers"] for b in bands) > 0
    assert np.array_equal(order, want)


def test_edge_ticks_the_reference_cannot_place_are_few():
    """Near a half-octave edge the float64 band of the reference and the float32 band of rts.h can differ.  Such ticks take their
    band from rtsh_split_front_order (follow_cases.pin) -- only within 2^-18 of an edge, relatively, which pin() asserts --; one that
    fits neither its float64 band nor a neighbour is dropped."""
    kept, dropped, pinned = fc.edge_ticks()
    total = fc.edge_ticks_all().size
    print(f"edge ticks: {total}, band taken from the split planner: {pinned}, dropped: {dropped}")
    assert kept.size + dropped == total
    assert dropped <= 0.01 * total
    big = fc.edge_ticks_all()[np.isin(fc.edge_ticks_all(), fc._pin_ticks)].astype(np.float64)
    x = np.log2(big * 0.01) * 2                                                # (pin() asserts the same of every tick it records)
    assert (np.abs(x - np.round(x)) / 2 * np.log(2) < 2.0 ** -18).all(), "pinned only within float32's doubt of an edge"
    assert (big > 2e6).all()                                                   # (where one tick is less than 2^-20 of the count)


@pytest.mark.parametrize("dist", fc.DISTRIBUTIONS)
def test_distribution_reaches_what_it_is_for(dist):
    """Computed from deal_reference's band statistics alone."""
    for (bx, by), (S, B) in fc.REACH_AT[dist]:
        assert fc.reaches(dist, bx, by, S, B), (dist, bx, by, S, B)


# No (geometry, distribution) pair is skipped: the numpy restatement takes 0.1 s on (257, 259), the largest.
@pytest.mark.parametrize("dist", fc.DISTRIBUTIONS)
@pytest.mark.parametrize("dims", fc.GEOMETRIES, ids=lambda d: f"{d[0]}x{d[1]}")
def test_twin_equals_the_reference_on_chosen_lives(dims, dist):
    bx, by = dims
    for S, B in fc.SETTINGS:
        ticks, _ = fc.lives(dist, bx, by, S, B)
        for first in (0, 5):
            got = api.follow_order(ticks, bx, by, first_record=first, xcd_square=S, life_block=B)
            want = fc.deal_reference(ticks, bx, by, first, S, B)
            assert np.array_equal(got, want), (S, B, first, int(np.flatnonzero(got != want)[0]))


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
