"""CPU: the conditions the cases of tests/alltable_cases.py exist for (the GPU tests of the ALLTABLE instantiations build on them), so
that no case silently loses its point: the sky frame's three kinds of tile, the long frames' tile counts, the row ranges' ends, the
lights, the refused texels' places, and the restated selection rule against the header's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import alltable_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_sky_frame_has_sky_mixed_and_covered_tiles():
    wl = ac.frame(ac.SKY, "point")
    sky, mixed, covered = ac.assert_sky(wl.positions)
    bg = ac.background(wl.positions)
    assert (wl.positions[bg][:, :3] == 0).all()                              # a background texel is (0, 0, 0, 0)
    assert set(np.unique(wl.positions[..., 3]).tolist()) == {0.0, 1.0}
    bx, by = ac.tiles_of(wl.W, wl.H)
    assert len(sky) + len(mixed) + len(covered) == bx * by
    for light in ac.LIGHTS:                                                  # (and its masks are no constants)
        want = ac.frame(ac.SKY, light).want
        assert 0 < int(want[~bg].sum()) < int((~bg).sum()), light


@pytest.mark.parametrize("f", ac.CORNELL + ac.LONG, ids=ac.frame_id)
def test_the_cornell_frames(f):
    _, W, H = f
    bx, by = ac.tiles_of(W, H)
    if f in ac.LONG:
        assert max(bx, by) == 258 and min(bx, by) == 1 and (bx * by) % 8 != 0          # a coordinate above 255; records no multiple of 8
    if f == ac.CORNELL[1]:
        assert W % 8 and H % 8 and bx > 1 and by > 1                                   # ragged both ways, several blocks
    point, directional = ac.frame(f, "point"), ac.frame(f, "directional")
    assert point.light is not None and directional.light is None
    assert point.positions is directional.positions                                    # one G-buffer under both lights
    for wl in (point, directional):
        assert wl.want.shape == (H, W) and set(np.unique(wl.want).tolist()) == {0, 1}  # lit and shadowed texels in each
    assert not np.array_equal(point.want, directional.want)


@pytest.mark.parametrize("f", ac.CORNELL, ids=ac.frame_id)
def test_the_row_ranges(f):
    H = f[2]
    (a0, a1), (b0, b1), (c0, c1) = ac.row_ranges(H)
    # (a range's tiles start at its first row: its end is inside a tile when its length is no multiple of 8)
    assert a0 % 8 and (a1 - a0) % 8 and (a0, a1) == (13, H - 5)            # starts inside a tile of the frame, ends inside one of its own
    assert b0 % 8 == 0 and (b1 - b0) % 8 and b1 % 8 and b0 > 0             # from a tile boundary to inside a tile
    assert c1 - c0 == 1
    for r0, r1 in ((a0, a1), (b0, b1), (c0, c1)):
        assert 0 < r0 < r1 < H
        out = ac.rows_of(ac.frame(f, "point").want, r0, r1)
        assert (out[:r0] == ac.FILL).all() and (out[r1:] == ac.FILL).all() and (out[r0:r1] != ac.FILL).all()


def test_the_refused_texels():
    wl = ac.frame(ac.CORNELL[1], "point")
    at = ac.one_per_tile(wl.W, wl.H)
    bx, by = ac.tiles_of(wl.W, wl.H)
    assert len({(y // 8, x // 8) for y, x in at}) == bx * by == len(at)
    pos = ac.bad_texels(wl, at)
    assert pos is not wl.positions and (pos[at[1][0], at[1][1], :3] == ac.BAD_VALUES[1]).all()
    assert 0 < float(ac.BAD_VALUES[1]) < np.finfo(np.float32).tiny          # a denormal


def test_soft_lights_count_samples():
    for light in ac.LIGHTS:
        wl = ac.frame(ac.CORNELL[1], light)
        soft = ac.soft_light(wl, light, 4)
        assert soft.nsamples == 4
        want = ac.want(wl, light=soft)
        assert want.max() == 4 and want.min() == 0


def test_the_restated_rule_is_the_headers(tmp_path):
    """all_table_rule against allTableRule (rts_alltable.h through tests/cpp/alltable_host.cpp): every single flag flipped from the
    launch the GPU tests state, and grids that do not hold exactly the records."""
    so = str(tmp_path / "liballtable_host.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "alltable_host.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.alltable_rule.restype = C.c_int
    lib.alltable_rule.argtypes = [C.c_void_p]
    base = dict(blocks_x=9, blocks_y=6, records=54, piece_rows=6)
    flips = [{}, dict(table=False), dict(has_pieces=True), dict(all_in_table=False), dict(front_map=False), dict(waves_per_block=4),
             dict(nsamples=4), dict(wide_lane=True), dict(follow=True), dict(stripes=True), dict(wave_stats=True), dict(scene_bounds=False),
             dict(piece_rows=0), dict(records=53), dict(piece_rows=7), dict(blocks_x=1, blocks_y=258, records=258, piece_rows=258)]
    seen = set()
    for flip in flips:
        kw = dict(dict(table=True, has_pieces=False, all_in_table=True, front_map=True, waves_per_block=1, nsamples=1, wide_lane=False,
                       follow=False, stripes=False, wave_stats=False, scene_bounds=True), **base)
        kw.update(flip)
        # facts of alltable_host.cpp: {wavesPerBlock, nsamples, wideLane, follow, table, hasPieces, allInTable, frontMap, stripes, waveStats,
        # sceneBounds, nPieces, blocksX, pieceRows}
        facts = np.array([kw["waves_per_block"], kw["nsamples"], kw["wide_lane"], kw["follow"], kw["table"], kw["has_pieces"], kw["all_in_table"],
                          kw["front_map"], kw["stripes"], kw["wave_stats"], kw["scene_bounds"], kw["records"], kw["blocks_x"], kw["piece_rows"]],
                         np.uint32)
        mine = ac.all_table_rule(**kw)
        assert bool(lib.alltable_rule(facts.ctypes.data)) == mine, flip
        seen.add(mine)
    assert seen == {True, False}
