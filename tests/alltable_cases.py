"""Shared by tests/test_alltable_cases_host.py and tests/test_gpu_alltable_edges.py (the ALLTABLE instantiation of the wide packet
kernel): the frames, the lights and the expected masks.  No GPU is needed to import or to use any of it.

Every expected mask is oracle.shadow_mask over the packed stream that is installed, the light of the trace and the positions that
are uploaded: the committed CPU oracle, compared byte for byte.  Every trace writes into a mask preset to FILL; rows outside a
traced range must hold FILL afterwards (rows_of).

Frames, made once per process and read-only:
  cornell 72 x 40 and 67 x 45     several blocks; ragged (edge lanes without a pixel, 9 x 6 tiles with a partial column and row)
  city 96 x 64                    a frame with sky: tiles of background texels only, tiles that mix background and surface, covered tiles
  cornell 2064 x 8 and 8 x 2064   258 tiles along one axis: bx (then by) above 255 in the 16-bit halves of a record, and 258 records --
                                  no multiple of 8, so the last slots (id & 7) * frontStride + (id >> 3) of the XCD-major map are uneven
each under the scene's point light and under the directional light of the constants (workloads.prepare / workloads.relight)."""
import numpy as np

import oracle
from raytracedshadows_amd import api, scenes, workloads

FILL = 77
WHOLE = dict(min_life_us=1e9, piece_us=1e9, front_share=1.0)      # no tile is long enough to split, every tile is a front record
LIGHTS = ("point", "directional")
CORNELL = [("cornell", 72, 40), ("cornell", 67, 45)]
SKY = ("city", 96, 64)
LONG = [("cornell", 2064, 8), ("cornell", 8, 2064)]
FRAMES = CORNELL + [SKY] + LONG
BAD_VALUES = (np.float32(0.0), np.float32(1e-40), np.float32(1e38))   # texels the one-gate ray set-up refuses: 0, a denormal, huge
# 3e7 lies in [2^24, 2^25) and 7e7 in [2^26, 2^27): roots that cross powers of two on x (tests/test_gpu_alltable.py)
ROOTS = (3e7, 7e7)

_BASE, _LIT = {}, {}


def frame_id(f):
    return f"{f[0]}-{f[1]}x{f[2]}"


def tiles_of(W, H):
    return (W + 7) // 8, (H + 7) // 8


def want(wl, packed=None, positions=None, light="own"):
    """The oracle's mask of `wl` (or of another stream, other positions, another light of it)."""
    lt = wl.light if isinstance(light, str) else light
    mask, _, _ = oracle.shadow_mask(wl.packed if packed is None else packed, wl.constants.as_array(), oracle.light_from_product(lt, wl.constants),
                                    wl.positions if positions is None else positions, wl.W, wl.H)
    return mask


def frame(f, light="point"):
    """The workload of frame f = (scene, W, H) under `light`, with .want (the oracle's mask); arrays read-only."""
    if f not in _BASE:
        wl = workloads.prepare(f[0], f[1], f[2], via_obj=False)
        for a in (wl.positions, wl.packed, wl.vertices):
            a.setflags(write=False)
        _BASE[f] = wl
    if (f, light) not in _LIT:
        wl = workloads.relight(_BASE[f], light)
        assert (wl.light is None) == (light == "directional")          # (the reference's directional light travels as "no light")
        wl.want = want(wl)
        wl.want.setflags(write=False)
        _LIT[(f, light)] = wl
    return _LIT[(f, light)]


def soft_light(wl, light, nsamples=4):
    """`nsamples` samples of the frame's light (a dispatch no table applies to)."""
    sc = wl.scene
    if light == "directional":
        return api.Light.make(api.Light.DIRECTIONAL, sc.light_direction, scenes.jitter_offsets(nsamples, 0.05))
    r = 0.01 * float(np.linalg.norm(sc.bbox_max - sc.bbox_min))
    return api.Light.make(api.Light.POINT, sc.light_point, scenes.jitter_offsets(nsamples, r), nsamples=nsamples)


def background(positions):
    """bool[H, W]: texels the primary pass left as background (w == 0; a surface texel has w == 1)."""
    return positions[..., 3] == 0


def tile_census(positions):
    """int[tiles y, tiles x]: background texels per 8 x 8 tile, and the texels each tile has (partial edge tiles have fewer than 64)."""
    H, W = positions.shape[:2]
    bx, by = tiles_of(W, H)
    bg = np.zeros((by * 8, bx * 8), np.int64)
    own = np.zeros((by * 8, bx * 8), np.int64)
    bg[:H, :W] = background(positions)
    own[:H, :W] = 1
    fold = lambda a: a.reshape(by, 8, bx, 8).sum(axis=(1, 3))
    return fold(bg), fold(own)


def sky_tiles(positions):
    """(tiles of background only, tiles that mix background and surface, tiles fully covered), each int[k, 2] of (ty, tx)."""
    bg, own = tile_census(positions)
    return np.argwhere(bg == own), np.argwhere((bg > 0) & (bg < own)), np.argwhere(bg == 0)


def assert_sky(positions):
    """The point of the sky frame: at least one tile of each kind."""
    sky, mixed, covered = sky_tiles(positions)
    assert len(sky) >= 1 and len(mixed) >= 1 and len(covered) >= 1, (len(sky), len(mixed), len(covered))
    return sky, mixed, covered


def rows_of(mask, row_begin, row_end):
    """What a trace of rows [row_begin, row_end) leaves in a mask preset to FILL."""
    out = np.full_like(mask, FILL)
    out[row_begin:row_end] = mask[row_begin:row_end]
    return out


def row_ranges(H):
    """(row_begin, row_end) of the range tests: both ends inside tiles; from a tile boundary to inside a tile; one row."""
    return [(13, H - 5), (8, H - 3), (H // 2 + 1, H // 2 + 2)]


def bad_texels(wl, where):
    """A copy of the positions with one refused value at each (y, x) of `where`, the values taken in turn."""
    pos = wl.positions.copy()
    for n, (y, x) in enumerate(where):
        pos[y, x, :3] = BAD_VALUES[n % 3]
    return pos


def one_per_tile(W, H):
    """(y, x) of one texel in every tile (3 rows down, 5 across, clamped into the frame: partial edge tiles have one too)."""
    return [(min(ty + 3, H - 1), min(tx + 5, W - 1)) for ty in range(0, H, 8) for tx in range(0, W, 8)]


def moved(wl, x):
    """The scene's vertices with the one of largest x moved out to x: the root box's upper x bound becomes x."""
    w = wl.vertices.copy()
    w[int(np.argmax(w[:, 0])), 0] = np.float32(x)
    return w


def all_table_rule(blocks_x, blocks_y, records, piece_rows, table=True, has_pieces=False, all_in_table=True, front_map=True, waves_per_block=1,
                   nsamples=1, wide_lane=False, follow=False, stripes=False, wave_stats=False, scene_bounds=True):
    """allTableRule of raytracedshadows_amd/csrc/rts_alltable.h restated from its text, for the tests that state a launch's facts.
    (tests/test_alltable_host.py checks the header itself against its truth table.)  blocks_y is no term of it."""
    return (waves_per_block == 1 and nsamples == 1 and not wide_lane and not follow and table and not has_pieces and all_in_table and front_map
            and not stripes and not wave_stats and scene_bounds and piece_rows != 0 and blocks_x * piece_rows == records)
