"""Shared by the sparse light list tests (include/rts_scene.h: rtsh_compact_light_map*; include/rts.h: rts_trace_*light_list_sparse*;
DESIGN.md 4.33): the numpy restatement of the compaction rule, written from the header's text and from nothing of the library's; the
compaction cases; the golden frames, lists and pixel lists of the sparse traces.

Compaction cases.  Frames: 1 x 1, 7 x 9, 8 x 8, 9 x 8, 17 x 5, 70 x 33 (partial tiles right and below), and 8192 x 8 / 8200 x 8 -- 1024
tiles, exactly what one scan workgroup of the device form handles (SCAN_TILES), and the same frame with one tile more.  Maps: all zero,
all set, bits from `count` up only (an empty list), one marked pixel in the frame's last (partial) tile, random maps of about 1 % and
about 50 % marked pixels.  Capacities: n - 1, n, n + 1 and 1 (those that are positive).  And three frames of many groups of tiles
(MANY_FRAMES: 3, 257 and 1027 groups) with two arithmetic maps each, for the kernel that sums the groups' totals.

Sparse traces.  The bottom-right 48 x 40 of cornell_128 and 40 x 36 of terrain_96 (tests/golden/), lists of 1 and 8 lights -- soft
entries of 2 and 16 samples and hard entries mixed, point and directional --, a map that mixes every bit pattern with whole zero
bytes, and pixel lists made from it."""
import os

import numpy as np

from distance_cases import golden_frame
from raytracedshadows_amd import api, scenes

SCAN_TILES = 1024                                    # rts_scene.h: groups of 1024 tiles
FRAMES = [(1, 1), (7, 9), (8, 8), (9, 8), (17, 5), (70, 33), (8 * SCAN_TILES, 8), (8 * SCAN_TILES + 8, 8)]
MAPS = ["zero", "all", "above_count", "last_tile", "one_percent", "half"]
COUNTS = (1, 3, 8)
FILL = 0xAB


# ----------------------------------------------------------------------------------------------------- the rule, from the header's text
def compact_rule(count, lights_map):
    """The whole list: the marked pixels (a bit below `count` set), tiles of 8 x 8 row-major over the frame, pixels row-major in a tile."""
    H, W = lights_map.shape
    below = (1 << count) - 1
    out = []
    for ty in range((H + 7) // 8):
        for tx in range((W + 7) // 8):
            tile = lights_map[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
            ys, xs = np.nonzero(tile & below)                            # (np.nonzero walks row-major: y ascending, then x)
            out.append((ty * 8 + ys) * W + (tx * 8 + xs))
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)


def compact_rule_fast(count, lights_map):
    """The same list without a Python loop over the tiles (the wide frames): a stable sort of the marked pixels by tile number."""
    H, W = lights_map.shape
    ys, xs = np.nonzero(lights_map & ((1 << count) - 1))
    key = ((ys >> 3) * ((W + 7) // 8) + (xs >> 3)) * 64 + (ys & 7) * 8 + (xs & 7)
    return (ys * W + xs)[np.argsort(key, kind="stable")].astype(np.uint32)


_MAPS = {}


def light_map(kind, wh, count):
    """uint8[H, W], read-only."""
    key = (kind, wh, count)
    if key not in _MAPS:
        W, H = wh
        rs = np.random.RandomState(W * 131 + H * 7 + count)
        below = (1 << count) - 1
        if kind == "zero":
            m = np.zeros((H, W), np.uint8)
        elif kind == "all":
            m = np.full((H, W), 0xFF, np.uint8)
        elif kind == "above_count":
            m = (rs.randint(0, 256, (H, W)) & (0xFF & ~below)).astype(np.uint8)
        elif kind == "last_tile":
            m = np.zeros((H, W), np.uint8)
            m[0, 0] = 0xFF & ~below                                      # (not marked)
            m[H - 1, W - 1] = 1
        else:
            share = 0.01 if kind == "one_percent" else 0.5
            bits = rs.randint(1, 256, (H, W)).astype(np.uint8)
            m = np.where(rs.random_sample((H, W)) < share, bits, bits & np.uint8(0xFF & ~below)).astype(np.uint8)
        m.setflags(write=False)
        _MAPS[key] = m
    return _MAPS[key]


def compaction_cases():
    """(kind, (W, H), count): every frame with every map at 8 lights, and the counts 1 and 3 on the maps where the count matters."""
    out = [(kind, wh, 8) for wh in FRAMES for kind in MAPS if kind != "above_count"]
    out += [(kind, wh, c) for wh in FRAMES for kind in ("above_count", "half") for c in (1, 3)]
    return out


def capacities(n):
    return sorted({c for c in (n - 1, n, n + 1, 1) if c >= 1})


# ---------------------------------------------------------------------------------------------- compaction over many groups of tiles
# The third kernel of the device form sums the groups' totals in ONE workgroup: four totals per lane, 256 lanes, strips of 1024 totals
# with a carry.  On FRAMES (at most two groups) only lane 0 of it ever holds a non-zero value.  These frames give it 3 groups (one
# lane, more than one total in it), 257 groups (512 x 513 tiles: 65 lanes, so two waves of the block scan) and 1027 groups (1025 x 1025
# = 1026 * 1024 + 1 tiles: a second strip, so the carry, and a last group of one tile).  Kept out of compaction_cases(): each frame
# meets its two maps only, at 8 lights.
MANY_FRAMES = [(1024, 136), (4096, 4104), (8200, 8200)]
MANY_GROUPS = {(1024, 136): 3, (4096, 4104): 257, (8200, 8200): 1027}
MANY_MAPS = ["sparse", "full_group"]
MANY_STRIDE = 4099                                   # a prime just above 4096: about one marked pixel per 4096, drifting over the columns


def full_group_of(wh):
    """The group that "full_group" marks whole: a middle one, all of whose tiles lie inside the frame (every MANY_FRAMES side is a
    multiple of 8, so no tile is partial), with a group on either side."""
    return max(1, MANY_GROUPS[wh] // 2)


def _tile_pixel(W, tile, slot):
    """Flat index of slot `slot` (row-major in the tile) of tile `tile` (row-major over the frame)."""
    bx = (W + 7) // 8
    return ((tile // bx) * 8 + (slot >> 3)) * W + (tile % bx) * 8 + (slot & 7)


def many_groups_pinned(wh):
    """Flat indices both maps mark whatever the stride does: the frame's first and last pixel, one pixel in the last tile of group 0,
    one in the first tile of the last group, and -- where the frame has it -- one in the first tile of group 1024 (the second strip)."""
    W, H = wh
    groups = MANY_GROUPS[wh]
    pins = [0, W * H - 1, _tile_pixel(W, SCAN_TILES - 1, 37), _tile_pixel(W, (groups - 1) * SCAN_TILES, 0)]
    if groups > SCAN_TILES:
        pins.append(_tile_pixel(W, SCAN_TILES * SCAN_TILES, 9))
    return pins


def many_groups_map(kind, wh):
    """uint8[H, W], read-only, made by arithmetic alone.  "sparse": every MANY_STRIDE-th pixel and the pinned ones, bytes 1 .. 255.
    "full_group": the same, except that group full_group_of(wh) is marked whole (65 536 entries) and its two neighbours not at all
    (but for a pinned pixel, which only the frame of 3 groups has there)."""
    key = ("many", kind, wh)
    if key not in _MAPS:
        W, H = wh
        assert ((W + 7) // 8) * ((H + 7) // 8) > (MANY_GROUPS[wh] - 1) * SCAN_TILES and W % 8 == 0 and H % 8 == 0
        idx = np.concatenate([np.arange(0, W * H, MANY_STRIDE, dtype=np.int64), np.array(many_groups_pinned(wh), np.int64)])
        flat = np.zeros(W * H, np.uint8)
        flat[idx] = (1 + idx % 255).astype(np.uint8)
        m = flat.reshape(H, W)
        if kind == "full_group":
            bx, g = W // 8, full_group_of(wh)
            group = (((idx // W) >> 3) * bx + ((idx % W) >> 3)) // SCAN_TILES
            pinned = np.isin(idx, many_groups_pinned(wh))                # (3 groups: the pinned pixels stay in the neighbours, all else goes)
            flat[idx[((group == g - 1) | (group == g + 1)) & ~pinned]] = 0
            tiles = np.arange(g * SCAN_TILES, (g + 1) * SCAN_TILES)
            for ty in np.unique(tiles // bx):                            # (a group is a few runs of tiles along tile rows)
                tx = tiles[tiles // bx == ty] % bx
                m[ty * 8:ty * 8 + 8, tx.min() * 8:tx.max() * 8 + 8] = 0x80 | (ty & 0x7F)
        m.setflags(write=False)
        _MAPS[key] = m
    return _MAPS[key]


def group_totals(wh, pixels):
    """Marked pixels per group of SCAN_TILES tiles, from a list of flat indices (what the third kernel sums)."""
    W, H = wh
    p = np.asarray(pixels, np.int64)
    tile = ((p // W) >> 3) * ((W + 7) // 8) + ((p % W) >> 3)
    return np.bincount(tile // SCAN_TILES, minlength=MANY_GROUPS[wh])


# ------------------------------------------------------------------------------------------------------------ the sparse traces' cases
SCENES = [("cornell_128", 48, 40), ("terrain_96", 40, 36)]
TABLE = scenes.jitter_offsets(48, 1.0, 23)
_SCENES = {}


class SparseScene:
    """A golden frame (read-only), its lists and its map."""

    def __init__(self, name, W, H):
        self.name, self.W, self.H = name, W, H
        self.packed, self.k, point, pos = golden_frame(name, W, H)
        self.pos = np.ascontiguousarray(pos)
        self.pos.setflags(write=False)
        P, D = api.Light.POINT, api.Light.DIRECTIONAL
        lp = np.array(list(point.xyz), np.float32)
        ld = np.array(list(self.k.lightDirection)[:3], np.float32)
        span = float(np.abs(self.pos[..., :3]).max()) * 0.05 + 0.05
        shifted = lambda dx, dy, dz: tuple(lp + np.array((dx, dy, dz), np.float32) * np.float32(span * 4))
        tilted = tuple(ld + np.array((0.2, 0.0, -0.1), np.float32))
        self.soft = {
            1: api.SoftLightList.make([(P, tuple(lp), 16, 8, span)], TABLE),
            8: api.SoftLightList.make([(P, tuple(lp)), (D, tuple(ld), 2, 0, 0.05), (P, shifted(1, 0, 0), 16, 30, span), (D, tilted),
                                       (P, shifted(0, 0, 1), 2, 46, span * 2), (D, tilted, 16, 3, 0.1), (P, shifted(-1, 0, -1)),
                                       (P, shifted(0, -1, 0), 2, 20, span)], TABLE),
        }
        self.hard = {c: s.hard_list() for c, s in self.soft.items()}
        y, x = np.mgrid[0:H, 0:W]
        m = ((x * 7 + y * 13 + (x >> 2) * 5 + 1) & 0xFF).astype(np.uint8)
        m[(x + 2 * y) % 7 == 0] = 0
        m[(x * 3 + y) % 5 != 0] &= 0xFE                                   # light 0 thinned out: waves in which one lane carries it
        self.map = np.ascontiguousarray(m)
        self.map.setflags(write=False)

    def marked(self, count, lights_map="own"):
        m = self.map if isinstance(lights_map, str) else lights_map
        return compact_rule(count, m)


def scene(name, W, H):
    if (name, W, H) not in _SCENES:
        _SCENES[(name, W, H)] = SparseScene(name, W, H)
    return _SCENES[(name, W, H)]


def expected(sc, form, count, pixels, lights_map, before):
    """What a sparse trace must leave in planes preset to `before`: api.soft_light_list / api.light_list under the map at every listed
    pair, `before` everywhere else.  Written here from the definition in rts.h, apart from the twin in api.py."""
    W, H, n = sc.W, sc.H, sc.W * sc.H
    listed = np.zeros(n, bool)
    px = np.asarray(pixels, np.uint32)
    listed[px[px < n]] = True
    listed = listed.reshape(H, W)
    on = np.full((H, W), (1 << count) - 1, np.uint8) if lights_map is None else lights_map & ((1 << count) - 1)
    clean = np.where(listed[..., None], sc.pos, np.float32(0)).astype(np.float32)      # unlisted positions are never read
    cut = np.where(listed, on, 0).astype(np.uint8)
    out = before.copy()
    if form == "soft":
        full = api.soft_light_list(sc.packed, sc.k, sc.soft[count], clean, W, H, lights_map=cut)
        for l in range(count):
            sel = ((cut >> l) & 1).astype(bool)
            out[l][sel] = full[l][sel]
    else:
        full = api.light_list(sc.packed, sc.k, sc.hard[count], clean, W, H, lights_map=cut)
        out[:] = (out & ~cut) | (full & cut)
    return out


def trace_lists(sc, count):
    """name -> (pixels uint32[], n given to the trace, capacity): the awkward lists of the GPU tests, from the scene's own map."""
    base = sc.marked(8)                                                  # (for a shorter list some listed pixels carry no light below count)
    rs = np.random.RandomState(5)
    out = {}
    for length in (0, 1, 63, 64, 65, 255, 256, 257):
        assert base.size >= length
        out[f"len{length}"] = (base[:length].copy(), length, max(length, 1))
    out["all"] = (base.copy(), base.size, base.size)
    out["shuffled"] = (rs.permutation(base).astype(np.uint32), base.size, base.size)
    dup = np.concatenate([base[:100], base[:100][::-1], base[100:]]).astype(np.uint32)
    out["duplicates"] = (dup, dup.size, dup.size)
    beyond = base.copy()
    n = sc.W * sc.H
    beyond[::7] = (n + (np.arange(beyond[::7].size, dtype=np.int64) * 0x01000193) % (2 ** 32 - n)).astype(np.uint32)      # all >= W * H
    beyond[0], beyond[3] = n, 0xFFFFFFFF
    out["beyond"] = (beyond, beyond.size, beyond.size)
    flat = sc.map.reshape(-1)
    without, with0 = base[(flat[base] & 1) == 0], base[(flat[base] & 1) == 1]
    assert without.size >= 127 and with0.size >= 1
    one = without[:127].copy()
    one[81] = with0[0]                                                   # the second wave: one lane alone carries light 0
    out["one_lane"] = (one, one.size, one.size)
    out["n_above_capacity"] = (base.copy(), base.size + 1000, 130)       # only the first 130 entries may be traced
    return out


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
