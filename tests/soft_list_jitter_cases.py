"""Shared by the jittered soft light list tests: the lists, the table and the frames of tests/soft_list_cases.py, unchanged, each with a
probe vector and a vector of per-pixel jitter tables, and the expected planes from the untouched oracle alone.

The definition (include/rts.h), per light l with n samples, the probe k = probes[l] and the table T = tables[l]: the plane and bit l of
`refined` are what the one-light trace writes for the derived light `lights.light(l, table=T)` -- T scaled offsets, rts_light.table = T,
so pixel p aims sample j at entry (start(p) + j) mod T, start(p) hashed from p's index in the full frame -- with probe k (k == 0: the
full count, no refined bit).  `definition` takes each light's rays from oracle.gen_rays, which honours the table, through
tests/adaptive_cases.definition, whose counting it uses as it is, and and's the result with the map's bit.

`oracle_planes` asserts on the ORACLE's planes that no case degenerates:
  * per light, soft_list_adaptive_cases.assert_light: a refining light has both unanimous classes, a refined pixel with a partial
    count and a byte that is not c_n; k == 1 and radius 0 never refine; k == 0 has byte == c_n;
  * a case that has a light with k >= 1 AND a table has one such light whose plane differs somewhere from the same case with tables
    all 0 (a light without a table is, by definition, the untabled light: only a tabled one can show the table);
  * a light with k == 0 and T == n EQUALS the untabled plane -- a rotation of all n samples keeps the count;
  * a light with k == 0 and T > n differs from it.

What the cases cover: `one` (4) (16): T == n under a probe; `one` (2) (40): first 8, so 8 + 40 = 48, a range ending at the last slot;
`mixed`: hard entries (table 0), T == n, T > n, T == n again on a range that ends at slot 48; `shared16`: a radius-0 light with a
table beside a tabled and an untabled one; `48` with probe 4 and with probe 0; `overlap`: jittered full-count lights beside an untabled
adaptive one; `8x2`: eight k = 1 lights with T == n == 2, which never refine and enter no second phase."""
import numpy as np

import adaptive_cases
from raytracedshadows_amd import api
from soft_list_adaptive_cases import assert_light, case_id, under  # noqa: F401  (re-exported to the tests)
from soft_list_cases import FORMS, FRAMES, LISTS, TABLE, list_frame, make_list, samples  # noqa: F401  (re-exported to the tests)

#: (list name, probes, tables): in the order of the issue's table
CASES = [("one", (4,), (16,)), ("one", (2,), (40,)), ("mixed", (0, 2, 2, 0, 2), (0, 6, 12, 0, 3)), ("shared16", (4, 3, 4), (16, 0, 16)),
         ("48", (4,), (48,)), ("48", (0,), (48,)), ("overlap", (0, 4, 0), (20, 0, 12)), ("8x2", (1,) * 8, (2,) * 8)]


def definition(packed, k, lights, probes, tables, pos, lights_map=None):
    """(uint8[count, H, W] counts, uint8[H, W] refined, uint8[count, H, W] c_n) from the oracle alone."""
    H, W = pos.shape[:2]
    counts, cn = np.zeros((lights.count, H, W), np.uint8), np.zeros((lights.count, H, W), np.uint8)
    refined = np.zeros((H, W), np.uint8)
    assert len(probes) == lights.count == len(tables)
    for l in range(lights.count):
        n, probe = samples(lights, l), probes[l]
        assert 0 <= probe < n
        mask, took, full = adaptive_cases.definition(packed, k, lights.light(l, table=tables[l]), pos, max(1, probe))
        if probe == 0:                                   # traced in full: the count of every sample, never a refined bit
            mask, took = full, np.zeros_like(took)
        if lights_map is not None:
            bit = (lights_map >> l) & 1
            mask, took, full = mask * bit, took * bit, full * bit
        counts[l], cn[l] = mask, full
        refined |= (took << l).astype(np.uint8)
    return counts, refined, cn


class JitterListFrame:
    """A frame of tests/soft_list_cases.py and, per (list, probes, tables), the oracle's planes (asserted not to degenerate) and the
    host twin's -- computed once, shared, never written to."""

    def __init__(self, W, H):
        self.fr = fr = list_frame(W, H)
        self.W, self.H, self.k, self.packed, self.pos, self.nrm, self.wl = W, H, fr.k, fr.packed, fr.pos, fr.nrm, fr.wl
        self._oracle, self._want = {}, {}

    def facing(self, name):
        return self.fr.facing(name)

    def _planes(self, name, probes, tables):
        key = (name, probes, tables)
        if key not in self._oracle:
            out = definition(self.packed, self.k, make_list(name), probes, tables, self.pos)
            for a in out:
                a.setflags(write=False)
            self._oracle[key] = out
        return self._oracle[key]

    def oracle_planes(self, name, probes, tables):
        lights = make_list(name)
        counts, refined, cn = self._planes(name, probes, tables)
        if any(tables):
            what = (self.W, self.H, name, probes, tables)
            plain = self._planes(name, probes, (0,) * lights.count)[0]
            shown = []
            for l in range(lights.count):
                assert_light(counts, refined, cn, lights, probes, l, what)
                n, same = samples(lights, l), np.array_equal(counts[l], plain[l])
                if tables[l] == 0:
                    assert same, what + (l,)
                elif probes[l] == 0:
                    assert same == (tables[l] == n), what + (l, "a rotation of all samples keeps the count; a longer table does not")
                else:
                    shown.append(not same)
            assert any(shown) or not shown, what + ("no tabled light with a probe differs from the untabled case",)
            assert int(refined.max()) < (1 << lights.count)
        return counts, refined, cn

    def want(self, name, probes, tables):
        """The host twin's (counts, refined) without a map (tests/test_soft_list_jitter_host.py pins them to oracle_planes)."""
        key = (name, probes, tables)
        if key not in self._want:
            self.oracle_planes(name, probes, tables)
            c, r = api.soft_light_list_adaptive(self.packed, self.k, make_list(name), probes, self.pos, self.W, self.H, tables=tables)
            c.setflags(write=False)
            r.setflags(write=False)
            self._want[key] = (c, r)
        return self._want[key]


_FRAMES = {}


def jitter_list_frame(W, H):
    if (W, H) not in _FRAMES:
        _FRAMES[(W, H)] = JitterListFrame(W, H)
    return _FRAMES[(W, H)]


def light_map(fr, count):
    """A map that mixes every bit pattern below `count` with bits above it, whole zero bytes included."""
    y, x = np.mgrid[0:fr.H, 0:fr.W]
    m = ((x * 7 + y * 13 + (x >> 3) * 5) & 0xFF).astype(np.uint8)
    m[(x + y) % 5 == 0] = 0
    assert ((m & ((1 << count) - 1)) == 0).any() and (m != 0).any()
    return m
