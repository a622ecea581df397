"""Shared by the adaptive soft light list tests: the lists, the table and the frames of tests/soft_list_cases.py, unchanged, each with
one or two probe vectors, and the expected planes from the untouched oracle alone.

The definition (include/rts.h), per light l of n samples with the probe count k = probes[l]: k == 0 -- the plane is the full count
c_n and bit l of `refined` is 0; k >= 1 -- the plane and bit l of `refined` are what the adaptive soft mask trace writes for the
derived light of entry l (api.SoftLightList.light) with probe k.  `definition` takes each light's rays from oracle.gen_rays and their
bytes from oracle.trace_rays through tests/adaptive_cases.definition, whose counting it uses as it is, and and's the result with
the map's bit.

`oracle_planes` asserts per light that the case does not degenerate, with adaptive_cases.assert_case: a light with k >= 2 and a radius
above 0 has a pixel in both unanimous classes, a refined pixel with a count strictly between 0 and n, and a pixel whose byte is not
c_n; a light with k == 1 cannot refine (0 < c_1 < 1 has no solution) and is checked with refines=False; a light of radius 0 -- every
sample is the light itself -- never refines and has byte == c_n everywhere; a light with k == 0 has byte == c_n and no refined bit.

What the probe vectors cover: `one` (4) and (2): one light of 16, penumbra in few tiles, so most tiles leave between the barriers of the
4-wave form; `mixed` (0,2,2,0,2) and (0,5,4,0,1): hard entries, a directional light, n - k = 1 so that waves own no refinement pair, a
k = 1 light beside refining ones, tiles that refine one light and skip another; `8x2` (1,...,1): eight lights that never refine, no tile
enters the second phase; `shared16` (4,3,4): the light of radius 0; `end48` (5,0): a range ending at slot 48 and a full-count hard light
behind an adaptive one; `48` (4) and (3): the longest deal, and with 3 probe samples a wave that owns no probe pair; `3pairs` (0,1): a
first phase of two pairs in all; `overlap` (3,4,2) and (0,4,0): adaptive and full-count soft lights in one list."""
import numpy as np

import adaptive_cases
from raytracedshadows_amd import api
from soft_list_cases import FORMS, FRAMES, LISTS, TABLE, list_frame, make_list, samples  # noqa: F401  (re-exported to the tests)

#: (list name, probes): in the order of the issue's table
CASES = [("one", (4,)), ("one", (2,)), ("mixed", (0, 2, 2, 0, 2)), ("mixed", (0, 5, 4, 0, 1)), ("8x2", (1,) * 8), ("shared16", (4, 3, 4)),
         ("end48", (5, 0)), ("48", (4,)), ("48", (3,)), ("3pairs", (0, 1)), ("overlap", (3, 4, 2)), ("overlap", (0, 4, 0))]


def case_id(v):
    return "-".join(map(str, v)) if isinstance(v, tuple) else None


def definition(packed, k, lights, probes, pos, lights_map=None):
    """(uint8[count, H, W] counts, uint8[H, W] refined, uint8[count, H, W] c_n) from the oracle alone."""
    H, W = pos.shape[:2]
    counts, cn = np.zeros((lights.count, H, W), np.uint8), np.zeros((lights.count, H, W), np.uint8)
    refined = np.zeros((H, W), np.uint8)
    assert len(probes) == lights.count
    for l in range(lights.count):
        n, probe = samples(lights, l), probes[l]
        assert 0 <= probe < n
        mask, took, full = adaptive_cases.definition(packed, k, lights.light(l), pos, max(1, probe))
        if probe == 0:                                   # traced in full: the count of every sample, never a refined bit
            mask, took = full, np.zeros_like(took)
        if lights_map is not None:
            bit = (lights_map >> l) & 1
            mask, took, full = mask * bit, took * bit, full * bit
        counts[l], cn[l] = mask, full
        refined |= (took << l).astype(np.uint8)
    return counts, refined, cn


def assert_light(counts, refined, cn, lights, probes, l, what):
    """The case of light l does not degenerate (see the module's text)."""
    e, n, probe = lights.lights[l], samples(lights, l), probes[l]
    took = (refined >> l) & 1
    what = what + (l,)
    if probe == 0:
        assert np.array_equal(counts[l], cn[l]) and not took.any(), what
    elif n > 1 and e.radius == 0:
        assert np.array_equal(counts[l], cn[l]) and not took.any() and set(np.unique(counts[l])) == {0, n}, what
    else:
        adaptive_cases.assert_case(counts[l], took, cn[l], n, what, refines=probe > 1)


class AdaptiveListFrame:
    """A frame of tests/soft_list_cases.py and, per (list, probes), the oracle's planes (asserted not to degenerate) and the host
    twin's -- computed once, shared, never written to."""

    def __init__(self, W, H):
        self.fr = fr = list_frame(W, H)
        self.W, self.H, self.k, self.packed, self.pos, self.nrm, self.wl = W, H, fr.k, fr.packed, fr.pos, fr.nrm, fr.wl
        self._oracle, self._want = {}, {}

    def facing(self, name):
        return self.fr.facing(name)

    def oracle_planes(self, name, probes):
        if (name, probes) not in self._oracle:
            lights = make_list(name)
            counts, refined, cn = definition(self.packed, self.k, lights, probes, self.pos)
            for l in range(lights.count):
                assert_light(counts, refined, cn, lights, probes, l, (self.W, self.H, name, probes))
            assert int(refined.max()) < (1 << lights.count)
            for a in (counts, refined, cn):
                a.setflags(write=False)
            self._oracle[(name, probes)] = (counts, refined, cn)
        return self._oracle[(name, probes)]

    def want(self, name, probes):
        """The host twin's (counts, refined) without a map (tests/test_soft_list_adaptive_host.py pins them to oracle_planes)."""
        if (name, probes) not in self._want:
            self.oracle_planes(name, probes)
            c, r = api.soft_light_list_adaptive(self.packed, self.k, make_list(name), probes, self.pos, self.W, self.H)
            c.setflags(write=False)
            r.setflags(write=False)
            self._want[(name, probes)] = (c, r)
        return self._want[(name, probes)]


_FRAMES = {}


def adaptive_list_frame(W, H):
    if (W, H) not in _FRAMES:
        _FRAMES[(W, H)] = AdaptiveListFrame(W, H)
    return _FRAMES[(W, H)]


def under(counts, refined, lights_map):
    """(counts, refined) of a trace without a map, as the same trace writes them under `lights_map`: every light's plane and bit where
    the map has the light's bit -- a light's bytes depend on its own bit alone."""
    count = counts.shape[0]
    c = np.stack([counts[l] * ((lights_map >> l) & 1) for l in range(count)])
    return c, (refined & lights_map & ((1 << count) - 1)).astype(np.uint8)
