"""Shared by the soft light list distance tests: the frames and lists of tests/soft_list_cases.py, and the expected distance and count
planes from the untouched oracle alone.

The definition (include/rts.h): distance plane l at pixel p = the float the soft distance trace writes at p for the derived light of
entry l alone (api.SoftLightList.light) -- the minimum over its samples of the one-ray distance --, count plane l = the number of
samples whose distance is +Inf, both where bit l of the light map's byte is set (no map: everywhere), else +0 and 0.  `definition`
takes each light's planes from soft_distance_cases.definition (oracle.gen_rays, the oracle's any-hit bisected, an integer minimum).

Beside the three pixel classes of soft_list_cases, which `oracle_planes` asserts of the counts again, it asserts for every soft light
with a radius above 0 that at least 1 % of the pixels have a finite minimum that is NOT sample 0's distance, and for every list that
at least 1 % have one that is not their light's LAST sample's: a kernel that keeps the first distance it sees, or the last, fails.
(Per light the last sample is not asked for: the two samples of "8x2" light 1, a directional light, are ordered alike in every pixel.)

LISTS is soft_list_cases.LISTS with ONE entry changed.  Light 5 of "8x2" (p3, two samples from 25 on, radius 1.5) has a minimum that
is not sample 0's in 17 pixels of 3072 (64 x 48) and 9 of 2257 (61 x 37), against the bars of 30 and 22: the point light is nearer to
sample 25's side almost everywhere.  From 26 on the same light shows 313 and 190 such pixels, and its count classes (0 / n / between)
are 65 / 2741 / 266 and 37 / 2058 / 162.  The smallest share that remains is light 2 of "8x2": 40 and 28 pixels."""
import numpy as np

import oracle
import soft_distance_cases
from distance_cases import INF_BITS, bisect_distance, bits
from raytracedshadows_amd import api
import soft_list_cases
from soft_list_cases import FORMS, FRAMES, TABLE, list_frame, samples  # noqa: F401  (re-exported to the tests)

LISTS = dict(soft_list_cases.LISTS)
LISTS["8x2"] = LISTS["8x2"][:5] + (soft_list_cases._soft("p3", 2, 26, 1.5),) + LISTS["8x2"][6:]


def make_list(name):
    return api.SoftLightList.make(LISTS[name], TABLE)

DIST_GUARD = 0xFFC0DE01                          # a NaN's bit pattern no trace writes: the distances' guard


def under(dist, counts, m):
    """The planes under a map: +0 and 0 where the map's bit is clear."""
    bit = np.stack([((m >> l) & 1).astype(bool) for l in range(dist.shape[0])])
    return np.where(bit, dist, np.float32(0)), np.where(bit, counts, 0).astype(np.uint8)


def definition(packed, k, lights, pos, lights_map=None):
    """(float32[count, H, W], uint8[count, H, W]) from the oracle alone."""
    H, W = pos.shape[:2]
    dist, counts = np.zeros((lights.count, H, W), np.float32), np.zeros((lights.count, H, W), np.uint8)
    for l in range(lights.count):
        dist[l], counts[l] = soft_distance_cases.definition(packed, k, lights.light(l), pos)
    if lights_map is not None:
        dist, counts = under(dist, counts, lights_map)
    return dist, counts


def sample_distance_bits(packed, k, light, pos, j):
    """uint32[H, W]: the one-ray distance of sample j alone, from the oracle's rays and any-hit."""
    H, W = pos.shape[:2]
    ol = oracle.light_from_product(light, k)
    n = max(1, ol.nsamples)
    rays = oracle.gen_rays(k.as_array(), ol, pos).reshape(H * W, n, 8)
    return bits(bisect_distance(packed, np.ascontiguousarray(rays[:, j]))).reshape(H, W)


class SoftListDistanceFrame:
    """A frame of soft_list_cases and, per list, the oracle's planes (asserted not to degenerate) and the host twin's -- computed
    once, shared, never written to."""

    def __init__(self, W, H):
        self.fr = fr = list_frame(W, H)
        self.W, self.H, self.k, self.packed, self.pos, self.nrm, self.wl = W, H, fr.k, fr.packed, fr.pos, fr.nrm, fr.wl
        self._oracle, self._want, self._facing = {}, {}, {}

    def facing(self, name):
        if name not in self._facing:
            f = api.facing_lights(self.k, make_list(name).hard_list(), self.pos, self.nrm)
            f.setflags(write=False)
            self._facing[name] = f
        return self._facing[name]

    def oracle_planes(self, name):
        if name not in self._oracle:
            lights = make_list(name)
            dist, counts = definition(self.packed, self.k, lights, self.pos)
            if LISTS[name] == soft_list_cases.LISTS[name]:
                assert np.array_equal(counts, self.fr.oracle_planes(name)), name
            least, not_last = dist[0].size // 100, 0
            for l in range(lights.count):
                e, n = lights.lights[l], samples(lights, l)
                got = bits(dist[l])
                assert np.array_equal(got == INF_BITS, counts[l] == n), (name, l)
                at0, atn = int((counts[l] == 0).sum()), int((counts[l] == n).sum())
                between = counts[l].size - at0 - atn
                what = (self.W, self.H, name, l, at0, atn, between, least)
                if n > 1 and e.radius > 0:
                    assert min(at0, atn, between) >= least, what
                else:
                    assert min(at0, atn) >= least and between == 0, what
                if n > 1 and e.radius > 0:
                    finite = got != INF_BITS
                    for j in (0, n - 1):
                        one = sample_distance_bits(self.packed, self.k, lights.light(l), self.pos, j)
                        assert (got <= one).all(), (name, l, j)
                        other = int((finite & (got != one)).sum())
                        print(f"soft_list_distance_cases: {self.W}x{self.H} {name} light {l}: minimum is not sample {j}'s in {other} "
                              f"pixels of {got.size} (bar {least})")
                        if j == 0:
                            assert other >= least, (self.W, self.H, name, l, other, least)
                        else:
                            not_last += other
            assert not_last >= least or all(samples(lights, l) == 1 or lights.lights[l].radius == 0 for l in range(lights.count)), \
                (self.W, self.H, name, not_last, least)
            dist.setflags(write=False)
            counts.setflags(write=False)
            self._oracle[name] = (dist, counts)
        return self._oracle[name]

    def want(self, name):
        """The host twin's planes without a map (tests/test_soft_list_distance_host.py pins them to oracle_planes)."""
        if name not in self._want:
            d, c = api.soft_light_list_distance(self.packed, self.k, make_list(name), self.pos, self.W, self.H)
            d.setflags(write=False)
            c.setflags(write=False)
            self._want[name] = (d, c)
        return self._want[name]


_FRAMES = {}


def distance_frame(W, H):
    if (W, H) not in _FRAMES:
        _FRAMES[(W, H)] = SoftListDistanceFrame(W, H)
    return _FRAMES[(W, H)]
