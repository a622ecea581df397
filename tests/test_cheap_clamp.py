"""The near end of the cheap slab test for segment rays (tools/gen_wide_asm.py: cheap_pair, rts_kernels.hip: cheapNear).

A point light's rays are segments (d = L - o, tmax = 1), and their wide walk reduces the three near values with one
`v_max3_f32 ... clamp` (min(max(n, 0), 1)) instead of max(max3, 0).  The six products and the far value are the same in
both forms, so the clamped test must accept every box the unclamped one accepts, and accept more only where near > 1.
This restates both reductions in float32 (the reductions are exact: max/min/clamp round nothing) and checks that."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32 = np.float32
FMAX = np.finfo(F32).max
TINY = np.finfo(F32).tiny
DEN = F32(1e-45)


def _edge_values():
    v = [0.0, -0.0, DEN, -DEN, TINY, -TINY, TINY / 2, 1.0, -1.0, FMAX, -FMAX, np.inf, -np.inf, 0.5, 2.0, 1e-30, -1e-30, 1e30]
    v += [np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)), np.nextafter(F32(0), F32(1)), np.nextafter(F32(0), F32(-1))]
    return np.array(v, F32)


def _samples(rng, n):
    """far/near triples: random magnitudes over the whole range, values straddling 0 and 1, and every edge value."""
    parts = [(rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-40, 38, (n, 3))).astype(F32),
             rng.uniform(-0.5, 1.5, (n, 3)).astype(F32),
             (F32(1) + rng.integers(-64, 65, (n, 3)).astype(F32) * np.finfo(F32).eps).astype(F32),
             (rng.integers(-64, 65, (n, 3)).astype(F32) * DEN).astype(F32)]
    e = _edge_values()
    parts.append(e[rng.integers(0, e.size, (n, 3))])
    return np.concatenate(parts)


def _hw_max(a, b):
    """v_max_f32 in IEEE mode on quiet NaNs: the other operand (the fma results the test reduces are never signalling)."""
    return np.fmax(a, b)


def _old_near(n):
    """v_max_f32 n0, n0, n1 ; v_max3_f32 n0, n0, n2, 0"""
    return _hw_max(_hw_max(_hw_max(n[:, 0], n[:, 1]), n[:, 2]), F32(0))


def _new_near(n):
    """v_max3_f32 n0, n0, n1, n2 clamp  (dx10_clamp: NaN -> 0)"""
    m = _hw_max(_hw_max(n[:, 0], n[:, 1]), n[:, 2])
    m = np.where(np.isnan(m), F32(0), m)
    return np.minimum(np.maximum(m, F32(0)), F32(1))


def _far(f):
    """v_min3_f32"""
    return np.fmin(np.fmin(f[:, 0], f[:, 1]), f[:, 2])


def test_clamped_near_accepts_a_superset_and_more_only_beyond_the_light():
    rng = np.random.default_rng(20261016)
    n = _samples(rng, 200000)
    f = _samples(rng, 200000)
    with np.errstate(invalid="ignore"):
        far, old_near, new_near = _far(f), _old_near(n), _new_near(n)
        old, new = far >= old_near, far >= new_near
    assert old_near.dtype == F32 and new_near.dtype == F32
    assert (new_near <= old_near).all()                      # clamp(n) <= max(n, 0), signed zeros compare equal
    assert not (old & ~new).any()                            # the superset property
    extra = new & ~old
    assert extra.any()                                       # (the samples reach the case at all)
    assert (old_near[extra] > 1).all() and (far[extra] >= 1).all() and (far[extra] < old_near[extra]).all()
    # where near <= 1 both forms are the same test
    low = old_near <= 1
    assert (old[low] == new[low]).all()


def test_empty_slot_stays_rejected():
    """An empty slot's far plane gives -huge or -inf; near is >= 0 in both forms."""
    rng = np.random.default_rng(7)
    n = _samples(rng, 20000)
    for far_value in (-np.inf, -FMAX, F32(-1e30)):
        far = np.full(n.shape[0], far_value, F32)
        with np.errstate(invalid="ignore"):
            assert not (far >= _new_near(n)).any()
            assert not (far >= _old_near(n)).any()


def test_generator_emits_the_clamp_for_segment_rays_only():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_wide_asm as g
    finally:
        sys.path.pop(0)
    for octant in range(9):
        plain, seg = g.cheap_pair(0, 1, octant), g.cheap_pair(0, 1, octant, True)
        assert not any("clamp" in line for line in plain)
        assert sum("clamp" in line for line in seg) == 2
        assert len(seg) == len(plain) - 2                        # one VALU fewer per slot
        assert [x for x in plain if "fma" in x] == [x for x in seg if "fma" in x]
        assert [x for x in plain if "cmp" in x] == [x for x in seg if "cmp" in x]
        # the directional loop is the unclamped one; the segment loop differs only in the cheap test
        assert not any("clamp" in line for line in g.loop(octant))
        assert sum("clamp" in line for line in g.loop(octant, True)) == 4
    assert not any("clamp" in line for line in g.loop_range())     # the piece loop keeps the unclamped test (EXPERIMENTS.md)
