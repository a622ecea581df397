"""The fast ray set-up of makeShadowRay (rts_kernels.hip), restated in numpy with float32 semantics.

A wave takes the fast set-up when one ballot says every lane passes its gate; it must then produce the general set-up's
o, d, 1/d and tmax bit for bit, and a wide-walk eligibility that is never looser than wideRaySetup(...) && raySafe(...).
Here: the identities the fast path rests on (exhaustive over exponents), and both forms side by side on edge inputs.
"""
import numpy as np
import pytest

F = np.float32
INF = F(np.inf)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def flt(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def epsilon_for(f, diff=13):                     # comp:113-120 (epsilonFor)
    u = bits(f).astype(np.int64)
    e = (u >> 23) & 0xFF
    e = e - np.minimum(diff, e)
    return flt(((u & ~(0xFF << 23)) | (e << 23)).astype(np.uint32))


def gmax(x, y):                                  # GLSL max: (x < y) ? y : x
    return np.where(x < y, y, x)


def all_floats_by_exponent(mantissas):
    e = np.arange(256, dtype=np.uint32)[:, None]
    return flt((e << 23) | np.asarray(mantissas, dtype=np.uint32)[None, :]).ravel()


MANT = np.array([0, 1, 2, 0x3FFFFF, 0x400000, 0x555555, 0x7FFFFE, 0x7FFFFF], dtype=np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# item 3: bias from one exponent cut
# ---------------------------------------------------------------------------------------------------------------------
def test_epsilon_identity_every_exponent_pair():
    v = all_floats_by_exponent(MANT)
    v = v[np.isfinite(v)]                                             # (non-finite values never pass the gate)
    a, b = np.meshgrid(v, v, indexing="ij")
    a, b = a.ravel(), b.ravel()
    m = np.maximum(a, b)
    gate = bits(m) >= (14 << 23)                                      # max(mo, mr) >= 2^-113
    fast = flt(bits(m) - np.uint32(13 << 23))
    slow = gmax(epsilon_for(a), epsilon_for(b))
    assert np.array_equal(bits(fast[gate]), bits(slow[gate]))
    assert np.array_equal(bits(fast[gate]), bits(epsilon_for(m)[gate]))
    # below the cut the clamped exponent makes epsilonFor non-monotone: such waves have to stay on the general path
    lo = ~gate
    assert np.any(bits(slow[lo]) != bits(epsilon_for(m)[lo]))


def test_epsilon_gate_boundary():
    assert bits(F(2.0 ** -113)) == 14 << 23
    below = flt(np.uint32((14 << 23) - 1))
    assert bits(below) < (14 << 23)


def test_max_of_bits_is_float_max():
    v = all_floats_by_exponent(MANT)
    v = v[np.isfinite(v)]
    a, b = np.meshgrid(np.abs(v), np.abs(v), indexing="ij")
    assert np.array_equal(np.maximum(bits(a), bits(b)), bits(np.maximum(a, b)))


# ---------------------------------------------------------------------------------------------------------------------
# item 2: sqrt without its scaling and fix-up
# ---------------------------------------------------------------------------------------------------------------------
def sqrt_gate(dd):                                                    # 2^-96 <= dd < inf as one unsigned compare
    return (bits(dd) - np.uint32(31 << 23)) < np.uint32(0x7F800000 - (31 << 23))


def test_sqrt_gate_is_the_range():
    v = all_floats_by_exponent(MANT)
    v = np.concatenate([v, -v, flt(np.array([0x7FC00000, 0xFFC00000, 0x7F800001], dtype=np.uint32))])
    with np.errstate(invalid="ignore"):
        want = (v >= F(2.0 ** -96)) & (v < INF)
    assert np.array_equal(sqrt_gate(v), want)
    # in the range the compiler's sequence neither scales (x < 2^-96) nor takes its zero / +inf fix-up
    assert sqrt_gate(F(2.0 ** -96)) and not sqrt_gate(flt(np.uint32((31 << 23) - 1)))
    assert sqrt_gate(F(np.finfo(np.float32).max)) and not sqrt_gate(INF)


def sqrt_core(x, s):
    """sqrtCore's fix-up for a v_sqrt_f32 result s: the signs of fma(-down, s, x) and fma(-up, s, x) are exact in
    float64 (the products are exact, and a rounded difference keeps its sign)."""
    x64, s64 = x.astype(np.float64), s.astype(np.float64)
    down, up = flt(bits(s) - np.uint32(1)), flt(bits(s) + np.uint32(1))
    r = np.where(x64 - down.astype(np.float64) * s64 <= 0, down, s)
    return np.where(x64 - up.astype(np.float64) * s64 > 0, up, r)


def test_sqrt_core_corrects_one_ulp():
    rng = np.random.default_rng(7)
    e = rng.integers(31, 255, 200_000).astype(np.uint32)
    x = flt((e << 23) | rng.integers(0, 1 << 23, e.size).astype(np.uint32))
    x = np.concatenate([x, all_floats_by_exponent(MANT)])
    x = x[sqrt_gate(x)]
    want = np.sqrt(x)
    for k in (-1, 0, 1):                                              # v_sqrt_f32 is within one ulp
        s = flt(bits(want).astype(np.int64) + k)
        assert np.array_equal(bits(sqrt_core(x, s)), bits(want)), k


# ---------------------------------------------------------------------------------------------------------------------
# item 4: the bound on |d| that replaces the root-box overflow test
# ---------------------------------------------------------------------------------------------------------------------
def wide_axis_bound(lo, hi):
    a, b = bits(lo) & np.uint32(0x7FFFFFFF), bits(hi) & np.uint32(0x7FFFFFFF)
    e = np.maximum(a, b) >> np.uint32(23)
    return np.where(e == 255, np.uint32(0x7F800000), (np.maximum(e, np.uint32(148)) - np.uint32(121)) << np.uint32(23))


def test_wide_bound_keeps_root_times_inv_below_1e37():
    r = all_floats_by_exponent(MANT)
    r = r[np.isfinite(r)]
    bound = flt(wide_axis_bound(r, F(0)))
    assert np.all(bound >= F(2.0 ** -100))
    with np.errstate(over="ignore"):
        for d in (bound, flt(bits(bound) + np.uint32(1)), flt(bits(bound) + np.uint32(0x3FFFFF))):
            ok = d < F(2.0 ** 100)
            inv = F(1) / d[ok]
            assert np.all(r[ok] * inv < F(1e37))                          # the test it replaces: M < 1e37
    assert np.all(flt(wide_axis_bound(flt(np.array([0x7F800000, 0x7FC00000], dtype=np.uint32)), F(0))) == INF)


def rcp_in_range(x):
    e = (bits(x) >> np.uint32(23)) & np.uint32(0xFF)
    return (e - np.uint32(27)) <= np.uint32(199)


def test_d_range_implies_rcp_in_range():
    v = all_floats_by_exponent(MANT)
    v = np.concatenate([v, -v])
    with np.errstate(invalid="ignore"):
        gate = (np.abs(v) >= F(2.0 ** -100)) & (np.abs(v) < F(2.0 ** 100))
    assert np.array_equal(gate, rcp_in_range(v))


# ---------------------------------------------------------------------------------------------------------------------
# both set-up forms side by side
# ---------------------------------------------------------------------------------------------------------------------
C1, C2, C3 = F(4.76837158e-7), F(2.38418579e-7), F(7.5e-37)


def slow_setup(cam, light, point, rel):
    o = cam + rel
    mo = gmax(gmax(np.abs(o[:, 0]), np.abs(o[:, 1])), np.abs(o[:, 2]))
    mr = gmax(gmax(np.abs(rel[:, 0]), np.abs(rel[:, 1])), np.abs(rel[:, 2]))
    bias = gmax(epsilon_for(mo), epsilon_for(mr))[:, None]
    L = np.broadcast_to(light, o.shape)
    if point:
        d0 = L - o
        ln = np.sqrt((d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]) + d0[:, 2] * d0[:, 2])
        inv = (F(1) / ln)[:, None]
        o = o + (d0 * inv) * bias
        d, tmax = L - o, F(1)
    else:
        o = o + L * bias
        d, tmax = L.copy(), F(1e9)
    return o, d, F(1) / d, tmax


def slow_wide_ok(o, inv, lo, hi):
    ok = np.ones(len(o), bool)
    for a in range(3):
        E = np.fmax(np.abs(lo[a] - o[:, a]), np.abs(hi[a] - o[:, a]))
        oi = o[:, a] * inv[:, a]
        slack = ((E * np.abs(inv[:, a])) * C1 + np.abs(oi) * C2) + C3
        M = np.fmax(np.abs(lo[a]), np.abs(hi[a])) * np.abs(inv[:, a])
        ok &= (slack < INF) & (M < F(1e37)) & (np.abs(oi) < F(1e37))
    fin = np.all(np.isfinite(o), axis=1)
    safe = fin & np.all(np.isfinite(inv) & (inv != 0), axis=1)
    return ok & safe


def fast_setup(cam, light, point, rel, lo_bits):
    """The fast path as the kernel computes it, with its per-lane gate (v_max3 drops NaNs: np.fmax)."""
    o = cam + rel
    mo = bits(np.fmax(np.fmax(np.abs(o[:, 0]), np.abs(o[:, 1])), np.abs(o[:, 2])))
    mr = np.maximum(np.maximum(bits(rel[:, 0]) & np.uint32(0x7FFFFFFF), bits(rel[:, 1]) & np.uint32(0x7FFFFFFF)),
                    bits(rel[:, 2]) & np.uint32(0x7FFFFFFF))
    m = np.maximum(mo, mr)
    gate = m >= np.uint32(14 << 23)
    bias = flt(m - np.uint32(13 << 23))[:, None]
    L = np.broadcast_to(light, o.shape)
    if point:
        d0 = L - o
        dd = (d0[:, 0] * d0[:, 0] + d0[:, 1] * d0[:, 1]) + d0[:, 2] * d0[:, 2]
        gate &= sqrt_gate(dd)
        inv = (F(1) / np.sqrt(dd))[:, None]                           # sqrtCore and rcpFast where the gate holds
        o = o + (d0 * inv) * bias
        d, tmax = L - o, F(1)
    else:
        o = o + L * bias
        d, tmax = L.copy(), F(1e9)
        gate &= np.all((bits(o) & np.uint32(0x7FFFFFFF)) < np.uint32(0x7F800000), axis=1)   # v_cmp_class 0x1F8
    ad = np.abs(d)
    with np.errstate(invalid="ignore"):
        gate &= np.all(ad >= flt(lo_bits)[None, :], axis=1)
        gate &= np.fmax(np.fmax(ad[:, 0], ad[:, 1]), ad[:, 2]) < F(2.0 ** 100)
    return o, d, F(1) / d, tmax, gate


def fast_wide_ok(o, inv):
    oi = o * inv
    return np.fmax(np.fmax(np.abs(oi[:, 0]), np.abs(oi[:, 1])), np.abs(oi[:, 2])) < F(1e37)


def edge_values():
    s = [0.0, -0.0, 1e-45, -1e-45, 1e-40, 2.0 ** -126, 2.0 ** -114, 2.0 ** -113, 2.0 ** -112, 1e-30, 1e-3, 0.5, 1.0, -3.0,
         7.25, 1e3, 1e6, 1e18, 2.0 ** 63, 1e30, 1e37, 3e38, np.finfo(np.float32).max, np.inf, -np.inf, np.nan]
    return np.array(s, dtype=np.float32)


def inputs(rng, n=60_000):
    ev = edge_values()
    rel = rng.standard_normal((n, 3)).astype(np.float32) * F(30)
    pick = rng.random((n, 3)) < 0.2
    rel[pick] = rng.choice(ev, pick.sum())
    rel[:64] = 0                                                      # a point light on a texel: len = 0 lanes
    return rel


LIGHTS = [(1, (3.0, 40.0, -2.0)), (1, (0.0, 0.0, 0.0)), (1, (1e30, -2e30, 5.0)), (1, (3e38, 1.0, 1.0)),
          (1, (np.nan, 1.0, 1.0)), (0, (0.3, 0.9, -0.2)), (0, (0.0, 1.0, 0.0)), (0, (1e-35, 1.0, 0.5)),
          (0, (np.inf, 1.0, 0.0))]
ROOTS = [((-50.0, -2.0, -60.0), (55.0, 30.0, 40.0)), ((-1e30, 0.0, -5.0), (4e36, 1.0, 5.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))]


@pytest.mark.parametrize("light", LIGHTS, ids=[f"{'point' if k else 'dir'}{i}" for i, (k, _) in enumerate(LIGHTS)])
@pytest.mark.parametrize("root", ROOTS, ids=["scene", "huge", "point"])
def test_fast_setup_equals_general_setup(light, root):
    rng = np.random.default_rng(11)
    rel = inputs(rng)
    cam = np.array([0.0, 0.0, 0.0], np.float32)
    point, L = light[0] == 1, np.array(light[1], np.float32)
    lo, hi = np.array(root[0], np.float32), np.array(root[1], np.float32)
    with np.errstate(all="ignore"):
        o0, d0, i0, t0 = slow_setup(cam, L, point, rel)
        ok0 = slow_wide_ok(o0, i0, lo, hi)
        for lo_bits in (np.full(3, 27 << 23, np.uint32), wide_axis_bound(lo, hi)):
            o1, d1, i1, t1, gate = fast_setup(cam, L, point, rel, lo_bits)
            g = gate
            assert np.array_equal(bits(o1[g]), bits(o0[g]))
            assert np.array_equal(bits(d1[g]), bits(d0[g]))
            assert np.array_equal(bits(i1[g]), bits(i0[g]))
            assert t1 == t0
            assert np.all(rcp_in_range(d1[g]))                        # rcpFast is the division there
        # the wide walk's eligibility: never looser than today's
        o1, d1, i1, t1, gate = fast_setup(cam, L, point, rel, wide_axis_bound(lo, hi))
        fast_ok = gate & fast_wide_ok(o1, i1)
        assert not np.any(fast_ok & ~ok0)
    if light[1] in ((3.0, 40.0, -2.0), (0.3, 0.9, -0.2)) and root[0][0] == -50.0:
        assert gate.mean() > 0.5                                      # a scene-sized light: the fast path is the common case


def test_fast_setup_nonzero_camera():
    rng = np.random.default_rng(5)
    rel = inputs(rng, 20_000)
    for cam in (np.array([3.5, -1e6, 2e-40], np.float32), np.array([np.inf, 0.0, 0.0], np.float32)):
        for point, L in ((True, np.array([10.0, 20.0, 30.0], np.float32)), (False, np.array([0.0, 1.0, 0.0], np.float32))):
            with np.errstate(all="ignore"):
                o0, d0, i0, t0 = slow_setup(cam, L, point, rel)
                o1, d1, i1, t1, g = fast_setup(cam, L, point, rel, np.full(3, 27 << 23, np.uint32))
            assert np.array_equal(bits(o1[g]), bits(o0[g])) and np.array_equal(bits(i1[g]), bits(i0[g]))
            assert np.array_equal(bits(d1[g]), bits(d0[g]))
