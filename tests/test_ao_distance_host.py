"""CPU: AO distance and falloff on the host (include/rts_scene.h: rtsh_ambient_occlusion_distance).  The twin against the
numpy rule of tests/ao_distance_cases.py (rays_distance over the numpy rays, checked against the oracle's any-hit byte; minimum, bins,
weights, A and the quotient in numpy integers), bit for bit, on every frame of ao_cases with n of 1, 3, 4, 5, 16, 48, tables 0, n and
64, masked and unmasked maps and four falloffs; the five anchors; each output None in turn; NaN positions under an inactive map;
below-horizon directions and the ground quad; a d_j of exactly +0; the bin edges through the rule and (on the shared per-sample source)
in tests/cpp/ao_distance_host.cpp under the host sanitizers; the guard that the frames spread over bins and hold partly free pixels,
from the rule alone; refusals, guard bytes and rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ao_cases as ac
import ao_distance_cases as dc
from raytracedshadows_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32 = np.float32, np.uint32
NS, SHARES = dc.NS, dc.SHARES
# The guard's ladder (5, 10, 20, 50 % of the diagonal) stops at its FIRST rung on ("cornell_128", 48, 40), n = 16: the blocked samples
# fall into all 64 bins and 171 pixels have 0 < c < n (4.36's figure).
GUARD_SHARE = 0.05


@pytest.fixture(scope="module", params=ac.FRAMES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}")
def fr(request):
    return ac.frame(*request.param)


def _twin(fr, n, table, share, fall, masked=False, dirs_key=None, **kw):
    ao = fr.ao(n, table, share, dirs=None if dirs_key is None else ac.below_horizon_dirs())
    pos, act = (fr.dirty, fr.active) if masked else (fr.pos, None)
    return api.ambient_occlusion_distance(fr.packed, fr.k, ao, dc.falloff(fall) if fall else None, pos, fr.nrm, fr.W, fr.H, active=act, **kw)


def test_twin_equals_the_rule_bit_for_bit_and_the_anchors_hold(fr):
    mixed = blocked = 0
    for n in NS:
        S = 65535 // n
        for table in ac.tables(n):
            for masked in (False, True):
                share = SHARES[n]
                live = dc.live_of(fr.nrm, fr.active if masked else None)
                planes = {}
                for fall in dc.FALLOFFS:
                    got = _twin(fr, n, table, share, fall, masked)
                    dc.same_planes(got, dc.want(fr, n, table, share, fall, masked), (n, table, masked, fall))
                    planes[fall] = got
                counts, distance, obs = planes["saw"]
                # anchor 1: counts is the AO twin's plane; distance is finite exactly where counts < n (at a live pixel)
                assert np.array_equal(counts, fr.want(n, table, share, masked))
                assert np.array_equal(dc.bits(distance)[live] < dc.INF_BITS, counts[live] < n)
                # inactive: 0, +0.0f, 0 -- under NaN positions where masked
                assert (counts[~live] == 0).all() and (dc.bits(distance)[~live] == 0).all() and (obs[~live] == 0).all()
                # anchors 2, 3, 4
                assert np.array_equal(planes["zeros"][2], counts.astype(np.uint16) * S)
                assert (planes["full"][2][live] == n * S).all()
                for fall in dc.FALLOFFS:
                    assert (planes[fall][2] >= counts.astype(np.int64) * S).all() and (planes[fall][2] <= n * S).all()
                assert (planes["linear"][2] >= planes["zeros"][2]).all() and (planes["full"][2] >= planes["linear"][2]).all()
                mixed += bool(((counts > 0) & (counts < n)).any())
                blocked += int((counts[live] < n).sum())
    assert (mixed >= 2 and blocked > 0) or fr.W * fr.H < 100, "no partly free pixel in nearly every case"


def test_raising_one_weight_never_lowers_a_pixel():
    fr = ac.frame("cornell_128", 48, 40)
    d = dc.distances(fr, 16, 0, GUARD_SHARE)
    live = ~fr.background
    base = dc.falloff("saw").weights()
    _, _, low = _twin(fr, 16, 0, GUARD_SHARE, "saw")
    rose = 0
    for b in (0, 1, 17, 62, 63):
        w = base.copy()
        w[b] = 255
        ao = fr.ao(16, 0, GUARD_SHARE)
        _, _, high = api.ambient_occlusion_distance(fr.packed, fr.k, ao, api.AoFalloff.make(w), fr.pos, fr.nrm, fr.W, fr.H)
        assert np.array_equal(high, dc.rule_from_distances(d, 16, w, live)[2])
        assert (high >= low).all()
        rose += int((high > low).sum())
    assert rose > 0


def test_one_sample_is_the_hard_point_lights_distance():
    """Anchor 5: with n == 1 distance is bit for bit rtsh_shadow_distance's for the hard point light at ao_cases.aim_rule's L, on a
    one-pixel frame."""
    fr = ac.frame("cornell_128", 17, 5)
    seen_blocked = seen_free = 0
    for share in (0.05, 0.5, 10.0):
        ao = fr.ao(1, 0, share)
        counts, distance, _ = api.ambient_occlusion_distance(fr.packed, fr.k, ao, api.AoFalloff.linear(), fr.pos, fr.nrm, fr.W, fr.H)
        for y, x in np.argwhere(~fr.background)[::3]:
            L = ac.aim_rule(fr.k, ao, fr.pos, fr.nrm, int(y), int(x), 0)
            light = api.Light.make(api.Light.POINT, [float(v) for v in L])
            one, mask = api.shadow_distance(fr.packed, fr.k, light, np.ascontiguousarray(fr.pos[y:y + 1, x:x + 1]), 1, 1)
            assert dc.bits(one)[0, 0] == dc.bits(distance)[y, x] and mask[0, 0] == counts[y, x], (share, y, x)
            seen_blocked += int(mask[0, 0] == 0); seen_free += int(mask[0, 0] == 1)
    assert seen_blocked > 0 and seen_free > 0


def test_each_output_none_in_turn(fr):
    counts, distance, obs = _twin(fr, 5, 64, 0.5, "linear")
    a = _twin(fr, 5, 64, 0.5, "linear", want_counts=False)
    assert a[0] is None
    dc.same_planes(a, (counts, distance, obs), "counts None")
    b = _twin(fr, 5, 64, 0.5, "linear", want_distance=False)
    assert b[1] is None
    dc.same_planes(b, (counts, distance, obs), "distance None")
    c = _twin(fr, 5, 64, 0.5, None, want_obscurance=False)               # (no falloff is needed without the plane)
    assert c[2] is None
    dc.same_planes(c, (counts, distance, obs), "obscurance None")


def test_guard_bins_and_partly_free_pixels_by_the_rule_alone():
    share, nbins, partly = dc.guard_radius()
    print(f"guard: radius {share} of the diagonal: blocked samples in {nbins} bins, {partly} pixels with 0 < c < 16")
    assert nbins >= 8 and partly >= 32, (share, nbins, partly)
    assert share == GUARD_SHARE
    fr = ac.frame("cornell_128", 48, 40)
    for fall in ("linear", "saw"):
        dc.same_planes(_twin(fr, 16, 0, share, fall), dc.want(fr, 16, 0, share, fall), ("the guard's case", fall))
    lin, saw = _twin(fr, 16, 0, share, "linear")[2], _twin(fr, 16, 0, share, "saw")[2]
    assert (lin != saw).any() and (lin != _twin(fr, 16, 0, share, "zeros")[2]).any()


def test_bin_edges_and_a_distance_of_exactly_zero():
    """The bins through the rule's float32 arithmetic: k / 64 opens bin k, the float in front of it closes bin k - 1, +0 and the
    denormals are bin 0, 1.0 and beyond bin 63 (tests/cpp/ao_distance_host.cpp asks the same of the shared function itself).  Then a
    d_j of exactly +0 through the twin, on ao_distance_cases.zero_distance_case: the surface point IS the world's origin, so the bias
    is 0, the ray starts in the quad's plane and the accepted t is a zero -- bin 0, whatever the direction."""
    edges = np.arange(1, 65, dtype=np.float64) / 64.0
    e = edges.astype(f32).view(u32)
    assert np.array_equal(dc.bin_rule(e), np.minimum(np.arange(1, 65), 63))
    assert np.array_equal(dc.bin_rule(e - u32(1)), np.arange(0, 64))
    assert dc.bin_rule(np.array([0, 1, 0x007FFFFF, 0x3F800001, 0x40F00000, dc.INF_BITS - 1], u32)).tolist() == [0, 0, 0, 63, 63, 63]
    packed, k, pos, nrm, at_origin = dc.zero_distance_case()
    H, W = pos.shape[:2]
    w = np.full(64, 200, np.uint8)
    w[0] = 3
    fall = api.AoFalloff.make(w)
    for n in (1, 4, 5):
        ao = api.AoParams.make(n, 2.0, seed=n)
        got = api.ambient_occlusion_distance(packed, k, ao, fall, pos, nrm, W, H)
        rule = dc.distance_rule(packed, k, ao, fall, pos, nrm)
        dc.same_planes(got, rule[:3], ("d == +0", n))
        assert (rule[3][at_origin] == 0).all()                           # every d_j there is exactly +0
        assert (got[0][at_origin] == 0).all() and (dc.bits(got[1])[at_origin] == 0).all()
        assert (got[2][at_origin] == (2 * 3 * n * (65535 // n) + 255) // 510).all()
        elsewhere = dc.live_of(nrm) & ~at_origin
        assert (got[0][elsewhere] == n).all()                            # (lifted off the plane by the bias: free)


def test_below_horizon_dirs_and_ground_quad():
    fr = ac.frame("terrain_96", 40, 36)
    for n, table in ((16, 64), (4, 0)):
        for fall in ("linear", "saw"):
            dc.same_planes(_twin(fr, n, table, 0.5, fall, dirs_key="below"), dc.want(fr, n, table, 0.5, fall, dirs_key="below"),
                           ("below", n, table, fall))
    packed, k, pos, nrm = ac.ground_quad()
    H, W = pos.shape[:2]
    live = dc.live_of(nrm)
    for n in NS:
        for table in ac.tables(n):
            ao = api.AoParams.make(n, 2.0, table=table, seed=n)
            fall = dc.falloff("saw")
            got = api.ambient_occlusion_distance(packed, k, ao, fall, pos, nrm, W, H)
            dc.same_planes(got, dc.distance_rule(packed, k, ao, fall, pos, nrm)[:3], ("quad", n, table))
            # every segment leaves the surface upwards: free, +Inf, n * S -- whatever the falloff
            assert (got[0][live] == n).all() and (dc.bits(got[1])[live] == dc.INF_BITS).all() and (got[2][live] == n * (65535 // n)).all()


def test_refusals_guards_and_rows():
    fr = ac.frame("cornell_128", 17, 5)
    W, H = fr.W, fr.H
    lib, ptr = api._lib, api._ptr
    pos, nrm = np.ascontiguousarray(fr.pos), np.ascontiguousarray(fr.nrm)
    packed = np.ascontiguousarray(fr.packed)
    buf = np.full(W * H + 64, ac.GUARD, np.uint8)
    counts = buf[32:32 + W * H]
    fbuf = np.full(W * H + 64, np.frombuffer(bytes([ac.GUARD] * 4), f32)[0], f32)
    dist = fbuf[32:32 + W * H]
    sbuf = np.full(W * H + 64, 0xABAB, np.uint16)
    obs = sbuf[32:32 + W * H]
    good = fr.ao(4, 0, 0.5)
    fall = dc.falloff("saw")
    at = lambda a, off=0: C.c_void_p(a.ctypes.data + off) if a is not None else None

    def call(P=packed, K=fr.k, A=good, F=fall, X=pos, N=nrm, W_=W, H_=H, r0=0, r1=H, O=counts, D=dist, S=obs, d_off=0, s_off=0):
        return lib.rtsh_ambient_occlusion_distance(ptr(P) if P is not None else None, packed.shape[0], C.byref(K) if K is not None else None,
                                                   C.byref(A) if A is not None else None, C.byref(F) if F is not None else None,
                                                   ptr(X) if X is not None else None, ptr(N) if N is not None else None, None, W_, H_, r0, r1,
                                                   at(O), at(D, d_off), at(S, s_off), 0)

    def bad(**fields):
        a = fr.ao(4, 0, 0.5)
        for name, v in fields.items():
            setattr(a, name, v)
        return a

    for kw in (dict(P=None), dict(K=None), dict(A=None), dict(X=None), dict(N=None), dict(D=None, S=None), dict(F=None), dict(s_off=1),
               dict(d_off=1), dict(d_off=2), dict(d_off=3), dict(W_=0), dict(H_=0), dict(r0=3, r1=2), dict(r1=H + 1),
               dict(A=bad(nsamples=49)), dict(A=bad(table=3)), dict(A=bad(table=65)), dict(A=bad(nsamples=1, table=1)),
               dict(A=bad(nsamples=1, table=8)), dict(A=bad(radius=np.inf)), dict(A=bad(radius=-np.inf)), dict(A=bad(radius=np.nan))):
        assert call(**kw) == ac.INVALID, kw
    assert (buf == ac.GUARD).all() and (dc.bits(fbuf) == 0xABABABAB).all() and (sbuf == 0xABAB).all()
    assert call(r0=1, r1=3) == 0
    want_c, want_d, want_s = dc.want(fr, 4, 0, 0.5, "saw")
    c2, d2, s2 = counts.reshape(H, W), dist.reshape(H, W), obs.reshape(H, W)
    dc.same_planes((c2[1:3], d2[1:3], s2[1:3]), (want_c[1:3], want_d[1:3], want_s[1:3]), "rows 1..3")
    for plane, fill in ((c2, ac.GUARD), (dc.bits(d2), 0xABABABAB), (s2, 0xABAB)):
        assert (plane[0] == fill).all() and (plane[3:] == fill).all()
    assert (buf[:32] == ac.GUARD).all() and (buf[32 + W * H:] == ac.GUARD).all()
    assert (dc.bits(fbuf[:32]) == 0xABABABAB).all() and (dc.bits(fbuf[32 + W * H:]) == 0xABABABAB).all()
    assert (sbuf[:32] == 0xABAB).all() and (sbuf[32 + W * H:] == 0xABAB).all()
    assert call(r0=2, r1=2) == 0
    assert call(O=None) == 0 and call(D=None) == 0 and call(S=None) == 0 and call(S=None, F=None) == 0   # each plane is optional
    zero = api.ambient_occlusion_distance(packed, fr.k, bad(nsamples=0), fall, pos, nrm, W, H)
    dc.same_planes(zero, api.ambient_occlusion_distance(packed, fr.k, bad(nsamples=1), fall, pos, nrm, W, H), "nsamples 0 counts as 1")
    assert C.sizeof(api.AoFalloff) == 64


def test_falloff_constructors():
    lin, quad, zeros = api.AoFalloff.linear().weights(), api.AoFalloff.quadratic().weights(), api.AoFalloff.zeros().weights()
    centres = (np.arange(64) + 0.5) / 64.0
    assert np.array_equal(lin, np.rint(centres * 255.0).astype(np.uint8)) and (zeros == 0).all()
    assert np.array_equal(quad, np.rint((1.0 - (1.0 - centres) ** 2) * 255.0).astype(np.uint8))
    assert (np.diff(lin.astype(int)) >= 0).all() and (np.diff(quad.astype(int)) >= 0).all() and (quad >= lin).all()
    assert np.array_equal(api.AoFalloff.make(lambda t: 7.0).weights(), np.full(64, 255, np.uint8))       # clipped to [0, 1]
    assert np.array_equal(api.AoFalloff.make(np.arange(64)).weights(), np.arange(64, dtype=np.uint8))
    for wrong in (np.zeros(63), np.full(64, 256), np.full(64, -1)):
        with pytest.raises(api.RtsError):
            api.AoFalloff.make(wrong)


def test_twin_under_the_sanitizers(tmp_path):
    """tests/cpp/ao_distance_host.cpp: rtsh_ambient_occlusion_distance (rts_scene.cpp and the shared per-sample source, compiled into
    the program -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined over small frames in exact-size heap
    blocks, and the bin edges k / 64 with their predecessors on the shared function itself."""
    exe = str(tmp_path / "ao_distance_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "ao_distance_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100, run.stdout[-2000:]
