"""CPU: bent normals on the host (include/rts_scene.h: rtsh_ambient_occlusion_bent, rtsh_combine_visibility_list_ao_bent; DESIGN.md
4.36).  The twin against the numpy rule of tests/ao_bent_cases.py (the oracle's any-hit over the numpy rays, Q, integer sums, the frame
once), bit for bit, on every frame of ao_cases with n of 1, 3, 4, 5, 16, 48 and tables 0, n and 64; Q on the header's awkward values
through the library; below-horizon directions and the ground quad; full and empty pixels; the guard that the frames hold partly free
pixels, from the oracle alone; refusals, guard bytes and rows; the bent combine against its rule, with both anchors; and the twin and
the combine under the host sanitizers (tests/cpp/ao_bent_host.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ao_bent_cases as bc
import ao_cases as ac
from raytracedshadows_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NS = (1, 3, 4, 5, 16, 48)
SHARES = {1: 0.05, 3: 0.5, 4: 0.5, 5: 10.0, 16: 0.5, 48: 0.05}


@pytest.fixture(scope="module", params=ac.FRAMES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}")
def fr(request):
    return ac.frame(*request.param)


def _twin(fr, n, table, share, masked=False, dirs_key=None, **kw):
    ao = fr.ao(n, table, share, dirs=None if dirs_key is None else ac.below_horizon_dirs())
    pos, act = (fr.dirty, fr.active) if masked else (fr.pos, None)
    return api.ambient_occlusion_bent(fr.packed, fr.k, ao, pos, fr.nrm, fr.W, fr.H, active=act, **kw)


def test_twin_equals_the_rule_bit_for_bit(fr):
    mixed = 0
    for n in NS:
        for table in ac.tables(n):
            for masked in (False, True):
                share = SHARES[n]
                counts, bent = _twin(fr, n, table, share, masked)
                want_c, want_b, S = bc.want(fr, n, table, share, masked)
                assert np.array_equal(counts, want_c), (n, table, masked, np.argwhere(counts != want_c)[:4].tolist())
                bc.same_bent(bent, want_b, (n, table, masked))
                assert np.array_equal(bc.bits(bent[..., 3]), bc.bits(counts.astype(f32)))
                assert np.array_equal(counts, fr.want(n, table, share, masked))       # byte for byte the AO twin's plane
                live = bc.live_of(fr.nrm, fr.active if masked else None)
                assert (bc.bits(bent[~live]) == 0).all() and (counts[~live] == 0).all()
                mixed += bool(((counts > 0) & (counts < n)).any())
    assert mixed >= 2 or fr.W * fr.H < 100, "no partly free pixel in nearly every case: the cases check all-free sums alone"


def test_counts_null_gives_the_same_bent(fr):
    counts, bent = _twin(fr, 5, 64, 0.5)
    none, alone = _twin(fr, 5, 64, 0.5, want_counts=False)
    assert none is None and np.array_equal(bc.bits(alone), bc.bits(bent))


def test_guard_partly_free_and_fully_free_pixels_by_the_oracle_alone():
    share, partly, full = bc.guard_radius()
    print(f"guard: radius {share} of the diagonal: {partly} pixels with 0 < c < 16, {full} with c == 16")
    assert partly >= 32 and full >= 32, (share, partly, full)
    fr = ac.frame("cornell_128", 48, 40)
    counts, bent = _twin(fr, 16, 0, share)
    want_c, want_b, _ = bc.want(fr, 16, 0, share)
    assert np.array_equal(counts, want_c)
    bc.same_bent(bent, want_b, "the guard's case")


def test_full_and_empty_pixels(fr):
    """c == n: the frame applied to the table's full sum; c == 0: the frame applied to the zero sum through the written operations --
    every component a zero (its sign is the operations': -0 where all three products are -0)."""
    seen_full = seen_zero = 0
    for n, table, share in ((4, 0, 0.05), (16, 16, 10.0), (5, 64, 10.0), (48, 0, 0.5)):
        counts, bent = _twin(fr, n, table, share)
        live = ~fr.background
        q = bc.quantise_rule(fr.ao(n, table, share).dirs_array()[:, :3])
        total = q[:table or n].sum(0) if table in (0, n) else None
        full, zero = live & (counts == n), live & (counts == 0)
        if total is not None:
            S = np.broadcast_to(total, (fr.H, fr.W, 3))
            w = bc.bent_from_sum(fr.nrm, S, np.full((fr.H, fr.W), n), live)
            assert np.array_equal(bc.bits(bent[full]), bc.bits(w[full]))
        w0 = bc.bent_from_sum(fr.nrm, np.zeros((fr.H, fr.W, 3), np.int64), np.zeros((fr.H, fr.W), np.int64), live)
        assert np.array_equal(bc.bits(bent[zero]), bc.bits(w0[zero])) and (bent[zero] == 0).all()
        seen_full += int(full.sum()); seen_zero += int(zero.sum())
    # (the open terrain has no closed pixel at any of these radii; the closed box of cornell_128 has)
    assert (seen_full > 0 and (seen_zero > 0 or fr.name != "cornell_128")) or fr.W * fr.H < 100, (seen_full, seen_zero)


def test_quantise_rule_on_awkward_values():
    """NaN, +-Inf, +-0, +-1, 1.5, 2^-15 and 3 * 2^-15 (ties) and a denormal as the x and y of single directions over the ground quad,
    z = 1 (the segment leaves the surface upwards); at N = (0, 1, 0) the frame is T = (1, 0, -0), B = (0, 0, -1): bent = (f.x, f.z,
    -f.y) of the sample where it is free.  Whatever the ray of such a direction meets, the twin equals the rule."""
    packed, k, pos, nrm = ac.ground_quad()
    H, W = pos.shape[:2]
    values = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 1.5, 2.0 ** -15, 3 * 2.0 ** -15, -3 * 2.0 ** -15, 1e-40, 0.25]
    want_q = [0, 16384, -16384, 0, 0, 16384, -16384, 16384, 0, 2, -2, 0, 4096]
    assert bc.quantise_rule(np.array(values, f32)).tolist() == want_q
    finite_free = 0
    for v, q in zip(values, want_q):
        for axis in (0, 1):
            d = np.zeros((1, 3), f32)
            d[0, 2] = 1.0
            d[0, axis] = v
            ao = api.AoParams.make(1, 2.0, dirs=d)
            counts, bent = api.ambient_occlusion_bent(packed, k, ao, pos, nrm, W, H)
            want_c, want_b, S = bc.bent_rule(packed, k, ao, pos, nrm)
            assert np.array_equal(counts, want_c), (v, axis)
            bc.same_bent(bent, want_b, (v, axis))
            free = counts == 1
            if np.isfinite(v):
                assert free[bc.live_of(nrm)].all(), (v, axis)
                finite_free += 1
            if free.any():
                got = bent[free][0]
                assert got[1] == 1.0 and got[3] == 1.0                  # Q(1.0) * 2^-14 along the normal
                assert (got[0] if axis == 0 else -got[2]) == q * 2.0 ** -14, (v, axis, got.tolist())
                assert (S[free][0].tolist()[axis], S[free][0].tolist()[2]) == (q, 16384)
    assert finite_free == 2 * sum(np.isfinite(values))


def test_below_horizon_dirs_and_ground_quad():
    fr = ac.frame("terrain_96", 40, 36)
    for n, table in ((16, 64), (4, 0)):
        counts, bent = _twin(fr, n, table, 0.5, dirs_key="below")
        want_c, want_b, _ = bc.want(fr, n, table, 0.5, dirs_key="below")
        assert np.array_equal(counts, want_c)
        bc.same_bent(bent, want_b, ("below", n, table))
    packed, k, pos, nrm = ac.ground_quad()
    H, W = pos.shape[:2]
    for n in NS:
        for table in ac.tables(n):
            ao = api.AoParams.make(n, 2.0, table=table, seed=n)
            counts, bent = api.ambient_occlusion_bent(packed, k, ao, pos, nrm, W, H)
            want_c, want_b, _ = bc.bent_rule(packed, k, ao, pos, nrm)
            live = bc.live_of(nrm)
            assert (counts[live] == n).all() and np.array_equal(counts, want_c)
            bc.same_bent(bent, want_b, ("quad", n, table))
            assert (bent[live][:, 1] > 0).all()                          # every free direction has z > 0: the sum points up


def test_refusals_guards_and_rows():
    fr = ac.frame("cornell_128", 17, 5)
    W, H = fr.W, fr.H
    lib, ptr = api._lib, api._ptr
    pos, nrm = np.ascontiguousarray(fr.pos), np.ascontiguousarray(fr.nrm)
    packed = np.ascontiguousarray(fr.packed)
    buf = np.full(W * H + 64, ac.GUARD, np.uint8)
    counts = buf[32:32 + W * H]
    fbuf = np.full((W * H + 16) * 4, bc.GUARD_F32, f32)
    bent = fbuf[32:32 + W * H * 4]
    good = fr.ao(4, 0, 0.5)

    def call(P=packed, K=fr.k, A=good, X=pos, N=nrm, W_=W, H_=H, r0=0, r1=H, O=counts, B=bent):
        return lib.rtsh_ambient_occlusion_bent(ptr(P) if P is not None else None, packed.shape[0], C.byref(K) if K is not None else None,
                                               C.byref(A) if A is not None else None, ptr(X) if X is not None else None,
                                               ptr(N) if N is not None else None, None, W_, H_, r0, r1, ptr(O) if O is not None else None,
                                               ptr(B) if B is not None else None, 0)

    def bad(**fields):
        a = fr.ao(4, 0, 0.5)
        for name, v in fields.items():
            setattr(a, name, v)
        return a

    for kw in (dict(P=None), dict(K=None), dict(A=None), dict(X=None), dict(N=None), dict(B=None), dict(W_=0), dict(H_=0), dict(r0=3, r1=2),
               dict(r1=H + 1), dict(A=bad(nsamples=49)), dict(A=bad(table=3)), dict(A=bad(table=65)), dict(A=bad(nsamples=1, table=1)),
               dict(A=bad(nsamples=1, table=8)), dict(A=bad(radius=np.inf)), dict(A=bad(radius=-np.inf)), dict(A=bad(radius=np.nan))):
        assert call(**kw) == ac.INVALID, kw
    assert (buf == ac.GUARD).all() and (bc.bits(fbuf) == 0xABABABAB).all()
    assert call(r0=1, r1=3) == 0
    want_c, want_b, _ = bc.want(fr, 4, 0, 0.5)
    c2, b2 = counts.reshape(H, W), bent.reshape(H, W, 4)
    assert (c2[1:3] == want_c[1:3]).all() and (c2[0] == ac.GUARD).all() and (c2[3:] == ac.GUARD).all()
    assert np.array_equal(bc.bits(b2[1:3]), bc.bits(want_b[1:3])) and (bc.bits(b2[0]) == 0xABABABAB).all() and (bc.bits(b2[3:]) == 0xABABABAB).all()
    assert (buf[:32] == ac.GUARD).all() and (buf[32 + W * H:] == ac.GUARD).all()
    assert (bc.bits(fbuf[:32]) == 0xABABABAB).all() and (bc.bits(fbuf[32 + W * H * 4:]) == 0xABABABAB).all()
    assert call(r0=2, r1=2) == 0
    assert call(O=None) == 0                                             # counts are optional
    one = api.ambient_occlusion_bent(packed, fr.k, bad(nsamples=0), pos, nrm, W, H)
    assert np.array_equal(bc.bits(one[1]), bc.bits(api.ambient_occlusion_bent(packed, fr.k, bad(nsamples=1), pos, nrm, W, H)[1]))
    assert C.sizeof(api.SkyAmbient) == 48


def test_bent_combine_equals_its_rule_and_both_anchors_hold():
    k, lst, pos, nrm, vis, plane, bent, sky, lights_map, colors = bc.combine_case()
    white = api.SkyAmbient.make(up=tuple(sky.up))
    for m, c in ((None, None), (lights_map, colors)):
        got = api.combine_visibility_list_ao_bent(k, lst, pos, nrm, vis, plane, bent, sky, lights_map=m, colors=c)
        want = bc.combine_ao_bent_rule(k, lst, pos, nrm, vis, plane, bent, sky, m, c)
        assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
        ao_only = api.combine_visibility_list_ao(k, lst, pos, nrm, vis, plane, lights_map=m, colors=c)
        assert (got != ao_only).any()
        # anchor 1: sky == ground == (1, 1, 1) gives the AO combine's bytes (and the AO combine's own numpy rule)
        ones = api.combine_visibility_list_ao_bent(k, lst, pos, nrm, vis, plane, bent, white, lights_map=m, colors=c)
        assert np.array_equal(ones, ao_only) and np.array_equal(ones, ac.combine_ao_rule(k, lst, pos, nrm, vis, plane, m, c))
        # anchor 2: an all-zero bent texel gives h = 0.5 -- the tint half way, whatever up is
        zero = np.zeros_like(bent)
        tint = bc.sky_tint_rule(sky, zero)
        half = [f32(sky.ground[i]) + (f32(sky.sky[i]) - f32(sky.ground[i])) * f32(0.5) for i in range(3)]
        assert (tint == np.array(half, f32)).all()
        flat = api.SkyAmbient.make(up=tuple(sky.up), sky=half, ground=half)
        assert np.array_equal(api.combine_visibility_list_ao_bent(k, lst, pos, nrm, vis, plane, zero, sky, lights_map=m, colors=c),
                              api.combine_visibility_list_ao_bent(k, lst, pos, nrm, vis, plane, bent, flat, lights_map=m, colors=c))
    rgb = np.full((nrm.shape[0], nrm.shape[1], 3), ac.GUARD, np.uint8)
    args = lambda b, s: (C.byref(k), C.byref(lst), None, api._ptr(np.ascontiguousarray(pos)), api._ptr(np.ascontiguousarray(nrm)), None,
                         api._ptr(vis), api._ptr(plane), b, s, nrm.shape[1], nrm.shape[0], api._ptr(rgb))
    assert api._lib.rtsh_combine_visibility_list_ao_bent(*args(None, C.byref(sky))) == ac.INVALID
    assert api._lib.rtsh_combine_visibility_list_ao_bent(*args(api._ptr(bent), None)) == ac.INVALID
    assert (rgb == ac.GUARD).all()


def test_twin_and_combine_under_the_sanitizers(tmp_path):
    """tests/cpp/ao_bent_host.cpp: rtsh_ambient_occlusion_bent and rtsh_combine_visibility_list_ao_bent (rts_scene.cpp and the shared
    per-pixel source, compiled into the program -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined over small
    frames in exact-size heap blocks."""
    exe = str(tmp_path / "ao_bent_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "ao_bent_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100, run.stdout[-2000:]
