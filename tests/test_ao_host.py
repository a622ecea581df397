"""CPU: ambient occlusion on the host (include/rts_scene.h: rtsh_ambient_occlusion, rtsh_ao_rays, rtsh_combine_visibility_list_ao;
DESIGN.md 4.34).  The rays against the numpy restatement of the header (tests/ao_cases.py), bit for bit; the twin's counts against the
oracle's any-hit over those rays and against the oracle's shadow mask for the hard point light at L_j(p); a ground quad; every
refusal, guard bytes and rows outside the range; the count plane under the stand-in list through the R = 0 filter, the wide filter
and the moments pass; the AO combine; and the twin and rtsh_ao_rays under the host sanitizers (tests/cpp/ao_host.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ao_cases as ac
import list_moments_cases as mc
import list_wide_filter_cases as wc
import oracle
from raytracedshadows_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module", params=ac.FRAMES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}")
def fr(request):
    return ac.frame(*request.param)


# --------------------------------------------------------------------------------------------------------------------------- the rays
def test_ao_rays_equal_the_numpy_rule_bit_for_bit(fr):
    cases = [(n, t, r, None) for n, t, r in ac.param_cases() if (n, r) in ((1, 0.05), (3, 0.5), (5, 10.0), (48, 0.5))]
    cases += [(16, 64, 0.5, "below"), (4, 0, 0.05, "below")]
    for n, table, share, dirs_key in cases:
        ao = fr.ao(n, table, share, dirs=None if dirs_key is None else ac.below_horizon_dirs())
        for masked in (False, True):
            pos, act = (fr.dirty, fr.active) if masked else (fr.pos, None)
            got = api.ao_rays(fr.k, ao, pos, fr.nrm, fr.W, fr.H, active=act)
            want = ac.rays_rule(fr.k, ao, pos, fr.nrm, act)
            bad = np.argwhere(_bits(got) != _bits(want))
            assert bad.shape[0] == 0, (n, table, share, dirs_key, masked, bad[:4].tolist())
            live = ~fr.background & ((fr.active != 0) if masked else True)
            per_pixel = _bits(got).reshape(fr.H, fr.W, -1)
            assert (per_pixel[~live] == 0).all()                         # 32 zero bytes per ray of a pixel that sends none
            assert np.isfinite(got.reshape(fr.H, fr.W, -1)[live]).all() or dirs_key is not None


def test_special_normals_give_finite_orthonormal_frames():
    """N.z of +0, -0, exactly -1 and exactly +1 through the LIBRARY: with the unit axes as directions and radius 1, the segments of
    rtsh_ao_rays are T, B and N up to the bias (2^-13 of the origin's size), so they are finite, of unit length and orthogonal."""
    special = np.array([(0.6, 0.8, 0.0), (0.6, 0.8, -0.0), (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)], f32)
    assert np.signbit(special[1, 2]) and not np.signbit(special[0, 2])
    nrm = np.zeros((1, 4, 4), f32)
    nrm[0, :, :3] = special
    pos = np.zeros((1, 4, 4), f32)
    pos[0, :, :3] = [(0.5, -1.0, 0.25), (-0.5, 1.0, 0.75), (1.0, 0.5, -0.5), (-1.0, -0.5, 0.5)]
    k = api.RayTracingConstants.make((0.25, 0.5, -0.75), (0.0, -1.0, 0.0), 4, 1)
    ao = api.AoParams.make(3, 1.0, dirs=np.eye(3, dtype=f32))
    rays = api.ao_rays(k, ao, pos, nrm, 4, 1)
    assert np.array_equal(_bits(rays), _bits(ac.rays_rule(k, ao, pos, nrm)))
    d = rays.reshape(4, 3, 8)[..., 4:7].astype(np.float64)            # per pixel: T, B, N (less the bias along each)
    assert np.isfinite(rays).all()
    assert np.abs(np.linalg.norm(d, axis=-1) - 1).max() < 1e-3
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert np.abs((d[:, a] * d[:, b]).sum(-1)).max() < 1e-3
    assert np.abs(d[:, 2] - special).max() < 1e-3                       # the third direction is the normal itself


# ---------------------------------------------------------------------------------------------------------------------- exact anchors
def test_twin_counts_are_the_oracles_any_hit_sums(fr):
    mixed = 0
    for n, table, share in ((1, 0, 0.05), (5, 64, 0.5), (16, 16, 10.0), (48, 0, 0.05)):
        for masked in (False, True):
            ao = fr.ao(n, table, share)
            pos, act = (fr.dirty, fr.active) if masked else (fr.pos, None)
            rays = api.ao_rays(fr.k, ao, pos, fr.nrm, fr.W, fr.H, active=act)
            unoccluded, _, _ = oracle.trace_rays(fr.packed, rays)
            live = ~fr.background & ((fr.active != 0) if masked else True)
            want = np.where(live, unoccluded.reshape(fr.H, fr.W, n).sum(-1), 0).astype(np.uint8)
            got = fr.want(n, table, share, masked)
            assert np.array_equal(got, want), (n, table, share, masked, np.argwhere(got != want)[:4].tolist())
            mixed += 0 < int(got[live].astype(int).sum()) < n * int(live.sum())
    assert mixed >= 2 or fr.W * fr.H < 100, "every segment agrees in nearly every case: the cases check nothing"


def test_exact_L_gives_the_shadow_mask_ray():
    """The header's L itself (from the numpy rule) as a hard point light: the oracle's ray for it is the AO ray bit for bit, and the
    shadow bytes of that light -- the oracle's and the library's own host shadow path (rtsh_shadow_distance's mask, the byte
    rts_trace_shadow_mask* writes) -- summed over the samples are the twin's count: the AO sample IS that light's shadow ray."""
    fr = ac.frame("terrain_96", 40, 36)
    n, table, share = 4, 4, 0.5
    ao = fr.ao(n, table, share)
    got = fr.want(n, table, share)
    rays = ac.rays_rule(fr.k, ao, fr.pos, fr.nrm).reshape(fr.H, fr.W, n, 8)
    ys, xs = np.nonzero(~fr.background)
    py, px = np.nonzero(~fr.background & (got > 0) & (got < n))          # half of the subsample: partly occluded pixels
    assert py.size >= 6
    picks = [(int(ys[i]), int(xs[i])) for i in range(0, ys.size, max(1, ys.size // 6))][:6]
    picks += [(int(py[i]), int(px[i])) for i in range(0, py.size, max(1, py.size // 6))][:6]
    mixed = 0
    for y, x in picks:
        texel = fr.pos[y:y + 1, x:x + 1]
        total = own = 0
        for j in range(n):
            L = ac.aim_rule(fr.k, ao, fr.pos, fr.nrm, y, x, j)
            light = oracle.make_light(1, L)
            o4 = oracle.gen_rays(fr.k.as_array(), light, texel).reshape(-1, 8)[0]
            assert np.array_equal(_bits(o4[:7]), _bits(rays[y, x, j][:7])), (y, x, j)
            mask, _, _ = oracle.shadow_mask(fr.packed, fr.k.as_array(), light, texel, 1, 1)
            total += int(mask[0, 0])
            _, lib_mask = api.shadow_distance(fr.packed, fr.k, api.Light.make(api.Light.POINT, L), texel, 1, 1)
            own += int(lib_mask[0, 0])
        assert total == int(got[y, x]) and own == int(got[y, x]), (y, x, total, own, int(got[y, x]))
        mixed += 0 < total < n
    assert mixed > 0


def test_ground_quad_is_fully_open_for_every_table():
    packed, k, pos, nrm = ac.ground_quad()
    H, W = pos.shape[:2]
    for n in ac.NSAMPLES:
        for table in ac.tables(n):
            ao = api.AoParams.make(n, 2.0, table=table, seed=n)
            got = api.ambient_occlusion(packed, k, ao, pos, nrm, W, H)
            bg = (nrm[..., :3] == 0).all(-1)
            assert (got[~bg] == n).all() and (got[bg] == 0).all(), (n, table)


# ------------------------------------------------------------------------------------------------- refusals, guards, rows, make
def test_refusals_guards_and_rows():
    fr = ac.frame("cornell_128", 17, 5)
    W, H = fr.W, fr.H
    lib, ptr = api._lib, api._ptr
    pos, nrm = np.ascontiguousarray(fr.pos), np.ascontiguousarray(fr.nrm)
    packed = np.ascontiguousarray(fr.packed)
    buf = np.full(W * H + 64, ac.GUARD, np.uint8)
    counts = buf[32:32 + W * H]
    good = fr.ao(4, 0, 0.5)

    def call(P=packed, K=fr.k, A=good, X=pos, N=nrm, W_=W, H_=H, r0=0, r1=H, O=counts):
        return lib.rtsh_ambient_occlusion(ptr(P) if P is not None else None, packed.shape[0], C.byref(K) if K is not None else None,
                                          C.byref(A) if A is not None else None, ptr(X) if X is not None else None,
                                          ptr(N) if N is not None else None, None, W_, H_, r0, r1, ptr(O) if O is not None else None, 0)

    def bad(**fields):
        a = fr.ao(4, 0, 0.5)
        for name, v in fields.items():
            setattr(a, name, v)
        return a

    for kw in (dict(P=None), dict(K=None), dict(A=None), dict(X=None), dict(N=None), dict(O=None), dict(W_=0), dict(H_=0), dict(r0=3, r1=2),
               dict(r1=H + 1), dict(A=bad(nsamples=49)), dict(A=bad(table=3)), dict(A=bad(table=65)), dict(A=bad(nsamples=1, table=1)),
               dict(A=bad(nsamples=1, table=8)), dict(A=bad(radius=np.inf)), dict(A=bad(radius=-np.inf)), dict(A=bad(radius=np.nan))):
        assert call(**kw) == ac.INVALID, kw
    assert (buf == ac.GUARD).all()
    rays = np.zeros((W * H * 4, 8), f32)
    for a in (None, bad(nsamples=49), bad(table=3), bad(radius=np.nan)):
        assert lib.rtsh_ao_rays(C.byref(fr.k), C.byref(a) if a is not None else None, ptr(pos), ptr(nrm), None, W, H, ptr(rays)) == ac.INVALID
    assert lib.rtsh_ao_rays(C.byref(fr.k), C.byref(good), ptr(pos), ptr(nrm), None, W, H, None) == ac.INVALID
    assert not rays.any()
    # rows 1..3 alone are written, the guard bytes around the plane stay, nsamples 0 counts as 1, a negative radius is legal
    assert call(r0=1, r1=3) == 0
    want = fr.want(4, 0, 0.5)
    assert (counts.reshape(H, W)[1:3] == want[1:3]).all() and (counts.reshape(H, W)[0] == ac.GUARD).all()
    assert (counts.reshape(H, W)[3:] == ac.GUARD).all() and (buf[:32] == ac.GUARD).all() and (buf[32 + W * H:] == ac.GUARD).all()
    assert call(r0=2, r1=2) == 0
    one = api.ambient_occlusion(packed, fr.k, bad(nsamples=0), pos, nrm, W, H)
    assert np.array_equal(one, api.ambient_occlusion(packed, fr.k, bad(nsamples=1), pos, nrm, W, H))
    assert api.ambient_occlusion(packed, fr.k, bad(radius=-0.5), pos, nrm, W, H).shape == (H, W)
    assert C.sizeof(api.AoParams) == 1040


def test_make_is_deterministic_cosine_weighted_and_above_the_horizon():
    a, b = api.AoParams.make(16, 0.5, table=64, seed=7), api.AoParams.make(16, 0.5, table=64, seed=7)
    d = a.dirs_array()
    assert np.array_equal(_bits(d), _bits(b.dirs_array())) and not np.array_equal(d, api.AoParams.make(16, 0.5, table=64, seed=8).dirs_array())
    assert (d[:, 2] > 0).all() and np.abs(np.linalg.norm(d[:, :3].astype(np.float64), axis=1) - 1).max() < 1e-6
    # stratified: exactly one sample in each of the 64 equal-area rings of the disc (z^2 = 1 - u), and in each of the 64 azimuth sectors
    ring = np.floor((1.0 - d[:, 2].astype(np.float64) ** 2) * 64 + 1e-4).astype(int)
    sector = np.floor((np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) % 1.0) * 64 + 1e-4).astype(int)
    assert sorted(np.clip(ring, 0, 63)) == list(range(64)) and sorted(np.clip(sector, 0, 63)) == list(range(64))
    assert abs(float(d[:, 2].mean()) - 2.0 / 3.0) < 0.02                  # cosine-weighted: E[z] = 2/3
    lst = a.stand_in_list()
    assert lst.count == 1 and lst.lights[0].nsamples == 16
    assert api.AoParams.make(0, 1.0).stand_in_list().lights[0].nsamples == 1


# ------------------------------------------------------------------------------------------------ downstream under the stand-in list
def test_the_filters_and_the_moments_pass_take_the_plane_under_the_stand_in_list():
    fr = ac.frame("cornell_128", 48, 40)
    n = 16
    ao = fr.ao(n, 64, 0.5)
    counts = fr.want(n, 64, 0.5)[None]
    lst = ao.stand_in_list()
    vis = api.filter_soft_light_list(lst, api.FilterParams.make(0, 0.9, 0.05), fr.pos, fr.nrm, counts)
    want = np.where(fr.background, f32(0), counts[0].astype(f32) / f32(n))
    assert np.array_equal(_bits(vis[0]), _bits(want))
    assert 0 < float(vis[0][~fr.background].mean()) < 1
    # the wide filter, every pass count, against its numpy rule
    rule = wc.wide_filter_rule(lst, api.WideFilterParams.make(0, 0.9, 0.05), fr.pos, fr.nrm, counts, None)
    for passes in (0, 1, 3, 5):
        got = api.wide_filter_soft_light_list(lst, api.WideFilterParams.make(passes, 0.9, 0.05), fr.pos, fr.nrm, counts)
        wc.same_bits(got, rule[passes], passes)
    assert (rule[3] != rule[0]).any()
    # the moments pass (first frame), against its numpy rule
    p = api.TemporalParams.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, -1), 1.0, 1.0)
    mc.same_moments(api.accumulate_moments_soft_light_list(lst, p, fr.pos, fr.nrm, counts), mc.moments_rule(lst, p, fr.pos, fr.nrm, counts),
                    "first frame")


# ------------------------------------------------------------------------------------------------------------------- the AO combine
def test_ao_combine_equals_its_rule_and_with_ones_the_plain_combine():
    k, lst, pos, nrm, vis, plane, lights_map, colors = ac.combine_case()
    for m, c in ((None, None), (lights_map, colors)):
        got = api.combine_visibility_list_ao(k, lst, pos, nrm, vis, plane, lights_map=m, colors=c)
        want = ac.combine_ao_rule(k, lst, pos, nrm, vis, plane, m, c)
        assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
        ones = api.combine_visibility_list_ao(k, lst, pos, nrm, vis, np.ones_like(plane), lights_map=m, colors=c)
        plain = api.combine_visibility_list(k, lst, pos, nrm, vis, lights_map=m, colors=c)
        assert np.array_equal(ones, plain)
        assert (got != plain).any()
    rgb = np.full((nrm.shape[0], nrm.shape[1], 3), ac.GUARD, np.uint8)
    st = api._lib.rtsh_combine_visibility_list_ao(C.byref(k), C.byref(lst), None, api._ptr(np.ascontiguousarray(pos)),
                                                  api._ptr(np.ascontiguousarray(nrm)), None, api._ptr(vis), None, nrm.shape[1], nrm.shape[0],
                                                  api._ptr(rgb))
    assert st == ac.INVALID and (rgb == ac.GUARD).all()


# ------------------------------------------------------------------------------------------------------------------- the sanitizers
def test_twin_and_rays_under_the_sanitizers(tmp_path):
    """tests/cpp/ao_host.cpp: rtsh_ambient_occlusion and rtsh_ao_rays (rts_scene.cpp and the shared per-pixel source, compiled into the
    program -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined over small frames in exact-size heap blocks."""
    exe = str(tmp_path / "ao_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "ao_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100, run.stdout[-2000:]
