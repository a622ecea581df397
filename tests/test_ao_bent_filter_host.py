"""CPU: the host twin of the wide filter of the bent plane (rtsh_wide_filter_bent) against the numpy rule of
tests/ao_bent_filter_cases.py, bit for bit -- and what pins the rule: the six anchors, synthetic planes of awkward floats, traced planes
from the numpy rule of the bent trace, the guard that says the traced frame exercises the filter, `out` and `ao` inside guard bytes,
every refusal, and the twin under the address and UB sanitizers (tests/cpp/ao_bent_filter_host.cpp, a program of its own)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ao_bent_cases as bc
import ao_bent_filter_cases as bf
import list_wide_filter_cases as wc
import scene_pass_cases as sp
from raytracedshadows_amd import api

f32 = np.float32
INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("wh", wc.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twin_equals_the_numpy_rule(wh):
    """Awkward, geometric and (at the sizes the wide filter adds) flat frames; n of 1, 4, 16 and 48; with and without `active`;
    passes 0 .. 5; synthetic bent planes: NaN, +-Inf, +-0, values beyond +-n, ties, a denormal, .w non-integer or above n."""
    for kind in wc.kinds(wh):
        nrm, pos, _, _, lights_map, _ = wc.frame(kind, wh)
        for n in bf.SAMPLES:
            bent = bf.synthetic_bent(wh, n)
            for active in (None, bf.active_map(lights_map)):
                want = bf.bent_filter_rule(bf.params(0, kind), n, pos, nrm, bent, active)
                for passes in bf.PASSES:
                    out, ao = api.wide_filter_bent(bf.params(passes, kind), n, pos, nrm, bent, active)
                    bf.same_bits(out, want[passes], (kind, wh, n, active is not None, passes))
                    bf.same_bits(ao, want[passes][..., 3], (kind, wh, n, active is not None, passes, "ao"))


def test_the_synthetic_planes_hold_what_they_promise():
    """Exact ties, NaN, both infinities, both zeros, a denormal and values beyond +-n in xyz; a non-integer, a value above n, a negative
    one and a NaN in .w -- and nsamples == 0 behaves as 1."""
    for n in bf.SAMPLES:
        b = bf.synthetic_bent((72, 72), n)
        xyz, w = b[..., :3], b[..., 3]
        assert bf.exact_ties(b, n) >= 32, n
        assert np.isnan(xyz).any() and (xyz == np.inf).any() and (xyz == -np.inf).any() and (np.abs(xyz[np.isfinite(xyz)]) > n).any()
        assert ((xyz == 0) & np.signbit(xyz)).any() and ((xyz == 0) & ~np.signbit(xyz)).any() and (np.abs(xyz) == f32(1e-41)).any()
        assert np.isnan(w).any() and (w > n).any() and (w < 0).any() and (w != np.rint(w))[np.isfinite(w)].any()
    nrm, pos, _, _, lights_map, _ = wc.frame("geometric", (40, 72))
    b = bf.synthetic_bent((40, 72), 1)
    for passes in (0, 3):
        zero, one = (api.wide_filter_bent(bf.params(passes), n, pos, nrm, b, lights_map)[0] for n in (0, 1))
        bf.same_bits(zero, one, passes)


@pytest.mark.parametrize("case", [("cornell_128", 48, 40), ("terrain_96", 40, 36)], ids=lambda c: c[0])
def test_traced_planes(case):
    """Bent planes from ao_bent_cases.bent_rule: the twin equals the rule, and ANCHOR 1 -- out.w and ao equal, bit for bit, the wide
    filter of the trace's own counts under AoParams.stand_in_list() with a map of 0 / 1 bytes, for every passes."""
    for n, table in ((4, 64), (16, 0), (48, 0)):
        fr, ao, counts, bent = bf.traced(*case, n, table, 0.05)
        for active in (None, fr.active):
            act_counts, act_bent = counts, bent
            if active is not None:                                            # what the trace writes under the map: zeros
                act_counts = np.where(active != 0, counts, 0).astype(np.uint8)
                act_bent = np.where((active != 0)[..., None], bent, f32(0)).astype(f32)
            want = bf.bent_filter_rule(bf.traced_params(fr, 0), n, fr.pos, fr.nrm, act_bent, active)
            map01 = None if active is None else (active != 0).astype(np.uint8)
            for passes in bf.PASSES:
                p = bf.traced_params(fr, passes)
                out, plane = api.wide_filter_bent(p, n, fr.pos, fr.nrm, act_bent, active)
                bf.same_bits(out, want[passes], (case, n, passes))
                shipped = api.wide_filter_soft_light_list(ao.stand_in_list(), p, fr.pos, fr.nrm, act_counts[None], map01)
                bf.same_bits(out[..., 3], shipped[0], (case, n, passes, "anchor 1: out.w"))
                bf.same_bits(plane, shipped[0], (case, n, passes, "anchor 1: ao"))


def test_anchor_1_on_synthetic_frames_with_a_map():
    """Anchor 1 where the counts are arbitrary bytes and the map has holes: .w = the byte (bytes above n included)."""
    for kind in wc.KINDS:
        nrm, pos, planes, _, lights_map, _ = wc.frame(kind, (72, 40))
        for n in bf.SAMPLES:
            counts = planes[3]
            bent = np.array(bf.synthetic_bent((72, 40), n))
            bent[..., 3] = counts
            active = bf.active_map(lights_map)
            lst = api.AoParams.make(n, 1.0).stand_in_list()
            for passes in bf.PASSES:
                p = bf.params(passes, kind)
                out, ao = api.wide_filter_bent(p, n, pos, nrm, bent, active)
                shipped = api.wide_filter_soft_light_list(lst, p, pos, nrm, counts[None], (active != 0).astype(np.uint8))
                bf.same_bits(ao, shipped[0], (kind, n, passes))
                bf.same_bits(out[..., 3], shipped[0], (kind, n, passes))


def test_the_guard_holds_on_the_traced_frame():
    """From the rule alone, on the traced cornell frame at n = 4, table 64, passes = 3: at every pass at least 32 active pixels with a
    rejected in-frame tap and at least 32 with all in-frame taps accepted; at least 32 pixels that change a component by more than one
    quantum between X_0 and X_3; at least 32 negative components.  The first rung of the ladder holds."""
    rejected, full, moved, negative = bf.guard_counts(*bf.GUARD_LADDER[0])
    print("guard:", bf.GUARD_LADDER[0], rejected, full, moved, negative)
    assert rejected >= 32 and full >= 32 and moved >= 32 and negative >= 32, (rejected, full, moved, negative)


def test_anchor_negation():
    """Anchor 2: negating every bent.xyz negates every out.xyz exactly; a zero stays the +0 the division gives.  Against the rule."""
    for kind, wh, n in (("geometric", (72, 72), 4), ("awkward", (40, 72), 48), ("flat", (72, 40), 1)):
        nrm, pos, _, _, lights_map, _ = wc.frame(kind, wh)
        bent = bf.synthetic_bent(wh, n)
        neg = np.array(bent)
        neg[..., :3] = -neg[..., :3]
        want = bf.bent_filter_rule(bf.params(0, kind), n, pos, nrm, neg, lights_map)
        for passes in bf.PASSES:
            p = bf.params(passes, kind)
            plain = api.wide_filter_bent(p, n, pos, nrm, bent, lights_map)[0]
            flipped = api.wide_filter_bent(p, n, pos, nrm, neg, lights_map)[0]
            bf.same_bits(flipped, want[passes], (kind, passes, "the rule of the negated plane"))
            expect = plain.copy()
            expect[..., :3] = np.where(plain[..., :3] == 0, plain[..., :3], -plain[..., :3])
            bf.same_bits(flipped, expect, (kind, passes, "negation"))
            assert not np.signbit(flipped[flipped == 0]).any()
            assert (plain[..., :3] < 0).any() and (plain[..., :3] > 0).any()


def test_anchor_range():
    """Anchor 3: every X_(k+1).c lies between the smallest and the largest accepted X_k.c (the rule's planes, which the twin equals
    through its quotients: the division is monotonic); out.xyz stays in [-1, 1] and out.w in [0, 1]."""
    for kind in wc.KINDS:
        nrm, pos, _, _, lights_map, _ = wc.frame(kind, (72, 72))
        for n in (4, 48):
            bent = bf.synthetic_bent((72, 72), n)
            planes, census = [], {}
            want = bf.bent_filter_rule(bf.params(0, kind), n, pos, nrm, bent, lights_map, planes=planes, census=census)
            _, S_b, _ = bf.scales(n)
            for k in range(5):
                nxt = planes[k + 1][..., :3]
                assert (nxt >= census[k]["lo"]).all() and (nxt <= census[k]["hi"]).all(), (kind, n, k)
                out = api.wide_filter_bent(bf.params(k + 1, kind), n, pos, nrm, bent, lights_map)[0]
                bf.same_bits(out, want[k + 1], (kind, n, k))
                lo, hi = (c.astype(f32) / f32(n * S_b) for c in (census[k]["lo"], census[k]["hi"]))
                act = bf.active_of(nrm, lights_map)
                assert (out[..., :3][act] >= lo[act]).all() and (out[..., :3][act] <= hi[act]).all(), (kind, n, k)
                assert (np.abs(out[..., :3]) <= 1).all() and (out[..., 3] >= 0).all() and (out[..., 3] <= 1).all()


def test_anchor_no_neighbour_gives_the_passes_0_plane():
    """Anchor 4: thresholds that accept no neighbour give the passes == 0 plane at any passes."""
    for kind in ("awkward", "geometric"):
        nrm, pos, _, _, lights_map, _ = wc.frame(kind, (40, 72))
        for n in (4, 48):
            bent = bf.synthetic_bent((40, 72), n)
            for active in (None, bf.active_map(lights_map)):
                want = api.wide_filter_bent(bf.params(0, kind), n, pos, nrm, bent, active)[0]
                bf.same_bits(want, bf.bent_filter_rule(bf.params(0, kind), n, pos, nrm, bent, active, 0)[0], "passes 0")
                for closed in bf.CLOSED:
                    for passes in (1, 3, 5):
                        bf.same_bits(api.wide_filter_bent(closed(passes), n, pos, nrm, bent, active)[0], want, (kind, n, passes))


def test_anchor_equal_texels_give_that_texel():
    """Anchor 5: where every texel that can be accepted is the same, every pass returns it -- negative components included."""
    nrm, pos, _, _, lights_map, _ = wc.frame("geometric", (72, 72))
    for n, texel in ((4, (-3.3, 0.7, 1e-3, 3.0)), (48, (47.9, -48.0, -0.0, 17.0)), (1, (0.5000153, -1.0, 0.25, 1.0))):
        bent = np.broadcast_to(np.array(texel, f32), (72, 72, 4)).copy()
        want = api.wide_filter_bent(bf.params(0), n, pos, nrm, bent, lights_map)[0]
        for passes in (1, 3, 5):
            bf.same_bits(api.wide_filter_bent(bf.params(passes), n, pos, nrm, bent, lights_map)[0], want, (n, passes))


def test_anchor_combine_over_a_passes_0_plane():
    """Anchor 6: the bent combine over (ao, out) of a passes == 0 run gives the h of the raw plane wherever the raw vector quantises
    exactly -- here: vectors that are multiples of 1 / S_b times a power of two, where the tint of the rule is equal bit for bit.
    Not bit-equal in general: the direction is rounded to 1 / (n S_b); the bytes are not asserted."""
    k, lst, pos, nrm, vis, _, _, sky, lights_map, colors = bc.combine_case()
    H, W = nrm.shape[:2]
    n = 16
    _, S_b, _ = bf.scales(n)                                                 # 2047
    rs = np.random.RandomState(5)
    X = rs.randint(-n * S_b, n * S_b + 1, (H, W, 3))
    X[rs.random_sample((H, W)) < 0.1] = 0
    bent = np.zeros((H, W, 4), f32)
    bent[..., :3] = (X.astype(np.float64) / S_b).astype(f32)
    bent[..., 3] = rs.randint(0, n + 1, (H, W))
    exact = (bf.quantise_rule(bent, n, np.ones((H, W), bool))[..., :3] == X).all(-1)
    assert exact.sum() > exact.size // 2
    out, ao = api.wide_filter_bent(bf.params(0), n, pos, nrm, bent)
    act = bf.active_of(nrm)
    # out.xyz = X / (n S_b): the raw vector over n up to one rounding per component, so the normalised dot product -- h -- agrees to
    # float32 rounding (a few ulp), not to the bit
    raw, got = bc.sky_tint_rule(sky, bent), bc.sky_tint_rule(sky, out)
    where = exact & act
    assert np.abs(raw[where] - got[where]).max() <= 4e-6, np.abs(raw[where] - got[where]).max()
    rgb = api.combine_visibility_list_ao_bent(k, lst, pos, nrm, vis, ao, out, sky, lights_map, colors)
    want = bc.combine_ao_bent_rule(k, lst, pos, nrm, vis, ao, out, sky, lights_map, colors)
    assert (rgb == want).all()                                               # the combine takes the filtered planes as they are
    assert (ao[act] == (bent[..., 3] / f32(n))[act]).all()


def test_threads_change_nothing():
    nrm, pos, _, _, lights_map, _ = wc.frame("geometric", (72, 40))
    bent = bf.synthetic_bent((72, 40), 16)
    one = api.wide_filter_bent(bf.params(4), 16, pos, nrm, bent, lights_map, threads=1)
    seven = api.wide_filter_bent(bf.params(4), 16, pos, nrm, bent, lights_map, threads=7)
    bf.same_bits(seven[0], one[0], "7 threads")
    bf.same_bits(seven[1], one[1], "7 threads, ao")


def test_out_and_ao_inside_guard_bytes_and_unread_texels():
    """`out` and `ao` live inside larger blocks preset to 0xAB: nothing around them is written; ao may be NULL.  A background or inactive
    pixel's position and bent texel, and a background pixel's byte, are never looked at."""
    nrm, pos, _, _, lights_map, _ = (np.ascontiguousarray(a) for a in wc.frame("geometric", (17, 15)))
    n, W, H = 4, 17, 15
    bent, active = np.ascontiguousarray(bf.synthetic_bent((W, H), n)), bf.active_map(lights_map)
    p = bf.params(3)
    want = bf.bent_filter_rule(p, n, pos, nrm, bent, active)[3]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    block = np.full(64 + W * H * 16 + 64 + W * H * 4 + 64, 0xAB, np.uint8)
    out, ao = block[64:64 + W * H * 16], block[128 + W * H * 16:128 + W * H * 20]
    for with_ao in (True, False):
        block[:] = 0xAB
        assert api._lib.rtsh_wide_filter_bent(C.byref(p), n, ptr(pos), ptr(nrm), ptr(active), ptr(bent), W, H, ptr(out),
                                              ptr(ao) if with_ao else None, 0) == 0
        bf.same_bits(out.view(f32).reshape(H, W, 4), want, "out")
        if with_ao:
            bf.same_bits(ao.view(f32).reshape(H, W), want[..., 3], "ao")
        else:
            assert (ao == 0xAB).all()
        assert (block[:64] == 0xAB).all() and (block[64 + W * H * 16:128 + W * H * 16] == 0xAB).all() and (block[-64:] == 0xAB).all()
    act = bf.active_of(nrm, active)
    background = ~bf.active_of(nrm)
    pos2, bent2, active2 = pos.copy(), bent.copy(), active.copy()
    pos2[~act], bent2[~act] = np.nan, 3e38
    active2[background] ^= 0xFF
    bf.same_bits(api.wide_filter_bent(p, n, pos2, nrm, bent2, active2)[0], want, "poisoned unread texels")


def test_refusals_write_nothing():
    lib = api._lib
    nrm, pos, _, _, lights_map, _ = (np.ascontiguousarray(a) for a in wc.frame("geometric", (16, 16)))
    bent = np.ascontiguousarray(bf.synthetic_bent((16, 16), 4))
    out, ao = np.full((16, 16, 4), 7.5, f32), np.full((16, 16), 7.5, f32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ref = lambda s: C.byref(s) if s is not None else None
    good = bf.params(3)

    def call(p, n=4, pos_=pos, nrm_=nrm, bent_=bent, W=16, H=16, out_=out):
        return lib.rtsh_wide_filter_bent(ref(p), n, ptr(pos_), ptr(nrm_), ptr(lights_map), ptr(bent_), W, H, ptr(out_), ptr(ao), 0)

    assert call(good) == 0 and call(good, n=48) == 0 and call(good, n=0) == 0
    out[:], ao[:] = 7.5, 7.5
    bad = [None]
    for field, value in (("passes", 6), ("passes", 0xFFFFFFFF), ("normal_cos_min", np.nan), ("normal_cos_min", np.inf),
                         ("plane_eps", -np.inf), ("plane_eps", np.nan)):
        p = bf.params(3)
        setattr(p, field, value)
        bad.append(p)
    for p in bad:
        assert call(p) == INVALID
    for n in (49, 64, 0xFFFFFFFF):
        assert call(good, n=n) == INVALID
    assert call(good, pos_=None) == INVALID
    assert call(good, nrm_=None) == INVALID
    assert call(good, bent_=None) == INVALID
    assert call(good, out_=None) == INVALID
    assert call(good, W=0) == INVALID
    assert call(good, H=0) == INVALID
    assert call(good, W=0x7FFFFFF1, H=1) == INVALID
    assert call(good, W=1, H=0x7FFFFFF1) == INVALID
    assert (out == 7.5).all() and (ao == 7.5).all()
    p = bf.params(3)
    p.reserved_[0] = 0xFFFFFFFF                                              # (ignored)
    assert call(p) == 0
    with pytest.raises(api.RtsError):
        api.wide_filter_bent(good, 4, None, nrm, bent)
    with pytest.raises(api.RtsError):
        api.wide_filter_bent(good, 49, pos, nrm, bent)


def test_scratch_bytes():
    assert api.wide_filter_bent_scratch_bytes(3840, 2160) == 2 * 3840 * 2160 * 8
    assert api.wide_filter_bent_scratch_bytes(65536, 65536) == 2 * 65536 * 65536 * 8
    assert api.wide_filter_bent_scratch_bytes(0, 16) == 0 and api.wide_filter_bent_scratch_bytes(16, 0) == 0


def test_bent_filter_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/ao_bent_filter_host.cpp: the host twin itself (rts_scene.cpp and the shared per-pixel source, compiled into the program
    -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow, over every refusal and over the
    tiny and the 72 x 72 frames, whose buffers are heap blocks of exactly the size the header states."""
    exe = str(tmp_path / "ao_bent_filter_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "ao_bent_filter_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 1000, run.stdout[-2000:]
