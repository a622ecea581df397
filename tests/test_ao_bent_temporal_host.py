"""The temporal accumulation of the bent texel and the wide bent filter fed from it, on the host (include/rts_scene.h,
rtsh_accumulate_bent*, rtsh_wide_filter_bent_mean): the host twins against the numpy rules of
tests/ao_bent_temporal_cases.py bit for bit, the anchors of the header, the guards, and every refusal with preset outputs.  No GPU.  The
twins themselves run under the sanitizers in tests/cpp/ao_bent_temporal_host.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ao_bent_filter_cases as bf
import ao_bent_temporal_cases as bt
import list_motion_cases as ms
import list_temporal_cases as tc
from raytracedshadows_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, u32, u64, i64 = np.float32, np.uint32, np.uint64, np.int64


def still_params(max_length, reset=0):
    """A camera that does not move, looking down -z: list_temporal_cases' "subpixel" pair with no eye delta is not still, so the
    G-buffer below is its own -- a plane in front of the camera, every pixel reprojecting onto itself with one tap of weight 1024."""
    return api.TemporalParams.make((0.0, 0.0, 0.0), (1, 0, 0), (0, 1, 0), (0, 0, -1), 1.0, 1.0, 0.9, 0.02, max_length, reset)


def still_gbuffer(wh):
    """positions on the plane z = -4 through the pixel centres of a camera with scale 1 x 1, normals towards the camera."""
    W, H = wh
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    pos, nrm = np.zeros((H, W, 4), f32), np.zeros((H, W, 4), f32)
    pos[..., 0] = ((x + 0.5) / W * 2 - 1) * 4
    pos[..., 1] = (1 - (y + 0.5) / H * 2) * 4
    pos[..., 2], pos[..., 3] = -4.0, 1.0
    nrm[..., 2] = 1.0
    return pos, nrm


# ---------------------------------------------------------------------------------------------------------------- twin == rule
@pytest.mark.parametrize("n", bt.SAMPLES)
@pytest.mark.parametrize("wh", bt.FRAMES)
@pytest.mark.parametrize("motion", bt.MOTIONS)
def test_host_twin_equals_the_numpy_rule(motion, wh, n):
    """Both stages, as bits: every max_length, with and without `active`, with and without the reset bit and on the first frame; the
    filter over the accumulated texels for passes 0 .. 5.  The guards are asserted from the rule's census."""
    c = bt.case(motion, wh, n)
    for max_length in bt.MAX_LENGTHS:
        for active in (c["active"], None):
            for reset in (0, 1):
                p = tc.with_params(c["params"], max_length, reset)
                census = {}
                want = bt.accumulate_rule(p, n, c["pos"], c["nrm"], c["bent"], c["prev"], active, census)
                got = api.accumulate_bent(p, n, c["pos"], c["nrm"], c["bent"], c["prev"], active)
                bt.same_texels(got, want, (motion, wh, n, max_length, active is not None, reset))
                if max_length > 1 and not reset:
                    bt.accumulate_census_ok(motion, wh, census, (motion, wh, n, max_length))
    p = tc.with_params(c["params"], 255, 0)
    first = api.accumulate_bent(p, n, c["pos"], c["nrm"], c["bent"], None, c["active"])
    bt.same_texels(first, bt.accumulate_rule(p, n, c["pos"], c["nrm"], c["bent"], None, c["active"]), (motion, wh, n, "first frame"))
    texels, _ = api.accumulate_bent(p, n, c["pos"], c["nrm"], c["bent"], c["prev"], c["active"])
    for plane, what in ((texels, "accumulated"), (c["prev"][2], "awkward")):
        census = {}
        want = bt.mean_filter_rule(bf.params(0), n, c["pos"], c["nrm"], plane, c["active"], 5, census)
        for passes in bt.PASSES:
            out, ao = api.wide_filter_bent_mean(bf.params(passes), n, c["pos"], c["nrm"], plane, c["active"])
            bf.same_bits(out, want[passes], (motion, wh, n, what, passes))
            bf.same_bits(ao, want[passes][..., 3], (motion, wh, n, what, passes, "ao"))
            assert (out[..., :3] >= -1).all() and (out <= 1).all() and (out[..., 3] >= 0).all()
        if what == "awkward":
            bt.mean_census_ok(wh, census, (motion, wh, n))


def test_threads_change_nothing():
    c = bt.case("pixels", (72, 40), 4)
    one = api.accumulate_bent(c["params"], 4, c["pos"], c["nrm"], c["bent"], c["prev"], c["active"], threads=1)
    three = api.accumulate_bent(c["params"], 4, c["pos"], c["nrm"], c["bent"], c["prev"], c["active"], threads=3)
    bt.same_texels(three, one, "threads")
    a = api.wide_filter_bent_mean(bf.params(4), 4, c["pos"], c["nrm"], one[0], c["active"], threads=1)
    b = api.wide_filter_bent_mean(bf.params(4), 4, c["pos"], c["nrm"], one[0], c["active"], threads=3)
    bf.same_bits(a[0], b[0], "filter threads")


# ------------------------------------------------------------------------------------------------------ the anchors of stage 1
@pytest.mark.parametrize("motion", bt.MOTIONS)
def test_anchor_1_lengths_and_V_are_the_moments_pass(motion):
    """lengths_out and the V channel equal, byte for byte, lengths_out and mean_out of the moments pass over the counts under the
    stand-in list, a 0 / 1 map made from `active`, the same reset bit and a history whose V channel is that prev_mean."""
    for wh, n in (((72, 40), 4), ((40, 40), 48), ((17, 1), 1)):
        c = bt.case(motion, wh, n)
        counts, bent = bt.counted_bent(wh, n)
        lst = api.AoParams.make(n, 1.0).stand_in_list()
        prev_mean = bt.unpack(c["prev"][2])[..., 3].astype(np.uint16)[None]
        prev_square = np.zeros_like(prev_mean, dtype=np.uint32)
        map01 = (c["active"] != 0).astype(np.uint8)
        for max_length in (2, 5, 255):
            for reset in (0, 1):
                p = tc.with_params(c["params"], max_length, reset)
                texels, lengths = api.accumulate_bent(p, n, c["pos"], c["nrm"], bent, c["prev"], c["active"])
                mean, _, mlen = api.accumulate_moments_soft_light_list(
                    lst, p, c["pos"], c["nrm"], counts[None], (c["prev"][0], c["prev"][1], prev_mean, prev_square, c["prev"][3][None]), map01)
                assert (lengths == mlen[0]).all(), (motion, wh, n, max_length, reset)
                assert (bt.unpack(texels)[..., 3] == mean[0]).all(), (motion, wh, n, max_length, reset)


@pytest.mark.parametrize("motion", bt.MOTIONS)
def test_anchor_2_negation(motion):
    """Negating every bent.xyz and every history x, y, z (none of them -32768) negates every output x, y, z; V and the lengths stay."""
    for wh, n in (((72, 40), 4), ((40, 40), 48)):
        c = bt.case(motion, wh, n)
        texels, lengths = bt.history(wh, symmetric=True)
        H = bt.unpack(texels)
        assert (H[..., :3] != -32768).all() and (H[..., :3] == 32767).any() and (H[..., :3] == -32767).any()
        neg_hist = H.copy()
        neg_hist[..., :3] = -neg_hist[..., :3]
        neg_bent = np.array(c["bent"])
        neg_bent[..., :3] = -neg_bent[..., :3]
        for max_length in (2, 255):
            p = tc.with_params(c["params"], max_length, 0)
            a, la = api.accumulate_bent(p, n, c["pos"], c["nrm"], c["bent"], (c["prev"][0], c["prev"][1], texels, lengths), c["active"])
            b, lb = api.accumulate_bent(p, n, c["pos"], c["nrm"], neg_bent, (c["prev"][0], c["prev"][1], bt.pack(neg_hist), lengths), c["active"])
            A, B = bt.unpack(a), bt.unpack(b)
            assert (A[..., :3] == -B[..., :3]).all() and (A[..., 3] == B[..., 3]).all() and (la == lb).all(), (motion, wh, n, max_length)
            assert (A[..., :3] < 0).any() and (A[..., :3] > 0).any()


def test_anchor_3_still_camera_recurrence():
    """One tap of weight 1024: h_k = sign * ((2 * |(n_f - 1) * h_(k-1) + cur| + n_f) / (2 * n_f)) per component, n_f = min(k, max_length),
    over a chain of frames fed with changing float planes."""
    wh, n = (40, 24), 4
    pos, nrm = still_gbuffer(wh)
    for max_length in (2, 5, 255):
        p = still_params(max_length)
        prev, h, length = None, None, 0
        for k in range(1, 9):
            bent = np.array(bf.synthetic_bent(wh, n))
            bent[..., :3] = np.roll(bent[..., :3], k, axis=1) * f32(1 if k % 2 else -1)
            texels, lengths = api.accumulate_bent(p, n, pos, nrm, bent, prev)
            cur = bf.quantise_rule(bent, n, np.ones(wh[::-1], bool))
            nf = min(length + 1, max_length)
            if h is None or nf == 1:
                h = cur
            else:
                num = (nf - 1) * h + cur
                h = np.sign(num) * ((2 * np.abs(num) + nf) // (2 * nf))
            length = nf
            assert (lengths == nf).all(), (max_length, k, np.unique(lengths))
            assert (bt.unpack(texels) == h).all(), (max_length, k)
            prev = (pos, nrm, texels, lengths)


def test_explicit_tie_rounds_half_away_from_zero():
    """Still camera, history x = -1 of length 1, current 0, max_length 2: num = -1024, den = 2048, the result is -1; with +1 it is +1.  A
    floor or a half-up division gives 0 for one of them."""
    wh = (5, 3)
    pos, nrm = still_gbuffer(wh)
    bent = np.zeros((3, 5, 4), f32)
    for value in (-1, 1):
        hist = np.zeros((3, 5, 4), i64)
        hist[..., 0], hist[..., 2] = value, -value
        texels, lengths = api.accumulate_bent(still_params(2), 4, pos, nrm, bent, (pos, nrm, bt.pack(hist), np.ones((3, 5), np.uint8)))
        got = bt.unpack(texels)
        assert (got[..., 0] == value).all() and (got[..., 2] == -value).all() and (got[..., 1] == 0).all() and (lengths == 2).all(), got[0, 0]


@pytest.mark.parametrize("motion", bt.MOTIONS)
def test_anchor_4_pass_through(motion):
    """max_length == 1, the reset bit and the first frame give pack(X_0, V_0) and length 1 at active pixels, zeros elsewhere."""
    for wh, n in (((72, 40), 4), ((3, 2), 48)):
        c = bt.case(motion, wh, n)
        act = bf.active_of(c["nrm"], c["active"])
        want = (bt.pack(bf.quantise_rule(c["bent"], n, act)), act.astype(np.uint8))
        for p, prev in ((tc.with_params(c["params"], 1, 0), c["prev"]), (tc.with_params(c["params"], 5, 1), c["prev"]),
                        (tc.with_params(c["params"], 5, 0xFF), c["prev"]), (tc.with_params(c["params"], 5, 0), None)):
            bt.same_texels(api.accumulate_bent(p, n, c["pos"], c["nrm"], c["bent"], prev, c["active"]), want, (motion, wh, n))
        # bits of reset_lights above bit 0 do not reset
        p = tc.with_params(c["params"], 5, 0xFE)
        bt.same_texels(api.accumulate_bent(p, n, c["pos"], c["nrm"], c["bent"], c["prev"], c["active"]),
                       api.accumulate_bent(tc.with_params(c["params"], 5, 0), n, c["pos"], c["nrm"], c["bent"], c["prev"], c["active"]), "0xFE")


@pytest.mark.parametrize("motion", bt.MOTIONS)
def test_anchor_5_range(motion):
    """Every output component lies between the smallest and the largest of its accepted history values and the current one: the twin's
    output (equal to the rule's) against the rule's own boxes."""
    for wh, n in (((72, 40), 4), ((40, 40), 1)):
        c = bt.case(motion, wh, n)
        for max_length in (2, 255):
            p = tc.with_params(c["params"], max_length, 0)
            parts = {}
            bt.accumulate_rule(p, n, c["pos"], c["nrm"], c["bent"], c["prev"], c["active"], None, parts)
            got = bt.unpack(api.accumulate_bent(p, n, c["pos"], c["nrm"], c["bent"], c["prev"], c["active"])[0])
            on = parts["act"]
            assert ((got >= parts["lo"]) & (got <= parts["hi"]))[on].all(), (motion, wh, n, max_length)
            if motion != "away":
                assert parts["blend"].any() and (parts["lo"] < parts["hi"])[parts["blend"]].any()


@pytest.mark.parametrize("motion", bt.MOTIONS)
def test_anchor_6_equal_values_give_that_value(motion):
    wh = (72, 40)
    for n, texel in ((4, (-3.3, 0.7, 1e-3, 3.0)), (48, (47.9, -48.0, -0.0, 17.0)), (1, (0.5000153, -1.0, 0.25, 1.0))):
        c = bt.case(motion, wh, n)
        bent = np.empty((wh[1], wh[0], 4), f32)
        bent[...] = np.array(texel, f32)
        X = bf.quantise_rule(bent, n, np.ones((wh[1], wh[0]), bool))
        hist = bt.pack(X)
        for max_length in (2, 5, 255):
            texels, lengths = api.accumulate_bent(tc.with_params(c["params"], max_length, 0), n, c["pos"], c["nrm"], bent,
                                                  (c["prev"][0], c["prev"][1], hist, c["prev"][3]), c["active"])
            act = bf.active_of(c["nrm"], c["active"])
            assert (texels[act] == hist[act]).all() and (texels[~act] == 0).all(), (motion, n, max_length)
            assert motion == "away" or (lengths > 1).any()


# ------------------------------------------------------------------------------------------------------ the anchors of stage 2
def test_mean_anchor_1_first_frame_texels_give_the_float_filter():
    """Over the texels of a first-frame accumulate, out and ao are bit for bit rtsh_wide_filter_bent's of the float plane, every passes."""
    for motion, wh, n in (("pixels", (72, 40), 4), ("turn", (40, 40), 48), ("subpixel", (17, 1), 1), ("away", (3, 2), 4)):
        c = bt.case(motion, wh, n)
        for active in (c["active"], None):
            texels, _ = api.accumulate_bent(c["params"], n, c["pos"], c["nrm"], c["bent"], None, active)
            for passes in bt.PASSES:
                want = api.wide_filter_bent(bf.params(passes), n, c["pos"], c["nrm"], c["bent"], active)
                got = api.wide_filter_bent_mean(bf.params(passes), n, c["pos"], c["nrm"], texels, active)
                bf.same_bits(got[0], want[0], (motion, wh, n, passes))
                bf.same_bits(got[1], want[1], (motion, wh, n, passes, "ao"))


def test_mean_anchor_2_passes_0_is_the_quotient_of_the_clamped_texel():
    for n in bt.SAMPLES:
        c = bt.case("pixels", (72, 40), n)
        N, S_b, S_l = bf.scales(n)
        X = bt.unpack(c["prev"][2])
        act = bf.active_of(c["nrm"], c["active"])
        want = np.zeros((40, 72, 4), f32)
        want[..., :3] = np.clip(X[..., :3], -N * S_b, N * S_b).astype(f32) / f32(N * S_b)
        want[..., 3] = np.minimum(X[..., 3], N * S_l).astype(f32) / f32(N * S_l)
        want = np.where(act[..., None], want, f32(0))
        out, ao = api.wide_filter_bent_mean(bf.params(0), n, c["pos"], c["nrm"], c["prev"][2], c["active"])
        bf.same_bits(out, want, n)
        bf.same_bits(ao, want[..., 3], n)


def test_mean_anchor_3_negation_closed_thresholds_and_equal_texels():
    c = bt.case("turn", (72, 40), 4)
    texels, _ = bt.history((72, 40), symmetric=True)
    H = bt.unpack(texels)
    H[..., :3] = -H[..., :3]
    for passes in bt.PASSES:
        a, _ = api.wide_filter_bent_mean(bf.params(passes), 4, c["pos"], c["nrm"], texels, c["active"])
        b, _ = api.wide_filter_bent_mean(bf.params(passes), 4, c["pos"], c["nrm"], bt.pack(H), c["active"])
        want = np.where(a == 0, a, -a)
        want[..., 3] = a[..., 3]
        bf.same_bits(b, want, ("negation", passes))
    zero, _ = api.wide_filter_bent_mean(bf.params(0), 4, c["pos"], c["nrm"], texels, c["active"])
    for closed in bf.CLOSED:
        for passes in (1, 3, 5):
            out, _ = api.wide_filter_bent_mean(closed(passes), 4, c["pos"], c["nrm"], texels, c["active"])
            bf.same_bits(out, zero, ("closed", passes))
    same = np.full((40, 72), bt.pack(np.array([[[-77, 32764, 5, 1234]]]))[0, 0], u64)
    zero, _ = api.wide_filter_bent_mean(bf.params(0), 4, c["pos"], c["nrm"], same, c["active"])
    for passes in bt.PASSES:
        out, _ = api.wide_filter_bent_mean(bf.params(passes), 4, c["pos"], c["nrm"], same, c["active"])
        bf.same_bits(out, zero, ("equal", passes))


# --------------------------------------------------------------------------------------------------------------- the motion form
@pytest.mark.parametrize("wh", ms.FRAMES)
@pytest.mark.parametrize("move", ("static", "translate", "rotate", "degenerate"))
def test_motion_form_matches_the_rule(move, wh):
    """The moved streams of list_motion_cases against reproject_inputs in front of the blend; with static motion planes the motion form
    gives the parent's bits."""
    for name, camera in (("cornell", "moved"), ("terrain", "still")):
        f = bt.pair(name, move, wh, camera)
        texels, lengths = bt.history(wh)
        active, bent = bt.active_plane(wh, 1), bf.synthetic_bent(wh, 4)
        prev, mo = (f["prev_pos"], f["prev_nrm"], texels, lengths), (f["pts"], f["pnr"])
        for max_length in (2, 255):
            p = tc.with_params(f["params"], max_length, 0)
            census = {}
            want = bt.accumulate_motion_rule(p, 4, f["nrm"], bent, prev, active, mo, census)
            got = api.accumulate_bent(p, 4, f["pos"], f["nrm"], bent, prev, active, motion=mo)
            bt.same_texels(got, want, (name, move, wh, max_length))
            assert census["negative"] > 0 and (camera == "still" or census["shared"] > 0), (name, move, wh, census)   # (still: one tap)
            if move == "static":
                bt.same_texels(got, api.accumulate_bent(p, 4, f["pos"], f["nrm"], bent, prev, active), (name, wh, "static == parent"))
        first = api.accumulate_bent(f["params"], 4, f["pos"], f["nrm"], bent, None, active, motion=(None, None))
        bt.same_texels(first, bt.accumulate_rule(f["params"], 4, f["pos"], f["nrm"], bent, None, active), (name, move, wh, "first frame"))


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing():
    lib, INVALID = api._lib, 1
    wh, n = (16, 8), 4
    c = bt.case("pixels", (72, 40), n)
    W, H = wh
    pos, nrm = (np.ascontiguousarray(a[:H, :W]) for a in (c["pos"], c["nrm"]))
    bent = np.ascontiguousarray(bf.synthetic_bent(wh, n))
    ppos, pnrm = pos.copy(), nrm.copy()
    ptex, plen = (np.ascontiguousarray(a) for a in bt.history(wh))
    active = np.ascontiguousarray(bt.active_plane(wh))
    texels, lengths = np.full((H, W), 0xABABABABABABABAB, u64), np.full((H, W), 0xAB, np.uint8)
    good = api.TemporalParams.from_buffer_copy(c["params"])
    P = api._ptr

    def call(p=good, ns=n, po=pos, no=nrm, be=bent, pp=ppos, pn=pnrm, pt=ptex, pl=plen, w=W, h=H, to=texels, lo=lengths, motion=None):
        q = lambda a: None if a is None else P(a)
        head = (None if p is None else C.byref(p), ns, q(po), q(no), P(active), q(be), q(pp), q(pn), q(pt), q(pl))
        if motion is not None:
            return lib.rtsh_accumulate_bent_motion(*head, q(motion[0]), q(motion[1]), w, h, q(to), q(lo), 1)
        return lib.rtsh_accumulate_bent(*head, w, h, q(to), q(lo), 1)

    def refused(what, **kw):
        assert call(**kw) == INVALID, what
        assert (texels == 0xABABABABABABABAB).all() and (lengths == 0xAB).all(), what

    refused("NULL params", p=None)
    for ns in (49, 64, 0xFFFFFFFF):
        refused("nsamples", ns=ns)
    for name in ("po", "no", "be", "to", "lo"):
        refused("NULL " + name, **{name: None})
    for name in ("pp", "pn", "pt", "pl"):
        refused("some but not all prev: " + name, **{name: None})
    refused("texels_out == prev_texels", pt=texels)
    refused("lengths_out == prev_lengths", pl=lengths)
    for w, h in ((0, H), (W, 0), (65537, 1), (1, 65537)):
        refused("frame", w=w, h=h)
    for max_length in (0, 256):
        refused("max_length", p=tc.with_params(good, max_length, 0))
    for field in ("eye_delta", "prev_right", "prev_up", "prev_fwd"):
        for v in (np.nan, np.inf):
            q = api.TemporalParams.from_buffer_copy(good)
            getattr(q, field)[1] = v
            refused(field, p=q)
    for field, values in (("normal_cos_min", (np.nan, np.inf)), ("plane_eps", (np.nan, -np.inf)), ("prev_scale_x", (np.nan, 0.0, -1.0, np.inf)),
                          ("prev_scale_y", (np.nan, 0.0, -1.0, np.inf))):
        for v in values:
            q = api.TemporalParams.from_buffer_copy(good)
            setattr(q, field, v)
            refused(field, p=q)
    pts = pos.copy()
    refused("motion: NULL prev_points", motion=(None, pts))
    refused("motion: NULL prev_point_normals", motion=(pts, None))
    assert call(motion=(pts, nrm.copy())) == 0 and call(ns=48) == 0 and call(ns=0) == 0
    assert call(pp=None, pn=None, pt=None, pl=None, motion=(None, None)) == 0          # the first frame reads neither motion plane

    # the filter over the texels: the parent's refusals, texels in the place of bent
    out, ao = np.full((H, W, 4), 7.5, f32), np.full((H, W), 7.5, f32)

    def fcall(p, ns=n, po=pos, no=nrm, tx=ptex, w=W, h=H, o=out):
        q = lambda a: None if a is None else P(a)
        return lib.rtsh_wide_filter_bent_mean(None if p is None else C.byref(p), ns, q(po), q(no), P(active), q(tx), w, h, q(o), P(ao), 1)

    def frefused(what, *a, **kw):
        assert fcall(*a, **kw) == INVALID, what
        assert (out == 7.5).all() and (ao == 7.5).all(), what

    ok = bf.params(3)
    frefused("NULL params", None)
    frefused("passes", api.WideFilterParams.make(6, 0.9, 0.02))
    frefused("cos", api.WideFilterParams.make(3, np.nan, 0.02))
    frefused("eps", api.WideFilterParams.make(3, 0.9, np.inf))
    frefused("nsamples", ok, ns=49)
    for name in ("po", "no", "tx", "o"):
        frefused("NULL " + name, ok, **{name: None})
    for w, h in ((0, H), (W, 0)):
        frefused("frame", ok, w=w, h=h)
    assert fcall(ok) == 0 and fcall(ok, ns=48) == 0


def test_python_wrappers_refuse_buffers_that_do_not_fit():
    c = bt.case("pixels", (72, 40), 4)
    with pytest.raises(api.RtsError):
        api.accumulate_bent(c["params"], 4, c["pos"], c["nrm"], c["bent"][:10], c["prev"], c["active"])
    with pytest.raises(api.RtsError):
        api.accumulate_bent(c["params"], 4, c["pos"], c["nrm"], c["bent"], c["prev"][:3] + (c["prev"][3][:5],), c["active"])
    with pytest.raises(api.RtsError):
        api.wide_filter_bent_mean(bf.params(1), 4, c["pos"], c["nrm"], c["prev"][2][:7], c["active"])


def test_bent_temporal_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/ao_bent_temporal_host.cpp: the host twins themselves (rts_scene.cpp and the shared per-pixel source, compiled into the
    program -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow, over every refusal and
    over small frames whose buffers are heap blocks of exactly the size the header states."""
    exe = str(tmp_path / "ao_bent_temporal_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "ao_bent_temporal_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 1000, run.stdout[-2000:]
