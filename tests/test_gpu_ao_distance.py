"""GPU: AO distance and falloff traces (rts_trace_ambient_occlusion_distance*; include/rts.h) against the numpy rule of
tests/ao_distance_cases.py (rays_distance over the numpy rays, checked against the oracle's any-hit byte; minimum, bins, weights, A
and the quotient in numpy integers) -- never against the host twin alone --, byte for byte in `counts` and `obscurance` and as uint32
views in `distance`, on guarded, preset buffers: 67 x 45 and 40 x 24 crops in the lane-per-ray family ("kernel" 0) and the packet
family ("kernel" 3) with "soft_split" 1 and 0; n = 1, 2, 3 under four waves; a lonely last lane, tiles without a live pixel, a tile
whose every sample is blocked; tables 0 and 64; rows (5, 61) of a stacked frame; stripes; each output None in turn; the zeros and
all-255 falloffs; counts against the AO trace's plane; the host form; graph capture; counters and names; refusals; and the obscurance
plane through the wide mean filter."""
import ctypes as C

import numpy as np
import pytest

import ao_cases as ac
import ao_distance_cases as dc
import hipgraph
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
GUARD = dc.GUARD
GUARD16, GUARD32 = 0xABAB, 0xABABABAB
SHARE_NAME = "ambientOcclusionDistanceShareKernel"
FORMS = [(0, 1), (3, 1), (3, 0)]                     # ("kernel", "soft_split"): share, four waves per tile, one
COUNTERS = ("ao_distance_traces", "ao_traces", "ao_adaptive_traces", "ao_bent_traces", "soft_distance_traces", "distance_traces")


def _name(kernel, split, geom="rows"):
    return SHARE_NAME if kernel == 0 else "ambientOcclusionDistancePacketKernel<%d,%s>" % (4 if split else 1, geom)


def _form(ctx, kernel, split):
    ctx.set_option("kernel", kernel)
    ctx.set_option("soft_split", split)


def _reset(ctx):
    ctx.set_option("kernel", -1)
    ctx.set_option("soft_split", 1)


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    _reset(c)
    c.close()


class Crop:
    """A W x H crop of cornell_128 built like ao_cases' frames (its normals, background, map and NaN positions), at a size of its own:
    67 x 45 has partial tiles on both edges in both families, 40 x 24 is whole 8 x 8 tiles but one and a half 16 x 16 blocks."""
    _made = {}

    def __new__(cls, W, H):
        if (W, H) not in cls._made:
            cls._made[(W, H)] = ac.AoFrame("cornell_128", W, H, 32)
        return cls._made[(W, H)]


CROPS = [(67, 45), (40, 24)]


class _Dev:
    """The frame on the device; the three planes live inside one larger guarded block (distance 4-byte, obscurance 2-byte aligned)."""
    PAD = 256

    def __init__(self, ctx, W, H, pos, nrm, active=None):
        self.ctx, self.W, self.H = ctx, W, H
        n = W * H
        self.n16 = (n + 15) & ~15
        self.o_counts, self.o_dist = self.PAD, 2 * self.PAD + self.n16
        self.o_obs = self.o_dist + 4 * self.n16 + self.PAD
        self.size = self.o_obs + 2 * self.n16 + self.PAD
        self.d_pos, self.d_nrm, self.d_block = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(self.size)
        self.d_act = ctx.malloc(n) if active is not None else None
        self.d_counts, self.d_dist, self.d_obs = self.d_block + self.o_counts, self.d_block + self.o_dist, self.d_block + self.o_obs
        ctx.h2d(self.d_pos, np.ascontiguousarray(pos))
        ctx.h2d(self.d_nrm, np.ascontiguousarray(nrm))
        if active is not None:
            ctx.h2d(self.d_act, np.ascontiguousarray(active))

    def guard(self):
        self.ctx.h2d(self.d_block, np.full(self.size, GUARD, np.uint8))

    def read(self, stream=None):
        """(counts[H, W], distance bits uint32[H, W], obscurance uint16[H, W]); every byte around the three planes must be the guard's."""
        self.ctx.synchronize(stream)
        block = np.empty(self.size, np.uint8)
        self.ctx.d2h(block, self.d_block)
        n = self.W * self.H
        keep = np.ones(self.size, bool)
        for o, size in ((self.o_counts, n), (self.o_dist, 4 * n), (self.o_obs, 2 * n)):
            keep[o:o + size] = False
        assert (block[keep] == GUARD).all(), "a byte outside the planes was written"
        return (block[self.o_counts:self.o_counts + n].reshape(self.H, self.W),
                block[self.o_dist:self.o_dist + 4 * n].view(u32).reshape(self.H, self.W),
                block[self.o_obs:self.o_obs + 2 * n].view(np.uint16).reshape(self.H, self.W))

    def close(self):
        for d in (self.d_pos, self.d_nrm, self.d_block, self.d_act):
            if d is not None:
                self.ctx.free(d)


def _same(got, want, what, rows=None, given=(True, True, True)):
    """got = _Dev.read(); want = (counts, distance, obscurance) of the rule.  rows: the rows the call owns (the others keep the guard);
    given: which planes the call was handed (the others keep the guard)."""
    fills = (GUARD, GUARD32, GUARD16)
    wants = [np.asarray(want[0]), dc.bits(want[1]), np.asarray(want[2])]
    for i, name in enumerate(("counts", "distance", "obscurance")):
        w = wants[i]
        if rows is not None:
            w = np.where(rows[:, None], w, fills[i]).astype(w.dtype)
        if not given[i]:
            w = np.full_like(w, fills[i])
        bad = np.argwhere(got[i] != w)
        assert bad.shape[0] == 0, (what, name, bad.shape[0], bad[:4].tolist(), [hex(int(got[i][tuple(b)])) for b in bad[:4]],
                                   [hex(int(w[tuple(b)])) for b in bad[:4]])


def _trace(ctx, dev, k, ao, fall, want, what, rows=None, given=(True, True, True), **kw):
    dev.guard()
    ctx.trace_ambient_occlusion_distance_device(k, ao, fall, dev.d_pos, dev.d_nrm, dev.W, dev.H, dev.d_counts if given[0] else None,
                                                dev.d_dist if given[1] else None, dev.d_obs if given[2] else None, d_active=dev.d_act, **kw)
    got = dev.read(kw.get("stream"))
    _same(got, want, what, rows, given)
    return got


def _rule(fr, ao, fall, pos=None, nrm=None, active=None):
    return dc.distance_rule(fr.packed, fr.k, ao, fall, fr.pos if pos is None else pos, fr.nrm if nrm is None else nrm, active)[:3]


@pytest.mark.parametrize("size", CROPS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_equals_the_rule_in_every_form(ctx, size):
    """n of 1, 2 and 3 leave waves of the four-wave form without a sample, 5 gives them an uneven share; with a table idx is per lane.
    Each output None in turn; the zeros and all-255 falloffs (anchors 2 and 3); counts against the AO trace's own plane (anchor 1)."""
    fr = Crop(*size)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.W, fr.H, fr.pos, fr.nrm)
    d_plain = ctx.malloc(fr.W * fr.H)
    live = ~fr.background
    try:
        for n, table, share in ((1, 0, 0.05), (2, 0, 0.5), (3, 0, 0.5), (5, 64, 0.5), (16, 0, 0.05), (48, 64, 0.05)):
            ao = fr.ao(n, table, share)
            d = dc.sample_distances(fr.packed, fr.k, ao, fr.pos, fr.nrm)
            S = 65535 // n
            wants = {name: dc.rule_from_distances(d, n, dc.falloff(name).weights(), live)[:3] for name in dc.FALLOFFS}
            assert np.array_equal(wants["zeros"][2], wants["zeros"][0].astype(np.uint16) * S) and (wants["full"][2][live] == n * S).all()
            for kernel, split in FORMS:
                _form(ctx, kernel, split)
                what = (fr.W, fr.H, n, table, kernel, split)
                got = _trace(ctx, dev, fr.k, ao, dc.falloff("saw"), wants["saw"], what)
                assert ctx.last_kernel_name() == _name(kernel, split), (kernel, split, ctx.last_kernel_name())
                assert np.array_equal(got[1][live] < dc.INF_BITS, got[0][live] < n)
                for name in ("zeros", "full", "linear"):
                    _trace(ctx, dev, fr.k, ao, dc.falloff(name), wants[name], what + (name,))
                _trace(ctx, dev, fr.k, ao, dc.falloff("saw"), wants["saw"], what + ("counts None",), given=(False, True, True))
                _trace(ctx, dev, fr.k, ao, dc.falloff("saw"), wants["saw"], what + ("distance None",), given=(True, False, True))
                _trace(ctx, dev, fr.k, ao, None, wants["saw"], what + ("obscurance None",), given=(True, True, False))
                ctx.trace_ambient_occlusion_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, fr.H, d_plain)
                ctx.synchronize()
                plain = np.empty((fr.H, fr.W), np.uint8)
                ctx.d2h(plain, d_plain)
                assert np.array_equal(got[0], plain), what
    finally:
        _reset(ctx)
        ctx.free(d_plain)
        dev.close()


def _lonely_map(fr):
    """An all-zero map but for lane 63 of one full 8 x 8 tile whose last pixel has a surface -> (map, (y, x))."""
    a = np.zeros((fr.H, fr.W), np.uint8)
    for y in range(0, fr.H - 7, 8):
        for x in range(0, fr.W - 7, 8):
            if not fr.background[y + 7, x + 7]:
                a[y + 7, x + 7] = 1
                return a, (y + 7, x + 7)
    raise AssertionError("no full tile ends on a surface")


@pytest.mark.parametrize("which", ["mixed", "lonely"])
def test_awkward_maps(ctx, which):
    """mixed: ao_cases' map over NaN positions -- whole tiles without a live pixel (all four waves leave early, wave 0 stores the
    zeros), single pixels, full tiles -- with n = 1, 2, 3 under four waves per tile.  lonely: the only live pixel of the frame is lane
    63 of a tile; every other lane stands in for it."""
    fr = Crop(67, 45)
    nrm, pos, active = fr.nrm, fr.dirty, fr.active
    if which == "lonely":
        active, at = _lonely_map(fr)
        pos = fr.pos.copy()
        pos[active == 0] = np.nan
    live = dc.live_of(nrm, active)
    assert sum(not live[y:y + 8, x:x + 8].any() for y in range(0, fr.H, 8) for x in range(0, fr.W, 8)) >= 1
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.W, fr.H, pos, nrm, active)
    try:
        for n, table in ((1, 0), (2, 0), (3, 3), (16, 64)):
            ao, fall = fr.ao(n, table, 0.5), dc.falloff("saw")
            want = _rule(fr, ao, fall, pos, nrm, active)
            if which == "lonely":
                assert int(live.sum()) == 1 and live[at]
            for kernel, split in FORMS:
                _form(ctx, kernel, split)
                _trace(ctx, dev, fr.k, ao, fall, want, (which, n, table, kernel, split))
    finally:
        _reset(ctx)
        dev.close()


def test_a_tile_whose_every_sample_is_blocked_and_a_distance_of_zero(ctx):
    """ao_distance_cases.zero_distance_case, 9 x 8: at the pixels on the world's origin every sample's distance is exactly +0 -- bin 0 --;
    with directions turned over (z < 0 at a surface seen from below) a whole tile has no free sample: counts 0, a finite distance and
    A made of weights alone."""
    packed, k, pos, nrm, at_origin = dc.zero_distance_case()
    H, W = pos.shape[:2]
    w = np.full(64, 200, np.uint8)
    w[0] = 3
    fall = api.AoFalloff.make(w)
    ctx.set_bvh(packed)
    # the same quad seen from below: the normals point down, so every segment starts under the plane and runs up into it
    under = nrm.copy()
    under[..., 1] = -under[..., 1]
    below = pos.copy()
    below[..., 1] = -0.01
    below[:, 8] = pos[:, 8]                                              # (the ninth column: a partial tile that stays above)
    under[:, 8] = nrm[:, 8]
    devs = [_Dev(ctx, W, H, pos, nrm), _Dev(ctx, W, H, below, under)]
    try:
        for n in (1, 3, 16):
            ao = api.AoParams.make(n, 2.0, seed=n)
            flipped = api.AoParams.make(n, 2.0, dirs=ao.dirs_array()[:, :3] * f32(-1.0))
            want0 = dc.distance_rule(packed, k, ao, fall, pos, nrm)
            assert (want0[3][at_origin] == 0).all()
            want1 = dc.distance_rule(packed, k, flipped, fall, below, under)
            tile = np.zeros((H, W), bool)
            tile[:, :8] = dc.live_of(under)[:, :8]
            assert (want1[0][tile] == 0).all() and (dc.bits(want1[1])[tile] < dc.INF_BITS).all() and tile.sum() >= 60
            for kernel, split in FORMS:
                _form(ctx, kernel, split)
                got = _trace(ctx, devs[0], k, ao, fall, want0[:3], ("d == +0", n, kernel, split))
                assert (got[2][at_origin] == (2 * 3 * n * (65535 // n) + 255) // 510).all() and (got[1][at_origin] == 0).all()
                _trace(ctx, devs[1], k, flipped, fall, want1[:3], ("all blocked", n, kernel, split))
    finally:
        _reset(ctx)
        for d in devs:
            d.close()


def test_rows_stripes_the_host_form_and_the_counters(ctx):
    fr = Crop(67, 45)
    n, table = 5, 64
    ao, fall = fr.ao(n, table, 0.5), dc.falloff("linear")
    want = _rule(fr, ao, fall)
    H = fr.H
    # rows (5, 61) of the frame stacked twice: the start of a pixel hashes its index in the FULL frame, so the copies' rows differ
    pos2, nrm2 = np.concatenate([fr.pos, fr.pos]), np.concatenate([fr.nrm, fr.nrm])
    want2 = _rule(fr, ao, fall, pos2, nrm2)
    assert (want2[2][:H] != want2[2][H:]).any()
    ctx.set_bvh(fr.packed)
    dev, dev2 = _Dev(ctx, fr.W, H, fr.pos, fr.nrm), _Dev(ctx, fr.W, 2 * H, pos2, nrm2)
    try:
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            for r0, r1 in ((5, 61), (9, 10), (7, 7)):
                rows = (np.arange(2 * H) >= r0) & (np.arange(2 * H) < r1)
                before = [ctx.get_option(c) for c in COUNTERS]
                _trace(ctx, dev2, fr.k, ao, fall, want2, (kernel, split, r0, r1), rows=rows, row_begin=r0, row_end=r1)
                assert [ctx.get_option(c) for c in COUNTERS] == [before[0] + (1 if r1 > r0 else 0)] + before[1:]
            band, geom = (16, None) if kernel == 0 else (8, "bands")
            for stripes in (2, 3):
                total = [np.full((H, fr.W), GUARD, np.uint8), np.full((H, fr.W), GUARD32, u32), np.full((H, fr.W), GUARD16, np.uint16)]
                for s in range(stripes):
                    own = (np.arange(H) // band) % stripes == s
                    dev.guard()
                    ctx.trace_ambient_occlusion_distance_stripes_device(fr.k, ao, fall, dev.d_pos, dev.d_nrm, fr.W, H, dev.d_counts,
                                                                        dev.d_dist, dev.d_obs, band, stripes, s)
                    got = dev.read()
                    _same(got, want, (kernel, split, band, stripes, s), rows=own)
                    assert ctx.last_kernel_name() == _name(kernel, split, geom)
                    for t, g in zip(total, got):
                        t[own] = g[own]
                _same(total, want, (kernel, split, stripes, "all stripes"))
            # a stripe that owns no band launches nothing, writes nothing and returns RTS_OK
            before = ctx.get_option("ao_distance_traces")
            dev.guard()
            ctx.trace_ambient_occlusion_distance_stripes_device(fr.k, ao, fall, dev.d_pos, dev.d_nrm, fr.W, H, dev.d_counts, dev.d_dist,
                                                                dev.d_obs, 32, 3, 2)
            got = dev.read()
            assert (got[0] == GUARD).all() and (got[1] == GUARD32).all() and (got[2] == GUARD16).all()
            assert ctx.get_option("ao_distance_traces") == before
            # the host form stages rows 5..30 as a frame of their own: its pixel 0 is pixel 5 * W of the caller's frame
            out, dist, obs = np.full((H, fr.W), GUARD, np.uint8), np.full((H, fr.W), GUARD32, u32).view(f32), np.full((H, fr.W), GUARD16, np.uint16)
            ctx.trace_ambient_occlusion_distance(fr.k, ao, fall, fr.pos, fr.nrm, fr.W, H, row_begin=5, row_end=30, out=out, distance=dist,
                                                 obscurance=obs)
            _same((out, dc.bits(dist), obs), want, (kernel, split, "host rows"), rows=(np.arange(H) >= 5) & (np.arange(H) < 30))
            dc.same_planes(ctx.trace_ambient_occlusion_distance(fr.k, ao, fall, fr.pos, fr.nrm, fr.W, H, want_counts=False), want, "host, counts None")
            dc.same_planes(ctx.trace_ambient_occlusion_distance(fr.k, ao, None, fr.pos, fr.nrm, fr.W, H, want_obscurance=False), want,
                           "host, obscurance None")
            dc.same_planes(ctx.trace_ambient_occlusion_distance(fr.k, ao, fall, fr.pos, fr.nrm, fr.W, H, want_distance=False), want,
                           "host, distance None")
        with pytest.raises(api.RtsError):                                # a band that is no whole number of block rows
            ctx.trace_ambient_occlusion_distance_stripes_device(fr.k, ao, fall, dev.d_pos, dev.d_nrm, fr.W, H, dev.d_counts, dev.d_dist,
                                                                dev.d_obs, 12, 2, 0)
        ctx.set_option("kernel", -1)
        _trace(ctx, dev, fr.k, ao, fall, want, "defaults")
        assert ctx.last_kernel_name() == SHARE_NAME                      # below 256 K pixels: the lane-per-ray family
    finally:
        _reset(ctx)
        dev.close()
        dev2.close()


def test_one_sample_is_the_distance_trace_of_the_hard_point_light(ctx):
    """Anchor 5 on the device: n == 1, one-pixel frames, against rts_trace_shadow_distance_device for the light at ao_cases.aim_rule's L."""
    fr = Crop(40, 24)
    ctx.set_bvh(fr.packed)
    ao = fr.ao(1, 0, 0.5)
    dev = _Dev(ctx, fr.W, fr.H, fr.pos, fr.nrm)
    d_one, d_mask, d_px = ctx.malloc(4), ctx.malloc(1), ctx.malloc(16)
    try:
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            got = _trace(ctx, dev, fr.k, ao, None, _rule(fr, ao, dc.falloff("zeros")), ("n == 1", kernel, split), given=(True, True, False))
            blocked = free = 0
            for y, x in np.argwhere(~fr.background)[::97]:
                L = ac.aim_rule(fr.k, ao, fr.pos, fr.nrm, int(y), int(x), 0)
                ctx.h2d(d_px, np.ascontiguousarray(fr.pos[y, x]))
                ctx.trace_shadow_distance_device(fr.k, d_px, 1, 1, d_one, d_mask=d_mask, light=api.Light.make(api.Light.POINT, [float(v) for v in L]))
                ctx.synchronize()
                one, m = np.empty(1, u32), np.empty(1, np.uint8)
                ctx.d2h(one, d_one)
                ctx.d2h(m, d_mask)
                assert one[0] == got[1][y, x] and m[0] == got[0][y, x], (kernel, split, y, x)
                blocked += int(m[0] == 0); free += int(m[0] == 1)
            assert blocked > 0 and free > 0
    finally:
        _reset(ctx)
        for d in (d_one, d_mask, d_px):
            ctx.free(d)
        dev.close()


@pytest.mark.parametrize("kernel,split", FORMS)
def test_capture_adds_one_kernel_node_and_replays_over_changed_inputs(ctx, kernel, split):
    fr = ac.frame("cornell_128", 48, 40)
    n, table = 4, 64
    ones = np.ones((fr.H, fr.W), np.uint8)
    want_all = dc.want(fr, n, table, 0.5, "saw")
    want_masked = dc.want(fr, n, table, 0.5, "saw", masked=True)
    assert (want_all[2] != want_masked[2]).any()
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.W, fr.H, fr.pos, fr.nrm, ones)
    stream = ctx.stream_create()
    g = None
    try:
        _form(ctx, kernel, split)
        ao, fall = fr.ao(n, table, 0.5), dc.falloff("saw")
        before = [ctx.get_option(c) for c in COUNTERS]
        g = hipgraph.capture(stream, lambda: ctx.trace_ambient_occlusion_distance_device(fr.k, ao, fall, dev.d_pos, dev.d_nrm, fr.W, fr.H,
                                                                                          dev.d_counts, dev.d_dist, dev.d_obs,
                                                                                          d_active=dev.d_act, stream=stream))
        assert g.node_types() == [hipgraph.KERNEL]
        assert [ctx.get_option(c) for c in COUNTERS] == [before[0] + 1] + before[1:]
        assert ctx.last_kernel_name() == _name(kernel, split)
        # the host structs -- the falloff's bytes among them -- are overwritten and the options changed: the graph holds what was captured
        C.memset(C.byref(ao), 0xFF, C.sizeof(ao))
        C.memset(C.byref(fall), 0x5A, C.sizeof(fall))
        ctx.set_option("kernel", 3 if kernel == 0 else 0)
        dev.guard()
        g.launch(stream)
        _same(dev.read(stream), want_all, (kernel, split, "replay"))
        # the input buffers' contents change (the map, and NaN positions wherever it is 0): the replay reads them anew
        ctx.h2d(dev.d_act, np.ascontiguousarray(fr.active))
        ctx.h2d(dev.d_pos, np.ascontiguousarray(fr.dirty))
        dev.guard()
        g.launch(stream)
        _same(dev.read(stream), want_masked, (kernel, split, "replay over changed inputs"))
    finally:
        if g is not None:
            g.close()
        ctx.stream_destroy(stream)
        _reset(ctx)
        dev.close()


def test_refusals_leave_the_buffers_and_the_counters_alone(ctx):
    fr = ac.frame("cornell_128", 17, 5)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.W, fr.H, fr.pos, fr.nrm)
    good, fall = fr.ao(4, 0, 0.5), dc.falloff("saw")

    def bad(**fields):
        a = fr.ao(4, 0, 0.5)
        for name, v in fields.items():
            setattr(a, name, v)
        return a

    def call(K=fr.k, A=good, F=fall, X=dev.d_pos, N=dev.d_nrm, O=dev.d_counts, D=dev.d_dist, S=dev.d_obs, W=fr.W, H=fr.H, r0=0, r1=fr.H):
        return api._lib.rts_trace_ambient_occlusion_distance_device(ctx.handle, C.byref(K) if K is not None else None,
                                                                    C.byref(A) if A is not None else None,
                                                                    C.byref(F) if F is not None else None, C.c_void_p(X), C.c_void_p(N), None,
                                                                    W, H, r0, r1, C.c_void_p(O), C.c_void_p(D), C.c_void_p(S), None)

    try:
        dev.guard()
        before = [ctx.get_option(c) for c in COUNTERS]
        for kw in (dict(K=None), dict(A=None), dict(X=0), dict(N=0), dict(D=0, S=0), dict(F=None), dict(S=dev.d_obs + 1), dict(D=dev.d_dist + 1),
                   dict(D=dev.d_dist + 2), dict(D=dev.d_dist + 3), dict(W=0), dict(H=0), dict(r0=3, r1=2), dict(r1=fr.H + 1),
                   dict(A=bad(nsamples=49)), dict(A=bad(table=3)), dict(A=bad(table=65)), dict(A=bad(nsamples=1, table=1)),
                   dict(A=bad(nsamples=1, table=8)), dict(A=bad(radius=np.inf)), dict(A=bad(radius=-np.inf)), dict(A=bad(radius=np.nan))):
            assert call(**kw) == dc.INVALID, kw
        host, hdist, hobs = np.full((fr.H, fr.W), GUARD, np.uint8), np.full((fr.H, fr.W), GUARD32, u32).view(f32), np.full((fr.H, fr.W), GUARD16, np.uint16)
        for a in (None, bad(nsamples=49), bad(radius=np.nan), bad(table=3)):
            with pytest.raises(api.RtsError):
                ctx.trace_ambient_occlusion_distance(fr.k, a, fall, fr.pos, fr.nrm, fr.W, fr.H, out=host, distance=hdist, obscurance=hobs)
        with pytest.raises(api.RtsError):                                # obscurance without a falloff
            ctx.trace_ambient_occlusion_distance(fr.k, good, None, fr.pos, fr.nrm, fr.W, fr.H, out=host, distance=hdist, obscurance=hobs)
        with pytest.raises(api.RtsError):                                # both outputs None
            ctx.trace_ambient_occlusion_distance(fr.k, good, fall, fr.pos, fr.nrm, fr.W, fr.H, out=host, want_distance=False, want_obscurance=False)
        with pytest.raises(api.RtsError):
            ctx.trace_ambient_occlusion_distance_stripes_device(fr.k, good, fall, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts, dev.d_dist,
                                                                dev.d_obs, 8, 2, 2)
        with pytest.raises(api.RtsError):
            ctx.trace_ambient_occlusion_distance_stripes_device(fr.k, good, fall, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts, None, None, 8, 2, 0)
        got = dev.read()
        assert (host == GUARD).all() and (dc.bits(hdist) == GUARD32).all() and (hobs == GUARD16).all()
        assert (got[0] == GUARD).all() and (got[1] == GUARD32).all() and (got[2] == GUARD16).all()
        assert [ctx.get_option(c) for c in COUNTERS] == before
        with pytest.raises(api.RtsError):
            ctx.set_option("ao_distance_traces", 0)                      # get-only
        assert call() == 0
        _same(dev.read(), dc.want(fr, 4, 0, 0.5, "saw"), "the good call")
        assert [ctx.get_option(c) for c in COUNTERS] == [before[0] + 1] + before[1:]
    finally:
        dev.close()


def test_obscurance_goes_through_the_wide_mean_filter_as_it_is(ctx):
    """The downstream anchor: the device's obscurance plane as `mean` of wide_filter_mean_soft_light_list_device at 2 passes under the
    stand-in list equals the host chain (the rule's plane through the host filter) bit for bit; with the zeros falloff it equals
    wide_filter_soft_light_list_device over the counts."""
    fr = ac.frame("cornell_128", 48, 40)
    n, W, H = 16, fr.W, fr.H
    ao = fr.ao(n, 0, 0.05)
    lst = ao.stand_in_list()
    params = api.WideFilterParams.make(2, 0.9, 0.05)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, W, H, fr.pos, fr.nrm)
    d_vis, d_vis2 = ctx.malloc(W * H * 4), ctx.malloc(W * H * 4)
    d_scratch = ctx.malloc(api.wide_filter_scratch_bytes(1, W, H))

    def filtered(run):
        ctx.h2d(d_vis, np.full(W * H, GUARD32, u32))
        run(d_vis)
        ctx.synchronize()
        out = np.empty((H, W), f32)
        ctx.d2h(out, d_vis)
        return out

    try:
        for name in ("linear", "zeros"):
            fall = dc.falloff(name)
            want = dc.want(fr, n, 0, 0.05, name)
            _trace(ctx, dev, fr.k, ao, fall, want, ("downstream", name))
            got = filtered(lambda v: api.wide_filter_mean_soft_light_list_device(ctx, lst, params, dev.d_pos, dev.d_nrm, dev.d_obs, W, H, v,
                                                                                 d_scratch=d_scratch))
            host = api.wide_filter_mean_soft_light_list(lst, params, fr.pos, fr.nrm, want[2][None])
            assert np.array_equal(dc.bits(got), dc.bits(host[0])), (name, np.argwhere(dc.bits(got) != dc.bits(host[0]))[:4].tolist())
            if name == "zeros":
                over_counts = filtered(lambda v: api.wide_filter_soft_light_list_device(ctx, lst, params, dev.d_pos, dev.d_nrm, dev.d_counts,
                                                                                        W, H, v, d_scratch=d_scratch))
                assert np.array_equal(dc.bits(got), dc.bits(over_counts))
            else:
                assert (got[~fr.background] > 0).any() and (got <= 1.0).all()
    finally:
        for d in (d_vis, d_vis2, d_scratch):
            ctx.free(d)
        dev.close()
