"""GPU: bent-normal ambient occlusion traces (rts_trace_ambient_occlusion_bent*; include/rts.h) against the numpy rule
of tests/ao_bent_cases.py (the oracle's any-hit over the numpy rays, Q, integer sums, the frame once) -- never against the host twin
alone --, bit for bit in `bent` and byte for byte in `counts`, on guarded, preset buffers: every frame of ao_cases (1 x 1, 17 x 5 and
61 x 37 among them) in the lane-per-ray family ("kernel" 0) and the packet family ("kernel" 3) with "soft_split" 1 and 0; n of 1, 3,
4, 5, 48 with tables 0, n and 64; counts against the AO trace's own plane; counts = None; waves without a sample, a lonely last lane,
tiles without a live pixel, a background normal of -0; a row range, stripes; graph capture; refusals; and the bent combine."""
import ctypes as C

import numpy as np
import pytest

import ao_bent_cases as bc
import ao_cases as ac
import hipgraph
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = bc.GUARD
GUARD32 = 0xABABABAB
SHARE_NAME = "ambientOcclusionBentShareKernel"
FORMS = [(0, 1), (3, 1), (3, 0)]                     # ("kernel", "soft_split"): share, four waves per tile, one
NS = (1, 3, 4, 5, 48)
SHARES = {1: 0.05, 2: 0.5, 3: 0.5, 4: 0.5, 5: 10.0, 16: 0.5, 48: 0.05}
COUNTERS = ("ao_bent_traces", "ao_traces", "ao_adaptive_traces")


def _name(kernel, split, geom="rows"):
    return SHARE_NAME if kernel == 0 else "ambientOcclusionBentPacketKernel<%d,%s>" % (4 if split else 1, geom)


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


class _Dev:
    """The frame on the device; counts and bent live inside one larger guarded block (bent 16-byte aligned)."""
    PAD = 256

    def __init__(self, ctx, W, H, pos, nrm, active=None):
        self.ctx, self.W, self.H = ctx, W, H
        n = W * H
        self.n16 = (n + 15) & ~15
        self.size = self.n16 + 16 * n + 3 * self.PAD
        self.d_pos, self.d_nrm, self.d_block = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(self.size)
        self.d_act = ctx.malloc(n) if active is not None else None
        self.d_counts = self.d_block + self.PAD
        self.d_bent = self.d_block + 2 * self.PAD + self.n16
        ctx.h2d(self.d_pos, np.ascontiguousarray(pos))
        ctx.h2d(self.d_nrm, np.ascontiguousarray(nrm))
        if active is not None:
            ctx.h2d(self.d_act, np.ascontiguousarray(active))

    def guard(self):
        self.ctx.h2d(self.d_block, np.full(self.size, GUARD, np.uint8))

    def read(self, stream=None):
        """(counts[H, W], bent bits uint32[H, W, 4]); the bytes in front of, between and behind the planes must be the guard's."""
        self.ctx.synchronize(stream)
        block = np.empty(self.size, np.uint8)
        self.ctx.d2h(block, self.d_block)
        n, P, a = self.W * self.H, self.PAD, 2 * self.PAD + self.n16
        assert (block[:P] == GUARD).all() and (block[P + n:a] == GUARD).all() and (block[a + 16 * n:] == GUARD).all(), \
            "a byte outside the planes was written"
        return block[P:P + n].reshape(self.H, self.W), block[a:a + 16 * n].view(np.uint32).reshape(self.H, self.W, 4)

    def close(self):
        for d in (self.d_pos, self.d_nrm, self.d_block, self.d_act):
            if d is not None:
                self.ctx.free(d)


def _same(got, want, what, rows=None, counts=True):
    """got = _Dev.read(); want = (counts, bent) of the rule.  rows: the rows the call owns (the others keep the guard)."""
    wc, wb = want[0], bc.bits(want[1])
    if rows is not None:
        wc = np.where(rows[:, None], wc, GUARD).astype(np.uint8)
        wb = np.where(rows[:, None, None], wb, np.uint32(GUARD32))
    if not counts:
        wc = np.full_like(wc, GUARD)
    for name, g, w in (("counts", got[0], wc), ("bent", got[1], wb)):
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, name, bad.shape[0], bad[:4].tolist(), [hex(int(g[tuple(b)])) for b in bad[:4]],
                                   [hex(int(w[tuple(b)])) for b in bad[:4]])
    if counts and rows is None:
        assert np.array_equal(got[1][..., 3], bc.bits(got[0].astype(f32))), (what, "bent.w is not the count")


def _trace(ctx, dev, k, ao, want, what, rows=None, counts=True, **kw):
    dev.guard()
    ctx.trace_ambient_occlusion_bent_device(k, ao, dev.d_pos, dev.d_nrm, dev.W, dev.H, dev.d_counts if counts else None, dev.d_bent,
                                            d_active=dev.d_act, **kw)
    got = dev.read(kw.get("stream"))
    _same(got, want, what, rows, counts)
    return got


@pytest.fixture(scope="module", params=ac.FRAMES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}")
def fr(request):
    return ac.frame(*request.param)


def test_device_equals_the_rule_in_every_form(ctx, fr):
    """n of 1 and 3 leave waves of the four-wave form without a sample, 5 gives them an uneven share; with a table idx is per lane."""
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.W, fr.H, fr.pos, fr.nrm)
    d_plain = ctx.malloc(fr.W * fr.H)
    try:
        for n in NS:
            for table in ac.tables(n):
                ao, want = fr.ao(n, table, SHARES[n]), bc.want(fr, n, table, SHARES[n])
                for kernel, split in FORMS:
                    _form(ctx, kernel, split)
                    got = _trace(ctx, dev, fr.k, ao, want, (fr.name, fr.W, fr.H, n, table, kernel, split))
                    assert ctx.last_kernel_name() == _name(kernel, split), (kernel, split, ctx.last_kernel_name())
                    _trace(ctx, dev, fr.k, ao, want, (fr.name, fr.W, fr.H, n, table, kernel, split, "counts None"), counts=False)
                    # counts: byte for byte the AO trace's own plane
                    ctx.trace_ambient_occlusion_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, fr.H, d_plain)
                    ctx.synchronize()
                    plain = np.empty((fr.H, fr.W), np.uint8)
                    ctx.d2h(plain, d_plain)
                    assert np.array_equal(got[0], plain), (n, table, kernel, split)
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


@pytest.mark.parametrize("which", ["mixed", "lonely", "minus_zero"])
def test_awkward_maps(ctx, which):
    """mixed: ao_cases' map over NaN positions -- whole tiles without a live pixel (all four waves leave early, wave 0 stores the zero
    texels), single pixels, full tiles -- with n = 1, 2, 3 under four waves per tile.  lonely: the only live pixel of the frame is lane
    63 of a tile; every other lane stands in for it.  minus_zero: background normals of -0."""
    fr = ac.frame("cornell_128", 61, 37)
    nrm, pos, active = fr.nrm, fr.dirty, fr.active
    if which == "lonely":
        active, at = _lonely_map(fr)
        pos = fr.pos.copy()
        pos[active == 0] = np.nan
    if which == "minus_zero":
        nrm = fr.nrm.copy()
        nrm[fr.background] = [-0.0, 0.0, -0.0, 1.0]
        active, pos = None, fr.pos
    live = bc.live_of(nrm, active)
    tiles_dead = sum(not live[y:y + 8, x:x + 8].any() for y in range(0, fr.H, 8) for x in range(0, fr.W, 8))
    assert which == "minus_zero" or tiles_dead >= 1
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.W, fr.H, pos, nrm, active)
    try:
        for n, table in ((1, 0), (2, 0), (3, 3), (16, 64)):
            ao = fr.ao(n, table, SHARES[n])
            want = bc.bent_rule(fr.packed, fr.k, ao, pos, nrm, active)
            assert (bc.bits(want[1][~live]) == 0).all()
            if which == "lonely":
                assert int(live.sum()) == 1 and live[at]
            for kernel, split in FORMS:
                _form(ctx, kernel, split)
                _trace(ctx, dev, fr.k, ao, want, (which, n, table, kernel, split))
    finally:
        _reset(ctx)
        dev.close()


def test_rows_stripes_the_host_form_and_the_counters(ctx):
    fr = ac.frame("cornell_128", 61, 37)
    n, table = 5, 64
    ao, want = fr.ao(n, table, SHARES[n]), bc.want(fr, n, table, SHARES[n])
    H = fr.H
    # a taller frame for (5, 61): the 61 x 37 crop turned into 37 x 61 would change the scene, so rows 5..61 are those of a frame
    # stacked twice -- the start of a pixel hashes its index in the FULL frame, so the second copy's rows differ from the first's
    pos2, nrm2 = np.concatenate([fr.pos, fr.pos]), np.concatenate([fr.nrm, fr.nrm])
    want2 = bc.bent_rule(fr.packed, fr.k, ao, pos2, nrm2)
    assert (bc.bits(want2[1][:H]) != bc.bits(want2[1][H:])).any()
    ctx.set_bvh(fr.packed)
    dev, dev2 = _Dev(ctx, fr.W, H, fr.pos, fr.nrm), _Dev(ctx, fr.W, 2 * H, pos2, nrm2)
    try:
        for kernel, split in FORMS:
            _form(ctx, kernel, split)
            for r0, r1 in ((5, 61), (9, 10), (7, 7)):
                rows = (np.arange(2 * H) >= r0) & (np.arange(2 * H) < r1)
                before = [ctx.get_option(c) for c in COUNTERS]
                _trace(ctx, dev2, fr.k, ao, want2, (kernel, split, r0, r1), rows=rows, row_begin=r0, row_end=r1)
                assert [ctx.get_option(c) for c in COUNTERS] == [before[0] + (1 if r1 > r0 else 0), before[1], before[2]]
            band, geom = (16, None) if kernel == 0 else (8, "bands")
            for stripes in (2, 3):
                total = [np.full((H, fr.W), GUARD, np.uint8), np.full((H, fr.W, 4), GUARD32, np.uint32)]
                for s in range(stripes):
                    own = (np.arange(H) // band) % stripes == s
                    dev.guard()
                    ctx.trace_ambient_occlusion_bent_stripes_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, H, dev.d_counts, dev.d_bent, band,
                                                                    stripes, s)
                    got = dev.read()
                    _same(got, want, (kernel, split, band, stripes, s), rows=own)
                    assert ctx.last_kernel_name() == _name(kernel, split, geom)
                    total[0][own], total[1][own] = got[0][own], got[1][own]
                _same(total, want, (kernel, split, stripes, "all stripes"))
            # a stripe that owns no band launches nothing, writes nothing and returns RTS_OK
            before = ctx.get_option("ao_bent_traces")
            dev.guard()
            ctx.trace_ambient_occlusion_bent_stripes_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, H, dev.d_counts, dev.d_bent, 32, 3, 2)
            got = dev.read()
            assert (got[0] == GUARD).all() and (got[1] == GUARD32).all() and ctx.get_option("ao_bent_traces") == before
            # the host form stages rows 5..30 as a frame of their own: its pixel 0 is pixel 5 * W of the caller's frame
            out, bent = np.full((H, fr.W), GUARD, np.uint8), np.full((H, fr.W, 4), bc.GUARD_F32, f32)
            ctx.trace_ambient_occlusion_bent(fr.k, ao, fr.pos, fr.nrm, fr.W, H, row_begin=5, row_end=30, out=out, bent=bent)
            _same((out, bc.bits(bent)), want, (kernel, split, "host rows"), rows=(np.arange(H) >= 5) & (np.arange(H) < 30))
            none, alone = ctx.trace_ambient_occlusion_bent(fr.k, ao, fr.pos, fr.nrm, fr.W, H, want_counts=False)
            assert none is None and np.array_equal(bc.bits(alone), bc.bits(want[1]))
        with pytest.raises(api.RtsError):                                # a band that is no whole number of block rows
            ctx.trace_ambient_occlusion_bent_stripes_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, H, dev.d_counts, dev.d_bent, 12, 2, 0)
        ctx.set_option("kernel", -1)
        _trace(ctx, dev, fr.k, ao, want, "defaults")
        assert ctx.last_kernel_name() == SHARE_NAME                      # below 256 K pixels: the lane-per-ray family
    finally:
        _reset(ctx)
        dev.close()
        dev2.close()


@pytest.mark.parametrize("kernel,split", FORMS)
def test_capture_adds_one_kernel_node_and_replays_over_changed_inputs(ctx, kernel, split):
    fr = ac.frame("cornell_128", 48, 40)
    n, table = 4, 64
    ones = np.ones((fr.H, fr.W), np.uint8)
    want_all = bc.want(fr, n, table, SHARES[n])
    want_masked = bc.want(fr, n, table, SHARES[n], masked=True)
    assert (bc.bits(want_all[1]) != bc.bits(want_masked[1])).any()
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.W, fr.H, fr.pos, fr.nrm, ones)
    stream = ctx.stream_create()
    g = None
    try:
        _form(ctx, kernel, split)
        ao = fr.ao(n, table, SHARES[n])
        before = [ctx.get_option(c) for c in COUNTERS]
        g = hipgraph.capture(stream, lambda: ctx.trace_ambient_occlusion_bent_device(fr.k, ao, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts,
                                                                                      dev.d_bent, d_active=dev.d_act, stream=stream))
        assert g.node_types() == [hipgraph.KERNEL]
        assert [ctx.get_option(c) for c in COUNTERS] == [before[0] + 1, before[1], before[2]]
        assert ctx.last_kernel_name() == _name(kernel, split)
        # the host struct is overwritten and the options changed: the graph holds what was captured
        C.memset(C.byref(ao), 0xFF, C.sizeof(ao))
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
    good = fr.ao(4, 0, 0.5)

    def bad(**fields):
        a = fr.ao(4, 0, 0.5)
        for name, v in fields.items():
            setattr(a, name, v)
        return a

    def call(K=fr.k, A=good, X=dev.d_pos, N=dev.d_nrm, O=dev.d_counts, B=dev.d_bent, W=fr.W, H=fr.H, r0=0, r1=fr.H):
        return api._lib.rts_trace_ambient_occlusion_bent_device(ctx.handle, C.byref(K) if K is not None else None,
                                                                C.byref(A) if A is not None else None, C.c_void_p(X), C.c_void_p(N), None,
                                                                W, H, r0, r1, C.c_void_p(O), C.c_void_p(B), None)

    try:
        dev.guard()
        before = [ctx.get_option(c) for c in COUNTERS]
        for kw in (dict(K=None), dict(A=None), dict(X=0), dict(N=0), dict(B=0), dict(W=0), dict(H=0), dict(r0=3, r1=2), dict(r1=fr.H + 1),
                   dict(A=bad(nsamples=49)), dict(A=bad(table=3)), dict(A=bad(table=65)), dict(A=bad(nsamples=1, table=1)),
                   dict(A=bad(nsamples=1, table=8)), dict(A=bad(radius=np.inf)), dict(A=bad(radius=-np.inf)), dict(A=bad(radius=np.nan))):
            assert call(**kw) == bc.INVALID, kw
        host, hbent = np.full((fr.H, fr.W), GUARD, np.uint8), np.full((fr.H, fr.W, 4), bc.GUARD_F32, f32)
        for a in (None, bad(nsamples=49), bad(radius=np.nan), bad(table=3)):
            with pytest.raises(api.RtsError):
                ctx.trace_ambient_occlusion_bent(fr.k, a, fr.pos, fr.nrm, fr.W, fr.H, out=host, bent=hbent)
        assert api._lib.rts_trace_ambient_occlusion_bent(ctx.handle, C.byref(fr.k), C.byref(good), api._ptr(np.ascontiguousarray(fr.pos)),
                                                         api._ptr(np.ascontiguousarray(fr.nrm)), None, fr.W, fr.H, 0, fr.H, api._ptr(host),
                                                         None) == bc.INVALID
        with pytest.raises(api.RtsError):
            ctx.trace_ambient_occlusion_bent_stripes_device(fr.k, good, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts, dev.d_bent, 8, 2, 2)
        with pytest.raises(api.RtsError):
            ctx.trace_ambient_occlusion_bent_stripes_device(fr.k, good, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts, None, 8, 2, 0)
        got = dev.read()
        assert (host == GUARD).all() and (bc.bits(hbent) == GUARD32).all() and (got[0] == GUARD).all() and (got[1] == GUARD32).all()
        assert [ctx.get_option(c) for c in COUNTERS] == before
        with pytest.raises(api.RtsError):
            ctx.set_option("ao_bent_traces", 0)                          # get-only
        assert call() == 0
        _same(dev.read(), bc.want(fr, 4, 0, 0.5), "the good call")
        assert [ctx.get_option(c) for c in COUNTERS] == [before[0] + 1, before[1], before[2]]
    finally:
        dev.close()


def test_bent_combine_device_equals_the_twin_and_the_rule(ctx):
    k, lst, pos, nrm, vis, plane, bent, sky, lights_map, colors = bc.combine_case(48, 40)
    H, W = nrm.shape[:2]
    assert (W, H) == (48, 40) and lst.count == 2
    n = W * H
    d = {name: ctx.malloc(a.nbytes) for name, a in (("pos", pos), ("nrm", nrm), ("vis", vis), ("ao", plane), ("bent", bent), ("map", lights_map))}
    d_rgb = ctx.malloc(n * 3 + 512)
    stream = ctx.stream_create()
    g = None
    try:
        for name, a in (("pos", pos), ("nrm", nrm), ("vis", vis), ("ao", plane), ("bent", bent), ("map", lights_map)):
            ctx.h2d(d[name], np.ascontiguousarray(a))

        def run(b_sky, m, c, d_bent=None, **kw):
            ctx.h2d(d_rgb, np.full(n * 3 + 512, GUARD, np.uint8))
            api.combine_visibility_list_ao_bent_device(ctx, k, lst, d["pos"], d["nrm"], d["vis"], d["ao"], d_bent or d["bent"], b_sky, W, H,
                                                       d_rgb + 256, d_lights_map=d["map"] if m is not None else None, colors=c, **kw)
            ctx.synchronize(kw.get("stream"))
            out = np.empty(n * 3 + 512, np.uint8)
            ctx.d2h(out, d_rgb)
            assert (out[:256] == GUARD).all() and (out[256 + n * 3:] == GUARD).all()
            return out[256:256 + n * 3].reshape(H, W, 3)

        white = api.SkyAmbient.make(up=tuple(sky.up))
        for m, c in ((None, None), (lights_map, colors)):
            got = run(sky, m, c)
            rule = bc.combine_ao_bent_rule(k, lst, pos, nrm, vis, plane, bent, sky, m, c)
            twin = api.combine_visibility_list_ao_bent(k, lst, pos, nrm, vis, plane, bent, sky, lights_map=m, colors=c)
            assert np.array_equal(got, rule), np.argwhere(got != rule)[:4].tolist()
            assert np.array_equal(twin, rule)
            # anchor 1: a white sky gives the AO combine's bytes
            assert np.array_equal(run(white, m, c), ac.combine_ao_rule(k, lst, pos, nrm, vis, plane, m, c))
            # anchor 2: an all-zero bent plane is h = 0.5
            d_zero = ctx.malloc(bent.nbytes)
            ctx.h2d(d_zero, np.zeros_like(bent))
            half = [f32(sky.ground[i]) + (f32(sky.sky[i]) - f32(sky.ground[i])) * f32(0.5) for i in range(3)]
            flat = api.SkyAmbient.make(up=tuple(sky.up), sky=half, ground=half)
            zero = run(sky, m, c, d_bent=d_zero)
            ctx.free(d_zero)
            assert np.array_equal(zero, run(flat, m, c))
            assert np.array_equal(zero, bc.combine_ao_bent_rule(k, lst, pos, nrm, vis, plane, np.zeros_like(bent), sky, m, c))
        g = hipgraph.capture(stream, lambda: api.combine_visibility_list_ao_bent_device(ctx, k, lst, d["pos"], d["nrm"], d["vis"], d["ao"],
                                                                                         d["bent"], sky, W, H, d_rgb + 256, stream=stream))
        assert g.node_types() == [hipgraph.KERNEL]
        for b_, s_ in ((0, sky), (d["bent"], None)):
            assert api._lib.rtsh_combine_visibility_list_ao_bent_device(ctx.handle, C.byref(k), C.byref(lst), None, C.c_void_p(d["pos"]),
                                                                        C.c_void_p(d["nrm"]), None, C.c_void_p(d["vis"]), C.c_void_p(d["ao"]),
                                                                        C.c_void_p(b_), C.byref(s_) if s_ is not None else None, W, H,
                                                                        C.c_void_p(d_rgb + 256), None) == bc.INVALID
    finally:
        if g is not None:
            g.close()
        ctx.stream_destroy(stream)
        for a in d.values():
            ctx.free(a)
        ctx.free(d_rgb)
