"""GPU: ambient occlusion traces (rts_trace_ambient_occlusion*; include/rts.h) against the host twin
(rtsh_ambient_occlusion, which tests/test_ao_host.py pins to the oracle), byte for byte on guarded, preset buffers: every frame, sample
count, table and radius of tests/ao_cases.py in the lane-per-ray family and the packet family with four waves and one per tile; the
direction set below the horizon and the mixed active map over NaN positions; row ranges that start and end inside a tile; stripes; the
byte sums of trace_rays over ao_rays; graph capture; a non-default stream; the counter and the kernel names; every refusal; and the
AO combine on the device."""
import ctypes as C

import numpy as np
import pytest

import ao_cases as ac
import hipgraph
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = ac.GUARD
SHARE = "ambientOcclusionShareKernel"
FORMS = [(7, 1), (3, 1), (3, 0)]                     # ("kernel", "soft_split")


def _name(kernel, split, geom="rows"):
    return SHARE if kernel == 7 else "ambientOcclusionPacketKernel<%d,%s>" % (4 if split else 1, geom)


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.set_option("kernel", -1)
    c.set_option("soft_split", 1)
    c.close()


class _Dev:
    """The frame on the device; the counts live inside a larger guarded block."""
    PAD = 256

    def __init__(self, ctx, fr):
        self.ctx, self.W, self.H = ctx, fr.W, fr.H
        n = fr.W * fr.H
        self.d_pos, self.d_dirty, self.d_nrm, self.d_act = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n)
        self.d_block = ctx.malloc(n + 2 * self.PAD)
        self.d_counts = self.d_block + self.PAD
        ctx.h2d(self.d_pos, np.ascontiguousarray(fr.pos))
        ctx.h2d(self.d_dirty, np.ascontiguousarray(fr.dirty))
        ctx.h2d(self.d_nrm, np.ascontiguousarray(fr.nrm))
        ctx.h2d(self.d_act, np.ascontiguousarray(fr.active))

    def guard(self):
        self.ctx.h2d(self.d_block, np.full(self.W * self.H + 2 * self.PAD, GUARD, np.uint8))

    def read(self, stream=None):
        self.ctx.synchronize(stream)
        block = np.empty(self.W * self.H + 2 * self.PAD, np.uint8)
        self.ctx.d2h(block, self.d_block)
        assert (block[:self.PAD] == GUARD).all() and (block[-self.PAD:] == GUARD).all(), "a byte outside the plane was written"
        return block[self.PAD:-self.PAD].reshape(self.H, self.W)

    def close(self):
        for d in (self.d_pos, self.d_dirty, self.d_nrm, self.d_act, self.d_block):
            self.ctx.free(d)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:4].tolist(), [int(got[tuple(b)]) for b in bad[:4]], [int(want[tuple(b)]) for b in bad[:4]])


def _trace(ctx, dev, fr, ao, want, what, masked=False, rows=None, **kw):
    dev.guard()
    ctx.trace_ambient_occlusion_device(fr.k, ao, dev.d_dirty if masked else dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts,
                                       d_active=dev.d_act if masked else None, **kw)
    if rows is not None:
        want = np.where(rows[:, None], want, GUARD).astype(np.uint8)
    _same(dev.read(kw.get("stream")), want, what)


@pytest.fixture(scope="module", params=ac.FRAMES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}")
def fr(request):
    return ac.frame(*request.param)


def test_device_equals_the_twin_on_every_case(ctx, fr):
    """Every (nsamples, table, radius) of the cases, then the directions below the horizon and the mixed active map over NaN positions,
    in the three forms."""
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    cases = [(n, t, r, False, None) for n, t, r in ac.param_cases()]
    cases += [(n, t, 0.5, True, None) for n in (1, 3, 5, 48) for t in ac.tables(n)]
    cases += [(16, 64, 0.5, False, "below"), (4, 0, 0.05, True, "below"), (5, 5, 10.0, True, "below")]
    try:
        for n, table, share, masked, dirs_key in cases:
            ao = fr.ao(n, table, share, dirs=None if dirs_key is None else ac.below_horizon_dirs())
            want = fr.want(n, table, share, masked, dirs_key)
            for kernel, split in FORMS:
                ctx.set_option("kernel", kernel)
                ctx.set_option("soft_split", split)
                _trace(ctx, dev, fr, ao, want, (fr.name, n, table, share, masked, dirs_key, kernel, split), masked)
                assert ctx.last_kernel_name() == _name(kernel, split), (kernel, split, ctx.last_kernel_name())
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()


def test_rows_inside_tiles_the_host_form_and_the_counter(ctx):
    fr = ac.frame("cornell_128", 61, 37)
    n, table, share = 5, 64, 0.5
    ao, want, wantm = fr.ao(n, table, share), fr.want(n, table, share), fr.want(n, table, share, True)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    try:
        for kernel, split in FORMS:
            ctx.set_option("kernel", kernel)
            ctx.set_option("soft_split", split)
            for r0, r1 in ((3, 29), (9, 10), (17, 37), (5, 5)):
                rows = (np.arange(fr.H) >= r0) & (np.arange(fr.H) < r1)
                before = ctx.get_option("ao_traces"), ctx.get_option("soft_distance_traces"), ctx.get_option("active_traces")
                _trace(ctx, dev, fr, ao, want, (kernel, split, r0, r1), rows=rows, row_begin=r0, row_end=r1)
                _trace(ctx, dev, fr, ao, wantm, (kernel, split, r0, r1, "masked"), masked=True, rows=rows, row_begin=r0, row_end=r1)
                after = ctx.get_option("ao_traces"), ctx.get_option("soft_distance_traces"), ctx.get_option("active_traces")
                assert after == (before[0] + (2 if r1 > r0 else 0), before[1], before[2])
            # the host form stages rows 3..29 as a frame of their own: its pixel 0 is pixel 3 * W of the caller's frame
            out = np.full((fr.H, fr.W), GUARD, np.uint8)
            ctx.trace_ambient_occlusion(fr.k, ao, fr.dirty, fr.nrm, fr.W, fr.H, row_begin=3, row_end=29, active=fr.active, out=out)
            rows = (np.arange(fr.H) >= 3) & (np.arange(fr.H) < 29)
            _same(out, np.where(rows[:, None], wantm, GUARD).astype(np.uint8), (kernel, split, "host rows"))
            _same(ctx.trace_ambient_occlusion(fr.k, ao, fr.pos, fr.nrm, fr.W, fr.H), want, (kernel, split, "host whole"))
        ctx.set_option("kernel", -1)
        _trace(ctx, dev, fr, ao, want, "defaults")
        assert ctx.last_kernel_name() == SHARE                           # below 256 K pixels: the lane-per-ray family
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()


@pytest.mark.parametrize("stripes", (2, 3))
def test_stripes(ctx, stripes):
    fr = ac.frame("cornell_128", 61, 37)
    n, table, share = 4, 64, 0.5
    ao, want = fr.ao(n, table, share), fr.want(n, table, share, True)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    try:
        for kernel, split, band, geom in ((7, 1, 16, None), (3, 1, 8, "bands"), (3, 0, 8, "bands"), (3, 1, 24, "general")):
            ctx.set_option("kernel", kernel)
            ctx.set_option("soft_split", split)
            total = np.full((fr.H, fr.W), GUARD, np.uint8)
            for s in range(stripes):
                own = (np.arange(fr.H) // band) % stripes == s            # band b belongs to stripe b mod stripes
                dev.guard()
                ctx.trace_ambient_occlusion_stripes_device(fr.k, ao, dev.d_dirty, dev.d_nrm, fr.W, fr.H, dev.d_counts, band, stripes, s,
                                                           d_active=dev.d_act)
                got = dev.read()
                _same(got, np.where(own[:, None], want, GUARD).astype(np.uint8), (kernel, split, band, s))
                if own.any():
                    assert ctx.last_kernel_name() == _name(kernel, split, geom), (ctx.last_kernel_name(), kernel, split, band)
                total[own] = got[own]
            _same(total, want, (kernel, split, band, "all stripes"))
        # a stripe that owns no band launches nothing, writes nothing and returns RTS_OK
        before = ctx.get_option("ao_traces")
        dev.guard()
        ctx.trace_ambient_occlusion_stripes_device(fr.k, ao, dev.d_dirty, dev.d_nrm, fr.W, fr.H, dev.d_counts, 32, 3, 2, d_active=dev.d_act)
        assert (dev.read() == GUARD).all() and ctx.get_option("ao_traces") == before
        # a band that is no whole number of block rows is refused
        with pytest.raises(api.RtsError):
            ctx.trace_ambient_occlusion_stripes_device(fr.k, ao, dev.d_dirty, dev.d_nrm, fr.W, fr.H, dev.d_counts, 12, 2, 0)
        assert ctx.get_option("ao_traces") == before
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()


def test_counts_are_the_byte_sums_of_trace_rays_over_ao_rays(ctx):
    fr = ac.frame("terrain_96", 40, 36)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    try:
        for n, table, share in ((3, 0, 0.05), (16, 64, 0.5)):
            ao = fr.ao(n, table, share)
            rays = api.ao_rays(fr.k, ao, fr.dirty, fr.nrm, fr.W, fr.H, active=fr.active)
            d_rays, d_out = ctx.malloc(rays.nbytes), ctx.malloc(rays.shape[0])
            try:
                ctx.h2d(d_rays, rays)
                ctx.trace_rays_device(d_rays, rays.shape[0], d_out)
                ctx.synchronize()
                out = np.empty(rays.shape[0], np.uint8)
                ctx.d2h(out, d_out)
            finally:
                ctx.free(d_rays)
                ctx.free(d_out)
            live = ~fr.background & (fr.active != 0)
            sums = np.where(live, out.reshape(fr.H, fr.W, n).sum(-1), 0).astype(np.uint8)
            for kernel, split in FORMS:
                ctx.set_option("kernel", kernel)
                ctx.set_option("soft_split", split)
                _trace(ctx, dev, fr, ao, sums, (n, table, kernel, split, "ray sums"), masked=True)
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()


def test_counts_are_the_shadow_mask_sums_for_the_point_light_at_L(ctx):
    """On a subsample of pixels: the device count is the sum over j of the byte rts_trace_shadow_mask writes at p for the hard point
    light { POINT, 1 sample, L_j(p) } -- the 1 x 1 frame that holds p's texel alone, L from the numpy rule."""
    fr = ac.frame("terrain_96", 40, 36)
    n, table, share = 4, 4, 0.5
    ao = fr.ao(n, table, share)
    ctx.set_bvh(fr.packed)
    counts = ctx.trace_ambient_occlusion(fr.k, ao, fr.pos, fr.nrm, fr.W, fr.H)
    _same(counts, fr.want(n, table, share), "host form")
    ys, xs = np.nonzero(~fr.background)
    py, px = np.nonzero(~fr.background & (counts > 0) & (counts < n))          # half of the subsample: partly occluded pixels
    assert py.size >= 6
    picks = [(int(ys[i]), int(xs[i])) for i in range(0, ys.size, max(1, ys.size // 6))][:6]
    picks += [(int(py[i]), int(px[i])) for i in range(0, py.size, max(1, py.size // 6))][:6]
    mixed = 0
    for y, x in picks:
        total = 0
        for j in range(n):
            light = api.Light.make(api.Light.POINT, ac.aim_rule(fr.k, ao, fr.pos, fr.nrm, y, x, j))
            total += int(ctx.trace_shadow_mask(fr.k, fr.pos[y:y + 1, x:x + 1], 1, 1, light=light)[0, 0])
        assert total == int(counts[y, x]), (y, x, total, int(counts[y, x]))
        mixed += 0 < total < n
    assert mixed > 0


@pytest.mark.parametrize("kernel,split", FORMS)
def test_capture_adds_one_kernel_node_and_replays_the_captured_parameters(ctx, kernel, split):
    fr = ac.frame("cornell_128", 48, 40)
    n, table, share = 5, 64, 0.5
    want = fr.want(n, table, share, True)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    stream = ctx.stream_create()
    g = None
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        # a non-default stream, eagerly
        _trace(ctx, dev, fr, fr.ao(n, table, share), want, (kernel, split, "stream"), masked=True, stream=stream)
        ao = fr.ao(n, table, share)
        before = ctx.get_option("ao_traces")
        g = hipgraph.capture(stream, lambda: ctx.trace_ambient_occlusion_device(fr.k, ao, dev.d_dirty, dev.d_nrm, fr.W, fr.H, dev.d_counts,
                                                                                 stream=stream, d_active=dev.d_act))
        assert g.node_types() == [hipgraph.KERNEL]
        assert ctx.get_option("ao_traces") == before + 1
        # the host struct is overwritten and the options changed: the graph holds what was captured
        C.memset(C.byref(ao), 0xFF, C.sizeof(ao))
        ctx.set_option("kernel", 7 if kernel != 7 else 3)
        dev.guard()
        g.launch(stream)
        _same(dev.read(stream), want, (kernel, split, "replay"))
        # ... and reads the buffers as they are at the replay: with every pixel marked inactive it writes zeros
        ctx.h2d(dev.d_act, np.zeros(fr.W * fr.H, np.uint8))
        dev.guard()
        g.launch(stream)
        assert (dev.read(stream) == 0).all()
    finally:
        if g is not None:
            g.close()
        ctx.stream_destroy(stream)
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()


def test_refusals_leave_the_buffers_and_the_counter_alone(ctx):
    fr = ac.frame("cornell_128", 17, 5)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr)
    good = fr.ao(4, 0, 0.5)

    def bad(**fields):
        a = fr.ao(4, 0, 0.5)
        for name, v in fields.items():
            setattr(a, name, v)
        return a

    def call(K=fr.k, A=good, X=dev.d_pos, N=dev.d_nrm, O=dev.d_counts, W=fr.W, H=fr.H, r0=0, r1=fr.H):
        return api._lib.rts_trace_ambient_occlusion_device(ctx.handle, C.byref(K) if K is not None else None,
                                                           C.byref(A) if A is not None else None, C.c_void_p(X), C.c_void_p(N), None, W, H, r0,
                                                           r1, C.c_void_p(O), None)

    try:
        dev.guard()
        before = ctx.get_option("ao_traces")
        for kw in (dict(K=None), dict(A=None), dict(X=0), dict(N=0), dict(O=0), dict(W=0), dict(H=0), dict(r0=3, r1=2), dict(r1=fr.H + 1),
                   dict(A=bad(nsamples=49)), dict(A=bad(table=3)), dict(A=bad(table=65)), dict(A=bad(nsamples=1, table=1)),
                   dict(A=bad(radius=np.inf)), dict(A=bad(radius=np.nan))):
            assert call(**kw) == ac.INVALID, kw
        host = np.full((fr.H, fr.W), GUARD, np.uint8)
        for a in (None, bad(nsamples=49), bad(radius=np.nan)):
            with pytest.raises(api.RtsError):
                ctx.trace_ambient_occlusion(fr.k, a, fr.pos, fr.nrm, fr.W, fr.H, out=host)
        with pytest.raises(api.RtsError):
            ctx.trace_ambient_occlusion_stripes_device(fr.k, good, dev.d_pos, dev.d_nrm, fr.W, fr.H, dev.d_counts, 8, 2, 2)
        assert (host == GUARD).all() and (dev.read() == GUARD).all()
        assert ctx.get_option("ao_traces") == before
        with pytest.raises(api.RtsError):
            ctx.set_option("ao_traces", 0)                               # get-only
        assert call() == 0
        _same(dev.read(), fr.want(4, 0, 0.5), "the good call")
        assert ctx.get_option("ao_traces") == before + 1
    finally:
        dev.close()


def test_device_ao_combine_equals_the_host_one_with_one_node(ctx):
    k, lst, pos, nrm, vis, plane, lights_map, colors = ac.combine_case()
    H, W = nrm.shape[:2]
    want = api.combine_visibility_list_ao(k, lst, pos, nrm, vis, plane, lights_map=lights_map, colors=colors)
    bufs = [np.ascontiguousarray(a) for a in (pos, nrm, vis, plane, lights_map)]
    d = [ctx.malloc(a.nbytes) for a in bufs]
    d_rgb = ctx.malloc(W * H * 3 + 64)
    stream = ctx.stream_create()
    g = None
    try:
        for dp, a in zip(d, bufs):
            ctx.h2d(dp, a)

        def run(s=None):
            api.combine_visibility_list_ao_device(ctx, k, lst, d[0], d[1], d[2], d[3], W, H, d_rgb, d_lights_map=d[4], colors=colors, stream=s)

        def read(s=None):
            ctx.synchronize(s)
            out = np.empty(W * H * 3 + 64, np.uint8)
            ctx.d2h(out, d_rgb)
            assert (out[W * H * 3:] == GUARD).all()
            return out[:W * H * 3].reshape(H, W, 3)

        ctx.h2d(d_rgb, np.full(W * H * 3 + 64, GUARD, np.uint8))
        run()
        assert np.array_equal(read(), want)
        g = hipgraph.capture(stream, lambda: run(stream))
        assert g.node_types() == [hipgraph.KERNEL]
        ctx.h2d(d_rgb, np.full(W * H * 3 + 64, GUARD, np.uint8))
        g.launch(stream)
        assert np.array_equal(read(stream), want)
        st = api._lib.rtsh_combine_visibility_list_ao_device(ctx.handle, C.byref(k), C.byref(lst), None, C.c_void_p(d[0]), C.c_void_p(d[1]), None,
                                                             C.c_void_p(d[2]), None, W, H, C.c_void_p(d_rgb), None)
        assert st == ac.INVALID
    finally:
        if g is not None:
            g.close()
        ctx.stream_destroy(stream)
        for dp in d + [d_rgb]:
            ctx.free(dp)
