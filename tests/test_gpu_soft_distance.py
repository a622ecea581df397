"""GPU: the soft-shadow occluder distance (rts_trace_soft_distance*; include/rts.h) against its host twin (rtsh_soft_distance, which
tests/test_soft_distance_host.py pins to the oracle), as uint32 and bytes, on guard-filled buffers: every kernel family and split
with its name, sample counts that leave a wave without a sample or with unequal shares, per-pixel jitter through whole frames, row
ranges and the host form, active maps, stripes, dissolving packets, the exact path's streams, the one-sample case, the counters, and
the device forms under graph capture."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import streams
from distance_cases import INF_BITS, bits
from raytracedshadows_amd import api
from soft_distance_cases import RADIUS, assert_classes, radius_for, soft_frame

pytestmark = pytest.mark.gpu

GUARD_F = np.float32(-123.25)
GUARD_B = 0xAB
SHARE = "shadowSoftDistanceShareKernel"
TABLE = ("point", 4, 16, RADIUS)                        # 4 of 16 offsets per pixel, the start hashed from the pixel's frame index


def _packet(split, geom="rows"):
    return "shadowSoftDistancePacketKernel<%d,%s>" % (4 if split else 1, geom)


def _name(kernel, split, geom="rows"):
    return SHARE if kernel in (0, 1, 2, 7) else _packet(split, geom)


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.set_option("kernel", -1)
    c.set_option("soft_split", 1)
    c.close()


class _Dev:
    def __init__(self, ctx, positions, W, H):
        self.ctx, self.W, self.H = ctx, W, H
        positions = np.ascontiguousarray(positions, np.float32)
        self.d_pos, self.d_act, self.d_mask, self.d_dist = ctx.malloc(positions.nbytes), ctx.malloc(W * H), ctx.malloc(W * H), ctx.malloc(W * H * 4)
        ctx.h2d(self.d_pos, positions)

    def guard(self):
        self.ctx.h2d(self.d_mask, np.full(self.W * self.H, GUARD_B, np.uint8))
        self.ctx.h2d(self.d_dist, np.full(self.W * self.H, GUARD_F, np.float32))

    def read(self, stream=None):
        d, m = np.empty((self.H, self.W), np.float32), np.empty((self.H, self.W), np.uint8)
        self.ctx.synchronize(stream)
        self.ctx.d2h(d, self.d_dist)
        self.ctx.d2h(m, self.d_mask)
        return d, m

    def close(self):
        for d in (self.d_pos, self.d_act, self.d_mask, self.d_dist):
            self.ctx.free(d)


def _expect(want, active=None, rows=None):
    d, m = want
    if active is not None:
        d, m = np.where(active != 0, d, np.float32(0.0)).astype(np.float32), (m * (active != 0)).astype(np.uint8)
    if rows is not None:
        d, m = np.where(rows[:, None], d, GUARD_F).astype(np.float32), np.where(rows[:, None], m, GUARD_B).astype(np.uint8)
    return d, m


def _same(got, want, what):
    for g, w, part in ((bits(got[0]), bits(want[0]), "distance"), (got[1], want[1], "mask")):
        bad = np.argwhere(g != w)
        assert bad.shape[0] == 0, (what, part, bad.shape[0], bad[:4].tolist(), [g[tuple(b)] for b in bad[:4]], [w[tuple(b)] for b in bad[:4]])


def _trace(ctx, dev, fr, light, want, what, active=None, rows=None, **kw):
    if active is not None:
        ctx.h2d(dev.d_act, np.ascontiguousarray(active, np.uint8))
    dev.guard()
    ctx.trace_soft_distance_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, d_mask=dev.d_mask, light=light,
                                   d_active=dev.d_act if active is not None else None, **kw)
    _same(dev.read(), _expect(want, active, rows), what)


FORMS = [(7, 1), (3, 1), (3, 0), (8, 1), (8, 0)]        # ("kernel", "soft_split")


# n = 3: a wave of the 4-wave form owns no sample; 5: unequal shares; 2 and 64: the ends of the range
@pytest.mark.parametrize("key,balanced", [(("point", 2), True), (("point", 3), True), (("point", 5), True), (("point", 16), True),
                                          (("point", 64), True), (("point", 4), False), (("directional", 4), False)],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_every_family_and_split_equals_the_twin(ctx, key, balanced):
    fr = soft_frame(61, 37)
    key = key + (0, radius_for(key[1])) if key[0] == "point" else key
    light, want = fr.light(key), fr.want(key, balanced)
    assert light.nsamples == key[1]
    assert np.array_equal(want[1] == key[1], bits(want[0]) == INF_BITS)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        for kernel, split in FORMS:
            ctx.set_option("kernel", kernel)
            ctx.set_option("soft_split", split)
            _trace(ctx, dev, fr, light, want, (key, kernel, split))
            assert ctx.last_kernel_name() == _name(kernel, split), (kernel, split, ctx.last_kernel_name())
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()


def test_auto_takes_the_lane_walk_below_256k_pixels(ctx):
    fr = soft_frame(61, 37)
    key = ("point", 5, 0, RADIUS)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        assert ctx.get_option("kernel") == -1
        _trace(ctx, dev, fr, fr.light(key), fr.want(key), "defaults")
        assert ctx.last_kernel_name() == SHARE
    finally:
        dev.close()


@pytest.mark.parametrize("kernel,split", [(7, 1), (3, 1), (3, 0)])
def test_table_jitter_whole_rows_and_host_form(ctx, kernel, split):
    fr = soft_frame(64, 48)
    light, want = fr.light(TABLE), fr.want(TABLE)
    assert light.table == 16 and light.nsamples == 4
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    rows = (np.arange(fr.H) >= 8) & (np.arange(fr.H) < 24)
    assert_classes(want[1][8:24], 4, "rows 8..24")
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        _trace(ctx, dev, fr, light, want, (kernel, split, "whole"))
        _trace(ctx, dev, fr, light, want, (kernel, split, "device rows"), rows=rows, row_begin=8, row_end=24)
        assert ctx.last_kernel_name() == _name(kernel, split)
        # the host form stages rows 8..24 as a frame of their own: its pixel 0 is pixel 8 * W of the caller's frame ("pixelBase")
        out, om = np.full((fr.H, fr.W), GUARD_F, np.float32), np.full((fr.H, fr.W), GUARD_B, np.uint8)
        ctx.trace_soft_distance(fr.k, fr.pos, fr.W, fr.H, light=light, row_begin=8, row_end=24, out=out, mask=om)
        _same((out, om), _expect(want, None, rows), (kernel, split, "host rows"))
        d, m = ctx.trace_soft_distance(fr.k, fr.pos, fr.W, fr.H, light=light)
        _same((d, m), want, (kernel, split, "host whole"))
        d, m = ctx.trace_soft_distance(fr.k, fr.pos, fr.W, fr.H, light=light, want_mask=False)
        assert m is None and np.array_equal(bits(d), bits(want[0]))
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()


_HOST_ROWS = {}


def _host_rows_case():
    """Frame 61 x 37 under 5 of 16 jittered samples, the checker map (zero bytes and set bytes), and the twin's values under that
    map: computed once."""
    if not _HOST_ROWS:
        fr = soft_frame(61, 37)
        light = fr.light(("point", 5, 16, RADIUS))
        assert light.nsamples == 5 and light.table == 16
        active = _maps(fr)["checker"]
        assert 0 < np.count_nonzero(active[3:30]) < active[3:30].size
        want = api.soft_distance(fr.packed, fr.k, light, fr.pos, fr.W, fr.H, active=active)
        for a in (active,) + want:
            a.setflags(write=False)
        _HOST_ROWS.update(fr=fr, light=light, active=active, want=want)
    return _HOST_ROWS["fr"], _HOST_ROWS["light"], _HOST_ROWS["active"], _HOST_ROWS["want"]


@pytest.mark.parametrize("kernel,split", [(7, 1), (3, 1), (3, 0)])
def test_host_form_with_an_active_map_and_a_row_range(ctx, kernel, split):
    """The host-pointer form with a per-pixel map AND a row range, under per-pixel jitter: rows [3, 30) of the positions and of the
    map travel through the staging buffers as a frame of their own, and every pixel's samples still start where its index in the
    caller's frame says ("pixelBase").  Inside the rows the twin's bits, outside them the guard the arrays were filled with."""
    fr, light, active, want = _host_rows_case()
    rows = (np.arange(fr.H) >= 3) & (np.arange(fr.H) < 30)
    ctx.set_bvh(fr.packed)
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        out, om = np.full((fr.H, fr.W), GUARD_F, np.float32), np.full((fr.H, fr.W), GUARD_B, np.uint8)
        ctx.trace_soft_distance(fr.k, fr.pos, fr.W, fr.H, light=light, row_begin=3, row_end=30, active=active, out=out, mask=om)
        assert ctx.last_kernel_name() == _name(kernel, split), ctx.last_kernel_name()
        _same((out, om), _expect(want, None, rows), (kernel, split, "host rows with a map"))
        out = np.full((fr.H, fr.W), GUARD_F, np.float32)
        d, m = ctx.trace_soft_distance(fr.k, fr.pos, fr.W, fr.H, light=light, row_begin=3, row_end=30, active=active, out=out, want_mask=False)
        assert d is out and m is None
        assert np.array_equal(bits(out), bits(_expect(want, None, rows)[0])), (kernel, split, "distances alone")
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)


def _maps(fr):
    y, x = np.mgrid[0:fr.H, 0:fr.W]
    tile = np.ones((fr.H, fr.W), np.uint8)
    tile[8:16, 16:24] = 0                                # one 8 x 8 tile wholly inactive beside active ones
    single = np.zeros((fr.H, fr.W), np.uint8)
    single[21, 34] = 7                                   # one active pixel, in the middle of its tile; nothing else in the frame
    single[16:24, 8:16] = 1                              # ... and a full tile beside it
    return {"checker": (((x + y) & 1) * 255).astype(np.uint8), "tile": tile, "zeros": np.zeros((fr.H, fr.W), np.uint8), "single": single}


@pytest.mark.parametrize("kernel,split", [(7, 1), (3, 1), (3, 0)])
def test_active_maps(ctx, kernel, split):
    fr = soft_frame(64, 48)
    light, want = fr.light(TABLE), fr.want(TABLE)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    d_ref = ctx.malloc(fr.W * fr.H)
    rows = (np.arange(fr.H) >= 5) & (np.arange(fr.H) < 42)
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        for name, active in _maps(fr).items():
            dirty = fr.pos.copy()                        # inactive texels may hold anything
            dirty[active == 0] = np.array([np.nan, np.inf, 1e38, -np.inf], np.float32)
            ctx.h2d(dev.d_pos, dirty)
            _trace(ctx, dev, fr, light, want, (kernel, split, name), active=active)
            _trace(ctx, dev, fr, light, want, (kernel, split, name, "rows"), active=active, rows=rows, row_begin=5, row_end=42)
            # the mask is the active soft mask trace's, byte for byte
            ctx.h2d(d_ref, np.full(fr.W * fr.H, GUARD_B, np.uint8))
            ctx.trace_shadow_mask_device(fr.k, dev.d_pos, fr.W, fr.H, d_ref, light=light, d_active=dev.d_act, row_begin=5, row_end=42)
            ctx.synchronize()
            ref = np.empty((fr.H, fr.W), np.uint8)
            ctx.d2h(ref, d_ref)
            assert np.array_equal(dev.read()[1], ref), (kernel, split, name)
        # d_mask is optional: the distances alone
        ctx.h2d(dev.d_pos, fr.pos)
        dev.guard()
        ctx.trace_soft_distance_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, light=light)
        d, m = dev.read()
        assert np.array_equal(bits(d), bits(want[0])) and (m == GUARD_B).all()
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        ctx.free(d_ref)
        dev.close()


@pytest.mark.parametrize("kernel,split,band", [(3, 1, 8), (3, 1, 16), (3, 1, 32), (3, 0, 8), (3, 0, 16), (7, 1, 16), (7, 1, 32)])
def test_stripes(ctx, kernel, split, band):
    fr = soft_frame(61, 37)
    key = ("point", 4, 16, RADIUS)
    light, want = fr.light(key), fr.want(key)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    active = _maps(fr)["checker"]
    ctx.h2d(dev.d_act, active)
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        for with_map in (False, True):
            for stripe in range(3):                      # (37 rows in bands of 16 or more: a stripe that owns no band)
                rows = ((np.arange(fr.H) // band) % 3) == stripe
                n0 = ctx.get_option("soft_distance_traces")
                dev.guard()
                ctx.trace_soft_distance_stripes_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, band, 3, stripe, d_mask=dev.d_mask,
                                                       light=light, d_active=dev.d_act if with_map else None)
                _same(dev.read(), _expect(want, active if with_map else None, rows), (kernel, split, band, with_map, stripe))
                # a stripe without a band launches nothing, and the counter does not move
                assert ctx.get_option("soft_distance_traces") == n0 + (1 if rows.any() else 0), (band, stripe)
                if rows.any():
                    assert ctx.last_kernel_name() == _name(kernel, split, "bands"), ctx.last_kernel_name()
        # a band that is no whole number of workgroup rows is refused, and nothing is written
        bad = 12 if kernel == 3 else 8
        dev.guard()
        n0 = ctx.get_option("soft_distance_traces")
        with pytest.raises(api.RtsError):
            ctx.trace_soft_distance_stripes_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, bad, 2, 0, d_mask=dev.d_mask, light=light)
        _same(dev.read(), _expect(want, None, np.zeros(fr.H, bool)), (kernel, bad, "refused"))
        assert ctx.get_option("soft_distance_traces") == n0
        if kernel == 3:                                  # 24 rows: not a power of two -- the general form
            rows = ((np.arange(fr.H) // 24) % 2) == 1
            dev.guard()
            ctx.trace_soft_distance_stripes_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, 24, 2, 1, d_mask=dev.d_mask, light=light)
            _same(dev.read(), _expect(want, None, rows), (kernel, split, 24))
            assert ctx.last_kernel_name() == _name(kernel, split, "general")
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()


@pytest.mark.parametrize("split", [1, 0])
def test_dissolving_packets_keep_each_samples_minimum(ctx, split):
    fr = soft_frame(64, 48)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    before = (ctx.get_option("packet_budget"), ctx.get_option("packet_share"))
    try:
        ctx.set_option("packet_budget", 1)               # the input of test_dissolving_packets_keep_their_minimum (test_gpu_distance.py)
        ctx.set_option("packet_share", 16)
        ctx.set_option("kernel", 3)
        ctx.set_option("soft_split", split)
        for key in (TABLE, ("point", 5, 0, RADIUS), ("directional", 4)):
            want = fr.want(key, key[0] == "point")
            _trace(ctx, dev, fr, fr.light(key), want, ("dissolve", split, key))
            _trace(ctx, dev, fr, fr.light(key), want, ("dissolve", split, key, "map"), active=_maps(fr)["checker"])
    finally:
        ctx.set_option("packet_budget", before[0])
        ctx.set_option("packet_share", before[1])
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()


def test_streams_of_the_exact_path(ctx):
    fr = soft_frame(64, 48)
    light = fr.light(TABLE)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    try:
        for what, packed in (("infinite root", streams.infinite_root(fr.packed)), ("swapped boxes", streams.swapped_boxes(fr.packed))):
            want = api.soft_distance(packed, fr.k, light, fr.pos, fr.W, fr.H)
            assert 0 < int((bits(want[0]) != INF_BITS).sum()) < want[0].size, what
            ctx.set_bvh(packed)
            assert ctx.get_option("bvh_finite" if what == "infinite root" else "bvh_ordered") == 0
            for kernel, split in FORMS:
                ctx.set_option("kernel", kernel)
                ctx.set_option("soft_split", split)
                _trace(ctx, dev, fr, light, want, (what, kernel, split))
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()


def test_one_sample_is_the_distance_trace(ctx):
    fr = soft_frame(64, 48)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    one = api.Light.make(api.Light.POINT, list(fr.wl.light.xyz))
    zero = api.Light.make(api.Light.POINT, list(fr.wl.light.xyz))
    zero.nsamples = 0
    try:
        for kernel, name in ((3, "shadowDistancePacketKernel<rows>"), (7, "shadowDistanceShareKernel")):
            ctx.set_option("kernel", kernel)
            for lt in (one, zero, None):
                dev.guard()
                ctx.trace_shadow_distance_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, d_mask=dev.d_mask, light=lt)
                ref = dev.read()
                assert ctx.last_kernel_name() == name
                n0, s0 = ctx.get_option("distance_traces"), ctx.get_option("soft_distance_traces")
                dev.guard()
                ctx.trace_soft_distance_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, d_mask=dev.d_mask, light=lt)
                got = dev.read()
                assert ctx.last_kernel_name() == name, ctx.last_kernel_name()
                assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
                _same(got, api.shadow_distance(fr.packed, fr.k, lt, fr.pos, fr.W, fr.H), (kernel, "twin"))
                # it IS the one-sample call: counted as a distance trace
                assert (ctx.get_option("distance_traces"), ctx.get_option("soft_distance_traces")) == (n0 + 1, s0)
    finally:
        ctx.set_option("kernel", -1)
        dev.close()


def test_counter_and_untouched_options(ctx):
    fr = soft_frame(64, 48)
    light, want = fr.light(TABLE), fr.want(TABLE)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    keys = ["kernel", "xcd_swizzle", "packet_budget", "packet_share", "block_waves", "row_order", "wide_lane", "soft_split", "tile_splits",
            "follow", "tile_order", "tile_order_tiles", "active_traces", "follow_traces", "distance_traces"]
    try:
        ctx.set_option("kernel", 3)
        order = np.arange(((fr.W + 7) // 8) * ((fr.H + 7) // 8), dtype=np.uint32)[::-1].copy()
        ctx.set_tile_order(order)
        before = {k: ctx.get_option(k) for k in keys}
        assert before["tile_order_tiles"] == order.size
        n0 = ctx.get_option("soft_distance_traces")
        _trace(ctx, dev, fr, light, want, "counter")
        assert ctx.last_kernel_name() == _packet(1)
        ctx.trace_soft_distance_stripes_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, 16, 2, 1, light=light)
        ctx.trace_soft_distance_stripes_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, 32, 3, 2, light=light)      # owns no band: no launch
        ctx.trace_soft_distance(fr.k, fr.pos, fr.W, fr.H, light=light)
        ctx.synchronize()
        assert ctx.get_option("soft_distance_traces") == n0 + 3
        assert {k: ctx.get_option(k) for k in keys} == before
        with pytest.raises(api.RtsError):                # read-only
            ctx.set_option("soft_distance_traces", 0)
        many = type(light).from_buffer_copy(light)
        many.nsamples, many.table = 65, 0
        with pytest.raises(api.RtsError):
            ctx.trace_soft_distance_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_dist, light=many)
        assert ctx.get_option("soft_distance_traces") == n0 + 3
        # the installed order still drives the plain trace, which still equals the oracle's count (the twin's mask, pinned to it on the CPU)
        ctx.h2d(dev.d_mask, np.full(fr.W * fr.H, GUARD_B, np.uint8))
        ctx.trace_shadow_mask_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_mask, light=light)
        ctx.synchronize()
        assert np.array_equal(dev.read()[1], want[1])
    finally:
        ctx.set_tile_order(None)
        ctx.set_option("kernel", -1)
        dev.close()


def _copy(struct):
    return type(struct).from_buffer_copy(struct)


@pytest.mark.parametrize("form", ["whole", "rows", "stripe"])
@pytest.mark.parametrize("kernel,split", [(3, 1), (3, 0), (7, 1)])
def test_device_forms_under_capture(ctx, kernel, split, form):
    fr = soft_frame(64, 48)
    want = fr.want(TABLE)
    ctx.set_bvh(fr.packed)
    dev = _Dev(ctx, fr.pos, fr.W, fr.H)
    checker = _maps(fr)["checker"]
    stream = ctx.stream_create()
    k, light = _copy(fr.k), _copy(fr.light(TABLE))
    g = None
    try:
        ctx.set_option("kernel", kernel)
        ctx.set_option("soft_split", split)
        ctx.h2d(dev.d_act, checker)
        ctx.trace_shadow_mask_device(fr.k, dev.d_pos, fr.W, fr.H, dev.d_mask, light=fr.light(TABLE), stream=stream)   # a stream that has traced
        ctx.synchronize(stream)
        rows = None
        if form == "whole":
            record = lambda: ctx.trace_soft_distance_device(k, dev.d_pos, fr.W, fr.H, dev.d_dist, d_mask=dev.d_mask, light=light,
                                                            stream=stream, d_active=dev.d_act)
        elif form == "rows":
            rows = (np.arange(fr.H) >= 5) & (np.arange(fr.H) < 41)
            record = lambda: ctx.trace_soft_distance_device(k, dev.d_pos, fr.W, fr.H, dev.d_dist, d_mask=dev.d_mask, light=light,
                                                            stream=stream, d_active=dev.d_act, row_begin=5, row_end=41)
        else:
            rows = ((np.arange(fr.H) // 16) % 2) == 1
            record = lambda: ctx.trace_soft_distance_stripes_device(k, dev.d_pos, fr.W, fr.H, dev.d_dist, 16, 2, 1, d_mask=dev.d_mask,
                                                                    light=light, stream=stream, d_active=dev.d_act)
        n0 = ctx.get_option("soft_distance_traces")
        g = hipgraph.capture(stream, record)
        assert ctx.get_option("soft_distance_traces") == n0 + 1
        types = g.node_types()
        assert types == [hipgraph.KERNEL], (kernel, split, form, types)   # one kernel node; no memcpy, memset or allocation node
        for s in (k, light):                             # what a caller may do to its structs between capture and replay
            C.memset(C.byref(s), 0x7F, C.sizeof(s))
        # the replay follows the buffers: the map the device holds at the replay, not the one it held at the capture
        for replay, active in enumerate((checker, (255 - checker).astype(np.uint8))):
            ctx.h2d(dev.d_act, active)
            dev.guard()
            g.launch(stream)
            _same(dev.read(stream), _expect(want, active, rows), (kernel, split, form, replay))
    finally:
        if g:
            g.close()
        ctx.synchronize(stream)
        ctx.stream_destroy(stream)
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)
        dev.close()
