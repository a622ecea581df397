"""GPU: the four kernels of raytracedshadows_amd/csrc/rts_primary.hip -- gbufferKernel, combineKernel, facingKernel and
facingLightsKernel -- on the awkward inputs of tests/scene_pass_cases.py, against the oracle and the float32 numpy rules (the host
twins are not the checker here).  Every comparison is bit for bit, every output buffer carries 256 spare bytes preset to 0xAB that
must come back unchanged, and every refusal must leave its buffers untouched."""
import ctypes as C

import numpy as np
import pytest

import oracle
import scene_pass_cases as sp
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID, NO_BVH = 1, 4


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


class _Guarded:
    """A device buffer of nbytes + 256, all of it preset to 0xAB."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = ctx.malloc(nbytes + GUARD)
        self.reset()

    def reset(self):
        self.ctx.h2d(self.ptr, np.full(self.nbytes + GUARD, 0xAB, np.uint8))

    def read(self, dtype, shape):
        """The payload; asserts the spare bytes."""
        raw = np.zeros(self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.ptr)
        assert (raw[self.nbytes:] == 0xAB).all(), "bytes behind the buffer were written"
        return raw[:self.nbytes].view(dtype).reshape(shape)

    def untouched(self):
        raw = np.zeros(self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.ptr)
        return bool((raw == 0xAB).all())

    def free(self):
        self.ctx.free(self.ptr)


def _same(got, want, what):
    g, w = (sp.bits(got), sp.bits(want)) if got.dtype == np.float32 else (got, want)
    bad = np.argwhere(g != w)
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def _gbuffer_on_the_device(ctx, case, want_pos, want_nrm):
    name, packed, eye, target, fovy, W, H, _ = case
    ctx.set_bvh(packed)
    d_pos, d_nrm = _Guarded(ctx, W * H * 16), _Guarded(ctx, W * H * 16)
    try:
        api.primary_gbuffer_device(ctx, eye, target, fovy, W, H, d_pos.ptr, d_nrm.ptr)
        ctx.synchronize()
        _same(d_pos.read(np.float32, (H, W, 4)), want_pos, name + " positions")
        _same(d_nrm.read(np.float32, (H, W, 4)), want_nrm, name + " normals")
        d_pos.reset()
        d_nrm.reset()
        api.primary_gbuffer_device(ctx, eye, target, fovy, W, H, d_pos.ptr, None)
        ctx.synchronize()
        _same(d_pos.read(np.float32, (H, W, 4)), want_pos, name + " positions, no normals")
        assert d_nrm.untouched()
    finally:
        d_pos.free()
        d_nrm.free()


@pytest.mark.parametrize("name", sp.gbuffer_names())
def test_gbuffer_on_the_device_equals_the_oracle(ctx, name):
    want_pos, want_nrm, _ = sp.oracle_gbuffer(name)
    _gbuffer_on_the_device(ctx, sp.gbuffer_case(name), want_pos, want_nrm)


def test_tallest_frame_equals_the_oracle_and_a_taller_one_is_refused(ctx):
    """W = 1, H = 8 * 65535 fills the grid's y extent; one row more is RTS_ERR_INVALID_ARG before any launch, nothing written."""
    case = sp.tall_case()
    name, packed, eye, target, fovy, W, H, _ = case
    assert H == 8 * 65535
    want_pos, want_nrm, hits = oracle.primary_gbuffer(packed, eye, target, fovy, W, H)
    assert 0 < hits < H
    _gbuffer_on_the_device(ctx, case, want_pos, want_nrm)
    d_pos, d_nrm = _Guarded(ctx, (H + 1) * 16), _Guarded(ctx, (H + 1) * 16)
    try:
        e = (C.c_float * 3)(*eye)
        t = (C.c_float * 3)(*target)
        st = api._lib.rtsh_primary_gbuffer_device(ctx.handle, e, t, fovy, 1, H + 1, C.c_void_p(d_pos.ptr), C.c_void_p(d_nrm.ptr), None)
        ctx.synchronize()
        assert st == INVALID
        assert d_pos.untouched() and d_nrm.untouched()
    finally:
        d_pos.free()
        d_nrm.free()


class _Table:
    """A texel table on the device, and guarded outputs for the three passes."""

    def __init__(self, ctx, shape):
        self.ctx, self.shape = ctx, shape
        H, W = shape
        self.nrm, self.pos, self.mask = sp.texels(shape)
        self.d_nrm, self.d_pos, self.d_mask = ctx.malloc(self.nrm.nbytes), ctx.malloc(self.pos.nbytes), ctx.malloc(max(self.mask.nbytes, 1))
        ctx.h2d(self.d_nrm, self.nrm)
        ctx.h2d(self.d_pos, self.pos)
        ctx.h2d(self.d_mask, self.mask)
        self.rgb, self.byte = _Guarded(ctx, H * W * 3), _Guarded(ctx, H * W)

    def free(self):
        for p in (self.d_nrm, self.d_pos, self.d_mask):
            self.ctx.free(p)
        self.rgb.free()
        self.byte.free()


@pytest.fixture(scope="module", params=sp.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def table(ctx, request):
    t = _Table(ctx, request.param)
    yield t
    t.free()


@pytest.fixture(scope="module")
def streams_(ctx):
    s = ctx.stream_create()
    yield (None, s)
    ctx.stream_destroy(s)


def test_combine_on_the_device_equals_the_oracle_and_the_rule(ctx, table, streams_):
    H, W = table.shape
    lights = sp.lights()
    for kind, name, with_pos in sp.pass_runs():
        k, light = sp.constants(kind), lights[name]
        p = table.pos if with_pos else None
        want = sp.oracle_combine(k, light, p, table.nrm, table.mask)
        assert np.array_equal(want, sp.combine_rule(k, light, p, table.nrm, table.mask))
        for stream in streams_:
            table.rgb.reset()
            api.combine_device(ctx, k, light, table.d_pos if with_pos else None, table.d_nrm, table.d_mask, W, H, table.rgb.ptr, stream)
            ctx.synchronize(stream)
            got = table.rgb.read(np.uint8, (H, W, 3))
            bad = np.argwhere((got != want).any(axis=-1))
            assert bad.shape[0] == 0, (table.shape, kind, name, with_pos, stream is not None, bad.shape[0],
                                       [(table.nrm[y, x, :3].tolist(), table.pos[y, x, :3].tolist(), int(table.mask[y, x]), int(got[y, x, 0]),
                                         int(want[y, x, 0])) for y, x in bad[:6].tolist()])


def test_facing_mark_on_the_device_equals_the_rule(ctx, table, streams_):
    H, W = table.shape
    lights = sp.lights()
    for kind, name, with_pos in sp.pass_runs():
        k, light = sp.constants(kind), lights[name]
        want = sp.facing_rule(k, light, table.pos if with_pos else None, table.nrm)
        for stream in streams_:
            table.byte.reset()
            api.facing_active_device(ctx, k, light, table.d_pos if with_pos else None, table.d_nrm, W, H, table.byte.ptr, stream)
            ctx.synchronize(stream)
            got = table.byte.read(np.uint8, (H, W))
            assert np.array_equal(got, want), (table.shape, kind, name, with_pos, stream is not None, np.argwhere(got != want)[:8].tolist())


def test_light_map_on_the_device_equals_the_rule(ctx, table, streams_):
    H, W = table.shape
    k = sp.constants("unit")
    for name, (lst, has_point) in sp.light_lists().items():
        for with_pos in ((True,) if has_point else (True, False)):
            want = sp.facing_lights_rule(k, lst, table.pos if with_pos else None, table.nrm)
            for stream in streams_:
                table.byte.reset()
                api.facing_lights_device(ctx, k, lst, table.d_pos if with_pos else None, table.d_nrm, W, H, table.byte.ptr, stream)
                ctx.synchronize(stream)
                got = table.byte.read(np.uint8, (H, W))
                assert np.array_equal(got, want), (table.shape, name, with_pos, stream is not None, np.argwhere(got != want)[:8].tolist())


def test_refusals_write_nothing(ctx):
    """A null context, null normals, zero W or H, a point light without positions, a list with a point light without positions, and
    no installed stream: the status, and not a byte of the outputs."""
    lib = api._lib
    t = _Table(ctx, (16, 16))
    gpos, gnrm = _Guarded(ctx, 16 * 16 * 16), _Guarded(ctx, 16 * 16 * 16)
    k = sp.constants("unit")
    point = sp.lights()["point1"]
    lst3 = sp.light_lists()["3"][0]
    v = C.c_void_p
    e = (C.c_float * 3)(0, 0, 0)
    tg = (C.c_float * 3)(0, 0, -1)
    h = ctx.handle
    try:
        ctx.set_bvh(sp.one_triangle())
        assert lib.rtsh_primary_gbuffer_device(None, e, tg, 1.0, 16, 16, v(gpos.ptr), v(gnrm.ptr), None) == INVALID
        assert lib.rtsh_primary_gbuffer_device(h, None, tg, 1.0, 16, 16, v(gpos.ptr), v(gnrm.ptr), None) == INVALID
        assert lib.rtsh_primary_gbuffer_device(h, e, None, 1.0, 16, 16, v(gpos.ptr), v(gnrm.ptr), None) == INVALID
        assert lib.rtsh_primary_gbuffer_device(h, e, tg, 1.0, 16, 16, None, v(gnrm.ptr), None) == INVALID
        assert lib.rtsh_primary_gbuffer_device(h, e, tg, 1.0, 0, 16, v(gpos.ptr), v(gnrm.ptr), None) == INVALID
        assert lib.rtsh_primary_gbuffer_device(h, e, tg, 1.0, 16, 0, v(gpos.ptr), v(gnrm.ptr), None) == INVALID
        with api.ShadowContext(0) as empty:
            assert lib.rtsh_primary_gbuffer_device(empty.handle, e, tg, 1.0, 16, 16, v(gpos.ptr), v(gnrm.ptr), None) == NO_BVH
            with pytest.raises(api.RtsError) as err:
                api.primary_gbuffer_device(empty, (0, 0, 0), (0, 0, -1), 1.0, 16, 16, gpos.ptr, gnrm.ptr)
            assert err.value.status == NO_BVH

        kk = C.byref(k)
        args = (v(t.d_pos), v(t.d_nrm), v(t.d_mask), 16, 16, v(t.rgb.ptr), None)
        assert lib.rtsh_combine_device(None, kk, None, *args) == INVALID
        assert lib.rtsh_combine_device(h, None, None, *args) == INVALID
        assert lib.rtsh_combine_device(h, kk, None, v(t.d_pos), None, v(t.d_mask), 16, 16, v(t.rgb.ptr), None) == INVALID
        assert lib.rtsh_combine_device(h, kk, None, v(t.d_pos), v(t.d_nrm), None, 16, 16, v(t.rgb.ptr), None) == INVALID
        assert lib.rtsh_combine_device(h, kk, None, v(t.d_pos), v(t.d_nrm), v(t.d_mask), 0, 16, v(t.rgb.ptr), None) == INVALID
        assert lib.rtsh_combine_device(h, kk, None, v(t.d_pos), v(t.d_nrm), v(t.d_mask), 16, 0, v(t.rgb.ptr), None) == INVALID
        assert lib.rtsh_combine_device(h, kk, C.byref(point), None, v(t.d_nrm), v(t.d_mask), 16, 16, v(t.rgb.ptr), None) == INVALID

        assert lib.rtsh_facing_active_device(None, kk, None, v(t.d_pos), v(t.d_nrm), 16, 16, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_active_device(h, None, None, v(t.d_pos), v(t.d_nrm), 16, 16, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_active_device(h, kk, None, v(t.d_pos), None, 16, 16, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_active_device(h, kk, None, v(t.d_pos), v(t.d_nrm), 0, 16, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_active_device(h, kk, None, v(t.d_pos), v(t.d_nrm), 16, 0, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_active_device(h, kk, C.byref(point), None, v(t.d_nrm), 16, 16, v(t.byte.ptr), None) == INVALID

        ll = C.byref(lst3)
        assert lib.rtsh_facing_lights_device(None, kk, ll, v(t.d_pos), v(t.d_nrm), 16, 16, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_lights_device(h, None, ll, v(t.d_pos), v(t.d_nrm), 16, 16, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_lights_device(h, kk, None, v(t.d_pos), v(t.d_nrm), 16, 16, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_lights_device(h, kk, ll, v(t.d_pos), None, 16, 16, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_lights_device(h, kk, ll, v(t.d_pos), v(t.d_nrm), 0, 16, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_lights_device(h, kk, ll, v(t.d_pos), v(t.d_nrm), 16, 0, v(t.byte.ptr), None) == INVALID
        assert lib.rtsh_facing_lights_device(h, kk, ll, None, v(t.d_nrm), 16, 16, v(t.byte.ptr), None) == INVALID       # a point light in the list
        ctx.synchronize()
        assert gpos.untouched() and gnrm.untouched() and t.rgb.untouched() and t.byte.untouched()
    finally:
        t.free()
        gpos.free()
        gnrm.free()
