"""GPU: the clamped forms of the moments pass (rtsh_accumulate_moments_soft_light_list_clamped_device and ..._clamped_motion_device;
accumulateMomentsClampedKernel<false> and <true> of raytracedshadows_amd/csrc/rts_moments.inc): the device forms equal the host twins
bit for bit (the twins equal the numpy rule in tests/test_list_moments_clamp_host.py).  Frames: (1, 1) and (3, 2) -- one block, most of
whose lanes lie outside the frame and must still reach every barrier --, (17, 1), (40, 40), (40, 72) and (72, 40): block edges that cut
windows in both axes.  Every frame runs once with all pointers as allocated and once with every buffer one ELEMENT into a larger
allocation.  Every output carries spare bytes preset to 0xAB that must come back unchanged.  No BVH is installed but in the chain
test."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import list_combine_cases as lc
import list_moments_cases as mc
import list_moments_clamp_cases as cc
import list_motion_cases as ms
import list_motion_edge_cases as ec
import list_temporal_cases as tc
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID = 1
f32, u32 = np.float32, np.uint32
FRAMES = [(1, 1), (3, 2), (17, 1), (40, 40), (40, 72), (72, 40)]
DTYPES = (np.uint16, np.uint32, np.uint8)
#: radius x sigma_k4 x margin 0 and 65535: forty selections per frame and shift
GRID = [(r, k, m) for r in cc.RADII for k in cc.SIGMA_K4 for m in (0, 65535)]


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def other_stream(ctx):
    s = ctx.stream_create()
    yield s
    ctx.stream_destroy(s)


class _Guarded:
    """A device buffer of shift + nbytes + 256 bytes, all of it preset to 0xAB; the payload starts `shift` bytes in."""

    def __init__(self, ctx, nbytes, shift):
        self.ctx, self.nbytes, self.shift = ctx, nbytes, shift
        self.base = ctx.malloc(shift + nbytes + GUARD)
        self.ptr = self.base + shift
        self.reset()

    def reset(self):
        self.ctx.h2d(self.base, np.full(self.shift + self.nbytes + GUARD, 0xAB, np.uint8))

    def raw(self):
        raw = np.zeros(self.shift + self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.base)
        return raw

    def read(self, shape, dtype=np.uint8):
        raw = self.raw()
        assert (raw[:self.shift] == 0xAB).all() and (raw[self.shift + self.nbytes:] == 0xAB).all(), "bytes around the buffer were written"
        return raw[self.shift:self.shift + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.raw() == 0xAB).all())

    def free(self):
        self.ctx.free(self.base)


class _Pool:
    """Device buffers that live as long as a test; `up` uploads an array `shift` ELEMENTS into its block."""

    def __init__(self, ctx, shift):
        self.ctx, self.shift, self.blocks = ctx, shift, []

    def up(self, array):
        a = np.ascontiguousarray(array)
        base = self.ctx.malloc(a.nbytes + 16)
        self.blocks.append(base)
        self.ctx.h2d(base + self.shift * a.itemsize, a)
        return base + self.shift * a.itemsize

    def raw(self, nbytes):
        base = self.ctx.malloc(nbytes)
        self.blocks.append(base)
        return base

    def out(self, n, dtype):
        g = _Guarded(self.ctx, 8 * n * np.dtype(dtype).itemsize, self.shift * np.dtype(dtype).itemsize)
        self.blocks.append(g)
        return g

    def free(self):
        for b in self.blocks:
            b.free() if isinstance(b, _Guarded) else self.ctx.free(b)


def _read_moments(outs, count, H, W):
    got = []
    for g, dtype in zip(outs, DTYPES):
        a = g.read((8, H, W), dtype)
        assert (a[count:].view(np.uint8) == 0xAB).all(), "a plane from the count up was written"
        got.append(a[:count])
    return tuple(got)


# ------------------------------------------------------------------------------------------------------------ device == twin
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("wh", FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_clamped_device_forms_equal_the_host_twins(ctx, other_stream, wh, shift):
    """Both kernels over every radius, the four sigma_k4 and margin 0 and 65535; lists of 1, 3 and 8 lights; the four motions of the
    camera and the stale history; max_length 1 (nothing is staged), 2, 5, 32; a reset light in the middle of a list, all lights reset;
    with and without the map; the first frame; one run per frame on a second stream."""
    W, H = wh
    n = W * H
    pool = _Pool(ctx, shift)
    try:
        outs = [pool.out(n, t) for t in DTYPES]
        dev = {}
        for i, (count, kind) in enumerate([(8, "pixels"), (3, "turn"), (1, "subpixel"), (8, "stale"), (3, "away")]):
            lst = mc.the_list(count, i % 4)
            c = cc.stale_case("turn", wh, lst) if kind == "stale" else mc.moments_case(kind, wh, lst)
            motion = ec.motion_planes(c, wh, i)
            d = {k: pool.up(c[k]) for k in ("pos", "nrm", "map", "counts")}
            d_prev = tuple(pool.up(a) for a in c["prev"])
            d_motion = tuple(pool.up(a) for a in motion)
            dev[i] = (lst, c, motion, d, d_prev, d_motion)
        for j, clamp in enumerate(GRID):
            lst, c, motion, d, d_prev, d_motion = dev[j % 5]
            max_length = (5, 32, 2, 1)[(j // 5 + j) % 4] if j % 11 else 1
            reset = (0, 0b010, 0, 0xFF, 0b101)[(j // 3) % 5]
            first = j % 13 == 12
            with_map = (j // 2) % 2 == 0
            p = tc.with_params(c["params"], max_length, reset)
            h_clamp = api.MomentsClamp.make(*clamp)
            for moving in (False, True):
                stream = other_stream if (j == 7 and moving) or (j == 22 and not moving) else None
                for g in outs:
                    g.reset()
                api.accumulate_moments_soft_light_list_device(ctx, lst, p, d["pos"], d["nrm"], d["counts"], W, H, *(g.ptr for g in outs),
                                                              d_prev=None if first else d_prev, d_lights_map=d["map"] if with_map else None,
                                                              stream=stream, d_motion=d_motion if moving else None, clamp=h_clamp)
                ctx.synchronize(stream)
                want = api.accumulate_moments_soft_light_list(lst, p, c["pos"], c["nrm"], c["counts"], None if first else c["prev"],
                                                              c["map"] if with_map else None, motion=motion if moving else None, clamp=h_clamp)
                mc.same_moments(_read_moments(outs, lst.count, H, W), want, (wh, shift, j, clamp, lst.count, max_length, reset, first, with_map, moving))
    finally:
        pool.free()


def test_the_selections_reach_what_the_docstring_says():
    runs = [((5, 32, 2, 1)[(j // 5 + j) % 4] if j % 11 else 1, (0, 0b010, 0, 0xFF, 0b101)[(j // 3) % 5], j % 13 == 12, j % 5) for j in range(len(GRID))]
    assert {r[0] for r in runs} == {1, 2, 5, 32} and {r[1] for r in runs} == {0, 0b010, 0xFF, 0b101}
    assert any(r[2] for r in runs) and {r[3] for r in runs} == set(range(5))
    assert any(m > 1 and reset == 0b010 and not first and case in (0, 3) for m, reset, first, case in runs), "a reset light inside eight"
    assert {g[0] for g in GRID} == set(cc.RADII) and {g[1] for g in GRID} == set(cc.SIGMA_K4) and len(GRID) == 40


# ------------------------------------------------------------------------------------------------------------ refusals, capture
@pytest.mark.parametrize("moving", [False, True], ids=["plain", "motion"])
def test_refusals_launch_nothing_and_capture_adds_one_kernel_node(ctx, other_stream, moving):
    lib = api._lib
    wh = (40, 40)
    W, H = wh
    lst = mc.the_list(4, 1)
    c = cc.stale_case("turn", wh, lst)
    motion = ec.motion_planes(c, wh)
    pool = _Pool(ctx, 0)
    h, v = ctx.handle, C.c_void_p
    ref = lambda s: C.byref(s) if s is not None else None
    try:
        outs = [pool.out(W * H, t) for t in DTYPES]
        d = {k: pool.up(c[k]) for k in ("pos", "nrm", "map", "counts")}
        prev = [pool.up(a) for a in c["prev"]]
        mot = [pool.up(a) for a in motion]
        good, clamp = tc.with_params(c["params"], 32, 0), api.MomentsClamp.make(4, 8, 0)
        _, soft_bad = lc.bad_lists()

        def call(lst_=lst, p=good, ctx_=h, nrm=d["nrm"], cnt=d["counts"], prev_=prev, mot_=mot, W_=W, H_=H, out=None, clamp_=clamp):
            out = out or [g.ptr for g in outs]
            if moving:
                return lib.rtsh_accumulate_moments_soft_light_list_clamped_motion_device(
                    ctx_, ref(lst_), ref(p), v(d["pos"]), v(nrm), v(d["map"]), v(cnt), *(v(a) for a in prev_), *(v(a) for a in mot_), W_, H_,
                    *(v(a) for a in out), ref(clamp_), None)
            return lib.rtsh_accumulate_moments_soft_light_list_clamped_device(ctx_, ref(lst_), ref(p), v(d["pos"]), v(nrm), v(d["map"]), v(cnt),
                                                                              *(v(a) for a in prev_), W_, H_, *(v(a) for a in out), ref(clamp_), None)

        assert call(clamp_=None) == INVALID
        for field, value in (("radius", 5), ("radius", 0xFFFFFFFF), ("sigma_k4", 256), ("margin", 65536)):
            bad = api.MomentsClamp.make(4, 8, 0)
            setattr(bad, field, value)
            assert call(clamp_=bad) == INVALID, (field, value)
        for b in soft_bad:
            assert call(lst_=b) == INVALID
        for field, value in (("max_length", 0), ("max_length", 256), ("plane_eps", np.nan), ("prev_scale_x", 0.0)):
            p = tc.with_params(good)
            setattr(p, field, value)
            assert call(p=p) == INVALID
        assert call(p=None) == INVALID and call(ctx_=None) == INVALID and call(nrm=0) == INVALID and call(cnt=0) == INVALID
        for i in range(3):
            assert call(out=[0 if j == i else g.ptr for j, g in enumerate(outs)]) == INVALID
            assert call(prev_=prev[:2] + [outs[j].ptr if j == i else prev[2 + j] for j in range(3)]) == INVALID
        for i in range(5):
            assert call(prev_=[0 if j == i else a for j, a in enumerate(prev)]) == INVALID
        assert call(W_=0) == INVALID and call(H_=0) == INVALID and call(W_=65537, H_=1) == INVALID
        if moving:
            assert call(mot_=[0, mot[1]]) == INVALID and call(mot_=[mot[0], 0]) == INVALID
        ctx.synchronize()
        assert all(g.untouched() for g in outs)
        # under capture: one kernel node, list, params and clamp by value; two replays, the second over changed counts
        p, k = tc.with_params(good), api.MomentsClamp.make(4, 8, 0)
        launch = lambda: api.accumulate_moments_soft_light_list_device(ctx, lst, p, d["pos"], d["nrm"], d["counts"], W, H, *(g.ptr for g in outs),
                                                                       d_prev=tuple(prev), d_lights_map=d["map"], stream=other_stream,
                                                                       d_motion=tuple(mot) if moving else None, clamp=k)
        twin = lambda counts: api.accumulate_moments_soft_light_list(lst, good, c["pos"], c["nrm"], counts, c["prev"], c["map"],
                                                                     motion=motion if moving else None, clamp=clamp)
        g = hipgraph.capture(other_stream, launch)
        try:
            assert g.node_types() == [hipgraph.KERNEL], g.node_types()
            assert all(o.untouched() for o in outs), "the capture itself ran a kernel"
            p.max_length, p.reset_lights = 1, 0xFF                       # by value: the graph holds its own copies
            k.radius, k.sigma_k4, k.margin = 0, 255, 65535
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            want = twin(c["counts"])
            unclamped = api.accumulate_moments_soft_light_list(lst, good, c["pos"], c["nrm"], c["counts"], c["prev"], c["map"],
                                                               motion=motion if moving else None)
            assert (want[0] != unclamped[0]).sum() > 100, "the clamp never bit"
            mc.same_moments(_read_moments(outs, 4, H, W), want, "first replay")
            changed = np.ascontiguousarray(c["counts"][:, ::-1, ::-1] // 2)
            ctx.h2d(d["counts"], changed)
            g.launch(other_stream)
            ctx.synchronize(other_stream)
            want2 = twin(changed)
            assert (want2[0] != want[0]).any()
            mc.same_moments(_read_moments(outs, 4, H, W), want2, "replay over changed counts")
        finally:
            g.close()
    finally:
        pool.free()


# ------------------------------------------------------------------------------------------------------------ the chain
def test_three_frame_chain_equals_the_chain_of_host_twins(ctx):
    """snapshot, refit, motion G-buffer, soft light list trace, clamped motion moments, guided temporal mean filter, combine: three
    frames on the device, the box moving a third of T per frame, the histories ping-ponged, equal the same chain through the host
    twins byte for byte; the moved box keeps a history of length 3."""
    W, H = 72, 40
    n = W * H
    sc = ms._scene("cornell")
    s = ms.streams("cornell", "static")
    idx, P = np.ascontiguousarray(sc["faces"].reshape(-1)), sc["faces"].shape[0]
    vid = np.unique(sc["faces"][sc["part"]])
    nv = s["packed"].shape[0]
    entries = [(api.Light.POINT, [5.0, 9.5, 5.0], 4, 0, 1.0), (api.Light.POINT, [2.0, 9.0, 8.0], 16, 4, 0.3), (api.Light.POINT, [7.0, 7.0, 4.0], 1, 0, 0.0)]
    from raytracedshadows_amd import scenes
    lst = api.SoftLightList.make(entries, scenes.jitter_offsets(48, 1.0, 19))
    hard = lst.hard_list()
    fp = api.WideGuideTemporalParams.make(2, 12, 2, 0.9, 0.05)
    clamp = api.MomentsClamp.make(2, 8, 0)
    eyes = [s["eye"], (s["eye"] + np.array([0.1, 0.0, 0.05], f32)).astype(f32), (s["eye"] + np.array([0.2, 0.05, 0.1], f32)).astype(f32)]
    pool = _Pool(ctx, 0)
    try:
        ctx.set_bvh(s["packed"])
        d_snap = pool.raw(nv * 16)
        g = [{k: pool.raw(n * 16) for k in ("pos", "nrm", "pts", "pnr")} for _ in range(2)]
        d_counts, d_vis, d_rgb, d_scratch = pool.raw(8 * n), pool.raw(32 * n), pool.raw(3 * n), pool.raw(48 * n)
        d_mom = [[pool.out(n, t) for t in DTYPES] for _ in range(2)]
        host_prev_stream, host_prev, mom, pts = s["packed"], None, None, None
        for k in range(3):
            verts = sc["verts"].copy()
            verts[vid] += ms.T * (k / 3.0)
            verts = np.ascontiguousarray(verts, f32)
            eye, prev_eye = eyes[k], eyes[max(k - 1, 0)]
            constants = api.RayTracingConstants.make(eye, (0.3, 1.0, 0.2), W, H)
            p = ms.params_of(s, (W, H), eye, prev_eye)
            # the chain of host twins
            packed = api.bvh_refit(s["packed"], verts, 3, idx, P)
            pos, nrm, pts, pnr, _, _ = api.primary_gbuffer_motion(packed, host_prev_stream, eye, prev_eye, s["target"], s["fovy"], W, H, want_leaves=False)
            counts = api.soft_light_list(packed, constants, lst, pos, W, H)
            mom = api.accumulate_moments_soft_light_list(lst, p, pos, nrm, counts, None if k == 0 else host_prev + mom, motion=(pts, pnr), clamp=clamp)
            vis = api.wide_filter_guided_temporal_mean_soft_light_list(lst, fp, pos, nrm, counts, mom)
            rgb = api.combine_visibility_list(constants, hard, pos, nrm, vis)
            host_prev_stream, host_prev = packed, (pos, nrm)
            # the device chain
            cur, prv = g[k % 2], g[1 - k % 2]
            o, h = d_mom[k % 2], d_mom[1 - k % 2]
            api.snapshot_bvh_device(ctx, d_snap, nv)
            api.bvh_refit_device(ctx, verts, 3, idx, P)
            api.primary_gbuffer_motion_device(ctx, d_snap, nv, eye, prev_eye, s["target"], s["fovy"], W, H, cur["pos"], cur["nrm"], cur["pts"], cur["pnr"])
            ctx.trace_soft_light_list_device(constants, lst, cur["pos"], W, H, d_counts)
            api.accumulate_moments_soft_light_list_device(ctx, lst, p, cur["pos"], cur["nrm"], d_counts, W, H, *(b.ptr for b in o),
                                                          d_prev=None if k == 0 else (prv["pos"], prv["nrm"]) + tuple(b.ptr for b in h),
                                                          d_motion=(cur["pts"], cur["pnr"]), clamp=clamp)
            api.wide_filter_guided_temporal_mean_soft_light_list_device(ctx, lst, fp, cur["pos"], cur["nrm"], d_counts, tuple(b.ptr for b in o),
                                                                        W, H, d_vis, d_scratch=d_scratch)
            api.combine_visibility_list_device(ctx, constants, hard, cur["pos"], cur["nrm"], d_vis, W, H, d_rgb)
            ctx.synchronize()
            mc.same_moments(_read_moments(o, 3, H, W), mom, ("chain, moments", k))
            got_vis, got_rgb = np.zeros((8, H, W), f32), np.zeros((H, W, 3), np.uint8)
            ctx.d2h(got_vis, d_vis)
            ctx.d2h(got_rgb, d_rgb)
            assert (got_vis[:3].view(u32) == vis.view(u32)).all(), ("chain, filtered mean", k)
            assert (got_rgb == rgb).all(), ("chain, image", k)
        assert mom[2].max() == 3 and (mom[2][0][pts[..., 3] == 2] == 3).any(), "the chain must follow the moving box"
        unclamped = api.accumulate_moments_soft_light_list(lst, p, pos, nrm, counts, None, motion=(pts, pnr))
        assert unclamped[2].max() == 1
    finally:
        pool.free()
