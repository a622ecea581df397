"""GPU: the temporal accumulation of the bent texel and the wide bent filter fed from it (rtsh_accumulate_bent_device,
rtsh_accumulate_bent_motion_device, rtsh_wide_filter_bent_mean_device; raytracedshadows_amd/csrc/rts_bent_temporal.inc, included by
rts_primary.hip): device = host twin = the numpy rules of tests/ao_bent_temporal_cases.py, bit for bit.  Every output
carries 256 spare bytes preset to 0xAB on both sides that must come back unchanged; the filter's scratch stays untouched in its second
half for passes <= 2 and altogether for passes <= 1."""
import ctypes as C

import numpy as np
import pytest

import ao_bent_cases as bc
import ao_bent_filter_cases as bf
import ao_bent_temporal_cases as bt
import hipgraph
import list_motion_cases as ms
import list_temporal_cases as tc
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

INVALID = 1
f32, u64 = np.float32, np.uint64
SAMPLES = (4, 48)
MAX_LENGTHS = (1, 5, 255)
CANARY = 0xABABABABABABABAB


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


GUARD = 256


class _Guarded:
    """A device buffer of 256 + nbytes + 256 bytes, all of it preset to 0xAB; the payload starts 256 bytes in (16-byte aligned)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.base = ctx.malloc(2 * GUARD + nbytes)
        self.ptr = self.base + GUARD
        self.reset()

    def reset(self):
        self.ctx.h2d(self.base, np.full(2 * GUARD + self.nbytes, 0xAB, np.uint8))

    def raw(self):
        raw = np.zeros(2 * GUARD + self.nbytes, np.uint8)
        self.ctx.d2h(raw, self.base)
        return raw

    def read(self, shape, dtype=np.uint8):
        raw = self.raw()
        assert (raw[:GUARD] == 0xAB).all() and (raw[GUARD + self.nbytes:] == 0xAB).all(), "bytes around the buffer were written"
        return raw[GUARD:GUARD + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.raw() == 0xAB).all())

    def free(self):
        self.ctx.free(self.base)


class _Frame:
    """Both frames of a pair on the device, with guarded texels_out, lengths_out, out, ao and scratch."""

    PLANES = (("pos", 16), ("nrm", 16), ("bent", 16), ("ppos", 16), ("pnrm", 16), ("ptex", 8), ("plen", 1), ("act", 1), ("pts", 16), ("pnr", 16))

    def __init__(self, ctx, W, H):
        self.ctx, self.W, self.H = ctx, W, H
        n = W * H
        self.d = {name: ctx.malloc(n * size + 16) for name, size in self.PLANES}
        self.texels, self.lengths = _Guarded(ctx, n * 8), _Guarded(ctx, n)
        self.out, self.ao, self.scratch = _Guarded(ctx, n * 16), _Guarded(ctx, n * 4), _Guarded(ctx, 2 * n * 8)

    def upload(self, **planes):
        for name, a in planes.items():
            if a is not None:
                self.ctx.h2d(self.d[name], np.ascontiguousarray(a))

    def launch(self, p, n, history=True, with_active=True, motion=False, stream=None, texels_out=None, lengths_out=None, d_prev=None):
        d = self.d
        prev = d_prev or ((d["ppos"], d["pnrm"], d["ptex"], d["plen"]) if history else None)
        api.accumulate_bent_device(self.ctx, p, n, d["pos"], d["nrm"], d["bent"], self.W, self.H, texels_out or self.texels.ptr,
                                   lengths_out or self.lengths.ptr, d_prev=prev, d_active=d["act"] if with_active else None,
                                   d_motion=(d["pts"], d["pnr"]) if motion else None, stream=stream)

    def run(self, p, n, history=True, with_active=True, motion=False, stream=None):
        self.texels.reset()
        self.lengths.reset()
        self.launch(p, n, history, with_active, motion, stream)
        self.ctx.synchronize(stream)
        return self.texels.read((self.H, self.W), u64), self.lengths.read((self.H, self.W))

    def launch_filter(self, p, n, d_texels, with_active=True, stream=None, scratch=True, ao=True):
        api.wide_filter_bent_mean_device(self.ctx, p, n, self.d["pos"], self.d["nrm"], d_texels, self.W, self.H, self.out.ptr,
                                         d_ao=self.ao.ptr if ao else None, d_scratch=self.scratch.ptr if scratch else None,
                                         d_active=self.d["act"] if with_active else None, stream=stream)

    def run_filter(self, p, n, d_texels, with_active=True, stream=None, scratch=True, ao=True):
        for g in (self.out, self.ao, self.scratch):
            g.reset()
        self.launch_filter(p, n, d_texels, with_active, stream, scratch, ao)
        self.ctx.synchronize(stream)
        mid = self.scratch.read((2, self.W * self.H), u64)
        if p.passes <= 2:
            assert (mid[1] == CANARY).all(), "the second half of the scratch was written"
        if p.passes <= 1:
            assert (mid[0] == CANARY).all(), "the scratch was written"
        plane = self.ao.read((self.H, self.W), f32)
        if not ao:
            assert (plane.view(np.uint32) == 0xABABABAB).all(), "ao was written"
        return self.out.read((self.H, self.W, 4), f32), plane if ao else None

    def free(self):
        for p in self.d.values():
            self.ctx.free(p)
        for g in (self.texels, self.lengths, self.out, self.ao, self.scratch):
            g.free()


def _upload_case(f, c):
    f.upload(pos=c["pos"], nrm=c["nrm"], bent=c["bent"], ppos=c["prev"][0], pnrm=c["prev"][1], ptex=c["prev"][2], plen=c["prev"][3],
             act=c["active"])


@pytest.mark.parametrize("wh", bt.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("motion", bt.MOTIONS)
def test_accumulate_device_equals_the_twin_and_the_rule(ctx, other_stream, motion, wh):
    """The four motions on the four frames; n of 4 and 48; max_length 1, 5, 255; with and without `active`; with and without the reset
    bit; the first frame; one run per case on a second stream."""
    f = _Frame(ctx, *wh)
    try:
        for n in SAMPLES:
            c = bt.case(motion, wh, n)
            _upload_case(f, c)
            for max_length in MAX_LENGTHS:
                for with_active in (True, False):
                    for reset in (0, 1):
                        p = tc.with_params(c["params"], max_length, reset)
                        a = c["active"] if with_active else None
                        stream = other_stream if max_length == 255 and with_active else None
                        got = f.run(p, n, True, with_active, stream=stream)
                        what = (motion, wh, n, max_length, with_active, reset)
                        bt.same_texels(got, bt.accumulate_rule(p, n, c["pos"], c["nrm"], c["bent"], c["prev"], a), what)
                        bt.same_texels(got, api.accumulate_bent(p, n, c["pos"], c["nrm"], c["bent"], c["prev"], a), what + ("twin",))
            got = f.run(c["params"], n, False)
            bt.same_texels(got, bt.accumulate_rule(c["params"], n, c["pos"], c["nrm"], c["bent"], None, c["active"]), (motion, wh, n, "first"))
    finally:
        f.free()


@pytest.mark.parametrize("wh", ms.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_motion_kernel_on_moved_streams(ctx, wh):
    """accumulateBentMotionKernel over list_motion_cases' moved streams (the G-buffers and motion planes of the host pass)."""
    f = _Frame(ctx, *wh)
    try:
        texels, lengths = bt.history(wh)
        active, bent = bt.active_plane(wh, 1), bf.synthetic_bent(wh, 4)
        for name, move, camera in (("cornell", "translate", "moved"), ("terrain", "rotate", "still"), ("cornell", "degenerate", "moved")):
            fr = bt.pair(name, move, wh, camera)
            f.upload(pos=fr["pos"], nrm=fr["nrm"], bent=bent, ppos=fr["prev_pos"], pnrm=fr["prev_nrm"], ptex=texels, plen=lengths, act=active,
                     pts=fr["pts"], pnr=fr["pnr"])
            prev, mo = (fr["prev_pos"], fr["prev_nrm"], texels, lengths), (fr["pts"], fr["pnr"])
            for max_length in (2, 255):
                p = tc.with_params(fr["params"], max_length, 0)
                got = f.run(p, 4, True, True, motion=True)
                bt.same_texels(got, bt.accumulate_motion_rule(p, 4, fr["nrm"], bent, prev, active, mo), (name, move, wh, max_length))
                bt.same_texels(got, api.accumulate_bent(p, 4, fr["pos"], fr["nrm"], bent, prev, active, motion=mo), (name, move, wh, "twin"))
            got = f.run(fr["params"], 4, False, True, motion=True)             # the first frame reads neither motion plane
            bt.same_texels(got, bt.accumulate_rule(fr["params"], 4, fr["pos"], fr["nrm"], bent, None, active), (name, move, wh, "first"))
    finally:
        f.free()


@pytest.mark.parametrize("wh", [(72, 40), (72, 72), (17, 1), (3, 2)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_mean_filter_device_equals_the_twin_and_the_rule(ctx, other_stream, wh):
    """passes 0 .. 5 (the conversion, dense steps 1, 2, 4, direct 8, 16) over an awkward texel plane and over an accumulated one; the
    scratch rules; one run on a second stream, one without `ao`, the passes <= 1 runs of one case without scratch."""
    if wh == (72, 72):
        c = dict(bt.case("pixels", (72, 40), 4))
        tall = tc.geometric("pixels", wh)
        c.update(pos=tall["pos"], nrm=tall["nrm"], active=bt.active_plane(wh))
        planes = [bt.history(wh)[0]]
    else:
        c = bt.case("pixels", wh, 4)
        planes = [c["prev"][2], api.accumulate_bent(tc.with_params(c["params"], 255, 0), 4, c["pos"], c["nrm"], c["bent"], c["prev"], c["active"])[0]]
    f = _Frame(ctx, *wh)
    try:
        f.upload(pos=c["pos"], nrm=c["nrm"], act=c["active"])
        for i, plane in enumerate(planes):
            f.upload(ptex=plane)
            for n in SAMPLES:
                for with_active in (True, False):
                    a = c["active"] if with_active else None
                    want = bt.mean_filter_rule(bf.params(0), n, c["pos"], c["nrm"], plane, a)
                    for passes in bt.PASSES:
                        p = bf.params(passes)
                        stream = other_stream if passes == 3 and n == 4 else None
                        with_ao = not (passes == 4 and n == 48)
                        got, ao = f.run_filter(p, n, f.d["ptex"], with_active, stream, scratch=not (passes <= 1 and n == 48), ao=with_ao)
                        what = (wh, i, n, with_active, passes)
                        bf.same_bits(got, want[passes], what)
                        if with_ao:
                            bf.same_bits(ao, want[passes][..., 3], what + ("ao",))
                        bf.same_bits(got, api.wide_filter_bent_mean(p, n, c["pos"], c["nrm"], plane, a)[0], what + ("twin",))
    finally:
        f.free()


def test_graph_capture_node_counts_and_replay(ctx, other_stream):
    """Captured, an accumulate is ONE kernel node and the filter max(1, passes), parameters by value; a replay gives the eager bytes."""
    wh, n = (72, 40), 4
    c = bt.case("turn", wh, n)
    f = _Frame(ctx, *wh)
    try:
        _upload_case(f, c)
        for motion in (False, True):
            if motion:
                f.upload(pts=c["pos"], pnr=c["nrm"])
            p = tc.with_params(c["params"], 5, 0)
            eager = f.run(p, n, motion=motion)
            f.texels.reset()
            f.lengths.reset()
            g = hipgraph.capture(other_stream, lambda: f.launch(p, n, motion=motion, stream=other_stream))
            try:
                assert g.node_types() == [hipgraph.KERNEL], g.node_types()
                assert f.texels.untouched() and f.lengths.untouched(), "the capture itself ran a kernel"
                p.max_length = 1                                             # by value: the graph holds its own copy
                g.launch(other_stream)
                ctx.synchronize(other_stream)
                bt.same_texels((f.texels.read((wh[1], wh[0]), u64), f.lengths.read((wh[1], wh[0]))), eager, ("replay", motion))
            finally:
                g.close()
        for passes in (0, 1, 2, 5):
            p = bf.params(passes)
            eager, eager_ao = f.run_filter(p, n, f.d["ptex"])
            for guard in (f.out, f.ao, f.scratch):
                guard.reset()
            g = hipgraph.capture(other_stream, lambda: f.launch_filter(p, n, f.d["ptex"], stream=other_stream))
            try:
                assert g.node_types() == [hipgraph.KERNEL] * max(1, passes), (passes, g.node_types())
                assert f.out.untouched() and f.ao.untouched() and f.scratch.untouched(), "the capture itself ran a kernel"
                p.passes = (passes + 1) % 6
                g.launch(other_stream)
                ctx.synchronize(other_stream)
                bf.same_bits(f.out.read((wh[1], wh[0], 4), f32), eager, ("filter replay", passes))
                bf.same_bits(f.ao.read((wh[1], wh[0]), f32), eager_ao, ("filter replay, ao", passes))
            finally:
                g.close()
    finally:
        f.free()


def _crop_camera(pos, nrm, W, H, max_length):
    """A previous camera at the origin of the crop's camera-relative positions that sees every surface point of the crop inside a W x H
    frame -- not the crop's own (an off-centre window of a larger frame has none in rtsh_temporal_params), but close to it: most points
    land near their own pixel and find their own surface there."""
    on = (nrm[..., :3] != 0).any(-1)
    P = pos[..., :3][on].astype(np.float64)
    fwd = P.mean(0) / np.linalg.norm(P.mean(0))
    right = np.cross(fwd, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    z = P @ fwd
    sx, sy = np.abs(P @ right / z).max() * 1.02, np.abs(P @ up / z).max() * 1.02
    return api.TemporalParams.make((0.0, 0.0, 0.0), right, up, fwd, sx, sy, 0.9, 0.05 * float(np.abs(P).max()), max_length, 0)


def test_chained_frame_loop_on_the_device(ctx):
    """Three frames on the cornell crop (48, 40), n = 4, table 64: trace_ambient_occlusion_bent_device with dirs turned per frame ->
    accumulate with ping-pong -> 2 passes over the mean -> the bent combine; no plane goes through the host between the stages, and
    every plane is checked against the same chain of host twins (the trace's: the numpy rule of ao_bent_cases over the oracle)."""
    n, frames = 4, 3
    fr, ao0, _, _ = bf.traced("cornell_128", 48, 40, n, 64, 0.5)
    W, H = fr.W, fr.H
    k, lst, _, _, vis, _, _, sky, _, colors = bc.combine_case(W, H)
    p = _crop_camera(fr.pos, fr.nrm, W, H, 255)
    fp = bf.traced_params(fr, 2)
    f = _Frame(ctx, W, H)
    ping = [(_Guarded(ctx, W * H * 8), _Guarded(ctx, W * H)) for _ in range(2)]
    d_counts, d_vis, d_rgb = ctx.malloc(W * H), ctx.malloc(vis.nbytes), _Guarded(ctx, W * H * 3)
    try:
        ctx.set_bvh(fr.packed)
        f.upload(pos=fr.pos, nrm=fr.nrm, ppos=fr.pos, pnrm=fr.nrm)
        ctx.h2d(d_vis, np.ascontiguousarray(vis))
        host_prev = None
        for frame in range(frames):
            ao = ao0.rotated(frame)
            ctx.trace_ambient_occlusion_bent_device(fr.k, ao, f.d["pos"], f.d["nrm"], W, H, d_counts, f.d["bent"])
            cur, old = ping[frame & 1], ping[(frame + 1) & 1]
            prev = (f.d["ppos"], f.d["pnrm"], old[0].ptr, old[1].ptr) if frame else None
            f.launch(p, n, history=False, with_active=False, texels_out=cur[0].ptr, lengths_out=cur[1].ptr, d_prev=prev)
            ctx.synchronize()
            host_bent = bc.bent_rule(fr.packed, fr.k, ao, fr.pos, fr.nrm)[1]
            got_bent = np.zeros((H, W, 4), f32)
            ctx.d2h(got_bent, f.d["bent"])
            bf.same_bits(got_bent, host_bent, ("trace", frame))
            host_prev = api.accumulate_bent(p, n, fr.pos, fr.nrm, host_bent, None if frame == 0 else (fr.pos, fr.nrm) + host_prev)
            bt.same_texels((cur[0].read((H, W), u64), cur[1].read((H, W))), host_prev, ("accumulate", frame))
        assert (host_prev[1] == frames).any() and (host_prev[1] == 0).any(), np.unique(host_prev[1])
        last = ping[(frames - 1) & 1][0]
        out, plane = f.run_filter(fp, n, last.ptr, with_active=False)
        host_out, host_ao = api.wide_filter_bent_mean(fp, n, fr.pos, fr.nrm, host_prev[0])
        bf.same_bits(out, host_out, "filter")
        bf.same_bits(plane, host_ao, "filter ao")
        api.combine_visibility_list_ao_bent_device(ctx, k, lst, f.d["pos"], f.d["nrm"], d_vis, f.ao.ptr, f.out.ptr, sky, W, H, d_rgb.ptr,
                                                   colors=colors)
        ctx.synchronize()
        want = api.combine_visibility_list_ao_bent(k, lst, fr.pos, fr.nrm, vis, host_ao, host_out, sky, colors=colors)
        assert np.array_equal(d_rgb.read((H, W, 3)), want)
    finally:
        f.free()
        for a, b in ping:
            a.free()
            b.free()
        d_rgb.free()
        ctx.free(d_counts)
        ctx.free(d_vis)


def test_refusals_launch_nothing(ctx):
    """The alignment and aliasing refusals of both device forms, and a sample of the shared ones: RTS_ERR_INVALID_ARG and not a byte of
    any output."""
    lib = api._lib
    wh, n = (16, 16), 4
    c = bt.case("pixels", (72, 40), n)
    W, H = wh
    f = _Frame(ctx, W, H)
    h, v = ctx.handle, C.c_void_p
    d = f.d
    good = api.TemporalParams.from_buffer_copy(c["params"])
    half = W * H * 8

    def call(p=good, ns=n, ctx_=h, bent=d["bent"], pp=d["ppos"], pn=d["pnrm"], pt=d["ptex"], pl=d["plen"], w=W, hh=H, to=f.texels.ptr,
             lo=f.lengths.ptr, motion=None):
        head = (ctx_, None if p is None else C.byref(p), ns, v(d["pos"]), v(d["nrm"]), v(d["act"]), v(bent), v(pp), v(pn), v(pt), v(pl))
        if motion is not None:
            return lib.rtsh_accumulate_bent_motion_device(*head, v(motion[0]), v(motion[1]), w, hh, v(to), v(lo), None)
        return lib.rtsh_accumulate_bent_device(*head, w, hh, v(to), v(lo), None)

    def fcall(p, ns=n, ctx_=h, tx=d["ptex"], w=W, hh=H, out=f.out.ptr, ao=f.ao.ptr, scratch=f.scratch.ptr):
        return lib.rtsh_wide_filter_bent_mean_device(ctx_, None if p is None else C.byref(p), ns, v(d["pos"]), v(d["nrm"]), v(d["act"]), v(tx), w,
                                                     hh, v(out), v(ao), v(scratch), None)

    try:
        f.upload(pos=c["pos"][:H, :W], nrm=c["nrm"][:H, :W], ppos=c["pos"][:H, :W], pnrm=c["nrm"][:H, :W], bent=bf.synthetic_bent(wh, n),
                 ptex=bt.history(wh)[0], plen=bt.history(wh)[1], act=bt.active_plane(wh))
        assert call(ctx_=None) == INVALID and call(p=None) == INVALID and call(ns=49) == INVALID
        assert call(bent=0) == INVALID and call(to=0) == INVALID and call(lo=0) == INVALID
        for name in ("pp", "pn", "pt", "pl"):
            assert call(**{name: 0}) == INVALID                              # some but not all of the four prev_*
        assert call(pt=f.texels.ptr) == INVALID and call(pl=f.lengths.ptr) == INVALID   # history must ping-pong
        assert call(bent=d["bent"] + 8) == INVALID                           # whole texels: 16-byte alignment
        assert call(to=f.texels.ptr + 4) == INVALID and call(pt=d["ptex"] + 4) == INVALID   # 8-byte texels
        assert call(w=0) == INVALID and call(hh=0) == INVALID and call(w=1, hh=16 * 65535 + 1) == INVALID
        assert call(p=tc.with_params(good, 0, 0)) == INVALID and call(p=tc.with_params(good, 256, 0)) == INVALID
        assert call(motion=(0, d["pnr"])) == INVALID and call(motion=(d["pts"], 0)) == INVALID
        ok = bf.params(3)
        assert fcall(ok, ctx_=None) == INVALID and fcall(None) == INVALID and fcall(ok, ns=49) == INVALID
        assert fcall(ok, tx=0) == INVALID and fcall(ok, out=0) == INVALID and fcall(bf.params(2), scratch=0) == INVALID
        assert fcall(ok, tx=d["ptex"] + 4) == INVALID                        # 8-byte texels
        assert fcall(ok, out=f.out.ptr + 8) == INVALID and fcall(ok, scratch=f.scratch.ptr + 4) == INVALID
        for alias in (f.scratch.ptr, f.scratch.ptr + half):
            assert fcall(ok, tx=alias) == INVALID                            # texels on the scratch or its second half
            assert fcall(ok, out=alias) == INVALID and fcall(ok, ao=alias) == INVALID
        assert fcall(ok, tx=f.out.ptr) == INVALID and fcall(ok, tx=f.ao.ptr) == INVALID   # texels on out, on ao
        assert fcall(ok, w=0) == INVALID and fcall(ok, w=1, hh=16 * 65535 + 1) == INVALID
        ctx.synchronize()
        for g in (f.texels, f.lengths, f.out, f.ao, f.scratch):
            assert g.untouched()
        assert call() == 0 and call(pp=0, pn=0, pt=0, pl=0, motion=(0, 0)) == 0 and fcall(bf.params(1), scratch=0) == 0
        ctx.synchronize()
    finally:
        f.free()
