"""GPU: the renderer's whole light-list frame on the device, eager and captured, against the chain of host twins -- the three recipes
of tests/list_frame_cases.py (its module text states them, the substitutions and what is not compared).  Every stage of a frame is
issued back to back on a stream created for the test, with ONE synchronisation per frame; the buffers a frame writes before it reads
them are preset to 0xAB before every frame (the host chain presets its own to 0x5A), every buffer has 256 spare bytes that must come
back unchanged, and after each frame EVERY plane of list_frame_cases.PLANES is compared, floats bit for bit."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import list_frame_cases as fc
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu

GUARD = 256
f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def ctx():
    c = api.ShadowContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def stream(ctx):
    s = ctx.stream_create()
    yield s
    ctx.stream_destroy(s)


class _Guarded:
    """A device buffer of nbytes + 256 bytes, all of it preset to 0xAB."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = ctx.malloc(nbytes + GUARD)
        self.reset()

    def reset(self):
        self.ctx.h2d(self.ptr, np.full(self.nbytes + GUARD, fc.PRESET_DEVICE, np.uint8))

    def read(self):
        raw = np.zeros(self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.ptr)
        assert (raw[self.nbytes:] == fc.PRESET_DEVICE).all(), "bytes behind the buffer were written"
        return raw[:self.nbytes]

    def untouched(self):
        raw = np.zeros(self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.ptr)
        return bool((raw == fc.PRESET_DEVICE).all())

    def free(self):
        self.ctx.free(self.ptr)


class Env:
    """The device side of a recipe: every buffer of the frame loop, guarded; count planes, moments and visibility of eight planes, the
    low-resolution buffers of the largest phase."""

    def __init__(self, ctx, stream, R):
        n, lo = fc.N, fc.LO
        self.ctx, self.stream, self.snapshot_stream, self.R = ctx, stream, None, R
        sizes = {"snap": fc.geometry()["nvec4"] * 16, "pts": n * 16, "pnr": n * 16, "map": n, "vis": 8 * n * 4, "rgb": n * 3,
                 "scratch": fc.scratch_bytes(R)}
        for parity in "01":
            sizes.update({"pos" + parity: n * 16, "nrm" + parity: n * 16})
            if R.name == "C":
                sizes.update({"hvis" + parity: 8 * n * 4, "hlen" + parity: 8 * n})
            else:
                sizes.update({"mean" + parity: 8 * n * 2, "square" + parity: 8 * n * 4, "mlen" + parity: 8 * n})
        if R.name == "C":
            sizes["mask"] = n
        else:
            sizes.update({"counts": 8 * n, "lpos": lo * 16, "lnrm": lo * 16, "lmap": lo, "lo": R.count * lo, "keep": n})
        self.buffers = {name: _Guarded(ctx, nbytes) for name, nbytes in sizes.items()}
        self.p = {name: b.ptr for name, b in self.buffers.items()}

    def preset(self):
        for name in fc.PRESETS[self.R.name] + ["scratch"]:
            self.buffers[name].reset()

    def presets_untouched(self):
        return all(self.buffers[name].untouched() for name in fc.PRESETS[self.R.name] + ["scratch"])

    def read(self, f):
        """name -> payload bytes of every compared plane (this frame's of a ping-ponged one); every guard is checked."""
        got = {}
        for name, b in self.buffers.items():
            raw = b.read()
            if name[-1] in "01":
                if name[-1] == f.c:
                    got[name[:-1]] = raw
            else:
                got[name] = raw
        return got

    def free(self):
        for b in self.buffers.values():
            b.free()


def install(ctx):
    ctx.set_bvh(fc.geometry()["packed"])


def eager_chain(ctx, stream, e, R, want, fixed=False, frames=fc.FRAMES, what="eager"):
    """`frames` frames through the device wrappers, each compared with the host chain; returns the payloads read after every frame."""
    out = []
    for k in range(frames):
        f = fc.Frame(R, k, fixed)
        e.preset()
        fc.run_device_frame(R, e, f)
        ctx.synchronize(stream)
        got = e.read(f)
        fc.compare_frame(R, got, want[k], (R.name, what, "frame", k))
        out.append(got)
    return out


@pytest.mark.parametrize("name", sorted(fc.RECIPES))
def test_eager_chain_equals_the_host_chain(ctx, stream, name):
    R = fc.RECIPES[name]
    install(ctx)
    e = Env(ctx, stream, R)
    try:
        eager_chain(ctx, stream, e, R, fc.host_chain(name))
    finally:
        e.free()


def test_frame_reuse_a_second_sequence_equals_the_first(ctx, stream):
    """Recipe B twice on the same buffers, nothing freed or cleared but the presets: no history and no per-stream state leaks from one
    sequence into the next (frame 0 passes d_prev = None, as the renderer does)."""
    R = fc.RECIPES["B"]
    install(ctx)
    e = Env(ctx, stream, R)
    try:
        want = fc.host_chain("B")
        first = eager_chain(ctx, stream, e, R, want, what="first run")
        second = eager_chain(ctx, stream, e, R, want, what="second run")
        for k, (a, b) in enumerate(zip(first, second)):
            for plane in fc.PLANES["B"]:
                assert (a[plane] == b[plane]).all(), ("frame", k, plane, "the second run differs from the first")
    finally:
        e.free()


def test_one_graph_per_parity_replayed_over_moving_geometry(ctx, stream):
    """Recipe A, camera, phase and jitter rotation fixed: frame 0 eagerly (per-stream state is never created inside a capture), then
    the odd and the even frame captured as two graphs and replayed alternately for four more frames, the refit between the replays."""
    R = fc.RECIPES["A"]
    frames = fc.FRAMES + 1
    want = fc.host_chain("A", fixed=True, frames=frames)
    install(ctx)
    e = Env(ctx, stream, R)
    graphs, alone = {}, []
    try:
        eager = eager_chain(ctx, stream, e, R, want, fixed=True, frames=frames, what="eager, fixed")
        # the captured chain starts over: frame 0 eagerly, on the stream, every stage of it
        e.snapshot_stream = stream
        f0 = fc.Frame(R, 0, fixed=True)
        e.preset()
        ctx.synchronize()
        fc.run_device_frame(R, e, f0, ["snapshot"])
        ctx.synchronize(stream)                                           # (the refit runs on the default stream)
        fc.run_device_frame(R, e, f0, R.stages[1:])
        ctx.synchronize(stream)
        fc.compare_frame(R, e.read(f0), want[0], "frame 0 before the captures")
        stages = fc.captured_stages(R)
        recorded = {parity: fc.Frame(R, 2 - parity, fixed=True) for parity in (0, 1)}       # frames 2 and 1: both read a history
        e.preset()
        for parity in (0, 1):
            graphs[parity] = hipgraph.capture(stream, lambda: fc.run_device_frame(R, e, recorded[parity], stages))
        per_stage = 0
        for s in stages:
            alone.append(hipgraph.capture(stream, lambda: fc.run_device_frame(R, e, recorded[1], [s])))
            per_stage += len(alone[-1].node_types())
        ctx.synchronize(stream)
        assert e.presets_untouched(), "a capture itself ran"
        fc.compare_frame(R, e.read(f0) | {k: eager[0][k] for k in fc.PRESETS["A"]}, want[0], "frame 0 after the captures")
        for parity in (0, 1):
            types = graphs[parity].node_types()
            assert sorted(set(types)) == [hipgraph.KERNEL, hipgraph.MEMCPY] and types.count(hipgraph.MEMCPY) == 1, types
            assert len(types) == per_stage, (len(types), per_stage, "the frame's graph is not the sum of its stages' nodes")
        for f in recorded.values():                                       # a replay uses the values as they were at the capture
            for s in f.structs():
                C.memset(C.addressof(s), 0xFF, C.sizeof(s))
            f.colors[:] = np.nan
        g = fc.geometry()
        for k in range(1, frames):
            f = fc.Frame(R, k, fixed=True)
            e.preset()
            api.bvh_refit_device(ctx, f.verts, 3, g["idx"], g["P"])     # the next vertex stream, outside the graph
            graphs[k % 2].launch(stream)
            ctx.synchronize(stream)
            got = e.read(f)
            fc.compare_frame(R, got | {"snap": eager[k]["snap"]}, want[k], ("replay", k))
            for plane in fc.PLANES["A"]:
                if plane != "snap":
                    assert (got[plane] == eager[k][plane]).all(), ("replay", k, plane, "differs from the eager run")
            refit = api.bvh_refit(g["packed"], f.verts, 3, g["idx"], g["P"])
            assert (got["snap"].view(u32).reshape(-1, 4) == refit).all(), ("replay", k, "the snapshot at the end of the frame")
    finally:
        for gr in list(graphs.values()) + alone:
            gr.close()
        e.snapshot_stream = None
        e.free()
