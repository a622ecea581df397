"""GPU: compacted light maps and sparse light list traces (rtsh_compact_light_map_device, raytracedshadows_amd/csrc/rts_compact.inc;
rts_trace_light_list_sparse_device, rts_trace_soft_light_list_sparse_device, rts_light_list_sparse.inc) on the cases of
tests/list_sparse_cases.py.  Compaction: the device form equals the host twin word for word on every CPU case and capacity, both
sizes around one scan workgroup's reach included, every buffer inside a larger allocation preset to 0xAB; api.COMPACT_NODES kernel
nodes under capture and no other node; a replay compacts the map the buffer holds then.  Sparse traces: the device form equals the
host twin byte for byte over planes preset to 0xAB -- list lengths on either side of a wave and of a block, *d_n above the capacity, no
map, a wave in which one lane carries a light, NaN at unlisted pixels, shuffled lists, duplicates, entries beyond the frame --; no
option changes a byte; one counter, one kernel node; a replay traces the list the buffers hold then; the refusals write nothing.  The
half-resolution chain through compact + sparse on a non-default stream, both anchors."""
import ctypes as C

import numpy as np
import pytest

import hipgraph
import list_combine_cases as lc
import list_sparse_cases as sc
import list_upsample_cases as uc
from raytracedshadows_amd import api
from soft_list_cases import make_list, workload

pytestmark = pytest.mark.gpu

GUARD = 256
INVALID, NO_BVH = 1, 4
FILL = sc.FILL
FILL32 = np.uint32(0xABABABAB)


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
    """A device buffer of shift + nbytes + 256 bytes preset to 0xAB; the payload starts `shift` bytes in."""

    def __init__(self, ctx, nbytes, shift, fill=None):
        self.ctx, self.nbytes, self.shift = ctx, nbytes, shift
        self.base = ctx.malloc(shift + nbytes + GUARD)
        self.ptr = self.base + shift
        self.reset(fill)

    def reset(self, fill=None):
        raw = np.full(self.shift + self.nbytes + GUARD, FILL, np.uint8)
        if fill is not None:
            b = np.ascontiguousarray(fill).view(np.uint8).reshape(-1)
            raw[self.shift:self.shift + b.size] = b
        self.ctx.h2d(self.base, raw)

    def read(self, shape, dtype=np.uint8):
        raw = np.zeros(self.shift + self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.base)
        assert (raw[:self.shift] == FILL).all() and (raw[self.shift + self.nbytes:] == FILL).all(), "bytes around the buffer were written"
        return raw[self.shift:self.shift + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        raw = np.zeros(self.shift + self.nbytes + GUARD, np.uint8)
        self.ctx.d2h(raw, self.base)
        return bool((raw == FILL).all())

    def free(self):
        self.ctx.free(self.base)


# ---------------------------------------------------------------------------------------------------------------------- compaction
@pytest.mark.parametrize("wh", sc.FRAMES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_compaction_equals_the_host_twin(ctx, other_stream, wh):
    W, H = wh
    cases = [c for c in sc.compaction_cases() if c[1] == wh]
    scratch_bytes = api.compact_scratch_bytes(W, H)
    d_map = _Guarded(ctx, W * H, 1)
    d_list = _Guarded(ctx, 4 * (W * H + 1), 4)
    d_n = _Guarded(ctx, 4, 4)
    d_scratch = _Guarded(ctx, scratch_bytes, 4)
    try:
        for i, (kind, _, count) in enumerate(cases):
            m = sc.light_map(kind, wh, count)
            want, n = api.compact_light_map(count, m)
            d_map.reset(m)
            for capacity in sc.capacities(n):
                stream = other_stream if (i + capacity) % 2 else None
                d_list.reset()
                d_n.reset()
                api.compact_light_map_device(ctx, count, d_map.ptr, W, H, d_list.ptr, capacity, d_n.ptr, d_scratch.ptr, stream=stream)
                ctx.synchronize(stream)
                what = (kind, wh, count, capacity)
                assert int(d_n.read((1,), np.uint32)[0]) == n, what
                got = d_list.read((W * H + 1,), np.uint32)
                k = min(n, capacity)
                assert np.array_equal(got[:k], want[:k]), what
                assert (got[k:] == FILL32).all(), what
                d_scratch.read((scratch_bytes,))                          # (its guards)
    finally:
        for b in (d_map, d_list, d_n, d_scratch):
            b.free()


@pytest.mark.parametrize("kind", sc.MANY_MAPS)
@pytest.mark.parametrize("wh", sc.MANY_FRAMES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_compaction_over_many_groups_equals_the_rule(ctx, wh, kind):
    """3, 257 and 1027 groups of tiles: the kernel that sums the groups' totals with data in more than one total of a lane, in more than
    one wave of its block scan, and in a second strip (the carry).  Against the numpy rule; capacities n and n - 1, a guard behind the
    list."""
    W, H = wh
    m = sc.many_groups_map(kind, wh)
    want = sc.compact_rule_fast(8, m)
    n = want.size
    scratch_bytes = api.compact_scratch_bytes(W, H)
    assert scratch_bytes >= 4 * ((W // 8) * (H // 8) + sc.MANY_GROUPS[wh])
    d_map = _Guarded(ctx, W * H, 1, m)
    d_list = _Guarded(ctx, 4 * n, 4)
    d_n = _Guarded(ctx, 4, 4)
    d_scratch = _Guarded(ctx, scratch_bytes, 4)
    try:
        for capacity in (n, n - 1):
            d_list.reset()
            d_n.reset()
            api.compact_light_map_device(ctx, 8, d_map.ptr, W, H, d_list.ptr, capacity, d_n.ptr, d_scratch.ptr)
            ctx.synchronize()
            what = (kind, wh, capacity)
            got_n = int(d_n.read((1,), np.uint32)[0])
            assert got_n == n, (what, got_n, n)
            got = d_list.read((n,), np.uint32)                            # (read() checks the guard words behind the list)
            bad = np.flatnonzero(got[:capacity] != want[:capacity])
            assert bad.size == 0, (what, bad.size, bad[:4].tolist(), sc.group_totals(wh, want)[:8].tolist())
            assert (got[capacity:] == FILL32).all(), what
            d_scratch.read((scratch_bytes,))                              # (its guards)
        d_map.read((W * H,))                                              # (the map's guards: nothing wrote around it)
    finally:
        for b in (d_map, d_list, d_n, d_scratch):
            b.free()


def test_compaction_under_capture(ctx, other_stream):
    """COMPACT_NODES kernel nodes and no other node; nothing runs during the capture; a replay after the map was changed on the device
    gives the new map's list."""
    wh, count = (70, 33), 8
    W, H = wh
    first, second = sc.light_map("half", wh, 8), sc.light_map("one_percent", wh, 8)
    d_map = _Guarded(ctx, W * H, 1, first)
    d_list = _Guarded(ctx, 4 * W * H, 4)
    d_n = _Guarded(ctx, 4, 4)
    d_scratch = _Guarded(ctx, api.compact_scratch_bytes(W, H), 4)
    s = other_stream
    try:
        g = hipgraph.capture(s, lambda: api.compact_light_map_device(ctx, count, d_map.ptr, W, H, d_list.ptr, W * H, d_n.ptr, d_scratch.ptr, stream=s))
        try:
            assert g.node_types() == [hipgraph.KERNEL] * api.COMPACT_NODES, g.node_types()
            assert d_list.untouched() and d_n.untouched(), "the capture itself ran a kernel"
            for m in (first, second, first):
                d_map.reset(m)
                d_list.reset()
                g.launch(s)
                ctx.synchronize(s)
                want, n = api.compact_light_map(count, m)
                assert int(d_n.read((1,), np.uint32)[0]) == n
                got = d_list.read((W * H,), np.uint32)
                assert np.array_equal(got[:n], want) and (got[n:] == FILL32).all()
        finally:
            g.close()
    finally:
        for b in (d_map, d_list, d_n, d_scratch):
            b.free()


def test_compaction_refusals_write_nothing(ctx):
    W, H = 17, 5
    d_map = _Guarded(ctx, W * H, 1, sc.light_map("half", (W, H), 8))
    d_list = _Guarded(ctx, 4 * W * H, 4)
    d_n = _Guarded(ctx, 4, 4)
    d_scratch = _Guarded(ctx, api.compact_scratch_bytes(W, H), 4)
    lib, v = api._lib, C.c_void_p

    def call(c=ctx.handle, count=3, M=d_map.ptr, W_=W, H_=H, O=d_list.ptr, capacity=W * H, N=d_n.ptr, S=d_scratch.ptr):
        return lib.rtsh_compact_light_map_device(c, count, v(M), W_, H_, v(O), capacity, v(N), v(S), None)

    try:
        for kw in (dict(c=None), dict(count=0), dict(count=9), dict(M=0), dict(O=0), dict(N=0), dict(S=0), dict(W_=0), dict(H_=0),
                   dict(capacity=0), dict(W_=1 << 16, H_=(1 << 15) + 1)):
            assert call(**kw) == INVALID, kw
        ctx.synchronize()
        assert d_list.untouched() and d_n.untouched() and d_scratch.untouched()
        assert call() == 0
        ctx.synchronize()
        assert int(d_n.read((1,), np.uint32)[0]) == sc.compact_rule(3, sc.light_map("half", (W, H), 8)).size
    finally:
        for b in (d_map, d_list, d_n, d_scratch):
            b.free()


# ------------------------------------------------------------------------------------------------------------------- sparse traces
class _Scene:
    """A scene of the cases on the device: positions one float, map and planes one byte, the list and its length one word into their
    blocks."""

    def __init__(self, ctx, scn):
        self.ctx, self.scn = ctx, scn
        n = scn.W * scn.H
        self.cap = 2 * n
        self.pos = _Guarded(ctx, 16 * n, 4, scn.pos)
        self.map = _Guarded(ctx, n, 1, scn.map)
        self.planes = _Guarded(ctx, 8 * n, 1)
        self.list = _Guarded(ctx, 4 * self.cap, 4)
        self.n = _Guarded(ctx, 4, 4)

    def set_list(self, pixels, n):
        self.list.reset(np.ascontiguousarray(pixels, np.uint32))
        self.n.reset(np.array([n], np.uint32))

    def trace(self, form, count, capacity, with_map=True, stream=None):
        s = self.scn
        fn = self.ctx.trace_soft_light_list_sparse_device if form == "soft" else self.ctx.trace_light_list_sparse_device
        fn(s.k, s.soft[count] if form == "soft" else s.hard[count], self.pos.ptr, s.W, s.H, self.list.ptr, self.n.ptr, capacity,
           self.planes.ptr, d_lights_map=self.map.ptr if with_map else None, stream=stream)

    def free(self):
        for b in (self.pos, self.map, self.planes, self.list, self.n):
            b.free()


@pytest.fixture(scope="module", params=sc.SCENES, ids=lambda s: s[0])
def dev(ctx, request):
    scn = sc.scene(*request.param)
    ctx.set_bvh(scn.packed)
    d = _Scene(ctx, scn)
    yield d
    d.free()


def _want(scn, form, count, pixels, lights_map):
    before = np.full((count, scn.H, scn.W) if form == "soft" else (scn.H, scn.W), FILL, np.uint8)
    fn = api.soft_light_list_sparse if form == "soft" else api.light_list_sparse
    return fn(scn.packed, scn.k, scn.soft[count] if form == "soft" else scn.hard[count], scn.pos, scn.W, scn.H, pixels, before,
              lights_map=lights_map)


def _check_planes(dev, form, count, want, what):
    scn = dev.scn
    got = dev.planes.read((8, scn.H, scn.W))
    used = count if form == "soft" else 1
    assert np.array_equal(got[:used].reshape(want.shape), want), what
    assert (got[used:] == FILL).all(), what


@pytest.mark.parametrize("count", (1, 8))
@pytest.mark.parametrize("form", ("soft", "hard"))
def test_sparse_trace_equals_the_host_twin(ctx, dev, other_stream, form, count):
    scn = dev.scn
    for i, (name, (pixels, n, capacity)) in enumerate(sc.trace_lists(scn, count).items()):
        traced = pixels[:min(n, capacity)]
        stream = other_stream if i % 2 else None
        dev.planes.reset()
        dev.set_list(pixels, n)
        dev.trace(form, count, capacity, stream=stream)
        ctx.synchronize(stream)
        _check_planes(dev, form, count, _want(scn, form, count, traced, scn.map), (form, count, name))
    assert ctx.last_kernel_name() == ("shadowSoftLightListSparseKernel" if form == "soft" else "shadowLightListSparseKernel")


@pytest.mark.parametrize("form", ("soft", "hard"))
def test_no_map_and_nan_at_unlisted_pixels(ctx, dev, form):
    scn, count = dev.scn, 8
    pixels = scn.marked(count)[::2]
    listed = np.zeros(scn.W * scn.H, bool)
    listed[pixels] = True
    poisoned = scn.pos.copy()
    poisoned.reshape(-1, 4)[~listed] = np.nan
    try:
        dev.pos.reset(poisoned)
        dev.set_list(pixels, pixels.size)
        for with_map in (False, True):
            dev.planes.reset()
            dev.trace(form, count, pixels.size, with_map=with_map)
            ctx.synchronize()
            _check_planes(dev, form, count, _want(scn, form, count, pixels, scn.map if with_map else None), (form, with_map))
    finally:
        dev.pos.reset(scn.pos)


@pytest.mark.parametrize("form", ("soft", "hard"))
def test_no_option_changes_a_byte_and_one_counter_moves(ctx, dev, form):
    scn, count = dev.scn, 8
    pixels = scn.marked(count)
    want = _want(scn, form, count, pixels, scn.map)
    dev.set_list(pixels, pixels.size)
    counters = ["launches", "light_list_traces", "soft_light_list_traces", "active_traces", "distance_traces", "soft_distance_traces",
                "adaptive_traces", "soft_list_adaptive_traces", "soft_list_jitter_traces", "soft_list_distance_traces"]
    counters = [c for c in counters if _has_option(ctx, c)]
    try:
        for kernel in range(-1, ctx.get_option("kernel_count")):
            for split in (0, 1):
                ctx.set_option("kernel", kernel)
                ctx.set_option("soft_split", split)
                before = {c: ctx.get_option(c) for c in counters}
                sparse = ctx.get_option("sparse_list_traces")
                dev.planes.reset()
                dev.trace(form, count, pixels.size)
                ctx.synchronize()
                _check_planes(dev, form, count, want, (form, kernel, split))
                assert ctx.get_option("sparse_list_traces") == sparse + 1
                moved = [c for c in counters if c != "launches" and ctx.get_option(c) != before[c]]
                assert moved == [], moved
    finally:
        ctx.set_option("kernel", -1)
        ctx.set_option("soft_split", 1)


def _has_option(ctx, key):
    try:
        ctx.get_option(key)
        return True
    except api.RtsError:
        return False


@pytest.mark.parametrize("form", ("soft", "hard"))
def test_capture_is_one_kernel_node_and_a_replay_reads_the_list_anew(ctx, dev, other_stream, form):
    scn, count, s = dev.scn, 8, other_stream
    base = scn.marked(count)
    first, second = base[:200], base[150:471][::-1].copy()
    dev.set_list(first, first.size)
    dev.planes.reset()
    g = hipgraph.capture(s, lambda: dev.trace(form, count, dev.cap, stream=s))
    try:
        assert g.node_types() == [hipgraph.KERNEL], g.node_types()
        assert dev.planes.untouched(), "the capture itself ran the kernel"
        for pixels in (first, second):
            dev.set_list(pixels, pixels.size)                             # list and length rewritten on the device
            dev.planes.reset()
            g.launch(s)
            ctx.synchronize(s)
            _check_planes(dev, form, count, _want(scn, form, count, pixels, scn.map), (form, pixels.size))
    finally:
        g.close()


def test_refusals_write_nothing(ctx, dev):
    scn = dev.scn
    lib, h, v = api._lib, ctx.handle, C.c_void_p
    W, H = scn.W, scn.H
    pixels = scn.marked(8)
    dev.set_list(pixels, pixels.size)
    dev.planes.reset()
    hard_bad, soft_bad = lc.bad_lists()
    ref = lambda s: C.byref(s) if s is not None else None

    def call(form, lst, c=h, k=scn.k, P=dev.pos.ptr, W_=W, H_=H, L=dev.list.ptr, N=dev.n.ptr, capacity=pixels.size, O=dev.planes.ptr):
        fn = lib.rts_trace_soft_light_list_sparse_device if form == "soft" else lib.rts_trace_light_list_sparse_device
        return fn(c, ref(k), ref(lst), v(P), v(dev.map.ptr), W_, H_, v(L), v(N), capacity, v(O), None)

    sparse, launches = ctx.get_option("sparse_list_traces"), ctx.get_option("launches") if _has_option(ctx, "launches") else 0
    for form, good, bad in (("soft", scn.soft[8], soft_bad), ("hard", scn.hard[8], hard_bad)):
        for b in bad:
            assert call(form, b) == INVALID, form
        for kw in (dict(c=None), dict(k=None), dict(P=0), dict(W_=0), dict(H_=0), dict(L=0), dict(N=0), dict(capacity=0), dict(O=0),
                   dict(W_=1 << 16, H_=(1 << 15) + 1)):
            assert call(form, good, **kw) == INVALID, (form, kw)
    with api.ShadowContext(0) as bare:                                    # no BVH: behind the argument checks
        assert call("soft", scn.soft[8], c=bare.handle) == NO_BVH and call("hard", scn.hard[8], c=bare.handle) == NO_BVH
        assert call("soft", scn.soft[8], c=bare.handle, capacity=0) == INVALID
        assert bare.get_option("sparse_list_traces") == 0
        # host forms: the same refusals
        planes = np.full((8, H, W), FILL, np.uint8)
        for kw in (dict(pixels=None), dict(planes=None), dict(W_=0)):
            st = lib.rts_trace_soft_light_list_sparse(bare.handle, C.byref(scn.k), C.byref(scn.soft[8]), api._ptr(scn.pos), None, kw.get("W_", W), H,
                                                      api._ptr(pixels) if "pixels" not in kw else None, pixels.size,
                                                      api._ptr(planes) if "planes" not in kw else None)
            assert st == INVALID, kw
        assert lib.rts_trace_light_list_sparse(bare.handle, C.byref(scn.k), C.byref(scn.hard[8]), api._ptr(scn.pos), None, W, H, api._ptr(pixels),
                                               pixels.size, api._ptr(planes)) == NO_BVH
        assert (planes == FILL).all()
    ctx.synchronize()
    assert dev.planes.untouched()
    assert ctx.get_option("sparse_list_traces") == sparse
    if _has_option(ctx, "launches"):
        assert ctx.get_option("launches") == launches


@pytest.mark.parametrize("form", ("soft", "hard"))
def test_host_forms_equal_the_host_twin(ctx, dev, form):
    scn, count = dev.scn, 8
    pixels = sc.trace_lists(scn, count)["beyond"][0]
    before = np.full((count, scn.H, scn.W) if form == "soft" else (scn.H, scn.W), FILL, np.uint8)
    fn = ctx.trace_soft_light_list_sparse if form == "soft" else ctx.trace_light_list_sparse
    lst = scn.soft[count] if form == "soft" else scn.hard[count]
    got = fn(scn.k, lst, scn.pos, scn.W, scn.H, pixels, before.copy(), lights_map=scn.map)
    assert np.array_equal(got, _want(scn, form, count, pixels, scn.map))
    assert np.array_equal(fn(scn.k, lst, scn.pos, scn.W, scn.H, np.zeros(0, np.uint32), before.copy(), lights_map=scn.map), before)


# ------------------------------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("phase", uc.PHASES, ids=str)
def test_chain_on_a_stream_through_compact_and_sparse(ctx, other_stream, phase):
    """Both CPU anchors with device forms throughout on a non-default stream, no synchronisation inside the chain: G-buffer on the
    device -> facing map -> subsample -> trace at w x h -> retrace map -> compact -> sparse trace -> upsample with keep.  With
    plane_eps = -1 it equals the plain device trace; with the ordinary thresholds the existing chain (masked trace), byte for byte."""
    W, H = 61, 37
    wl = workload(W, H)
    ctx.set_bvh(wl.packed)
    s = other_stream
    w, h = api.subsampled_size(W, H, *phase)
    n, m, k = W * H, w * h, wl.constants
    soft = make_list("mixed")
    hard = soft.hard_list()
    count = soft.count
    sizes = dict(pos=16 * n, nrm=16 * n, map=n, lo_pos=16 * m, lo_nrm=16 * m, lo_map=m, lo=count * m, keep=n, out=count * n, want=count * n,
                 list=4 * n, n=4, scratch=api.compact_scratch_bytes(W, H), zero=count * n)
    d = {name: ctx.malloc(size) for name, size in sizes.items()}
    try:
        ctx.h2d(d["pos"], wl.pos)
        ctx.h2d(d["nrm"], wl.nrm)
        ctx.synchronize()

        def read(name, shape):
            a = np.zeros(shape, np.uint8)
            ctx.d2h(a, d[name])
            return a

        for thresholds in (uc.NONE_ACCEPTED, uc.ORDINARY):
            p = uc.params(phase, thresholds)
            for form in ("soft", "hard"):
                lst, planes = (soft, count) if form == "soft" else (hard, 1)
                trace = ctx.trace_soft_light_list_device if form == "soft" else ctx.trace_light_list_device
                sparse = ctx.trace_soft_light_list_sparse_device if form == "soft" else ctx.trace_light_list_sparse_device
                upsample = api.upsample_soft_light_list_device if form == "soft" else api.upsample_light_list_device
                ctx.h2d(d["out"], np.full(count * n, FILL if form == "soft" else 0, np.uint8))      # (a hard mask starts at 0: test_list_sparse_host.py)
                ctx.synchronize()
                # the new chain, on the stream, nothing read back in between
                api.facing_lights_device(ctx, k, hard, d["pos"], d["nrm"], W, H, d["map"], stream=s)
                api.subsample_gbuffer_device(ctx, p, d["pos"], d["nrm"], W, H, d["lo_pos"], d["lo_nrm"], d_lights_map=d["map"], d_lo_lights_map=d["lo_map"],
                                             stream=s)
                trace(k, lst, d["lo_pos"], w, h, d["lo"], d_lights_map=d["lo_map"], stream=s)
                api.upsample_retrace_map_device(ctx, count, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], W, H, d["keep"], d_lights_map=d["map"],
                                                d_lo_lights_map=d["lo_map"], stream=s)
                api.compact_light_map_device(ctx, count, d["keep"], W, H, d["list"], n, d["n"], d["scratch"], stream=s)
                sparse(k, lst, d["pos"], W, H, d["list"], d["n"], n, d["out"], d_lights_map=d["keep"], stream=s)
                upsample(ctx, lst, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], d["lo"], W, H, d["out"], d_lights_map=d["map"],
                         d_lo_lights_map=d["lo_map"], d_keep=d["keep"], stream=s)
                # what it must equal
                if thresholds is uc.NONE_ACCEPTED:
                    trace(k, lst, d["pos"], W, H, d["want"], d_lights_map=d["map"], stream=s)
                else:
                    trace(k, lst, d["pos"], W, H, d["want"], d_lights_map=d["keep"], stream=s)
                    upsample(ctx, lst, p, d["pos"], d["nrm"], d["lo_pos"], d["lo_nrm"], d["lo"], W, H, d["want"], d_lights_map=d["map"],
                             d_lo_lights_map=d["lo_map"], d_keep=d["keep"], stream=s)
                ctx.synchronize(s)
                got, want = read("out", (planes, H, W)), read("want", (planes, H, W))
                assert np.array_equal(got, want), (form, phase, thresholds)
                assert len(np.unique(want)) > (3 if form == "soft" else 1)
                listed = np.zeros(1, np.uint32)
                ctx.d2h(listed, d["n"])
                keep = read("keep", (H, W))
                assert int(listed[0]) == int(((keep & ((1 << count) - 1)) != 0).sum()) > 0
                if thresholds is uc.ORDINARY:
                    assert int(listed[0]) < n // 2
    finally:
        for ptr in d.values():
            ctx.free(ptr)
