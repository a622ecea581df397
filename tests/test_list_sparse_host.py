"""CPU: compacted light maps and the sparse light list twins on the host (include/rts_scene.h: rtsh_compact_light_map; api.py:
soft_light_list_sparse, light_list_sparse).  The compaction twin against the numpy rule of tests/list_sparse_cases.py
word for word over every frame, map and capacity of the cases, guard words around the list; its refusals; the twin under the
sanitizers (tests/cpp/list_sparse_host.cpp); the sparse twins on cornell_128 and terrain_96 against the list traces' twins under the
map; and the two anchors of the half-resolution chain through compact + sparse trace.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import list_sparse_cases as sc
import list_upsample_cases as uc
from raytracedshadows_amd import api
from soft_list_cases import make_list, workload

ROOT = sc.ROOT
INVALID = 1
FILL = sc.FILL
FILL32 = np.uint32(0xABABABAB)
GUARD = 16


@pytest.mark.parametrize("case", sc.compaction_cases(), ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}")
def test_compaction_equals_the_rule(case):
    kind, wh, count = case
    m = sc.light_map(kind, wh, count)
    want = sc.compact_rule(count, m) if wh[0] * wh[1] < 20000 else sc.compact_rule_fast(count, m)
    if wh == (70, 33):
        assert np.array_equal(want, sc.compact_rule_fast(count, m))     # (the two restatements agree where both are affordable)
    n = want.size
    if kind in ("zero", "above_count"):
        assert n == 0
    if kind == "all":
        assert n == wh[0] * wh[1]
    if kind == "last_tile":
        assert n == 1 and want[0] == wh[0] * wh[1] - 1
    if kind == "one_percent" and wh[0] * wh[1] > 2000:
        assert 0 < n < wh[0] * wh[1] // 20
    for capacity in sc.capacities(n):
        raw = np.full(GUARD + capacity + 2 + GUARD, FILL32, np.uint32)    # the list: `capacity` entries, two more, guards around it
        out = raw[GUARD:GUARD + capacity]
        got = C.c_uint32(0xABABABAB)
        status = api._lib.rtsh_compact_light_map(count, api._ptr(m), wh[0], wh[1], api._ptr(out), capacity, C.byref(got))
        assert status == 0 and got.value == n, (case, capacity, got.value, n)
        k = min(n, capacity)
        assert np.array_equal(out[:k], want[:k]), (case, capacity)
        assert (out[k:] == FILL32).all() and (raw[:GUARD] == FILL32).all() and (raw[GUARD + capacity:] == FILL32).all(), (case, capacity)
    pixels, n2 = api.compact_light_map(count, m)
    assert n2 == n and np.array_equal(pixels, want)


@pytest.mark.parametrize("wh", sc.MANY_FRAMES, ids=lambda wh: f"{wh[0]}x{wh[1]}")
def test_the_many_group_maps_hold_what_their_cases_are_for(wh):
    """No library: the arithmetic maps of the many-group frames against the numpy rule."""
    W, H = wh
    tiles, groups = (W // 8) * (H // 8), sc.MANY_GROUPS[wh]
    assert (tiles + sc.SCAN_TILES - 1) // sc.SCAN_TILES == groups
    g = sc.full_group_of(wh)
    for kind in sc.MANY_MAPS:
        m = sc.many_groups_map(kind, wh)
        want = sc.compact_rule_fast(8, m)
        flat = m.reshape(-1)
        assert all(flat[p] != 0 for p in sc.many_groups_pinned(wh)), kind        # first and last pixel, group edges
        totals = sc.group_totals(wh, want)
        assert totals.sum() == want.size and totals[0] > 0 and totals[-1] > 0
        if kind == "sparse":
            assert abs(want.size - W * H / 4096) < W * H / 4096 * 0.01 + 8
            assert (totals > 0).sum() >= groups - 1                                # (data in every lane of the sum)
        else:
            assert totals[g] == 64 * sc.SCAN_TILES
            assert totals[g - 1] <= 3 and totals[g + 1] <= 3
            if groups > 3:
                assert totals[g - 1] == 0 and totals[g + 1] == 0


@pytest.mark.parametrize("kind", sc.MANY_MAPS)
def test_compaction_of_three_groups_equals_the_rule(kind):
    wh = sc.MANY_FRAMES[0]
    m = sc.many_groups_map(kind, wh)
    want = sc.compact_rule_fast(8, m)
    n = want.size
    for capacity in (n - 1, n):
        raw = np.full(capacity + 1 + GUARD, FILL32, np.uint32)                    # the list, then a guard
        got = C.c_uint32(0xABABABAB)
        assert api._lib.rtsh_compact_light_map(8, api._ptr(m), wh[0], wh[1], api._ptr(raw), capacity, C.byref(got)) == 0
        assert got.value == n, (kind, capacity, got.value, n)
        assert np.array_equal(raw[:capacity], want[:capacity]) and (raw[capacity:] == FILL32).all(), (kind, capacity)


def test_compaction_refusals_write_nothing():
    m = sc.light_map("half", (17, 5), 8)
    out = np.full(100, FILL32, np.uint32)
    n = C.c_uint32(0xABABABAB)
    lib, v = api._lib, C.c_void_p

    def call(count=3, M=m, W=17, H=5, O=out, capacity=100, N=n):
        return lib.rtsh_compact_light_map(count, api._ptr(M) if M is not None else None, W, H, api._ptr(O) if O is not None else None, capacity,
                                          C.byref(N) if N is not None else None)

    for kw in (dict(count=0), dict(count=9), dict(M=None), dict(O=None), dict(N=None), dict(W=0), dict(H=0), dict(capacity=0),
               dict(W=1 << 16, H=(1 << 15) + 1), dict(W=0xFFFFFFFF, H=0xFFFFFFFF)):
        assert call(**kw) == INVALID, kw
    assert (out == FILL32).all() and n.value == 0xABABABAB
    assert api.compact_scratch_bytes(0, 5) == 0 and api.compact_scratch_bytes(1 << 16, (1 << 15) + 1) == 0
    assert api.compact_scratch_bytes(8 * sc.SCAN_TILES, 8) == 4 * (sc.SCAN_TILES + 1)
    assert api.compact_scratch_bytes(8 * sc.SCAN_TILES + 1, 8) == 4 * (sc.SCAN_TILES + 1 + 2)
    assert api.COMPACT_NODES == 4
    assert call() == 0 and n.value == sc.compact_rule(3, m).size        # (the call was a good one)


def test_on_small_frames_under_the_sanitizers(tmp_path):
    """tests/cpp/list_sparse_host.cpp: the compaction twin (rts_scene.cpp and the shared per-pixel source, compiled into the program --
    nothing sanitized is loaded into Python) under -fsanitize=address,undefined over the frames of the cases in exact-size heap blocks,
    every capacity, and the refusals."""
    exe = str(tmp_path / "list_sparse_host")
    csrc = os.path.join(ROOT, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "list_sparse_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 100, run.stdout[-2000:]


# ------------------------------------------------------------------------------------------------------------------ the sparse twins
def _twin(scn, form, count, pixels, lights_map, before):
    planes = before.copy()
    if form == "soft":
        return api.soft_light_list_sparse(scn.packed, scn.k, scn.soft[count], scn.pos, scn.W, scn.H, pixels, planes, lights_map=lights_map)
    return api.light_list_sparse(scn.packed, scn.k, scn.hard[count], scn.pos, scn.W, scn.H, pixels, planes, lights_map=lights_map)


@pytest.fixture(scope="module", params=sc.SCENES, ids=lambda s: s[0])
def scn(request):
    return sc.scene(*request.param)


@pytest.mark.parametrize("count", (1, 8))
def test_sparse_twins_equal_the_list_traces_under_the_map(scn, count):
    W, H = scn.W, scn.H
    pixels = scn.marked(count)
    below = (1 << count) - 1
    assert 0 < pixels.size < W * H
    # soft: the marked pairs hold the full trace's byte, everything else the preset
    before = np.full((8, H, W), FILL, np.uint8)
    got = _twin(scn, "soft", count, pixels, scn.map, before)
    full = api.soft_light_list(scn.packed, scn.k, scn.soft[count], scn.pos, W, H, lights_map=scn.map)
    for l in range(8):
        on = ((scn.map >> l) & 1).astype(bool) if l < count else np.zeros((H, W), bool)
        assert (got[l][~on] == FILL).all() and (l >= count or np.array_equal(got[l][on], full[l][on])), l
    assert len(np.unique(full)) > (2 if scn.name == "cornell_128" else 1)      # (the terrain's lights shade next to nothing)
    assert np.array_equal(got[:count], sc.expected(scn, "soft", count, pixels, scn.map, before[:count]))
    # hard: the marked bits are the full trace's, the other bits of a listed pixel's byte and every unlisted byte keep the preset
    before = np.full((H, W), FILL, np.uint8)
    got = _twin(scn, "hard", count, pixels, scn.map, before)
    full = api.light_list(scn.packed, scn.k, scn.hard[count], scn.pos, W, H, lights_map=scn.map)
    on = scn.map & below
    assert np.array_equal(got & on, full & on) and np.array_equal(got & ~on, FILL & ~on)
    assert (on != 0).any() and (on != below).any() and 0 < (full & on).sum()
    assert np.array_equal(got, sc.expected(scn, "hard", count, pixels, scn.map, before))
    # no map: every light below count at every listed pixel
    some = pixels[::3]
    for form, before in (("soft", np.full((count, H, W), FILL, np.uint8)), ("hard", np.full((H, W), FILL, np.uint8))):
        got = _twin(scn, form, count, some, None, before)
        assert np.array_equal(got, sc.expected(scn, form, count, some, None, before)), form
        untouched = np.ones(W * H, bool)
        untouched[some] = False
        flat = got.reshape(-1, W * H)
        assert (flat[:, untouched] == FILL).all()


@pytest.mark.parametrize("form", ("soft", "hard"))
def test_order_duplicates_and_entries_beyond_the_frame(scn, form):
    count, W, H = 8, scn.W, scn.H
    lists = sc.trace_lists(scn, count)
    before = np.full((count, H, W) if form == "soft" else (H, W), FILL, np.uint8)
    base = _twin(scn, form, count, lists["all"][0], scn.map, before)
    assert np.array_equal(_twin(scn, form, count, lists["shuffled"][0], scn.map, before), base)
    assert np.array_equal(_twin(scn, form, count, lists["duplicates"][0], scn.map, before), base)
    beyond = lists["beyond"][0]
    kept = beyond[beyond < W * H]
    assert 0 < kept.size < beyond.size
    got = _twin(scn, form, count, beyond, scn.map, before)
    assert np.array_equal(got, _twin(scn, form, count, kept, scn.map, before))
    assert np.array_equal(got, sc.expected(scn, form, count, kept, scn.map, before))
    # an unlisted pixel's position is never read: NaN there changes nothing
    poisoned = scn.pos.copy()
    listed = np.zeros(W * H, bool)
    listed[kept] = True
    poisoned.reshape(-1, 4)[~listed] = np.nan
    fn = api.soft_light_list_sparse if form == "soft" else api.light_list_sparse
    lst = scn.soft[count] if form == "soft" else scn.hard[count]
    assert np.array_equal(fn(scn.packed, scn.k, lst, poisoned, W, H, kept, before.copy(), lights_map=scn.map), got)


# ------------------------------------------------------------------------------------------------------- the chain through the new path
@pytest.fixture(scope="module")
def cornell():
    return workload(33, 21)


@pytest.mark.parametrize("phase", uc.PHASES, ids=str)
def test_chain_anchors_through_compact_and_sparse(cornell, phase):
    """4.32's anchor 4 through the new path: with plane_eps = -1 and the facing map, subsample -> trace at w x h -> retrace map ->
    compact -> sparse trace -> upsample with keep equals the plain full-resolution trace byte for byte; with the ordinary thresholds the
    same chain equals the existing chain (masked trace in place of compact + sparse) byte for byte.  Soft and hard."""
    wl = cornell
    W, H, k = 33, 21, wl.constants
    w, h = api.subsampled_size(W, H, *phase)
    soft = make_list("mixed")
    hard = soft.hard_list()
    count = soft.count
    facing = api.facing_lights(k, hard, wl.pos, wl.nrm)
    for thresholds in (uc.NONE_ACCEPTED, uc.ORDINARY):
        p = uc.params(phase, thresholds)
        lo_pos, lo_nrm, lo_map = api.subsample_gbuffer(p, wl.pos, wl.nrm, facing)
        keep = api.upsample_retrace_map(count, p, wl.pos, wl.nrm, lo_pos, lo_nrm, facing, lo_map)
        pixels, n = api.compact_light_map(count, keep)
        assert n == pixels.size == int((keep & ((1 << count) - 1) != 0).sum()) and n > 0
        for form in ("soft", "hard"):
            lst, trace, sparse, up = ((soft, api.soft_light_list, api.soft_light_list_sparse, api.upsample_soft_light_list) if form == "soft" else
                                      (hard, api.light_list, api.light_list_sparse, api.upsample_light_list))
            shape = (count, H, W) if form == "soft" else (H, W)
            lo = trace(wl.packed, k, lst, lo_pos, w, h, lights_map=lo_map)
            # (a hard mask starts at 0: where all of a pixel's lights are retraced the upsample leaves the byte alone, and the sparse trace
            #  keeps the bits from `count` up that the masked trace would have cleared)
            planes = sparse(wl.packed, k, lst, wl.pos, W, H, pixels, np.full(shape, FILL if form == "soft" else 0, np.uint8), lights_map=keep)
            got = up(lst, p, wl.pos, wl.nrm, lo_pos, lo_nrm, lo, facing, lo_map, keep, out=planes)
            if thresholds is uc.NONE_ACCEPTED:
                want = trace(wl.packed, k, lst, wl.pos, W, H, lights_map=facing)
                assert len(np.unique(want)) > (3 if form == "soft" else 1)
            else:
                assert n < W * H // 2
                masked = trace(wl.packed, k, lst, wl.pos, W, H, lights_map=keep)
                want = up(lst, p, wl.pos, wl.nrm, lo_pos, lo_nrm, lo, facing, lo_map, keep, out=masked)
            assert np.array_equal(got, want), (form, phase, thresholds)
