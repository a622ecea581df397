"""CPU: the host twins of the filter of a light list's planes (rtsh_filter_light_list, rtsh_filter_soft_light_list) and of the
visibility combine (rtsh_combine_visibility_list) against the numpy rules of tests/list_filter_cases.py, bit for bit -- and what pins
the rules: both anchors, the planes that are never touched, every refusal, and the combine anchor over an R = 0 filter."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import list_combine_cases as lc
import list_filter_cases as fc
import scene_pass_cases as sp
from raytracedshadows_amd import api

f32 = np.float32
INVALID = 1


def _twin(form, lst, p, pos, nrm, planes, mask, lights_map, dist, threads=0):
    if form == "hard":
        return api.filter_light_list(lst, p, pos, nrm, mask, lights_map, threads)
    return api.filter_soft_light_list(lst, p, pos, nrm, planes, lights_map, dist, threads)


@pytest.mark.parametrize("radius", fc.RADII)
@pytest.mark.parametrize("wh", fc.FRAMES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_twins_equal_the_numpy_rule(wh, radius):
    """Awkward and geometric frames, hard and soft lists of 1, 2, 3 and 8 lights, with and without map and distances."""
    for kind in ("awkward", "geometric"):
        nrm, pos, planes, mask, lights_map, dist = fc.frame(kind, wh)
        p = fc.params(radius, kind)
        for form, name, with_map, with_dist in fc.runs(radius):
            lst = fc.the_list(form, name)
            m, d = (lights_map if with_map else None), (dist if with_dist else None)
            want = fc.filter_rule(lst, p, pos, nrm, mask if form == "hard" else planes, m, d)
            fc.same_bits(_twin(form, lst, p, pos, nrm, planes, mask, m, d), want, (kind, wh, radius, form, name, with_map, with_dist))


def test_the_geometric_frame_makes_every_test_accept_and_reject():
    """(asserted inside list_filter_cases.geometric for the 33 x 18 frame) -- and the filter changes that frame: it is no identity."""
    nrm, pos, planes, mask, lights_map, dist = fc.geometric((33, 18))
    lst = fc.the_list("soft", "8")
    plain = api.filter_soft_light_list(lst, fc.params(0), pos, nrm, planes, lights_map, None)
    wide = api.filter_soft_light_list(lst, fc.params(2), pos, nrm, planes, lights_map, None)
    guided = api.filter_soft_light_list(lst, fc.params(2), pos, nrm, planes, lights_map, dist)
    assert (plain != wide).any() and (wide != guided).any()
    assert ((wide > 0) & (wide < 1)).any()


def test_threads_change_nothing():
    nrm, pos, planes, mask, lights_map, dist = fc.geometric((33, 18))
    lst = fc.the_list("soft", "8")
    one = _twin("soft", lst, fc.params(2), pos, nrm, planes, mask, lights_map, dist, threads=1)
    fc.same_bits(_twin("soft", lst, fc.params(2), pos, nrm, planes, mask, lights_map, dist, threads=7), one, "7 threads")


@pytest.mark.parametrize("kind", ["awkward", "geometric"])
def test_anchor_no_neighbour_gives_the_combine_quotient(kind):
    """R = 0 -- or thresholds no neighbour passes (a negative plane distance: fabsf(h) <= it never holds) -- gives (float)c / (float)n_l
    where the pixel is active and +0 elsewhere: the quotient of the list combine pass."""
    for wh in ((17, 15), (3, 333)):
        nrm, pos, planes, mask, lights_map, dist = fc.frame(kind, wh)
        background = (nrm[..., :3] == 0).all(axis=-1)
        for form in ("hard", "soft"):
            lst = fc.the_list(form, "8")
            for with_map in (False, True):
                want = np.zeros((8,) + background.shape, f32)
                for l in range(8):
                    on = ~background & ((((lights_map >> l) & 1) != 0) if with_map else True)
                    byte = ((mask >> l) & 1) if form == "hard" else planes[l]
                    samples = f32(1 if form == "hard" else max(1, lst.lights[l].nsamples))
                    want[l] = np.where(on, byte.astype(f32) / samples, f32(0))
                m = lights_map if with_map else None
                closed = [api.FilterParams.make(0, 0.9, 0.02), api.FilterParams.make(8, 3e38, -1.0), api.FilterParams.make(2, -1e30, -1e-30)]
                for p in closed:
                    got = _twin(form, lst, p, pos, nrm, planes, mask, m, dist if form == "soft" else None)
                    fc.same_bits(got, want, (kind, wh, form, with_map, p.radius))


def test_anchor_one_byte_per_light_gives_its_quotient():
    """Where every tap that can be accepted carries the same byte c, the result is (float)c / (float)n_l whatever the window, the
    thresholds and the distances accept -- the licence of the device form's shortcut."""
    nrm, pos, planes, mask, lights_map, dist = fc.geometric((33, 18))
    background = (nrm[..., :3] == 0).all(axis=-1)
    lst = fc.the_list("soft", "8")
    flat = np.stack([np.full(background.shape, b, np.uint8) for b in (0, 1, 2, 3, 16, 17, 48, 255)])
    for radius in (1, 2, 8):
        for d in (None, dist):
            got = api.filter_soft_light_list(lst, fc.params(radius), pos, nrm, flat, lights_map, d)
            for l in range(8):
                on = ~background & (((lights_map >> l) & 1) != 0)
                want = np.where(on, f32(flat[l, 0, 0]) / f32(max(1, lst.lights[l].nsamples)), f32(0))
                fc.same_bits(got[l], want, (radius, d is not None, l))
    hard = fc.the_list("hard", "8")
    got = api.filter_light_list(hard, fc.params(8), pos, nrm, np.full(background.shape, 0xA5, np.uint8), lights_map)
    for l in range(8):
        on = ~background & (((lights_map >> l) & 1) != 0)
        fc.same_bits(got[l], np.where(on, f32((0xA5 >> l) & 1), f32(0)), ("hard", l))


def test_planes_from_the_count_up_are_never_touched():
    """Exactly `count` planes of counts, distances and visibility: a heap block of that size, poison behind it in a larger one."""
    nrm, pos, planes, mask, lights_map, dist = fc.geometric((17, 15))
    lst = fc.the_list("soft", "3")
    p = fc.params(2)
    want = fc.filter_rule(lst, p, pos, nrm, planes, lights_map, dist)
    lib = api._lib
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    counts, distances = planes.copy(), dist.copy()
    counts[3:] = 0xFF
    distances[3:] = np.nan
    vis = np.full((8, 15, 17), 7.5, f32)
    nrm_c, pos_c = np.ascontiguousarray(nrm), np.ascontiguousarray(pos)
    assert lib.rtsh_filter_soft_light_list(C.byref(lst), C.byref(p), ptr(pos_c), ptr(nrm_c), ptr(np.ascontiguousarray(lights_map)), ptr(counts),
                                           ptr(distances), 17, 15, ptr(vis), 0) == 0
    fc.same_bits(vis[:3], want, "planes below the count")
    assert (vis[3:] == 7.5).all()
    # a background pixel's position, map byte, count bytes and distances, and the bytes of a light whose map bit is clear
    background = (nrm[..., :3] == 0).all(axis=-1)
    counts, distances, map2 = planes.copy(), dist.copy(), lights_map.copy()
    for l in range(3):
        off = ((lights_map >> l) & 1) == 0
        counts[l][off] ^= 0xFF
        distances[l][off] = 0.0
    counts[:, background] ^= 0xFF
    map2[background] ^= 0xFF
    fc.same_bits(api.filter_soft_light_list(lst, p, pos, nrm, counts, map2, distances), want, "poisoned unread bytes")


def test_refusals_write_nothing():
    lib = api._lib
    nrm, pos, planes, mask, lights_map, dist = (np.ascontiguousarray(a) for a in fc.geometric((16, 16)))
    vis = np.full((8, 16, 16), 7.5, f32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ref = lambda s: C.byref(s) if s is not None else None
    good = fc.params(2)
    hard_bad, soft_bad = lc.bad_lists()
    hard, soft = fc.the_list("hard", "3"), fc.the_list("soft", "3")

    def call(form, lst, p, pos_=pos, nrm_=nrm, plane="x", dist_=dist, W=16, H=16, out=vis):
        if form == "hard":
            return lib.rtsh_filter_light_list(ref(lst), ref(p), ptr(pos_) if pos_ is not None else None, ptr(nrm_) if nrm_ is not None else None,
                                              ptr(lights_map), ptr(mask) if plane is not None else None, W, H,
                                              ptr(out) if out is not None else None, 0)
        return lib.rtsh_filter_soft_light_list(ref(lst), ref(p), ptr(pos_) if pos_ is not None else None, ptr(nrm_) if nrm_ is not None else None,
                                               ptr(lights_map), ptr(planes) if plane is not None else None,
                                               ptr(dist_) if dist_ is not None else None, W, H, ptr(out) if out is not None else None, 0)

    def bad_params():
        out = [None]
        for field, value in (("radius", 9), ("radius", 0xFFFFFFFF), ("normal_cos_min", np.nan), ("normal_cos_min", np.inf),
                             ("plane_eps", -np.inf), ("plane_eps", np.nan)):
            p = fc.params(2)
            setattr(p, field, value)
            out.append(p)
        return out

    for form, lst, bad in (("hard", hard, hard_bad), ("soft", soft, soft_bad)):
        assert call(form, lst, good) == 0
        vis[:] = 7.5
        for b in bad:
            assert call(form, b, good) == INVALID, form
        for p in bad_params():
            assert call(form, lst, p) == INVALID, form
        assert call(form, lst, good, pos_=None) == INVALID             # positions are always required
        assert call(form, lst, good, nrm_=None) == INVALID
        assert call(form, lst, good, plane=None) == INVALID
        assert call(form, lst, good, out=None) == INVALID
        assert call(form, lst, good, W=0) == INVALID
        assert call(form, lst, good, H=0) == INVALID
        assert (vis == 7.5).all(), form
    for l, value in ((0, -1.0), (1, np.nan), (2, np.inf), (2, -1e-45)):
        p = fc.params(2)
        p.spread[l] = value
        assert call("soft", soft, p) == INVALID, (l, value)              # with distances ...
        assert call("soft", soft, p, dist_=None) == 0                    # ... and ignored without
        vis[:] = 7.5
    p = fc.params(2)
    p.spread[3] = np.nan                                                 # (a spread from the count up is not looked at)
    assert call("soft", soft, p) == 0
    with pytest.raises(api.RtsError):
        api.filter_soft_light_list(soft, good, None, nrm, planes)


@pytest.mark.parametrize("kind", ["awkward", "geometric"])
def test_visibility_combine_over_an_r0_filter_is_the_list_combine(kind):
    """combine_visibility_list over the planes of an R = 0 filter: combine_soft_light_list's bytes (combine_light_list's for a hard
    list), byte for byte -- with and without map, white, tame and wild colours."""
    k = sp.constants("unit")
    for wh in ((16, 16), (3, 333)):
        nrm, pos, planes, mask, lights_map, _ = fc.frame(kind, wh)
        for name in ("3", "8"):
            soft, hard = fc.the_list("soft", name), fc.the_list("hard", name)
            for with_map in (False, True):
                m = lights_map if with_map else None
                for colours, colors in lc.colour_sets(soft.count).items():
                    vis = api.filter_soft_light_list(soft, fc.params(0), pos, nrm, planes, m)
                    got = api.combine_visibility_list(k, soft.hard_list(), pos, nrm, vis, m, colors)
                    want = api.combine_soft_light_list(k, soft, pos, nrm, planes, m, colors)
                    assert (got == want).all(), (kind, wh, name, with_map, colours, "soft")
                    vis = api.filter_light_list(hard, fc.params(0), pos, nrm, mask, m)
                    got = api.combine_visibility_list(k, hard, pos, nrm, vis, m, colors)
                    want = api.combine_light_list(k, hard, pos, nrm, mask, m, colors)
                    assert (got == want).all(), (kind, wh, name, with_map, colours, "hard")


@pytest.mark.parametrize("wh", [(1, 1), (1, 5), (16, 16), (3, 333)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_visibility_combine_equals_its_numpy_rule(wh):
    """Arbitrary finite, negative, huge, NaN and Inf visibility; lists of 1, 3 and 8 lights; with and without positions and map."""
    nrm, pos, _, _, lights_map = lc.frame(wh)
    vis = fc.wild_visibility(wh)
    for kind in ("unit", "zero", "long"):
        k = sp.constants(kind)
        for name, (lst, has_point) in lc.hard_lists().items():
            for with_map in (False, True):
                for colours, colors in lc.colour_sets(lst.count).items():
                    if kind != "unit" and colours != "wild":
                        continue
                    for p in ((pos,) if has_point else (pos, None)):
                        m = lights_map if with_map else None
                        want = fc.visibility_combine_rule(k, lst, p, nrm, vis, m, colors)
                        got = api.combine_visibility_list(k, lst, p, nrm, vis, m, colors)
                        assert (got == want).all(), (wh, kind, name, with_map, colours, p is not None)


def test_visibility_combine_refusals_write_nothing():
    lib = api._lib
    nrm, pos, _, _, lights_map = (np.ascontiguousarray(a) for a in lc.frame((16, 16)))
    vis = fc.wild_visibility((16, 16))
    rgb = np.full((16, 16, 3), 0xAB, np.uint8)
    k = sp.constants("unit")
    kk = C.byref(k)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ref = lambda s: C.byref(s) if s is not None else None
    fn = lib.rtsh_combine_visibility_list
    two, three = lc.the_list("hard", "2_directional"), lc.the_list("hard", "3")
    assert fn(kk, ref(two), None, None, p(nrm), p(lights_map), p(vis), 16, 16, p(rgb)) == 0
    rgb[:] = 0xAB
    for lst in lc.bad_lists()[0]:
        assert fn(kk, ref(lst), None, p(pos), p(nrm), p(lights_map), p(vis), 16, 16, p(rgb)) == INVALID
    assert fn(None, ref(two), None, p(pos), p(nrm), p(lights_map), p(vis), 16, 16, p(rgb)) == INVALID
    assert fn(kk, ref(two), None, p(pos), None, p(lights_map), p(vis), 16, 16, p(rgb)) == INVALID
    assert fn(kk, ref(two), None, p(pos), p(nrm), p(lights_map), None, 16, 16, p(rgb)) == INVALID
    assert fn(kk, ref(two), None, p(pos), p(nrm), p(lights_map), p(vis), 16, 16, None) == INVALID
    assert fn(kk, ref(three), None, None, p(nrm), p(lights_map), p(vis), 16, 16, p(rgb)) == INVALID      # a point light, no positions
    assert fn(kk, ref(two), None, p(pos), p(nrm), p(lights_map), p(vis), 0, 16, p(rgb)) == INVALID
    assert fn(kk, ref(two), None, p(pos), p(nrm), p(lights_map), p(vis), 16, 0, p(rgb)) == INVALID
    assert (rgb == 0xAB).all()


def test_list_filter_under_address_and_ub_sanitizers(tmp_path):
    """tests/cpp/list_filter_host.cpp: the host twins themselves (rts_scene.cpp and the shared per-pixel source, compiled into the
    program -- nothing sanitized is loaded into Python) under -fsanitize=address,undefined,float-cast-overflow, over every refusal and
    over small frames of awkward texels whose buffers are heap blocks of exactly the size the header states."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "list_filter_host")
    csrc = os.path.join(root, "raytracedshadows_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined,float-cast-overflow",
                    "-fno-sanitize-recover=all", os.path.join(root, "tests", "cpp", "list_filter_host.cpp"),
                    os.path.join(csrc, "rts_scene.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    assert run.stdout.startswith("ok ") and int(run.stdout.split()[1]) > 1000, run.stdout[-2000:]
