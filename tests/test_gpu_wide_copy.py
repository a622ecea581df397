"""GPU: kernel 8's private copy, the device verdict and the confirmation of triangle hits, against the numpy restatement
(tests/wide_copy.py) and the CPU oracle.

* The copy rtsh_ctx_read_private_copy returns after an install, and after an in-place refit, must be the restatement's byte
  for byte, on scene streams, every device producer's, at the scan's tile boundaries and on hand-made shapes.
* The verdict (bvh_finite / bvh_ordered / bvh_enclosed, and refusal) must be the restated one on the mutation corpus, and every
  kernel must still trace each accepted stream as the oracle does.
* Chains at the 512-level cut-off, and boxes shrunk so that triangles stick out of them: the wide kernels are exact only
  because a triangle hit is confirmed against the exact box of the leaf's parent."""
import numpy as np
import pytest

import oracle
import streams
import wide_copy as wc
from raytracedshadows_amd import api, scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert api.device_count() >= 1, "no GPU visible: the shadow path has no CPU fallback"
    c = api.ShadowContext(0)
    yield c
    c.close()


def _kernels(ctx):
    return list(range(ctx.get_option("kernel_count")))


def _copy_matches(ctx, packed, what):
    """The installed stream's verdict, wide_nodes / wide_levels and private copy are the restatement's."""
    rs = wc.restate(packed)
    P = (np.asarray(packed).reshape(-1, 4).shape[0] + 2) // 5
    bits = rs["bits"]
    assert ctx.get_option("bvh_finite") == int(not bits & wc.NONFINITE), what
    assert ctx.get_option("bvh_ordered") == int(not bits & wc.UNORDERED), what
    assert ctx.get_option("bvh_enclosed") == int(not bits & wc.NOT_ENCLOSED), what
    assert ctx.get_option("wide_nodes") == rs["wide_nodes"], (what, ctx.get_option("wide_nodes"), rs["wide_nodes"])
    assert ctx.get_option("wide_levels") == rs["levels"], (what, ctx.get_option("wide_levels"), rs["levels"])
    got = api.read_private_copy(ctx)
    diff = wc.first_difference(got, rs, P)
    assert diff is None, f"{what}: {diff}"
    return rs


_triangles_of = streams.triangles_of


def _moved(v):
    w = v.copy()
    span = float(np.ptp(v[:, 0])) + 1.0
    w[:, 1] += (0.02 * span * np.sin(5.0 * v[:, 0] / span + 0.4)).astype(np.float32)
    return w


def _install_check_refit(ctx, packed, v, stride, idx, what):
    ctx.set_bvh(packed)
    rs = _copy_matches(ctx, packed, what)
    P = idx.size // 3
    got, _, _ = api.bvh_refit_device(ctx, _moved(v), stride, idx, P, want_packed=True)
    assert not np.array_equal(got, packed)
    after = _copy_matches(ctx, got, what + ", after a device refit")
    return rs, after


def _shape(name):
    rs = np.random.RandomState(len(name))
    if name.startswith("soup"):
        P = int(name[4:])
        c = rs.random_sample((P, 1, 3)) * 50
        t = (c + (rs.random_sample((P, 3, 3)) - 0.5) * 2).astype(np.float32)
        v, idx = t.reshape(-1, 3), np.arange(3 * P, dtype=np.uint32)
        return api.BVHBuilder().build(v, 3, idx, P).m_packedNodes, v, idx
    if name == "deep_bushy":
        packed = streams.deep_bushy_stream(25)
    else:
        P = int(name.split("_")[1])
        t = (rs.random_sample((P, 1, 3)) * 20 + rs.random_sample((P, 3, 3))).astype(np.float32)
        packed = streams.stream_from_tree(wc.chain(P) if name.startswith("chain") else wc.complete(0, P), t)
    t = _triangles_of(packed)
    return packed, t.reshape(-1, 3), np.arange(t.shape[0] * 3, dtype=np.uint32)


# P = 512 / 513: N = 1023 / 1025 (one and two scan tiles); 131072 / 131073: 256 and 257 tiles (a second scanOfSums round)
@pytest.mark.parametrize("name", ["soup2", "soup3", "soup512", "soup513", "soup131072", "soup131073", "chain_300", "chain_3000",
                                  "complete_1024", "complete_777", "deep_bushy"])
def test_copy_of_shapes_and_scan_boundaries(ctx, name):
    packed, v, idx = _shape(name)
    rs, _ = _install_check_refit(ctx, packed, v, 3, idx, name)
    assert (rs["wide_nodes"] > 0) == (name != "chain_3000")


@pytest.mark.parametrize("name", ["cornell", "atrium", "city"])
def test_copy_of_scene_streams(ctx, name):
    v, idx = scenes.SCENES[name]().flat()
    P = idx.size // 3
    packed = api.BVHBuilder().build(v, 8, idx, P).m_packedNodes
    rs, _ = _install_check_refit(ctx, packed, v, 8, idx, name)
    assert rs["wide_nodes"] > 0


@pytest.mark.parametrize("algo", ["sah", "lbvh", "ploc", "ploc_sah"])
def test_copy_of_every_device_producer(ctx, algo):
    rs = np.random.RandomState(9)
    P = 30011
    t = (rs.random_sample((P, 1, 3)) * 40 + (rs.random_sample((P, 3, 3)) - 0.5) * 1.5).astype(np.float32)
    v, idx = t.reshape(-1, 3), np.arange(3 * P, dtype=np.uint32)
    packed, _ = api.bvh_build_device(ctx, v, 3, idx, P, install=True, algorithm=algo)
    _copy_matches(ctx, packed, algo)
    got, _, _ = api.bvh_refit_device(ctx, _moved(v), 3, idx, P, want_packed=True)
    _copy_matches(ctx, got, algo + ", after a device refit")


_aimed_frame = streams.aimed_frame


def _every_kernel_equals_oracle(ctx, packed, pos, k, light, what):
    H, W = pos.shape[:2]
    want, _, _ = oracle.shadow_mask(packed, k.as_array(), oracle.light_from_product(light, k), pos, W, H)
    try:
        for kernel in _kernels(ctx):
            ctx.set_option("kernel", kernel)
            got = ctx.trace_shadow_mask(k, pos, W, H, light=light)
            assert (got == want).all(), (what, kernel, int((got != want).sum()))
    finally:
        ctx.set_option("kernel", -1)
    return want


@pytest.mark.parametrize("case", wc.corpus(), ids=lambda c: c[0])
def test_verdict_on_the_mutation_corpus(ctx, case):
    name, packed, expected, compared, target = case
    bits = wc.verdict(packed)
    assert bits & compared == expected
    if bits & wc.STRUCTURE:
        with pytest.raises(api.RtsError) as e:
            ctx.set_bvh(packed)
        assert e.value.status == 5, name                   # RTS_ERR_BAD_BVH
        return
    ctx.set_bvh(packed)
    _copy_matches(ctx, packed, name)
    pos, k, light = _aimed_frame(packed, target)
    _every_kernel_equals_oracle(ctx, packed, pos, k, light, name)


@pytest.mark.parametrize("P", [512, 513, 514])
def test_depth_cut_off(ctx, P):
    """Chains whose deepest leaf sits at depth 511, 512, 513: the first two get a copy, the last none; every kernel is exact."""
    packed, v, idx = _shape(f"chain_{P}")
    ctx.set_bvh(packed)
    rs = _copy_matches(ctx, packed, f"chain {P}")
    assert rs["levels"] == ((P - 1) // 2 + 1 if P <= 513 else 0)
    assert (ctx.get_option("wide_nodes") == 0) == (P == 514)
    pos, k, light = _aimed_frame(packed, 0, 40, 24, seed=P)
    want = _every_kernel_equals_oracle(ctx, packed, pos, k, light, f"chain {P}")
    assert 0 < want.sum() < want.size


# ---- confirmation at its edge ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def confirm():
    s = wc.confirmation_scene()
    rng = np.random.RandomState(5)
    offsets = np.zeros((16, 4), np.float32)
    offsets[:, :3] = (rng.random_sample((16, 3)) * 2 - 1) * 4e-3          # crossing points move by about +-30 ulps
    s["offsets"] = offsets
    s["count"] = wc.confirmation_rays(s)
    s["count16"] = wc.confirmation_rays(s, offsets)
    return s


def _device_mask(ctx, k, d_pos, d_mask, W, H, light):
    got = np.full((H, W), 9, np.uint8)
    ctx.h2d(d_mask, got)
    ctx.trace_shadow_mask_device(k, d_pos, W, H, d_mask, light=light)
    ctx.synchronize()
    ctx.d2h(got, d_mask)
    return got


def test_confirmation_at_the_edge_of_shrunk_boxes(ctx, confirm):
    s = confirm
    n, n16 = s["count"], s["count16"]
    print(f"\nconfirmation: {n['teeth']} of {n['rays']} rays (16 samples: {n16['teeth']} of {n16['rays']}) hit a triangle outside "
          f"its exact parent box within 16 ulps of the face and are lit; by parent depth even/odd: {n['by_depth_parity']}")
    assert n["teeth"] >= 0.03 * n["rays"] and n16["teeth"] >= 0.03 * n16["rays"]
    packed = s["packed"]
    ctx.set_bvh(packed)
    rs = _copy_matches(ctx, packed, "shrunk boxes")
    assert rs["bits"] == 0 and ctx.get_option("wide_nodes") > 0
    H, W = s["k"].shape
    k = api.RayTracingConstants.make([0, 0, 0], [0, 1, 0], W, H)
    point = api.Light.make(api.Light.POINT, s["light"])
    soft = api.Light.make(api.Light.POINT, s["light"], s["offsets"])
    pos = s["positions"]
    want = {}
    for name, lt in (("point", point), ("soft", soft)):
        want[name], _, _ = oracle.shadow_mask(packed, k.as_array(), oracle.light_from_product(lt, k), pos, W, H)
    d_pos, d_mask = ctx.malloc(pos.nbytes), ctx.malloc(W * H)
    ctx.h2d(d_pos, pos)
    defaults = {key: ctx.get_option(key) for key in ("kernel", "packet_share", "wide_lane", "soft_split", "block_waves")}
    try:
        for kernel in _kernels(ctx):                                          # every kernel, default options
            ctx.set_option("kernel", kernel)
            got = _device_mask(ctx, k, d_pos, d_mask, W, H, point)
            assert (got == want["point"]).all(), ("every kernel", kernel, int((got != want["point"]).sum()))
        for kernel in (8, 9):                                                 # the wide loops, dissolved lanes of both kinds
            for lane in (0, 1):
                for share in (0, 16, defaults["packet_share"]):
                    ctx.set_option("kernel", kernel)
                    ctx.set_option("wide_lane", lane)
                    ctx.set_option("packet_share", share)
                    got = _device_mask(ctx, k, d_pos, d_mask, W, H, point)
                    assert (got == want["point"]).all(), (kernel, lane, share, int((got != want["point"]).sum()))
                    for split in (0, 1):                                      # 16 jittered samples straddling the faces
                        ctx.set_option("soft_split", split)
                        got = _device_mask(ctx, k, d_pos, d_mask, W, H, soft)
                        assert (got == want["soft"]).all(), ("soft", kernel, lane, share, split, int((got != want["soft"]).sum()))
                    ctx.set_option("soft_split", defaults["soft_split"])
        ctx.set_option("wide_lane", 0)
        ctx.set_option("packet_share", defaults["packet_share"])
        ctx.set_option("block_waves", 1)
        for kernel in (3, 8):                                                 # split pieces (TEAM) walk index ranges
            ctx.set_option("kernel", kernel)
            tiles, pieces = ctx.plan_splits(k, d_pos, W, H, d_mask, light=point, min_life_us=0.3, piece_us=0.2, max_pieces=16,
                                            front_share=0.4)
            assert tiles > 0 and ctx.get_option("split_pieces") > 0, (kernel, tiles, pieces)
            for share in (0, 16, defaults["packet_share"]):
                ctx.set_option("packet_share", share)
                got = _device_mask(ctx, k, d_pos, d_mask, W, H, point)
                assert (got == want["point"]).all(), ("split table", kernel, share, int((got != want["point"]).sum()))
            ctx.set_option("packet_share", defaults["packet_share"])
            ctx.clear_splits()
        ctx.set_option("block_waves", defaults["block_waves"])
        # a ragged frame: the same rays without the last three columns and two rows
        Hr, Wr = H - 2, W - 3
        rpos = np.ascontiguousarray(pos[:Hr, :Wr])
        rk = api.RayTracingConstants.make([0, 0, 0], [0, 1, 0], Wr, Hr)
        rwant, _, _ = oracle.shadow_mask(packed, rk.as_array(), oracle.light_from_product(point, rk), rpos, Wr, Hr)
        assert (rwant == want["point"][:Hr, :Wr]).all()
        for kernel in _kernels(ctx):
            ctx.set_option("kernel", kernel)
            got = ctx.trace_shadow_mask(rk, rpos, Wr, Hr, light=point)
            assert (got == rwant).all(), ("ragged", kernel, int((got != rwant).sum()))
    finally:
        for key, val in defaults.items():
            ctx.set_option(key, val)
        ctx.clear_splits()
        ctx.free(d_pos)
        ctx.free(d_mask)
