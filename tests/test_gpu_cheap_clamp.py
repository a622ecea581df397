"""Masks of the wide kernels with the clamped cheap test of segment rays (tools/gen_wide_asm.py: cheap_pair),
byte for byte against the CPU oracle, on frames where many boxes straddle t = 1: the point light sits inside the geometry,
just above it, or on a triangle's plane.  Kernels 8 and 9, wide_lane on and off, split-table pieces, 16-sample soft lights
and the directional light."""
import numpy as np
import pytest

import oracle
from raytracedshadows_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    assert api.device_count() >= 1, "no GPU visible: the shadow path has no CPU fallback"
    c = api.ShadowContext(0)
    yield c
    c.close()


def _soup(n=6000, seed=3):
    """n small triangles in the unit cube plus a floor (y = 0) of two large ones."""
    rng = np.random.RandomState(seed)
    c = rng.random_sample((n, 1, 3))
    tri = c + (rng.random_sample((n, 3, 3)) - 0.5) * 0.06
    floor = np.array([[[-1, 0, -1], [2, 0, -1], [2, 0, 2]], [[-1, 0, -1], [2, 0, 2], [-1, 0, 2]]], np.float64)
    tri = np.concatenate([tri, floor]).astype(np.float32)
    verts = np.zeros((tri.shape[0] * 3, 8), np.float32)
    verts[:, :3] = tri.reshape(-1, 3)
    idx = np.arange(tri.shape[0] * 3, dtype=np.uint32)
    packed = api.BVHBuilder().build(verts, 8, idx, tri.shape[0]).m_packedNodes
    return packed, tri


def _frame(tri, W=64, H=48, seed=4):
    """G-buffer positions: points on random triangles (origins on the faces, where the bias decides)."""
    rng = np.random.RandomState(seed)
    t = tri[rng.randint(0, tri.shape[0], H * W)].astype(np.float64)
    u, v = rng.random_sample((2, H * W, 1))
    flip = (u + v) > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    p = t[:, 0] + u * (t[:, 1] - t[:, 0]) + v * (t[:, 2] - t[:, 0])
    pos = np.zeros((H, W, 4), np.float32)
    pos[..., :3] = p.reshape(H, W, 3)
    return pos


LIGHTS = {
    "inside": [0.5, 0.5, 0.5],          # boxes all around the light: near > 1 beyond it
    "just_above": [0.5, 1.035, 0.5],    # a hair above the top of the soup
    "on_floor_plane": [0.3, 0.0, 0.7],  # on the plane of the floor's triangles
    "corner": [1.02, 1.02, 1.02],
}


def _mask(ctx, k, pos, light):
    H, W = pos.shape[:2]
    return ctx.trace_shadow_mask(k, pos, W, H, light=light)


def _want(packed, k, pos, light):
    H, W = pos.shape[:2]
    want, _, _ = oracle.shadow_mask(packed, k.as_array(), oracle.light_from_product(light, k), pos, W, H)
    return want


@pytest.fixture(scope="module")
def soup():
    return _soup()


@pytest.mark.parametrize("where", sorted(LIGHTS))
def test_wide_kernels_equal_the_oracle_with_the_light_among_the_boxes(ctx, soup, where):
    packed, tri = soup
    ctx.set_bvh(packed)
    assert ctx.get_option("wide_nodes") > 0
    pos = _frame(tri)
    H, W = pos.shape[:2]
    k = api.RayTracingConstants.make([0, 0, 0], [0.3, 0.8, 0.5], W, H)
    point = api.Light.make(api.Light.POINT, np.array(LIGHTS[where], np.float32))
    rng = np.random.RandomState(11)
    offsets = np.zeros((16, 4), np.float32)
    offsets[:, :3] = (rng.random_sample((16, 3)) * 2 - 1) * 0.05
    soft = api.Light.make(api.Light.POINT, np.array(LIGHTS[where], np.float32), offsets)
    want = {"point": _want(packed, k, pos, point), "soft": _want(packed, k, pos, soft)}
    assert int((want["point"] == 0).sum()) > 0                             # some pixels are shadowed
    defaults = {key: ctx.get_option(key) for key in ("kernel", "wide_lane", "soft_split", "packet_share")}
    try:
        for kernel in (8, 9):
            for lane in (0, 1):
                for share in (0, 16):
                    ctx.set_option("kernel", kernel)
                    ctx.set_option("wide_lane", lane)
                    ctx.set_option("packet_share", share)
                    got = _mask(ctx, k, pos, point)
                    assert (got == want["point"]).all(), (where, kernel, lane, share, int((got != want["point"]).sum()))
                    for split in (0, 1):
                        ctx.set_option("soft_split", split)
                        got = _mask(ctx, k, pos, soft)
                        assert (got == want["soft"]).all(), ("soft", where, kernel, lane, share, split,
                                                             int((got != want["soft"]).sum()))
                    ctx.set_option("soft_split", defaults["soft_split"])
    finally:
        for key, val in defaults.items():
            ctx.set_option(key, val)


def test_split_pieces_and_the_directional_light(ctx, soup):
    packed, tri = soup
    ctx.set_bvh(packed)
    pos = _frame(tri, 96, 64, seed=9)
    H, W = pos.shape[:2]
    k = api.RayTracingConstants.make([0, 0, 0], [0.3, 0.8, 0.5], W, H)
    lights = {"inside": api.Light.make(api.Light.POINT, np.array(LIGHTS["inside"], np.float32)),
              "just_above": api.Light.make(api.Light.POINT, np.array(LIGHTS["just_above"], np.float32)),
              "directional": api.Light.make(api.Light.DIRECTIONAL, np.array([0.3, 0.8, 0.5], np.float32))}
    d_pos, d_mask = ctx.malloc(pos.nbytes), ctx.malloc(W * H)
    ctx.h2d(d_pos, pos)
    defaults = {key: ctx.get_option(key) for key in ("kernel", "wide_lane", "packet_share", "block_waves")}
    try:
        for name, light in lights.items():
            want = _want(packed, k, pos, light)
            for kernel in (8, 9):                                            # whole frame, both lane modes
                for lane in (0, 1):
                    ctx.set_option("kernel", kernel)
                    ctx.set_option("wide_lane", lane)
                    got = _mask(ctx, k, pos, light)
                    assert (got == want).all(), (name, kernel, lane, int((got != want).sum()))
            ctx.set_option("wide_lane", 0)
            ctx.set_option("block_waves", 1)
            ctx.set_option("kernel", 8)                                      # split pieces walk index ranges (wideDescendRange)
            tiles, _ = ctx.plan_splits(k, d_pos, W, H, d_mask, light=light, min_life_us=0.3, piece_us=0.2, max_pieces=16,
                                       front_share=0.4)
            assert tiles > 0 and ctx.get_option("split_pieces") > 0, name
            for share in (0, 16, defaults["packet_share"]):
                ctx.set_option("packet_share", share)
                got = np.full((H, W), 9, np.uint8)
                ctx.h2d(d_mask, got)
                ctx.trace_shadow_mask_device(k, d_pos, W, H, d_mask, light=light)
                ctx.synchronize()
                ctx.d2h(got, d_mask)
                assert (got == want).all(), ("split table", name, share, int((got != want).sum()))
            ctx.set_option("packet_share", defaults["packet_share"])
            ctx.clear_splits()
            ctx.set_option("block_waves", defaults["block_waves"])
    finally:
        for key, val in defaults.items():
            ctx.set_option(key, val)
        ctx.clear_splits()
        ctx.free(d_pos)
        ctx.free(d_mask)
