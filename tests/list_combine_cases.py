"""Shared by the list combine tests (tests/test_list_combine_host.py, tests/test_gpu_list_combine.py): awkward frames for the combine
pass of a light list (include/rts_scene.h, rtsh_combine_light_list* / rtsh_combine_soft_light_list*) and the expected bytes from a
float32 numpy restatement of its per-pixel rule, written here from the header's text and independently of the C++.  The awkward
texels, the constants, the lights, the light lists and N.L come from tests/scene_pass_cases.py.  No GPU code is touched here.

A frame is (normals[H, W, 4], positions[H, W, 4], planes[8, H, W], mask[H, W], lights_map[H, W]): every pixel takes one entry of
scene_pass_cases' NORMALS and POSITIONS (29 and 8 entries, cycling from a start that differs per frame), every plane one of BYTES
(9 entries, a different stride per plane: bytes above every sample count among them), the hard mask and the light map arbitrary bytes.
All eight planes are always there, so that the planes from a list's count up can be poisoned.  Everything is compared byte for byte."""
import numpy as np

import scene_pass_cases as sp
from raytracedshadows_amd import api

f32 = np.float32
NAN, INF = np.nan, np.inf

#: W x H of the frames: every W * H mod 4, odd plane strides, sizes around one workgroup of 256 lanes and of 4 x 256 pixels
FRAMES = [(1, 1), (1, 3), (2, 2), (1, 5), (1, 255), (16, 16), (1, 257), (3, 333), (1, 1021)]
#: plane bytes: 0, counts inside 2, 16 and 48 samples, and bytes above each of them
BYTES = np.array([0, 1, 2, 3, 16, 17, 48, 64, 255], np.uint8)

_FRAMES = {}


def frame(wh):
    """(normals, positions, planes, mask, lights_map) of a W x H frame: built once, shared, read-only."""
    if wh not in _FRAMES:
        W, H = wh
        i = np.arange(H * W) + 17 * ((31 * W + H) % 29)
        nrm = np.zeros((H * W, 4), f32)
        pos = np.ones((H * W, 4), f32)
        nrm[:, :3] = sp.NORMALS[i % len(sp.NORMALS)]
        pos[:, :3] = sp.POSITIONS[(i // 3) % len(sp.POSITIONS)]
        planes = np.stack([BYTES[(i * (l + 1) + 2 * l) % len(BYTES)] for l in range(8)]).astype(np.uint8)
        mask = ((i * 73 + 5) % 256).astype(np.uint8)
        lights_map = ((i * 37 + 11) % 256).astype(np.uint8)
        out = (nrm.reshape(H, W, 4), pos.reshape(H, W, 4), np.ascontiguousarray(planes.reshape(8, H, W)), mask.reshape(H, W),
               lights_map.reshape(H, W))
        for a in out:
            a.setflags(write=False)
        _FRAMES[wh] = out
    return _FRAMES[wh]


def hard_lists():
    """name -> (LightList, whether it holds a point light): scene_pass_cases' lists of 1, 3 and 8 mixed lights, and two directional."""
    return sp.light_lists()


#: nsamples of entry l of a soft list: hard entries (0 and 1) inside, and 2, 16 and 48 samples
NSAMPLES = [16, 2, 1, 48, 0, 16, 2, 3]


def soft_lists():
    """name -> (SoftLightList, whether it holds a point light): the hard lists' types and positions, entry l of NSAMPLES[l] samples."""
    out = {}
    for name, (lst, has_point) in sp.light_lists().items():
        entries = []
        for l in range(lst.count):
            n = NSAMPLES[l]
            entries.append((lst.lights[l].type, list(lst.lights[l].xyz), n, 0 if n < 2 else 48 - n, 0.25))
        out[name] = (api.SoftLightList.make(entries, np.zeros((48, 3), f32)), has_point)
    return out


def one_soft(light):
    """The one-entry soft list of a ``Light``: its type, centre and sample count (the combine pass looks at nothing else)."""
    return api.SoftLightList.make([(light.type, list(light.xyz), light.nsamples, 0, 1.0)], np.zeros((48, 3), f32))


def colour_sets(count):
    """name -> None or float32[count, 4]: white by default, tame colours, and wild ones -- 0, negative, above 1, +Inf and NaN."""
    tame = np.array([(1.0, 0.5, 0.25, 9.0), (0.125, 1.0, 0.75, NAN), (0.3, 0.3, 1.0, 0.0), (0.7, 0.2, 0.1, 1.0)], f32)
    wild = np.array([(0.0, -1.0, 2.5, 0.0), (1.0, 0.1, -0.0, 1.0), (INF, 0.5, 0.5, 0.0), (0.25, NAN, 1e30, 0.0), (-3.0, 7.0, 1e-41, 0.0),
                     (1.0, 1.0, 1.0, 0.0), (-INF, 0.2, 0.0, 0.0), (0.5, 0.5, 3e38, 0.0)], f32)
    k = np.arange(count)
    return {"white": None, "tame": np.ascontiguousarray(tame[k % len(tame)]), "wild": np.ascontiguousarray(wild[(k + count) % len(wild)])}


# ---------------------------------------------------------------------------------------------- the per-pixel rule, written out in float32
def list_combine_rule(k, lst, positions, normals, planes, lights_map=None, colors=None):
    """uint8[H, W, 3] of a light list's combine pass, in float32, operation for operation (numpy has no fused multiply-add) --
        background (normal all zero): 0, 0, 0
        ambient = 0.15 + 0.05 * (1 - max0(N . -view)), once per pixel, view = cameraDirection normalised where its length is > 0
        sum[c]  = +0;  for l in list order, where the map is None or has bit l:
                  direct = (1.25 * max0(N . L_l)) * (byte_l / samples_l);   sum[c] = sum[c] + direct * color_l[c]
        byte    = 255 where scaled >= 255, int(scaled) where 0 < scaled < 255, 0 otherwise (a NaN included), scaled = (sum + ambient) * 255 + 0.5
    ``lst`` a ``LightList``: ``planes`` is the mask, byte_l = its bit l, samples_l = 1; a ``SoftLightList``: byte_l = planes[l],
    samples_l = max(1, nsamples_l).  N . L_l is scene_pass_cases.ndl_rule for the light of entry l's type and position alone."""
    hard = isinstance(lst, api.LightList)
    with np.errstate(all="ignore"):
        n = np.ascontiguousarray(normals, f32)
        nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
        cx, cy, cz = (f32(k.cameraDirection[i]) for i in range(3))
        cl = np.sqrt((cx * cx + cy * cy) + cz * cz)
        if cl > 0:
            inv = f32(1.0) / cl
            cx, cy, cz = cx * inv, cy * inv, cz * inv
        ndv = (nx * (cx * f32(-1.0)) + ny * (cy * f32(-1.0))) + nz * (cz * f32(-1.0))
        ndv = np.where(ndv > 0, ndv, f32(0))
        ambient = f32(0.15) + f32(0.05) * (f32(1.0) - ndv)
        planes = np.ascontiguousarray(planes, np.uint8)
        sums = [np.zeros(nx.shape, f32) for _ in range(3)]
        for l in range(lst.count):
            e = lst.lights[l]
            ndl = sp.ndl_rule(k, api.Light.make(e.type, list(e.xyz)), positions, normals)
            ndl = np.where(ndl > 0, ndl, f32(0))
            if hard:
                byte, samples = ((planes >> l) & 1).astype(f32), f32(1.0)
            else:
                byte, samples = planes[l].astype(f32), f32(max(1, e.nsamples))
            direct = (f32(1.25) * ndl) * (byte / samples)
            on = np.ones(nx.shape, bool) if lights_map is None else ((np.asarray(lights_map, np.uint8) >> l) & 1) != 0
            for c in range(3):
                color = f32(1.0) if colors is None else f32(np.asarray(colors, f32)[l, c])
                product = (direct * color).astype(f32)
                sums[c] = np.where(on, sums[c] + product, sums[c]).astype(f32)
        background = (nx == 0) & (ny == 0) & (nz == 0)
        out = np.zeros(nx.shape + (3,), np.uint8)
        for c in range(3):
            scaled = (sums[c] + ambient) * f32(255.0) + f32(0.5)
            assert scaled.dtype == f32
            inside = (scaled > 0) & (scaled < 255)
            byte = np.where(scaled >= 255, 255, np.where(inside, np.where(inside, scaled, 0).astype(np.int32), 0))
            out[..., c] = np.where(background, 0, byte).astype(np.uint8)
        return out


def _soft(entries):
    return api.SoftLightList.make(entries, np.zeros((48, 3), f32))


def bad_lists():
    """(hard lists, soft lists) that rts_trace_light_list* / rts_trace_soft_light_list* refuse; None stands for a NULL list."""
    D = api.Light.DIRECTIONAL
    up = (0.0, 1.0, 0.0)
    empty, nine, kind = api.LightList.make([(D, up)]), api.LightList.make([(D, up)] * 8), api.LightList.make([(D, up), (2, up)])
    empty.count, nine.count = 0, 9
    s_empty, s_nine = _soft([(D, up)]), _soft([(D, up)] * 8)
    s_empty.count, s_nine.count = 0, 9
    soft = [None, s_empty, s_nine, _soft([(2, up)]), _soft([(D, up, 49, 0, 1.0)]), _soft([(D, up, 16, 33, 1.0)]),
            _soft([(D, up, 4, 0, np.inf)]), _soft([(D, up), (D, up, 1, 0, np.nan)])]
    return [None, empty, nine, kind], soft


def runs():
    """(form, list name, with positions, with map, colour set) of every run over a frame; a list with a point light needs positions."""
    out = []
    for form, lists in (("hard", hard_lists()), ("soft", soft_lists())):
        for name, (_, has_point) in lists.items():
            for with_map in (False, True):
                for colours in ("white", "tame", "wild"):
                    out.append((form, name, True, with_map, colours))
            if not has_point:
                out.append((form, name, False, True, "tame"))
    return out


def the_list(form, name):
    return (hard_lists() if form == "hard" else soft_lists())[name][0]
