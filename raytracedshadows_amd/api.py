"""ctypes view of ``librts.so`` (C ABI: ``include/rts.h`` / ``include/rts_scene.h``).

Mirrors the reference's interface for the shadow path:

* :class:`BVHBuilder` -- ``BVHBuilder::build(vertices, stride, indices, primCount)`` with the
  public members ``m_nodes`` / ``m_packedNodes`` (reference ``Source/BVHBuilder.h:27-32``).
* :class:`RayTracingConstants` -- the 64-byte UBO (``Source/RayTracedShadows.h:56-62``).
* :class:`ShadowContext` -- owns the device BVH buffer and issues the dispatch that
  ``RayTracedShadowsApp::renderShadowMaskCompute`` issues (``Source/RayTracedShadows.cpp:570-595``).

No CPU fallback exists here by design: a missing library raises at import, a missing GPU raises
at context creation.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # RTS_LIB lets an experiment load an alternative build of the SAME library (e.g. other compiler flags)
    return os.environ.get("RTS_LIB") or os.path.join(_HERE, "librts.so")


class RtsError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        msg = _lib.rts_status_string(status).decode() if _lib is not None else "?"
        super().__init__(f"{where}: rts status {status} ({msg})")


def _load():
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the shadow path.")
    return C.CDLL(path)


_lib = None
_lib = _load()

_u32p = C.POINTER(C.c_uint32)
_f32p = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)


class RayTracingConstants(C.Structure):
    """``struct RayTracingConstants`` (RayTracedShadows.h:56-62) == UBO ``Constants`` (comp:3-9)."""
    _fields_ = [("cameraPosition", C.c_float * 4), ("cameraDirection", C.c_float * 4),
                ("lightDirection", C.c_float * 4), ("renderTargetSize", C.c_float * 4)]

    @classmethod
    def make(cls, camera_position, light_direction, width, height, camera_direction=(0, 0, -1)):
        k = cls()
        for i in range(3):
            k.cameraPosition[i] = np.float32(camera_position[i])
            k.cameraDirection[i] = np.float32(camera_direction[i])
            k.lightDirection[i] = np.float32(light_direction[i])
        k.renderTargetSize[0] = width
        k.renderTargetSize[1] = height
        k.renderTargetSize[2] = 1.0 / width
        k.renderTargetSize[3] = 1.0 / height
        return k

    def as_array(self):
        return np.frombuffer(bytes(self), dtype=np.float32).copy()


class Light(C.Structure):
    """``rts_light``: directional (the reference) / point light, 1..64 samples."""
    _fields_ = [("type", C.c_uint32), ("nsamples", C.c_uint32), ("xyz", C.c_float * 3),
                ("table", C.c_uint32), ("offsets", (C.c_float * 4) * 64)]
    DIRECTIONAL = 0
    POINT = 1

    @classmethod
    def make(cls, kind, xyz, offsets=None, nsamples=None):
        """offsets: the sample offsets (<= 64).  nsamples < len(offsets): PER-PIXEL jitter -- every pixel takes `nsamples`
        consecutive entries of the table from a start hashed from its index (``rts_light.table``, include/rts.h)."""
        lt = cls()
        lt.type = kind
        for i in range(3):
            lt.xyz[i] = np.float32(xyz[i])
        lt.nsamples = 1
        if offsets is not None:
            offsets = np.asarray(offsets, dtype=np.float32)
            lt.nsamples = offsets.shape[0]
            if nsamples is not None and nsamples != offsets.shape[0]:
                lt.nsamples, lt.table = nsamples, offsets.shape[0]
            for j in range(offsets.shape[0]):
                for i in range(3):
                    lt.offsets[j][i] = offsets[j, i]
        return lt


class LightEntry(C.Structure):
    """``rts_light_entry``: one hard light of a light list (type and xyz as in ``rts_light``, one sample)."""
    _fields_ = [("type", C.c_uint32), ("xyz", C.c_float * 3)]


class LightList(C.Structure):
    """``rts_light_list``: up to 8 hard lights traced in one dispatch, light ``l`` in bit ``l`` of the mask byte."""
    _fields_ = [("count", C.c_uint32), ("reserved_", C.c_uint32 * 3), ("lights", LightEntry * 8)]
    MAX = 8

    @classmethod
    def make(cls, lights):
        """lights: a sequence of ``(kind, xyz)`` pairs, ``Light`` structs (type and xyz are taken, one sample) or ``LightEntry``."""
        lights = list(lights)
        if len(lights) > cls.MAX:
            raise RtsError(1, "LightList.make: at most 8 lights")
        ll = cls()
        ll.count = len(lights)
        for l, item in enumerate(lights):
            kind, xyz = (item.type, item.xyz) if isinstance(item, (Light, LightEntry)) else item
            ll.lights[l].type = kind
            for i in range(3):
                ll.lights[l].xyz[i] = np.float32(xyz[i])
        return ll

    def light(self, l):
        """Light ``l`` alone, as the ``Light`` of the one-light entry points."""
        return Light.make(self.lights[l].type, list(self.lights[l].xyz))


class SoftLightEntry(C.Structure):
    """``rts_soft_light_entry``: one light of a soft light list -- hard (``nsamples`` 0 or 1) or soft (2..48 samples: the entries
    ``first`` .. ``first + nsamples - 1`` of the list's shared offset table, scaled by ``radius``)."""
    _fields_ = [("type", C.c_uint32), ("nsamples", C.c_uint32), ("first", C.c_uint32), ("radius", C.c_float), ("xyz", C.c_float * 3),
                ("reserved_", C.c_uint32)]


class SoftLightList(C.Structure):
    """``rts_soft_light_list``: up to 8 lights, hard or soft, traced in one dispatch, a count plane per light."""
    _fields_ = [("count", C.c_uint32), ("reserved_", C.c_uint32 * 3), ("lights", SoftLightEntry * 8), ("offsets", (C.c_float * 4) * 48)]
    MAX = 8
    OFFSETS = 48

    @classmethod
    def make(cls, lights, offsets=None):
        """lights: a sequence of ``(kind, xyz)`` (a hard light), ``(kind, xyz, nsamples, first, radius)`` or ``SoftLightEntry``.
        offsets: the shared table, at most 48 rows of 3 (or 4) floats; the rows not given are 0."""
        lights = list(lights)
        if len(lights) > cls.MAX:
            raise RtsError(1, "SoftLightList.make: at most 8 lights")
        sl = cls()
        sl.count = len(lights)
        for l, item in enumerate(lights):
            if isinstance(item, SoftLightEntry):
                item = (item.type, list(item.xyz), item.nsamples, item.first, item.radius)
            kind, xyz, nsamples, first, radius = tuple(item) + ((1, 0, 1.0) if len(item) == 2 else ())
            e = sl.lights[l]
            e.type, e.nsamples, e.first, e.radius = kind, nsamples, first, np.float32(radius)
            for i in range(3):
                e.xyz[i] = np.float32(xyz[i])
        if offsets is not None:
            offsets = np.asarray(offsets, dtype=np.float32)
            if offsets.ndim != 2 or offsets.shape[0] > cls.OFFSETS or offsets.shape[1] < 3:
                raise RtsError(1, "SoftLightList.make: offsets is at most 48 rows of 3 floats")
            for j in range(offsets.shape[0]):
                for i in range(3):
                    sl.offsets[j][i] = offsets[j, i]
        return sl

    def light(self, l, table=0):
        """Light ``l`` alone, as the derived ``Light`` of include/rts.h: offsets'[j] = radius * offsets[first + j], the product
        rounded to float32 on its own; a hard entry gives the hard ``Light``.  ``table`` != 0 (a soft entry, ``nsamples <= table <=
        48 - first``): the derived light of a jittered list -- ``table`` scaled offsets and ``Light.table`` set, also where it
        equals ``nsamples``."""
        e = self.lights[l]
        if e.nsamples < 2:
            if table:
                raise RtsError(1, "SoftLightList.light: a hard entry has no table")
            return Light.make(e.type, list(e.xyz))
        if table and (table < e.nsamples or e.first + table > self.OFFSETS):
            raise RtsError(1, "SoftLightList.light: table is 0 or nsamples .. 48 - first")
        rows = np.array([[self.offsets[e.first + j][i] for i in range(3)] for j in range(table or e.nsamples)], dtype=np.float32)
        lt = Light.make(e.type, list(e.xyz), np.float32(e.radius) * rows, nsamples=e.nsamples)
        lt.table = table
        return lt

    def hard_list(self):
        """The ``LightList`` of the same types and positions: what ``facing_lights`` makes this list's light map from."""
        return LightList.make([(self.lights[l].type, list(self.lights[l].xyz)) for l in range(self.count)])


#: the turn of ``AoParams.rotated`` per frame, in radians
GOLDEN_ANGLE = float(np.pi * (3.0 - np.sqrt(5.0)))


class AoParams(C.Structure):
    """``rts_ao_params``: an ambient occlusion trace -- ``nsamples`` segment rays of length ``radius`` per pixel, aimed by the
    tangent-space directions ``dirs`` (x, y in the tangent plane, z along the normal) through the frame around the G-buffer's normal."""
    _fields_ = [("nsamples", C.c_uint32), ("table", C.c_uint32), ("radius", C.c_float), ("reserved_", C.c_uint32),
                ("dirs", (C.c_float * 4) * 64)]
    MAX_SAMPLES = 48
    MAX_DIRS = 64

    @classmethod
    def make(cls, nsamples, radius, table=0, seed=0, dirs=None):
        """``table or nsamples`` cosine-weighted directions with z > 0, stratified (a Latin square over radius and azimuth, one sample
        per row and per column, jittered inside its cell by ``numpy.random.RandomState(seed)``): deterministic, numpy only.
        ``dirs``: the directions to use instead, at most 64 rows of 3 (or 4) floats, any float allowed."""
        ao = cls()
        ao.nsamples, ao.table, ao.radius = int(nsamples), int(table), np.float32(radius)
        if dirs is None:
            m = max(1, min(int(table) if table else int(nsamples), cls.MAX_DIRS))
            rng = np.random.RandomState(seed)
            u = (np.arange(m) + rng.random_sample(m)) / m                 # the fraction of the disc's area inside the sample
            v = (rng.permutation(m) + rng.random_sample(m)) / m           # its azimuth, in turns
            r = np.sqrt(u)
            dirs = np.stack([r * np.cos(2.0 * np.pi * v), r * np.sin(2.0 * np.pi * v), np.sqrt(1.0 - u)], axis=1)
        dirs = np.asarray(dirs, dtype=np.float32)
        if dirs.ndim != 2 or dirs.shape[0] > cls.MAX_DIRS or dirs.shape[1] < 3:
            raise RtsError(1, "AoParams.make: dirs is at most 64 rows of 3 floats")
        for j in range(dirs.shape[0]):
            for i in range(3):
                ao.dirs[j][i] = dirs[j, i]
        return ao

    @property
    def samples(self):
        """The rays per pixel: ``max(1, nsamples)``."""
        return max(1, int(self.nsamples))

    def dirs_array(self):
        """``float32[64, 4]``, a copy."""
        return np.ctypeslib.as_array(self.dirs).reshape(64, 4).astype(np.float32).copy()

    def rotated(self, frame):
        """A copy whose ``dirs`` are turned about the normal (tangent-space z) by ``frame`` times the golden angle, formed in float64
        and rounded once: a frame loop's direction set for frame ``frame`` (``accumulate_bent`` averages them; frame 0 is ``self``)."""
        out = type(self).from_buffer_copy(self)
        if frame:
            d = self.dirs_array().astype(np.float64)
            c, s = np.cos(frame * GOLDEN_ANGLE), np.sin(frame * GOLDEN_ANGLE)
            np.ctypeslib.as_array(out.dirs)[:, :2] = np.stack([c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1]], axis=1)
        return out

    def stand_in_list(self):
        """The one-entry ``SoftLightList`` of the same ``nsamples``: what the filters, the moments pass and the upsample take an AO
        count plane under (they read a count plane and its sample count, and nothing else of a light without ``distances``)."""
        return SoftLightList.make([(Light.POINT, (0.0, 0.0, 0.0), self.samples, 0, 0.0)])


class AoFalloff(C.Structure):
    """``rts_ao_falloff``: the falloff of ``trace_ambient_occlusion_distance`` -- ``weight[b]`` says how open (0: a full occluder,
    255: no occlusion) a sample counts whose nearest blocker lies in the b-th 64th of its segment."""
    _fields_ = [("weight", C.c_uint8 * 64)]

    @classmethod
    def make(cls, curve):
        """``curve``: a callable on [0, 1), evaluated at the 64 bin centres ``(b + 0.5) / 64``, clipped to [0, 1] and rounded to
        0..255; or 64 bytes taken as they are."""
        if callable(curve):
            w = np.rint(np.clip([float(curve((b + 0.5) / 64.0)) for b in range(64)], 0.0, 1.0) * 255.0)
        else:
            w = np.asarray(curve)
            if w.shape != (64,) or (w < 0).any() or (w > 255).any():
                raise RtsError(1, "AoFalloff.make: a callable, or 64 values in 0..255")
        f = cls()
        for b in range(64):
            f.weight[b] = int(w[b])
        return f

    @classmethod
    def zeros(cls):
        """Every blocker a full occluder: the obscurance is the count times S."""
        return cls.make(np.zeros(64, np.uint8))

    @classmethod
    def linear(cls):
        """Occlusion fades linearly to nothing at the end of the segment."""
        return cls.make(lambda t: t)

    @classmethod
    def quadratic(cls):
        """Occlusion ``(1 - t)^2``: it fades faster than linearly."""
        return cls.make(lambda t: 1.0 - (1.0 - t) * (1.0 - t))

    def weights(self):
        """``uint8[64]``, a copy."""
        return np.ctypeslib.as_array(self.weight).astype(np.uint8).copy()


class SkyAmbient(C.Structure):
    """``rtsh_sky_ambient``: the hemispheric sky of ``combine_visibility_list_ao_bent`` -- the ambient light's colour where a pixel's
    bent vector points along ``up`` (``sky``) and against it (``ground``)."""
    _fields_ = [("up", C.c_float * 3), ("sky", C.c_float * 3), ("ground", C.c_float * 3), ("reserved_", C.c_float * 3)]

    @classmethod
    def make(cls, up=(0.0, 1.0, 0.0), sky=(1.0, 1.0, 1.0), ground=(1.0, 1.0, 1.0)):
        """``up`` is used as given: normalise it."""
        s = cls()
        for i in range(3):
            s.up[i], s.sky[i], s.ground[i] = np.float32(up[i]), np.float32(sky[i]), np.float32(ground[i])
        return s


class FilterParams(C.Structure):
    """``rtsh_filter_params``: the window radius (0..8), the two geometry thresholds and, for the distance guide, one spread per light."""
    _fields_ = [("radius", C.c_uint32), ("normal_cos_min", C.c_float), ("plane_eps", C.c_float), ("spread", C.c_float * 8),
                ("reserved_", C.c_uint32 * 5)]
    MAX_RADIUS = 8

    @classmethod
    def make(cls, radius, normal_cos_min=0.9, plane_eps=0.05, spread=None):
        """spread: None (0 for every light), one float for all lights, or up to 8 floats."""
        p = cls()
        p.radius, p.normal_cos_min, p.plane_eps = radius, np.float32(normal_cos_min), np.float32(plane_eps)
        if spread is not None:
            values = np.broadcast_to(np.asarray(spread, np.float32), (8,)) if np.ndim(spread) == 0 else np.asarray(spread, np.float32)
            if values.ndim != 1 or values.shape[0] > 8:
                raise RtsError(1, "FilterParams.make: spread is one float or at most 8")
            for l in range(values.shape[0]):
                p.spread[l] = values[l]
        return p


class WideFilterParams(C.Structure):
    """``rtsh_wide_filter_params``: the number of a-trous passes (0..5; the reach is 2 * (2**passes - 1) pixels) and the two geometry
    thresholds."""
    _fields_ = [("passes", C.c_uint32), ("normal_cos_min", C.c_float), ("plane_eps", C.c_float), ("reserved_", C.c_uint32 * 5)]
    MAX_PASSES = 5

    @classmethod
    def make(cls, passes, normal_cos_min=0.9, plane_eps=0.05):
        p = cls()
        p.passes, p.normal_cos_min, p.plane_eps = passes, np.float32(normal_cos_min), np.float32(plane_eps)
        return p


class UpsampleParams(C.Structure):
    """``rtsh_upsample_params``: the phase of the half-resolution lattice (low-resolution pixel (X, Y) is full-resolution pixel
    (2X + phase_x, 2Y + phase_y)) and the two geometry thresholds of a tap."""
    _fields_ = [("phase_x", C.c_uint32), ("phase_y", C.c_uint32), ("normal_cos_min", C.c_float), ("plane_eps", C.c_float),
                ("reserved_", C.c_uint32 * 4)]

    @classmethod
    def make(cls, phase_x=0, phase_y=0, normal_cos_min=0.9, plane_eps=0.05):
        p = cls()
        p.phase_x, p.phase_y, p.normal_cos_min, p.plane_eps = phase_x, phase_y, np.float32(normal_cos_min), np.float32(plane_eps)
        return p


class WideGuideParams(C.Structure):
    """``rtsh_wide_guide_params``: ``WideFilterParams`` plus ``guide_k4``, the variance guide's tolerance in quarter standard deviations
    (0..255; 12 is k = 3, 0 accepts equal values only)."""
    _fields_ = [("passes", C.c_uint32), ("normal_cos_min", C.c_float), ("plane_eps", C.c_float), ("guide_k4", C.c_uint32),
                ("reserved_", C.c_uint32 * 4)]
    MAX_PASSES = 5
    MAX_K4 = 255

    @classmethod
    def make(cls, passes, guide_k4=12, normal_cos_min=0.9, plane_eps=0.05):
        p = cls()
        p.passes, p.guide_k4, p.normal_cos_min, p.plane_eps = passes, guide_k4, np.float32(normal_cos_min), np.float32(plane_eps)
        return p


class WideGuideTemporalParams(C.Structure):
    """``rtsh_wide_guide_temporal_params``: ``WideGuideParams`` plus ``min_history`` (1..255): a pixel whose count moments hold at
    least that many frames gives the guide its temporal variance, every other pixel this frame's Bernoulli estimate."""
    _fields_ = [("passes", C.c_uint32), ("normal_cos_min", C.c_float), ("plane_eps", C.c_float), ("guide_k4", C.c_uint32),
                ("min_history", C.c_uint32), ("reserved_", C.c_uint32 * 3)]
    MAX_PASSES = 5
    MAX_K4 = 255

    @classmethod
    def make(cls, passes, guide_k4=12, min_history=4, normal_cos_min=0.9, plane_eps=0.05):
        p = cls()
        p.passes, p.guide_k4, p.min_history = passes, guide_k4, min_history
        p.normal_cos_min, p.plane_eps = np.float32(normal_cos_min), np.float32(plane_eps)
        return p


class WideGuidePropagatedParams(C.Structure):
    """``rtsh_wide_guide_propagated_params``: ``WideGuideTemporalParams`` plus ``by_length`` (0 or 1): the temporal variance is divided
    by the history's length before it is carried through the passes."""
    _fields_ = [("passes", C.c_uint32), ("normal_cos_min", C.c_float), ("plane_eps", C.c_float), ("guide_k4", C.c_uint32),
                ("min_history", C.c_uint32), ("by_length", C.c_uint32), ("reserved_", C.c_uint32 * 2)]
    MAX_PASSES = 5
    MAX_K4 = 255

    @classmethod
    def make(cls, passes, guide_k4=12, min_history=4, by_length=0, normal_cos_min=0.9, plane_eps=0.05):
        p = cls()
        p.passes, p.guide_k4, p.min_history, p.by_length = passes, guide_k4, min_history, by_length
        p.normal_cos_min, p.plane_eps = np.float32(normal_cos_min), np.float32(plane_eps)
        return p


class TemporalParams(C.Structure):
    """``rtsh_temporal_params``: the camera motion (current eye minus previous eye, the previous camera's basis and scales), the two
    geometry thresholds, the longest history (1..255) and the lights that take no history this frame (a bit per light)."""
    _fields_ = [("eye_delta", C.c_float * 3), ("prev_right", C.c_float * 3), ("prev_up", C.c_float * 3), ("prev_fwd", C.c_float * 3),
                ("prev_scale_x", C.c_float), ("prev_scale_y", C.c_float), ("normal_cos_min", C.c_float), ("plane_eps", C.c_float),
                ("max_length", C.c_uint32), ("reset_lights", C.c_uint32), ("reserved_", C.c_uint32 * 2)]

    @classmethod
    def make(cls, eye_delta, prev_right, prev_up, prev_fwd, prev_scale_x, prev_scale_y, normal_cos_min=0.9, plane_eps=0.05, max_length=32,
             reset_lights=0):
        p = cls()
        for field, value in (("eye_delta", eye_delta), ("prev_right", prev_right), ("prev_up", prev_up), ("prev_fwd", prev_fwd)):
            getattr(p, field)[:] = [np.float32(v) for v in value]
        p.prev_scale_x, p.prev_scale_y = np.float32(prev_scale_x), np.float32(prev_scale_y)
        p.normal_cos_min, p.plane_eps, p.max_length, p.reset_lights = np.float32(normal_cos_min), np.float32(plane_eps), max_length, reset_lights
        return p

    @classmethod
    def from_cameras(cls, cur, prev, width, height, normal_cos_min=0.9, plane_eps=0.05, max_length=32, reset_lights=0):
        """``cur`` and ``prev``: ``(eye, target, fovy)`` of this frame's and the previous frame's camera.  The numbers are
        ``camera_basis``'s: the ones the G-buffer pass itself used; eye_delta is the float32 difference of the two eyes."""
        c, q = camera_basis(*cur, width, height), camera_basis(*prev, width, height)
        tan_half, aspect = q["tan_half"], q["aspect"]
        return cls.make(c["eye"] - q["eye"], q["right"], q["up"], q["fwd"], np.float32(tan_half * aspect), tan_half, normal_cos_min, plane_eps,
                        max_length, reset_lights)


class HistoryClamp(C.Structure):
    """``rtsh_history_clamp``: the neighbourhood clamp of the temporal accumulation -- a window of (2 * radius + 1)^2 pixels
    (radius 0..4) whose current minimum and maximum, widened by ``margin`` (finite, >= 0), bound the reprojected history."""
    _fields_ = [("radius", C.c_uint32), ("margin", C.c_float), ("reserved_", C.c_uint32 * 2)]

    @classmethod
    def make(cls, radius, margin=0.0):
        c = cls()
        c.radius, c.margin = radius, np.float32(margin)
        return c


class MomentsClamp(C.Structure):
    """``rtsh_moments_clamp``: the neighbourhood clamp of the moments pass -- a window of (2 * radius + 1)^2 pixels (radius 0..4) of
    this frame's V_0 whose [min, max], intersected with mean +- ``sigma_k4``/4 standard deviations (0..255; 36 and above: the range
    alone) and widened by ``margin`` units of V_0 (0..65535), bounds the reprojected tap sums."""
    _fields_ = [("radius", C.c_uint32), ("sigma_k4", C.c_uint32), ("margin", C.c_uint32), ("reserved_", C.c_uint32)]

    @classmethod
    def make(cls, radius, sigma_k4=8, margin=0):
        c = cls()
        c.radius, c.sigma_k4, c.margin = radius, sigma_k4, margin
        return c


#: numpy view of ``struct BVHNode`` (BVHBuilder.h:8-20)
BVHNode_dtype = np.dtype([("bboxMin", np.float32, 3), ("prim", np.uint32),
                          ("bboxMax", np.float32, 3), ("next", np.uint32)])


def _sig(name, restype, *argtypes):
    fn = getattr(_lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


_sig("rts_status_string", C.c_char_p, C.c_int)
_sig("rts_bvh_packed_count", C.c_size_t, C.c_uint32)
_sig("rts_bvh_node_count", C.c_size_t, C.c_uint32)
_sig("rts_bvh_build", C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p)
_sig("rts_bvh_build_ex", C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int,
     C.c_void_p, C.c_size_t, C.c_void_p)
_sig("rts_bvh_validate", C.c_int, C.c_void_p, C.c_size_t, _u32p)
_sig("rts_bvh_build_device", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32,
     C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_float))
_sig("rts_bvh_build_device_ex", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int,
     C.c_uint32, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_float))
_sig("rts_bvh_refit", C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t)
_sig("rts_ctx_refit_bvh_device", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32,
     C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_float))
_sig("rtsh_ctx_read_private_copy", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t))
_sig("rts_device_count", C.c_int, C.POINTER(C.c_int))
_sig("rts_ctx_create", C.c_int, C.c_int, C.POINTER(C.c_void_p))
_sig("rts_ctx_destroy", C.c_int, C.c_void_p)
_sig("rts_ctx_set_bvh", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
_sig("rts_ctx_set_option", C.c_int, C.c_void_p, C.c_char_p, C.c_int)
_sig("rts_ctx_get_option", C.c_int, C.c_void_p, C.c_char_p, C.POINTER(C.c_int))
_sig("rts_trace_shadow_mask", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rts_trace_shadow_mask_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light),
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_shadow_mask_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light),
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_shadow_mask_active", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rts_trace_shadow_mask_active_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_shadow_mask_active_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_rays", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_sig("rts_trace_rays_device", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)
_sig("rts_trace_rays_distance", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_sig("rts_trace_rays_distance_device", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)
_sig("rts_trace_shadow_distance", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_shadow_distance_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rts_trace_shadow_distance_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_rays_distance", C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int)
_sig("rtsh_shadow_distance", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rts_trace_soft_distance", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_soft_distance_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rts_trace_soft_distance_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_soft_distance", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rts_trace_ambient_occlusion", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rts_trace_ambient_occlusion_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_ambient_occlusion_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_ambient_occlusion", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rts_trace_ambient_occlusion_adaptive", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_ambient_occlusion_adaptive_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rts_trace_ambient_occlusion_adaptive_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams),
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
     C.c_void_p)
_sig("rtsh_ambient_occlusion_adaptive", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rts_trace_ambient_occlusion_bent", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_ambient_occlusion_bent_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rts_trace_ambient_occlusion_bent_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams),
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_ambient_occlusion_bent", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rts_trace_ambient_occlusion_distance", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.POINTER(AoFalloff),
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rts_trace_ambient_occlusion_distance_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams),
     C.POINTER(AoFalloff), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p)
_sig("rts_trace_ambient_occlusion_distance_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(AoParams),
     C.POINTER(AoFalloff), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_ambient_occlusion_distance", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(AoParams),
     C.POINTER(AoFalloff), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int)
_sig("rtsh_combine_visibility_list_ao_bent", C.c_int, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SkyAmbient), C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rtsh_combine_visibility_list_ao_bent_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SkyAmbient), C.c_uint32, C.c_uint32, C.c_void_p,
     C.c_void_p)
_sig("rtsh_ao_rays", C.c_int, C.POINTER(RayTracingConstants), C.POINTER(AoParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
     C.c_uint32, C.c_void_p)
_sig("rtsh_combine_visibility_list_ao", C.c_int, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rtsh_combine_visibility_list_ao_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_light_list", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rts_trace_light_list_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(LightList),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_light_list_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(LightList),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_light_list", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rts_trace_soft_light_list", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rts_trace_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_soft_light_list_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_soft_light_list", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rts_trace_soft_light_list_distance", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_soft_light_list_distance_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rts_trace_soft_light_list_distance_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_soft_light_list_distance", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rts_trace_soft_light_list_adaptive", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u32p, C.c_void_p)
_sig("rts_trace_soft_light_list_adaptive_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u32p, C.c_void_p, C.c_void_p)
_sig("rts_trace_soft_light_list_adaptive_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u32p, C.c_void_p, C.c_void_p)
_sig("rtsh_soft_light_list_adaptive", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u32p, C.c_void_p, C.c_int)
_sig("rts_trace_soft_light_list_jittered", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u32p, _u32p, C.c_void_p)
_sig("rts_trace_soft_light_list_jittered_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u32p, _u32p, C.c_void_p, C.c_void_p)
_sig("rts_trace_soft_light_list_jittered_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u32p, _u32p, C.c_void_p, C.c_void_p)
_sig("rtsh_soft_light_list_jittered", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, _u32p, _u32p, C.c_void_p, C.c_int)
_sig("rts_trace_shadow_mask_adaptive", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_shadow_mask_adaptive_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rts_trace_shadow_mask_adaptive_stripes_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light),
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_shadow_mask_adaptive", C.c_int, C.c_void_p, C.c_size_t, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rtsh_facing_lights", C.c_int, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
     C.c_void_p)
_sig("rtsh_facing_lights_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_light_list_sparse", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p)
_sig("rts_trace_light_list_sparse_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rts_trace_soft_light_list_sparse", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p)
_sig("rts_trace_soft_light_list_sparse_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_compact_scratch_bytes", C.c_size_t, C.c_uint32, C.c_uint32)
_sig("rtsh_compact_nodes", C.c_int)
_sig("rtsh_compact_light_map", C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, _u32p)
_sig("rtsh_compact_light_map_device", C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
     C.c_void_p, C.c_void_p)
COMPACT_NODES = int(_lib.rtsh_compact_nodes())      # kernel nodes of compact_light_map_device under graph capture (rts_scene.h)
_sig("rts_device_malloc", C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t)
_sig("rts_device_free", C.c_int, C.c_void_p, C.c_void_p)
_sig("rts_memcpy_h2d", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
_sig("rts_memcpy_d2h", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
_sig("rts_stream_synchronize", C.c_int, C.c_void_p, C.c_void_p)
_sig("rts_timer_begin", C.c_int, C.c_void_p, C.c_void_p)
_sig("rts_timer_end", C.c_int, C.c_void_p, C.c_void_p)
_sig("rts_timer_elapsed_ms", C.c_int, C.c_void_p, C.POINTER(C.c_float))
_sig("rts_ctx_last_kernel_name", C.c_char_p, C.c_void_p)
_sig("rts_ctx_set_tile_order", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
_sig("rts_ctx_read_wave_stats", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
_sig("rts_ctx_read_wave_realtime", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
_sig("rts_ctx_read_clock_probe", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
_sig("rts_stream_create", C.c_int, C.c_void_p, C.POINTER(C.c_void_p))
_sig("rts_stream_destroy", C.c_int, C.c_void_p, C.c_void_p)
_sig("rts_ctx_autotune", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
     C.POINTER(C.c_int), C.POINTER(C.c_float))


def split_front_order(life_us, tiles, first_record=0, xcd_square=0, life_block=0):
    """rtsh_split_front_order: the planner's front order (host logic, no device): indices of the tiles in record order."""
    life = np.ascontiguousarray(life_us, np.float32)
    t = np.ascontiguousarray(tiles, np.uint32)
    out = np.zeros(t.size, np.uint32)
    _check(_lib.rtsh_split_front_order(_ptr(life), _ptr(t), t.size, first_record, xcd_square, life_block, _ptr(out)), "rtsh_split_front_order")
    return out


_sig("rtsh_follow_order", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rts_ctx_read_follow", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)


def follow_order(life_ticks, blocks_x, blocks_y, first_record=0, xcd_square=0, life_block=1):
    """rtsh_follow_order: follow mode's order on the host (no device) -- row-major tile ids in record order."""
    life = np.ascontiguousarray(life_ticks, np.uint32).ravel()
    if life.size != blocks_x * blocks_y:
        raise RtsError(1, "follow_order: life_ticks must hold blocks_x * blocks_y entries")
    out = np.zeros(life.size, np.uint32)
    _check(_lib.rtsh_follow_order(_ptr(life), blocks_x, blocks_y, first_record, xcd_square, life_block, _ptr(out)), "rtsh_follow_order")
    return out


_sig("rtsh_follow_plan_device", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)


def follow_plan_device(ctx, life_ticks, blocks_x, blocks_y, xcd_square=0, life_block=1, start_ticks=None):
    """rtsh_follow_plan_device: follow mode's device planner run on the given lives (and start stamps) -- row-major tile ids in
    record order, as follow_order returns them."""
    life = np.ascontiguousarray(life_ticks, np.uint32).ravel()
    if life.size != blocks_x * blocks_y:
        raise RtsError(1, "follow_plan_device: life_ticks must hold blocks_x * blocks_y entries")
    start = None
    if start_ticks is not None:
        start = np.ascontiguousarray(start_ticks, np.uint32).ravel()
        if start.size != life.size:
            raise RtsError(1, "follow_plan_device: start_ticks must hold blocks_x * blocks_y entries")
    out = np.zeros(life.size, np.uint32)
    _check(_lib.rtsh_follow_plan_device(ctx.handle, _ptr(life), _ptr(start) if start is not None else None, blocks_x, blocks_y,
                                        xcd_square, life_block, _ptr(out)), "rtsh_follow_plan_device")
    return (out & 0xFFFF) + (out >> 16) * np.uint32(blocks_x)


def stripe_rows(height, band_rows, n_stripes, stripe):
    """rtsh_stripe_rows: the virtual rows of one interleaved stripe's dispatch (host logic, no device) -- band_rows x the
    bands the stripe owns, 0 for a stripe without a band."""
    rows = C.c_uint32(0)
    _check(_lib.rtsh_stripe_rows(height, band_rows, n_stripes, stripe, C.byref(rows)), "rtsh_stripe_rows")
    return int(rows.value)


class SplitPlan(C.Structure):
    """rts_split_plan (include/rts.h)."""
    _fields_ = [("min_life_us", C.c_float), ("end_after_us", C.c_float), ("piece_us", C.c_float), ("front_life_us", C.c_float), ("front_share", C.c_float), ("max_pieces", C.c_uint32), ("max_tiles", C.c_uint32),
                ("xcd_square", C.c_uint32), ("life_block", C.c_uint32), ("reserved_", C.c_uint32), ("prev_stats", C.c_void_p), ("prev_realtime", C.c_void_p), ("prev_waves", C.c_size_t)]


_sig("rts_ctx_plan_splits", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_uint32, C.c_uint32,
     C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(SplitPlan), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
_sig("rts_ctx_plan_splits_stripes", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_uint32,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(SplitPlan), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
_sig("rts_ctx_clear_splits", C.c_int, C.c_void_p)
_sig("rts_ctx_plan_tile_order", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_uint32, C.c_uint32,
     C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32))
_sig("rtsh_split_front_order", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rtsh_stripe_rows", C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32))
_sig("rts_selftest_reciprocal", C.c_int, C.c_void_p, C.c_void_p)
_sig("rts_ctx_get_split_plan", C.c_int, C.c_void_p, C.POINTER(SplitPlan))
_sig("rts_ctx_autotune_stripes", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
     C.c_uint32, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float))
_sig("rts_ctx_read_piece_stats", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
_sig("rts_timer_mark", C.c_int, C.c_void_p, C.c_void_p, C.c_uint32)
_sig("rts_timer_between_ms", C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float))
_sig("rts_device_mem_info", C.c_int, C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t))
_sig("rtsh_primary_positions", C.c_int, C.c_void_p, C.c_size_t, _f32p, _f32p, C.c_float, C.c_uint32, C.c_uint32,
     C.c_void_p, C.POINTER(C.c_uint64), C.c_int)
_sig("rtsh_primary_gbuffer", C.c_int, C.c_void_p, C.c_size_t, _f32p, _f32p, C.c_float, C.c_uint32, C.c_uint32,
     C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_int)
_sig("rtsh_primary_gbuffer_device", C.c_int, C.c_void_p, _f32p, _f32p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p,
     C.c_void_p, C.c_void_p)
_sig("rtsh_combine_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_combine", C.c_int, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rtsh_combine_light_list", C.c_int, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rtsh_combine_soft_light_list", C.c_int, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rtsh_combine_light_list_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_combine_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(SoftLightList), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_filter_light_list", C.c_int, C.POINTER(LightList), C.POINTER(FilterParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_filter_soft_light_list", C.c_int, C.POINTER(SoftLightList), C.POINTER(FilterParams), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_filter_light_list_device", C.c_int, C.c_void_p, C.POINTER(LightList), C.POINTER(FilterParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_filter_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList), C.POINTER(FilterParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_subsampled_size", C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
_sig("rtsh_subsample_gbuffer", C.c_int, C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
     C.c_void_p, C.c_void_p)
_sig("rtsh_subsample_gbuffer_device", C.c_int, C.c_void_p, C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_upsample_retrace_map", C.c_int, C.c_uint32, C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_upsample_retrace_map_device", C.c_int, C.c_void_p, C.c_uint32, C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_upsample_light_list", C.c_int, C.POINTER(LightList), C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_upsample_soft_light_list", C.c_int, C.POINTER(SoftLightList), C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_upsample_light_list_device", C.c_int, C.c_void_p, C.POINTER(LightList), C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_upsample_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList), C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_wide_filter_scratch_bytes", C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32)
_sig("rtsh_wide_filter_light_list", C.c_int, C.POINTER(LightList), C.POINTER(WideFilterParams), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_wide_filter_soft_light_list", C.c_int, C.POINTER(SoftLightList), C.POINTER(WideFilterParams), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_wide_filter_light_list_device", C.c_int, C.c_void_p, C.POINTER(LightList), C.POINTER(WideFilterParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_wide_filter_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList), C.POINTER(WideFilterParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_wide_filter_bent_scratch_bytes", C.c_size_t, C.c_uint32, C.c_uint32)
_sig("rtsh_wide_filter_bent", C.c_int, C.POINTER(WideFilterParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
     C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rtsh_wide_filter_bent_device", C.c_int, C.c_void_p, C.POINTER(WideFilterParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_accumulate_bent", C.c_int, C.POINTER(TemporalParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rtsh_accumulate_bent_device", C.c_int, C.c_void_p, C.POINTER(TemporalParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_accumulate_bent_motion", C.c_int, C.POINTER(TemporalParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rtsh_accumulate_bent_motion_device", C.c_int, C.c_void_p, C.POINTER(TemporalParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
     C.c_void_p)
_sig("rtsh_wide_filter_bent_mean", C.c_int, C.POINTER(WideFilterParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rtsh_wide_filter_bent_mean_device", C.c_int, C.c_void_p, C.POINTER(WideFilterParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_wide_filter_guided_scratch_bytes", C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32)
_sig("rtsh_wide_guide_threshold", C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32)
_sig("rtsh_wide_filter_guided_soft_light_list", C.c_int, C.POINTER(SoftLightList), C.POINTER(WideGuideParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_wide_filter_guided_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList), C.POINTER(WideGuideParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_combine_visibility_list", C.c_int, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rtsh_combine_visibility_list_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(LightList), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_camera_basis", C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p)
_sig("rtsh_accumulate_visibility_list", C.c_int, C.POINTER(LightList), C.POINTER(TemporalParams), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int)
_sig("rtsh_accumulate_visibility_list_device", C.c_int, C.c_void_p, C.POINTER(LightList), C.POINTER(TemporalParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_accumulate_visibility_list_clamped", C.c_int, C.POINTER(LightList), C.POINTER(TemporalParams), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(HistoryClamp),
     C.c_int)
_sig("rtsh_accumulate_visibility_list_clamped_device", C.c_int, C.c_void_p, C.POINTER(LightList), C.POINTER(TemporalParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
     C.POINTER(HistoryClamp), C.c_void_p)
_sig("rtsh_accumulate_moments_soft_light_list", C.c_int, C.POINTER(SoftLightList), C.POINTER(TemporalParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_int)
_sig("rtsh_accumulate_moments_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList), C.POINTER(TemporalParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_primary_gbuffer_motion", C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, _f32p, _f32p, _f32p, C.c_float, C.c_uint32,
     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_int)
_sig("rtsh_primary_gbuffer_motion_device", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, _f32p, _f32p, _f32p, C.c_float, C.c_uint32,
     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_ctx_snapshot_bvh_device", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_sig("rtsh_ctx_bvh_count", C.c_size_t, C.c_void_p)
_sig("rtsh_accumulate_visibility_list_motion", C.c_int, C.POINTER(LightList), C.POINTER(TemporalParams), C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
     C.c_int)
_sig("rtsh_accumulate_visibility_list_motion_device", C.c_int, C.c_void_p, C.POINTER(LightList), C.POINTER(TemporalParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
     C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_accumulate_visibility_list_clamped_motion", C.c_int, C.POINTER(LightList), C.POINTER(TemporalParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
     C.c_void_p, C.POINTER(HistoryClamp), C.c_int)
_sig("rtsh_accumulate_visibility_list_clamped_motion_device", C.c_int, C.c_void_p, C.POINTER(LightList), C.POINTER(TemporalParams),
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
     C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(HistoryClamp), C.c_void_p)
_sig("rtsh_accumulate_moments_soft_light_list_motion", C.c_int, C.POINTER(SoftLightList), C.POINTER(TemporalParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
_sig("rtsh_accumulate_moments_soft_light_list_motion_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList), C.POINTER(TemporalParams),
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_moments_clamp_bounds", None, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
_sig("rtsh_accumulate_moments_soft_light_list_clamped", C.c_int, C.POINTER(SoftLightList), C.POINTER(TemporalParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
     C.c_void_p, C.POINTER(MomentsClamp), C.c_int)
_sig("rtsh_accumulate_moments_soft_light_list_clamped_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList), C.POINTER(TemporalParams),
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MomentsClamp), C.c_void_p)
_sig("rtsh_accumulate_moments_soft_light_list_clamped_motion", C.c_int, C.POINTER(SoftLightList), C.POINTER(TemporalParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MomentsClamp), C.c_int)
_sig("rtsh_accumulate_moments_soft_light_list_clamped_motion_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList),
     C.POINTER(TemporalParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(MomentsClamp), C.c_void_p)
_sig("rtsh_wide_filter_guided_temporal_soft_light_list", C.c_int, C.POINTER(SoftLightList), C.POINTER(WideGuideTemporalParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_wide_filter_guided_temporal_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList),
     C.POINTER(WideGuideTemporalParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_wide_filter_mean_soft_light_list", C.c_int, C.POINTER(SoftLightList), C.POINTER(WideFilterParams), C.c_void_p, C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_wide_filter_mean_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList), C.POINTER(WideFilterParams), C.c_void_p,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_wide_filter_guided_temporal_mean_soft_light_list", C.c_int, C.POINTER(SoftLightList), C.POINTER(WideGuideTemporalParams),
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_wide_filter_guided_temporal_mean_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList),
     C.POINTER(WideGuideTemporalParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_wide_filter_propagated_scratch_bytes", C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32)
_sig("rtsh_wide_variance_step", C.c_uint32, C.c_uint64, C.c_uint32)
_sig("rtsh_wide_filter_propagated_mean_soft_light_list", C.c_int, C.POINTER(SoftLightList), C.POINTER(WideGuidePropagatedParams),
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int)
_sig("rtsh_wide_filter_propagated_mean_soft_light_list_device", C.c_int, C.c_void_p, C.POINTER(SoftLightList),
     C.POINTER(WideGuidePropagatedParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
     C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p)
_sig("rtsh_facing_active", C.c_int, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
     C.c_void_p)
_sig("rtsh_facing_active_device", C.c_int, C.c_void_p, C.POINTER(RayTracingConstants), C.POINTER(Light), C.c_void_p, C.c_void_p,
     C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
_sig("rtsh_obj_load", C.c_int, C.c_char_p, C.c_void_p, C.c_size_t, _u32p, _f32p, _f32p)
_sig("rtsh_obj_parse_float", C.c_float, C.c_char_p, C.POINTER(C.c_int))


def _check(status, where):
    if status != 0:
        raise RtsError(status, where)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ptr_or_none(a):
    return _ptr(a) if a is not None else None


def _ref(struct):
    """``byref(struct)``, or None (a NULL pointer) for None."""
    return C.byref(struct) if struct is not None else None


def _frame_inputs(where, positions, width, height, per_pixel=None, map_name="active"):
    """The positions of a frame and its optional per-pixel byte map, contiguous and of the frame's size."""
    positions = np.ascontiguousarray(positions, dtype=np.float32)
    if positions.size != width * height * 4:
        raise RtsError(1, f"{where}: positions must be W*H*4 floats")
    if per_pixel is not None:
        per_pixel = np.ascontiguousarray(per_pixel, dtype=np.uint8)
        if per_pixel.size != width * height:
            raise RtsError(1, f"{where}: {map_name} must be W*H bytes")
    return positions, per_pixel


def packed_count(prim_count):
    """``m_packedNodes.size()`` for ``prim_count`` triangles (= 5P-2)."""
    return int(_lib.rts_bvh_packed_count(prim_count))


def bvh_validate(packed):
    packed = np.ascontiguousarray(packed, dtype=np.uint32).reshape(-1, 4)
    p = C.c_uint32(0)
    _check(_lib.rts_bvh_validate(_ptr(packed), packed.shape[0], C.byref(p)), "rts_bvh_validate")
    return int(p.value)


def device_count():
    n = C.c_int(0)
    _lib.rts_device_count(C.byref(n))
    return int(n.value)


class BVHBuilder:
    """Same surface as the reference's ``struct BVHBuilder`` (Source/BVHBuilder.h:27-32).

    ``m_nodes``: structured array of ``BVHNode`` (2P-1), ``m_packedNodes``: ``uint32[5P-2, 4]``
    (one row per ``BVHPackedNode`` / GLSL ``vec4``).
    """

    def __init__(self, sah_prim_limit=1000000, threads=0):
        self.m_nodes = np.zeros(0, dtype=BVHNode_dtype)
        self.m_packedNodes = np.zeros((0, 4), dtype=np.uint32)
        self.sah_prim_limit = sah_prim_limit
        self.threads = threads

    def build(self, vertices, stride, indices, primCount):
        """``stride`` is in floats, exactly like the reference (it passes 8)."""
        vertices = np.ascontiguousarray(vertices, dtype=np.float32)
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        if primCount > 0:
            if indices.size < 3 * primCount:
                raise RtsError(1, "BVHBuilder.build: indices shorter than 3*primCount")
            if vertices.size < (int(indices[:3 * primCount].max()) * stride + 3):
                raise RtsError(1, "BVHBuilder.build: index out of range of the vertex array")
        n = packed_count(primCount)
        packed = np.zeros((max(n, 1), 4), dtype=np.uint32)
        nodes = np.zeros(max(2 * primCount - 1, 1), dtype=BVHNode_dtype)
        st = _lib.rts_bvh_build_ex(_ptr(vertices), stride, _ptr(indices), primCount, self.sah_prim_limit,
                                   self.threads, _ptr(packed), packed.shape[0], _ptr(nodes))
        _check(st, "rts_bvh_build")
        self.m_packedNodes = packed[:n]
        self.m_nodes = nodes[:2 * primCount - 1]
        return self


def _geometry(vertices, stride, indices, prim_count):
    """The geometry arguments of the device entries: ``vertices`` an array or ``(device pointer, number of floats)``,
    ``indices`` an array or a device pointer.  Returns (vertex pointer, number of floats, index pointer, arrays to keep alive)."""
    import numbers

    def device_pointer(v):                           # a plain or numpy integer, or a ctypes pointer value
        if isinstance(v, C.c_void_p):
            v = v.value
        if isinstance(v, numbers.Integral) and not isinstance(v, bool) and int(v) > 0:
            return int(v)
        return None

    if isinstance(vertices, tuple):                  # (device pointer, number of floats): geometry already on the device
        if len(vertices) != 2 or device_pointer(vertices[0]) is None or int(vertices[1]) < 3 * stride:
            raise ValueError("vertices: expected (device pointer, number of floats >= 3 * stride)")
        v_ptr, v_floats = C.c_void_p(device_pointer(vertices[0])), int(vertices[1])
    else:
        vertices = np.ascontiguousarray(vertices, dtype=np.float32)
        if vertices.ndim == 0 or vertices.size < 3 * stride:
            raise ValueError("vertices: an array of at least one triangle's floats is required")
        v_ptr, v_floats = _ptr(vertices), vertices.size
    if device_pointer(indices) is not None:
        i_ptr = C.c_void_p(device_pointer(indices))
    else:
        indices = np.ascontiguousarray(indices, dtype=np.uint32)
        if indices.ndim == 0 or indices.size < 3 * prim_count:       # C reads 3 * prim_count words from this array
            raise ValueError(f"indices: {indices.size} entries for {prim_count} triangles")
        i_ptr = _ptr(indices)
    return v_ptr, v_floats, i_ptr, (vertices, indices)


def bvh_build_device(ctx, vertices, stride, indices, prim_count, install=False, want_packed=True, algorithm="sah",
                     radius=0):
    """BVH build on the GPU.  "sah" (default): BVHBuilder's own split rule for every node, level by level on the device
    -- ``radius`` is then the range size above which the median split is used, 0 = the reference's 1 000 000.  Over the
    Morton order: "ploc" (locally-ordered clustering, ``radius`` neighbours each way, 0 = 16), "lbvh" (Karras hierarchy),
    "ploc_sah" (PLOC below 65 536 clusters, full-sweep SAH over the clusters on the host above).
    ``vertices`` may be ``(device pointer, number of floats)`` and ``indices`` a device pointer: geometry that already lives on
    the context's device is used in place.  Returns (packed or None, device milliseconds)."""
    v_ptr, v_floats, i_ptr, _keep = _geometry(vertices, stride, indices, prim_count)
    n = packed_count(prim_count)
    packed = np.zeros((max(n, 1), 4), dtype=np.uint32) if want_packed else None
    ms = C.c_float(0)
    algo = {"lbvh": 0, "ploc": 1, "ploc_sah": 2, "sah": 3}[algorithm]
    _check(_lib.rts_bvh_build_device_ex(ctx.handle, v_ptr, v_floats, stride, i_ptr, prim_count,
                                        algo, radius, _ptr(packed) if want_packed else None, n if want_packed else 0,
                                        int(install), C.byref(ms)), "rts_bvh_build_device_ex")
    return (packed[:n] if want_packed else None), float(ms.value)


def bvh_refit(packed, vertices, stride, indices, prim_count):
    """rts_bvh_refit on the host: a new array holding ``packed``'s topology with boxes and leaf data recomputed from the new
    vertices (include/rts.h).  Host arrays only: ``(device pointer, floats)`` geometry raises ValueError --
    the device form is :func:`bvh_refit_device`."""
    v_ptr, v_floats, i_ptr, _keep = _geometry(vertices, stride, indices, prim_count)
    if isinstance(vertices, tuple) or not isinstance(_keep[1], np.ndarray):
        raise ValueError("bvh_refit is the host form: vertices and indices must be host arrays (see bvh_refit_device)")
    out = np.array(np.asarray(packed, dtype=np.uint32).reshape(-1, 4), dtype=np.uint32, order="C")
    _check(_lib.rts_bvh_refit(v_ptr, v_floats, stride, i_ptr, prim_count, _ptr(out), out.shape[0]), "rts_bvh_refit")
    return out


def bvh_refit_device(ctx, vertices, stride, indices, prim_count, want_packed=False):
    """rts_ctx_refit_bvh_device: the context's installed stream refitted in place on the device (geometry as in
    :func:`bvh_build_device`).  Returns (packed or None, device milliseconds, cost_ratio)."""
    v_ptr, v_floats, i_ptr, _keep = _geometry(vertices, stride, indices, prim_count)
    n = packed_count(prim_count)
    packed = np.zeros((max(n, 1), 4), dtype=np.uint32) if want_packed else None
    ms, ratio = C.c_float(0), C.c_float(0)
    _check(_lib.rts_ctx_refit_bvh_device(ctx.handle, v_ptr, v_floats, stride, i_ptr, prim_count,
                                         _ptr(packed) if want_packed else None, n if want_packed else 0,
                                         C.byref(ms), C.byref(ratio)), "rts_ctx_refit_bvh_device")
    return (packed[:n] if want_packed else None), float(ms.value), float(ratio.value)


def read_private_copy(ctx):
    """rtsh_ctx_read_private_copy (diagnostics): the private copy of kernel 8 as bytes -- wide nodes, triangle records,
    parents -- or an empty array when the stream has none."""
    size = C.c_size_t(0)
    _check(_lib.rtsh_ctx_read_private_copy(ctx.handle, None, 0, C.byref(size)), "rtsh_ctx_read_private_copy")
    out = np.zeros(size.value, np.uint8)
    if size.value:
        _check(_lib.rtsh_ctx_read_private_copy(ctx.handle, _ptr(out), out.size, C.byref(size)), "rtsh_ctx_read_private_copy")
    return out


class ShadowContext:
    """Device-side half of the path: BVH storage buffer + the shadow dispatch."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(_lib.rts_ctx_create(device, C.byref(h)), "rts_ctx_create")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            _lib.rts_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    def set_bvh(self, packed):
        packed = np.ascontiguousarray(packed, dtype=np.uint32).reshape(-1, 4)
        _check(_lib.rts_ctx_set_bvh(self._h, _ptr(packed), packed.shape[0]), "rts_ctx_set_bvh")

    def set_option(self, key, value):
        _check(_lib.rts_ctx_set_option(self._h, key.encode(), int(value)), f"rts_ctx_set_option({key})")

    def get_option(self, key):
        v = C.c_int(0)
        _check(_lib.rts_ctx_get_option(self._h, key.encode(), C.byref(v)), f"rts_ctx_get_option({key})")
        return int(v.value)

    def trace_shadow_mask(self, constants, positions, width, height, light=None, row_begin=0, row_end=None,
                          out=None, active=None):
        """Host-pointer dispatch; returns the ``uint8[H, W]`` mask (1 = lit).  ``active``: an active map, ``uint8[H, W]``
        (non-zero = trace the pixel, zero = send no ray and write 0; include/rts.h), or None for every pixel."""
        positions, active = _frame_inputs("trace_shadow_mask", positions, width, height, active)
        row_end = height if row_end is None else row_end
        mask = out if out is not None else np.zeros((height, width), dtype=np.uint8)
        if active is not None:
            _check(_lib.rts_trace_shadow_mask_active(self._h, C.byref(constants), _ref(light), _ptr(positions), _ptr(active),
                                                     width, height, row_begin, row_end, _ptr(mask)), "rts_trace_shadow_mask_active")
            return mask
        _check(_lib.rts_trace_shadow_mask(self._h, C.byref(constants), _ref(light), _ptr(positions), width, height,
                                          row_begin, row_end, _ptr(mask)), "rts_trace_shadow_mask")
        return mask

    def trace_shadow_mask_device(self, constants, d_positions, width, height, d_mask, light=None, row_begin=0,
                                 row_end=None, stream=None, d_active=None):
        """``d_active``: device pointer of an active map (width * height bytes), or None for every pixel."""
        row_end = height if row_end is None else row_end
        if d_active is not None:
            _check(_lib.rts_trace_shadow_mask_active_device(self._h, C.byref(constants), _ref(light), C.c_void_p(d_positions),
                                                            C.c_void_p(d_active), width, height, row_begin, row_end,
                                                            C.c_void_p(d_mask), C.c_void_p(stream or 0)),
                   "rts_trace_shadow_mask_active_device")
            return
        _check(_lib.rts_trace_shadow_mask_device(self._h, C.byref(constants), _ref(light), C.c_void_p(d_positions), width,
                                                 height, row_begin, row_end, C.c_void_p(d_mask),
                                                 C.c_void_p(stream or 0)), "rts_trace_shadow_mask_device")

    def trace_shadow_mask_stripes_device(self, constants, d_positions, width, height, d_mask, band_rows, n_stripes,
                                         stripe, light=None, stream=None, d_active=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        if d_active is not None:
            _check(_lib.rts_trace_shadow_mask_active_stripes_device(self._h, C.byref(constants), _ref(light),
                                                                    C.c_void_p(d_positions), C.c_void_p(d_active), width, height,
                                                                    band_rows, n_stripes, stripe, C.c_void_p(d_mask),
                                                                    C.c_void_p(stream or 0)),
                   "rts_trace_shadow_mask_active_stripes_device")
            return
        _check(_lib.rts_trace_shadow_mask_stripes_device(self._h, C.byref(constants), _ref(light), C.c_void_p(d_positions),
                                                         width, height, band_rows, n_stripes, stripe,
                                                         C.c_void_p(d_mask), C.c_void_p(stream or 0)),
               "rts_trace_shadow_mask_stripes_device")

    def trace_rays(self, rays):
        """``rays``: float32[n, 8] = {o.xyz, tmax, d.xyz, 0}; returns uint8[n] (1 = not occluded)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], dtype=np.uint8)
        _check(_lib.rts_trace_rays(self._h, _ptr(rays), rays.shape[0], _ptr(out)), "rts_trace_rays")
        return out

    def trace_rays_device(self, d_rays, n, d_out, stream=None):
        """Device-pointer form of :meth:`trace_rays` (asynchronous on ``stream``)."""
        _check(_lib.rts_trace_rays_device(self._h, C.c_void_p(d_rays), n, C.c_void_p(d_out), C.c_void_p(stream or 0)),
               "rts_trace_rays_device")

    # -- occluder distance (include/rts.h): the nearest accepted triangle's ray parameter, +Inf where the ray is lit ----------
    def trace_rays_distance(self, rays):
        """``rays``: float32[n, 8] = {o.xyz, tmax, d.xyz, 0}; returns float32[n]."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], dtype=np.float32)
        _check(_lib.rts_trace_rays_distance(self._h, _ptr(rays), rays.shape[0], _ptr(out)), "rts_trace_rays_distance")
        return out

    def trace_rays_distance_device(self, d_rays, n, d_out_t, stream=None):
        """Device-pointer form of :meth:`trace_rays_distance` (asynchronous on ``stream``); d_out_t = n floats."""
        _check(_lib.rts_trace_rays_distance_device(self._h, C.c_void_p(d_rays), n, C.c_void_p(d_out_t), C.c_void_p(stream or 0)),
               "rts_trace_rays_distance_device")

    def trace_shadow_distance(self, constants, positions, width, height, light=None, row_begin=0, row_end=None, active=None,
                              out=None, mask=None, want_mask=True):
        """Host-pointer dispatch; returns ``(float32[H, W] distance, uint8[H, W] mask)`` (mask None with ``want_mask`` False).
        ``out`` / ``mask``: arrays to write into (rows outside the range keep their contents)."""
        positions, active = _frame_inputs("trace_shadow_distance", positions, width, height, active)
        row_end = height if row_end is None else row_end
        dist = out if out is not None else np.zeros((height, width), dtype=np.float32)
        if mask is None and want_mask:
            mask = np.zeros((height, width), dtype=np.uint8)
        _check(_lib.rts_trace_shadow_distance(self._h, C.byref(constants), _ref(light), _ptr(positions), _ptr_or_none(active),
                                              width, height, row_begin, row_end, _ptr(dist), _ptr_or_none(mask)),
               "rts_trace_shadow_distance")
        return dist, mask

    def trace_shadow_distance_device(self, constants, d_positions, width, height, d_distance, d_mask=None, light=None, row_begin=0,
                                     row_end=None, stream=None, d_active=None):
        """Device pointers, asynchronous: d_distance = width * height floats, d_mask / d_active = width * height bytes or None."""
        row_end = height if row_end is None else row_end
        _check(_lib.rts_trace_shadow_distance_device(self._h, C.byref(constants), _ref(light), C.c_void_p(d_positions),
                                                     C.c_void_p(d_active or 0), width, height, row_begin, row_end,
                                                     C.c_void_p(d_distance), C.c_void_p(d_mask or 0), C.c_void_p(stream or 0)),
               "rts_trace_shadow_distance_device")

    def trace_shadow_distance_stripes_device(self, constants, d_positions, width, height, d_distance, band_rows, n_stripes, stripe,
                                             d_mask=None, light=None, stream=None, d_active=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        _check(_lib.rts_trace_shadow_distance_stripes_device(self._h, C.byref(constants), _ref(light), C.c_void_p(d_positions),
                                                             C.c_void_p(d_active or 0), width, height, band_rows, n_stripes, stripe,
                                                             C.c_void_p(d_distance), C.c_void_p(d_mask or 0), C.c_void_p(stream or 0)),
               "rts_trace_shadow_distance_stripes_device")

    # -- soft-shadow occluder distance (include/rts.h): the nearest blocker over all light samples, and the count of unoccluded ones --
    def trace_soft_distance(self, constants, positions, width, height, light=None, row_begin=0, row_end=None, active=None,
                            out=None, mask=None, want_mask=True):
        """Host-pointer dispatch; returns ``(float32[H, W] distance, uint8[H, W] mask)`` (mask None with ``want_mask`` False):
        the minimum of the samples' distances and the number of unoccluded samples.  ``out`` / ``mask``: arrays to write into."""
        positions, active = _frame_inputs("trace_soft_distance", positions, width, height, active)
        row_end = height if row_end is None else row_end
        dist = out if out is not None else np.zeros((height, width), dtype=np.float32)
        if mask is None and want_mask:
            mask = np.zeros((height, width), dtype=np.uint8)
        _check(_lib.rts_trace_soft_distance(self._h, C.byref(constants), _ref(light), _ptr(positions), _ptr_or_none(active),
                                            width, height, row_begin, row_end, _ptr(dist), _ptr_or_none(mask)),
               "rts_trace_soft_distance")
        return dist, mask

    def trace_soft_distance_device(self, constants, d_positions, width, height, d_distance, d_mask=None, light=None, row_begin=0,
                                   row_end=None, stream=None, d_active=None):
        """Device pointers, asynchronous: d_distance = width * height floats, d_mask / d_active = width * height bytes or None."""
        row_end = height if row_end is None else row_end
        _check(_lib.rts_trace_soft_distance_device(self._h, C.byref(constants), _ref(light), C.c_void_p(d_positions),
                                                   C.c_void_p(d_active or 0), width, height, row_begin, row_end,
                                                   C.c_void_p(d_distance), C.c_void_p(d_mask or 0), C.c_void_p(stream or 0)),
               "rts_trace_soft_distance_device")

    def trace_soft_distance_stripes_device(self, constants, d_positions, width, height, d_distance, band_rows, n_stripes, stripe,
                                           d_mask=None, light=None, stream=None, d_active=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        _check(_lib.rts_trace_soft_distance_stripes_device(self._h, C.byref(constants), _ref(light), C.c_void_p(d_positions),
                                                           C.c_void_p(d_active or 0), width, height, band_rows, n_stripes, stripe,
                                                           C.c_void_p(d_distance), C.c_void_p(d_mask or 0), C.c_void_p(stream or 0)),
               "rts_trace_soft_distance_stripes_device")

    # -- ambient occlusion (include/rts.h): hemisphere segments around the normal, the unoccluded ones counted --
    def trace_ambient_occlusion(self, constants, ao, positions, normals, width, height, row_begin=0, row_end=None, active=None, out=None):
        """Host-pointer dispatch; returns ``uint8[H, W]`` counts of unoccluded samples (0 on the background and where ``active`` is 0).
        ``out``: an array to write into (rows outside the range keep their contents)."""
        positions, active = _frame_inputs("trace_ambient_occlusion", positions, width, height, active)
        normals, _ = _frame_inputs("trace_ambient_occlusion (normals)", normals, width, height)
        row_end = height if row_end is None else row_end
        counts = out if out is not None else np.zeros((height, width), dtype=np.uint8)
        _check(_lib.rts_trace_ambient_occlusion(self._h, C.byref(constants), _ref(ao), _ptr(positions), _ptr(normals), _ptr_or_none(active),
                                                width, height, row_begin, row_end, _ptr(counts)), "rts_trace_ambient_occlusion")
        return counts

    def trace_ambient_occlusion_device(self, constants, ao, d_positions, d_normals, width, height, d_counts, row_begin=0, row_end=None,
                                       stream=None, d_active=None):
        """Device pointers, asynchronous: d_positions / d_normals = width * height RGBA32F, d_counts / d_active = width * height bytes."""
        row_end = height if row_end is None else row_end
        _check(_lib.rts_trace_ambient_occlusion_device(self._h, C.byref(constants), _ref(ao), C.c_void_p(d_positions or 0),
                                                       C.c_void_p(d_normals or 0), C.c_void_p(d_active or 0), width, height, row_begin,
                                                       row_end, C.c_void_p(d_counts or 0), C.c_void_p(stream or 0)),
               "rts_trace_ambient_occlusion_device")

    def trace_ambient_occlusion_stripes_device(self, constants, ao, d_positions, d_normals, width, height, d_counts, band_rows, n_stripes,
                                               stripe, stream=None, d_active=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        _check(_lib.rts_trace_ambient_occlusion_stripes_device(self._h, C.byref(constants), _ref(ao), C.c_void_p(d_positions or 0),
                                                               C.c_void_p(d_normals or 0), C.c_void_p(d_active or 0), width, height,
                                                               band_rows, n_stripes, stripe, C.c_void_p(d_counts or 0),
                                                               C.c_void_p(stream or 0)),
               "rts_trace_ambient_occlusion_stripes_device")

    # -- adaptive ambient occlusion (include/rts.h): `probe` AO samples per pixel, the remaining ones only where the probe disagrees --
    def trace_ambient_occlusion_adaptive(self, constants, ao, positions, normals, width, height, probe, row_begin=0, row_end=None,
                                         active=None, out=None, refined=None, want_refined=True):
        """Host-pointer dispatch; returns ``(uint8[H, W] counts, uint8[H, W] refined)`` (refined None with ``want_refined`` False):
        the count of unoccluded samples where ``refined`` is 1, else 0 or ``ao.samples`` by the probe's verdict.  ``out`` / ``refined``:
        arrays to write into (rows outside the range keep their contents)."""
        positions, active = _frame_inputs("trace_ambient_occlusion_adaptive", positions, width, height, active)
        normals, _ = _frame_inputs("trace_ambient_occlusion_adaptive (normals)", normals, width, height)
        row_end = height if row_end is None else row_end
        counts = out if out is not None else np.zeros((height, width), dtype=np.uint8)
        if refined is None and want_refined:
            refined = np.zeros((height, width), dtype=np.uint8)
        _check(_lib.rts_trace_ambient_occlusion_adaptive(self._h, C.byref(constants), _ref(ao), _ptr(positions), _ptr(normals),
                                                         _ptr_or_none(active), width, height, row_begin, row_end, probe, _ptr(counts),
                                                         _ptr_or_none(refined)), "rts_trace_ambient_occlusion_adaptive")
        return counts, refined

    def trace_ambient_occlusion_adaptive_device(self, constants, ao, d_positions, d_normals, width, height, d_counts, probe,
                                                d_refined=None, row_begin=0, row_end=None, stream=None, d_active=None):
        """Device pointers, asynchronous: d_positions / d_normals = width * height RGBA32F, d_counts = width * height bytes,
        d_refined / d_active = the same or None."""
        row_end = height if row_end is None else row_end
        _check(_lib.rts_trace_ambient_occlusion_adaptive_device(self._h, C.byref(constants), _ref(ao), C.c_void_p(d_positions or 0),
                                                                C.c_void_p(d_normals or 0), C.c_void_p(d_active or 0), width, height,
                                                                row_begin, row_end, probe, C.c_void_p(d_counts or 0),
                                                                C.c_void_p(d_refined or 0), C.c_void_p(stream or 0)),
               "rts_trace_ambient_occlusion_adaptive_device")

    def trace_ambient_occlusion_adaptive_stripes_device(self, constants, ao, d_positions, d_normals, width, height, d_counts, band_rows,
                                                        n_stripes, stripe, probe, d_refined=None, stream=None, d_active=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        _check(_lib.rts_trace_ambient_occlusion_adaptive_stripes_device(self._h, C.byref(constants), _ref(ao), C.c_void_p(d_positions or 0),
                                                                        C.c_void_p(d_normals or 0), C.c_void_p(d_active or 0), width,
                                                                        height, band_rows, n_stripes, stripe, probe,
                                                                        C.c_void_p(d_counts or 0), C.c_void_p(d_refined or 0),
                                                                        C.c_void_p(stream or 0)),
               "rts_trace_ambient_occlusion_adaptive_stripes_device")

    # -- bent normals (include/rts.h): the AO trace with the frame applied to the integer sum of its unoccluded directions --
    def trace_ambient_occlusion_bent(self, constants, ao, positions, normals, width, height, row_begin=0, row_end=None, active=None,
                                     out=None, bent=None, want_counts=True):
        """Host-pointer dispatch; returns ``(uint8[H, W] counts, float32[H, W, 4] bent)`` (counts None with ``want_counts`` False):
        ``bent[..., :3]`` the unnormalised mean free direction times the count, ``bent[..., 3]`` the count.  ``out`` / ``bent``: arrays
        to write into (rows outside the range keep their contents)."""
        positions, active = _frame_inputs("trace_ambient_occlusion_bent", positions, width, height, active)
        normals, _ = _frame_inputs("trace_ambient_occlusion_bent (normals)", normals, width, height)
        row_end = height if row_end is None else row_end
        counts = out if out is not None else (np.zeros((height, width), dtype=np.uint8) if want_counts else None)
        if bent is None:
            bent = np.zeros((height, width, 4), dtype=np.float32)
        _check(_lib.rts_trace_ambient_occlusion_bent(self._h, C.byref(constants), _ref(ao), _ptr(positions), _ptr(normals),
                                                     _ptr_or_none(active), width, height, row_begin, row_end, _ptr_or_none(counts),
                                                     _ptr(bent)), "rts_trace_ambient_occlusion_bent")
        return counts, bent

    def trace_ambient_occlusion_bent_device(self, constants, ao, d_positions, d_normals, width, height, d_counts, d_bent, row_begin=0,
                                            row_end=None, stream=None, d_active=None):
        """Device pointers, asynchronous: d_positions / d_normals / d_bent = width * height RGBA32F, d_counts (or None) / d_active (or
        None) = width * height bytes."""
        row_end = height if row_end is None else row_end
        _check(_lib.rts_trace_ambient_occlusion_bent_device(self._h, C.byref(constants), _ref(ao), C.c_void_p(d_positions or 0),
                                                            C.c_void_p(d_normals or 0), C.c_void_p(d_active or 0), width, height,
                                                            row_begin, row_end, C.c_void_p(d_counts or 0), C.c_void_p(d_bent or 0),
                                                            C.c_void_p(stream or 0)),
               "rts_trace_ambient_occlusion_bent_device")

    def trace_ambient_occlusion_bent_stripes_device(self, constants, ao, d_positions, d_normals, width, height, d_counts, d_bent,
                                                    band_rows, n_stripes, stripe, stream=None, d_active=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        _check(_lib.rts_trace_ambient_occlusion_bent_stripes_device(self._h, C.byref(constants), _ref(ao), C.c_void_p(d_positions or 0),
                                                                    C.c_void_p(d_normals or 0), C.c_void_p(d_active or 0), width, height,
                                                                    band_rows, n_stripes, stripe, C.c_void_p(d_counts or 0),
                                                                    C.c_void_p(d_bent or 0), C.c_void_p(stream or 0)),
               "rts_trace_ambient_occlusion_bent_stripes_device")

    # -- AO distance and falloff (include/rts.h): the AO trace with the nearest blocker and the falloff-weighted obscurance --
    def trace_ambient_occlusion_distance(self, constants, ao, falloff, positions, normals, width, height, row_begin=0, row_end=None,
                                         active=None, out=None, distance=None, obscurance=None, want_counts=True, want_distance=True,
                                         want_obscurance=True):
        """Host-pointer dispatch; returns ``(uint8[H, W] counts, float32[H, W] distance, uint16[H, W] obscurance)``, each None where
        its ``want_`` is False: the AO count, the nearest blocker over the pixel's samples as a fraction of the segment (+Inf where
        every sample is free) and the obscurance in the wide filter's fixed point.  ``out`` / ``distance`` / ``obscurance``: arrays to
        write into (rows outside the range keep their contents)."""
        positions, active = _frame_inputs("trace_ambient_occlusion_distance", positions, width, height, active)
        normals, _ = _frame_inputs("trace_ambient_occlusion_distance (normals)", normals, width, height)
        row_end = height if row_end is None else row_end
        counts = out if out is not None else (np.zeros((height, width), dtype=np.uint8) if want_counts else None)
        if distance is None and want_distance:
            distance = np.zeros((height, width), dtype=np.float32)
        if obscurance is None and want_obscurance:
            obscurance = np.zeros((height, width), dtype=np.uint16)
        _check(_lib.rts_trace_ambient_occlusion_distance(self._h, C.byref(constants), _ref(ao), _ref(falloff), _ptr(positions),
                                                         _ptr(normals), _ptr_or_none(active), width, height, row_begin, row_end,
                                                         _ptr_or_none(counts), _ptr_or_none(distance), _ptr_or_none(obscurance)),
               "rts_trace_ambient_occlusion_distance")
        return counts, distance, obscurance

    def trace_ambient_occlusion_distance_device(self, constants, ao, falloff, d_positions, d_normals, width, height, d_counts, d_distance,
                                                d_obscurance, row_begin=0, row_end=None, stream=None, d_active=None):
        """Device pointers, asynchronous: d_positions / d_normals = width * height RGBA32F, d_counts (or None) / d_active (or None) =
        width * height bytes, d_distance (or None) = width * height floats, d_obscurance (or None) = width * height uint16."""
        row_end = height if row_end is None else row_end
        _check(_lib.rts_trace_ambient_occlusion_distance_device(self._h, C.byref(constants), _ref(ao), _ref(falloff),
                                                                C.c_void_p(d_positions or 0), C.c_void_p(d_normals or 0),
                                                                C.c_void_p(d_active or 0), width, height, row_begin, row_end,
                                                                C.c_void_p(d_counts or 0), C.c_void_p(d_distance or 0),
                                                                C.c_void_p(d_obscurance or 0), C.c_void_p(stream or 0)),
               "rts_trace_ambient_occlusion_distance_device")

    def trace_ambient_occlusion_distance_stripes_device(self, constants, ao, falloff, d_positions, d_normals, width, height, d_counts,
                                                        d_distance, d_obscurance, band_rows, n_stripes, stripe, stream=None, d_active=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        _check(_lib.rts_trace_ambient_occlusion_distance_stripes_device(self._h, C.byref(constants), _ref(ao), _ref(falloff),
                                                                        C.c_void_p(d_positions or 0), C.c_void_p(d_normals or 0),
                                                                        C.c_void_p(d_active or 0), width, height, band_rows, n_stripes,
                                                                        stripe, C.c_void_p(d_counts or 0), C.c_void_p(d_distance or 0),
                                                                        C.c_void_p(d_obscurance or 0), C.c_void_p(stream or 0)),
               "rts_trace_ambient_occlusion_distance_stripes_device")

    # -- light lists (include/rts.h): up to 8 hard lights in one dispatch, light l in bit l of the mask byte --
    def trace_light_list(self, constants, lights, positions, width, height, lights_map=None, row_begin=0, row_end=None, out=None):
        """Host-pointer dispatch; returns ``uint8[H, W]``: bit ``l`` = light ``l``'s shadow byte where ``lights_map`` (uint8[H, W], or
        None: everywhere) has bit ``l`` set.  ``out``: an array to write the rows into."""
        positions, lights_map = _frame_inputs("trace_light_list", positions, width, height, lights_map, "lights_map")
        row_end = height if row_end is None else row_end
        mask = out if out is not None else np.zeros((height, width), dtype=np.uint8)
        _check(_lib.rts_trace_light_list(self._h, C.byref(constants), _ref(lights), _ptr(positions),
                                         _ptr_or_none(lights_map), width, height, row_begin, row_end,
                                         _ptr(mask)), "rts_trace_light_list")
        return mask

    def trace_light_list_device(self, constants, lights, d_positions, width, height, d_mask, d_lights_map=None, row_begin=0,
                                row_end=None, stream=None):
        """Device pointers, asynchronous: d_mask / d_lights_map = width * height bytes (the map may be None)."""
        row_end = height if row_end is None else row_end
        _check(_lib.rts_trace_light_list_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                C.c_void_p(d_lights_map or 0), width, height, row_begin, row_end, C.c_void_p(d_mask),
                                                C.c_void_p(stream or 0)),
               "rts_trace_light_list_device")

    def trace_light_list_stripes_device(self, constants, lights, d_positions, width, height, d_mask, band_rows, n_stripes, stripe,
                                        d_lights_map=None, stream=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        _check(_lib.rts_trace_light_list_stripes_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                        C.c_void_p(d_lights_map or 0), width, height, band_rows, n_stripes, stripe,
                                                        C.c_void_p(d_mask), C.c_void_p(stream or 0)),
               "rts_trace_light_list_stripes_device")

    # -- soft light lists (include/rts.h): up to 8 lights, hard or soft, in one dispatch, a count plane per light --
    def trace_soft_light_list(self, constants, lights, positions, width, height, lights_map=None, row_begin=0, row_end=None, out=None):
        """Host-pointer dispatch; returns ``uint8[count, H, W]``: plane ``l`` = light ``l``'s unoccluded samples where ``lights_map``
        (uint8[H, W], or None: everywhere) has bit ``l`` set.  ``out``: an array of at least ``count`` planes to write the rows into."""
        positions, lights_map = _frame_inputs("trace_soft_light_list", positions, width, height, lights_map, "lights_map")
        row_end = height if row_end is None else row_end
        counts = out if out is not None else np.zeros((lights.count if lights is not None else 1, height, width), dtype=np.uint8)
        _check(_lib.rts_trace_soft_light_list(self._h, C.byref(constants), _ref(lights), _ptr(positions),
                                              _ptr_or_none(lights_map), width, height, row_begin, row_end,
                                              _ptr(counts)), "rts_trace_soft_light_list")
        return counts

    def trace_soft_light_list_device(self, constants, lights, d_positions, width, height, d_counts, d_lights_map=None, row_begin=0,
                                     row_end=None, stream=None):
        """Device pointers, asynchronous: d_counts = count * width * height bytes, d_lights_map = width * height bytes or None."""
        row_end = height if row_end is None else row_end
        _check(_lib.rts_trace_soft_light_list_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                     C.c_void_p(d_lights_map or 0), width, height, row_begin, row_end,
                                                     C.c_void_p(d_counts), C.c_void_p(stream or 0)),
               "rts_trace_soft_light_list_device")

    def trace_soft_light_list_stripes_device(self, constants, lights, d_positions, width, height, d_counts, band_rows, n_stripes, stripe,
                                             d_lights_map=None, stream=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        _check(_lib.rts_trace_soft_light_list_stripes_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                             C.c_void_p(d_lights_map or 0), width, height, band_rows, n_stripes, stripe,
                                                             C.c_void_p(d_counts), C.c_void_p(stream or 0)),
               "rts_trace_soft_light_list_stripes_device")

    # -- sparse light lists (include/rts.h): the two list traces over a list of pixels, the marked pairs alone written --
    def _sparse_host(self, fn, name, constants, lights, positions, width, height, pixels, planes, planes_shape, lights_map):
        positions, lights_map = _frame_inputs(name, positions, width, height, lights_map, "lights_map")
        pixels = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        if planes is None or planes.dtype != np.uint8 or not planes.flags.c_contiguous or planes.size < int(np.prod(planes_shape)):
            raise RtsError(1, f"{name}: the planes must be contiguous uint8 of the list's planes (they are merged into, in place)")
        if pixels.size == 0:
            pixels = np.zeros(1, np.uint32)
            n = 0
        else:
            n = pixels.size
        _check(fn(self._h, C.byref(constants), _ref(lights), _ptr(positions), _ptr_or_none(lights_map), width, height, _ptr(pixels), n,
                  _ptr(planes)), name)
        return planes

    def trace_light_list_sparse(self, constants, lights, positions, width, height, pixels, mask, lights_map=None):
        """Host-pointer sparse trace of a hard light list: ``mask`` (``uint8[H, W]``) is MERGED INTO, in place: bit ``l`` of
        ``mask[p]`` for every ``p`` in ``pixels`` (uint32 indices ``y * W + x``) and ``l`` with bit ``l`` of ``lights_map[p]`` set
        (None: every ``l < count``); nothing else is touched.  Returns ``mask``."""
        return self._sparse_host(_lib.rts_trace_light_list_sparse, "rts_trace_light_list_sparse", constants, lights, positions, width, height,
                                 pixels, mask, (height, width), lights_map)

    def trace_light_list_sparse_device(self, constants, lights, d_positions, width, height, d_pixels, d_n, capacity, d_mask,
                                       d_lights_map=None, stream=None):
        """Device pointers, asynchronous, one kernel: d_pixels = ``capacity`` uint32 entries, d_n = one uint32 (the list's length), both
        read on the device; the first ``min(*d_n, capacity)`` entries are traced."""
        _check(_lib.rts_trace_light_list_sparse_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                       C.c_void_p(d_lights_map or 0), width, height, C.c_void_p(d_pixels or 0),
                                                       C.c_void_p(d_n or 0), capacity, C.c_void_p(d_mask), C.c_void_p(stream or 0)),
               "rts_trace_light_list_sparse_device")

    def trace_soft_light_list_sparse(self, constants, lights, positions, width, height, pixels, counts, lights_map=None):
        """Host-pointer sparse trace of a soft light list: ``counts`` (``uint8[count, H, W]``) is MERGED INTO, in place: plane ``l`` at
        every ``p`` in ``pixels`` with bit ``l`` of ``lights_map[p]`` set (None: every ``l < count``).  Returns ``counts``."""
        count = lights.count if lights is not None and 1 <= lights.count <= 8 else 1
        return self._sparse_host(_lib.rts_trace_soft_light_list_sparse, "rts_trace_soft_light_list_sparse", constants, lights, positions, width,
                                 height, pixels, counts, (count, height, width), lights_map)

    def trace_soft_light_list_sparse_device(self, constants, lights, d_positions, width, height, d_pixels, d_n, capacity, d_counts,
                                            d_lights_map=None, stream=None):
        """Device pointers, asynchronous, one kernel: as trace_light_list_sparse_device, d_counts = count planes of width * height bytes."""
        _check(_lib.rts_trace_soft_light_list_sparse_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                            C.c_void_p(d_lights_map or 0), width, height, C.c_void_p(d_pixels or 0),
                                                            C.c_void_p(d_n or 0), capacity, C.c_void_p(d_counts), C.c_void_p(stream or 0)),
               "rts_trace_soft_light_list_sparse_device")

    # -- soft light list distance (include/rts.h): a soft light list with the nearest blocker per light beside its count --
    def trace_soft_light_list_distance(self, constants, lights, positions, width, height, lights_map=None, row_begin=0, row_end=None,
                                       out=None, counts=None, want_counts=True):
        """Host-pointer dispatch; returns ``(float32[count, H, W] distances, uint8[count, H, W] counts)`` (counts None with
        ``want_counts`` False): plane ``l`` = the minimum of light ``l``'s samples' distances and the number of unoccluded ones where
        ``lights_map`` (uint8[H, W], or None: everywhere) has bit ``l`` set, else +0 and 0.  ``out`` / ``counts``: arrays of at least
        ``count`` planes to write the rows into."""
        positions, lights_map = _frame_inputs("trace_soft_light_list_distance", positions, width, height, lights_map, "lights_map")
        row_end = height if row_end is None else row_end
        planes = lights.count if lights is not None else 1
        dist = out if out is not None else np.zeros((planes, height, width), dtype=np.float32)
        if counts is None and want_counts:
            counts = np.zeros((planes, height, width), dtype=np.uint8)
        _check(_lib.rts_trace_soft_light_list_distance(self._h, C.byref(constants), _ref(lights), _ptr(positions),
                                                       _ptr_or_none(lights_map), width, height, row_begin, row_end,
                                                       _ptr_or_none(dist), _ptr_or_none(counts)), "rts_trace_soft_light_list_distance")
        return dist, counts

    def trace_soft_light_list_distance_device(self, constants, lights, d_positions, width, height, d_distances, d_counts=None,
                                              d_lights_map=None, row_begin=0, row_end=None, stream=None):
        """Device pointers, asynchronous: d_distances = count * width * height floats, d_counts = count * width * height bytes or None,
        d_lights_map = width * height bytes or None."""
        row_end = height if row_end is None else row_end
        _check(_lib.rts_trace_soft_light_list_distance_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                              C.c_void_p(d_lights_map or 0), width, height, row_begin, row_end,
                                                              C.c_void_p(d_distances or 0), C.c_void_p(d_counts or 0),
                                                              C.c_void_p(stream or 0)),
               "rts_trace_soft_light_list_distance_device")

    def trace_soft_light_list_distance_stripes_device(self, constants, lights, d_positions, width, height, d_distances, band_rows,
                                                      n_stripes, stripe, d_counts=None, d_lights_map=None, stream=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        _check(_lib.rts_trace_soft_light_list_distance_stripes_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                                      C.c_void_p(d_lights_map or 0), width, height, band_rows, n_stripes,
                                                                      stripe, C.c_void_p(d_distances or 0), C.c_void_p(d_counts or 0),
                                                                      C.c_void_p(stream or 0)),
               "rts_trace_soft_light_list_distance_stripes_device")

    # -- adaptive soft light lists (include/rts.h): a soft light list with a probe count per light, its penumbra alone refined --
    def trace_soft_light_list_adaptive(self, constants, lights, probes, positions, width, height, lights_map=None, row_begin=0,
                                       row_end=None, out=None, refined=None, want_refined=True, tables=None):
        """Host-pointer dispatch; returns ``(uint8[count, H, W] counts, uint8[H, W] refined)`` (refined None with ``want_refined``
        False).  ``probes``: ``count`` integers, 0 = light ``l`` in full, else its probe; bit ``l`` of ``refined`` = light ``l`` took
        its full count there.  ``out`` / ``refined``: arrays to write the rows into.  ``tables``: None, or ``count`` integers, the
        per-pixel jitter table of each light (0: none) -- rts_trace_soft_light_list_jittered."""
        positions, lights_map = _frame_inputs("trace_soft_light_list_adaptive", positions, width, height, lights_map, "lights_map")
        row_end = height if row_end is None else row_end
        counts = out if out is not None else np.zeros((lights.count if lights is not None else 1, height, width), dtype=np.uint8)
        if refined is None and want_refined:
            refined = np.zeros((height, width), dtype=np.uint8)
        if tables is not None:
            _check(_lib.rts_trace_soft_light_list_jittered(self._h, C.byref(constants), _ref(lights), _ptr(positions),
                                                           _ptr_or_none(lights_map), width, height, row_begin, row_end, _ptr(counts),
                                                           _probes(lights, probes), _probes(lights, tables, "tables"),
                                                           _ptr_or_none(refined)),
                   "rts_trace_soft_light_list_jittered")
            return counts, refined
        _check(_lib.rts_trace_soft_light_list_adaptive(self._h, C.byref(constants), _ref(lights), _ptr(positions),
                                                       _ptr_or_none(lights_map), width, height, row_begin, row_end, _ptr(counts),
                                                       _probes(lights, probes), _ptr_or_none(refined)),
               "rts_trace_soft_light_list_adaptive")
        return counts, refined

    def trace_soft_light_list_adaptive_device(self, constants, lights, probes, d_positions, width, height, d_counts, d_refined=None,
                                              d_lights_map=None, row_begin=0, row_end=None, stream=None, tables=None):
        """Device pointers, asynchronous: d_counts = count * width * height bytes, d_refined / d_lights_map = width * height bytes or
        None.  ``probes`` and ``tables`` (None: today's call) are read at the call."""
        row_end = height if row_end is None else row_end
        if tables is not None:
            _check(_lib.rts_trace_soft_light_list_jittered_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                                  C.c_void_p(d_lights_map or 0), width, height, row_begin, row_end,
                                                                  C.c_void_p(d_counts), _probes(lights, probes),
                                                                  _probes(lights, tables, "tables"), C.c_void_p(d_refined or 0),
                                                                  C.c_void_p(stream or 0)),
                   "rts_trace_soft_light_list_jittered_device")
            return
        _check(_lib.rts_trace_soft_light_list_adaptive_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                              C.c_void_p(d_lights_map or 0), width, height, row_begin, row_end,
                                                              C.c_void_p(d_counts), _probes(lights, probes), C.c_void_p(d_refined or 0),
                                                              C.c_void_p(stream or 0)),
               "rts_trace_soft_light_list_adaptive_device")

    def trace_soft_light_list_adaptive_stripes_device(self, constants, lights, probes, d_positions, width, height, d_counts, band_rows,
                                                      n_stripes, stripe, d_refined=None, d_lights_map=None, stream=None, tables=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        if tables is not None:
            _check(_lib.rts_trace_soft_light_list_jittered_stripes_device(self._h, C.byref(constants), _ref(lights),
                                                                          C.c_void_p(d_positions), C.c_void_p(d_lights_map or 0), width,
                                                                          height, band_rows, n_stripes, stripe, C.c_void_p(d_counts),
                                                                          _probes(lights, probes), _probes(lights, tables, "tables"),
                                                                          C.c_void_p(d_refined or 0), C.c_void_p(stream or 0)),
                   "rts_trace_soft_light_list_jittered_stripes_device")
            return
        _check(_lib.rts_trace_soft_light_list_adaptive_stripes_device(self._h, C.byref(constants), _ref(lights), C.c_void_p(d_positions),
                                                                      C.c_void_p(d_lights_map or 0), width, height, band_rows,
                                                                      n_stripes, stripe, C.c_void_p(d_counts), _probes(lights, probes),
                                                                      C.c_void_p(d_refined or 0), C.c_void_p(stream or 0)),
               "rts_trace_soft_light_list_adaptive_stripes_device")

    # -- adaptive soft shadows (include/rts.h): `probe` samples per pixel, the remaining ones only where the probe disagrees --
    def trace_shadow_mask_adaptive(self, constants, positions, width, height, light, probe, row_begin=0, row_end=None, active=None,
                                   out=None, refined=None, want_refined=True):
        """Host-pointer dispatch; returns ``(uint8[H, W] mask, uint8[H, W] refined)`` (refined None with ``want_refined`` False):
        the count of unoccluded samples where ``refined`` is 1, else 0 or ``nsamples`` by the probe's verdict.  ``out`` / ``refined``:
        arrays to write into (rows outside the range keep their contents)."""
        positions, active = _frame_inputs("trace_shadow_mask_adaptive", positions, width, height, active)
        row_end = height if row_end is None else row_end
        mask = out if out is not None else np.zeros((height, width), dtype=np.uint8)
        if refined is None and want_refined:
            refined = np.zeros((height, width), dtype=np.uint8)
        _check(_lib.rts_trace_shadow_mask_adaptive(self._h, C.byref(constants), _ref(light), _ptr(positions), _ptr_or_none(active),
                                                   width, height, row_begin, row_end, probe, _ptr(mask), _ptr_or_none(refined)),
               "rts_trace_shadow_mask_adaptive")
        return mask, refined

    def trace_shadow_mask_adaptive_device(self, constants, d_positions, width, height, d_mask, light, probe, d_refined=None,
                                          row_begin=0, row_end=None, stream=None, d_active=None):
        """Device pointers, asynchronous: d_mask = width * height bytes, d_refined / d_active = the same or None."""
        row_end = height if row_end is None else row_end
        _check(_lib.rts_trace_shadow_mask_adaptive_device(self._h, C.byref(constants), _ref(light), C.c_void_p(d_positions),
                                                          C.c_void_p(d_active or 0), width, height, row_begin, row_end, probe,
                                                          C.c_void_p(d_mask), C.c_void_p(d_refined or 0), C.c_void_p(stream or 0)),
               "rts_trace_shadow_mask_adaptive_device")

    def trace_shadow_mask_adaptive_stripes_device(self, constants, d_positions, width, height, d_mask, band_rows, n_stripes, stripe,
                                                  light, probe, d_refined=None, stream=None, d_active=None):
        """One dispatch over the interleaved bands `stripe, stripe + n_stripes, ...` of band_rows rows each."""
        _check(_lib.rts_trace_shadow_mask_adaptive_stripes_device(self._h, C.byref(constants), _ref(light), C.c_void_p(d_positions),
                                                                  C.c_void_p(d_active or 0), width, height, band_rows, n_stripes,
                                                                  stripe, probe, C.c_void_p(d_mask), C.c_void_p(d_refined or 0),
                                                                  C.c_void_p(stream or 0)),
               "rts_trace_shadow_mask_adaptive_stripes_device")

    # -- plumbing ---------------------------------------------------------------------------
    def stream_create(self):
        s = C.c_void_p()
        _check(_lib.rts_stream_create(self._h, C.byref(s)), "rts_stream_create")
        return s.value

    def stream_destroy(self, stream):
        _check(_lib.rts_stream_destroy(self._h, C.c_void_p(stream)), "rts_stream_destroy")

    def malloc(self, nbytes):
        p = C.c_void_p()
        _check(_lib.rts_device_malloc(self._h, C.byref(p), nbytes), "rts_device_malloc")
        return p.value

    def free(self, ptr):
        _check(_lib.rts_device_free(self._h, C.c_void_p(ptr)), "rts_device_free")

    def h2d(self, dptr, array):
        array = np.ascontiguousarray(array)
        _check(_lib.rts_memcpy_h2d(self._h, C.c_void_p(dptr), _ptr(array), array.nbytes), "rts_memcpy_h2d")

    def d2h(self, array, dptr):
        _check(_lib.rts_memcpy_d2h(self._h, _ptr(array), C.c_void_p(dptr), array.nbytes), "rts_memcpy_d2h")

    def mem_info(self):
        """(free, total) device memory in bytes."""
        f, t = C.c_size_t(0), C.c_size_t(0)
        _check(_lib.rts_device_mem_info(self._h, C.byref(f), C.byref(t)), "rts_device_mem_info")
        return f.value, t.value

    def synchronize(self, stream=None):
        _check(_lib.rts_stream_synchronize(self._h, C.c_void_p(stream or 0)), "rts_stream_synchronize")

    def timer_begin(self, stream=None):
        _check(_lib.rts_timer_begin(self._h, C.c_void_p(stream or 0)), "rts_timer_begin")

    def timer_end(self, stream=None):
        _check(_lib.rts_timer_end(self._h, C.c_void_p(stream or 0)), "rts_timer_end")

    def timer_elapsed_ms(self):
        ms = C.c_float(0)
        _check(_lib.rts_timer_elapsed_ms(self._h, C.byref(ms)), "rts_timer_elapsed_ms")
        return float(ms.value)

    def timer_mark(self, slot, stream=None):
        _check(_lib.rts_timer_mark(self._h, C.c_void_p(stream or 0), slot), "rts_timer_mark")

    def timer_between_ms(self, slot_a, slot_b):
        ms = C.c_float(0)
        _check(_lib.rts_timer_between_ms(self._h, slot_a, slot_b, C.byref(ms)), "rts_timer_between_ms")
        return float(ms.value)

    def last_kernel_name(self):
        return _lib.rts_ctx_last_kernel_name(self._h).decode()

    def set_tile_order(self, order):
        if order is None:
            _check(_lib.rts_ctx_set_tile_order(self._h, None, 0), "rts_ctx_set_tile_order")
            return
        order = np.ascontiguousarray(order, np.uint32)
        _check(_lib.rts_ctx_set_tile_order(self._h, _ptr(order), order.size), "rts_ctx_set_tile_order")

    def read_follow(self, tiles, stream=None):
        """rts_ctx_read_follow: (lives in 100 MHz ticks per row-major tile of the stream's last traced dispatch, the order its next
        trace runs as bx | by << 16 per record).  Synchronises the stream."""
        lives = np.zeros(tiles, np.uint32)
        order = np.zeros(tiles, np.uint32)
        _check(_lib.rts_ctx_read_follow(self._h, C.c_void_p(stream or 0), _ptr(lives), _ptr(order), tiles), "rts_ctx_read_follow")
        return lives, order

    def read_wave_stats(self, waves):
        out = np.zeros((waves, 4), dtype=np.uint64)
        _check(_lib.rts_ctx_read_wave_stats(self._h, _ptr(out), waves), "rts_ctx_read_wave_stats")
        return out

    def read_wave_realtime(self, waves):
        out = np.zeros((waves, 4), dtype=np.uint64)
        _check(_lib.rts_ctx_read_wave_realtime(self._h, _ptr(out), waves), "rts_ctx_read_wave_realtime")
        return out

    def autotune(self, constants, d_positions, width, height, d_mask, light=None, stripes=None):
        """rts_ctx_autotune(_stripes): times the candidate kernels, launch options and split tables on this dispatch (stripes =
        (band_rows, n_stripes, stripe) for one rank's interleaved stripe), keeps the fastest; returns (kernel id, ms)."""
        chosen, ms = C.c_int(-1), C.c_float(0)
        lp = C.byref(light) if light is not None else None
        if stripes is not None:
            _check(_lib.rts_ctx_autotune_stripes(self._h, C.byref(constants), lp, C.c_void_p(d_positions), width, height, stripes[0],
                                                 stripes[1], stripes[2], C.c_void_p(d_mask), C.byref(chosen), C.byref(ms)),
                   "rts_ctx_autotune_stripes")
        else:
            _check(_lib.rts_ctx_autotune(self._h, C.byref(constants), lp, C.c_void_p(d_positions), width, height,
                                         C.c_void_p(d_mask), C.byref(chosen), C.byref(ms)), "rts_ctx_autotune")
        return int(chosen.value), float(ms.value)

    def plan_tile_order(self, constants, d_positions, width, height, d_mask, light=None, stripes=None, xcd_square=32, life_block=0):
        """rts_ctx_plan_tile_order: measures this dispatch, installs the longest-first, XCD-dealt tile order; returns the tiles ordered."""
        tiles = C.c_uint32(0)
        band, n, r = stripes if stripes is not None else (0, 1, 0)
        _check(_lib.rts_ctx_plan_tile_order(self._h, C.byref(constants), C.byref(light) if light is not None else None, C.c_void_p(d_positions),
                                            width, height, band, n, r, C.c_void_p(d_mask), xcd_square, life_block, C.byref(tiles)),
               "rts_ctx_plan_tile_order")
        return int(tiles.value)

    def split_plan(self):
        """Parameters of the installed split table as a dict (None without a table): rts_ctx_get_split_plan."""
        plan = SplitPlan()
        if _lib.rts_ctx_get_split_plan(self._h, C.byref(plan)) != 0:
            return None
        return {"min_life_us": float(plan.min_life_us), "end_after_us": float(plan.end_after_us), "piece_us": float(plan.piece_us),
                "front_life_us": float(plan.front_life_us), "front_share": float(plan.front_share), "max_pieces": int(plan.max_pieces),
                "max_tiles": int(plan.max_tiles), "xcd_square": int(plan.xcd_square), "life_block": int(plan.life_block)}

    def plan_splits(self, constants, d_positions, width, height, d_mask, light=None, min_life_us=20.0, piece_us=10.0,
                    max_pieces=8, max_tiles=0, row_begin=0, row_end=None, stripes=None, prev=None, end_after_us=0.0, front_life_us=0.0, front_share=0.0,
                    xcd_square=0, life_block=0):
        """rts_ctx_plan_splits(_stripes): measures the dispatch, installs the split table; returns (tiles, pieces).
        stripes = (band_rows, n_stripes, stripe) plans the interleaved-stripe dispatch; prev = (stats, realtime) arrays of an
        earlier frame (read_wave_stats / read_wave_realtime) instead of a measuring launch."""
        plan = SplitPlan(min_life_us, end_after_us, piece_us, front_life_us, front_share, max_pieces, max_tiles, xcd_square, life_block, 0, None, None, 0)
        keep = None
        if prev is not None:
            keep = (np.ascontiguousarray(prev[0], np.uint64), np.ascontiguousarray(prev[1], np.uint64))
            plan.prev_stats, plan.prev_realtime, plan.prev_waves = keep[0].ctypes.data, keep[1].ctypes.data, keep[0].size // 4
        tiles, pieces = C.c_uint32(0), C.c_uint32(0)
        lp = C.byref(light) if light is not None else None
        if stripes is not None:
            _check(_lib.rts_ctx_plan_splits_stripes(self._h, C.byref(constants), lp, C.c_void_p(d_positions), width, height,
                                                    stripes[0], stripes[1], stripes[2], C.c_void_p(d_mask), C.byref(plan),
                                                    C.byref(tiles), C.byref(pieces)), "rts_ctx_plan_splits_stripes")
        else:
            row_end = height if row_end is None else row_end
            _check(_lib.rts_ctx_plan_splits(self._h, C.byref(constants), lp, C.c_void_p(d_positions), width, height, row_begin,
                                            row_end, C.c_void_p(d_mask), C.byref(plan), C.byref(tiles), C.byref(pieces)),
                   "rts_ctx_plan_splits")
        return int(tiles.value), int(pieces.value)

    def read_piece_stats(self, pieces, clocks=True):
        """(records uint32[pieces, 8], clocks uint64[pieces, 8] or None): rts_ctx_read_piece_stats."""
        rec = np.zeros((pieces, 8), np.uint32)
        clk = np.zeros((pieces, 8), np.uint64) if clocks else None
        _check(_lib.rts_ctx_read_piece_stats(self._h, _ptr(rec), _ptr(clk) if clocks else None, pieces), "rts_ctx_read_piece_stats")
        return rec, clk

    def selftest_reciprocal(self):
        """(patterns checked, patterns that differ from the IEEE division, an example): rts_selftest_reciprocal."""
        out = np.zeros(3, np.uint64)
        _check(_lib.rts_selftest_reciprocal(self._h, _ptr(out)), "rts_selftest_reciprocal")
        return int(out[0]), int(out[1]), int(out[2])

    def clear_splits(self):
        _check(_lib.rts_ctx_clear_splits(self._h), "rts_ctx_clear_splits")

    def clock_probe_mhz(self, rows):
        """Shader clock held during the launches since set_option("clock_probe", rows) (the timed launches themselves)."""
        out = np.zeros((rows, 4), np.uint64)
        _check(_lib.rts_ctx_read_clock_probe(self._h, _ptr(out), rows), "rts_ctx_read_clock_probe")
        self.last_clock_probe = out.copy()                      # (tools: wave lifetimes, hardware slots)
        end = out[:, 1] & np.uint64(0x0000FFFFFFFFFFFF)         # the top 16 bits carry the wave's hardware slot (HW_ID)
        ok = (end > out[:, 0]) & (out[:, 3] > out[:, 2])
        if not ok.any():
            return None
        return float((end[ok] - out[ok, 0]).astype(np.float64).sum() / (out[ok, 3] - out[ok, 2]).astype(np.float64).sum() * 100.0)

    def measure_shader_clock_mhz(self, trace, waves, launches=8):
        """Clock the chip holds while `trace()` (one dispatch of a packet kernel with `waves` one-wave workgroups) runs
        back to back: shader clocks per 100 MHz realtime tick, summed over every wave of the last launch
        (MI355X_MICROARCH.md, DVFS give-back item 6).  Diagnostics build of the kernel; results are not touched."""
        self.set_option("wave_stats", waves)
        try:
            for _ in range(launches):
                trace()
            self.synchronize()
            st = self.read_wave_stats(waves)
            rt = self.read_wave_realtime(waves)
        finally:
            self.set_option("wave_stats", 0)
        ok = (rt[:, 1] > rt[:, 0]) & (st[:, 1] > st[:, 0])
        if not ok.any():
            return None
        clocks = (st[ok, 1] - st[ok, 0]).astype(np.float64).sum()
        ticks = (rt[ok, 1] - rt[ok, 0]).astype(np.float64).sum()
        return float(clocks / ticks * 100.0)


# -- harness entry points -----------------------------------------------------------------------
def primary_positions(packed, eye, target, fovy, width, height, threads=0):
    """G-buffer position target (camera-relative closest hit per pixel); see include/rts_scene.h."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32).reshape(-1, 4)
    pos = np.zeros((height, width, 4), dtype=np.float32)
    e = (C.c_float * 3)(*[float(x) for x in eye])
    t = (C.c_float * 3)(*[float(x) for x in target])
    hits = C.c_uint64(0)
    _check(_lib.rtsh_primary_positions(_ptr(packed), packed.shape[0], e, t, fovy, width, height, _ptr(pos),
                                       C.byref(hits), threads), "rtsh_primary_positions")
    return pos, int(hits.value)


def primary_gbuffer(packed, eye, target, fovy, width, height, threads=0):
    """Positions + normals targets (host)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32).reshape(-1, 4)
    pos = np.zeros((height, width, 4), dtype=np.float32)
    nrm = np.zeros((height, width, 4), dtype=np.float32)
    e = (C.c_float * 3)(*[float(x) for x in eye])
    t = (C.c_float * 3)(*[float(x) for x in target])
    hits = C.c_uint64(0)
    _check(_lib.rtsh_primary_gbuffer(_ptr(packed), packed.shape[0], e, t, fovy, width, height, _ptr(pos), _ptr(nrm),
                                     C.byref(hits), threads), "rtsh_primary_gbuffer")
    return pos, nrm, int(hits.value)


def primary_gbuffer_device(ctx, eye, target, fovy, width, height, d_positions, d_normals=None, stream=None):
    """The G-buffer pass on the GPU, through the BVH uploaded to `ctx` (device pointers, asynchronous)."""
    e = (C.c_float * 3)(*[float(x) for x in eye])
    t = (C.c_float * 3)(*[float(x) for x in target])
    _check(_lib.rtsh_primary_gbuffer_device(ctx.handle, e, t, fovy, width, height, C.c_void_p(d_positions),
                                            C.c_void_p(d_normals or 0), C.c_void_p(stream or 0)),
           "rtsh_primary_gbuffer_device")


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v]) if v is not None else None


def primary_gbuffer_motion(packed, prev_packed, eye, prev_eye, target, fovy, width, height, threads=0, want_leaves=True):
    """The motion G-buffer pass on the host (rtsh_primary_gbuffer_motion): ``(positions, normals, prev_points, prev_point_normals,
    leaves or None, hits)``.  ``prev_packed``: the previous frame's stream, a refit sibling of ``packed``; ``prev_points[..., 3]`` is 1
    where the hit triangle did not move, 2 where it did, 0 on the background."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32).reshape(-1, 4) if packed is not None else None
    prev_packed = np.ascontiguousarray(prev_packed, dtype=np.uint32).reshape(-1, 4) if prev_packed is not None else None
    pos, nrm, pts, pnr = (np.zeros((height, width, 4), dtype=np.float32) for _ in range(4))
    leaves = np.zeros((height, width), np.uint32) if want_leaves else None
    hits = C.c_uint64(0)
    _check(_lib.rtsh_primary_gbuffer_motion(_ptr_or_none(packed), packed.shape[0] if packed is not None else 0, _ptr_or_none(prev_packed),
                                            prev_packed.shape[0] if prev_packed is not None else 0, _f3(eye), _f3(prev_eye), _f3(target), fovy,
                                            width, height, _ptr(pos), _ptr(nrm), _ptr(pts), _ptr(pnr), _ptr_or_none(leaves), C.byref(hits),
                                            threads), "rtsh_primary_gbuffer_motion")
    return pos, nrm, pts, pnr, leaves, int(hits.value)


def primary_gbuffer_motion_device(ctx, d_prev_packed, prev_count, eye, prev_eye, target, fovy, width, height, d_positions, d_normals,
                                  d_prev_points, d_prev_point_normals, d_leaves=None, stream=None):
    """The motion G-buffer pass on the GPU, through the stream installed in ``ctx`` and the previous stream at ``d_prev_packed``
    (``prev_count`` vec4, e.g. from :func:`snapshot_bvh_device`).  Device pointers, one kernel, asynchronous."""
    _check(_lib.rtsh_primary_gbuffer_motion_device(ctx.handle, C.c_void_p(d_prev_packed or 0), prev_count, _f3(eye), _f3(prev_eye), _f3(target),
                                                   fovy, width, height, C.c_void_p(d_positions or 0), C.c_void_p(d_normals or 0),
                                                   C.c_void_p(d_prev_points or 0), C.c_void_p(d_prev_point_normals or 0),
                                                   C.c_void_p(d_leaves or 0), C.c_void_p(stream or 0)), "rtsh_primary_gbuffer_motion_device")


def bvh_count_device(ctx):
    """The size in vec4 of the stream installed in ``ctx`` (0 before ``set_bvh``)."""
    return int(_lib.rtsh_ctx_bvh_count(ctx.handle))


def snapshot_bvh_device(ctx, d_out, capacity_vec4, stream=None):
    """rtsh_ctx_snapshot_bvh_device: the installed stream copied into the device buffer ``d_out`` (one asynchronous device-to-device
    copy).  Returns the stream's size in vec4."""
    _check(_lib.rtsh_ctx_snapshot_bvh_device(ctx.handle, C.c_void_p(d_out or 0), capacity_vec4, C.c_void_p(stream or 0)),
           "rtsh_ctx_snapshot_bvh_device")
    return bvh_count_device(ctx)


def combine(constants, light, positions, normals, mask):
    """Combine.frag on the host: uint8[H, W, 3]."""
    H, W = mask.shape
    normals = np.ascontiguousarray(normals, np.float32)
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    mask = np.ascontiguousarray(mask, np.uint8)
    rgb = np.zeros((H, W, 3), np.uint8)
    lp = C.byref(light) if light is not None else None
    _check(_lib.rtsh_combine(C.byref(constants), lp, _ptr(positions) if positions is not None else None, _ptr(normals),
                             _ptr(mask), W, H, _ptr(rgb)), "rtsh_combine")
    return rgb


def combine_device(ctx, constants, light, d_positions, d_normals, d_mask, width, height, d_rgb, stream=None):
    """Combine.frag on the GPU: device pointers, d_rgb = width*height*3 bytes, asynchronous."""
    lp = C.byref(light) if light is not None else None
    _check(_lib.rtsh_combine_device(ctx.handle, C.byref(constants), lp, C.c_void_p(d_positions or 0), C.c_void_p(d_normals),
                                    C.c_void_p(d_mask), width, height, C.c_void_p(d_rgb), C.c_void_p(stream or 0)),
           "rtsh_combine_device")


def facing_active(constants, light, positions, normals):
    """The facing mark on the host (rtsh_facing_active): ``uint8[H, W]``, 0 for the background and where N.L <= 0 -- the pixels whose
    shadow byte the combine pass cannot show -- and 1 elsewhere.  ``normals``: float32[H, W, 4]."""
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    active = np.zeros((H, W), np.uint8)
    lp = C.byref(light) if light is not None else None
    _check(_lib.rtsh_facing_active(C.byref(constants), lp, _ptr(positions) if positions is not None else None, _ptr(normals),
                                   W, H, _ptr(active)), "rtsh_facing_active")
    return active


def facing_active_device(ctx, constants, light, d_positions, d_normals, width, height, d_active, stream=None):
    """The facing mark on the GPU: device pointers, d_active = width*height bytes, asynchronous."""
    lp = C.byref(light) if light is not None else None
    _check(_lib.rtsh_facing_active_device(ctx.handle, C.byref(constants), lp, C.c_void_p(d_positions or 0), C.c_void_p(d_normals),
                                          width, height, C.c_void_p(d_active), C.c_void_p(stream or 0)),
           "rtsh_facing_active_device")


def rays_distance(packed, rays, threads=0):
    """Occluder distance of generic rays on the host (rtsh_rays_distance, no GPU): float32[n]."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    out = np.zeros(rays.shape[0], np.float32)
    _check(_lib.rtsh_rays_distance(_ptr(packed), packed.shape[0], _ptr(rays), rays.shape[0], _ptr(out), threads), "rtsh_rays_distance")
    return out


def shadow_distance(packed, constants, light, positions, width, height, active=None, row_begin=0, row_end=None, out=None, mask=None,
                    threads=0, want_mask=True):
    """Occluder distance of a frame's shadow rays on the host (rtsh_shadow_distance, no GPU): ``(float32[H, W], uint8[H, W])``
    (mask None with ``want_mask`` False).  ``out`` / ``mask``: arrays to write into (rows outside the range keep their contents)."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, active = _frame_inputs("shadow_distance", positions, width, height, active)
    row_end = height if row_end is None else row_end
    dist = out if out is not None else np.zeros((height, width), np.float32)
    if mask is None and want_mask:
        mask = np.zeros((height, width), np.uint8)
    _check(_lib.rtsh_shadow_distance(_ptr(packed), packed.shape[0], C.byref(constants), _ref(light), _ptr(positions),
                                     _ptr_or_none(active), width, height, row_begin, row_end, _ptr(dist),
                                     _ptr_or_none(mask), threads), "rtsh_shadow_distance")
    return dist, mask


def soft_distance(packed, constants, light, positions, width, height, active=None, row_begin=0, row_end=None, out=None, mask=None,
                  threads=0, want_mask=True):
    """Soft-shadow occluder distance on the host (rtsh_soft_distance, no GPU): ``(float32[H, W], uint8[H, W])`` -- the minimum of the
    light samples' distances and the number of unoccluded samples (mask None with ``want_mask`` False)."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, active = _frame_inputs("soft_distance", positions, width, height, active)
    row_end = height if row_end is None else row_end
    dist = out if out is not None else np.zeros((height, width), np.float32)
    if mask is None and want_mask:
        mask = np.zeros((height, width), np.uint8)
    _check(_lib.rtsh_soft_distance(_ptr(packed), packed.shape[0], C.byref(constants), _ref(light), _ptr(positions),
                                   _ptr_or_none(active), width, height, row_begin, row_end, _ptr(dist),
                                   _ptr_or_none(mask), threads), "rtsh_soft_distance")
    return dist, mask


def ambient_occlusion(packed, constants, ao, positions, normals, width, height, active=None, row_begin=0, row_end=None, out=None, threads=0):
    """Ambient occlusion on the host (rtsh_ambient_occlusion, no GPU): ``uint8[H, W]`` -- per pixel the number of the ``ao`` samples
    whose segment meets no triangle; 0 on the background and where ``active`` is 0.  ``out``: an array to write into."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, active = _frame_inputs("ambient_occlusion", positions, width, height, active)
    normals, _ = _frame_inputs("ambient_occlusion (normals)", normals, width, height)
    row_end = height if row_end is None else row_end
    counts = out if out is not None else np.zeros((height, width), np.uint8)
    _check(_lib.rtsh_ambient_occlusion(_ptr(packed), packed.shape[0], C.byref(constants), _ref(ao), _ptr(positions), _ptr(normals),
                                       _ptr_or_none(active), width, height, row_begin, row_end, _ptr(counts), threads),
           "rtsh_ambient_occlusion")
    return counts


def ambient_occlusion_adaptive(packed, constants, ao, positions, normals, width, height, probe, active=None, row_begin=0, row_end=None,
                               out=None, refined=None, threads=0, want_refined=True):
    """Adaptive ambient occlusion on the host (rtsh_ambient_occlusion_adaptive, no GPU): ``(uint8[H, W] counts, uint8[H, W] refined)``
    -- the first ``probe`` samples of every active, non-background pixel, the remaining ones only where they disagree (refined None
    with ``want_refined`` False)."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, active = _frame_inputs("ambient_occlusion_adaptive", positions, width, height, active)
    normals, _ = _frame_inputs("ambient_occlusion_adaptive (normals)", normals, width, height)
    row_end = height if row_end is None else row_end
    counts = out if out is not None else np.zeros((height, width), np.uint8)
    if refined is None and want_refined:
        refined = np.zeros((height, width), np.uint8)
    _check(_lib.rtsh_ambient_occlusion_adaptive(_ptr(packed), packed.shape[0], C.byref(constants), _ref(ao), _ptr(positions),
                                                _ptr(normals), _ptr_or_none(active), width, height, row_begin, row_end, probe,
                                                _ptr(counts), _ptr_or_none(refined), threads), "rtsh_ambient_occlusion_adaptive")
    return counts, refined


def ambient_occlusion_bent(packed, constants, ao, positions, normals, width, height, active=None, row_begin=0, row_end=None, out=None,
                           bent=None, threads=0, want_counts=True):
    """Bent normals on the host (rtsh_ambient_occlusion_bent, no GPU): ``(uint8[H, W] counts, float32[H, W, 4] bent)`` -- the AO count
    and, per pixel, the frame applied to the integer sum of the unoccluded samples' quantised directions, with the count in ``.w``
    (counts None with ``want_counts`` False)."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, active = _frame_inputs("ambient_occlusion_bent", positions, width, height, active)
    normals, _ = _frame_inputs("ambient_occlusion_bent (normals)", normals, width, height)
    row_end = height if row_end is None else row_end
    counts = out if out is not None else (np.zeros((height, width), np.uint8) if want_counts else None)
    if bent is None:
        bent = np.zeros((height, width, 4), np.float32)
    _check(_lib.rtsh_ambient_occlusion_bent(_ptr(packed), packed.shape[0], C.byref(constants), _ref(ao), _ptr(positions), _ptr(normals),
                                            _ptr_or_none(active), width, height, row_begin, row_end, _ptr_or_none(counts), _ptr(bent),
                                            threads), "rtsh_ambient_occlusion_bent")
    return counts, bent


def ambient_occlusion_distance(packed, constants, ao, falloff, positions, normals, width, height, active=None, row_begin=0, row_end=None,
                               out=None, distance=None, obscurance=None, threads=0, want_counts=True, want_distance=True,
                               want_obscurance=True):
    """AO distance and falloff on the host (rtsh_ambient_occlusion_distance, no GPU): ``(uint8[H, W] counts, float32[H, W] distance,
    uint16[H, W] obscurance)``, each None where its ``want_`` is False -- what ``ShadowContext.trace_ambient_occlusion_distance``
    returns, bit for bit."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, active = _frame_inputs("ambient_occlusion_distance", positions, width, height, active)
    normals, _ = _frame_inputs("ambient_occlusion_distance (normals)", normals, width, height)
    row_end = height if row_end is None else row_end
    counts = out if out is not None else (np.zeros((height, width), np.uint8) if want_counts else None)
    if distance is None and want_distance:
        distance = np.zeros((height, width), np.float32)
    if obscurance is None and want_obscurance:
        obscurance = np.zeros((height, width), np.uint16)
    _check(_lib.rtsh_ambient_occlusion_distance(_ptr(packed), packed.shape[0], C.byref(constants), _ref(ao), _ref(falloff), _ptr(positions),
                                                _ptr(normals), _ptr_or_none(active), width, height, row_begin, row_end,
                                                _ptr_or_none(counts), _ptr_or_none(distance), _ptr_or_none(obscurance), threads),
           "rtsh_ambient_occlusion_distance")
    return counts, distance, obscurance


def ao_rays(constants, ao, positions, normals, width, height, active=None):
    """The rays of an ambient occlusion trace as ``rts_ray`` records (rtsh_ao_rays): ``float32[H * W * n, 8]``, the ``n = ao.samples``
    rays of pixel ``p`` at rows ``p * n .. p * n + n - 1``; all zero for a background or inactive pixel.  What ``trace_rays`` takes."""
    positions, active = _frame_inputs("ao_rays", positions, width, height, active)
    normals, _ = _frame_inputs("ao_rays (normals)", normals, width, height)
    n = ao.samples if ao is not None else 1
    rays = np.zeros((width * height * n, 8), np.float32)
    _check(_lib.rtsh_ao_rays(C.byref(constants), _ref(ao), _ptr(positions), _ptr(normals), _ptr_or_none(active), width, height, _ptr(rays)),
           "rtsh_ao_rays")
    return rays


def shadow_mask_adaptive(packed, constants, light, positions, width, height, probe, active=None, row_begin=0, row_end=None, out=None,
                         refined=None, threads=0, want_refined=True):
    """The adaptive soft mask on the host (rtsh_shadow_mask_adaptive, no GPU): ``(uint8[H, W] mask, uint8[H, W] refined)`` -- the
    first ``probe`` samples of every active pixel, the remaining ones only where they disagree (refined None with ``want_refined``
    False)."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, active = _frame_inputs("shadow_mask_adaptive", positions, width, height, active)
    row_end = height if row_end is None else row_end
    mask = out if out is not None else np.zeros((height, width), np.uint8)
    if refined is None and want_refined:
        refined = np.zeros((height, width), np.uint8)
    _check(_lib.rtsh_shadow_mask_adaptive(_ptr(packed), packed.shape[0], C.byref(constants), _ref(light), _ptr(positions),
                                          _ptr_or_none(active), width, height, row_begin, row_end, probe, _ptr(mask),
                                          _ptr_or_none(refined), threads), "rtsh_shadow_mask_adaptive")
    return mask, refined


def light_list(packed, constants, lights, positions, width, height, lights_map=None, row_begin=0, row_end=None, out=None, threads=0):
    """A light list trace on the host (rtsh_light_list, no GPU): ``uint8[H, W]``, bit ``l`` = light ``l`` is unoccluded, where
    ``lights_map`` (None: everywhere) has bit ``l`` set."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, lights_map = _frame_inputs("light_list", positions, width, height, lights_map, "lights_map")
    row_end = height if row_end is None else row_end
    mask = out if out is not None else np.zeros((height, width), np.uint8)
    _check(_lib.rtsh_light_list(_ptr(packed), packed.shape[0], C.byref(constants), _ref(lights), _ptr(positions),
                                _ptr_or_none(lights_map), width, height, row_begin, row_end, _ptr(mask),
                                threads), "rtsh_light_list")
    return mask


def soft_light_list(packed, constants, lights, positions, width, height, lights_map=None, row_begin=0, row_end=None, out=None, threads=0):
    """A soft light list trace on the host (rtsh_soft_light_list, no GPU): ``uint8[count, H, W]``, plane ``l`` = the unoccluded
    samples of light ``l`` where ``lights_map`` (None: everywhere) has bit ``l`` set.  ``out``: at least ``count`` planes to write into."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, lights_map = _frame_inputs("soft_light_list", positions, width, height, lights_map, "lights_map")
    row_end = height if row_end is None else row_end
    counts = out if out is not None else np.zeros((lights.count if lights is not None else 1, height, width), np.uint8)
    _check(_lib.rtsh_soft_light_list(_ptr(packed), packed.shape[0], C.byref(constants), _ref(lights), _ptr(positions),
                                     _ptr_or_none(lights_map), width, height, row_begin, row_end, _ptr(counts),
                                     threads), "rtsh_soft_light_list")
    return counts


def soft_light_list_distance(packed, constants, lights, positions, width, height, lights_map=None, row_begin=0, row_end=None, out=None,
                             counts=None, threads=0, want_counts=True):
    """A soft light list distance trace on the host (rtsh_soft_light_list_distance, no GPU): ``(float32[count, H, W], uint8[count, H,
    W])`` -- per light the minimum of its samples' distances and the number of unoccluded ones where ``lights_map`` (None: everywhere)
    has bit ``l`` set, else +0 and 0 (counts None with ``want_counts`` False).  ``out`` / ``counts``: at least ``count`` planes."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, lights_map = _frame_inputs("soft_light_list_distance", positions, width, height, lights_map, "lights_map")
    row_end = height if row_end is None else row_end
    planes = lights.count if lights is not None else 1
    dist = out if out is not None else np.zeros((planes, height, width), np.float32)
    if counts is None and want_counts:
        counts = np.zeros((planes, height, width), np.uint8)
    _check(_lib.rtsh_soft_light_list_distance(_ptr(packed), packed.shape[0], C.byref(constants), _ref(lights), _ptr(positions),
                                              _ptr_or_none(lights_map), width, height, row_begin, row_end, _ptr_or_none(dist),
                                              _ptr_or_none(counts), threads), "rtsh_soft_light_list_distance")
    return dist, counts


def _probes(lights, probes, what="probes"):
    """``probes`` (None, or any sequence of ``lights.count`` integers) as the ``uint32`` array the C entry points read by value;
    ``tables`` travels the same way."""
    if probes is None:
        return None
    probes = [int(v) for v in probes]
    if lights is not None and len(probes) != lights.count:
        raise RtsError(1, what + ": one integer per light of the list")
    if any(v < 0 or v > 0xFFFFFFFF for v in probes):
        raise RtsError(1, what + ": unsigned 32-bit integers")
    return (C.c_uint32 * max(1, len(probes)))(*probes)


def soft_light_list_adaptive(packed, constants, lights, probes, positions, width, height, lights_map=None, row_begin=0, row_end=None,
                             out=None, refined=None, threads=0, want_refined=True, tables=None):
    """An adaptive soft light list trace on the host (rtsh_soft_light_list_adaptive, no GPU): ``(uint8[count, H, W] counts,
    uint8[H, W] refined)`` -- per light its first ``probes[l]`` samples, the remaining ones only where they disagree (``probes[l]`` 0:
    all of them); bit ``l`` of ``refined`` = light ``l`` took its full count there (None with ``want_refined`` False).  ``tables``:
    None, or per light the size of its per-pixel jitter table (0: none) -- rtsh_soft_light_list_jittered."""
    packed = np.ascontiguousarray(packed, np.uint32).reshape(-1, 4)
    positions, lights_map = _frame_inputs("soft_light_list_adaptive", positions, width, height, lights_map, "lights_map")
    row_end = height if row_end is None else row_end
    counts = out if out is not None else np.zeros((lights.count if lights is not None else 1, height, width), np.uint8)
    if refined is None and want_refined:
        refined = np.zeros((height, width), np.uint8)
    if tables is not None:
        _check(_lib.rtsh_soft_light_list_jittered(_ptr(packed), packed.shape[0], C.byref(constants), _ref(lights), _ptr(positions),
                                                  _ptr_or_none(lights_map), width, height, row_begin, row_end, _ptr(counts),
                                                  _probes(lights, probes), _probes(lights, tables, "tables"), _ptr_or_none(refined),
                                                  threads), "rtsh_soft_light_list_jittered")
        return counts, refined
    _check(_lib.rtsh_soft_light_list_adaptive(_ptr(packed), packed.shape[0], C.byref(constants), _ref(lights), _ptr(positions),
                                              _ptr_or_none(lights_map), width, height, row_begin, row_end, _ptr(counts),
                                              _probes(lights, probes), _ptr_or_none(refined), threads), "rtsh_soft_light_list_adaptive")
    return counts, refined


def facing_lights(constants, lights, positions, normals):
    """The light map of a light list on the host (rtsh_facing_lights): ``uint8[H, W]``, bit ``l`` = ``facing_active`` for light ``l``."""
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    lights_map = np.zeros((H, W), np.uint8)
    lp = C.byref(lights) if lights is not None else None
    _check(_lib.rtsh_facing_lights(C.byref(constants), lp, _ptr(positions) if positions is not None else None, _ptr(normals),
                                   W, H, _ptr(lights_map)), "rtsh_facing_lights")
    return lights_map


def facing_lights_device(ctx, constants, lights, d_positions, d_normals, width, height, d_lights_map, stream=None):
    """The light map on the GPU: device pointers, d_lights_map = width*height bytes, asynchronous."""
    lp = C.byref(lights) if lights is not None else None
    _check(_lib.rtsh_facing_lights_device(ctx.handle, C.byref(constants), lp, C.c_void_p(d_positions or 0), C.c_void_p(d_normals),
                                          width, height, C.c_void_p(d_lights_map), C.c_void_p(stream or 0)),
           "rtsh_facing_lights_device")


def _colors(lights, colors):
    """``colors`` (None: every light white, or ``count`` rows of 3 or 4 floats) as the host array of ``count * 4`` float32 the C
    entry points read by value."""
    if colors is None:
        return None
    colors = np.asarray(colors, np.float32)
    if colors.ndim != 2 or colors.shape[1] not in (3, 4) or (lights is not None and colors.shape[0] != lights.count):
        raise RtsError(1, "colors: one row of 3 (or 4) floats per light of the list")
    out = np.zeros((max(1, colors.shape[0]), 4), np.float32)
    out[:colors.shape[0], :colors.shape[1]] = colors
    return out


def _combine_list(fn, name, constants, lights, positions, normals, planes, lights_map, colors):
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    planes = np.ascontiguousarray(planes, np.uint8)
    lights_map = np.ascontiguousarray(lights_map, np.uint8) if lights_map is not None else None
    if planes.size < (lights.count if name.startswith("rtsh_combine_soft") and lights is not None else 1) * H * W or \
            (lights_map is not None and lights_map.size != H * W) or (positions is not None and positions.size != H * W * 4):
        raise RtsError(1, name + ": a buffer does not fit the frame of the normals")
    colors = _colors(lights, colors)
    rgb = np.zeros((H, W, 3), np.uint8)
    _check(fn(C.byref(constants), _ref(lights), _ptr_or_none(colors), _ptr_or_none(positions), _ptr(normals), _ptr_or_none(lights_map),
              _ptr(planes), W, H, _ptr(rgb)), name)
    return rgb


def combine_light_list(constants, light_list, positions, normals, mask, lights_map=None, colors=None):
    """The combine pass of a hard light list on the host (rtsh_combine_light_list): ``uint8[H, W, 3]`` -- every light's direct term
    over its bit of ``mask`` (rts_trace_light_list*'s), times its colour, summed in list order, plus one ambient term.  ``colors``:
    None (white), or one row of 3 floats per light; ``lights_map``: None, or ``uint8[H, W]`` (a light whose bit is clear adds nothing)."""
    return _combine_list(_lib.rtsh_combine_light_list, "rtsh_combine_light_list", constants, light_list, positions, normals, mask,
                         lights_map, colors)


def combine_soft_light_list(constants, lights, positions, normals, counts, lights_map=None, colors=None):
    """The combine pass of a soft light list on the host (rtsh_combine_soft_light_list): ``uint8[H, W, 3]`` -- light ``l``'s direct
    term over plane ``l`` of ``counts`` (``uint8[>= count, H, W]``, rts_trace_soft_light_list*'s) divided by its sample count."""
    return _combine_list(_lib.rtsh_combine_soft_light_list, "rtsh_combine_soft_light_list", constants, lights, positions, normals, counts,
                         lights_map, colors)


def combine_light_list_device(ctx, constants, light_list, d_positions, d_normals, d_mask, width, height, d_rgb, d_lights_map=None,
                              colors=None, stream=None):
    """The combine pass of a hard light list on the GPU: device pointers (``colors`` stays a host array), d_rgb = width*height*3
    bytes, one kernel, asynchronous."""
    colors = _colors(light_list, colors)
    _check(_lib.rtsh_combine_light_list_device(ctx.handle, C.byref(constants), _ref(light_list), _ptr_or_none(colors),
                                               C.c_void_p(d_positions or 0), C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0),
                                               C.c_void_p(d_mask), width, height, C.c_void_p(d_rgb), C.c_void_p(stream or 0)),
           "rtsh_combine_light_list_device")


def combine_soft_light_list_device(ctx, constants, lights, d_positions, d_normals, d_counts, width, height, d_rgb, d_lights_map=None,
                                   colors=None, stream=None):
    """The combine pass of a soft light list on the GPU: device pointers (``colors`` stays a host array), d_counts = count planes of
    width*height bytes, d_rgb = width*height*3 bytes, one kernel, asynchronous."""
    colors = _colors(lights, colors)
    _check(_lib.rtsh_combine_soft_light_list_device(ctx.handle, C.byref(constants), _ref(lights), _ptr_or_none(colors),
                                                    C.c_void_p(d_positions or 0), C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0),
                                                    C.c_void_p(d_counts), width, height, C.c_void_p(d_rgb), C.c_void_p(stream or 0)),
           "rtsh_combine_soft_light_list_device")


def _filter_list(soft, lights, params, positions, normals, planes, lights_map, distances, threads):
    name = "rtsh_filter_soft_light_list" if soft else "rtsh_filter_light_list"
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    count = lights.count if lights is not None and 1 <= lights.count <= 8 else 1
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    planes = np.ascontiguousarray(planes, np.uint8)
    lights_map = np.ascontiguousarray(lights_map, np.uint8) if lights_map is not None else None
    distances = np.ascontiguousarray(distances, np.float32) if distances is not None else None
    if planes.size < (count if soft else 1) * H * W or (lights_map is not None and lights_map.size != H * W) or \
            (positions is not None and positions.size != H * W * 4) or (distances is not None and distances.size < count * H * W):
        raise RtsError(1, name + ": a buffer does not fit the frame of the normals")
    visibility = np.zeros((count, H, W), np.float32)
    if soft:
        status = _lib.rtsh_filter_soft_light_list(_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals), _ptr_or_none(lights_map),
                                                  _ptr(planes), _ptr_or_none(distances), W, H, _ptr(visibility), threads)
    else:
        status = _lib.rtsh_filter_light_list(_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals), _ptr_or_none(lights_map),
                                             _ptr(planes), W, H, _ptr(visibility), threads)
    _check(status, name)
    return visibility


def filter_light_list(light_list, params, positions, normals, mask, lights_map=None, threads=0):
    """The filter of a hard light list's mask on the host (rtsh_filter_light_list): ``float32[count, H, W]``, plane ``l`` the
    edge-aware tent average of bit ``l`` of ``mask`` over the window of ``params`` (a ``FilterParams``)."""
    return _filter_list(False, light_list, params, positions, normals, mask, lights_map, None, threads)


def filter_soft_light_list(lights, params, positions, normals, counts, lights_map=None, distances=None, threads=0):
    """The filter of a soft light list's count planes on the host (rtsh_filter_soft_light_list): ``float32[count, H, W]`` visibility.
    ``distances``: None, or the ``float32[>= count, H, W]`` planes of a soft light list distance trace (the contact-hardening guide,
    with ``params.spread``)."""
    return _filter_list(True, lights, params, positions, normals, counts, lights_map, distances, threads)


def filter_light_list_device(ctx, light_list, params, d_positions, d_normals, d_mask, width, height, d_visibility, d_lights_map=None,
                             stream=None):
    """The filter of a hard light list's mask on the GPU: device pointers, d_visibility = count planes of width*height floats, one
    kernel, asynchronous."""
    _check(_lib.rtsh_filter_light_list_device(ctx.handle, _ref(light_list), _ref(params), C.c_void_p(d_positions or 0), C.c_void_p(d_normals),
                                              C.c_void_p(d_lights_map or 0), C.c_void_p(d_mask), width, height, C.c_void_p(d_visibility),
                                              C.c_void_p(stream or 0)), "rtsh_filter_light_list_device")


def filter_soft_light_list_device(ctx, lights, params, d_positions, d_normals, d_counts, width, height, d_visibility, d_lights_map=None,
                                  d_distances=None, stream=None):
    """The filter of a soft light list's count planes on the GPU: device pointers (d_distances: None, or the distance planes), one
    kernel, asynchronous."""
    _check(_lib.rtsh_filter_soft_light_list_device(ctx.handle, _ref(lights), _ref(params), C.c_void_p(d_positions or 0), C.c_void_p(d_normals),
                                                   C.c_void_p(d_lights_map or 0), C.c_void_p(d_counts), C.c_void_p(d_distances or 0), width,
                                                   height, C.c_void_p(d_visibility), C.c_void_p(stream or 0)),
           "rtsh_filter_soft_light_list_device")


def subsampled_size(width, height, phase_x=0, phase_y=0):
    """``(w, h)`` of the half-resolution frame of a ``width`` x ``height`` one in the given phase (rtsh_subsampled_size): the sampled
    pixels ``(2X + phase_x, 2Y + phase_y)`` inside the frame.  Refused (RtsError) where there is none."""
    w, h = C.c_uint32(0), C.c_uint32(0)
    _check(_lib.rtsh_subsampled_size(width, height, phase_x, phase_y, C.byref(w), C.byref(h)), "rtsh_subsampled_size")
    return int(w.value), int(h.value)


def _upsample_frame(name, params, positions, normals, lights_map):
    """The full-resolution G-buffer of the half-resolution passes, contiguous and checked: (positions, normals, lights_map, W, H, w, h)."""
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    positions = np.ascontiguousarray(positions, np.float32)
    lights_map = np.ascontiguousarray(lights_map, np.uint8) if lights_map is not None else None
    if normals.size != H * W * 4 or positions.size != H * W * 4 or (lights_map is not None and lights_map.size != H * W):
        raise RtsError(1, name + ": a buffer does not fit the frame of the normals")
    w, h = subsampled_size(W, H, params.phase_x, params.phase_y) if params is not None else (1, 1)
    return positions, normals, lights_map, W, H, w, h


def _upsample_low(name, w, h, lo_positions, lo_normals, lo_lights_map):
    lo_positions, lo_normals = np.ascontiguousarray(lo_positions, np.float32), np.ascontiguousarray(lo_normals, np.float32)
    lo_lights_map = np.ascontiguousarray(lo_lights_map, np.uint8) if lo_lights_map is not None else None
    if lo_positions.size != w * h * 4 or lo_normals.size != w * h * 4 or (lo_lights_map is not None and lo_lights_map.size != w * h):
        raise RtsError(1, name + ": a low-resolution buffer does not fit the subsampled frame")
    return lo_positions, lo_normals, lo_lights_map


def subsample_gbuffer(params, positions, normals, lights_map=None):
    """The half-resolution G-buffer of a frame on the host (rtsh_subsample_gbuffer): ``(float32[h, w, 4] positions, float32[h, w, 4]
    normals, uint8[h, w] lights_map or None)``, the texels of the pixels ``(2X + phase_x, 2Y + phase_y)`` of ``params`` (an
    ``UpsampleParams``)."""
    positions, normals, lights_map, W, H, w, h = _upsample_frame("rtsh_subsample_gbuffer", params, positions, normals, lights_map)
    lo_pos, lo_nrm = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    lo_map = np.zeros((h, w), np.uint8) if lights_map is not None else None
    _check(_lib.rtsh_subsample_gbuffer(_ref(params), _ptr(positions), _ptr(normals), _ptr_or_none(lights_map), W, H, _ptr(lo_pos), _ptr(lo_nrm),
                                       _ptr_or_none(lo_map)), "rtsh_subsample_gbuffer")
    return lo_pos, lo_nrm, lo_map


def subsample_gbuffer_device(ctx, params, d_positions, d_normals, width, height, d_lo_positions, d_lo_normals, d_lights_map=None,
                             d_lo_lights_map=None, stream=None):
    """The half-resolution G-buffer on the GPU: device pointers, the low-resolution buffers of ``subsampled_size`` texels, one kernel,
    asynchronous."""
    _check(_lib.rtsh_subsample_gbuffer_device(ctx.handle, _ref(params), C.c_void_p(d_positions), C.c_void_p(d_normals),
                                              C.c_void_p(d_lights_map or 0), width, height, C.c_void_p(d_lo_positions),
                                              C.c_void_p(d_lo_normals), C.c_void_p(d_lo_lights_map or 0), C.c_void_p(stream or 0)),
           "rtsh_subsample_gbuffer_device")


def upsample_retrace_map(count, params, positions, normals, lo_positions, lo_normals, lights_map=None, lo_lights_map=None, threads=0):
    """The retrace map of a half-resolution light list on the host (rtsh_upsample_retrace_map): ``uint8[H, W]``, bit ``l`` set where
    the pixel is active for light ``l``, not sampled, and no low-resolution tap is accepted for it -- the ``lights_map`` of the
    full-resolution trace that fills those pixels."""
    name = "rtsh_upsample_retrace_map"
    positions, normals, lights_map, W, H, w, h = _upsample_frame(name, params, positions, normals, lights_map)
    lo_positions, lo_normals, lo_lights_map = _upsample_low(name, w, h, lo_positions, lo_normals, lo_lights_map)
    retrace = np.zeros((H, W), np.uint8)
    _check(_lib.rtsh_upsample_retrace_map(count, _ref(params), _ptr(positions), _ptr(normals), _ptr_or_none(lights_map), _ptr(lo_positions),
                                          _ptr(lo_normals), _ptr_or_none(lo_lights_map), W, H, _ptr(retrace), threads), name)
    return retrace


def upsample_retrace_map_device(ctx, count, params, d_positions, d_normals, d_lo_positions, d_lo_normals, width, height, d_retrace,
                                d_lights_map=None, d_lo_lights_map=None, stream=None):
    """The retrace map on the GPU: device pointers, d_retrace = width*height bytes, one kernel, asynchronous."""
    _check(_lib.rtsh_upsample_retrace_map_device(ctx.handle, count, _ref(params), C.c_void_p(d_positions), C.c_void_p(d_normals),
                                                 C.c_void_p(d_lights_map or 0), C.c_void_p(d_lo_positions), C.c_void_p(d_lo_normals),
                                                 C.c_void_p(d_lo_lights_map or 0), width, height, C.c_void_p(d_retrace),
                                                 C.c_void_p(stream or 0)), "rtsh_upsample_retrace_map_device")


def _upsample_list(soft, lights, params, positions, normals, lo_positions, lo_normals, lo_planes, lights_map, lo_lights_map, keep, out,
                   threads):
    name = "rtsh_upsample_soft_light_list" if soft else "rtsh_upsample_light_list"
    positions, normals, lights_map, W, H, w, h = _upsample_frame(name, params, positions, normals, lights_map)
    lo_positions, lo_normals, lo_lights_map = _upsample_low(name, w, h, lo_positions, lo_normals, lo_lights_map)
    count = lights.count if lights is not None and 1 <= lights.count <= 8 else 1
    lo_planes = np.ascontiguousarray(lo_planes, np.uint8)
    keep = np.ascontiguousarray(keep, np.uint8) if keep is not None else None
    shape = (count, H, W) if soft else (H, W)
    if out is None:
        out = np.zeros(shape, np.uint8)
    if lo_planes.size < (count if soft else 1) * w * h or (keep is not None and keep.size != H * W) or out.dtype != np.uint8 or \
            not out.flags.c_contiguous or out.size < int(np.prod(shape)):
        raise RtsError(1, name + ": a buffer does not fit the frame")
    fn = _lib.rtsh_upsample_soft_light_list if soft else _lib.rtsh_upsample_light_list
    _check(fn(_ref(lights), _ref(params), _ptr(positions), _ptr(normals), _ptr_or_none(lights_map), _ptr(lo_positions), _ptr(lo_normals),
              _ptr_or_none(lo_lights_map), _ptr(lo_planes), _ptr_or_none(keep), W, H, _ptr(out), threads), name)
    return out


def upsample_soft_light_list(lights, params, positions, normals, lo_positions, lo_normals, lo_counts, lights_map=None, lo_lights_map=None,
                             keep=None, out=None, threads=0):
    """The full-resolution count planes of a soft light list traced at half resolution, on the host (rtsh_upsample_soft_light_list):
    ``uint8[count, H, W]`` from ``lo_counts`` (``uint8[count, h, w]``) by four geometry-tested integer-weighted taps.  ``keep``
    (``uint8[H, W]``, the retrace map) and ``out`` (the planes a masked full-resolution trace wrote): a (pixel, light) whose keep bit
    is set is left as ``out`` holds it."""
    return _upsample_list(True, lights, params, positions, normals, lo_positions, lo_normals, lo_counts, lights_map, lo_lights_map, keep, out,
                          threads)


def upsample_light_list(light_list, params, positions, normals, lo_positions, lo_normals, lo_mask, lights_map=None, lo_lights_map=None,
                        keep=None, out=None, threads=0):
    """The same for a hard light list (rtsh_upsample_light_list): ``uint8[H, W]``, bit ``l`` from bit ``l`` of ``lo_mask``."""
    return _upsample_list(False, light_list, params, positions, normals, lo_positions, lo_normals, lo_mask, lights_map, lo_lights_map, keep,
                          out, threads)


def _upsample_list_device(fn, name, ctx, lights, params, d_positions, d_normals, d_lo_positions, d_lo_normals, d_lo_planes, width, height,
                          d_planes, d_lights_map, d_lo_lights_map, d_keep, stream):
    _check(fn(ctx.handle, _ref(lights), _ref(params), C.c_void_p(d_positions), C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0),
              C.c_void_p(d_lo_positions), C.c_void_p(d_lo_normals), C.c_void_p(d_lo_lights_map or 0), C.c_void_p(d_lo_planes),
              C.c_void_p(d_keep or 0), width, height, C.c_void_p(d_planes), C.c_void_p(stream or 0)), name)


def upsample_soft_light_list_device(ctx, lights, params, d_positions, d_normals, d_lo_positions, d_lo_normals, d_lo_counts, width, height,
                                    d_counts, d_lights_map=None, d_lo_lights_map=None, d_keep=None, stream=None):
    """The upsample of a soft light list's count planes on the GPU: device pointers, d_counts = count planes of width*height bytes,
    written except where ``d_keep`` has the light's bit, one kernel, asynchronous."""
    _upsample_list_device(_lib.rtsh_upsample_soft_light_list_device, "rtsh_upsample_soft_light_list_device", ctx, lights, params, d_positions,
                          d_normals, d_lo_positions, d_lo_normals, d_lo_counts, width, height, d_counts, d_lights_map, d_lo_lights_map, d_keep,
                          stream)


def upsample_light_list_device(ctx, light_list, params, d_positions, d_normals, d_lo_positions, d_lo_normals, d_lo_mask, width, height,
                               d_mask, d_lights_map=None, d_lo_lights_map=None, d_keep=None, stream=None):
    """The upsample of a hard light list's mask on the GPU: device pointers, d_mask = width*height bytes, one kernel, asynchronous."""
    _upsample_list_device(_lib.rtsh_upsample_light_list_device, "rtsh_upsample_light_list_device", ctx, light_list, params, d_positions,
                          d_normals, d_lo_positions, d_lo_normals, d_lo_mask, width, height, d_mask, d_lights_map, d_lo_lights_map, d_keep,
                          stream)


def compact_scratch_bytes(width, height):
    """The bytes of ``d_scratch`` of ``compact_light_map_device`` (rtsh_compact_scratch_bytes); 0 for a frame it refuses."""
    return int(_lib.rtsh_compact_scratch_bytes(width, height))


def compact_light_map(count, lights_map, capacity=None, out=None):
    """The list of a light map's marked pixels on the host (rtsh_compact_light_map): ``(pixels, n)``.  ``lights_map``: ``uint8[H, W]``;
    a pixel is marked when its byte has a bit below ``count``.  ``pixels``: uint32 indices ``y * W + x`` in TILE ORDER (8 x 8 tiles
    row-major over the frame, pixels row-major inside a tile), the first ``min(n, capacity)`` of them written into ``out`` (an array
    of ``capacity`` uint32; made here, of ``capacity`` = W * H entries by default, and then returned cut to the entries written);
    ``n``: the marked pixels of the whole frame."""
    lights_map = np.ascontiguousarray(lights_map, np.uint8)
    if lights_map.ndim != 2:
        raise RtsError(1, "rtsh_compact_light_map: the map must be uint8[H, W]")
    H, W = lights_map.shape
    made = out is None
    if made:
        capacity = W * H if capacity is None else capacity
        out = np.zeros(max(int(capacity), 1), np.uint32)
    elif capacity is None:
        capacity = out.size
    if out.dtype != np.uint32 or not out.flags.c_contiguous or out.size < capacity:
        raise RtsError(1, "rtsh_compact_light_map: out must be contiguous uint32 of at least capacity entries")
    n = C.c_uint32(0)
    _check(_lib.rtsh_compact_light_map(count, _ptr(lights_map), W, H, _ptr(out), capacity, C.byref(n)), "rtsh_compact_light_map")
    n = int(n.value)
    return (out[:min(n, capacity)] if made else out), n


def compact_light_map_device(ctx, count, d_lights_map, width, height, d_pixels, capacity, d_n, d_scratch, stream=None):
    """The same on the GPU: device pointers, d_pixels = ``capacity`` uint32, d_n = one uint32, d_scratch = ``compact_scratch_bytes``
    bytes; ``COMPACT_NODES`` kernels, asynchronous, nothing read back."""
    _check(_lib.rtsh_compact_light_map_device(ctx.handle, count, C.c_void_p(d_lights_map or 0), width, height, C.c_void_p(d_pixels or 0),
                                              capacity, C.c_void_p(d_n or 0), C.c_void_p(d_scratch or 0), C.c_void_p(stream or 0)),
           "rtsh_compact_light_map_device")


def _sparse_twin(trace, count, hard, packed, constants, lights, positions, width, height, pixels, planes, lights_map, threads):
    """The host twin of a sparse trace: the block trace's twin under the map cut down to the listed pixels, merged into ``planes`` at
    the listed pairs alone."""
    n = width * height
    pixels = np.asarray(pixels, np.uint32).reshape(-1)
    listed = np.zeros(n, bool)
    listed[pixels[pixels < n]] = True
    below = (1 << count) - 1
    on = np.full(n, below, np.uint8) if lights_map is None else (np.ascontiguousarray(lights_map, np.uint8).reshape(-1) & below)
    on = np.where(listed, on, 0).astype(np.uint8)                       # an unlisted pixel sends no ray: its position is never read
    traced = trace(packed, constants, lights, positions, width, height, lights_map=on.reshape(height, width), threads=threads)
    if hard:
        flat, got = planes.reshape(-1), traced.reshape(-1)
        flat[:] = (flat & ~on) | (got & on)
    else:
        flat, got = planes.reshape(-1)[:count * n].reshape(count, n), traced.reshape(count, n)
        for l in range(count):
            sel = ((on >> l) & 1).astype(bool)
            flat[l][sel] = got[l][sel]
    return planes


def light_list_sparse(packed, constants, lights, positions, width, height, pixels, mask, lights_map=None, threads=0):
    """The sparse hard light list trace on the host (no GPU): ``api.light_list`` under the map, merged into ``mask`` (``uint8[H, W]``,
    contiguous, changed in place and returned) at bit ``l`` of the listed pixels with bit ``l`` of the map set; nothing else changes."""
    return _sparse_twin(light_list, lights.count, True, packed, constants, lights, positions, width, height, pixels, mask, lights_map, threads)


def soft_light_list_sparse(packed, constants, lights, positions, width, height, pixels, counts, lights_map=None, threads=0):
    """The sparse soft light list trace on the host (no GPU): ``api.soft_light_list`` under the map, merged into ``counts``
    (``uint8[count, H, W]``, contiguous, changed in place and returned) at the listed pairs alone."""
    return _sparse_twin(soft_light_list, lights.count, False, packed, constants, lights, positions, width, height, pixels, counts, lights_map,
                        threads)


def wide_filter_scratch_bytes(count, width, height):
    """The bytes of ``d_scratch`` of the wide filter's device forms (rtsh_wide_filter_scratch_bytes): 2 * count * width * height
    uint16."""
    return int(_lib.rtsh_wide_filter_scratch_bytes(count, width, height))


_NO_MOMENTS = object()


def _wide_filter_frame(name, lights, positions, normals, planes, plane_type, lights_map, per_light=True, moments=_NO_MOMENTS):
    """What the host forms of the wide filters share before their call: the buffers made contiguous in their types, checked against
    the frame of the normals, and the zeroed visibility.  ``planes``: the first pass's input, one plane per light unless ``per_light``
    is false (the one mask plane of a hard list).  Returns (positions, normals, planes, lights_map, moments, W, H, visibility)."""
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    count = lights.count if lights is not None and 1 <= lights.count <= 8 else 1
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    planes = np.ascontiguousarray(planes, plane_type)
    lights_map = np.ascontiguousarray(lights_map, np.uint8) if lights_map is not None else None
    if moments is not _NO_MOMENTS:
        mean, square, lengths = (np.ascontiguousarray(a, t) for a, t in zip(moments, (np.uint16, np.uint32, np.uint8)))
        moments = (mean, square, lengths)
    else:
        moments = ()
    if planes.size < (count if per_light else 1) * H * W or (lights_map is not None and lights_map.size != H * W) or \
            (positions is not None and positions.size != H * W * 4) or any(a.size < count * H * W for a in moments):
        raise RtsError(1, name + ": a buffer does not fit the frame of the normals")
    return positions, normals, planes, lights_map, moments, W, H, np.zeros((count, H, W), np.float32)


def _wide_filter_list(soft, lights, params, positions, normals, planes, lights_map, threads):
    name = "rtsh_wide_filter_soft_light_list" if soft else "rtsh_wide_filter_light_list"
    positions, normals, planes, lights_map, _, W, H, visibility = _wide_filter_frame(name, lights, positions, normals, planes, np.uint8,
                                                                                     lights_map, per_light=soft)
    fn = _lib.rtsh_wide_filter_soft_light_list if soft else _lib.rtsh_wide_filter_light_list
    _check(fn(_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals), _ptr_or_none(lights_map), _ptr(planes), W, H,
              _ptr(visibility), threads), name)
    return visibility


def wide_filter_light_list(light_list, params, positions, normals, mask, lights_map=None, threads=0):
    """The wide (a-trous) filter of a hard light list's mask on the host (rtsh_wide_filter_light_list): ``float32[count, H, W]``,
    plane ``l`` the edge-aware average of bit ``l`` of ``mask`` after ``params.passes`` passes (a ``WideFilterParams``)."""
    return _wide_filter_list(False, light_list, params, positions, normals, mask, lights_map, threads)


def wide_filter_soft_light_list(lights, params, positions, normals, counts, lights_map=None, threads=0):
    """The wide (a-trous) filter of a soft light list's count planes on the host (rtsh_wide_filter_soft_light_list):
    ``float32[count, H, W]`` visibility."""
    return _wide_filter_list(True, lights, params, positions, normals, counts, lights_map, threads)


def wide_filter_light_list_device(ctx, light_list, params, d_positions, d_normals, d_mask, width, height, d_visibility, d_scratch=None,
                                  d_lights_map=None, stream=None):
    """The wide filter of a hard light list's mask on the GPU: device pointers, d_visibility = count planes of width*height floats,
    d_scratch = ``wide_filter_scratch_bytes(count, width, height)`` bytes (None allowed for passes <= 1); max(1, passes) kernels,
    asynchronous."""
    _check(_lib.rtsh_wide_filter_light_list_device(ctx.handle, _ref(light_list), _ref(params), C.c_void_p(d_positions or 0),
                                                   C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0), C.c_void_p(d_mask), width, height,
                                                   C.c_void_p(d_visibility), C.c_void_p(d_scratch or 0), C.c_void_p(stream or 0)),
           "rtsh_wide_filter_light_list_device")


def wide_filter_soft_light_list_device(ctx, lights, params, d_positions, d_normals, d_counts, width, height, d_visibility, d_scratch=None,
                                       d_lights_map=None, stream=None):
    """The wide filter of a soft light list's count planes on the GPU: as ``wide_filter_light_list_device``, over the count planes."""
    _check(_lib.rtsh_wide_filter_soft_light_list_device(ctx.handle, _ref(lights), _ref(params), C.c_void_p(d_positions or 0),
                                                        C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0), C.c_void_p(d_counts), width,
                                                        height, C.c_void_p(d_visibility), C.c_void_p(d_scratch or 0),
                                                        C.c_void_p(stream or 0)),
           "rtsh_wide_filter_soft_light_list_device")


def wide_filter_bent_scratch_bytes(width, height):
    """The bytes of ``d_scratch`` of ``wide_filter_bent_device`` (rtsh_wide_filter_bent_scratch_bytes): 2 * width * height texels of 8
    bytes, aligned to 8."""
    return int(_lib.rtsh_wide_filter_bent_scratch_bytes(width, height))


def wide_filter_bent(params, nsamples, positions, normals, bent, active=None, threads=0):
    """The wide (a-trous) filter of a bent trace's plane on the host (rtsh_wide_filter_bent): ``(float32[H, W, 4] out, float32[H, W]
    ao)`` -- ``out.xyz`` the mean free direction per sample after ``params.passes`` passes (a ``WideFilterParams``) over 16-bit integer
    vectors, ``out.w`` the AO visibility, ``ao`` its copy.  ``nsamples``: the trace's sample count; ``bent``: ``float32[H, W, 4]``, any
    float; ``active``: ``uint8[H, W]`` or None."""
    name = "rtsh_wide_filter_bent"
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    bent = np.ascontiguousarray(bent, np.float32) if bent is not None else None
    active = np.ascontiguousarray(active, np.uint8) if active is not None else None
    if (positions is not None and positions.size != H * W * 4) or (bent is not None and bent.size != H * W * 4) or \
            (active is not None and active.size != H * W):
        raise RtsError(1, name + ": a buffer does not fit the frame of the normals")
    out, ao = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)
    _check(_lib.rtsh_wide_filter_bent(_ref(params), nsamples, _ptr_or_none(positions), _ptr(normals), _ptr_or_none(active), _ptr_or_none(bent),
                                      W, H, _ptr(out), _ptr(ao), threads), name)
    return out, ao


def wide_filter_bent_device(ctx, params, nsamples, d_positions, d_normals, d_bent, width, height, d_out, d_ao=None, d_scratch=None,
                            d_active=None, stream=None):
    """The wide filter of a bent trace's plane on the GPU: device pointers, d_bent and d_out = width*height RGBA32F (aligned to 16
    bytes), d_ao = width*height floats or None, d_scratch = ``wide_filter_bent_scratch_bytes(width, height)`` bytes aligned to 8 (None
    allowed for passes <= 1); max(1, passes) kernels, asynchronous."""
    _check(_lib.rtsh_wide_filter_bent_device(ctx.handle, _ref(params), nsamples, C.c_void_p(d_positions or 0), C.c_void_p(d_normals or 0),
                                             C.c_void_p(d_active or 0), C.c_void_p(d_bent or 0), width, height, C.c_void_p(d_out or 0),
                                             C.c_void_p(d_ao or 0), C.c_void_p(d_scratch or 0), C.c_void_p(stream or 0)),
           "rtsh_wide_filter_bent_device")


def wide_filter_bent_mean(params, nsamples, positions, normals, texels, active=None, threads=0):
    """The wide bent filter over the accumulated texels on the host (rtsh_wide_filter_bent_mean): ``wide_filter_bent`` with ``texels``,
    the ``uint64[H, W]`` plane of ``accumulate_bent`` for this frame, in the place of ``bent``; the same ``(out, ao)``."""
    name = "rtsh_wide_filter_bent_mean"
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    texels = np.ascontiguousarray(texels, np.uint64) if texels is not None else None
    active = np.ascontiguousarray(active, np.uint8) if active is not None else None
    if (positions is not None and positions.size != H * W * 4) or (texels is not None and texels.size != H * W) or \
            (active is not None and active.size != H * W):
        raise RtsError(1, name + ": a buffer does not fit the frame of the normals")
    out, ao = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)
    _check(_lib.rtsh_wide_filter_bent_mean(_ref(params), nsamples, _ptr_or_none(positions), _ptr(normals), _ptr_or_none(active),
                                           _ptr_or_none(texels), W, H, _ptr(out), _ptr(ao), threads), name)
    return out, ao


def wide_filter_bent_mean_device(ctx, params, nsamples, d_positions, d_normals, d_texels, width, height, d_out, d_ao=None, d_scratch=None,
                                 d_active=None, stream=None):
    """The wide bent filter over the accumulated texels on the GPU: ``wide_filter_bent_device`` with d_texels = width*height texels of 8
    bytes (aligned to 8; not d_out, d_ao, d_scratch or its second half) in the place of d_bent; max(1, passes) kernels, asynchronous."""
    _check(_lib.rtsh_wide_filter_bent_mean_device(ctx.handle, _ref(params), nsamples, C.c_void_p(d_positions or 0),
                                                  C.c_void_p(d_normals or 0), C.c_void_p(d_active or 0), C.c_void_p(d_texels or 0), width,
                                                  height, C.c_void_p(d_out or 0), C.c_void_p(d_ao or 0), C.c_void_p(d_scratch or 0),
                                                  C.c_void_p(stream or 0)), "rtsh_wide_filter_bent_mean_device")


def accumulate_bent(params, nsamples, positions, normals, bent, prev=None, active=None, motion=None, threads=0):
    """The temporal accumulation of the bent texel on the host (rtsh_accumulate_bent, rtsh_accumulate_bent_motion): ``(uint64[H, W]
    texels, uint8[H, W] lengths)``.  A texel is int16 x, y, z and uint16 V, lowest bits first.  ``params``: a ``TemporalParams`` (bit 0
    of ``reset_lights`` resets); ``nsamples``: the trace's sample count; ``bent``: this frame's ``float32[H, W, 4]``, any float;
    ``prev``: None on the first frame, else ``(prev_positions, prev_normals, prev_texels, prev_lengths)`` of the previous frame (its
    G-buffer and what this call returned for it); ``active``: ``uint8[H, W]`` or None; ``motion``: None, or ``(prev_points,
    prev_point_normals)`` of this frame's motion G-buffer pass for the motion form."""
    name = "rtsh_accumulate_bent" + ("_motion" if motion is not None else "")
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    bent = np.ascontiguousarray(bent, np.float32) if bent is not None else None
    active = np.ascontiguousarray(active, np.uint8) if active is not None else None
    fits = (positions is None or positions.size == H * W * 4) and (bent is None or bent.size == H * W * 4) and \
        (active is None or active.size == H * W)
    if prev is not None:
        prev = tuple(np.ascontiguousarray(a, t) for a, t in zip(prev, (np.float32, np.float32, np.uint64, np.uint8)))
        fits = fits and len(prev) == 4 and prev[0].size == H * W * 4 and prev[1].size == H * W * 4 and \
            all(a.size == H * W for a in prev[2:])
    if not fits:
        raise RtsError(1, name + ": a buffer does not fit the frame of the normals")
    texels, lengths = np.zeros((H, W), np.uint64), np.zeros((H, W), np.uint8)
    pp = [_ptr(a) for a in prev] if prev is not None else [None] * 4
    head = (_ref(params), nsamples, _ptr_or_none(positions), _ptr(normals), _ptr_or_none(active), _ptr_or_none(bent), *pp)
    if motion is not None:
        mp = _motion_planes(motion, H, W, name)
        _check(_lib.rtsh_accumulate_bent_motion(*head, _ptr_or_none(mp[0]), _ptr_or_none(mp[1]), W, H, _ptr(texels), _ptr(lengths), threads),
               name)
        return texels, lengths
    _check(_lib.rtsh_accumulate_bent(*head, W, H, _ptr(texels), _ptr(lengths), threads), name)
    return texels, lengths


def accumulate_bent_device(ctx, params, nsamples, d_positions, d_normals, d_bent, width, height, d_texels_out, d_lengths_out, d_prev=None,
                           d_active=None, d_motion=None, stream=None):
    """The accumulation of the bent texel on the GPU: device pointers; d_bent = width*height RGBA32F aligned to 16 bytes; d_texels_out =
    width*height texels of 8 bytes aligned to 8, d_lengths_out of bytes; ``d_prev``: None on the first frame, else the device pointers
    ``(prev_positions, prev_normals, prev_texels, prev_lengths)``, which the outputs may not be.  ``d_motion``: None, or the device
    pointers ``(prev_points, prev_point_normals)`` for the motion form.  One kernel, asynchronous."""
    pp = tuple(d_prev) if d_prev is not None else (0, 0, 0, 0)
    head = (ctx.handle, _ref(params), nsamples, C.c_void_p(d_positions or 0), C.c_void_p(d_normals or 0), C.c_void_p(d_active or 0),
            C.c_void_p(d_bent or 0), C.c_void_p(pp[0] or 0), C.c_void_p(pp[1] or 0), C.c_void_p(pp[2] or 0), C.c_void_p(pp[3] or 0))
    tail = (width, height, C.c_void_p(d_texels_out or 0), C.c_void_p(d_lengths_out or 0), C.c_void_p(stream or 0))
    if d_motion is not None:
        _check(_lib.rtsh_accumulate_bent_motion_device(*head, C.c_void_p(d_motion[0] or 0), C.c_void_p(d_motion[1] or 0), *tail),
               "rtsh_accumulate_bent_motion_device")
        return
    _check(_lib.rtsh_accumulate_bent_device(*head, *tail), "rtsh_accumulate_bent_device")


def wide_filter_guided_scratch_bytes(count, width, height):
    """The bytes of ``d_scratch`` of the guided wide filter's device form (rtsh_wide_filter_guided_scratch_bytes): 3 * count * width *
    height uint16 -- two ping-pong sets and the planes of the threshold."""
    return int(_lib.rtsh_wide_filter_guided_scratch_bytes(count, width, height))


def wide_guide_threshold(G, D, n, guide_k4):
    """``T`` of the guided wide filter from its parts (rtsh_wide_guide_threshold): min(65535, isqrt(guide_k4**2 * G // (16 * D * n)))."""
    return int(_lib.rtsh_wide_guide_threshold(G, D, n, guide_k4))


def wide_filter_guided_soft_light_list(lights, params, positions, normals, counts, lights_map=None, threads=0):
    """The variance-guided wide (a-trous) filter of a soft light list's count planes on the host
    (rtsh_wide_filter_guided_soft_light_list): ``float32[count, H, W]`` visibility; ``params`` a ``WideGuideParams``."""
    name = "rtsh_wide_filter_guided_soft_light_list"
    positions, normals, counts, lights_map, _, W, H, visibility = _wide_filter_frame(name, lights, positions, normals, counts, np.uint8,
                                                                                     lights_map)
    _check(_lib.rtsh_wide_filter_guided_soft_light_list(_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals),
                                                        _ptr_or_none(lights_map), _ptr(counts), W, H, _ptr(visibility), threads), name)
    return visibility


def wide_filter_guided_soft_light_list_device(ctx, lights, params, d_positions, d_normals, d_counts, width, height, d_visibility,
                                              d_scratch=None, d_lights_map=None, stream=None):
    """The variance-guided wide filter of a soft light list's count planes on the GPU: device pointers, d_visibility = count planes of
    width*height floats, d_scratch = ``wide_filter_guided_scratch_bytes(count, width, height)`` bytes (None allowed for passes <= 1);
    max(1, passes) kernels, asynchronous."""
    _check(_lib.rtsh_wide_filter_guided_soft_light_list_device(ctx.handle, _ref(lights), _ref(params), C.c_void_p(d_positions or 0),
                                                               C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0), C.c_void_p(d_counts),
                                                               width, height, C.c_void_p(d_visibility), C.c_void_p(d_scratch or 0),
                                                               C.c_void_p(stream or 0)),
           "rtsh_wide_filter_guided_soft_light_list_device")


def combine_visibility_list(constants, light_list, positions, normals, visibility, lights_map=None, colors=None):
    """The visibility combine on the host (rtsh_combine_visibility_list): ``uint8[H, W, 3]`` -- the list combine pass with plane ``l``
    of ``visibility`` (``float32[>= count, H, W]``, a filter's output) as light ``l``'s shadow factor.  ``light_list``: a ``LightList``
    (for a soft list: its ``hard_list()``)."""
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    visibility = np.ascontiguousarray(visibility, np.float32)
    lights_map = np.ascontiguousarray(lights_map, np.uint8) if lights_map is not None else None
    if visibility.size < (light_list.count if light_list is not None and light_list.count <= 8 else 1) * H * W or \
            (lights_map is not None and lights_map.size != H * W) or (positions is not None and positions.size != H * W * 4):
        raise RtsError(1, "rtsh_combine_visibility_list: a buffer does not fit the frame of the normals")
    colors = _colors(light_list, colors)
    rgb = np.zeros((H, W, 3), np.uint8)
    _check(_lib.rtsh_combine_visibility_list(C.byref(constants), _ref(light_list), _ptr_or_none(colors), _ptr_or_none(positions),
                                             _ptr(normals), _ptr_or_none(lights_map), _ptr(visibility), W, H, _ptr(rgb)),
           "rtsh_combine_visibility_list")
    return rgb


def combine_visibility_list_device(ctx, constants, light_list, d_positions, d_normals, d_visibility, width, height, d_rgb,
                                   d_lights_map=None, colors=None, stream=None):
    """The visibility combine on the GPU: device pointers (``colors`` stays a host array), d_visibility = count planes of width*height
    floats, d_rgb = width*height*3 bytes, one kernel, asynchronous."""
    colors = _colors(light_list, colors)
    _check(_lib.rtsh_combine_visibility_list_device(ctx.handle, C.byref(constants), _ref(light_list), _ptr_or_none(colors),
                                                    C.c_void_p(d_positions or 0), C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0),
                                                    C.c_void_p(d_visibility), width, height, C.c_void_p(d_rgb), C.c_void_p(stream or 0)),
           "rtsh_combine_visibility_list_device")


def combine_visibility_list_ao(constants, light_list, positions, normals, visibility, ao, lights_map=None, colors=None):
    """The visibility combine with ambient occlusion on the host (rtsh_combine_visibility_list_ao): ``combine_visibility_list`` with the
    ambient term of pixel ``p`` times ``ao[p]`` (``float32[H, W]``: a filtered AO count plane)."""
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    visibility = np.ascontiguousarray(visibility, np.float32)
    ao = np.ascontiguousarray(ao, np.float32) if ao is not None else None
    lights_map = np.ascontiguousarray(lights_map, np.uint8) if lights_map is not None else None
    if visibility.size < (light_list.count if light_list is not None and light_list.count <= 8 else 1) * H * W or \
            (lights_map is not None and lights_map.size != H * W) or (positions is not None and positions.size != H * W * 4) or \
            (ao is not None and ao.size != H * W):
        raise RtsError(1, "rtsh_combine_visibility_list_ao: a buffer does not fit the frame of the normals")
    colors = _colors(light_list, colors)
    rgb = np.zeros((H, W, 3), np.uint8)
    _check(_lib.rtsh_combine_visibility_list_ao(C.byref(constants), _ref(light_list), _ptr_or_none(colors), _ptr_or_none(positions),
                                                _ptr(normals), _ptr_or_none(lights_map), _ptr(visibility), _ptr_or_none(ao), W, H,
                                                _ptr(rgb)), "rtsh_combine_visibility_list_ao")
    return rgb


def combine_visibility_list_ao_device(ctx, constants, light_list, d_positions, d_normals, d_visibility, d_ao, width, height, d_rgb,
                                      d_lights_map=None, colors=None, stream=None):
    """The visibility combine with ambient occlusion on the GPU: ``combine_visibility_list_device`` plus d_ao = width*height floats; one
    kernel, asynchronous."""
    colors = _colors(light_list, colors)
    _check(_lib.rtsh_combine_visibility_list_ao_device(ctx.handle, C.byref(constants), _ref(light_list), _ptr_or_none(colors),
                                                       C.c_void_p(d_positions or 0), C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0),
                                                       C.c_void_p(d_visibility), C.c_void_p(d_ao or 0), width, height, C.c_void_p(d_rgb),
                                                       C.c_void_p(stream or 0)), "rtsh_combine_visibility_list_ao_device")


def combine_visibility_list_ao_bent(constants, light_list, positions, normals, visibility, ao, bent, sky, lights_map=None, colors=None):
    """The visibility combine with ambient occlusion and a sky on the host (rtsh_combine_visibility_list_ao_bent):
    ``combine_visibility_list_ao`` with the ambient term of pixel ``p`` tinted between ``sky.ground`` and ``sky.sky`` by where
    ``bent[p]`` (``float32[H, W, 4]``, a bent trace's plane) points relative to ``sky.up``."""
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    visibility = np.ascontiguousarray(visibility, np.float32)
    ao = np.ascontiguousarray(ao, np.float32) if ao is not None else None
    bent = np.ascontiguousarray(bent, np.float32) if bent is not None else None
    lights_map = np.ascontiguousarray(lights_map, np.uint8) if lights_map is not None else None
    if visibility.size < (light_list.count if light_list is not None and light_list.count <= 8 else 1) * H * W or \
            (lights_map is not None and lights_map.size != H * W) or (positions is not None and positions.size != H * W * 4) or \
            (ao is not None and ao.size != H * W) or (bent is not None and bent.size != H * W * 4):
        raise RtsError(1, "rtsh_combine_visibility_list_ao_bent: a buffer does not fit the frame of the normals")
    colors = _colors(light_list, colors)
    rgb = np.zeros((H, W, 3), np.uint8)
    _check(_lib.rtsh_combine_visibility_list_ao_bent(C.byref(constants), _ref(light_list), _ptr_or_none(colors), _ptr_or_none(positions),
                                                     _ptr(normals), _ptr_or_none(lights_map), _ptr(visibility), _ptr_or_none(ao),
                                                     _ptr_or_none(bent), _ref(sky), W, H, _ptr(rgb)),
           "rtsh_combine_visibility_list_ao_bent")
    return rgb


def combine_visibility_list_ao_bent_device(ctx, constants, light_list, d_positions, d_normals, d_visibility, d_ao, d_bent, sky, width,
                                           height, d_rgb, d_lights_map=None, colors=None, stream=None):
    """The visibility combine with ambient occlusion and a sky on the GPU: ``combine_visibility_list_ao_device`` plus d_bent =
    width*height RGBA32F and ``sky`` (a ``SkyAmbient``, by value); one kernel, asynchronous."""
    colors = _colors(light_list, colors)
    _check(_lib.rtsh_combine_visibility_list_ao_bent_device(ctx.handle, C.byref(constants), _ref(light_list), _ptr_or_none(colors),
                                                            C.c_void_p(d_positions or 0), C.c_void_p(d_normals),
                                                            C.c_void_p(d_lights_map or 0), C.c_void_p(d_visibility), C.c_void_p(d_ao or 0),
                                                            C.c_void_p(d_bent or 0), _ref(sky), width, height, C.c_void_p(d_rgb),
                                                            C.c_void_p(stream or 0)), "rtsh_combine_visibility_list_ao_bent_device")


def camera_basis(eye, target, fovy, width, height):
    """The camera the primary pass builds from (eye, target, fovy, width, height) (rtsh_camera_basis): a dict of float32 ``eye``,
    ``fwd``, ``right``, ``up`` (3 each), ``tan_half`` and ``aspect``."""
    e, t, out = np.asarray(eye, np.float32).copy(), np.asarray(target, np.float32).copy(), np.zeros(14, np.float32)
    if e.shape != (3,) or t.shape != (3,):
        raise RtsError(1, "rtsh_camera_basis: eye and target are 3 floats")
    _check(_lib.rtsh_camera_basis(_ptr(e), _ptr(t), C.c_float(fovy), width, height, _ptr(out)), "rtsh_camera_basis")
    return {"eye": out[0:3].copy(), "fwd": out[3:6].copy(), "right": out[6:9].copy(), "up": out[9:12].copy(), "tan_half": out[12],
            "aspect": out[13]}


def accumulate_visibility_list(light_list, params, positions, normals, visibility, prev=None, lights_map=None, threads=0, clamp=None,
                               motion=None):
    """The temporal accumulation of a light list's visibility on the host (rtsh_accumulate_visibility_list): ``(float32[count, H, W]
    visibility, uint8[count, H, W] lengths)``.  ``visibility``: this frame's ``float32[>= count, H, W]`` (a filter's output);
    ``prev``: None on the first frame, else ``(prev_positions, prev_normals, prev_visibility, prev_lengths)`` of the previous frame
    (its G-buffer and what this call returned for it); ``params`` a ``TemporalParams``.  ``clamp``: None, or a ``HistoryClamp`` for
    the clamped form (rtsh_accumulate_visibility_list_clamped).  ``motion``: None, or ``(prev_points, prev_point_normals)`` -- this frame's
    planes from :func:`primary_gbuffer_motion`, either of which may be None -- for the motion forms (rtsh_accumulate_visibility_list_motion,
    ..._clamped_motion)."""
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    count = light_list.count if light_list is not None and 1 <= light_list.count <= 8 else 1
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    visibility = np.ascontiguousarray(visibility, np.float32)
    lights_map = np.ascontiguousarray(lights_map, np.uint8) if lights_map is not None else None
    fits = visibility.size >= count * H * W and (lights_map is None or lights_map.size == H * W) and \
        (positions is None or positions.size == H * W * 4)
    if prev is not None:
        prev = (np.ascontiguousarray(prev[0], np.float32), np.ascontiguousarray(prev[1], np.float32), np.ascontiguousarray(prev[2], np.float32),
                np.ascontiguousarray(prev[3], np.uint8))
        fits = fits and prev[0].size == H * W * 4 and prev[1].size == H * W * 4 and prev[2].size >= count * H * W and prev[3].size >= count * H * W
    if not fits:
        raise RtsError(1, "rtsh_accumulate_visibility_list: a buffer does not fit the frame of the normals")
    out, lengths = np.zeros((count, H, W), np.float32), np.zeros((count, H, W), np.uint8)
    pp = [_ptr(a) for a in prev] if prev is not None else [None] * 4
    if motion is not None:
        name = "rtsh_accumulate_visibility_list_clamped_motion" if clamp is not None else "rtsh_accumulate_visibility_list_motion"
        mp = _motion_planes(motion, H, W, name)
        args = (_ref(light_list), _ref(params), _ptr_or_none(positions), _ptr(normals), _ptr_or_none(lights_map), _ptr(visibility), pp[0], pp[1],
                pp[2], pp[3], _ptr_or_none(mp[0]), _ptr_or_none(mp[1]), W, H, _ptr(out), _ptr(lengths))
        _check(getattr(_lib, name)(*args, *((_ref(clamp),) if clamp is not None else ()), threads), name)
        return out, lengths
    if clamp is not None:
        _check(_lib.rtsh_accumulate_visibility_list_clamped(_ref(light_list), _ref(params), _ptr_or_none(positions), _ptr(normals),
                                                            _ptr_or_none(lights_map), _ptr(visibility), pp[0], pp[1], pp[2], pp[3], W, H,
                                                            _ptr(out), _ptr(lengths), _ref(clamp), threads),
               "rtsh_accumulate_visibility_list_clamped")
        return out, lengths
    _check(_lib.rtsh_accumulate_visibility_list(_ref(light_list), _ref(params), _ptr_or_none(positions), _ptr(normals), _ptr_or_none(lights_map),
                                                _ptr(visibility), pp[0], pp[1], pp[2], pp[3], W, H, _ptr(out), _ptr(lengths), threads),
           "rtsh_accumulate_visibility_list")
    return out, lengths


def _motion_planes(motion, H, W, name):
    planes = tuple(np.ascontiguousarray(a, np.float32) if a is not None else None for a in motion)
    if len(planes) != 2 or any(a is not None and a.size != H * W * 4 for a in planes):
        raise RtsError(1, name + ": motion is (prev_points, prev_point_normals), W*H*4 floats each")
    return planes


def accumulate_visibility_list_device(ctx, light_list, params, d_positions, d_normals, d_visibility, width, height, d_visibility_out,
                                      d_lengths_out, d_prev=None, d_lights_map=None, stream=None, clamp=None, d_motion=None):
    """The temporal accumulation on the GPU: device pointers; ``d_prev``: None on the first frame, else the device pointers
    ``(prev_positions, prev_normals, prev_visibility, prev_lengths)``.  d_visibility_out = count planes of width*height floats,
    d_lengths_out = count planes of width*height bytes; neither may be the history it reads.  One kernel, asynchronous.  ``clamp``: None,
    or a ``HistoryClamp`` for the clamped form (then d_visibility_out may not be d_visibility either).  ``d_motion``: None, or the device
    pointers ``(prev_points, prev_point_normals)`` of this frame's motion G-buffer pass for the motion forms."""
    pp = tuple(d_prev) if d_prev is not None else (0, 0, 0, 0)
    if d_motion is not None:
        args = (ctx.handle, _ref(light_list), _ref(params), C.c_void_p(d_positions or 0), C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0),
                C.c_void_p(d_visibility), C.c_void_p(pp[0] or 0), C.c_void_p(pp[1] or 0), C.c_void_p(pp[2] or 0), C.c_void_p(pp[3] or 0),
                C.c_void_p(d_motion[0] or 0), C.c_void_p(d_motion[1] or 0), width, height, C.c_void_p(d_visibility_out),
                C.c_void_p(d_lengths_out))
        if clamp is not None:
            _check(_lib.rtsh_accumulate_visibility_list_clamped_motion_device(*args, _ref(clamp), C.c_void_p(stream or 0)),
                   "rtsh_accumulate_visibility_list_clamped_motion_device")
        else:
            _check(_lib.rtsh_accumulate_visibility_list_motion_device(*args, C.c_void_p(stream or 0)),
                   "rtsh_accumulate_visibility_list_motion_device")
        return
    if clamp is not None:
        _check(_lib.rtsh_accumulate_visibility_list_clamped_device(ctx.handle, _ref(light_list), _ref(params), C.c_void_p(d_positions or 0),
                                                                   C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0),
                                                                   C.c_void_p(d_visibility), C.c_void_p(pp[0] or 0), C.c_void_p(pp[1] or 0),
                                                                   C.c_void_p(pp[2] or 0), C.c_void_p(pp[3] or 0), width, height,
                                                                   C.c_void_p(d_visibility_out), C.c_void_p(d_lengths_out), _ref(clamp),
                                                                   C.c_void_p(stream or 0)),
               "rtsh_accumulate_visibility_list_clamped_device")
        return
    _check(_lib.rtsh_accumulate_visibility_list_device(ctx.handle, _ref(light_list), _ref(params), C.c_void_p(d_positions or 0),
                                                       C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0), C.c_void_p(d_visibility),
                                                       C.c_void_p(pp[0] or 0), C.c_void_p(pp[1] or 0), C.c_void_p(pp[2] or 0),
                                                       C.c_void_p(pp[3] or 0), width, height, C.c_void_p(d_visibility_out),
                                                       C.c_void_p(d_lengths_out), C.c_void_p(stream or 0)),
           "rtsh_accumulate_visibility_list_device")


def moments_clamp_bounds(m, S1, S2, lo, hi, sigma_k4, margin=0):
    """``(Lv', Hv')`` of the clamped moments pass from a window's parts (rtsh_moments_clamp_bounds): ``m`` contributing taps, ``S1`` the
    sum of their V_0, ``S2`` the sum of the squares, ``lo`` and ``hi`` their minimum and maximum."""
    lv, hv = C.c_uint32(0), C.c_uint32(0)
    _lib.rtsh_moments_clamp_bounds(m, S1, S2, lo, hi, sigma_k4, margin, C.byref(lv), C.byref(hv))
    return int(lv.value), int(hv.value)


def accumulate_moments_soft_light_list(lights, params, positions, normals, counts, prev=None, lights_map=None, threads=0, motion=None,
                                       clamp=None):
    """The temporal accumulation of a soft light list's count moments on the host (rtsh_accumulate_moments_soft_light_list):
    ``(uint16[count, H, W] mean, uint32[count, H, W] square, uint8[count, H, W] lengths)``.  ``counts``: this frame's
    ``uint8[>= count, H, W]``; ``prev``: None on the first frame, else ``(prev_positions, prev_normals, prev_mean, prev_square,
    prev_lengths)`` of the previous frame (its G-buffer and what this call returned for it); ``params`` a ``TemporalParams``.  ``motion``:
    None, or ``(prev_points, prev_point_normals)`` of this frame's motion G-buffer pass for the motion form.  ``clamp``: None, or a
    ``MomentsClamp`` for the clamped form (rtsh_accumulate_moments_soft_light_list_clamped, ..._clamped_motion)."""
    name = "rtsh_accumulate_moments_soft_light_list" + ("_clamped" if clamp is not None else "") + ("_motion" if motion is not None else "")
    normals = np.ascontiguousarray(normals, np.float32)
    H, W = normals.shape[:2]
    count = lights.count if lights is not None and 1 <= lights.count <= 8 else 1
    positions = np.ascontiguousarray(positions, np.float32) if positions is not None else None
    counts = np.ascontiguousarray(counts, np.uint8)
    lights_map = np.ascontiguousarray(lights_map, np.uint8) if lights_map is not None else None
    fits = counts.size >= count * H * W and (lights_map is None or lights_map.size == H * W) and \
        (positions is None or positions.size == H * W * 4)
    if prev is not None:
        prev = tuple(np.ascontiguousarray(a, t) for a, t in zip(prev, (np.float32, np.float32, np.uint16, np.uint32, np.uint8)))
        fits = fits and len(prev) == 5 and prev[0].size == H * W * 4 and prev[1].size == H * W * 4 and \
            all(a.size >= count * H * W for a in prev[2:])
    if not fits:
        raise RtsError(1, name + ": a buffer does not fit the frame of the normals")
    mean, square, lengths = np.zeros((count, H, W), np.uint16), np.zeros((count, H, W), np.uint32), np.zeros((count, H, W), np.uint8)
    pp = [_ptr(a) for a in prev] if prev is not None else [None] * 5
    if motion is not None:
        mp = _motion_planes(motion, H, W, name)
        args = (_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals), _ptr_or_none(lights_map), _ptr(counts), pp[0], pp[1], pp[2],
                pp[3], pp[4], _ptr_or_none(mp[0]), _ptr_or_none(mp[1]), W, H, _ptr(mean), _ptr(square), _ptr(lengths))
        if clamp is not None:
            _check(_lib.rtsh_accumulate_moments_soft_light_list_clamped_motion(*args, _ref(clamp), threads), name)
            return mean, square, lengths
        _check(_lib.rtsh_accumulate_moments_soft_light_list_motion(*args, threads), name)
        return mean, square, lengths
    if clamp is not None:
        _check(_lib.rtsh_accumulate_moments_soft_light_list_clamped(_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals),
                                                                    _ptr_or_none(lights_map), _ptr(counts), pp[0], pp[1], pp[2], pp[3], pp[4],
                                                                    W, H, _ptr(mean), _ptr(square), _ptr(lengths), _ref(clamp), threads), name)
        return mean, square, lengths
    _check(_lib.rtsh_accumulate_moments_soft_light_list(_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals),
                                                        _ptr_or_none(lights_map), _ptr(counts), pp[0], pp[1], pp[2], pp[3], pp[4], W, H,
                                                        _ptr(mean), _ptr(square), _ptr(lengths), threads), name)
    return mean, square, lengths


def accumulate_moments_soft_light_list_device(ctx, lights, params, d_positions, d_normals, d_counts, width, height, d_mean_out,
                                              d_square_out, d_lengths_out, d_prev=None, d_lights_map=None, stream=None, d_motion=None,
                                              clamp=None):
    """The moments pass on the GPU: device pointers; ``d_prev``: None on the first frame, else the device pointers ``(prev_positions,
    prev_normals, prev_mean, prev_square, prev_lengths)``.  d_mean_out = count planes of width*height uint16, d_square_out of uint32,
    d_lengths_out of bytes; none may be the history it reads.  One kernel, asynchronous.  ``d_motion``: None, or the device pointers
    ``(prev_points, prev_point_normals)`` of this frame's motion G-buffer pass for the motion form.  ``clamp``: None, or a
    ``MomentsClamp`` for the clamped forms (one kernel as well)."""
    pp = tuple(d_prev) if d_prev is not None else (0, 0, 0, 0, 0)
    if clamp is not None:
        name = "rtsh_accumulate_moments_soft_light_list_clamped" + ("_motion" if d_motion is not None else "") + "_device"
        motion = (C.c_void_p(d_motion[0] or 0), C.c_void_p(d_motion[1] or 0)) if d_motion is not None else ()
        _check(getattr(_lib, name)(
            ctx.handle, _ref(lights), _ref(params), C.c_void_p(d_positions or 0), C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0),
            C.c_void_p(d_counts), C.c_void_p(pp[0] or 0), C.c_void_p(pp[1] or 0), C.c_void_p(pp[2] or 0), C.c_void_p(pp[3] or 0),
            C.c_void_p(pp[4] or 0), *motion, width, height, C.c_void_p(d_mean_out), C.c_void_p(d_square_out), C.c_void_p(d_lengths_out),
            _ref(clamp), C.c_void_p(stream or 0)), name)
        return
    if d_motion is not None:
        _check(_lib.rtsh_accumulate_moments_soft_light_list_motion_device(
            ctx.handle, _ref(lights), _ref(params), C.c_void_p(d_positions or 0), C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0),
            C.c_void_p(d_counts), C.c_void_p(pp[0] or 0), C.c_void_p(pp[1] or 0), C.c_void_p(pp[2] or 0), C.c_void_p(pp[3] or 0),
            C.c_void_p(pp[4] or 0), C.c_void_p(d_motion[0] or 0), C.c_void_p(d_motion[1] or 0), width, height, C.c_void_p(d_mean_out),
            C.c_void_p(d_square_out), C.c_void_p(d_lengths_out), C.c_void_p(stream or 0)),
            "rtsh_accumulate_moments_soft_light_list_motion_device")
        return
    _check(_lib.rtsh_accumulate_moments_soft_light_list_device(ctx.handle, _ref(lights), _ref(params), C.c_void_p(d_positions or 0),
                                                               C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0), C.c_void_p(d_counts),
                                                               C.c_void_p(pp[0] or 0), C.c_void_p(pp[1] or 0), C.c_void_p(pp[2] or 0),
                                                               C.c_void_p(pp[3] or 0), C.c_void_p(pp[4] or 0), width, height,
                                                               C.c_void_p(d_mean_out), C.c_void_p(d_square_out), C.c_void_p(d_lengths_out),
                                                               C.c_void_p(stream or 0)),
           "rtsh_accumulate_moments_soft_light_list_device")


def wide_filter_guided_temporal_soft_light_list(lights, params, positions, normals, counts, moments, lights_map=None, threads=0):
    """The guided wide filter with a temporal threshold on the host (rtsh_wide_filter_guided_temporal_soft_light_list):
    ``float32[count, H, W]`` visibility.  ``params`` a ``WideGuideTemporalParams``; ``moments`` = ``(mean, square, lengths)`` of
    ``accumulate_moments_soft_light_list`` for this frame."""
    name = "rtsh_wide_filter_guided_temporal_soft_light_list"
    positions, normals, counts, lights_map, (mean, square, lengths), W, H, visibility = _wide_filter_frame(
        name, lights, positions, normals, counts, np.uint8, lights_map, moments=moments)
    _check(_lib.rtsh_wide_filter_guided_temporal_soft_light_list(_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals),
                                                                 _ptr_or_none(lights_map), _ptr(counts), _ptr(mean), _ptr(square),
                                                                 _ptr(lengths), W, H, _ptr(visibility), threads), name)
    return visibility


def wide_filter_guided_temporal_soft_light_list_device(ctx, lights, params, d_positions, d_normals, d_counts, d_moments, width, height,
                                                       d_visibility, d_scratch=None, d_lights_map=None, stream=None):
    """The guided wide filter with a temporal threshold on the GPU: device pointers, ``d_moments`` = ``(d_mean, d_square, d_lengths)``,
    d_scratch = ``wide_filter_guided_scratch_bytes(count, width, height)`` bytes (None allowed for passes <= 1); max(1, passes)
    kernels, asynchronous."""
    m = tuple(d_moments)
    _check(_lib.rtsh_wide_filter_guided_temporal_soft_light_list_device(ctx.handle, _ref(lights), _ref(params), C.c_void_p(d_positions or 0),
                                                                        C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0),
                                                                        C.c_void_p(d_counts), C.c_void_p(m[0] or 0), C.c_void_p(m[1] or 0),
                                                                        C.c_void_p(m[2] or 0), width, height, C.c_void_p(d_visibility),
                                                                        C.c_void_p(d_scratch or 0), C.c_void_p(stream or 0)),
           "rtsh_wide_filter_guided_temporal_soft_light_list_device")


def wide_filter_mean_soft_light_list(lights, params, positions, normals, mean, lights_map=None, threads=0):
    """The wide (a-trous) filter of a soft light list's ACCUMULATED MEAN on the host (rtsh_wide_filter_mean_soft_light_list):
    ``float32[count, H, W]`` visibility.  ``params`` a ``WideFilterParams``; ``mean`` = the ``uint16[count, H, W]`` mean planes of
    ``accumulate_moments_soft_light_list`` for this frame."""
    name = "rtsh_wide_filter_mean_soft_light_list"
    positions, normals, mean, lights_map, _, W, H, visibility = _wide_filter_frame(name, lights, positions, normals, mean, np.uint16,
                                                                                   lights_map)
    _check(_lib.rtsh_wide_filter_mean_soft_light_list(_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals),
                                                      _ptr_or_none(lights_map), _ptr(mean), W, H, _ptr(visibility), threads), name)
    return visibility


def wide_filter_mean_soft_light_list_device(ctx, lights, params, d_positions, d_normals, d_mean, width, height, d_visibility, d_scratch=None,
                                            d_lights_map=None, stream=None):
    """The wide filter of a soft light list's accumulated mean on the GPU: as ``wide_filter_soft_light_list_device``, over the uint16
    mean planes of the moments pass in the place of the count planes."""
    _check(_lib.rtsh_wide_filter_mean_soft_light_list_device(ctx.handle, _ref(lights), _ref(params), C.c_void_p(d_positions or 0),
                                                             C.c_void_p(d_normals), C.c_void_p(d_lights_map or 0), C.c_void_p(d_mean or 0),
                                                             width, height, C.c_void_p(d_visibility), C.c_void_p(d_scratch or 0),
                                                             C.c_void_p(stream or 0)),
           "rtsh_wide_filter_mean_soft_light_list_device")


def wide_filter_guided_temporal_mean_soft_light_list(lights, params, positions, normals, counts, moments, lights_map=None, threads=0):
    """The guided wide filter with a temporal threshold over the ACCUMULATED MEAN on the host
    (rtsh_wide_filter_guided_temporal_mean_soft_light_list): ``float32[count, H, W]`` visibility.  Arguments as for
    ``wide_filter_guided_temporal_soft_light_list``; the passes average ``moments[0]``, ``counts`` feeds the threshold's fallback."""
    name = "rtsh_wide_filter_guided_temporal_mean_soft_light_list"
    positions, normals, counts, lights_map, (mean, square, lengths), W, H, visibility = _wide_filter_frame(
        name, lights, positions, normals, counts, np.uint8, lights_map, moments=moments)
    _check(_lib.rtsh_wide_filter_guided_temporal_mean_soft_light_list(_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals),
                                                                      _ptr_or_none(lights_map), _ptr(counts), _ptr(mean), _ptr(square),
                                                                      _ptr(lengths), W, H, _ptr(visibility), threads), name)
    return visibility


def wide_filter_guided_temporal_mean_soft_light_list_device(ctx, lights, params, d_positions, d_normals, d_counts, d_moments, width, height,
                                                            d_visibility, d_scratch=None, d_lights_map=None, stream=None):
    """The guided mean filter on the GPU: arguments as for ``wide_filter_guided_temporal_soft_light_list_device``; max(1, passes)
    kernels, asynchronous."""
    m = tuple(d_moments)
    _check(_lib.rtsh_wide_filter_guided_temporal_mean_soft_light_list_device(ctx.handle, _ref(lights), _ref(params),
                                                                             C.c_void_p(d_positions or 0), C.c_void_p(d_normals),
                                                                             C.c_void_p(d_lights_map or 0), C.c_void_p(d_counts or 0),
                                                                             C.c_void_p(m[0] or 0), C.c_void_p(m[1] or 0), C.c_void_p(m[2] or 0),
                                                                             width, height, C.c_void_p(d_visibility),
                                                                             C.c_void_p(d_scratch or 0), C.c_void_p(stream or 0)),
           "rtsh_wide_filter_guided_temporal_mean_soft_light_list_device")


def wide_filter_propagated_scratch_bytes(count, width, height):
    """The bytes of ``d_scratch`` of the propagated filter's device form (rtsh_wide_filter_propagated_scratch_bytes): 12 * count * width *
    height -- two ping-pong sets of uint16 values, then two of uint32 variance."""
    return int(_lib.rtsh_wide_filter_propagated_scratch_bytes(count, width, height))


def wide_variance_step(num_q, den):
    """``Q_(k+1) = (2 * num_q + den^2) // (2 * den^2)`` as host twin and kernels evaluate it (rtsh_wide_variance_step)."""
    return int(_lib.rtsh_wide_variance_step(int(num_q), int(den)))


def wide_filter_propagated_mean_soft_light_list(lights, params, positions, normals, counts, moments, lights_map=None, threads=0):
    """The guided mean filter with a variance plane carried through the passes, on the host
    (rtsh_wide_filter_propagated_mean_soft_light_list): ``float32[count, H, W]`` visibility.  ``params`` a
    ``WideGuidePropagatedParams``; the other arguments as for ``wide_filter_guided_temporal_mean_soft_light_list``."""
    name = "rtsh_wide_filter_propagated_mean_soft_light_list"
    positions, normals, counts, lights_map, (mean, square, lengths), W, H, visibility = _wide_filter_frame(
        name, lights, positions, normals, counts, np.uint8, lights_map, moments=moments)
    _check(_lib.rtsh_wide_filter_propagated_mean_soft_light_list(_ref(lights), _ref(params), _ptr_or_none(positions), _ptr(normals),
                                                                 _ptr_or_none(lights_map), _ptr(counts), _ptr(mean), _ptr(square),
                                                                 _ptr(lengths), W, H, _ptr(visibility), threads), name)
    return visibility


def wide_filter_propagated_mean_soft_light_list_device(ctx, lights, params, d_positions, d_normals, d_counts, d_moments, width, height,
                                                       d_visibility, d_scratch=None, d_lights_map=None, stream=None):
    """The propagated filter on the GPU: arguments as for ``wide_filter_guided_temporal_mean_soft_light_list_device``; d_scratch =
    ``wide_filter_propagated_scratch_bytes(count, width, height)`` bytes on a 4-byte boundary (None allowed for passes <= 1);
    max(1, passes) kernels, asynchronous."""
    m = tuple(d_moments)
    _check(_lib.rtsh_wide_filter_propagated_mean_soft_light_list_device(ctx.handle, _ref(lights), _ref(params),
                                                                        C.c_void_p(d_positions or 0), C.c_void_p(d_normals),
                                                                        C.c_void_p(d_lights_map or 0), C.c_void_p(d_counts or 0),
                                                                        C.c_void_p(m[0] or 0), C.c_void_p(m[1] or 0), C.c_void_p(m[2] or 0),
                                                                        width, height, C.c_void_p(d_visibility),
                                                                        C.c_void_p(d_scratch or 0), C.c_void_p(stream or 0)),
           "rtsh_wide_filter_propagated_mean_soft_light_list_device")


def write_ppm(path, rgb):
    """Binary PPM (P6) image dump."""
    H, W, _ = rgb.shape
    with open(path, "wb") as fh:
        fh.write(f"P6\n{W} {H}\n255\n".encode())
        fh.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
    return path


_BLOB_MAGIC = b"RTSBVH01"


def save_bvh(path, packed):
    """Serialises a packed node stream (cacheable scenes): magic, vec4 count, raw little-endian bytes."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32).reshape(-1, 4)
    bvh_validate(packed)
    with open(path, "wb") as fh:
        fh.write(_BLOB_MAGIC)
        fh.write(np.array([packed.shape[0]], np.uint64).tobytes())
        fh.write(packed.tobytes())
    return path


def load_bvh(path):
    with open(path, "rb") as fh:
        if fh.read(8) != _BLOB_MAGIC:
            raise RtsError(5, f"load_bvh: {path} is not a packed-BVH blob")
        n = int(np.frombuffer(fh.read(8), np.uint64)[0])
        packed = np.frombuffer(fh.read(n * 16), np.uint32).reshape(-1, 4).copy()
    if packed.shape[0] != n:
        raise RtsError(5, f"load_bvh: {path} is truncated")
    bvh_validate(packed)
    return packed


def obj_load(path):
    """OBJ -> flat ``float32[3T, 8]`` Vertex stream + ``indices[i] = i`` (loadModel semantics)."""
    n = C.c_uint32(0)
    _check(_lib.rtsh_obj_load(path.encode(), None, 0, C.byref(n), None, None), "rtsh_obj_load")
    verts = np.zeros((max(n.value, 1), 8), dtype=np.float32)
    lo = (C.c_float * 3)()
    hi = (C.c_float * 3)()
    _check(_lib.rtsh_obj_load(path.encode(), _ptr(verts), verts.shape[0], C.byref(n), lo, hi), "rtsh_obj_load")
    verts = verts[:n.value]
    return verts, np.arange(n.value, dtype=np.uint32), np.array(lo[:], np.float32), np.array(hi[:], np.float32)


def obj_parse_float(text):
    used = C.c_int(0)
    v = _lib.rtsh_obj_parse_float(text.encode(), C.byref(used))
    return np.float32(v), int(used.value)
