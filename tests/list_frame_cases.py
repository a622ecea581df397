"""Shared by the whole-frame tests (tests/test_list_frame_host.py, tests/test_gpu_list_frame.py): the renderer's light-list frame loop
(tools/render.py, soft_list_temporal and HalfRes.trace, which are the specification; nothing is imported from them) stated ONCE as an
ordered list of stages per recipe, and a runner that executes the same list either through the ``*_device`` wrappers of
raytracedshadows_amd/api.py on a context and a stream, or through the host twins over the numpy arrays of the previous stage.

Setup of every recipe: scenes.cornell() at 61 x 37 (odd both ways: partial 16 x 16, 32 x 8 and 8 x 8 blocks), FRAMES = 4 frames, the tall
box moving through the vertex stream by a third of list_motion_cases.T per frame, the eye turning ORBIT_DEG degrees per frame around
the target (the last frame is the scene's own camera, as in render.py), thresholds 0.9 / 0.05 in every stage, max_length 8.

Every frame begins  snapshot -> refit -> (frame 0: snapshot again, it has no previous stream but its own) -> motion G-buffer -> facing
map, and ends with combine_visibility_list.  Between them:

  A "everything"   subsample (phase (f & 1, (f >> 1) & 1)), jittered adaptive trace at w x h (3 lights: POINT 4 samples probe 2 table 8,
                   DIRECTIONAL hard, POINT 16 samples probe 4 table 24; the shared offsets rolled by one entry per frame), retrace map,
                   the same trace at W x H under the retrace map, upsample with keep = that map, moments clamped + motion
                   (MomentsClamp 2, 8, 1), propagated mean filter (3 passes, k4 12, min_history 2, by_length 1).
  B "no retrace"   subsample (phase (1, 1)), plain soft trace of 8 lights at w x h, upsample without keep (fallback pixels), moments
                   motion unclamped, guided temporal mean filter of 5 passes (k4 12, min_history 2).
  C "hard"         hard list of 8 lights traced at full resolution under the facing map, wide_filter_light_list of 2 passes,
                   accumulate_visibility_list clamped (radius 2, margin 0.05) + motion over the filtered planes; the combine reads the
                   accumulated planes.

SUBSTITUTIONS.  (1) render.py's command line refuses --half-res together with --adaptive / --table, and include/rts_scene.h lists the
adaptive and jittered forms as out of scope of the half-resolution passes (a jitter hash takes the index in the frame traced).  The
wrappers' argument lists allow the combination -- the upsample takes any count planes -- and both runners hash the same index, so
recipe A traces as the table of the issue asks; HalfRes.trace's stage order and arguments are kept.  (2) render.py combines the last
frame only; here every frame is combined, so that every frame has an image to compare.  (3) rts_ctx_refit_bvh_device runs on the
default stream, and a stream of rts_stream_create does not wait for that one: the eager runner issues the snapshot on the default
stream too (render.py's reading: it issues everything there), every other stage on the stream under test.  (4) A refit cannot be
captured, so a captured frame is  G-buffer ... combine -> snapshot  with the refit between two replays: the snapshot at the END of
frame k leaves stream k for frame k + 1, the data flow of render.py's order.  The captured chain is one eager frame 0 (no history) and
then FRAMES replayed frames, camera, phase and jitter rotation held fixed.

EXCLUDED BYTES: none of the compared planes.  Where a stage's rule says a byte "may hold anything" it speaks of an INPUT it does not
read (include/rts_scene.h: "n all zero (background): ... nothing else of p is looked at (position, map byte and plane bytes may hold
anything)"; include/rts.h: "Inactive positions may hold anything"); every OUTPUT byte of every stage used here is defined (a trace
writes 0 where the map's bit is clear, the filters and accumulates write +0 and 0 at inactive pairs, the upsample leaves a kept byte
to the masked trace, which wrote it).  Not compared, because no rule defines them: the filters' scratch, the bytes of the
low-resolution buffers beyond w * h texels (the buffers are sized for the largest phase; they must keep their preset), and planes
from `count` up (they must keep their preset too)."""
import numpy as np

import list_motion_cases as ms
from raytracedshadows_amd import api, scenes

f32, u32 = np.float32, np.uint32
W, H, FRAMES = 61, 37, 4
N = W * H
LO = ((W + 1) // 2) * ((H + 1) // 2)                      # the largest of the four phases' frames
NORMAL_COS, PLANE_EPS, MAX_LENGTH = 0.9, 0.05, 8
#: one degree: with two, every pixel the moving box resets is one the camera's own parallax resets too (the host test's census)
ORBIT_DEG = 1.0
FIXED_PHASE = (1, 0)
RING = [(5.0, 9.5, 5.0), (2.0, 9.0, 8.0), (7.5, 8.5, 7.0), (3.0, 8.0, 6.0), (6.5, 9.0, 3.0), (8.0, 7.5, 8.5), (1.5, 7.0, 4.0), (5.0, 6.5, 9.0)]
SUN = (0.3, 1.0, 0.2)
OFFSETS = scenes.jitter_offsets(48, 1.0, 19)
PRESET_DEVICE, PRESET_HOST = 0xAB, 0x5A


class Recipe:
    def __init__(self, name, count, stages, **kw):
        self.name, self.count, self.stages = name, count, stages
        self.half = kw.get("half")                        # None, or (retrace, phase or None: rotating)
        self.colors = np.array([[0.9, 0.5, 0.3], [0.2, 0.6, 0.9], [0.5, 0.5, 0.5], [0.3, 0.9, 0.4], [0.8, 0.2, 0.7], [0.6, 0.6, 0.1],
                                [0.1, 0.4, 0.8], [0.7, 0.7, 0.7]], f32)[:count] * f32(2.0 / count)


HEAD = ["snapshot", "refit", "resnapshot", "gbuffer", "facing"]
RECIPES = {
    "A": Recipe("A", 3, HEAD + ["subsample", "trace_lo", "retrace_map", "trace_masked", "upsample", "moments", "filter", "combine"],
                half=(True, None)),
    "B": Recipe("B", 8, HEAD + ["subsample", "trace_lo", "upsample", "moments", "filter", "combine"], half=(False, (1, 1))),
    "C": Recipe("C", 8, HEAD + ["trace_full", "filter", "accumulate", "combine"]),
}
#: the planes compared after every frame, per recipe (a name of the runner's state; ping-ponged ones are this frame's)
GBUFFER = ["snap", "pos", "nrm", "pts", "pnr", "map"]
PLANES = {
    "A": GBUFFER + ["lpos", "lnrm", "lmap", "lo", "keep", "counts", "mean", "square", "mlen", "vis", "rgb"],
    "B": GBUFFER + ["lpos", "lnrm", "lmap", "lo", "counts", "mean", "square", "mlen", "vis", "rgb"],
    "C": GBUFFER + ["mask", "vis", "hvis", "hlen", "rgb"],
}
#: what the presets of a frame cover: written by the frame before anything reads it
PRESETS = {"A": ["counts", "lo", "lpos", "lnrm", "lmap", "keep", "vis", "rgb"], "B": ["counts", "lo", "lpos", "lnrm", "lmap", "vis", "rgb"],
           "C": ["mask", "vis", "rgb"]}


def captured_stages(R):
    """The stage list of a captured frame: see SUBSTITUTIONS (4)."""
    return [s for s in R.stages if s not in ("snapshot", "refit", "resnapshot")] + ["snapshot"]


# ------------------------------------------------------------------------------------------------------------ the scene and a frame
_CACHE = {}


def geometry():
    """dict(packed, idx, P, vid, verts, eye, target, fovy, nvec4): the cornell room of list_motion_cases and its static stream."""
    if "geometry" not in _CACHE:
        sc, s = ms._scene("cornell"), ms.streams("cornell", "static")
        _CACHE["geometry"] = dict(packed=s["packed"], idx=np.ascontiguousarray(sc["faces"].reshape(-1)), P=sc["faces"].shape[0],
                                  vid=np.unique(sc["faces"][sc["part"]]), verts=sc["verts"], eye=s["eye"], target=s["target"], fovy=s["fovy"],
                                  nvec4=s["packed"].shape[0])
    return _CACHE["geometry"]


def vertices(k, still_box=False):
    g = geometry()
    v = g["verts"].copy()
    if not still_box:
        v[g["vid"]] += ms.T * (k / 3.0)
    return np.ascontiguousarray(v, f32)


def eye_of(k, fixed=False):
    """The eye of frame k: turned about the vertical axis through the target, the last frame the scene's own camera."""
    g = geometry()
    if fixed:
        return g["eye"].copy()
    a = np.deg2rad(ORBIT_DEG * (k - (FRAMES - 1)))
    d = g["eye"].astype(np.float64) - g["target"].astype(np.float64)
    x, z = np.cos(a) * d[0] + np.sin(a) * d[2], -np.sin(a) * d[0] + np.cos(a) * d[2]
    return (g["target"].astype(np.float64) + np.array([x, d[1], z])).astype(f32)


class Frame:
    """Everything frame k passes by value: cameras, constants, the lists, the params of every stage, the vertex stream."""

    def __init__(self, R, k, fixed=False, still_box=False):
        g = geometry()
        self.k, self.first, self.c, self.o = k, k == 0, str(k % 2), str(1 - k % 2)
        self.eye, self.prev_eye = eye_of(k, fixed), eye_of(max(k - 1, 0), fixed)
        self.target, self.fovy = g["target"], g["fovy"]
        self.verts = vertices(k, still_box)
        roll = 0 if fixed else k
        table = np.ascontiguousarray(np.roll(OFFSETS, -roll, axis=0))
        self.probes = self.tables = None
        if R.name == "A":
            self.lights = api.SoftLightList.make([(api.Light.POINT, RING[0], 4, 0, 0.8), (api.Light.DIRECTIONAL, SUN),
                                                  (api.Light.POINT, RING[1], 16, 8, 0.6)], table)
            self.probes, self.tables = (2, 0, 4), (8, 0, 24)
        elif R.name == "B":
            n = (4, 2, 6, 1, 4, 3, 8, 4)
            first = np.concatenate([[0], np.cumsum(n)[:-1]])
            self.lights = api.SoftLightList.make([(api.Light.DIRECTIONAL if l == 5 else api.Light.POINT, SUN if l == 5 else RING[l], n[l],
                                                   int(first[l]), 0.5 + 0.1 * l) for l in range(8)], table)
        else:
            self.lights = api.LightList.make([(api.Light.DIRECTIONAL, SUN) if l == 2 else
                                              (api.Light.DIRECTIONAL, (-0.4, 1.0, 0.3)) if l == 6 else (api.Light.POINT, RING[l]) for l in range(8)])
        self.hard = self.lights.hard_list() if R.name != "C" else self.lights
        self.constants = api.RayTracingConstants.make(self.eye, SUN, W, H)
        self.tp = api.TemporalParams.from_cameras((self.eye, self.target, self.fovy), (self.prev_eye, self.target, self.fovy), W, H,
                                                  NORMAL_COS, PLANE_EPS, MAX_LENGTH)
        self.colors = R.colors.copy()
        self.up = self.w = self.h = None
        if R.half is not None:
            px, py = R.half[1] if R.half[1] is not None else (FIXED_PHASE if fixed else (k & 1, (k >> 1) & 1))
            self.up = api.UpsampleParams.make(px, py, NORMAL_COS, PLANE_EPS)
            self.w, self.h = api.subsampled_size(W, H, px, py)
        self.moments_clamp = api.MomentsClamp.make(2, 8, 1) if R.name == "A" else None
        self.history_clamp = api.HistoryClamp.make(2, 0.05) if R.name == "C" else None
        self.filter = {"A": api.WideGuidePropagatedParams.make(3, 12, 2, 1, NORMAL_COS, PLANE_EPS),
                       "B": api.WideGuideTemporalParams.make(5, 12, 2, NORMAL_COS, PLANE_EPS),
                       "C": api.WideFilterParams.make(2, NORMAL_COS, PLANE_EPS)}[R.name]

    def structs(self):
        """Every host struct and array a stage reads by value (what a test overwrites after a capture)."""
        return [s for s in (self.constants, self.lights, self.hard, self.tp, self.up, self.moments_clamp, self.history_clamp, self.filter)
                if s is not None]


def scratch_bytes(R):
    return {"A": api.wide_filter_propagated_scratch_bytes, "B": api.wide_filter_guided_scratch_bytes,
            "C": api.wide_filter_scratch_bytes}[R.name](R.count, W, H)


# ------------------------------------------------------------------------------------------------------------ the stages, both ways
# device form: (R, e, f) with e.ctx, e.stream, e.p (name -> device pointer; ping-ponged names carry the parity), e.snapshot_stream
# host form:   (R, h, f) with h the state dict (name -> array; "prev_g" / "prev_m" / "prev_h" the previous frame's tuples)
def _d_snapshot(R, e, f):
    api.snapshot_bvh_device(e.ctx, e.p["snap"], geometry()["nvec4"], stream=e.snapshot_stream)


def _h_snapshot(R, h, f):
    h["snap"] = h["packed"].copy()


def _d_refit(R, e, f):
    g = geometry()
    api.bvh_refit_device(e.ctx, f.verts, 3, g["idx"], g["P"])


def _h_refit(R, h, f):
    g = geometry()
    h["packed"] = api.bvh_refit(g["packed"], f.verts, 3, g["idx"], g["P"])


def _d_resnapshot(R, e, f):
    if f.first:
        _d_snapshot(R, e, f)


def _h_resnapshot(R, h, f):
    if f.first:
        _h_snapshot(R, h, f)


def _d_gbuffer(R, e, f):
    p = e.p
    api.primary_gbuffer_motion_device(e.ctx, p["snap"], geometry()["nvec4"], f.eye, f.prev_eye, f.target, f.fovy, W, H, p["pos" + f.c],
                                      p["nrm" + f.c], p["pts"], p["pnr"], stream=e.stream)


def _h_gbuffer(R, h, f):
    h["pos"], h["nrm"], h["pts"], h["pnr"] = api.primary_gbuffer_motion(h["packed"], h["snap"], f.eye, f.prev_eye, f.target, f.fovy, W, H,
                                                                        want_leaves=False)[:4]


def _d_facing(R, e, f):
    p = e.p
    api.facing_lights_device(e.ctx, f.constants, f.hard, p["pos" + f.c], p["nrm" + f.c], W, H, p["map"], stream=e.stream)


def _h_facing(R, h, f):
    h["map"] = api.facing_lights(f.constants, f.hard, h["pos"], h["nrm"])


def _d_subsample(R, e, f):
    p = e.p
    api.subsample_gbuffer_device(e.ctx, f.up, p["pos" + f.c], p["nrm" + f.c], W, H, p["lpos"], p["lnrm"], d_lights_map=p["map"],
                                 d_lo_lights_map=p["lmap"], stream=e.stream)


def _h_subsample(R, h, f):
    h["lpos"], h["lnrm"], h["lmap"] = api.subsample_gbuffer(f.up, h["pos"], h["nrm"], h["map"])


def _d_trace(R, e, f, d_pos, w, h, d_out, d_map):
    if f.tables is not None:
        e.ctx.trace_soft_light_list_adaptive_device(f.constants, f.lights, f.probes, d_pos, w, h, d_out, d_lights_map=d_map, stream=e.stream,
                                                    tables=f.tables)
    else:
        e.ctx.trace_soft_light_list_device(f.constants, f.lights, d_pos, w, h, d_out, d_lights_map=d_map, stream=e.stream)


def _h_trace(R, hs, f, pos, w, h, out, lights_map):
    if f.tables is not None:
        api.soft_light_list_adaptive(hs["packed"], f.constants, f.lights, f.probes, pos, w, h, lights_map, out=out, want_refined=False,
                                     tables=f.tables)
    else:
        api.soft_light_list(hs["packed"], f.constants, f.lights, pos, w, h, lights_map, out=out)


def _d_trace_lo(R, e, f):
    _d_trace(R, e, f, e.p["lpos"], f.w, f.h, e.p["lo"], e.p["lmap"])


def _h_trace_lo(R, h, f):
    h["lo"] = h["lo_preset"][:R.count * f.w * f.h].reshape(R.count, f.h, f.w)       # (written into the preset bytes)
    _h_trace(R, h, f, h["lpos"], f.w, f.h, h["lo"], h["lmap"])


def _d_retrace_map(R, e, f):
    p = e.p
    api.upsample_retrace_map_device(e.ctx, R.count, f.up, p["pos" + f.c], p["nrm" + f.c], p["lpos"], p["lnrm"], W, H, p["keep"],
                                    d_lights_map=p["map"], d_lo_lights_map=p["lmap"], stream=e.stream)


def _h_retrace_map(R, h, f):
    h["keep"] = api.upsample_retrace_map(R.count, f.up, h["pos"], h["nrm"], h["lpos"], h["lnrm"], h["map"], h["lmap"])


def _d_trace_masked(R, e, f):
    _d_trace(R, e, f, e.p["pos" + f.c], W, H, e.p["counts"], e.p["keep"])


def _h_trace_masked(R, h, f):
    _h_trace(R, h, f, h["pos"], W, H, h["counts"], h["keep"])


def _d_upsample(R, e, f):
    p = e.p
    api.upsample_soft_light_list_device(e.ctx, f.lights, f.up, p["pos" + f.c], p["nrm" + f.c], p["lpos"], p["lnrm"], p["lo"], W, H, p["counts"],
                                        d_lights_map=p["map"], d_lo_lights_map=p["lmap"], d_keep=p["keep"] if R.half[0] else None,
                                        stream=e.stream)


def _h_upsample(R, h, f):
    api.upsample_soft_light_list(f.lights, f.up, h["pos"], h["nrm"], h["lpos"], h["lnrm"], h["lo"], h["map"], h["lmap"],
                                 keep=h["keep"] if R.half[0] else None, out=h["counts"])


def _d_trace_full(R, e, f):
    e.ctx.trace_light_list_device(f.constants, f.lights, e.p["pos" + f.c], W, H, e.p["mask"], d_lights_map=e.p["map"], stream=e.stream)


def _h_trace_full(R, h, f):
    api.light_list(h["packed"], f.constants, f.lights, h["pos"], W, H, h["map"], out=h["mask"])


def _d_moments(R, e, f):
    p = e.p
    prev = None if f.first else tuple(p[k + f.o] for k in ("pos", "nrm", "mean", "square", "mlen"))
    api.accumulate_moments_soft_light_list_device(e.ctx, f.lights, f.tp, p["pos" + f.c], p["nrm" + f.c], p["counts"], W, H, p["mean" + f.c],
                                                  p["square" + f.c], p["mlen" + f.c], d_prev=prev, d_lights_map=p["map"], stream=e.stream,
                                                  d_motion=(p["pts"], p["pnr"]), clamp=f.moments_clamp)


def _h_moments(R, h, f):
    prev = None if f.first else h["prev_g"] + h["prev_m"]
    h["mean"], h["square"], h["mlen"] = api.accumulate_moments_soft_light_list(f.lights, f.tp, h["pos"], h["nrm"], h["counts"], prev, h["map"],
                                                                               motion=(h["pts"], h["pnr"]), clamp=f.moments_clamp)


def _d_filter(R, e, f):
    p = e.p
    geom = (p["pos" + f.c], p["nrm" + f.c])
    if R.name == "C":
        api.wide_filter_light_list_device(e.ctx, f.lights, f.filter, *geom, p["mask"], W, H, p["vis"], d_scratch=p["scratch"],
                                          d_lights_map=p["map"], stream=e.stream)
        return
    fn = api.wide_filter_propagated_mean_soft_light_list_device if R.name == "A" else api.wide_filter_guided_temporal_mean_soft_light_list_device
    fn(e.ctx, f.lights, f.filter, *geom, p["counts"], (p["mean" + f.c], p["square" + f.c], p["mlen" + f.c]), W, H, p["vis"],
       d_scratch=p["scratch"], d_lights_map=p["map"], stream=e.stream)


def _h_filter(R, h, f):
    if R.name == "C":
        h["vis"] = api.wide_filter_light_list(f.lights, f.filter, h["pos"], h["nrm"], h["mask"], h["map"])
        return
    fn = api.wide_filter_propagated_mean_soft_light_list if R.name == "A" else api.wide_filter_guided_temporal_mean_soft_light_list
    h["vis"] = fn(f.lights, f.filter, h["pos"], h["nrm"], h["counts"], (h["mean"], h["square"], h["mlen"]), h["map"])


def _d_accumulate(R, e, f):
    p = e.p
    prev = None if f.first else tuple(p[k + f.o] for k in ("pos", "nrm", "hvis", "hlen"))
    api.accumulate_visibility_list_device(e.ctx, f.hard, f.tp, p["pos" + f.c], p["nrm" + f.c], p["vis"], W, H, p["hvis" + f.c], p["hlen" + f.c],
                                          d_prev=prev, d_lights_map=p["map"], stream=e.stream, clamp=f.history_clamp,
                                          d_motion=(p["pts"], p["pnr"]))


def _h_accumulate(R, h, f):
    prev = None if f.first else h["prev_g"] + h["prev_h"]
    h["hvis"], h["hlen"] = api.accumulate_visibility_list(f.hard, f.tp, h["pos"], h["nrm"], h["vis"], prev, h["map"], clamp=f.history_clamp,
                                                          motion=(h["pts"], h["pnr"]))


def _d_combine(R, e, f):
    p = e.p
    api.combine_visibility_list_device(e.ctx, f.constants, f.hard, p["pos" + f.c], p["nrm" + f.c], p["hvis" + f.c] if R.name == "C" else p["vis"],
                                       W, H, p["rgb"], d_lights_map=p["map"], colors=f.colors, stream=e.stream)


def _h_combine(R, h, f):
    h["rgb"] = api.combine_visibility_list(f.constants, f.hard, h["pos"], h["nrm"], h["hvis"] if R.name == "C" else h["vis"], h["map"],
                                           colors=f.colors)


STAGES = {name[3:]: (fn, globals()["_h_" + name[3:]]) for name, fn in list(globals().items())
          if name.startswith("_d_") and name != "_d_trace"}


# ------------------------------------------------------------------------------------------------------------ the two runners
def run_device_frame(R, e, f, stages=None):
    """The frame's stages back to back through the device wrappers; nothing is synchronised here."""
    for name in (R.stages if stages is None else stages):
        STAGES[name][0](R, e, f)


def new_host_state():
    return {"packed": geometry()["packed"]}


def run_host_frame(R, h, f, stages=None, perturb=None):
    """The same list through the host twins.  The arrays a twin writes INTO (the count planes, the low-resolution planes, the mask) are
    preset to 0x5A first; the other twins return fresh arrays.  `perturb`: None, or (stage, function(h)) run right after that stage."""
    if not f.first:
        h["prev_g"] = (h["pos"], h["nrm"])
        if "mean" in h:
            h["prev_m"] = (h["mean"], h["square"], h["mlen"])
        if "hvis" in h:
            h["prev_h"] = (h["hvis"], h["hlen"])
    h["counts"] = np.full((R.count, H, W), PRESET_HOST, np.uint8)
    h["mask"] = np.full((H, W), PRESET_HOST, np.uint8)
    h["lo_preset"] = np.full(R.count * LO, PRESET_HOST, np.uint8)
    for name in (R.stages if stages is None else stages):
        STAGES[name][1](R, h, f)
        if perturb is not None and perturb[0] == name:
            perturb[1](h)
    return h


def host_chain(name, fixed=False, still_box=False, frames=FRAMES):
    """The host chain of a recipe, computed once: a list of the state after every frame (the arrays are never written again)."""
    key = ("chain", name, fixed, still_box, frames)
    if key not in _CACHE:
        R, h, out = RECIPES[name], new_host_state(), []
        for k in range(frames):
            run_host_frame(R, h, Frame(R, k, fixed, still_box))
            out.append(dict(h))
        _CACHE[key] = out
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ the comparison
def compare_frame(R, got, want, what, preset=PRESET_DEVICE):
    """Every defined byte of every plane of PLANES[R.name]: `got[name]` is a buffer's payload as bytes (it may be longer than the
    plane: a low-resolution buffer in a small phase, planes from `count` up), `want[name]` the host chain's array.  The bytes of
    `want` must be equal -- floats bit for bit -- and whatever follows them must still hold `preset`."""
    for name in PLANES[R.name]:
        w = np.ascontiguousarray(want[name])
        g = np.asarray(got[name]).reshape(-1).view(np.uint8)
        assert g.size >= w.nbytes, (what, name, "the buffer is smaller than the plane", g.size, w.nbytes)
        head, tail = g[:w.nbytes], g[w.nbytes:]
        wb = w.reshape(-1).view(np.uint8)
        bad = np.nonzero(head != wb)[0]
        assert bad.size == 0, (what, name, f"{bad.size} bytes differ", "first at element",
                               np.unravel_index(int(bad[0]) // w.itemsize, w.shape), "got", head[bad[:4]].tolist(), "want", wb[bad[:4]].tolist())
        assert (tail == preset).all(), (what, name, "bytes behind the plane were written", int((tail != preset).sum()))
