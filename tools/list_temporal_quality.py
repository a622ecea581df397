"""What accumulating over frames buys in image quality, measured on the CPU with the host twins alone (no GPU): DESIGN.md 4.23.

    python tools/list_temporal_quality.py [--out profiles/r26/list_temporal_quality.jsonl]

Scenes: the cornell box at 128 x 128 and the terrain at 96 x 96 (the scenes of tests/golden/cornell_128.npz and terrain_96.npz), one
area light at the scene's point light, its radius 3 % and 10 % of the scene's diagonal, through the facing map.  The yardstick is the
UNFILTERED visibility of 48 samples (count / 48).  The trace is the jittered one of 4 samples (probe 2, a per-pixel table of 48
entries); frame k traces with the shared offsets table rotated by k entries.  Per scene and light, the mean absolute difference to the
yardstick over the active pixels of
    raw          count / 4 of frame 0                  (the number everything has to beat)
    filtered     rtsh_filter_soft_light_list at R = 2, N.N' >= 0.9, plane distance <= 0.5 % of the diagonal, of frame 0
    accumulated  rtsh_accumulate_visibility_list over 2, 4, 8 and 12 frames of a still camera (max_length 32: a running mean) of the raw
                 visibility, and of the filtered one
    single_16    count / 16 of ONE frame of 16 jittered samples: what four accumulated frames of 4 samples are to be compared with
A record, not a test: every row is written as it comes out.

    python tools/list_temporal_quality.py --jump [--out profiles/r28/list_clamp_quality.jsonl]

The neighbourhood clamp (rtsh_accumulate_visibility_list_clamped): the same scenes and light of 3 % of the diagonal;
the light stands for JUMP_AT frames, then JUMPS sideways by 15 % of the diagonal and stands for AFTER more.  Per frame after the jump,
the mean absolute difference to the 48-sample trace of the NEW light over its active pixels, of the raw (R = 0) and the filtered
(R = 2) planes accumulated
    unclamped    as before: the history of the old light is blended in
    clamp_r      clamped at r = 1, 2 and 4, margin 0
    reset        unclamped, with the light in reset_lights on the frame of the jump: its history thrown away
and a STILL row: the same light standing for all JUMP_AT + AFTER frames, where the clamp can only cost noise reduction.

    python tools/list_temporal_quality.py --guide-history [--out profiles/r31/list_moments_quality.jsonl]

The temporal guide of the wide filter (rtsh_accumulate_moments_soft_light_list, rtsh_wide_filter_guided_temporal_soft_light_list,
DESIGN.md 4.27): the still-camera scenes and lights of the first table; the count moments are accumulated per frame (max_length 32),
and after 4, 8 and 12 frames THAT frame's jittered counts are filtered, two passes, by the unguided wide filter, by 4.26's guide and
by the temporal guide (min_history 4) at guide_k4 8, 12 and 16; "raw" is count / 4 of that frame.  Every row twice: the shared table
rotated by one entry per frame, and by the sample count per frame (4).

    python tools/list_temporal_quality.py --mean-input [--out profiles/r32/list_mean_filter_quality.jsonl]

The wide filters fed from the accumulated mean (rtsh_wide_filter_mean_soft_light_list,
rtsh_wide_filter_guided_temporal_mean_soft_light_list): the protocol of --guide-history unchanged, and three more
columns per row: "mean_raw" the unfiltered mean plane (passes 0), "mean_unguided" the unguided filter over it, "mean_temporal" the
guided one at guide_k4 8, 12 and 16.

    python tools/list_temporal_quality.py --propagate [--out profiles/r36/list_propagated_quality.jsonl]

The guided mean filter with a propagated variance (rtsh_wide_filter_propagated_mean_soft_light_list): --mean-input's rows,
and per row "passes_2" and "passes_4": at that many passes the unguided mean filter, 4.27's guide ("temporal"), 4.28's guided mean filter
("mean_temporal") and the propagated filter without and with by_length, each guided one at guide_k4 8, 12 and 16.

    python tools/list_temporal_quality.py --move [--out profiles/r33/list_motion_quality.jsonl]

Motion vectors (rtsh_primary_gbuffer_motion, rtsh_accumulate_visibility_list_motion): cornell_128, a still camera in the
room's open front (MOVE_EYE, MOVE_TARGET), the
light of 3 % and 10 % of the diagonal; the tall box is translated by MOVE_STEP per frame and the stream refitted (api.bvh_refit of one
build).  Every frame traces 4 jittered samples; the raw (R = 0) visibility is accumulated (max_length 32) by the plain pass and by the
motion pass.  After 4, 8 and 12 frames: the mean absolute difference to the 48-sample trace of THAT frame's geometry, and the mean
history length, over the active pixels of the MOVED object (prev_points.w == 2) and over the rest; "raw" is that frame's count / 4.

    python tools/list_temporal_quality.py --jump --moments [--out profiles/r35/list_moments_clamp_quality.jsonl]
    python tools/list_temporal_quality.py --move --moments [--out ...]

The clamp of the moments' history (rtsh_accumulate_moments_soft_light_list_clamped*): the moments column set of the two
protocols above, cornell_128, lights of 3 % and 10 % of the diagonal.  --jump: the light stands for JUMP_AT frames, jumps and stands for
AFTER more; --move: the box moves every frame for JUMP_AT + AFTER frames and the error is taken over the REST pixels (the static
receivers, prev_points.w != 2) of the last AFTER frames.  Each also as a STILL scene (no jump, no move), where a clamp can only cost.
Per frame the mean absolute difference to the 48-sample trace of three quantities: "mean" the accumulated mean plane unfiltered,
"unguided" and "k4_12" the mean-input filters of 4.28 at two passes.  Columns: "unclamped"; "clamp_R_K4" for R in 1, 2, 4 and sigma_k4 in
4, 8, 36, margin 0; "reset" (reset_lights on the frame of the jump; --jump only); "single" one frame alone (max_length 1); and as
bases "float_clamp_1", 4.24's clamp at r = 1 over the raw float visibility.  "scatter" is the largest minus the smallest unclamped
error of the STILL scene over its last AFTER frames: the frame-to-frame noise a difference has to exceed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES = (2, 4, 8, 12)


JUMP_AT, AFTER, JUMP = 8, 4, 0.15
MODES = ("unclamped", "clamp_1", "clamp_2", "clamp_4", "reset")


def jump_rows():
    from raytracedshadows_amd import api, scenes
    rows = []
    for name, sc, W, H in (("cornell_128", scenes.cornell(), 128, 128), ("terrain_96", scenes.terrain(23), 96, 96)):
        verts, idx = sc.flat()
        packed = api.BVHBuilder().build(verts, 8, idx, sc.triangle_count).m_packedNodes
        pos, nrm, _ = api.primary_gbuffer(packed, sc.eye, sc.target, sc.fovy, W, H)
        k = api.RayTracingConstants.make(sc.eye, sc.light_direction, W, H)
        diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
        table = scenes.jitter_offsets(48, 1.0, 19)
        cam = (sc.eye, sc.target, sc.fovy)
        moved = tuple(float(v) for v in np.asarray(sc.light_point, np.float64) + np.array([JUMP * diag, 0.0, 0.0]))
        light = lambda at, n, t=table: api.SoftLightList.make([(api.Light.POINT, at, n, 0, 0.03 * diag)], t)
        jittered = lambda lst, facing: api.soft_light_list_adaptive(packed, k, lst, (2,), pos, W, H, facing, want_refined=False, tables=(48,))[0]
        filters = {"raw": api.FilterParams.make(0, 0.9, 0.005 * diag), "filtered": api.FilterParams.make(2, 0.9, 0.005 * diag)}
        for scenario in ("jump", "still"):
            frames, planes, truth = JUMP_AT + AFTER, {"raw": [], "filtered": []}, {}
            for frame in range(frames):
                at = moved if scenario == "jump" and frame >= JUMP_AT else tuple(sc.light_point)
                lst = light(at, 4, np.ascontiguousarray(np.roll(table, -frame, axis=0)))
                facing = api.facing_lights(k, lst.hard_list(), pos, nrm)
                if at not in truth:
                    truth[at] = ((facing & 1) != 0, api.soft_light_list(packed, k, light(at, 48), pos, W, H, facing)[0].astype(np.float32)
                                 / np.float32(48))
                counts = jittered(lst, facing)
                for key, fp in filters.items():
                    planes[key].append((at, lst.hard_list(), facing, api.filter_soft_light_list(lst, fp, pos, nrm, counts, facing)))
            for key in filters:
                row = {"scene": name, "scenario": scenario, "planes": key, "jump_at": JUMP_AT, "max_length": 32, "error": {}}
                for mode in MODES:
                    if scenario == "still" and mode == "reset":
                        continue
                    hist, errors = None, []
                    for frame, (at, hard, facing, vis) in enumerate(planes[key]):
                        reset = 1 if mode == "reset" and scenario == "jump" and frame == JUMP_AT else 0
                        tp = api.TemporalParams.from_cameras(cam, cam, W, H, 0.9, 0.005 * diag, 32, reset)
                        clamp = api.HistoryClamp.make(int(mode[-1])) if mode.startswith("clamp") else None
                        hist = api.accumulate_visibility_list(hard, tp, pos, nrm, vis, None if hist is None else (pos, nrm) + hist, facing,
                                                              clamp=clamp)
                        if frame >= JUMP_AT:
                            active, want = truth[at]
                            errors.append(round(float(np.abs(hist[0][0][active] - want[active]).mean()), 5))
                    row["error"][mode] = errors
                active, want = truth[planes[key][-1][0]]
                row["single_frame"] = round(float(np.abs(planes[key][-1][3][0][active] - want[active]).mean()), 5)
                rows.append(row)
                print(json.dumps(row))
    return rows


GUIDE_FRAMES, GUIDE_K4, GUIDE_PASSES, GUIDE_MIN_HISTORY = (4, 8, 12), (8, 12, 16), 2, 4


PROPAGATE_PASSES = (2, 4)


def guide_rows(mean_input=False, propagate=False):
    from raytracedshadows_amd import api, scenes
    rows = []
    for name, sc, W, H in (("cornell_128", scenes.cornell(), 128, 128), ("terrain_96", scenes.terrain(23), 96, 96)):
        verts, idx = sc.flat()
        packed = api.BVHBuilder().build(verts, 8, idx, sc.triangle_count).m_packedNodes
        pos, nrm, _ = api.primary_gbuffer(packed, sc.eye, sc.target, sc.fovy, W, H)
        k = api.RayTracingConstants.make(sc.eye, sc.light_direction, W, H)
        diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
        table = scenes.jitter_offsets(48, 1.0, 19)
        cam = (sc.eye, sc.target, sc.fovy)
        eps = 0.005 * diag
        tp = api.TemporalParams.from_cameras(cam, cam, W, H, 0.9, eps, 32)
        for radius in (0.03, 0.1):
            light = lambda n, t=table: api.SoftLightList.make([(api.Light.POINT, sc.light_point, n, 0, radius * diag)], t)
            facing = api.facing_lights(k, light(4).hard_list(), pos, nrm)
            active = (facing & 1) != 0
            truth = api.soft_light_list(packed, k, light(48), pos, W, H, facing)[0].astype(np.float32) / np.float32(48)
            mad = lambda v: round(float(np.abs(v[active] - truth[active]).mean()), 5)
            for rotate in (1, 4):
                moments = None
                for frame in range(max(GUIDE_FRAMES)):
                    lst = light(4, np.ascontiguousarray(np.roll(table, -frame * rotate, axis=0)))
                    counts = api.soft_light_list_adaptive(packed, k, lst, (2,), pos, W, H, facing, want_refined=False, tables=(48,))[0]
                    moments = api.accumulate_moments_soft_light_list(lst, tp, pos, nrm, counts, None if moments is None else (pos, nrm) + moments,
                                                                     facing)
                    if frame + 1 not in GUIDE_FRAMES:
                        continue
                    assert int(moments[2][0][active].min()) == frame + 1          # a still camera: every pixel keeps its history
                    row = {"scene": name, "light": radius, "rotate": rotate, "history": frame + 1, "passes": GUIDE_PASSES,
                           "min_history": GUIDE_MIN_HISTORY, "raw": mad(counts[0].astype(np.float32) / np.float32(4)),
                           "unguided": mad(api.wide_filter_soft_light_list(lst, api.WideFilterParams.make(GUIDE_PASSES, 0.9, eps), pos, nrm, counts,
                                                                           facing)[0]), "guided": {}, "temporal": {}}
                    for k4 in GUIDE_K4:
                        row["guided"][str(k4)] = mad(api.wide_filter_guided_soft_light_list(
                            lst, api.WideGuideParams.make(GUIDE_PASSES, k4, 0.9, eps), pos, nrm, counts, facing)[0])
                        row["temporal"][str(k4)] = mad(api.wide_filter_guided_temporal_soft_light_list(
                            lst, api.WideGuideTemporalParams.make(GUIDE_PASSES, k4, GUIDE_MIN_HISTORY, 0.9, eps), pos, nrm, counts, moments, facing)[0])
                    if mean_input:
                        row["mean_raw"] = mad(api.wide_filter_mean_soft_light_list(lst, api.WideFilterParams.make(0, 0.9, eps), pos, nrm,
                                                                                   moments[0], facing)[0])
                        row["mean_unguided"] = mad(api.wide_filter_mean_soft_light_list(lst, api.WideFilterParams.make(GUIDE_PASSES, 0.9, eps),
                                                                                        pos, nrm, moments[0], facing)[0])
                        row["mean_temporal"] = {str(k4): mad(api.wide_filter_guided_temporal_mean_soft_light_list(
                            lst, api.WideGuideTemporalParams.make(GUIDE_PASSES, k4, GUIDE_MIN_HISTORY, 0.9, eps), pos, nrm, counts, moments,
                            facing)[0]) for k4 in GUIDE_K4}
                    if propagate:
                        for passes in PROPAGATE_PASSES:
                            cell = {"unguided": mad(api.wide_filter_mean_soft_light_list(lst, api.WideFilterParams.make(passes, 0.9, eps), pos, nrm,
                                                                                         moments[0], facing)[0]),
                                    "temporal": {}, "mean_temporal": {}, "propagated": {}, "propagated_by_length": {}}
                            for k4 in GUIDE_K4:
                                gp = api.WideGuideTemporalParams.make(passes, k4, GUIDE_MIN_HISTORY, 0.9, eps)
                                cell["temporal"][str(k4)] = mad(api.wide_filter_guided_temporal_soft_light_list(lst, gp, pos, nrm, counts, moments,
                                                                                                                facing)[0])
                                cell["mean_temporal"][str(k4)] = mad(api.wide_filter_guided_temporal_mean_soft_light_list(lst, gp, pos, nrm, counts,
                                                                                                                          moments, facing)[0])
                                for by_length, key in ((0, "propagated"), (1, "propagated_by_length")):
                                    pp = api.WideGuidePropagatedParams.make(passes, k4, GUIDE_MIN_HISTORY, by_length, 0.9, eps)
                                    cell[key][str(k4)] = mad(api.wide_filter_propagated_mean_soft_light_list(lst, pp, pos, nrm, counts, moments,
                                                                                                             facing)[0])
                            row["passes_" + str(passes)] = cell
                    rows.append(row)
                    print(json.dumps(row))
    return rows


MOVE_FRAMES, MOVE_STEP = (4, 8, 12), (-0.12, 0.0, 0.04)      # (away from under the light: the box's seen faces stay lit for 12 frames)
#: a camera in the room's open front (the scene's own stands outside and sees a sliver of the box)
MOVE_EYE, MOVE_TARGET = (5.0, 5.0, 14.0), (4.0, 3.5, 3.0)


def move_rows():
    from raytracedshadows_amd import api, scenes
    rows = []
    sc, W, H = scenes.cornell(), 128, 128
    faces = np.ascontiguousarray(sc.faces, np.uint32)
    idx, P = np.ascontiguousarray(faces.reshape(-1)), faces.shape[0]
    box = np.unique(faces[640:832])                                     # the tall box: its own vertices
    base = np.ascontiguousarray(sc.verts, np.float64)
    built = api.BVHBuilder().build(np.ascontiguousarray(base, np.float32), 3, idx, P).m_packedNodes
    sc.eye, sc.target, sc.fovy = np.array(MOVE_EYE, np.float32), np.array(MOVE_TARGET, np.float32), 0.9
    k = api.RayTracingConstants.make(sc.eye, sc.light_direction, W, H)
    diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
    table = scenes.jitter_offsets(48, 1.0, 19)
    cam = (sc.eye, sc.target, sc.fovy)
    eps = 0.005 * diag
    tp = api.TemporalParams.from_cameras(cam, cam, W, H, 0.9, eps, 32)
    raw = api.FilterParams.make(0, 0.9, eps)
    for radius in (0.03, 0.1):
        light = lambda n, t=table: api.SoftLightList.make([(api.Light.POINT, sc.light_point, n, 0, radius * diag)], t)
        hard = light(4).hard_list()
        hist = {"plain": None, "motion": None}
        prev_stream = prev_g = None
        for frame in range(max(MOVE_FRAMES)):
            verts = base.copy()
            verts[box] += np.asarray(MOVE_STEP) * frame
            packed = api.bvh_refit(built, np.ascontiguousarray(verts, np.float32), 3, idx, P)
            pos, nrm, pts, pnr, _, _ = api.primary_gbuffer_motion(packed, packed if prev_stream is None else prev_stream, sc.eye, sc.eye, sc.target,
                                                                  sc.fovy, W, H, want_leaves=False)
            facing = api.facing_lights(k, hard, pos, nrm)
            lst = light(4, np.ascontiguousarray(np.roll(table, -frame, axis=0)))
            counts = api.soft_light_list_adaptive(packed, k, lst, (2,), pos, W, H, facing, want_refined=False, tables=(48,))[0]
            vis = api.filter_soft_light_list(lst, raw, pos, nrm, counts, facing)
            for key in hist:
                prev = None if hist[key] is None else prev_g + hist[key]
                hist[key] = api.accumulate_visibility_list(hard, tp, pos, nrm, vis, prev, facing, motion=(pts, pnr) if key == "motion" else None)
            prev_stream, prev_g = packed, (pos, nrm)
            if frame + 1 not in MOVE_FRAMES:
                continue
            active = (facing & 1) != 0
            truth = api.soft_light_list(packed, k, light(48), pos, W, H, facing)[0].astype(np.float32) / np.float32(48)
            regions = {"moved": active & (pts[..., 3] == 2), "rest": active & (pts[..., 3] != 2)}
            row = {"scene": "cornell_128", "light": radius, "frames": frame + 1, "step": list(MOVE_STEP), "max_length": 32}
            for name, where in regions.items():
                mad = lambda v: round(float(np.abs(v[where] - truth[where]).mean()), 5)
                row[name] = {"pixels": int(where.sum()), "raw": mad(vis[0]), "plain": mad(hist["plain"][0][0]), "motion": mad(hist["motion"][0][0]),
                             "plain_length": round(float(hist["plain"][1][0][where].mean()), 2),
                             "motion_length": round(float(hist["motion"][1][0][where].mean()), 2)}
            rows.append(row)
            print(json.dumps(row))
    return rows


MOMENTS_CLAMPS = [(r, k4) for r in (1, 2, 4) for k4 in (4, 8, 36)]


def moments_rows(protocol):
    """The moments column set of --jump and --move; see the module text."""
    from raytracedshadows_amd import api, scenes
    rows = []
    sc, W, H = scenes.cornell(), 128, 128
    faces = np.ascontiguousarray(sc.faces, np.uint32)
    idx, P = np.ascontiguousarray(faces.reshape(-1)), faces.shape[0]
    box = np.unique(faces[640:832])
    base = np.ascontiguousarray(sc.verts, np.float64)
    built = api.BVHBuilder().build(np.ascontiguousarray(base, np.float32), 3, idx, P).m_packedNodes
    if protocol == "move":
        sc.eye, sc.target, sc.fovy = np.array(MOVE_EYE, np.float32), np.array(MOVE_TARGET, np.float32), 0.9
    k = api.RayTracingConstants.make(sc.eye, sc.light_direction, W, H)
    diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
    table = scenes.jitter_offsets(48, 1.0, 19)
    cam = (sc.eye, sc.target, sc.fovy)
    eps = 0.005 * diag
    total = JUMP_AT + AFTER
    jumped = tuple(float(v) for v in np.asarray(sc.light_point, np.float64) + np.array([JUMP * diag, 0.0, 0.0]))
    modes = ["unclamped"] + [f"clamp_{r}_{k4}" for r, k4 in MOMENTS_CLAMPS] + (["reset"] if protocol == "jump" else []) + ["single", "float_clamp_1"]
    for radius in (0.03, 0.1):
        light = lambda at, n, t=table: api.SoftLightList.make([(api.Light.POINT, at, n, 0, radius * diag)], t)
        still_unclamped = None
        for scenario in ("still", protocol):
            frames, prev_stream = [], None
            for frame in range(total):
                at = jumped if scenario == "jump" and frame >= JUMP_AT else tuple(sc.light_point)
                verts = base.copy()
                if scenario == "move":
                    verts[box] += np.asarray(MOVE_STEP) * frame
                packed = api.bvh_refit(built, np.ascontiguousarray(verts, np.float32), 3, idx, P)
                pos, nrm, pts, pnr, _, _ = api.primary_gbuffer_motion(packed, packed if prev_stream is None else prev_stream, sc.eye, sc.eye,
                                                                      sc.target, sc.fovy, W, H, want_leaves=False)
                lst = light(at, 4, np.ascontiguousarray(np.roll(table, -frame, axis=0)))
                facing = api.facing_lights(k, lst.hard_list(), pos, nrm)
                counts = api.soft_light_list_adaptive(packed, k, lst, (2,), pos, W, H, facing, want_refined=False, tables=(48,))[0]
                where = truth = None
                if frame >= JUMP_AT:
                    where = ((facing & 1) != 0) & ((pts[..., 3] != 2) if protocol == "move" else True)
                    truth = api.soft_light_list(packed, k, light(at, 48), pos, W, H, facing)[0].astype(np.float32) / np.float32(48)
                frames.append((lst, facing, counts, pos, nrm, pts, pnr, where, truth))
                prev_stream = packed
            row = {"protocol": protocol, "scenario": scenario, "scene": "cornell_128", "light": radius, "jump_at": JUMP_AT, "max_length": 32,
                   "error": {}}
            for mode in modes:
                hist, prev_g, errors = None, None, {"mean": [], "unguided": [], "k4_12": []}
                for frame, (lst, facing, counts, pos, nrm, pts, pnr, where, truth) in enumerate(frames):
                    reset = 1 if mode == "reset" and scenario == "jump" and frame == JUMP_AT else 0
                    tp = api.TemporalParams.from_cameras(cam, cam, W, H, 0.9, eps, 1 if mode == "single" else 32, reset)
                    prev = None if hist is None else prev_g + hist
                    motion = (pts, pnr) if protocol == "move" else None
                    mad = lambda v: round(float(np.abs(v[where] - truth[where]).mean()), 5)
                    if mode == "float_clamp_1":
                        vis = api.filter_soft_light_list(lst, api.FilterParams.make(0, 0.9, eps), pos, nrm, counts, facing)
                        hist = api.accumulate_visibility_list(lst.hard_list(), tp, pos, nrm, vis, prev, facing, clamp=api.HistoryClamp.make(1),
                                                              motion=motion)
                        if frame >= JUMP_AT:
                            errors["mean"].append(mad(hist[0][0]))
                    else:
                        clamp = api.MomentsClamp.make(int(mode.split("_")[1]), int(mode.split("_")[2]), 0) if mode.startswith("clamp") else None
                        hist = api.accumulate_moments_soft_light_list(lst, tp, pos, nrm, counts, prev, facing, motion=motion, clamp=clamp)
                        if frame >= JUMP_AT:
                            errors["mean"].append(mad(api.wide_filter_mean_soft_light_list(lst, api.WideFilterParams.make(0, 0.9, eps), pos, nrm,
                                                                                           hist[0], facing)[0]))
                            errors["unguided"].append(mad(api.wide_filter_mean_soft_light_list(
                                lst, api.WideFilterParams.make(GUIDE_PASSES, 0.9, eps), pos, nrm, hist[0], facing)[0]))
                            errors["k4_12"].append(mad(api.wide_filter_guided_temporal_mean_soft_light_list(
                                lst, api.WideGuideTemporalParams.make(GUIDE_PASSES, 12, GUIDE_MIN_HISTORY, 0.9, eps), pos, nrm, counts, hist, facing)[0]))
                    prev_g = (pos, nrm)
                row["error"][mode] = {q: v for q, v in errors.items() if v}
            if scenario == "still":
                still_unclamped = row["error"]["unclamped"]
            row["scatter"] = {q: round(max(v) - min(v), 5) for q, v in still_unclamped.items()}
            rows.append(row)
            print(json.dumps(row))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--jump", action="store_true", help="the light-jump scenario of the neighbourhood clamp instead of the still-camera table")
    ap.add_argument("--guide-history", action="store_true", help="the temporal guide of the wide filter against the unguided filter and 4.26's guide")
    ap.add_argument("--mean-input", action="store_true", help="--guide-history's table with the mean-input filters' three columns beside it")
    ap.add_argument("--propagate", action="store_true", help="--mean-input's table with the propagated filter's columns at 2 and 4 passes")
    ap.add_argument("--move", action="store_true", help="the plain and the motion accumulate over a box translated and refitted every frame")
    ap.add_argument("--moments", action="store_true", help="with --jump or --move: the moments column set of the clamped moments pass")
    args = ap.parse_args()
    from raytracedshadows_amd import api, scenes
    if args.moments and (args.jump or args.move):
        rows = (moments_rows("jump") if args.jump else []) + (moments_rows("move") if args.move else [])
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                for row in rows:
                    f.write(json.dumps(row) + "\n")
        return
    rows = move_rows() if args.move else jump_rows() if args.jump else (
        guide_rows(args.mean_input or args.propagate, args.propagate) if args.guide_history or args.mean_input or args.propagate else [])
    if args.move or args.jump or args.guide_history or args.mean_input or args.propagate:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                for row in rows:
                    f.write(json.dumps(row) + "\n")
        return
    for name, sc, W, H in (("cornell_128", scenes.cornell(), 128, 128), ("terrain_96", scenes.terrain(23), 96, 96)):
        verts, idx = sc.flat()
        packed = api.BVHBuilder().build(verts, 8, idx, sc.triangle_count).m_packedNodes
        pos, nrm, _ = api.primary_gbuffer(packed, sc.eye, sc.target, sc.fovy, W, H)
        k = api.RayTracingConstants.make(sc.eye, sc.light_direction, W, H)
        diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
        table = scenes.jitter_offsets(48, 1.0, 19)
        cam = (sc.eye, sc.target, sc.fovy)
        tp = api.TemporalParams.from_cameras(cam, cam, W, H, 0.9, 0.005 * diag, 32)
        for radius in (0.03, 0.1):
            light = lambda n, t=table: api.SoftLightList.make([(api.Light.POINT, sc.light_point, n, 0, radius * diag)], t)
            hard = light(4).hard_list()
            facing = api.facing_lights(k, hard, pos, nrm)
            active = (facing & 1) != 0
            truth = api.soft_light_list(packed, k, light(48), pos, W, H, facing)[0].astype(np.float32) / np.float32(48)
            mad = lambda v: float(np.abs(v[active] - truth[active]).mean())
            jittered = lambda lst: api.soft_light_list_adaptive(packed, k, lst, (2,), pos, W, H, facing, want_refined=False, tables=(48,))[0]
            plain, wide = api.FilterParams.make(0, 0.9, 0.005 * diag), api.FilterParams.make(2, 0.9, 0.005 * diag)
            row = {"scene": name, "light": radius, "active_pixels": int(active.sum()),
                   "penumbra_pixels": int(((truth > 0) & (truth < 1) & active).sum()), "accumulated": {}, "accumulated_filtered": {}}
            hist = {"accumulated": None, "accumulated_filtered": None}
            for frame in range(max(FRAMES)):
                lst = light(4, np.ascontiguousarray(np.roll(table, -frame, axis=0)))
                counts = jittered(lst)
                for key, p in (("accumulated", plain), ("accumulated_filtered", wide)):
                    vis = api.filter_soft_light_list(lst, p, pos, nrm, counts, facing)
                    if frame == 0:
                        row["raw" if key == "accumulated" else "filtered"] = mad(vis[0])
                    prev = None if hist[key] is None else (pos, nrm) + hist[key]
                    hist[key] = api.accumulate_visibility_list(hard, tp, pos, nrm, vis, prev, facing)
                    if frame + 1 in FRAMES:
                        row[key][str(frame + 1)] = mad(hist[key][0][0])
                        assert int(hist[key][1][0][active].min()) == frame + 1          # a still camera: every pixel keeps its history
            row["single_16"] = mad(jittered(light(16))[0].astype(np.float32) / np.float32(16))
            rows.append(row)
            print(json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
