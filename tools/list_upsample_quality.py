"""What tracing a soft light list at half resolution costs in image quality, measured on the CPU with the host twins alone (no GPU):
DESIGN.md 4.32, the protocol of 4.27 (tools/list_temporal_quality.py) extended.

    python tools/list_upsample_quality.py [--out profiles/r37/list_upsample_quality.jsonl]

Scenes: the cornell box at 128 x 128 and the terrain at 96 x 96, one area light at the scene's point light, its radius 3 % and 10 % of
the scene's diagonal, through the facing map.  The yardstick is the UNFILTERED visibility of 48 samples at full resolution
(count / 48); every figure is the mean absolute difference to it over the active pixels.  The trace is the plain soft light list (the
jittered forms are out of the upsample's scope), phase (0, 0), taps at N.N' >= 0.9 and plane distance <= 0.5 % of the diagonal.
  row "single": columns full_4 (full resolution, 4 samples), full_16 (the control of half_16: the first 16 entries of the table are
      not the first 4, and a fixed table's subsets differ in bias), half_4 (half resolution, 4 samples: a quarter of the rays), half_16 (half
      resolution, 16 samples: equal rays); the half columns without and with the retrace ("_retrace": the pixels no tap stands for
      traced at full resolution with the column's own sample count); each "raw" (count / n) and "wide_2" (behind the 2-pass unguided
      wide filter); "retraced_share" of the active pixels; "half_4_exact": the same upsample computed in floating point without the
      rounding of the quotient -- the difference to half_4 raw is what rounding half up costs.
  row "temporal": a still camera, frame k traced with the shared offsets table rotated by k entries and -- at half resolution -- the
      phase rotated over the four pixels of a quad; the raw visibility accumulated (rtsh_accumulate_visibility_list, max_length 32)
      over 4, 8 and 12 frames: full_4, half_4, half_4_retrace and half_4_fixed (the phase NOT rotated).
A record, not a test: every row is written as it comes out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES = (4, 8, 12)
ROTATION = ((0, 0), (1, 1), (1, 0), (0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r37/list_upsample_quality.jsonl")
    args = ap.parse_args()
    from raytracedshadows_amd import api, scenes
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")

    def emit(row):
        line = json.dumps(row)
        out.write(line + "\n")
        out.flush()
        print(line, flush=True)

    for name, sc, W, H in (("cornell_128", scenes.cornell(), 128, 128), ("terrain_96", scenes.terrain(23), 96, 96)):
        verts, idx = sc.flat()
        packed = api.BVHBuilder().build(verts, 8, idx, sc.triangle_count).m_packedNodes
        pos, nrm, _ = api.primary_gbuffer(packed, sc.eye, sc.target, sc.fovy, W, H)
        k = api.RayTracingConstants.make(sc.eye, sc.light_direction, W, H)
        diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
        table = scenes.jitter_offsets(48, 1.0, 19)
        cam = (sc.eye, sc.target, sc.fovy)
        eps = 0.005 * diag
        for radius in (0.03, 0.1):
            light = lambda n, t=table: api.SoftLightList.make([(api.Light.POINT, tuple(sc.light_point), n, 0, radius * diag)], t)
            hard = light(4).hard_list()
            facing = api.facing_lights(k, hard, pos, nrm)
            active = (facing & 1) != 0
            truth = api.soft_light_list(packed, k, light(48), pos, W, H, facing)[0].astype(np.float32) / np.float32(48)
            err = lambda vis: round(float(np.abs(vis[active] - truth[active]).mean()), 5)
            raw = lambda lst, counts: api.wide_filter_soft_light_list(lst, api.WideFilterParams.make(0, 0.9, eps), pos, nrm, counts, facing)[0]
            wide = lambda lst, counts: api.wide_filter_soft_light_list(lst, api.WideFilterParams.make(2, 0.9, eps), pos, nrm, counts, facing)[0]

            def half(lst, phase, retrace):
                """(full-resolution counts, the retrace map or None, the low-resolution pieces) of one half-resolution frame."""
                p = api.UpsampleParams.make(phase[0], phase[1], 0.9, eps)
                lo_pos, lo_nrm, lo_map = api.subsample_gbuffer(p, pos, nrm, facing)
                lo = api.soft_light_list(packed, k, lst, lo_pos, lo_map.shape[1], lo_map.shape[0], lo_map)
                keep = planes = None
                if retrace:
                    keep = api.upsample_retrace_map(1, p, pos, nrm, lo_pos, lo_nrm, facing, lo_map)
                    planes = api.soft_light_list(packed, k, lst, pos, W, H, keep)
                counts = api.upsample_soft_light_list(lst, p, pos, nrm, lo_pos, lo_nrm, lo, facing, lo_map, keep, out=planes)
                return counts, keep, (p, lo_pos, lo_nrm, lo_map, lo)

            row = {"scene": name, "row": "single", "light_radius": radius, "active_pixels": int(active.sum())}
            full = api.soft_light_list(packed, k, light(4), pos, W, H, facing)
            row["full_4"] = {"raw": err(raw(light(4), full)), "wide_2": err(wide(light(4), full))}
            full = api.soft_light_list(packed, k, light(16), pos, W, H, facing)              # (the control of half_16: four times the rays)
            row["full_16"] = {"raw": err(raw(light(16), full)), "wide_2": err(wide(light(16), full))}
            for n in (4, 16):
                for retrace in (False, True):
                    counts, keep, pieces = half(light(n), (0, 0), retrace)
                    row[f"half_{n}" + ("_retrace" if retrace else "")] = {"raw": err(raw(light(n), counts)), "wide_2": err(wide(light(n), counts))}
                    if retrace:
                        row["retraced_share"] = round(float((keep[active] & 1).mean()), 4)
                    elif n == 4:                                         # the same taps in floating point, the quotient not rounded
                        sys.path.insert(0, os.path.join(ROOT, "tests"))
                        import list_upsample_cases as uc
                        p, lo_pos, lo_nrm, lo_map, lo = pieces
                        num, den = np.zeros((H, W)), np.zeros((H, W))
                        for X, Y, weight, bits, geom in uc._taps(1, p, pos, nrm, lo_pos, lo_nrm, lo_map):
                            take = geom & ((bits & 1) != 0)
                            num += np.where(take, weight * lo[0][Y, X].astype(np.float64), 0)
                            den += np.where(take, weight, 0)
                        exact = np.where(den > 0, num / np.maximum(den, 1), counts[0]) / 4.0
                        row["half_4_exact"] = {"raw": err(exact.astype(np.float32))}
            emit(row)

            row = {"scene": name, "row": "temporal", "light_radius": radius, "max_length": 32, "frames": list(FRAMES)}
            tp = api.TemporalParams.from_cameras(cam, cam, W, H, 0.9, eps, 32)
            for column, mode in (("full_4", None), ("half_4", (True, False)), ("half_4_retrace", (True, True)), ("half_4_fixed", (False, False))):
                hist, errors = None, []
                for frame in range(max(FRAMES)):
                    lst = light(4, np.ascontiguousarray(np.roll(table, -frame, axis=0)))
                    if mode is None:
                        counts = api.soft_light_list(packed, k, lst, pos, W, H, facing)
                    else:
                        counts = half(lst, ROTATION[frame % 4] if mode[0] else (0, 0), mode[1])[0]
                    hist = api.accumulate_visibility_list(hard, tp, pos, nrm, raw(lst, counts)[None], None if hist is None else (pos, nrm) + hist, facing)
                    if frame + 1 in FRAMES:
                        errors.append(err(hist[0][0]))
                row[column] = errors
            emit(row)


if __name__ == "__main__":
    main()
