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
A record, not a test: every row is written as it comes out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FRAMES = (2, 4, 8, 12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
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
