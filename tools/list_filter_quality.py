"""What the list filter buys in image quality, measured on the CPU with the host twins alone (no GPU): DESIGN.md 4.22.

    python tools/list_filter_quality.py [--radius 4] [--out profiles/r25/list_filter_quality.jsonl]
    python tools/list_filter_quality.py --wide [--light 0.1] [--out profiles/r29/list_wide_filter_quality.jsonl]      
    python tools/list_filter_quality.py --wide --guide 8,12,16 [--light 0.1] [--out profiles/r30/list_wide_guided_quality.jsonl]   (4.26)

Scenes: the cornell box at 128 x 128 and the terrain at 96 x 96 (the scenes of tests/golden/cornell_128.npz and terrain_96.npz), one
area light at the scene's point light, its radius --light (default 3 %) of the scene's diagonal, through the facing map.  The yardstick is the UNFILTERED
visibility of 48 samples (count / 48).  Per scene and per trace of 4 samples -- plain (the first four table entries), adaptive (probe
2) and jittered (probe 2, a per-pixel table of 48 entries) -- the mean absolute difference to the yardstick over the active pixels of
    raw       count / 4, unfiltered        (the number the filter has to beat)
    filtered  rtsh_filter_soft_light_list at --radius, N.N' >= 0.9, plane distance <= 0.5 % of the diagonal
    guided    the same with the distance planes of a 4-sample distance trace and spread 0.05 (plain trace only)
--wide: instead, per scene and trace, one row per tent radius R = 1, 2, 4, 8 ("filter": "tent") and one per number of passes 1 .. 4 of the
wide (a-trous) filter rtsh_wide_filter_soft_light_list ("filter": "wide", its reach 2, 6, 14, 30 pixels), same thresholds, same measure.
--wide --guide K4[,K4...]: only the wide rows, each with one more figure per K4 -- "guided_k4_<K4>", the variance-guided filter
rtsh_wide_filter_guided_soft_light_list at that tolerance (K4 / 4 standard deviations), same thresholds, same measure.
A record, not a test: every row is written as it comes out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--light", type=float, default=0.03, help="the light's radius as a share of the scene's diagonal")
    ap.add_argument("--wide", action="store_true", help="rows for R = 1, 2, 4, 8 and for 1 .. 4 passes of the wide filter")
    ap.add_argument("--guide", default="", metavar="K4[,K4...]", help="with --wide: guided figures at these tolerances (quarter deviations)")
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
        light = lambda n: api.SoftLightList.make([(api.Light.POINT, sc.light_point, n, 0, args.light * diag)], table)
        four, full = light(4), light(48)
        facing = api.facing_lights(k, four.hard_list(), pos, nrm)
        active = (facing & 1) != 0
        truth = api.soft_light_list(packed, k, full, pos, W, H, facing)[0].astype(np.float32) / np.float32(48)
        p = api.FilterParams.make(args.radius, 0.9, 0.005 * diag, 0.05)
        traces = {"plain": api.soft_light_list(packed, k, four, pos, W, H, facing),
                  "adaptive": api.soft_light_list_adaptive(packed, k, four, (2,), pos, W, H, facing, want_refined=False)[0],
                  "jittered": api.soft_light_list_adaptive(packed, k, four, (2,), pos, W, H, facing, want_refined=False, tables=(48,))[0]}
        dist, _ = api.soft_light_list_distance(packed, k, four, pos, W, H, facing)
        mad = lambda v: float(np.abs(v[active] - truth[active]).mean())
        for trace, counts in traces.items():
            if args.wide:
                base = {"scene": name, "trace": trace, "light": args.light, "active_pixels": int(active.sum()),
                        "penumbra_pixels": int(((truth > 0) & (truth < 1) & active).sum()),
                        "raw": mad(counts[0].astype(np.float32) / np.float32(4))}
                guides = [int(v) for v in args.guide.split(",") if v]
                for radius in () if guides else (1, 2, 4, 8):
                    q = api.FilterParams.make(radius, 0.9, 0.005 * diag)
                    rows.append(dict(base, filter="tent", radius=radius, reach=radius,
                                     filtered=mad(api.filter_soft_light_list(four, q, pos, nrm, counts, facing)[0])))
                    print(json.dumps(rows[-1]))
                for passes in (1, 2, 3, 4):
                    q = api.WideFilterParams.make(passes, 0.9, 0.005 * diag)
                    rows.append(dict(base, filter="wide", passes=passes, reach=2 * (2 ** passes - 1),
                                     filtered=mad(api.wide_filter_soft_light_list(four, q, pos, nrm, counts, facing)[0])))
                    for k4 in guides:
                        g = api.WideGuideParams.make(passes, k4, 0.9, 0.005 * diag)
                        rows[-1][f"guided_k4_{k4}"] = mad(api.wide_filter_guided_soft_light_list(four, g, pos, nrm, counts, facing)[0])
                    print(json.dumps(rows[-1]))
                continue
            row = {"scene": name, "trace": trace, "radius": args.radius, "light": args.light, "active_pixels": int(active.sum()),
                   "penumbra_pixels": int(((truth > 0) & (truth < 1) & active).sum()),
                   "raw": mad(counts[0].astype(np.float32) / np.float32(4)),
                   "filtered": mad(api.filter_soft_light_list(four, p, pos, nrm, counts, facing)[0])}
            if trace == "plain":
                row["guided"] = mad(api.filter_soft_light_list(four, p, pos, nrm, counts, facing, dist)[0])
            rows.append(row)
            print(json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
