"""What the adaptive ambient occlusion trace costs in image quality, measured on the CPU with the host twins alone (no GPU): DESIGN.md 4.35.

    python tools/ao_adaptive_quality.py [--radius 0.2] [--out profiles/r43/ao_adaptive_quality.jsonl]

Scenes: the cornell box at 128 x 128 and the terrain at 96 x 96 (the scenes of tests/golden/cornell_128.npz and terrain_96.npz), AO
segments of --radius (default 20 %) of the scene's diagonal, AoParams.make with seed 5.  Per scene, per (n, k) of (2, 1), (3, 1), (5, 4),
(4, 3), (16, 4), (48, 47) and (48, 1), without a table and with one of 64 entries -- against the FULL AO count of the same parameters
(rtsh_ambient_occlusion), over the pixels that have a surface:
    differ        the share of pixels whose byte differs from the full count
    refined       the share of pixels that took their full count
    raw           the mean absolute difference of count / n
    filtered      the same behind the 2-pass wide filter under the stand-in list (N.N' >= 0.9, plane distance <= 0.5 % of the diagonal),
                  both planes filtered
A record, not a test: every row is written as it comes out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAIRS = [(2, 1), (3, 1), (5, 4), (4, 3), (16, 4), (48, 47), (48, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=float, default=0.2, help="the segments' length as a share of the scene's diagonal")
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
        surface = ~(np.asarray(nrm)[..., :3] == 0).all(-1)
        q = api.WideFilterParams.make(2, 0.9, 0.005 * diag)
        for n, probe in PAIRS:
            for table in (0, 64):
                ao = api.AoParams.make(n, diag * args.radius, table=table, seed=5)
                full = api.ambient_occlusion(packed, k, ao, pos, nrm, W, H)
                counts, refined = api.ambient_occlusion_adaptive(packed, k, ao, pos, nrm, W, H, probe)
                lst = ao.stand_in_list()
                wide = lambda c: api.wide_filter_soft_light_list(lst, q, pos, nrm, c[None])[0]
                mad = lambda a, b: float(np.abs(a[surface] - b[surface]).mean())
                as_share = lambda c: c.astype(np.float32) / np.float32(n)
                rows.append({"scene": name, "n": n, "probe": probe, "table": table, "radius_share": args.radius,
                             "surface_pixels": int(surface.sum()), "differ": float((counts != full)[surface].mean()),
                             "refined": float(refined[surface].mean()), "raw": mad(as_share(counts), as_share(full)),
                             "filtered": mad(wide(counts), wide(full)), "full_mean": float(as_share(full)[surface].mean())})
                print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
