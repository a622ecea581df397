"""What the wide filter of the bent plane does to the DIRECTION, measured on the CPU with the host twins alone (no GPU): DESIGN.md 4.38.

    python tools/ao_bent_filter_quality.py [--out profiles/r46/ao_bent_filter_quality.jsonl] [--markdown FILE.jsonl]

Scenes: the cornell box at 128 x 128 and the terrain at 96 x 96 (the scenes of tests/golden/cornell_128.npz and terrain_96.npz).  Per scene,
n = 4 and 16 samples, table 0 and 64 (AoParams.make, seed 5), segments of 5 % and 20 % of the scene's diagonal: the raw bent plane of
rtsh_ambient_occlusion_bent and rtsh_wide_filter_bent of it after 1 .. 5 passes (N.N' >= 0.9, plane distance <= 0.5 % of the diagonal)
against the REFERENCE, the unfiltered 48-sample bent trace of the same radius without a table, over the pixels that have a surface and
whose reference vector is not zero:
    angle_deg   the mean angle between unit(xyz) and unit(reference xyz), in degrees (a zero vector counts as 90 degrees)
    h_mae       the mean absolute error of the combine's h = clamp(0.5 + 0.5 * unit(xyz) . up), up = +y
    worse       the share of those pixels whose angle is LARGER than the raw plane's by more than one degree
A record, not a test: every row is written as it comes out; `--markdown` prints the table for DESIGN.md, rows where a filtered figure is
worse than the raw one in bold."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = [(n, table, share) for n in (4, 16) for table in (0, 64) for share in (0.05, 0.20)]


def unit(v):
    length = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.divide(v, length, out=np.zeros_like(v), where=length > 0)


def angles(a, b):
    """Degrees between unit vectors; 90 where one of them is zero."""
    return np.degrees(np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0)))


def markdown(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    print("| scene | n | table | radius | figure | raw | 1 pass | 2 | 3 | 4 | 5 |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        for key, fmt in (("angle_deg", "{:.2f}"), ("h_mae", "{:.4f}")):
            cells = [fmt.format(v) for v in r[key]]
            cells = [cells[0]] + [f"**{c}**" if v > r[key][0] else c for c, v in zip(cells[1:], r[key][1:])]
            print(f"| {r['scene']} | {r['n']} | {r['table']} | {r['radius_share']:g} | {key} | " + " | ".join(cells) + " |")
        print(f"| {r['scene']} | {r['n']} | {r['table']} | {r['radius_share']:g} | worse | - | " + " | ".join(f"{v * 100:.1f} %" for v in r["worse"][1:]) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--markdown", default="", metavar="FILE.jsonl", help="print the table of a result file and exit")
    args = ap.parse_args()
    if args.markdown:
        return markdown(args.markdown)
    from raytracedshadows_amd import api, scenes
    rows = []
    up = np.array([0.0, 1.0, 0.0])
    for name, sc, W, H in (("cornell_128", scenes.cornell(), 128, 128), ("terrain_96", scenes.terrain(23), 96, 96)):
        verts, idx = sc.flat()
        packed = api.BVHBuilder().build(verts, 8, idx, sc.triangle_count).m_packedNodes
        pos, nrm, _ = api.primary_gbuffer(packed, sc.eye, sc.target, sc.fovy, W, H)
        k = api.RayTracingConstants.make(sc.eye, sc.light_direction, W, H)
        diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
        surface = ~(np.asarray(nrm)[..., :3] == 0).all(-1)
        refs = {}
        for n, table, share in CASES:
            if share not in refs:
                _, ref = api.ambient_occlusion_bent(packed, k, api.AoParams.make(48, diag * share, seed=5), pos, nrm, W, H)
                refs[share] = unit(ref[..., :3].astype(np.float64))
            ref = refs[share]
            where = surface & (np.abs(ref).sum(-1) > 0)
            h_ref = np.clip(0.5 + 0.5 * (ref * up).sum(-1), 0, 1)
            _, bent = api.ambient_occlusion_bent(packed, k, api.AoParams.make(n, diag * share, table=table, seed=5), pos, nrm, W, H)
            planes = [bent] + [api.wide_filter_bent(api.WideFilterParams.make(passes, 0.9, 0.005 * diag), n, pos, nrm, bent)[0]
                               for passes in range(1, 6)]
            row = {"scene": name, "n": n, "table": table, "radius_share": share, "pixels": int(where.sum()), "angle_deg": [], "h_mae": [],
                   "worse": []}
            raw_angle = None
            for plane in planes:
                u = unit(plane[..., :3].astype(np.float64))
                a = angles(u, ref)
                raw_angle = a if raw_angle is None else raw_angle
                row["angle_deg"].append(float(a[where].mean()))
                row["h_mae"].append(float(np.abs(np.clip(0.5 + 0.5 * (u * up).sum(-1), 0, 1) - h_ref)[where].mean()))
                row["worse"].append(float((a > raw_angle + 1.0)[where].mean()))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
