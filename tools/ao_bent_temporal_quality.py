"""What accumulating the bent texel over frames does to the DIRECTION, measured on the CPU with the host twins alone (no GPU):
DESIGN.md 4.39.

    python tools/ao_bent_temporal_quality.py [--out profiles/r47/ao_bent_temporal_quality.jsonl] [--markdown FILE.jsonl]

Scenes: the cornell box at 128 x 128 and the terrain at 96 x 96.  n = 4 samples, table 0 and 64 (AoParams.make, seed 5), segments of 5 %
of the scene's diagonal.  A frame loop of F = 1, 4, 8, 16 frames with max_length = F, the camera still or orbiting the target by 1 degree
per frame (the LAST frame is the scene's own camera): per frame the G-buffer (rtsh_primary_gbuffer), the bent trace with `dirs` turned
about the normal by k golden angles (AoParams.rotated), rtsh_accumulate_bent with ping-pong; on the last frame rtsh_wide_filter_bent_mean
with 0 and 2 passes (N.N' >= 0.9, plane distance <= 0.5 % of the diagonal; the accumulate's thresholds are the same) against the
REFERENCE, the unfiltered 48-sample bent trace of the last frame without a table, over the pixels that have a surface and whose
reference vector is not zero:
    angle_deg   the mean angle between unit(xyz) and unit(reference xyz), in degrees (a zero vector counts as 90 degrees)
    h_mae       the mean absolute error of the combine's h = clamp(0.5 + 0.5 * unit(xyz) . up), up = +y
    worse       the share of those pixels whose angle is LARGER than the single frame's (F = 1, the same passes) by more than one degree
A record, not a test: every row is written as it comes out; `--markdown` prints the table for DESIGN.md, figures worse than the single
frame's in bold."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FRAMES = (1, 4, 8, 16)
PASSES = (0, 2)


def unit(v):
    length = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.divide(v, length, out=np.zeros_like(v), where=length > 0)


def angles(a, b):
    """Degrees between unit vectors; 90 where one of them is zero."""
    return np.degrees(np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0)))


def markdown(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    print("| scene | table | camera | passes | figure | F = 1 | 4 | 8 | 16 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        for key, fmt in (("angle_deg", "{:.2f}"), ("h_mae", "{:.4f}")):
            cells = [fmt.format(v) for v in r[key]]
            cells = [cells[0]] + [f"**{c}**" if v > r[key][0] else c for c, v in zip(cells[1:], r[key][1:])]
            print(f"| {r['scene']} | {r['table']} | {r['camera']} | {r['passes']} | {key} | " + " | ".join(cells) + " |")
        print(f"| {r['scene']} | {r['table']} | {r['camera']} | {r['passes']} | worse | - | " +
              " | ".join(f"{v * 100:.1f} %" for v in r["worse"][1:]) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--markdown", default="", metavar="FILE.jsonl", help="print the table of a result file and exit")
    args = ap.parse_args()
    if args.markdown:
        return markdown(args.markdown)
    from list_temporal_ab import orbit
    from raytracedshadows_amd import api, scenes
    rows = []
    up = np.array([0.0, 1.0, 0.0])
    n, share = 4, 0.05
    for name, sc, W, H in (("cornell_128", scenes.cornell(), 128, 128), ("terrain_96", scenes.terrain(23), 96, 96)):
        verts, idx = sc.flat()
        packed = api.BVHBuilder().build(verts, 8, idx, sc.triangle_count).m_packedNodes
        diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
        cos_min, plane_eps = 0.9, 0.005 * diag
        gbuffers = {}

        def gbuffer(eye):
            key = tuple(float(v) for v in eye)
            if key not in gbuffers:
                pos, nrm, _ = api.primary_gbuffer(packed, eye, sc.target, sc.fovy, W, H)
                gbuffers[key] = (pos, nrm, api.RayTracingConstants.make(eye, sc.light_direction, W, H))
            return gbuffers[key]

        pos, nrm, k = gbuffer(sc.eye)
        surface = ~(np.asarray(nrm)[..., :3] == 0).all(-1)
        _, ref = api.ambient_occlusion_bent(packed, k, api.AoParams.make(48, diag * share, seed=5), pos, nrm, W, H)
        ref = unit(ref[..., :3].astype(np.float64))
        where = surface & (np.abs(ref).sum(-1) > 0)
        h_ref = np.clip(0.5 + 0.5 * (ref * up).sum(-1), 0, 1)
        for table in (0, 64):
            ao = api.AoParams.make(n, diag * share, table=table, seed=5)
            for camera, degrees in (("still", 0.0), ("orbit", 1.0)):
                by_passes = {passes: {"angle_deg": [], "h_mae": [], "worse": [], "single": None} for passes in PASSES}
                for frames in FRAMES:
                    eyes = [orbit(sc.eye, sc.target, degrees * (f - (frames - 1))) for f in range(frames)]
                    prev = None
                    for f, eye in enumerate(eyes):
                        p, m, kk = gbuffer(eye)
                        _, bent = api.ambient_occlusion_bent(packed, kk, ao.rotated(f), p, m, W, H)
                        if f:
                            b = api.camera_basis(eyes[f - 1], sc.target, sc.fovy, W, H)
                            tp = api.TemporalParams.make(np.asarray(eye, np.float32) - np.asarray(eyes[f - 1], np.float32), b["right"], b["up"],
                                                         b["fwd"], np.float32(b["tan_half"] * b["aspect"]), b["tan_half"], cos_min, plane_eps,
                                                         frames, 0)
                        else:
                            tp = api.TemporalParams.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1.0, 1.0, cos_min, plane_eps, frames, 0)
                        texels, lengths = api.accumulate_bent(tp, n, p, m, bent, prev)
                        prev = (p, m, texels, lengths)
                    for passes in PASSES:
                        out, _ = api.wide_filter_bent_mean(api.WideFilterParams.make(passes, cos_min, plane_eps), n, pos, nrm, prev[2])
                        u = unit(out[..., :3].astype(np.float64))
                        a = angles(u, ref)
                        r = by_passes[passes]
                        r["single"] = a if r["single"] is None else r["single"]
                        r["angle_deg"].append(float(a[where].mean()))
                        r["h_mae"].append(float(np.abs(np.clip(0.5 + 0.5 * (u * up).sum(-1), 0, 1) - h_ref)[where].mean()))
                        r["worse"].append(float((a > r["single"] + 1.0)[where].mean()))
                for passes in PASSES:
                    r = by_passes[passes]
                    row = {"scene": name, "n": n, "table": table, "radius_share": share, "camera": camera, "orbit_deg": degrees, "passes": passes,
                           "frames": list(FRAMES), "pixels": int(where.sum()), "angle_deg": r["angle_deg"], "h_mae": r["h_mae"], "worse": r["worse"]}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
