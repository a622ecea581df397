"""What the clamp of the moments' history costs (GPU box).  B: the clamped moments pass of this commit at r = 1, 2 and 4 (sigma_k4 8),
and its motion form.  A: the unclamped moments pass (and its motion form) of the PARENT commit's library (a built tree of the parent
commit, --parent-root).  The frames are those of tools/list_temporal_ab.py and tools/list_clamp_ab.py: a still camera and an orbit of
0.5 degree per frame, lists "4x4" and "2x16" through the facing map -- and the whole frame, trace + moments + guided temporal mean
filter (two passes, guide_k4 12) + visibility combine, for the still camera, with and without the clamp.  DESIGN.md 4.30.

    python tools/list_moments_clamp_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,courtyard_4k,atrium_1080p]
                                          [--out profiles/r35/list_moments_clamp_ab.jsonl] [--reps 2]

Each figure: 10 warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of its own,
under its own time limit, A and B alternating `reps` times (the smallest median of a row is kept, and every repetition is written);
this process never opens the GPU, and the tool stops at the first child that fails.  No threshold: after the raw rows one "ratio" row
per (config, list, motion, form, radius) gives B/A of the pass, the milliseconds the clamp adds, this library's unclamped pass over
the parent's (the noise yardstick) and B/A of the frame; "worse_than_float_clamp" marks a row whose B/A exceeds 2.02 (the float
clamp's worst) or whose added milliseconds exceed what the float clamp added on the same row of --float-clamp-rows
(profiles/r28/list_clamp_ab.jsonl)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
RADII = (1, 2, 4)
SIGMA_K4 = 8


def child(mode, config, root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, scenes, workloads
    from list_temporal_ab import LISTS, ORBIT_DEG, orbit
    from soft_list_ab import _timed, entries
    wl = workloads.prepare_config(config, cache=True)
    W, H, n = wl.W, wl.H, wl.W * wl.H
    med = lambda ts: float(np.median(ts))
    sc = wl.scene
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        nv = api.bvh_count_device(ctx)
        d_snap = ctx.malloc(nv * 16)
        api.snapshot_bvh_device(ctx, d_snap, nv)
        d_pos, d_nrm, d_map = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n)
        d_pts, d_pnr = ctx.malloc(n * 16), ctx.malloc(n * 16)
        d_counts, d_vis, d_rgb, d_scratch = ctx.malloc(4 * n), ctx.malloc(16 * n), ctx.malloc(3 * n), ctx.malloc(3 * 4 * n * 2)
        d_ppos, d_pnrm = ctx.malloc(n * 16), ctx.malloc(n * 16)
        d_mom = [(ctx.malloc(4 * n * 2), ctx.malloc(4 * n * 4), ctx.malloc(4 * n)) for _ in range(2)]
        for name, (count, spp) in LISTS.items():
            lights = api.SoftLightList.make(entries(sc, count, spp), scenes.jitter_offsets(48, 1.0, 19))
            hard = lights.hard_list()
            colors = np.full((count, 3), 1.0 / count, np.float32)
            diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
            gp = api.WideGuideTemporalParams.make(2, 12, 4, 0.9, 0.005 * diag)
            facing = lambda: api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
            trace = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_map)
            filt = lambda: api.wide_filter_guided_temporal_mean_soft_light_list_device(ctx, lights, gp, d_pos, d_nrm, d_counts, d_mom[1], W, H, d_vis,
                                                                                       d_scratch=d_scratch, d_lights_map=d_map)
            vis = lambda: api.combine_visibility_list_device(ctx, wl.constants, hard, d_pos, d_nrm, d_vis, W, H, d_rgb, d_lights_map=d_map,
                                                             colors=colors)
            for motion, degrees in (("still", 0.0), ("orbit", ORBIT_DEG)):
                prev_eye = orbit(sc.eye, sc.target, -degrees)
                tp = api.TemporalParams.from_cameras((sc.eye, sc.target, sc.fovy), (prev_eye, sc.target, sc.fovy), W, H, 0.9, 0.005 * diag, 32)
                # the previous frame: its G-buffer and counts, accumulated as a first frame into history 0
                api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
                facing(), trace()
                api.accumulate_moments_soft_light_list_device(ctx, lights, tp, d_pos, d_nrm, d_counts, W, H, *d_mom[0], d_lights_map=d_map)
                api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_ppos, d_pnrm)
                api.primary_gbuffer_motion_device(ctx, d_snap, nv, sc.eye, prev_eye, sc.target, sc.fovy, W, H, d_pos, d_nrm, d_pts, d_pnr)
                facing(), trace()
                ctx.synchronize()
                for form in ("plain", "motion"):
                    for radius in ((None,) if mode == "parent" else (None,) + RADII):
                        extra = {} if radius is None else {"clamp": api.MomentsClamp.make(radius, SIGMA_K4, 0)}
                        if form == "motion":
                            extra["d_motion"] = (d_pts, d_pnr)
                        acc = lambda: api.accumulate_moments_soft_light_list_device(ctx, lights, tp, d_pos, d_nrm, d_counts, W, H, *d_mom[1],
                                                                                    d_prev=(d_ppos, d_pnrm) + d_mom[0], d_lights_map=d_map, **extra)
                        r = {"config": config, "mode": mode, "list": name, "motion": motion, "form": form, "clamp_radius": radius,
                             "sigma_k4": SIGMA_K4, "steps": STEPS, "warmup": WARMUP}
                        r["moments_ms"] = med(_timed(ctx, acc, STEPS, WARMUP))
                        if motion == "still" and form == "plain":
                            r["frame_ms"] = med(_timed(ctx, lambda: (trace(), acc(), filt(), vis()), STEPS, WARMUP))
                        print(json.dumps(r), flush=True)


def float_clamp_added(path):
    """(config, list, motion, radius) -> the milliseconds 4.24's float clamp added, from its recorded ratio rows."""
    out = {}
    if path and os.path.exists(path):
        for line in open(path):
            row = json.loads(line)
            if row.get("mode") == "ratio":
                out[(row["config"], row["list"], row["motion"], row["clamp_radius"])] = row["added_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=False, default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r35/list_moments_clamp_ab.jsonl")
    ap.add_argument("--float-clamp-rows", default=os.path.join(ROOT, "profiles", "r28", "list_clamp_ab.jsonl"))
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--child", nargs=3, metavar=("MODE", "CONFIG", "ROOT"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if not args.parent_root:
        sys.exit("list_moments_clamp_ab: --parent-root is required: A is the parent commit's library")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    added_by_float = float_clamp_added(args.float_clamp_rows)
    best = {}
    with open(args.out, "w") as out:
        for config in args.configs.split(","):
            for rep in range(args.reps):
                for mode, root in (("parent", os.path.abspath(args.parent_root)), ("this", ROOT)):
                    env = dict(os.environ)
                    env.pop("RTS_LIB", None)
                    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root], env=env, capture_output=True,
                                         text=True, timeout=300)
                    if run.returncode != 0:
                        sys.exit(f"list_moments_clamp_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                    for line in run.stdout.splitlines():
                        if not line.startswith("{"):
                            continue
                        row = dict(json.loads(line), rep=rep)
                        out.write(json.dumps(row) + "\n")
                        out.flush()
                        key = (row["config"], row["mode"], row["list"], row["motion"], row["form"], row["clamp_radius"])
                        for field in ("moments_ms", "frame_ms"):
                            if field in row:
                                best[key + (field,)] = min(best.get(key + (field,), float("inf")), row[field])
        for (config, mode, name, motion, form, radius, field), b in sorted(best.items(), key=str):
            if mode != "this" or radius is None or field != "moments_ms":
                continue
            a = best[(config, "parent", name, motion, form, None, "moments_ms")]
            row = {"config": config, "mode": "ratio", "list": name, "motion": motion, "form": form, "clamp_radius": radius,
                   "a_unclamped_parent_ms": a, "b_clamped_ms": b, "b_over_a": b / a, "added_ms": b - a,
                   "this_unclamped_over_parent": best[(config, "this", name, motion, form, None, "moments_ms")] / a}
            float_added = added_by_float.get((config, name, motion, radius))
            row["float_clamp_added_ms"] = float_added
            row["worse_than_float_clamp"] = bool(b / a > 2.02 or (float_added is not None and b - a > float_added))
            if motion == "still" and form == "plain":
                fa, fb = best[(config, "parent", name, motion, form, None, "frame_ms")], best[(config, "this", name, motion, form, radius, "frame_ms")]
                row.update(a_frame_ms=fa, b_frame_ms=fb, frame_b_over_a=fb / fa)
            out.write(json.dumps(row) + "\n")
            print(json.dumps(row))


if __name__ == "__main__":
    main()
