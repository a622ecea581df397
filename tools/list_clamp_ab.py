"""What the neighbourhood clamp of the temporal accumulation costs (GPU box).  B: the clamped pass of this commit at r = 1, 2 and 4.
A: the unclamped pass of the PARENT commit's library (a built tree of the parent commit, --parent-root).  The frames are those of
tools/list_temporal_ab.py (profiles/r26/list_temporal_ab.jsonl): a still camera and an orbit of 0.5 degree per frame, lists "4x4" and
"2x16" through the facing map, the filter at R = 2 -- and the whole frame, trace + filter + accumulate + visibility combine, for the
still camera.  DESIGN.md 4.24.

    python tools/list_clamp_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,courtyard_4k,atrium_1080p]
                                  [--out profiles/r28/list_clamp_ab.jsonl] [--reps 2]

Each figure: 10 warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of its own,
under its own time limit, A and B alternating `reps` times (the smallest median of a row is kept, and every repetition is written);
this process never opens the GPU, and the tool stops at the first child that fails.  No threshold: after the raw rows one "ratio" row
per (config, list, motion, radius) gives B/A of the pass, the milliseconds the clamp adds, and B/A of the frame."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
RADII = (1, 2, 4)


def child(mode, config, root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, scenes, workloads
    from list_temporal_ab import LISTS, ORBIT_DEG, RADIUS, orbit
    from soft_list_ab import _timed, entries
    wl = workloads.prepare_config(config, cache=True)
    W, H, n = wl.W, wl.H, wl.W * wl.H
    med = lambda ts: float(np.median(ts))
    sc = wl.scene
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_map = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n)
        d_counts, d_vis, d_rgb = ctx.malloc(4 * n), ctx.malloc(16 * n), ctx.malloc(3 * n)
        d_ppos, d_pnrm = ctx.malloc(n * 16), ctx.malloc(n * 16)
        d_hist = [ctx.malloc(16 * n), ctx.malloc(16 * n)]
        d_len = [ctx.malloc(4 * n), ctx.malloc(4 * n)]
        for name, (count, spp) in LISTS.items():
            lights = api.SoftLightList.make(entries(sc, count, spp), scenes.jitter_offsets(48, 1.0, 19))
            hard = lights.hard_list()
            colors = np.full((count, 3), 1.0 / count, np.float32)
            fp = api.FilterParams.make(RADIUS, 0.9, 0.05, 0.25)
            facing = lambda: api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
            trace = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_map)
            filt = lambda: api.filter_soft_light_list_device(ctx, lights, fp, d_pos, d_nrm, d_counts, W, H, d_vis, d_lights_map=d_map)
            vis = lambda src: api.combine_visibility_list_device(ctx, wl.constants, hard, d_pos, d_nrm, src, W, H, d_rgb, d_lights_map=d_map,
                                                                 colors=colors)
            diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
            for motion, degrees in (("still", 0.0), ("orbit", ORBIT_DEG)):
                prev_eye = orbit(sc.eye, sc.target, -degrees)
                tp = api.TemporalParams.from_cameras((sc.eye, sc.target, sc.fovy), (prev_eye, sc.target, sc.fovy), W, H, 0.9, 0.005 * diag, 32)
                # the previous frame: its G-buffer, its visibility, accumulated as a first frame into history 0
                api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
                facing(), trace(), filt()
                api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_hist[0], d_len[0], d_lights_map=d_map)
                api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_ppos, d_pnrm)
                api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
                facing(), trace(), filt()
                ctx.synchronize()
                for radius in ((None,) if mode == "parent" else (None,) + RADII):
                    extra = {} if radius is None else {"clamp": api.HistoryClamp.make(radius, 0.0)}
                    acc = lambda: api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_hist[1], d_len[1],
                                                                        d_prev=(d_ppos, d_pnrm, d_hist[0], d_len[0]), d_lights_map=d_map, **extra)
                    r = {"config": config, "mode": mode, "list": name, "motion": motion, "clamp_radius": radius, "filter_radius": RADIUS,
                         "steps": STEPS, "warmup": WARMUP}
                    r["accumulate_ms"] = med(_timed(ctx, acc, STEPS, WARMUP))
                    if motion == "still":
                        r["frame_ms"] = med(_timed(ctx, lambda: (trace(), filt(), acc(), vis(d_hist[1])), STEPS, WARMUP))
                    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=False, default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r28/list_clamp_ab.jsonl")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--child", nargs=3, metavar=("MODE", "CONFIG", "ROOT"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if not args.parent_root:
        sys.exit("list_clamp_ab: --parent-root is required: A is the parent commit's library")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
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
                        sys.exit(f"list_clamp_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                    for line in run.stdout.splitlines():
                        if not line.startswith("{"):
                            continue
                        row = dict(json.loads(line), rep=rep)
                        out.write(json.dumps(row) + "\n")
                        out.flush()
                        key = (row["config"], row["mode"], row["list"], row["motion"], row["clamp_radius"])
                        for field in ("accumulate_ms", "frame_ms"):
                            if field in row:
                                best[key + (field,)] = min(best.get(key + (field,), float("inf")), row[field])
        for (config, mode, name, motion, radius, field), b in sorted(best.items(), key=str):
            if mode != "this" or radius is None or field != "accumulate_ms":
                continue
            a = best[(config, "parent", name, motion, None, "accumulate_ms")]
            row = {"config": config, "mode": "ratio", "list": name, "motion": motion, "clamp_radius": radius, "a_unclamped_parent_ms": a,
                   "b_clamped_ms": b, "b_over_a": b / a, "added_ms": b - a,
                   "this_unclamped_over_parent": best[(config, "this", name, motion, None, "accumulate_ms")] / a}
            if motion == "still":
                fa, fb = best[(config, "parent", name, motion, None, "frame_ms")], best[(config, "this", name, motion, radius, "frame_ms")]
                row.update(a_frame_ms=fa, b_frame_ms=fb, frame_b_over_a=fb / fa)
            out.write(json.dumps(row) + "\n")
            print(json.dumps(row))


if __name__ == "__main__":
    main()
