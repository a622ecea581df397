"""What the count moments and the temporal guide of the wide filter cost (GPU box), against the PARENT commit's library on the same
frames.  DESIGN.md 4.27.

    python tools/list_moments_ab.py --parent-root <tree of the parent commit, built> [--guide-k4 12] [--min-history 2]
                                    [--configs city_4k,courtyard_4k,atrium_1080p] [--out profiles/r31/list_moments_ab.jsonl]

Rows: lists "4x4" = 4 lights of 4 samples and "2x16" = 2 lights of 16 (tools/soft_list_ab.py: entries), through the facing map.
  "parent": the parent commit's library -- accumulate_ms: rtsh_accumulate_visibility_list_device (unclamped) over the passes == 0 plane,
            still camera and an orbit of 0.5 degree; filter_ms: rtsh_wide_filter_guided_soft_light_list_device at 1 .. 5 passes, and
            unguided_ms: rtsh_wide_filter_soft_light_list_device at the same passes; frame_ms: trace + guided filter (3 passes) +
            accumulate + visibility combine.
  "this":   this commit's -- moments_ms: rtsh_accumulate_moments_soft_light_list_device on the same two motions (it gathers the same
            taps and moves 7 bytes of history per tap and light where the float pass moves 5); filter_ms:
            rtsh_wide_filter_guided_temporal_soft_light_list_device at 1 .. 5 passes over moments of two accumulated frames (lengths up to 2: --min-history 2 sends them down the temporal branch);
            frame_ms: trace + moments + temporal-guided filter (3 passes) + accumulate + visibility combine.
Each figure: 10 warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of its own,
under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.  After the rows of a
config: one "ratio" row per list, with "first_pass_over_guided_plus_one_unguided": the temporal guide's ONE-pass filter over the
parent's one-pass guided filter plus the difference between two and one unguided passes (one more unguided pass).  No threshold: every
row is reported."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
LISTS = {"4x4": (4, 4), "2x16": (2, 16)}
PASSES = (1, 2, 3, 4, 5)
ORBIT_DEG = 0.5


def orbit(eye, target, degrees):
    a = math.radians(degrees)
    dx, dz = eye[0] - target[0], eye[2] - target[2]
    return (target[0] + dx * math.cos(a) - dz * math.sin(a), eye[1], target[2] + dx * math.sin(a) + dz * math.cos(a))


def child(mode, config, root, k4, min_history):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, scenes, workloads
    from soft_list_ab import _timed, entries
    wl = workloads.prepare_config(config, cache=True)
    W, H, n = wl.W, wl.H, wl.W * wl.H
    sc = wl.scene
    med = lambda ts: float(np.median(ts))
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_ppos, d_pnrm, d_map = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n)
        d_counts, d_vis, d_rgb, d_scratch = ctx.malloc(4 * n), ctx.malloc(16 * n), ctx.malloc(3 * n), ctx.malloc(24 * n)
        d_hist, d_len = [ctx.malloc(16 * n), ctx.malloc(16 * n)], [ctx.malloc(4 * n), ctx.malloc(4 * n)]
        d_mom = [(ctx.malloc(8 * n), ctx.malloc(16 * n), ctx.malloc(4 * n)) for _ in range(2)]
        diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
        for name, (count, spp) in LISTS.items():
            lights = api.SoftLightList.make(entries(sc, count, spp), scenes.jitter_offsets(48, 1.0, 19))
            hard = lights.hard_list()
            colors = np.full((count, 3), 1.0 / count, np.float32)
            facing = lambda: api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
            trace = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_map)
            convert = lambda: api.wide_filter_soft_light_list_device(ctx, lights, api.WideFilterParams.make(0, 0.9, 0.05), d_pos, d_nrm, d_counts, W,
                                                                     H, d_vis, d_lights_map=d_map)
            vis = lambda src: api.combine_visibility_list_device(ctx, wl.constants, hard, d_pos, d_nrm, src, W, H, d_rgb, d_lights_map=d_map,
                                                                 colors=colors)
            row = {"config": config, "mode": mode, "list": name, "steps": STEPS, "warmup": WARMUP}
            for motion, degrees in (("still", 0.0), ("orbit", ORBIT_DEG)):
                prev_eye = orbit(sc.eye, sc.target, -degrees)
                tp = api.TemporalParams.from_cameras((sc.eye, sc.target, sc.fovy), (prev_eye, sc.target, sc.fovy), W, H, 0.9, 0.005 * diag, 32)
                # the previous frame: its G-buffer, its planes, accumulated as a first frame into set 0
                api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
                facing(), trace(), convert()
                api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_hist[0], d_len[0], d_lights_map=d_map)
                if mode == "this":
                    api.accumulate_moments_soft_light_list_device(ctx, lights, tp, d_pos, d_nrm, d_counts, W, H, *d_mom[0], d_lights_map=d_map)
                api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_ppos, d_pnrm)
                api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
                facing(), trace(), convert()
                ctx.synchronize()
                acc = lambda: api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_hist[1], d_len[1],
                                                                    d_prev=(d_ppos, d_pnrm, d_hist[0], d_len[0]), d_lights_map=d_map)
                r = dict(row, motion=motion)
                if mode == "parent":
                    r["accumulate_ms"] = med(_timed(ctx, acc, STEPS, WARMUP))
                else:
                    mom = lambda: api.accumulate_moments_soft_light_list_device(ctx, lights, tp, d_pos, d_nrm, d_counts, W, H, *d_mom[1],
                                                                                d_prev=(d_ppos, d_pnrm) + d_mom[0], d_lights_map=d_map)
                    r["moments_ms"] = med(_timed(ctx, mom, STEPS, WARMUP))
                print(json.dumps(r), flush=True)
            # the filters, on the current frame (the orbit's moments: lengths 2 where history was found)
            for passes in PASSES:
                r = dict(row, passes=passes, guide_k4=k4)
                if mode == "parent":
                    gp, up = api.WideGuideParams.make(passes, k4, 0.9, 0.05), api.WideFilterParams.make(passes, 0.9, 0.05)
                    filt = lambda: api.wide_filter_guided_soft_light_list_device(ctx, lights, gp, d_pos, d_nrm, d_counts, W, H, d_vis,
                                                                                 d_scratch=d_scratch, d_lights_map=d_map)
                    unguided = lambda: api.wide_filter_soft_light_list_device(ctx, lights, up, d_pos, d_nrm, d_counts, W, H, d_vis,
                                                                              d_scratch=d_scratch, d_lights_map=d_map)
                    r["unguided_ms"] = med(_timed(ctx, unguided, STEPS, WARMUP))
                else:
                    tg = api.WideGuideTemporalParams.make(passes, k4, min_history, 0.9, 0.05)
                    r["min_history"] = min_history
                    filt = lambda: api.wide_filter_guided_temporal_soft_light_list_device(ctx, lights, tg, d_pos, d_nrm, d_counts, d_mom[1], W, H,
                                                                                          d_vis, d_scratch=d_scratch, d_lights_map=d_map)
                r["filter_ms"] = med(_timed(ctx, filt, STEPS, WARMUP))
                if passes == 3:
                    if mode == "parent":
                        r["frame_ms"] = med(_timed(ctx, lambda: (trace(), filt(), acc(), vis(d_hist[1])), STEPS, WARMUP))
                    else:
                        r["frame_ms"] = med(_timed(ctx, lambda: (trace(), mom(), filt(), acc(), vis(d_hist[1])), STEPS, WARMUP))
                print(json.dumps(r), flush=True)


def ratios(rows, config):
    out = []
    for name in LISTS:
        mine = [r for r in rows if r["config"] == config and r["list"] == name]
        pick = lambda mode, key, **kw: next((r[key] for r in mine if r["mode"] == mode and key in r and all(r.get(a) == b for a, b in kw.items())), None)
        r = {"config": config, "mode": "ratio", "list": name}
        try:
            r["moments_over_accumulate"] = {m: pick("this", "moments_ms", motion=m) / pick("parent", "accumulate_ms", motion=m) for m in ("still", "orbit")}
            r["temporal_over_guided_filter"] = {f"passes{n}": pick("this", "filter_ms", passes=n) / pick("parent", "filter_ms", passes=n) for n in PASSES}
            one_more = pick("parent", "unguided_ms", passes=2) - pick("parent", "unguided_ms", passes=1)
            r["first_pass_over_guided_plus_one_unguided"] = pick("this", "filter_ms", passes=1) / (pick("parent", "filter_ms", passes=1) + one_more)
            r["frame"] = pick("this", "frame_ms", passes=3) / pick("parent", "frame_ms", passes=3)
        except TypeError:
            continue
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--guide-k4", type=int, default=12)
    ap.add_argument("--min-history", type=int, default=2)
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r31/list_moments_ab.jsonl")
    ap.add_argument("--child", nargs=5, metavar=("MODE", "CONFIG", "ROOT", "K4", "MIN_HISTORY"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.child[2], int(args.child[3]), int(args.child[4]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        def emit(line):
            out.write(line + "\n")
            out.flush()
            print(line, flush=True)
        for config in args.configs.split(","):
            runs = [("this", ROOT)]
            if args.parent_root:
                runs.insert(0, ("parent", os.path.abspath(args.parent_root)))
            rows = []
            for mode, root in runs:
                env = dict(os.environ)
                env.pop("RTS_LIB", None)
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root, str(args.guide_k4),
                                      str(args.min_history)], env=env, capture_output=True, text=True, timeout=400)
                if run.returncode != 0:
                    sys.exit(f"list_moments_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                for line in run.stdout.splitlines():
                    if line.startswith("{"):
                        rows.append(json.loads(line))
                        emit(line)
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
