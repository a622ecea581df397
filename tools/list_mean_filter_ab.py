"""What the wide filters fed from the accumulated mean cost (GPU box), against their count-input counterparts.  DESIGN.md 4.28.

    python tools/list_mean_filter_ab.py [--parent-root <tree of the parent commit, built>] [--guide-k4 12] [--min-history 2]
                                        [--configs city_4k,courtyard_4k,atrium_1080p] [--out profiles/r32/list_mean_filter_ab.jsonl]

Rows: lists "4x4" = 4 lights of 4 samples and "2x16" = 2 lights of 16 (tools/soft_list_ab.py: entries), through the facing map, over
the moments of two accumulated frames (an orbit of 0.5 degree between them).
  "counterpart": rtsh_wide_filter_soft_light_list_device (unguided_ms) and rtsh_wide_filter_guided_temporal_soft_light_list_device
            (guided_ms) at 1 .. 5 passes; frame_ms: trace + moments + guided filter (3 passes) + visibility accumulation + visibility
            combine, the frame of DESIGN.md 4.27.  From the parent commit's library with --parent-root, else from this commit's own
            (each row says which in "library"): the count-input kernels of the two have the same instruction text
            (profiles/r32/kernel_resources.txt).
  "this":   rtsh_wide_filter_mean_soft_light_list_device (unguided_ms) and rtsh_wide_filter_guided_temporal_mean_soft_light_list_device
            (guided_ms) at the same passes; frame_ms: trace + moments + guided mean filter (3 passes) + visibility combine -- the mean is
            already integrated, the float accumulation after the filter is left out.
Each figure: 10 warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of its own,
under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.  After the rows of a
config: one "ratio" row per list, this over counterpart.  No threshold: every row is reported; 4.23 records 18 % run-to-run movement on
these passes, so the second digit of a ratio carries no weight."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
LISTS = {"4x4": (4, 4), "2x16": (2, 16)}
PASSES = (1, 2, 3, 4, 5)
ORBIT_DEG = 0.5


def child(mode, config, root, k4, min_history):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, scenes, workloads
    from list_moments_ab import orbit
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
            vis = lambda src: api.combine_visibility_list_device(ctx, wl.constants, hard, d_pos, d_nrm, src, W, H, d_rgb, d_lights_map=d_map,
                                                                 colors=colors)
            prev_eye = orbit(sc.eye, sc.target, -ORBIT_DEG)
            tp = api.TemporalParams.from_cameras((sc.eye, sc.target, sc.fovy), (prev_eye, sc.target, sc.fovy), W, H, 0.9, 0.005 * diag, 32)
            # the previous frame: its G-buffer, its counts, its moments and its visibility history as a first frame into set 0
            api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_ppos, d_pnrm)
            api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
            facing(), trace()
            api.accumulate_moments_soft_light_list_device(ctx, lights, tp, d_pos, d_nrm, d_counts, W, H, *d_mom[0], d_lights_map=d_map)
            api.wide_filter_soft_light_list_device(ctx, lights, api.WideFilterParams.make(0, 0.9, 0.05), d_pos, d_nrm, d_counts, W, H, d_vis,
                                                   d_lights_map=d_map)
            api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_hist[0], d_len[0], d_lights_map=d_map)
            api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
            facing(), trace()
            mom = lambda: api.accumulate_moments_soft_light_list_device(ctx, lights, tp, d_pos, d_nrm, d_counts, W, H, *d_mom[1],
                                                                        d_prev=(d_ppos, d_pnrm) + d_mom[0], d_lights_map=d_map)
            acc = lambda: api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_hist[1], d_len[1],
                                                                d_prev=(d_ppos, d_pnrm, d_hist[0], d_len[0]), d_lights_map=d_map)
            mom()
            ctx.synchronize()
            for passes in PASSES:
                up, tg = api.WideFilterParams.make(passes, 0.9, 0.05), api.WideGuideTemporalParams.make(passes, k4, min_history, 0.9, 0.05)
                r = {"config": config, "mode": "this" if mode == "this" else "counterpart", "library": mode, "list": name, "steps": STEPS,
                     "warmup": WARMUP, "passes": passes, "guide_k4": k4, "min_history": min_history}
                if mode == "this":
                    unguided = lambda: api.wide_filter_mean_soft_light_list_device(ctx, lights, up, d_pos, d_nrm, d_mom[1][0], W, H, d_vis,
                                                                                   d_scratch=d_scratch, d_lights_map=d_map)
                    guided = lambda: api.wide_filter_guided_temporal_mean_soft_light_list_device(ctx, lights, tg, d_pos, d_nrm, d_counts, d_mom[1],
                                                                                                 W, H, d_vis, d_scratch=d_scratch,
                                                                                                 d_lights_map=d_map)
                    frame = lambda: (trace(), mom(), guided(), vis(d_vis))
                else:
                    unguided = lambda: api.wide_filter_soft_light_list_device(ctx, lights, up, d_pos, d_nrm, d_counts, W, H, d_vis,
                                                                              d_scratch=d_scratch, d_lights_map=d_map)
                    guided = lambda: api.wide_filter_guided_temporal_soft_light_list_device(ctx, lights, tg, d_pos, d_nrm, d_counts, d_mom[1], W,
                                                                                            H, d_vis, d_scratch=d_scratch, d_lights_map=d_map)
                    frame = lambda: (trace(), mom(), guided(), acc(), vis(d_hist[1]))
                r["unguided_ms"] = med(_timed(ctx, unguided, STEPS, WARMUP))
                r["guided_ms"] = med(_timed(ctx, guided, STEPS, WARMUP))
                if passes == 3:
                    r["frame_ms"] = med(_timed(ctx, frame, STEPS, WARMUP))
                print(json.dumps(r), flush=True)


def ratios(rows, config):
    out = []
    for name in LISTS:
        mine = [r for r in rows if r["config"] == config and r["list"] == name]
        pick = lambda mode, key, n: next((r[key] for r in mine if r["mode"] == mode and key in r and r["passes"] == n), None)
        r = {"config": config, "mode": "ratio", "list": name}
        try:
            for key in ("unguided_ms", "guided_ms"):
                r[key[:-3] + "_mean_over_counts"] = {f"passes{n}": round(pick("this", key, n) / pick("counterpart", key, n), 3) for n in PASSES}
            r["frame"] = round(pick("this", "frame_ms", 3) / pick("counterpart", "frame_ms", 3), 3)
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
    ap.add_argument("--out", default="profiles/r32/list_mean_filter_ab.jsonl")
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
            runs = [("parent", os.path.abspath(args.parent_root)) if args.parent_root else ("this_library_count_input", ROOT), ("this", ROOT)]
            rows = []
            for mode, root in runs:
                env = dict(os.environ)
                env.pop("RTS_LIB", None)
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root, str(args.guide_k4),
                                      str(args.min_history)], env=env, capture_output=True, text=True, timeout=400)
                if run.returncode != 0:
                    sys.exit(f"list_mean_filter_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                for line in run.stdout.splitlines():
                    if line.startswith("{"):
                        rows.append(json.loads(line))
                        emit(line)
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
