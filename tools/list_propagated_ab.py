"""What carrying the variance through the passes costs (GPU box): the propagated filter against the guided mean filter.  DESIGN.md 4.31.

    python tools/list_propagated_ab.py [--parent-root <tree of the parent commit, built>] [--guide-k4 12] [--min-history 2]
                                       [--configs city_4k,courtyard_4k,atrium_1080p] [--out profiles/r36/list_propagated_ab.jsonl]

Rows: lists "4x4" = 4 lights of 4 samples and "2x16" = 2 lights of 16 (tools/soft_list_ab.py: entries), through the facing map, over
the moments of two accumulated frames (an orbit of 0.5 degree between them), as in tools/list_mean_filter_ab.py.
  "parent": rtsh_wide_filter_guided_temporal_mean_soft_light_list_device at 1 .. 5 passes (filter_ms), from the parent commit's library
            with --parent-root, else from this commit's own (each row says which in "library"): the kernels of the two have the same
            instruction text (profiles/r36/kernel_resources.txt).
  "this":   rtsh_wide_filter_propagated_mean_soft_light_list_device at the same passes, by_length 0 (filter_ms) and 1 (by_length_ms).
Each figure: 10 warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of its own,
under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.  After the rows of a
config one "ratio" row per list: this over parent at equal passes, and this at n passes over parent at n + 1 -- what a pass saved
would have to pay for.  No threshold: every row is reported."""
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
        d_counts, d_vis, d_scratch = ctx.malloc(4 * n), ctx.malloc(16 * n), ctx.malloc(48 * n)
        d_mom = [(ctx.malloc(8 * n), ctx.malloc(16 * n), ctx.malloc(4 * n)) for _ in range(2)]
        diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
        for name, (count, spp) in LISTS.items():
            lights = api.SoftLightList.make(entries(sc, count, spp), scenes.jitter_offsets(48, 1.0, 19))
            hard = lights.hard_list()
            facing = lambda: api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
            trace = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_map)
            prev_eye = orbit(sc.eye, sc.target, -ORBIT_DEG)
            tp = api.TemporalParams.from_cameras((sc.eye, sc.target, sc.fovy), (prev_eye, sc.target, sc.fovy), W, H, 0.9, 0.005 * diag, 32)
            api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_ppos, d_pnrm)
            api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
            facing(), trace()
            api.accumulate_moments_soft_light_list_device(ctx, lights, tp, d_pos, d_nrm, d_counts, W, H, *d_mom[0], d_lights_map=d_map)
            api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
            facing(), trace()
            api.accumulate_moments_soft_light_list_device(ctx, lights, tp, d_pos, d_nrm, d_counts, W, H, *d_mom[1],
                                                          d_prev=(d_ppos, d_pnrm) + d_mom[0], d_lights_map=d_map)
            ctx.synchronize()
            for passes in PASSES:
                r = {"config": config, "mode": "this" if mode == "this" else "parent", "library": mode, "list": name, "steps": STEPS,
                     "warmup": WARMUP, "passes": passes, "guide_k4": k4, "min_history": min_history}
                if mode == "this":
                    for by_length, key in ((0, "filter_ms"), (1, "by_length_ms")):
                        pp = api.WideGuidePropagatedParams.make(passes, k4, min_history, by_length, 0.9, 0.05)
                        call = lambda: api.wide_filter_propagated_mean_soft_light_list_device(ctx, lights, pp, d_pos, d_nrm, d_counts, d_mom[1], W,
                                                                                              H, d_vis, d_scratch=d_scratch, d_lights_map=d_map)
                        r[key] = med(_timed(ctx, call, STEPS, WARMUP))
                else:
                    tg = api.WideGuideTemporalParams.make(passes, k4, min_history, 0.9, 0.05)
                    call = lambda: api.wide_filter_guided_temporal_mean_soft_light_list_device(ctx, lights, tg, d_pos, d_nrm, d_counts, d_mom[1], W,
                                                                                               H, d_vis, d_scratch=d_scratch, d_lights_map=d_map)
                    r["filter_ms"] = med(_timed(ctx, call, STEPS, WARMUP))
                print(json.dumps(r), flush=True)


def ratios(rows, config):
    out = []
    for name in LISTS:
        mine = [r for r in rows if r["config"] == config and r["list"] == name]
        pick = lambda mode, n: next((r["filter_ms"] for r in mine if r["mode"] == mode and r["passes"] == n), None)
        r = {"config": config, "mode": "ratio", "list": name}
        try:
            r["equal_passes"] = {f"passes{n}": round(pick("this", n) / pick("parent", n), 3) for n in PASSES}
            r["against_one_more_pass"] = {f"passes{n}": round(pick("this", n) / pick("parent", n + 1), 3) for n in PASSES[:-1]}
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
    ap.add_argument("--out", default="profiles/r36/list_propagated_ab.jsonl")
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
            runs = [("parent", os.path.abspath(args.parent_root)) if args.parent_root else ("this_library_guided_mean", ROOT), ("this", ROOT)]
            rows = []
            for mode, root in runs:
                env = dict(os.environ)
                env.pop("RTS_LIB", None)
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root, str(args.guide_k4),
                                      str(args.min_history)], env=env, capture_output=True, text=True, timeout=400)
                if run.returncode != 0:
                    sys.exit(f"list_propagated_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                for line in run.stdout.splitlines():
                    if line.startswith("{"):
                        rows.append(json.loads(line))
                        emit(line)
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
