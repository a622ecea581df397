"""What the variance guide of the wide (a-trous) filter costs (GPU box), per number of passes, against the PARENT commit's library
running the unguided wide filter on the same frame.  DESIGN.md 4.26.

    python tools/list_wide_guided_ab.py --parent-root <tree of the parent commit, built> [--guide-k4 12]
                                        [--configs city_4k,courtyard_4k,atrium_1080p] [--out profiles/r30/list_wide_guided_ab.jsonl]

Rows: lists "4x4" = 4 lights of 4 samples and "2x16" = 2 lights of 16 (tools/soft_list_ab.py: entries), through the facing map;
passes 1 .. 5.  "parent": the parent commit's rtsh_wide_filter_soft_light_list_device; "this": this commit's
rtsh_wide_filter_guided_soft_light_list_device at --guide-k4.  filter_ms is the filter alone, frame_ms trace + filter + visibility
combine.  Each figure: 10 warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of
its own, under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.  After the
rows of a config: one "ratio" row per list -- guided over unguided at equal passes, filter and frame, and whether the guided filter at
p passes costs more than the parent's unguided filter at p + 1 (the guide then costs more than one extra pass would).  No threshold:
every row is reported."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
LISTS = {"4x4": (4, 4), "2x16": (2, 16)}
PASSES = (1, 2, 3, 4, 5)


def child(mode, config, root, k4):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, scenes, workloads
    from soft_list_ab import _timed, entries
    wl = workloads.prepare_config(config, cache=True)
    W, H = wl.W, wl.H
    med = lambda ts: float(np.median(ts))
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_map = ctx.malloc(W * H * 16), ctx.malloc(W * H * 16), ctx.malloc(W * H)
        d_counts, d_vis, d_rgb, d_scratch = ctx.malloc(4 * W * H), ctx.malloc(16 * W * H), ctx.malloc(3 * W * H), ctx.malloc(24 * W * H)
        api.primary_gbuffer_device(ctx, wl.scene.eye, wl.scene.target, wl.scene.fovy, W, H, d_pos, d_nrm)
        for name, (count, spp) in LISTS.items():
            lights = api.SoftLightList.make(entries(wl.scene, count, spp), scenes.jitter_offsets(48, 1.0, 19))
            hard = lights.hard_list()
            api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
            colors = np.full((count, 3), 1.0 / count, np.float32)
            trace = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_map)
            vis = lambda: api.combine_visibility_list_device(ctx, wl.constants, hard, d_pos, d_nrm, d_vis, W, H, d_rgb, d_lights_map=d_map,
                                                             colors=colors)
            row = {"config": config, "mode": mode, "list": name, "steps": STEPS, "warmup": WARMUP}
            trace()
            ctx.synchronize()
            for passes in PASSES:
                if mode == "parent":
                    p = api.WideFilterParams.make(passes, 0.9, 0.05)
                    filt = lambda: api.wide_filter_soft_light_list_device(ctx, lights, p, d_pos, d_nrm, d_counts, W, H, d_vis,
                                                                          d_scratch=d_scratch, d_lights_map=d_map)
                    r = dict(row, passes=passes)
                else:
                    assert api.wide_filter_guided_scratch_bytes(count, W, H) <= 24 * W * H
                    p = api.WideGuideParams.make(passes, k4, 0.9, 0.05)
                    filt = lambda: api.wide_filter_guided_soft_light_list_device(ctx, lights, p, d_pos, d_nrm, d_counts, W, H, d_vis,
                                                                                 d_scratch=d_scratch, d_lights_map=d_map)
                    r = dict(row, passes=passes, guide_k4=k4)
                r["filter_ms"] = med(_timed(ctx, filt, STEPS, WARMUP))
                r["frame_ms"] = med(_timed(ctx, lambda: (trace(), filt(), vis()), STEPS, WARMUP))
                print(json.dumps(r), flush=True)


def ratios(rows, config):
    out = []
    for name in LISTS:
        pick = lambda mode, n: next((r for r in rows if r["config"] == config and r["mode"] == mode and r["list"] == name and
                                     r["passes"] == n), None)
        this, parent = {n: pick("this", n) for n in PASSES}, {n: pick("parent", n) for n in PASSES}
        if not all(this.values()) or not all(parent.values()):
            continue
        out.append({"config": config, "mode": "ratio", "list": name,
                    "guided_over_unguided_filter": {f"passes{n}": this[n]["filter_ms"] / parent[n]["filter_ms"] for n in PASSES},
                    "guided_over_unguided_frame": {f"passes{n}": this[n]["frame_ms"] / parent[n]["frame_ms"] for n in PASSES},
                    "guided_over_unguided_one_more_pass": {f"passes{n}": this[n]["filter_ms"] / parent[n + 1]["filter_ms"]
                                                           for n in PASSES if n + 1 in parent}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--guide-k4", type=int, default=12)
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r30/list_wide_guided_ab.jsonl")
    ap.add_argument("--child", nargs=4, metavar=("MODE", "CONFIG", "ROOT", "K4"))
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], args.child[1], args.child[2], int(args.child[3]))
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
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root, str(args.guide_k4)], env=env,
                                     capture_output=True, text=True, timeout=400)
                if run.returncode != 0:
                    sys.exit(f"list_wide_guided_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                for line in run.stdout.splitlines():
                    if line.startswith("{"):
                        rows.append(json.loads(line))
                        emit(line)
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
