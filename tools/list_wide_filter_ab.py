"""What the wide (a-trous) filter of a light list's planes costs (GPU box), per number of passes, against the parent commit's tent filter
at R = 2, 4 and 8 on the same frame, and per staging form.  DESIGN.md 4.25.

    python tools/list_wide_filter_ab.py --parent-root <tree of the parent commit, built> [--direct-lib <librts.so built with
                                        EXTRA=-DRTS_WIDE_FILTER_DENSE_MAX_STEP=0>] [--configs city_4k,courtyard_4k,atrium_1080p]
                                        [--out profiles/r29/list_wide_filter_ab.jsonl]

Rows: lists "4x4" = 4 lights of 4 samples and "2x16" = 2 lights of 16 (tools/soft_list_ab.py: entries), through the facing map;
passes 1 .. 5 of this commit's library ("this"), the same once more with the library whose every pass takes the DIRECT form ("direct":
the difference at passes <= 3 is the dense LDS window's gain or loss per step), and the PARENT commit's library running
rtsh_filter_soft_light_list_device without distances at R = 2, 4 and 8 and trace + list combine ("parent").  Each figure: 10 warm-up and
60 timed launches between device events, the median.  Every library runs in a child process of its own, under its own time limit;
this process never opens the GPU, and the tool stops at the first child that fails.  After the rows of a config: one "ratio" row per
list -- passes 3 (reach 14) against the parent's R = 8, passes 2 (reach 6) against R = 4, and the whole frame (trace + wide filter +
visibility combine) against the parent's trace + list combine.  No threshold: every row is reported."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
LISTS = {"4x4": (4, 4), "2x16": (2, 16)}
RADII = (2, 4, 8)
PASSES = (1, 2, 3, 4, 5)


def child(mode, config, root):
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
        d_counts, d_vis, d_rgb, d_scratch = ctx.malloc(4 * W * H), ctx.malloc(16 * W * H), ctx.malloc(3 * W * H), ctx.malloc(16 * W * H)
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
            if mode == "parent":
                combine = lambda: api.combine_soft_light_list_device(ctx, wl.constants, lights, d_pos, d_nrm, d_counts, W, H, d_rgb,
                                                                     d_lights_map=d_map, colors=colors)
                row["trace_ms"] = med(_timed(ctx, trace, STEPS, WARMUP))
                row["frame_ms"] = med(_timed(ctx, lambda: (trace(), combine()), STEPS, WARMUP))
                print(json.dumps(row), flush=True)
                for radius in RADII:
                    p = api.FilterParams.make(radius, 0.9, 0.05)
                    filt = lambda: api.filter_soft_light_list_device(ctx, lights, p, d_pos, d_nrm, d_counts, W, H, d_vis, d_lights_map=d_map)
                    r = dict(row, radius=radius)
                    r["filter_ms"] = med(_timed(ctx, filt, STEPS, WARMUP))
                    r["frame_ms"] = med(_timed(ctx, lambda: (trace(), filt(), vis()), STEPS, WARMUP))
                    print(json.dumps(r), flush=True)
                continue
            assert api.wide_filter_scratch_bytes(count, W, H) <= 16 * W * H
            for passes in PASSES:
                p = api.WideFilterParams.make(passes, 0.9, 0.05)
                filt = lambda: api.wide_filter_soft_light_list_device(ctx, lights, p, d_pos, d_nrm, d_counts, W, H, d_vis, d_scratch=d_scratch,
                                                                      d_lights_map=d_map)
                r = dict(row, passes=passes)
                r["filter_ms"] = med(_timed(ctx, filt, STEPS, WARMUP))
                if mode == "this":
                    r["frame_ms"] = med(_timed(ctx, lambda: (trace(), filt(), vis()), STEPS, WARMUP))
                print(json.dumps(r), flush=True)


def ratios(rows, config):
    out = []
    for name in LISTS:
        pick = lambda mode, **kw: next((r for r in rows if r["config"] == config and r["mode"] == mode and r["list"] == name and
                                        all(r.get(k) == v for k, v in kw.items())), None)
        this = {n: pick("this", passes=n) for n in PASSES}
        parent = {n: pick("parent", radius=n) for n in RADII}
        base = next((r for r in rows if r["config"] == config and r["mode"] == "parent" and r["list"] == name and "radius" not in r), None)
        if not (this[2] and this[3] and parent[4] and parent[8] and base):
            continue
        out.append({"config": config, "mode": "ratio", "list": name,
                    "passes3_over_parent_r8": this[3]["filter_ms"] / parent[8]["filter_ms"],
                    "passes2_over_parent_r4": this[2]["filter_ms"] / parent[4]["filter_ms"],
                    "frame_over_parent_frame": {f"passes{n}": this[n]["frame_ms"] / base["frame_ms"] for n in PASSES if this[n]}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--direct-lib", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r29/list_wide_filter_ab.jsonl")
    ap.add_argument("--child", nargs=3, metavar=("MODE", "CONFIG", "ROOT"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        def emit(line):
            out.write(line + "\n")
            out.flush()
            print(line, flush=True)
        for config in args.configs.split(","):
            runs = [("this", ROOT, None)]
            if args.parent_root:
                runs.insert(0, ("parent", os.path.abspath(args.parent_root), None))
            if args.direct_lib:
                runs.append(("direct", ROOT, os.path.abspath(args.direct_lib)))
            rows = []
            for mode, root, lib in runs:
                env = dict(os.environ)
                env.pop("RTS_LIB", None)
                if lib:
                    env["RTS_LIB"] = lib
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root], env=env, capture_output=True,
                                     text=True, timeout=400)
                if run.returncode != 0:
                    sys.exit(f"list_wide_filter_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                for line in run.stdout.splitlines():
                    if line.startswith("{"):
                        rows.append(json.loads(line))
                        emit(line)
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
