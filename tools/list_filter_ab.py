"""What the filter of a light list's planes costs (GPU box): the filter alone and the whole frame -- trace + filter + visibility combine
-- against the parent commit's library running trace + rtsh_combine_soft_light_list_device on the same frame.  DESIGN.md 4.22.

    python tools/list_filter_ab.py --parent-root <tree of the parent commit, built> [--noshortcut-lib <librts.so built with
                                   EXTRA=-DRTS_FILTER_NO_SHORTCUT>] [--configs city_4k,courtyard_4k,atrium_1080p]
                                   [--out profiles/r25/list_filter_ab.jsonl]

Lists: "4x4" = 4 lights of 4 samples, "2x16" = 2 lights of 16 (tools/soft_list_ab.py: entries), through the facing map.  Radii 2, 4 and
8; every row with and without the distance planes (then the trace is the distance trace, on both sides of the comparison the one that
feeds the pass); every row of this commit once more with the library built without the block-uniform shortcut.  Each figure: 10
warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of its own, under its own time
limit; this process never opens the GPU, and the tool stops at the first child that fails.  No threshold: every row is reported."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
LISTS = {"4x4": (4, 4), "2x16": (2, 16)}
RADII = (2, 4, 8)


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
        d_counts, d_dist, d_vis, d_rgb = ctx.malloc(4 * W * H), ctx.malloc(16 * W * H), ctx.malloc(16 * W * H), ctx.malloc(3 * W * H)
        api.primary_gbuffer_device(ctx, wl.scene.eye, wl.scene.target, wl.scene.fovy, W, H, d_pos, d_nrm)
        for name, (count, spp) in LISTS.items():
            lights = api.SoftLightList.make(entries(wl.scene, count, spp), scenes.jitter_offsets(48, 1.0, 19))
            hard = lights.hard_list()
            api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
            colors = np.full((count, 3), 1.0 / count, np.float32)
            for with_dist in (False, True):
                if with_dist:
                    trace = lambda: ctx.trace_soft_light_list_distance_device(wl.constants, lights, d_pos, W, H, d_dist, d_counts, d_lights_map=d_map)
                else:
                    trace = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_map)
                combine = lambda: api.combine_soft_light_list_device(ctx, wl.constants, lights, d_pos, d_nrm, d_counts, W, H, d_rgb,
                                                                     d_lights_map=d_map, colors=colors)
                row = {"config": config, "mode": mode, "list": name, "distances": with_dist, "steps": STEPS, "warmup": WARMUP}
                trace()
                ctx.synchronize()
                if mode == "parent":
                    row["trace_ms"] = med(_timed(ctx, trace, STEPS, WARMUP))
                    row["frame_ms"] = med(_timed(ctx, lambda: (trace(), combine()), STEPS, WARMUP))
                    print(json.dumps(row), flush=True)
                    continue
                planes = np.zeros((count, H, W), np.uint8)
                ctx.d2h(planes, d_counts)
                row["uniform_share"] = float(np.mean([(planes[l] == planes[l, 0, 0]).mean() for l in range(count)]))
                for radius in RADII:
                    p = api.FilterParams.make(radius, 0.9, 0.05, 0.25)
                    filt = lambda: api.filter_soft_light_list_device(ctx, lights, p, d_pos, d_nrm, d_counts, W, H, d_vis, d_lights_map=d_map,
                                                                     d_distances=d_dist if with_dist else None)
                    vis = lambda: api.combine_visibility_list_device(ctx, wl.constants, hard, d_pos, d_nrm, d_vis, W, H, d_rgb,
                                                                     d_lights_map=d_map, colors=colors)
                    r = dict(row, radius=radius)
                    r["filter_ms"] = med(_timed(ctx, filt, STEPS, WARMUP))
                    r["frame_ms"] = med(_timed(ctx, lambda: (trace(), filt(), vis()), STEPS, WARMUP))
                    print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--noshortcut-lib", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r25/list_filter_ab.jsonl")
    ap.add_argument("--child", nargs=3, metavar=("MODE", "CONFIG", "ROOT"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for config in args.configs.split(","):
            runs = [("this", ROOT, None)]
            if args.parent_root:
                runs.insert(0, ("parent", os.path.abspath(args.parent_root), None))
            if args.noshortcut_lib:
                runs.append(("noshortcut", ROOT, os.path.abspath(args.noshortcut_lib)))
            for mode, root, lib in runs:
                env = dict(os.environ)
                env.pop("RTS_LIB", None)
                if lib:
                    env["RTS_LIB"] = lib
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root], env=env, capture_output=True,
                                     text=True, timeout=400)
                if run.returncode != 0:
                    sys.exit(f"list_filter_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                for line in run.stdout.splitlines():
                    if line.startswith("{"):
                        out.write(line + "\n")
                        out.flush()
                        print(line)


if __name__ == "__main__":
    main()
