"""What the motion G-buffer pass and the motion forms of the three temporal passes cost (GPU box), against the PARENT commit's library on
the same frames.  DESIGN.md 4.29.

    python tools/list_motion_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,courtyard_4k,atrium_1080p]
                                   [--out profiles/r33/list_motion_ab.jsonl]

Rows: the six of 4.23's table -- three configs, lists "4x4" = 4 lights of 4 samples and "2x16" = 2 lights of 16 (tools/soft_list_ab.py:
entries), through the facing map --, each for two frames: "static" (the previous stream is a snapshot of the installed one: every hit
STATIC) and "moved" (after the snapshot the vertices of the middle third of the scene's x extent are lifted by 1 % of the diagonal (twice plane_eps) and
the stream is refitted on the device: those hits are MOVED).  The camera orbits by 0.5 degree per frame in both (up to four taps).
  "parent": rtsh_primary_gbuffer_device, rtsh_accumulate_visibility_list_device, its clamped form (radius 2) and
            rtsh_accumulate_moments_soft_light_list_device, over the same refitted stream.
  "this":   rtsh_primary_gbuffer_motion_device and the three _motion_device forms; snapshot_ms: rtsh_ctx_snapshot_bvh_device.
Each figure: 10 warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of its own,
under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.  After the rows of a
config: one "ratio" row per list and frame, this / parent.  No threshold: every row is reported."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
LISTS = {"4x4": (4, 4), "2x16": (2, 16)}
ORBIT_DEG = 0.5
PASSES = ("gbuffer_ms", "accumulate_ms", "clamped_ms", "moments_ms")


def child(mode, config, root):
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
    motion = mode == "this"
    diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
    verts = np.array(wl.vertices, np.float32).reshape(-1, 8)
    lo, hi = float(sc.bbox_min[0]), float(sc.bbox_max[0])
    lifted = verts.copy()
    lifted[(verts[:, 0] > lo + (hi - lo) / 3) & (verts[:, 0] < lo + 2 * (hi - lo) / 3), 1] += np.float32(0.01 * diag)
    prev_eye = orbit(sc.eye, sc.target, -ORBIT_DEG)
    tp = api.TemporalParams.from_cameras((sc.eye, sc.target, sc.fovy), (prev_eye, sc.target, sc.fovy), W, H, 0.9, 0.005 * diag, 32)
    clamp = api.HistoryClamp.make(2, 0.0)
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        count_vec4 = int(np.asarray(wl.packed).reshape(-1, 4).shape[0])
        d_pos, d_nrm, d_ppos, d_pnrm, d_map = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n)
        d_pts, d_pnr = ctx.malloc(n * 16), ctx.malloc(n * 16)
        d_counts, d_vis = ctx.malloc(4 * n), ctx.malloc(16 * n)
        d_hist, d_len = [ctx.malloc(16 * n) for _ in range(3)], [ctx.malloc(4 * n) for _ in range(3)]
        d_mom = [(ctx.malloc(8 * n), ctx.malloc(16 * n), ctx.malloc(4 * n)) for _ in range(2)]
        d_snap = ctx.malloc(count_vec4 * 16) if motion else 0
        for frame in ("static", "moved"):
            for name, (count, spp) in LISTS.items():
                lights = api.SoftLightList.make(entries(sc, count, spp), scenes.jitter_offsets(48, 1.0, 19))
                hard = lights.hard_list()
                facing = lambda: api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
                trace = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_map)
                convert = lambda: api.wide_filter_soft_light_list_device(ctx, lights, api.WideFilterParams.make(0, 0.9, 0.05), d_pos, d_nrm, d_counts,
                                                                         W, H, d_vis, d_lights_map=d_map)
                # the previous frame: the original geometry from the previous eye, accumulated as a first frame into set 0
                api.bvh_refit_device(ctx, verts.reshape(-1), 8, wl.indices, wl.prim_count)
                api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
                facing(), trace(), convert()
                api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_hist[0], d_len[0], d_lights_map=d_map)
                api.accumulate_moments_soft_light_list_device(ctx, lights, tp, d_pos, d_nrm, d_counts, W, H, *d_mom[0], d_lights_map=d_map)
                api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_ppos, d_pnrm)
                row = {"config": config, "mode": mode, "list": name, "frame": frame, "steps": STEPS, "warmup": WARMUP}
                if motion:
                    snap = lambda: api.snapshot_bvh_device(ctx, d_snap, count_vec4)
                    row["snapshot_ms"] = med(_timed(ctx, snap, STEPS, WARMUP))
                if frame == "moved":
                    api.bvh_refit_device(ctx, lifted.reshape(-1), 8, wl.indices, wl.prim_count)
                if motion:
                    gbuffer = lambda: api.primary_gbuffer_motion_device(ctx, d_snap, count_vec4, sc.eye, prev_eye, sc.target, sc.fovy, W, H, d_pos,
                                                                        d_nrm, d_pts, d_pnr)
                    extra = dict(d_motion=(d_pts, d_pnr))
                else:
                    gbuffer = lambda: api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
                    extra = {}
                gbuffer(), facing(), trace(), convert()
                ctx.synchronize()
                prev = (d_ppos, d_pnrm, d_hist[0], d_len[0])
                acc = lambda: api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_hist[1], d_len[1], d_prev=prev,
                                                                    d_lights_map=d_map, **extra)
                clamped = lambda: api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_hist[2], d_len[2], d_prev=prev,
                                                                        d_lights_map=d_map, clamp=clamp, **extra)
                mom = lambda: api.accumulate_moments_soft_light_list_device(ctx, lights, tp, d_pos, d_nrm, d_counts, W, H, *d_mom[1],
                                                                            d_prev=(d_ppos, d_pnrm) + d_mom[0], d_lights_map=d_map, **extra)
                for key, launch in zip(PASSES, (gbuffer, acc, clamped, mom)):
                    row[key] = med(_timed(ctx, launch, STEPS, WARMUP))
                if motion:
                    pts = np.zeros((H, W, 4), np.float32)
                    ctx.d2h(pts, d_pts)
                    row["moved_pixels"], row["hit_pixels"] = int((pts[..., 3] == 2).sum()), int((pts[..., 3] != 0).sum())
                print(json.dumps(row), flush=True)


def ratios(rows, config):
    out = []
    for name in LISTS:
        for frame in ("static", "moved"):
            pick = {r["mode"]: r for r in rows if r["config"] == config and r["list"] == name and r["frame"] == frame}
            if "this" in pick and "parent" in pick:
                out.append(dict({"config": config, "mode": "ratio", "list": name, "frame": frame},
                                **{k[:-3]: round(pick["this"][k] / pick["parent"][k], 3) for k in PASSES}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r33/list_motion_ab.jsonl")
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
            runs = [("this", ROOT)]
            if args.parent_root:
                runs.insert(0, ("parent", os.path.abspath(args.parent_root)))
            rows = []
            for mode, root in runs:
                env = dict(os.environ)
                env.pop("RTS_LIB", None)
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root], env=env, capture_output=True,
                                     text=True, timeout=400)
                if run.returncode != 0:
                    sys.exit(f"list_motion_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                for line in run.stdout.splitlines():
                    if line.startswith("{"):
                        rows.append(json.loads(line))
                        emit(line)
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
