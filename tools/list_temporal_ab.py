"""What the temporal accumulation of a light list's visibility costs (GPU box): the pass alone for a still camera and for an orbit of
0.5 degree per frame, the pass against a device-to-device copy of the bytes it must move, and the whole frame -- trace + filter +
accumulate + visibility combine -- against the parent commit's library running trace + filter + visibility combine.  DESIGN.md 4.23.

    python tools/list_temporal_ab.py [--parent-root <tree of the parent commit, built>] [--variant-lib NAME=<librts.so of another build>]
                                     [--configs city_4k,courtyard_4k,atrium_1080p] [--out profiles/r26/list_temporal_ab.jsonl]

Lists: "4x4" = 4 lights of 4 samples, "2x16" = 2 lights of 16 (tools/soft_list_ab.py: entries), through the facing map; the filter at
R = 2.  Each figure: 10 warm-up and 60 timed launches between device events, the median.  The copy floor: one hipMemcpyAsync, device to
device, of `floor_bytes` on the same stream, timed the same way in the same process.  floor_bytes is NOMINAL, every tap that can carry weight counted as
accepted: per pixel with a surface 32 for its texel and 32 per tap for the previous frame's; per light facing it 4 of visibility, 4 + 1
per tap of history and length, 5 of output; a background pixel 16 (its normal) and every other (pixel, light) 5 of output.  Taps per
pixel: 1 for the still camera, 4 for the orbit.  Every library runs in a child process of its own, under its own time limit; this
process never opens the GPU, and the tool stops at the first child that fails.  No threshold: every row is reported."""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
LISTS = {"4x4": (4, 4), "2x16": (2, 16)}
RADIUS, ORBIT_DEG = 2, 0.5


def _loaded_runtime():
    """The libamdhip64 this process has mapped (the one librts.so is linked against), not whichever a search path finds."""
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split()[-1]
            if "libamdhip64.so" in path and path.startswith("/"):
                return path
    return "libamdhip64.so"


def orbit(eye, target, degrees):
    """The eye turned around the target's vertical axis by `degrees`."""
    a = math.radians(degrees)
    dx, dz = eye[0] - target[0], eye[2] - target[2]
    return (target[0] + dx * math.cos(a) - dz * math.sin(a), eye[1], target[2] + dx * math.sin(a) + dz * math.cos(a))


def child(mode, config, root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, scenes, workloads
    from soft_list_ab import _timed, entries
    wl = workloads.prepare_config(config, cache=True)
    W, H, n = wl.W, wl.H, wl.W * wl.H
    med = lambda ts: float(np.median(ts))
    sc = wl.scene
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        hip = C.CDLL(_loaded_runtime())
        d_pos, d_nrm, d_map = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n)
        d_counts, d_vis, d_rgb = ctx.malloc(4 * n), ctx.malloc(16 * n), ctx.malloc(3 * n)
        api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
        if mode != "parent":
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
            row = {"config": config, "mode": mode, "list": name, "radius": RADIUS, "steps": STEPS, "warmup": WARMUP}
            facing()
            trace()
            ctx.synchronize()
            if mode == "parent":
                row["frame_ms"] = med(_timed(ctx, lambda: (trace(), filt(), vis(d_vis)), STEPS, WARMUP))
                print(json.dumps(row), flush=True)
                continue
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
                acc = lambda: api.accumulate_visibility_list_device(ctx, hard, tp, d_pos, d_nrm, d_vis, W, H, d_hist[1], d_len[1],
                                                                    d_prev=(d_ppos, d_pnrm, d_hist[0], d_len[0]), d_lights_map=d_map)
                r = dict(row, motion=motion)
                r["accumulate_ms"] = med(_timed(ctx, acc, STEPS, WARMUP))
                lengths, fmap, nrm = np.zeros((count, H, W), np.uint8), np.zeros((H, W), np.uint8), np.zeros((H, W, 4), np.float32)
                ctx.d2h(lengths, d_len[1]), ctx.d2h(fmap, d_map), ctx.d2h(nrm, d_nrm)
                solid = (nrm[..., :3] != 0).any(axis=-1)
                lit = int(sum((solid & (((fmap >> l) & 1) != 0)).sum() for l in range(count)))
                taps = 1 if motion == "still" else 4
                r["surface_share"], r["history_share"] = float(solid.mean()), float((lengths > 1).sum() / max(1, lit))
                r["floor_bytes"] = int(solid.sum()) * (32 + 32 * taps) + int((~solid).sum()) * 16 + lit * (4 + 5 * taps) + count * n * 5
                if motion == "still":
                    r["frame_ms"] = med(_timed(ctx, lambda: (trace(), filt(), acc(), vis(d_hist[1])), STEPS, WARMUP))
                d_a, d_b = ctx.malloc(r["floor_bytes"]), ctx.malloc(r["floor_bytes"])
                copy = lambda: hip.hipMemcpyAsync(C.c_void_p(d_b), C.c_void_p(d_a), C.c_size_t(r["floor_bytes"]), 3, None)   # device to device
                assert copy() == 0
                r["copy_ms"] = med(_timed(ctx, copy, STEPS, WARMUP))
                ctx.free(d_a), ctx.free(d_b)
                print(json.dumps(r), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--variant-lib", default="", help="NAME=path: every row of this commit once more with that build of the library")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r26/list_temporal_ab.jsonl")
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
            if args.variant_lib:
                name, lib = args.variant_lib.split("=", 1)
                runs.append((name, ROOT, os.path.abspath(lib)))
            for mode, root, lib in runs:
                env = dict(os.environ)
                env.pop("RTS_LIB", None)
                if lib:
                    env["RTS_LIB"] = lib
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root], env=env, capture_output=True,
                                     text=True, timeout=400)
                if run.returncode != 0:
                    sys.exit(f"list_temporal_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                for line in run.stdout.splitlines():
                    if line.startswith("{"):
                        out.write(line + "\n")
                        out.flush()
                        print(line)


if __name__ == "__main__":
    main()
