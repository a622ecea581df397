"""What an ambient occlusion trace costs (GPU box), against the PARENT commit's library tracing the same rays as generic rays.
DESIGN.md 4.34.

    python tools/ao_ab.py --parent-root <tree of the parent commit, built>
                          [--configs city_4k,courtyard_4k,atrium_1080p] [--no-rays-on city_4k,courtyard_4k]
                          [--out profiles/r39/ao_ab.jsonl]

Rows: per config, n = 4 and 16 samples, a radius of 2 % and 20 % of the scene's diagonal, table 0 and 64 (AoParams.make, seed 5).
  "parent": the parent commit's library --
            rays_ms (a): rts_trace_rays_device over the n * W * H records of rtsh_ao_rays (made on the host by THIS tree's library,
            loaded beside the parent's for that host function alone, from the G-buffer the parent's pass wrote).  Building the rays,
            uploading 32 bytes per ray and summing the bytes are NOT timed, which favours the baseline;
            soft_mask_ms (e): for scale, the parent's soft mask trace of n samples of a point light (the scene's light, jittered by
            1 % of the diagonal), its default family.
  "this":   ao_ms (b): rts_trace_ambient_occlusion_device, the family blockFamily picks ("kernel" -1);  other_family_ms (c): the other
            family forced ("kernel" 7 where (b) ran the packet, 3 where it ran the lane walk);  split0_ms (d): the packet family with
            "soft_split" 0;  kernel: the name of (b)'s kernel;  mismatches: count bytes of (c) and (d) that differ from (b)'s (must be 0).
Each figure: 10 warm-up and 60 timed launches between device events, the median, ONE run of the tool.  Every library runs in a child
process of its own, under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.
After the rows of a config: one "ratio" row per case, (b) over (a), with ao_not_below_rays and other_family_beats_choice.  No
threshold: every row is reported.
--no-rays-on CONFIGS: leave column (a) out on these configs (rays_ms and what follows from it are null in their rows): for frames
with sky, whose all-zero records of rtsh_ao_rays walk the whole tree as generic rays."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
CASES = [(n, share, table) for n in (4, 16) for share in (0.02, 0.20) for table in (0, 64)]


def child(mode, config, root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, scenes, workloads
    from soft_list_ab import _timed
    print(f"ao_ab: {mode} on {config}: preparing the scene", file=sys.stderr, flush=True)
    wl = workloads.prepare_config(config, cache=True)
    W, H, px = wl.W, wl.H, wl.W * wl.H
    sc = wl.scene
    med = lambda ts: float(np.median(ts))
    diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
    if mode == "parent":                                 # this tree's AoParams and rtsh_ao_rays: host code only
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import importlib.util
        spec = importlib.util.spec_from_file_location("ao_api", os.path.join(ROOT, "raytracedshadows_amd", "api.py"))
        os.environ["RTS_LIB"] = os.path.join(ROOT, "raytracedshadows_amd", "librts.so")
        ao_api = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ao_api)
        os.environ.pop("RTS_LIB")
    else:
        ao_api = api
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_counts = ctx.malloc(px * 16), ctx.malloc(px * 16), ctx.malloc(px)
        api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
        ctx.synchronize()
        if mode == "parent":
            pos, nrm = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
            ctx.d2h(pos, d_pos)
            ctx.d2h(nrm, d_nrm)
            k = ao_api.RayTracingConstants.make(list(wl.constants.cameraPosition)[:3], list(wl.constants.lightDirection)[:3], W, H)
        for n, share, table in CASES:
            row = {"config": config, "mode": mode, "n": n, "radius_share": share, "table": table, "steps": STEPS, "warmup": WARMUP, "runs": 1,
                   "W": W, "H": H}
            ao = ao_api.AoParams.make(n, diag * share, table=table, seed=5)
            print(f"ao_ab: {mode} on {config}: n {n}, radius {share:g} of the diagonal, table {table}", file=sys.stderr, flush=True)
            if mode == "parent" and os.environ.get("AO_AB_NO_RAYS") == "1":
                row["rays_ms"] = None
            elif mode == "parent":
                rays = ao_api.ao_rays(k, ao, pos, nrm, W, H)
                d_rays, d_out = ctx.malloc(rays.nbytes), ctx.malloc(rays.shape[0])
                ctx.h2d(d_rays, rays)
                row["rays"] = int(rays.shape[0])
                row["rays_ms"] = med(_timed(ctx, lambda: ctx.trace_rays_device(d_rays, rays.shape[0], d_out), STEPS, WARMUP))
                row["rays_kernel"] = ctx.last_kernel_name()
                ctx.free(d_rays)
                ctx.free(d_out)
                del rays
            if mode == "parent":
                light = api.Light.make(api.Light.POINT, sc.light_point, scenes.jitter_offsets(n, 0.01 * diag, 1))
                row["soft_mask_ms"] = med(_timed(ctx, lambda: ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_counts, light=light),
                                                 STEPS, WARMUP))
                row["soft_mask_kernel"] = ctx.last_kernel_name()
            else:
                trace = lambda: ctx.trace_ambient_occlusion_device(wl.constants, ao, d_pos, d_nrm, W, H, d_counts)
                planes = []

                def run(key, kernel, split):
                    ctx.set_option("kernel", kernel)
                    ctx.set_option("soft_split", split)
                    row[key] = med(_timed(ctx, trace, STEPS, WARMUP))
                    out = np.zeros(px, np.uint8)
                    ctx.d2h(out, d_counts)
                    planes.append(out)
                    return ctx.last_kernel_name()

                row["kernel"] = run("ao_ms", -1, 1)
                packet = "Packet" in row["kernel"]
                row["other_family_kernel"] = run("other_family_ms", 7 if packet else 3, 1)
                row["split0_kernel"] = run("split0_ms", 3, 0)
                ctx.set_option("kernel", -1)
                ctx.set_option("soft_split", 1)
                row["mismatches"] = int((planes[1] != planes[0]).sum() + (planes[2] != planes[0]).sum())
                row["mean_openness"] = float(planes[0].mean()) / n
            print(json.dumps(row), flush=True)


def ratios(rows, config):
    out = []
    for n, share, table in CASES:
        pick = lambda mode: next((r for r in rows if r["mode"] == mode and (r["n"], r["radius_share"], r["table"]) == (n, share, table)), None)
        a, b = pick("parent"), pick("this")
        if a is None or b is None:
            continue
        out.append({"config": config, "mode": "ratio", "n": n, "radius_share": share, "table": table, "rays_ms": a["rays_ms"],
                    "ao_ms": b["ao_ms"], "other_family_ms": b["other_family_ms"], "split0_ms": b["split0_ms"], "soft_mask_ms": a["soft_mask_ms"],
                    "ao_over_rays": b["ao_ms"] / a["rays_ms"] if a["rays_ms"] else None,
                    "ao_not_below_rays": b["ao_ms"] >= a["rays_ms"] if a["rays_ms"] else None,
                    "other_family_beats_choice": b["other_family_ms"] < b["ao_ms"], "mismatches": b["mismatches"], "runs": 1})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--no-rays-on", default="")
    ap.add_argument("--out", default="profiles/r39/ao_ab.jsonl")
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
                env["AO_AB_NO_RAYS"] = "1" if config in args.no_rays_on.split(",") else "0"
                # (the child's rows are passed on as they come: a 4K case of 16 samples spends tens of seconds building its rays)
                run = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", mode, config, root], env=env,
                                       stdout=subprocess.PIPE, text=True)
                timer = threading.Timer(600, run.kill)
                timer.start()
                try:
                    for line in run.stdout:
                        if line.startswith("{"):
                            rows.append(json.loads(line))
                            emit(line.rstrip("\n"))
                    run.wait()
                finally:
                    timer.cancel()
                if run.returncode != 0:
                    sys.exit(f"ao_ab: {mode} on {config} failed or ran out of its time limit ({run.returncode})")
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
