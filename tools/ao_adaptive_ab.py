"""What an adaptive ambient occlusion trace costs (GPU box), against the PARENT commit's full AO trace.  DESIGN.md 4.35.

    python tools/ao_adaptive_ab.py --parent-root <tree of the parent commit, built>
                                   [--configs city_4k,courtyard_4k,atrium_1080p] [--out profiles/r43/ao_adaptive_ab.jsonl]

Rows: tools/ao_ab.py's -- per config, n = 4 and 16 samples, a radius of 2 % and 20 % of the scene's diagonal, table 0 and 64
(AoParams.make, seed 5) -- with probe 1 and 2 for n = 4 and probe 2 and 4 for n = 16.
  "parent": the parent commit's library, rts_trace_ambient_occlusion_device in the family blockFamily picks ("kernel" -1): ao_ms.
  "this":   adaptive_ms: rts_trace_ambient_occlusion_adaptive_device, "kernel" -1;  split0_ms: the packet family with "soft_split" 0;
            other_family_ms: the other family forced ("kernel" 7 where the choice ran the packet, 3 where it ran the lane walk);
            refined_share: the share of the frame's pixels that took their full count;  mismatches: bytes of counts or refined of
            the two other launches that differ from the first one's (must be 0).
Each figure: 10 warm-up and 60 timed launches between device events, the median, ONE run of the tool.  Every library runs in a child
process of its own, under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.
After the rows of a config: one "ratio" row per (case, probe), adaptive_ms over the parent's ao_ms, with adaptive_not_below_parent.
No threshold: every row is reported."""
import argparse
import json
import os
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
CASES = [(n, share, table) for n in (4, 16) for share in (0.02, 0.20) for table in (0, 64)]
PROBES = {4: (1, 2), 16: (2, 4)}


def child(mode, config, root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, workloads
    from soft_list_ab import _timed
    print(f"ao_adaptive_ab: {mode} on {config}: preparing the scene", file=sys.stderr, flush=True)
    wl = workloads.prepare_config(config, cache=True)
    W, H, px = wl.W, wl.H, wl.W * wl.H
    sc = wl.scene
    med = lambda ts: float(np.median(ts))
    diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_counts, d_ref = ctx.malloc(px * 16), ctx.malloc(px * 16), ctx.malloc(px), ctx.malloc(px)
        api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
        ctx.synchronize()
        for n, share, table in CASES:
            ao = api.AoParams.make(n, diag * share, table=table, seed=5)
            base = {"config": config, "mode": mode, "n": n, "radius_share": share, "table": table, "steps": STEPS, "warmup": WARMUP, "runs": 1,
                    "W": W, "H": H}
            print(f"ao_adaptive_ab: {mode} on {config}: n {n}, radius {share:g} of the diagonal, table {table}", file=sys.stderr, flush=True)
            if mode == "parent":
                row = dict(base)
                row["ao_ms"] = med(_timed(ctx, lambda: ctx.trace_ambient_occlusion_device(wl.constants, ao, d_pos, d_nrm, W, H, d_counts),
                                          STEPS, WARMUP))
                row["kernel"] = ctx.last_kernel_name()
                print(json.dumps(row), flush=True)
                continue
            for probe in PROBES[n]:
                row = dict(base, probe=probe)
                trace = lambda: ctx.trace_ambient_occlusion_adaptive_device(wl.constants, ao, d_pos, d_nrm, W, H, d_counts, probe, d_refined=d_ref)
                planes = []

                def run(key, kernel, split):
                    ctx.set_option("kernel", kernel)
                    ctx.set_option("soft_split", split)
                    row[key] = med(_timed(ctx, trace, STEPS, WARMUP))
                    out = np.zeros(2 * px, np.uint8)
                    ctx.d2h(out[:px], d_counts)
                    ctx.d2h(out[px:], d_ref)
                    planes.append(out)
                    return ctx.last_kernel_name()

                row["kernel"] = run("adaptive_ms", -1, 1)
                row["split0_kernel"] = run("split0_ms", 3, 0)
                row["other_family_kernel"] = run("other_family_ms", 7 if "Packet" in row["kernel"] else 3, 1)
                ctx.set_option("kernel", -1)
                ctx.set_option("soft_split", 1)
                row["mismatches"] = int((planes[1] != planes[0]).sum() + (planes[2] != planes[0]).sum())
                row["refined_share"] = float(planes[0][px:].mean())
                print(json.dumps(row), flush=True)


def ratios(rows, config):
    out = []
    for n, share, table in CASES:
        same = lambda r: (r["n"], r["radius_share"], r["table"]) == (n, share, table)
        a = next((r for r in rows if r["mode"] == "parent" and same(r)), None)
        for b in (r for r in rows if r["mode"] == "this" and same(r)):
            if a is None:
                continue
            out.append({"config": config, "mode": "ratio", "n": n, "probe": b["probe"], "radius_share": share, "table": table,
                        "parent_ao_ms": a["ao_ms"], "adaptive_ms": b["adaptive_ms"], "split0_ms": b["split0_ms"],
                        "other_family_ms": b["other_family_ms"], "refined_share": b["refined_share"],
                        "adaptive_over_parent": b["adaptive_ms"] / a["ao_ms"], "adaptive_not_below_parent": b["adaptive_ms"] >= a["ao_ms"],
                        "mismatches": b["mismatches"], "runs": 1})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r43/ao_adaptive_ab.jsonl")
    ap.add_argument("--limit", type=int, default=600, help="seconds a child may run")
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
                run = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", mode, config, root], env=env,
                                       stdout=subprocess.PIPE, text=True)
                timer = threading.Timer(args.limit, run.kill)
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
                    sys.exit(f"ao_adaptive_ab: {mode} on {config} failed or ran out of its time limit ({run.returncode})")
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
