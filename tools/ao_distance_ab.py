"""What an AO distance trace costs (GPU box), against the PARENT commit's AO trace over the same rays.  DESIGN.md 4.37.

    python tools/ao_distance_ab.py --parent-root <tree of the parent commit, built>
                                   [--configs atrium_1080p,city_4k,courtyard_4k] [--out profiles/r45/ao_distance_ab.jsonl]

Rows: tools/ao_ab.py's -- per config, n = 4 and 16 samples, a radius of 2 % and 20 % of the scene's diagonal, table 0 and 64
(AoParams.make, seed 5).
  "parent":  the parent commit's library, rts_trace_ambient_occlusion_device in the family blockFamily picks ("kernel" -1): ao_ms.  The
             parent runs TWICE per config, before and after this commit's library ("parent" and "parent_again"): the spread of its two
             medians is the row's noise figure.
  "this":    rts_trace_ambient_occlusion_distance_device, "kernel" -1, the linear falloff, in three variants -- distance_ms: counts +
             distance;  obscurance_ms: counts + obscurance;  all_ms: all three planes --, and mismatches: bytes of counts of the other
             two launches that differ from the first one's (must be 0).
Each figure: 10 warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of its own,
under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.
After the rows of a config: one "ratio" row per case -- the three figures over the mean of the parent's two medians, the noise figure,
and `above_noise` per variant where it exceeds that mean by more than the noise; `--markdown` prints the table for DESIGN.md with those
cells in bold.  No threshold: every row is reported."""
import argparse
import json
import os
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
CASES = [(n, share, table) for n in (4, 16) for share in (0.02, 0.20) for table in (0, 64)]
VARIANTS = ("distance_ms", "obscurance_ms", "all_ms")


def child(mode, config, root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, workloads
    from soft_list_ab import _timed
    print(f"ao_distance_ab: {mode} on {config}: preparing the scene", file=sys.stderr, flush=True)
    wl = workloads.prepare_config(config, cache=True)
    W, H, px = wl.W, wl.H, wl.W * wl.H
    sc = wl.scene
    med = lambda ts: float(np.median(ts))
    diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
    this = not mode.startswith("parent")
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_counts = ctx.malloc(px * 16), ctx.malloc(px * 16), ctx.malloc(px)
        d_dist, d_obs = (ctx.malloc(px * 4), ctx.malloc(px * 2)) if this else (None, None)
        falloff = api.AoFalloff.linear() if this else None
        api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
        ctx.synchronize()
        for n, share, table in CASES:
            ao = api.AoParams.make(n, diag * share, table=table, seed=5)
            row = {"config": config, "mode": mode, "n": n, "radius_share": share, "table": table, "steps": STEPS, "warmup": WARMUP, "W": W, "H": H}
            print(f"ao_distance_ab: {mode} on {config}: n {n}, radius {share:g} of the diagonal, table {table}", file=sys.stderr, flush=True)
            if not this:
                row["ao_ms"] = med(_timed(ctx, lambda: ctx.trace_ambient_occlusion_device(wl.constants, ao, d_pos, d_nrm, W, H, d_counts),
                                          STEPS, WARMUP))
                row["kernel"] = ctx.last_kernel_name()
                print(json.dumps(row), flush=True)
                continue
            planes = []
            for key, dist, obs in (("distance_ms", d_dist, None), ("obscurance_ms", None, d_obs), ("all_ms", d_dist, d_obs)):
                row[key] = med(_timed(ctx, lambda: ctx.trace_ambient_occlusion_distance_device(wl.constants, ao, falloff, d_pos, d_nrm, W, H,
                                                                                               d_counts, dist, obs), STEPS, WARMUP))
                out = np.zeros(px, np.uint8)
                ctx.d2h(out, d_counts)
                planes.append(out)
            row["kernel"] = ctx.last_kernel_name()
            row["mismatches"] = int((planes[1] != planes[0]).sum() + (planes[2] != planes[0]).sum())
            row["free_share"] = float(planes[0].mean()) / n
            print(json.dumps(row), flush=True)


def ratios(rows, config):
    out = []
    pick = lambda mode, same: next((r for r in rows if r["mode"] == mode and same(r)), None)
    for n, share, table in CASES:
        same = lambda r: (r.get("n"), r.get("radius_share"), r.get("table")) == (n, share, table)
        a, a2, b = pick("parent", same), pick("parent_again", same), pick("this", same)
        if a is None or a2 is None or b is None:
            continue
        parent, noise = 0.5 * (a["ao_ms"] + a2["ao_ms"]), abs(a["ao_ms"] - a2["ao_ms"])
        row = {"config": config, "mode": "ratio", "n": n, "radius_share": share, "table": table, "parent_ao_ms": [a["ao_ms"], a2["ao_ms"]],
               "noise_ms": noise, "mismatches": b["mismatches"], "kernel": b["kernel"], "free_share": b["free_share"]}
        for key in VARIANTS:
            stem = key[:-3]
            row[key] = b[key]
            row[stem + "_over_parent"] = b[key] / parent
            row[stem + "_above_noise"] = b[key] - parent > noise
        out.append(row)
    return out


def markdown(path):
    """The table of DESIGN.md 4.37 from a result file: figures above the parent by more than the row's noise figure in bold."""
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    print("| config | case | parent ms (twice) | noise ms | counts + distance ms (ratio) | counts + obscurance ms (ratio) | all three ms (ratio) |")
    print("|---|---|---|---|---|---|---|")
    for r in (r for r in rows if r["mode"] == "ratio"):
        two = r["parent_ao_ms"]
        cells = [r["config"], f"n {r['n']}, radius {r['radius_share']:g}, table {r['table']}", f"{two[0]:.3f} / {two[1]:.3f}", f"{r['noise_ms']:.3f}"]
        for key in VARIANTS:
            stem = key[:-3]
            cell = f"{r[key]:.3f} ({r[stem + '_over_parent']:.2f})"
            cells.append(f"**{cell}**" if r[stem + "_above_noise"] else cell)
        print("| " + " | ".join(cells) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="atrium_1080p,city_4k,courtyard_4k")
    ap.add_argument("--out", default="profiles/r45/ao_distance_ab.jsonl")
    ap.add_argument("--limit", type=int, default=420, help="seconds a child may run")
    ap.add_argument("--markdown", default="", metavar="FILE.jsonl", help="print the table of a result file and exit")
    ap.add_argument("--child", nargs=3, metavar=("MODE", "CONFIG", "ROOT"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if args.markdown:
        return markdown(args.markdown)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        def emit(line):
            out.write(line + "\n")
            out.flush()
            print(line, flush=True)
        for config in args.configs.split(","):
            runs = [("this", ROOT)]
            if args.parent_root:
                parent = os.path.abspath(args.parent_root)
                runs = [("parent", parent), ("this", ROOT), ("parent_again", parent)]
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
                    sys.exit(f"ao_distance_ab: {mode} on {config} failed or ran out of its time limit ({run.returncode})")
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
