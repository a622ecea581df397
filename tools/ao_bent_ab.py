"""What a bent-normal ambient occlusion trace costs (GPU box), against the PARENT commit's AO trace over the same rays.  DESIGN.md 4.36.

    python tools/ao_bent_ab.py --parent-root <tree of the parent commit, built>
                               [--configs atrium_1080p,city_4k] [--out profiles/r44/ao_bent_ab.jsonl]

Rows: tools/ao_ab.py's -- per config, n = 4 and 16 samples, a radius of 2 % and 20 % of the scene's diagonal, table 0 and 64
(AoParams.make, seed 5).
  "parent":  the parent commit's library, rts_trace_ambient_occlusion_device in the family blockFamily picks ("kernel" -1): ao_ms; and
             combine_ms, its rtsh_combine_visibility_list_ao_device over one light.  The parent runs TWICE per config, before and after
             this commit's library ("parent" and "parent_again"): the spread of its two medians is the row's noise figure.
  "this":    bent_ms: rts_trace_ambient_occlusion_bent_device with counts, "kernel" -1;  bent_alone_ms: the same with counts = NULL;
             split0_ms: the packet family with "soft_split" 0;  mismatches: words of bent or bytes of counts of the other launches
             that differ from the first one's (must be 0);  combine_ms: rtsh_combine_visibility_list_ao_bent_device over the same
             planes and the trace's bent plane.
Each figure: 10 warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of its own,
under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.
After the rows of a config: one "ratio" row per case -- bent_ms over the mean of the parent's two medians, the noise figure, and
`above_noise` where bent_ms exceeds that mean by more than the noise -- and one for the combine; `--markdown` prints the table for
DESIGN.md with those rows in bold.  No threshold: every row is reported."""
import argparse
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
    from raytracedshadows_amd import api, workloads
    from soft_list_ab import _timed
    print(f"ao_bent_ab: {mode} on {config}: preparing the scene", file=sys.stderr, flush=True)
    wl = workloads.prepare_config(config, cache=True)
    W, H, px = wl.W, wl.H, wl.W * wl.H
    sc = wl.scene
    med = lambda ts: float(np.median(ts))
    diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
    this = not mode.startswith("parent")
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_counts = ctx.malloc(px * 16), ctx.malloc(px * 16), ctx.malloc(px)
        d_bent = ctx.malloc(px * 16) if this else None
        api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
        ctx.synchronize()
        for n, share, table in CASES:
            ao = api.AoParams.make(n, diag * share, table=table, seed=5)
            row = {"config": config, "mode": mode, "n": n, "radius_share": share, "table": table, "steps": STEPS, "warmup": WARMUP, "W": W, "H": H}
            print(f"ao_bent_ab: {mode} on {config}: n {n}, radius {share:g} of the diagonal, table {table}", file=sys.stderr, flush=True)
            if not this:
                row["ao_ms"] = med(_timed(ctx, lambda: ctx.trace_ambient_occlusion_device(wl.constants, ao, d_pos, d_nrm, W, H, d_counts),
                                          STEPS, WARMUP))
                row["kernel"] = ctx.last_kernel_name()
                print(json.dumps(row), flush=True)
                continue
            planes = []

            def run(key, kernel, split, counts=True):
                ctx.set_option("kernel", kernel)
                ctx.set_option("soft_split", split)
                row[key] = med(_timed(ctx, lambda: ctx.trace_ambient_occlusion_bent_device(wl.constants, ao, d_pos, d_nrm, W, H,
                                                                                           d_counts if counts else None, d_bent), STEPS, WARMUP))
                out = np.zeros(17 * px, np.uint8)
                ctx.d2h(out[:16 * px], d_bent)
                ctx.d2h(out[16 * px:], d_counts)
                planes.append(out)
                return ctx.last_kernel_name()

            row["kernel"] = run("bent_ms", -1, 1)
            run("bent_alone_ms", -1, 1, counts=False)
            row["split0_kernel"] = run("split0_ms", 3, 0)
            ctx.set_option("kernel", -1)
            ctx.set_option("soft_split", 1)
            row["mismatches"] = int((planes[1] != planes[0]).sum() + (planes[2] != planes[0]).sum())
            row["free_share"] = float(planes[0][16 * px:].mean()) / n
            print(json.dumps(row), flush=True)
        # the combine: one light, a visibility plane and an AO plane of random floats; this commit's form reads the last trace's bent plane
        rs = np.random.RandomState(7)
        d_vis, d_ao, d_rgb = ctx.malloc(px * 4), ctx.malloc(px * 4), ctx.malloc(px * 3)
        ctx.h2d(d_vis, rs.random_sample(px).astype(np.float32))
        ctx.h2d(d_ao, rs.random_sample(px).astype(np.float32))
        lst = api.LightList.make([(api.Light.DIRECTIONAL, list(wl.constants.lightDirection)[:3])])
        row = {"config": config, "mode": mode, "case": "combine", "steps": STEPS, "warmup": WARMUP, "W": W, "H": H}
        if this:
            sky = api.SkyAmbient.make(up=(0.0, 1.0, 0.0), sky=(0.5, 0.7, 1.0), ground=(0.4, 0.3, 0.2))
            launch = lambda: api.combine_visibility_list_ao_bent_device(ctx, wl.constants, lst, d_pos, d_nrm, d_vis, d_ao, d_bent, sky, W, H, d_rgb)
        else:
            launch = lambda: api.combine_visibility_list_ao_device(ctx, wl.constants, lst, d_pos, d_nrm, d_vis, d_ao, W, H, d_rgb)
        row["combine_ms"] = med(_timed(ctx, launch, STEPS, WARMUP))
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
        out.append({"config": config, "mode": "ratio", "n": n, "radius_share": share, "table": table, "parent_ao_ms": [a["ao_ms"], a2["ao_ms"]],
                    "noise_ms": noise, "bent_ms": b["bent_ms"], "bent_alone_ms": b["bent_alone_ms"], "split0_ms": b["split0_ms"],
                    "bent_over_parent": b["bent_ms"] / parent, "above_noise": b["bent_ms"] - parent > noise, "mismatches": b["mismatches"],
                    "kernel": b["kernel"]})
    same = lambda r: r.get("case") == "combine"
    a, a2, b = pick("parent", same), pick("parent_again", same), pick("this", same)
    if a is not None and a2 is not None and b is not None:
        parent, noise = 0.5 * (a["combine_ms"] + a2["combine_ms"]), abs(a["combine_ms"] - a2["combine_ms"])
        out.append({"config": config, "mode": "ratio", "case": "combine", "parent_combine_ms": [a["combine_ms"], a2["combine_ms"]],
                    "noise_ms": noise, "combine_ms": b["combine_ms"], "bent_over_parent": b["combine_ms"] / parent,
                    "above_noise": b["combine_ms"] - parent > noise})
    return out


def markdown(path):
    """The table of DESIGN.md 4.36 from a result file: rows above the parent by more than their noise figure in bold."""
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    print("| config | case | parent ms (twice) | noise ms | this ms | ratio |")
    print("|---|---|---|---|---|---|")
    for r in (r for r in rows if r["mode"] == "ratio"):
        case = "combine" if r.get("case") == "combine" else f"n {r['n']}, radius {r['radius_share']:g}, table {r['table']}"
        two = r.get("parent_ao_ms") or r["parent_combine_ms"]
        ms = r.get("bent_ms", r.get("combine_ms"))
        cells = [r["config"], case, f"{two[0]:.3f} / {two[1]:.3f}", f"{r['noise_ms']:.3f}", f"{ms:.3f}", f"{r['bent_over_parent']:.2f}"]
        if r["above_noise"]:
            cells = [f"**{c}**" for c in cells]
        print("| " + " | ".join(cells) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="atrium_1080p,city_4k")
    ap.add_argument("--out", default="profiles/r44/ao_bent_ab.jsonl")
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
                    sys.exit(f"ao_bent_ab: {mode} on {config} failed or ran out of its time limit ({run.returncode})")
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
