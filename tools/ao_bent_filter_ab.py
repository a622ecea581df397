"""What the wide filter of the bent plane costs (GPU box), against the PARENT commit's wide filter of one count plane.  DESIGN.md 4.38.

    python tools/ao_bent_filter_ab.py --parent-root <tree of the parent commit, built>
                                      [--configs atrium_1080p,city_4k,courtyard_4k] [--out profiles/r46/ao_bent_filter_ab.jsonl]

Per config the frame is the primary G-buffer of the scene, the bent plane and the counts those of one 4-sample bent trace (radius 5 % of
the diagonal, table 64; in the parent's process: the AO trace's counts), thresholds N.N' >= 0.9 and 0.5 % of the diagonal; passes 1 .. 5.
  "parent":  the parent commit's library, rtsh_wide_filter_soft_light_list_device for ONE light (the stand-in list) over the counts:
             filter_ms.  The parent runs TWICE per config, before and after this commit's library ("parent" and "parent_again"): the
             spread of its two medians is the row's noise figure.
  "this":    rtsh_wide_filter_bent_device over the bent plane, with `ao`: bent_ms.
Each figure: 10 warm-up and 60 timed calls (a call is max(1, passes) launches) between device events, the median.  Every library runs in
a child process of its own, under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.
After the rows of a config: one "ratio" row per passes -- bent_ms over the mean of the parent's two medians (the bent filter moves four
channels to the baseline's one: a ratio above 1 is expected), the noise figure, and the per-step increments of both (passes k minus
passes k - 1) as DESIGN.md 4.25 reports them.  `--markdown` prints the table for DESIGN.md, ratios above 1 beyond the noise in bold.
No threshold: every row is reported."""
import argparse
import json
import os
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
PASSES = (1, 2, 3, 4, 5)


def child(mode, config, root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, workloads
    from soft_list_ab import _timed
    print(f"ao_bent_filter_ab: {mode} on {config}: preparing the scene", file=sys.stderr, flush=True)
    wl = workloads.prepare_config(config, cache=True)
    W, H, px = wl.W, wl.H, wl.W * wl.H
    sc = wl.scene
    med = lambda ts: float(np.median(ts))
    diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
    this = not mode.startswith("parent")
    ao = api.AoParams.make(4, diag * 0.05, table=64, seed=5)
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_counts, d_ao = ctx.malloc(px * 16), ctx.malloc(px * 16), ctx.malloc(px), ctx.malloc(px * 4)
        api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
        if this:
            d_bent, d_out = ctx.malloc(px * 16), ctx.malloc(px * 16)
            d_scratch = ctx.malloc(api.wide_filter_bent_scratch_bytes(W, H))
            ctx.trace_ambient_occlusion_bent_device(wl.constants, ao, d_pos, d_nrm, W, H, d_counts, d_bent)
        else:
            d_scratch = ctx.malloc(api.wide_filter_scratch_bytes(1, W, H))
            ctx.trace_ambient_occlusion_device(wl.constants, ao, d_pos, d_nrm, W, H, d_counts)
        ctx.synchronize()
        lst = ao.stand_in_list()
        for passes in PASSES:
            p = api.WideFilterParams.make(passes, 0.9, 0.005 * diag)
            row = {"config": config, "mode": mode, "passes": passes, "steps": STEPS, "warmup": WARMUP, "W": W, "H": H}
            if this:
                row["bent_ms"] = med(_timed(ctx, lambda: api.wide_filter_bent_device(ctx, p, 4, d_pos, d_nrm, d_bent, W, H, d_out, d_ao=d_ao,
                                                                                     d_scratch=d_scratch), STEPS, WARMUP))
            else:
                row["filter_ms"] = med(_timed(ctx, lambda: api.wide_filter_soft_light_list_device(ctx, lst, p, d_pos, d_nrm, d_counts, W, H, d_ao,
                                                                                                  d_scratch=d_scratch), STEPS, WARMUP))
            plane = np.zeros(px, np.float32)
            ctx.d2h(plane, d_ao)
            row["mean_ao"] = float(plane.mean())
            print(json.dumps(row), flush=True)


def ratios(rows, config):
    out = []
    pick = lambda mode, passes: next((r for r in rows if r["mode"] == mode and r["passes"] == passes), None)
    before = None
    for passes in PASSES:
        a, a2, b = pick("parent", passes), pick("parent_again", passes), pick("this", passes)
        if a is None or a2 is None or b is None:
            continue
        parent, noise = 0.5 * (a["filter_ms"] + a2["filter_ms"]), abs(a["filter_ms"] - a2["filter_ms"])
        row = {"config": config, "mode": "ratio", "passes": passes, "parent_filter_ms": [a["filter_ms"], a2["filter_ms"]], "noise_ms": noise,
               "bent_ms": b["bent_ms"], "bent_over_parent": b["bent_ms"] / parent, "above_noise": b["bent_ms"] - parent > noise,
               "same_ao": b["mean_ao"] == a["mean_ao"]}
        if before is not None:
            row["parent_step_ms"], row["bent_step_ms"] = parent - before[0], b["bent_ms"] - before[1]
        before = (parent, b["bent_ms"])
        out.append(row)
    return out


def markdown(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    print("| config | passes | parent, one plane ms (twice) | noise ms | bent ms | ratio | step: parent ms | step: bent ms |")
    print("|---|---|---|---|---|---|---|---|")
    for r in (r for r in rows if r["mode"] == "ratio"):
        two = r["parent_filter_ms"]
        ratio = f"{r['bent_over_parent']:.2f}"
        step = lambda key: f"{r[key]:.3f}" if key in r else "-"
        print(f"| {r['config']} | {r['passes']} | {two[0]:.3f} / {two[1]:.3f} | {r['noise_ms']:.3f} | {r['bent_ms']:.3f} | "
              f"{'**' + ratio + '**' if r['above_noise'] else ratio} | {step('parent_step_ms')} | {step('bent_step_ms')} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="atrium_1080p,city_4k,courtyard_4k")
    ap.add_argument("--out", default="profiles/r46/ao_bent_filter_ab.jsonl")
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
                    sys.exit(f"ao_bent_filter_ab: {mode} on {config} failed or ran out of its time limit ({run.returncode})")
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
