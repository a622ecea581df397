"""What accumulating the bent texel and filtering it from the mean cost (GPU box), against the PARENT commit's nearest shipped passes.
DESIGN.md 4.39.

    python tools/ao_bent_temporal_ab.py --parent-root <tree of the parent commit, built>
                                        [--configs atrium_1080p,city_4k,courtyard_4k] [--out profiles/r47/ao_bent_temporal_ab.jsonl]

Per config two frames: the previous eye is the scene's turned about the target by 1 degree, so that a pixel gathers four taps; both
G-buffers are the primary pass's.  One 4-sample bent trace per frame (radius 5 % of the diagonal, table 64, the second frame's directions
turned by one golden angle where the library has AoParams.rotated), thresholds N.N' >= 0.9 and 0.5 % of the diagonal, max_length 32.  The
history of the timed call is a first-frame accumulate of the previous frame.
  "parent":  the parent commit's library --
             accumulate_ms: rtsh_accumulate_moments_soft_light_list_device for ONE light (the stand-in list) over the trace's counts, the
                            nearest shipped pass (1 + 7 bytes per pixel plus up to 4 x 7 gathered);
             filter_ms:     rtsh_wide_filter_bent_device over this frame's float plane, passes 1 .. 5.
             The parent runs TWICE per config, before and after this commit's library ("parent" and "parent_again"): the spread of its
             two medians is the row's noise figure.
  "this":    accumulate_ms: rtsh_accumulate_bent_device (16 + 8 + 1 bytes per pixel plus up to 4 x 9 gathered);
             filter_ms:     rtsh_wide_filter_bent_mean_device over the accumulated texels, with `ao`, at the same passes.
Each figure: 10 warm-up and 60 timed calls (a filter call is max(1, passes) launches) between device events, the median.  Every library
runs in a child process of its own, under its own time limit; this process never opens the GPU, and the tool stops at the first child
that fails.  After the rows of a config: one "ratio" row for the accumulate and one per passes for the filter -- this commit's median
over the mean of the parent's two, and the noise figure.  `--markdown` prints the table for DESIGN.md, ratios above 1 beyond the noise
in bold.  No threshold: every row is reported."""
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
    from list_temporal_ab import orbit
    from soft_list_ab import _timed
    print(f"ao_bent_temporal_ab: {mode} on {config}: preparing the scene", file=sys.stderr, flush=True)
    wl = workloads.prepare_config(config, cache=True)
    W, H, px = wl.W, wl.H, wl.W * wl.H
    sc = wl.scene
    med = lambda ts: float(np.median(ts))
    diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
    this = not mode.startswith("parent")
    n = 4
    ao = api.AoParams.make(n, diag * 0.05, table=64, seed=5)
    cos_min, plane_eps = 0.9, 0.005 * diag
    prev_eye = orbit(sc.eye, sc.target, -1.0)
    b = api.camera_basis(prev_eye, sc.target, sc.fovy, W, H)
    tp = api.TemporalParams.make(np.asarray(sc.eye, np.float32) - np.asarray(prev_eye, np.float32), b["right"], b["up"], b["fwd"],
                                 np.float32(b["tan_half"] * b["aspect"]), b["tan_half"], cos_min, plane_eps, 32, 0)
    first = api.TemporalParams.make((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), 1.0, 1.0, cos_min, plane_eps, 32, 0)
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_ppos, d_pnrm = (ctx.malloc(px * 16) for _ in range(4))
        d_counts, d_bent, d_out, d_ao = ctx.malloc(px), ctx.malloc(px * 16), ctx.malloc(px * 16), ctx.malloc(px * 4)
        d_scratch = ctx.malloc(api.wide_filter_bent_scratch_bytes(W, H))
        api.primary_gbuffer_device(ctx, prev_eye, sc.target, sc.fovy, W, H, d_ppos, d_pnrm)
        api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
        k_prev = api.RayTracingConstants.make(prev_eye, sc.light_direction, W, H)
        row = {"config": config, "mode": mode, "stage": "accumulate", "steps": STEPS, "warmup": WARMUP, "W": W, "H": H}
        if this:
            hist, cur = (ctx.malloc(px * 8), ctx.malloc(px)), (ctx.malloc(px * 8), ctx.malloc(px))
            ctx.trace_ambient_occlusion_bent_device(k_prev, ao, d_ppos, d_pnrm, W, H, d_counts, d_bent)
            api.accumulate_bent_device(ctx, first, n, d_ppos, d_pnrm, d_bent, W, H, hist[0], hist[1])
            ctx.trace_ambient_occlusion_bent_device(wl.constants, ao.rotated(1), d_pos, d_nrm, W, H, d_counts, d_bent)
            ctx.synchronize()
            prev = (d_ppos, d_pnrm, hist[0], hist[1])
            row["accumulate_ms"] = med(_timed(ctx, lambda: api.accumulate_bent_device(ctx, tp, n, d_pos, d_nrm, d_bent, W, H, cur[0], cur[1],
                                                                                      d_prev=prev), STEPS, WARMUP))
            lengths = np.zeros(px, np.uint8)
            ctx.d2h(lengths, cur[1])
        else:
            lst = ao.stand_in_list()
            hist, cur = tuple(ctx.malloc(px * s) for s in (2, 4, 1)), tuple(ctx.malloc(px * s) for s in (2, 4, 1))
            ctx.trace_ambient_occlusion_bent_device(k_prev, ao, d_ppos, d_pnrm, W, H, d_counts, d_bent)
            api.accumulate_moments_soft_light_list_device(ctx, lst, first, d_ppos, d_pnrm, d_counts, W, H, *hist)
            ctx.trace_ambient_occlusion_bent_device(wl.constants, ao, d_pos, d_nrm, W, H, d_counts, d_bent)
            ctx.synchronize()
            prev = (d_ppos, d_pnrm) + hist
            row["accumulate_ms"] = med(_timed(ctx, lambda: api.accumulate_moments_soft_light_list_device(
                ctx, lst, tp, d_pos, d_nrm, d_counts, W, H, *cur, d_prev=prev), STEPS, WARMUP))
            lengths = np.zeros(px, np.uint8)
            ctx.d2h(lengths, cur[2])
        row["blended"] = float((lengths == 2).mean())                     # the share of pixels that found history: the same in both
        print(json.dumps(row), flush=True)
        for passes in PASSES:
            p = api.WideFilterParams.make(passes, cos_min, plane_eps)
            row = {"config": config, "mode": mode, "stage": "filter", "passes": passes, "steps": STEPS, "warmup": WARMUP, "W": W, "H": H}
            if this:
                row["filter_ms"] = med(_timed(ctx, lambda: api.wide_filter_bent_mean_device(ctx, p, n, d_pos, d_nrm, cur[0], W, H, d_out, d_ao=d_ao,
                                                                                            d_scratch=d_scratch), STEPS, WARMUP))
            else:
                row["filter_ms"] = med(_timed(ctx, lambda: api.wide_filter_bent_device(ctx, p, n, d_pos, d_nrm, d_bent, W, H, d_out, d_ao=d_ao,
                                                                                       d_scratch=d_scratch), STEPS, WARMUP))
            plane = np.zeros(px, np.float32)
            ctx.d2h(plane, d_ao)
            row["mean_ao"] = float(plane.mean())
            print(json.dumps(row), flush=True)


def ratios(rows, config):
    out = []

    def pick(mode, stage, passes=None):
        return next((r for r in rows if r["mode"] == mode and r["stage"] == stage and r.get("passes") == passes), None)

    for stage, key, each in (("accumulate", "accumulate_ms", (None,)), ("filter", "filter_ms", PASSES)):
        for passes in each:
            a, a2, b = pick("parent", stage, passes), pick("parent_again", stage, passes), pick("this", stage, passes)
            if a is None or a2 is None or b is None:
                continue
            parent, noise = 0.5 * (a[key] + a2[key]), abs(a[key] - a2[key])
            out.append({"config": config, "mode": "ratio", "stage": stage, "passes": passes, "parent_ms": [a[key], a2[key]], "noise_ms": noise,
                        "this_ms": b[key], "this_over_parent": b[key] / parent, "above_noise": b[key] - parent > noise})
    return out


def markdown(path):
    rows = [json.loads(line) for line in open(path) if line.startswith("{")]
    print("| config | stage | passes | parent ms (twice) | noise ms | this ms | ratio |")
    print("|---|---|---|---|---|---|---|")
    for r in (r for r in rows if r["mode"] == "ratio"):
        two = r["parent_ms"]
        ratio = f"{r['this_over_parent']:.2f}"
        print(f"| {r['config']} | {r['stage']} | {'-' if r['passes'] is None else r['passes']} | {two[0]:.3f} / {two[1]:.3f} | "
              f"{r['noise_ms']:.3f} | {r['this_ms']:.3f} | {'**' + ratio + '**' if r['above_noise'] else ratio} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="atrium_1080p,city_4k,courtyard_4k")
    ap.add_argument("--out", default="profiles/r47/ao_bent_temporal_ab.jsonl")
    ap.add_argument("--append", action="store_true", help="add to --out instead of starting it anew (one config per call)")
    ap.add_argument("--limit", type=int, default=420, help="seconds a child may run")
    ap.add_argument("--markdown", default="", metavar="FILE.jsonl", help="print the table of a result file and exit")
    ap.add_argument("--child", nargs=3, metavar=("MODE", "CONFIG", "ROOT"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    if args.markdown:
        return markdown(args.markdown)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as out:
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
                    sys.exit(f"ao_bent_temporal_ab: {mode} on {config} failed or ran out of its time limit ({run.returncode})")
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
