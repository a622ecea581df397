"""What the occluder distance costs (GPU box): the plain mask trace of the parent commit's library and of this one, the mask trace
forced to the stackless packet, and distance traces of this one, on the same frame in the same call -- DESIGN.md 4.12.

    python tools/distance_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,...] [--out profiles/r12/distance_ab.jsonl]

Variants (the untuned default launch, "kernel" -1, no table, unless said):
    A  plain mask trace, the parent commit's library   (twice: its own spread is the yardstick)
    B  plain mask trace, this commit                    (the one timing condition: not slower than A by more than max(1.5 %, spread))
    C  mask trace forced to "kernel" 3                  (the stackless packet with its any-hit early-out: what D is built on)
    D  distance trace with d_mask given                 (no early-out, 4 more bytes stored per pixel)
    E  D through the facing map
Every variant: 20 warm-up and 200 timed launches between device events, the median and the mean reported.  A and B..E run in child
processes of this tool (a fresh process per library, each under its own time limit; this process never opens the GPU), B..E
alternating inside one child in four rounds of 50 (5 warm-up launches each).  The tool stops at the first child that fails."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, ROUNDS = 200, 20, 4


def _timed(ctx, launch, n, warmup):
    for _ in range(warmup):
        launch()
    ctx.synchronize()
    ts = []
    for _ in range(n):
        ctx.timer_mark(0)
        launch()
        ctx.timer_mark(1)
        ts.append(ctx.timer_between_ms(0, 1))
    ctx.synchronize()
    return ts


def child(mode, config, root):
    sys.path.insert(0, root)
    import numpy as np
    from raytracedshadows_amd import api, workloads
    assert os.path.abspath(api.lib_path()).startswith(os.path.abspath(root)), api.lib_path()
    wl = workloads.prepare_config(config, cache=True)
    W, H = wl.W, wl.H
    row = {"config": config, "mode": mode, "lib": "this commit" if os.path.abspath(root) == ROOT else "parent commit", "steps": STEPS, "warmup": WARMUP}
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_mask = ctx.malloc(wl.positions.nbytes), ctx.malloc(W * H)
        ctx.h2d(d_pos, wl.positions)
        plain = lambda: ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_mask, light=wl.light)
        out = {}
        if mode == "plain":
            out["A"] = _timed(ctx, plain, STEPS, WARMUP)
            row["kernel_name"] = ctx.last_kernel_name()
        else:
            pos, nrm, _ = api.primary_gbuffer(wl.packed, wl.scene.eye, wl.scene.target, wl.scene.fovy, W, H)
            facing = api.facing_active(wl.constants, wl.light, pos, nrm)
            row["inactive_pixel_share"] = float(1.0 - facing.mean())
            d_facing, d_dist, d_mask2 = ctx.malloc(W * H), ctx.malloc(W * H * 4), ctx.malloc(W * H)
            ctx.h2d(d_facing, facing)

            mask_trace = plain
            # (variant, "kernel" option set once before its launches and outside the timed region, launch)
            launches = {"B": (-1, mask_trace), "C": (3, mask_trace),
                        "D": (-1, lambda: ctx.trace_shadow_distance_device(wl.constants, d_pos, W, H, d_dist, d_mask=d_mask2, light=wl.light)),
                        "E": (-1, lambda: ctx.trace_shadow_distance_device(wl.constants, d_pos, W, H, d_dist, d_mask=d_mask2, light=wl.light,
                                                                           d_active=d_facing))}
            names = {}
            for r in range(ROUNDS):                      # alternating: B C D E B C D E ...; 20 warm-up launches per variant in all
                for v, (kernel, launch) in launches.items():
                    ctx.set_option("kernel", kernel)
                    out.setdefault(v, []).extend(_timed(ctx, launch, STEPS // ROUNDS, WARMUP // ROUNDS))
                    names[v] = ctx.last_kernel_name()
            ctx.set_option("kernel", -1)
            row["kernel_names"] = names
            # parity at the size that was timed: D's mask against C's, and against its own distances
            ctx.set_option("kernel", 3)
            launches["C"][1]()
            ctx.set_option("kernel", -1)
            launches["D"][1]()
            ctx.synchronize()
            m3, m, d = np.empty((H, W), np.uint8), np.empty((H, W), np.uint8), np.empty((H, W), np.float32)
            ctx.d2h(m3, d_mask); ctx.d2h(m, d_mask2); ctx.d2h(d, d_dist)
            row["mismatches_D_mask"] = int((m != m3).sum()) + int((m != np.isinf(d)).sum())
            row["occluded_share"] = float(1.0 - m.mean())
            row["occluded_share_of_active"] = float(1.0 - m[facing != 0].mean())
        for v, ts in out.items():
            row[v] = {"median_ms": float(np.median(ts)), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts))}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p,city_4k_directional")
    ap.add_argument("--out", default="profiles/r12/distance_ab.jsonl")
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=170)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.config, os.path.abspath(args.root))
    parent = os.path.abspath(args.parent_root)
    if not os.path.exists(os.path.join(parent, "raytracedshadows_amd", "librts.so")):
        sys.exit(f"distance_ab: no built library under {parent} (export the parent commit there and build it)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k != "RTS_LIB"}
    with open(args.out, "a") as fh:
        for config in args.configs.split(","):
            rows = {}
            for tag, mode, root in (("A1", "plain", parent), ("new", "variants", ROOT), ("A2", "plain", parent)):
                cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child", mode,
                       "--config", config, "--root", root]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True)
                line = next((l for l in p.stdout.splitlines() if l.startswith("ROW ")), None)
                if p.returncode != 0 or line is None:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    sys.exit(f"distance_ab: {config} {tag} failed (exit {p.returncode}); nothing more is started")
                rows[tag] = json.loads(line[4:])
                rows[tag]["tag"] = tag
                fh.write(json.dumps(rows[tag]) + "\n")
                fh.flush()
            a1, a2, new = rows["A1"]["A"]["median_ms"], rows["A2"]["A"]["median_ms"], rows["new"]
            a = 0.5 * (a1 + a2)
            spread = abs(a1 - a2) / a
            bar = max(0.015, spread)
            b, c, d, e = (new[v]["median_ms"] for v in "BCDE")
            summary = {"config": config, "tag": "summary", "A_ms": [a1, a2], "A_spread": spread, "B_ms": b, "B_vs_A": b / a - 1.0,
                       "B_bar": bar, "B_holds": b <= a * (1.0 + bar), "C_ms": c, "D_ms": d, "E_ms": e, "D_over_C": d / c, "D_over_B": d / b,
                       "E_over_D": e / d, "occluded_share": new["occluded_share"], "occluded_share_of_active": new["occluded_share_of_active"],
                       "inactive_pixel_share": new["inactive_pixel_share"], "mismatches_D_mask": new["mismatches_D_mask"],
                       "kernel_names": new["kernel_names"]}
            fh.write(json.dumps(summary) + "\n")
            fh.flush()
            print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
