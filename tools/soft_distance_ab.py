"""What the soft-shadow occluder distance costs (GPU box): the soft mask trace of the parent commit's library and of this one, the
soft mask trace forced to the stackless packet, and soft distance traces of this one with four waves per tile and with one, with and
without the facing map, on the same frame in the same call -- DESIGN.md 4.13.

    python tools/soft_distance_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k_soft16,...] [--out profiles/r13/soft_distance_ab.jsonl]

Variants (the untuned default launch, "kernel" -1, "soft_split" 1, no table or order, unless said):
    A   soft mask trace, the parent commit's library   (twice: its own spread is the yardstick)
    B   soft mask trace, this commit                    (no mask kernel changed: within max(1.5 %, spread) of A)
    C   soft mask trace forced to "kernel" 3            (the stackless packet with its any-hit early-out, 4 waves per tile: what D4 is built on)
    D4  soft distance trace with d_mask given           (no early-out, 4 more bytes stored per pixel; "soft_split" 1)
    D1  the same with "soft_split" 0                    (one wave walks every sample)
    E4, E1  D4 and D1 through the facing map
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
            soft = lambda active: (lambda: ctx.trace_soft_distance_device(wl.constants, d_pos, W, H, d_dist, d_mask=d_mask2, light=wl.light,
                                                                          d_active=active))
            # (variant, "kernel" and "soft_split" set once before its launches and outside the timed region, launch)
            launches = {"B": (-1, 1, mask_trace), "C": (3, 1, mask_trace), "D4": (-1, 1, soft(None)), "D1": (-1, 0, soft(None)),
                        "E4": (-1, 1, soft(d_facing)), "E1": (-1, 0, soft(d_facing))}
            names = {}
            for r in range(ROUNDS):                      # alternating: B C D4 D1 E4 E1 B C ...; 20 warm-up launches per variant in all
                for v, (kernel, split, launch) in launches.items():
                    ctx.set_option("kernel", kernel)
                    ctx.set_option("soft_split", split)
                    out.setdefault(v, []).extend(_timed(ctx, launch, STEPS // ROUNDS, WARMUP // ROUNDS))
                    names[v] = ctx.last_kernel_name()
            ctx.set_option("kernel", 3)
            ctx.set_option("soft_split", 1)
            row["kernel_names"] = names
            # parity at the size that was timed: both splits' counts against C's, and against their own distances
            launches["C"][2]()
            ctx.synchronize()
            m3, m, d = np.empty((H, W), np.uint8), np.empty((H, W), np.uint8), np.empty((H, W), np.float32)
            ctx.d2h(m3, d_mask)
            bad = 0
            ctx.set_option("kernel", -1)
            for split in (1, 0):
                ctx.set_option("soft_split", split)
                soft(None)()
                ctx.synchronize()
                ctx.d2h(m, d_mask2); ctx.d2h(d, d_dist)
                bad += int((m != m3).sum()) + int(((m == wl.light.nsamples) != np.isinf(d)).sum())
            ctx.set_option("soft_split", 1)
            row["mismatches_D_mask"] = bad
            n = float(wl.light.nsamples)
            row["occluded_share"] = float(1.0 - m.mean() / n)                       # of the rays
            row["occluded_share_of_active"] = float(1.0 - m[facing != 0].mean() / n)
            row["pixels_with_a_blocker"] = float(np.isfinite(d).mean())
        for v, ts in out.items():
            row[v] = {"median_ms": float(np.median(ts)), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts))}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k_soft16,courtyard_4k_soft16")
    ap.add_argument("--out", default="profiles/r13/soft_distance_ab.jsonl")
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=280)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.config, os.path.abspath(args.root))
    parent = os.path.abspath(args.parent_root)
    if not os.path.exists(os.path.join(parent, "raytracedshadows_amd", "librts.so")):
        sys.exit(f"soft_distance_ab: no built library under {parent} (export the parent commit there and build it)")
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
                    sys.exit(f"soft_distance_ab: {config} {tag} failed (exit {p.returncode}); nothing more is started")
                rows[tag] = json.loads(line[4:])
                rows[tag]["tag"] = tag
                fh.write(json.dumps(rows[tag]) + "\n")
                fh.flush()
            a1, a2, new = rows["A1"]["A"]["median_ms"], rows["A2"]["A"]["median_ms"], rows["new"]
            a = 0.5 * (a1 + a2)
            spread = abs(a1 - a2) / a
            bar = max(0.015, spread)
            b, c, d4, d1, e4, e1 = (new[v]["median_ms"] for v in ("B", "C", "D4", "D1", "E4", "E1"))
            summary = {"config": config, "tag": "summary", "A_ms": [a1, a2], "A_spread": spread, "B_ms": b, "B_vs_A": b / a - 1.0,
                       "B_bar": bar, "B_holds": b <= a * (1.0 + bar), "C_ms": c, "D4_ms": d4, "D1_ms": d1, "E4_ms": e4, "E1_ms": e1,
                       "D4_over_C": d4 / c, "D1_over_C": d1 / c, "D4_over_D1": d4 / d1, "E4_over_D4": e4 / d4, "E1_over_D1": e1 / d1,
                       "occluded_share": new["occluded_share"], "occluded_share_of_active": new["occluded_share_of_active"],
                       "pixels_with_a_blocker": new["pixels_with_a_blocker"], "inactive_pixel_share": new["inactive_pixel_share"],
                       "mismatches_D_mask": new["mismatches_D_mask"], "kernel_names": new["kernel_names"]}
            fh.write(json.dumps(summary) + "\n")
            fh.flush()
            print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
