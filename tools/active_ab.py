"""What an active map buys (GPU box): plain traces of the parent commit's library and of this one, and active traces of this one, on
the same frame in the same call -- DESIGN.md 4.11.

    python tools/active_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,...] [--out profiles/r09/active_ab.jsonl]

Variants (all the untuned default launch, "kernel" -1, no table, unless said):
    A  plain trace, the parent commit's library      (twice: its own spread is the yardstick)
    B  plain trace, this commit                       (the one timing condition: not slower than A by more than max(1.5 %, spread))
    C  active trace, all-ones map                     (the price of the byte and the ballot)
    D  active trace, facing map made once, untimed
    E  D + rtsh_facing_active_device in every frame   (a renderer that does not write the byte in its G-buffer pass)
    F  A after rts_ctx_autotune                       ("every ray, tuned")
Every variant: 20 warm-up and 200 timed launches between device events, the median and the mean reported.  A, B..E and F run in
child processes of this tool (a fresh process per library, each under its own time limit; this process never opens the GPU), B..E
alternating inside one child in four rounds of 50.  The tool stops at the first child that fails."""
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
    sys.path.insert(0, os.path.join(ROOT, "tests"))
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
        if mode in ("plain", "tuned"):
            if mode == "tuned":
                row["tuned_kernel"], row["tuner_ms"] = ctx.autotune(wl.constants, d_pos, W, H, d_mask, light=wl.light)
            out["F" if mode == "tuned" else "A"] = _timed(ctx, plain, STEPS, WARMUP)
            row["kernel_name"] = ctx.last_kernel_name()
        else:
            import oracle
            pos, nrm, _ = api.primary_gbuffer(wl.packed, wl.scene.eye, wl.scene.target, wl.scene.fovy, W, H)
            facing = api.facing_active(wl.constants, wl.light, pos, nrm)
            tiles = facing[:H - H % 8, :W - W % 8].reshape(H // 8, 8, W // 8, 8).max(axis=(1, 3))
            row["inactive_pixel_share"] = float(1.0 - facing.mean())
            row["idle_tile_share"] = float(1.0 - tiles.mean())
            d_nrm, d_ones, d_facing, d_scratch = ctx.malloc(nrm.nbytes), ctx.malloc(W * H), ctx.malloc(W * H), ctx.malloc(W * H)
            ctx.h2d(d_nrm, nrm)
            ctx.h2d(d_ones, np.ones(W * H, np.uint8))
            ctx.h2d(d_facing, facing)

            def per_frame():
                api.facing_active_device(ctx, wl.constants, wl.light, d_pos, d_nrm, W, H, d_scratch)
                ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_mask, light=wl.light, d_active=d_scratch)

            launches = {"B": plain,
                        "C": lambda: ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_mask, light=wl.light, d_active=d_ones),
                        "D": lambda: ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_mask, light=wl.light, d_active=d_facing),
                        "E": per_frame}
            names = {}
            for r in range(ROUNDS):                      # alternating: B C D E B C D E ...
                for v, launch in launches.items():
                    out.setdefault(v, []).extend(_timed(ctx, launch, STEPS // ROUNDS, WARMUP))
                    names[v] = ctx.last_kernel_name()
            row["kernel_names"] = names
            # parity at the size that was timed: D's mask against the oracle's times the map
            want, _, _ = oracle.shadow_mask(wl.packed, wl.constants.as_array(), oracle.light_from_product(wl.light, wl.constants), wl.positions, W, H)
            launches["D"]()
            got = np.empty((H, W), np.uint8)
            ctx.synchronize()
            ctx.d2h(got, d_mask)
            row["mismatches_D"] = int((got != want * (facing != 0)).sum())
        for v, ts in out.items():
            row[v] = {"median_ms": float(np.median(ts)), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts))}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p,city_4k_directional,city_4k_soft16")
    ap.add_argument("--out", default="profiles/r09/active_ab.jsonl")
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=170)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.config, os.path.abspath(args.root))
    parent = os.path.abspath(args.parent_root)
    if not os.path.exists(os.path.join(parent, "raytracedshadows_amd", "librts.so")):
        sys.exit(f"active_ab: no built library under {parent} (export the parent commit there and build it)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k != "RTS_LIB"}
    with open(args.out, "a") as fh:
        for config in args.configs.split(","):
            rows = {}
            for tag, mode, root in (("A1", "plain", parent), ("new", "variants", ROOT), ("A2", "plain", parent), ("F", "tuned", parent)):
                cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child", mode,
                       "--config", config, "--root", root]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True)
                line = next((l for l in p.stdout.splitlines() if l.startswith("ROW ")), None)
                if p.returncode != 0 or line is None:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    sys.exit(f"active_ab: {config} {tag} failed (exit {p.returncode}); nothing more is started")
                rows[tag] = json.loads(line[4:])
                rows[tag]["tag"] = tag
                fh.write(json.dumps(rows[tag]) + "\n")
                fh.flush()
            a1, a2, new = rows["A1"]["A"]["median_ms"], rows["A2"]["A"]["median_ms"], rows["new"]
            a = 0.5 * (a1 + a2)
            spread = abs(a1 - a2) / a
            bar = max(0.015, spread)
            summary = {"config": config, "tag": "summary", "A_ms": [a1, a2], "A_spread": spread, "B_ms": new["B"]["median_ms"],
                       "B_vs_A": new["B"]["median_ms"] / a - 1.0, "B_bar": bar, "B_holds": new["B"]["median_ms"] <= a * (1.0 + bar),
                       "C_vs_B": new["C"]["median_ms"] / new["B"]["median_ms"] - 1.0, "D_ms": new["D"]["median_ms"],
                       "D_of_A": new["D"]["median_ms"] / a, "E_ms": new["E"]["median_ms"], "E_of_A": new["E"]["median_ms"] / a,
                       "F_ms": rows["F"]["F"]["median_ms"], "F_of_A": rows["F"]["F"]["median_ms"] / a,
                       "inactive_pixel_share": new["inactive_pixel_share"], "idle_tile_share": new["idle_tile_share"],
                       "mismatches_D": new["mismatches_D"]}
            fh.write(json.dumps(summary) + "\n")
            fh.flush()
            print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
