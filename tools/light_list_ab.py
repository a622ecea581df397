"""What one light list dispatch costs against one dispatch per light (GPU box): L point lights on a ring around the scene's light, each
through its facing map, traced one after the other with the active mask trace and in one list trace, on the same frame in the same
call; and the plain mask trace of this commit against the parent commit's library -- DESIGN.md 4.14.

    python tools/light_list_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,atrium_1080p] [--lights 4,8]
                                  [--out profiles/r14/light_list_ab.jsonl]

Variants ("soft_split" 1, no table or order, unless said):
    P   plain mask trace of the workload's own light, the parent commit's library   (twice: its own spread is the yardstick)
    Q   the same, this commit                       (no mask kernel changed: within max(1.5 %, spread) of P)
    A   L successive active mask traces, light l through its own facing map, forced to "kernel" 3   (the list trace's family)
    A'  the same at the default kernel ("kernel" -1), untuned
    B4  ONE list trace through the facing_lights map, "kernel" 3, "soft_split" 1    (four waves per tile, wave w: lights w, w + 4)
    B1  the same with "soft_split" 0                (one wave walks every light)
Every variant: 20 warm-up and 200 timed launches (of all L traces, for A and A') between device events, the median and the mean
reported.  P and Q..B run in child processes of this tool (a fresh process per library, each under its own time limit; this process
never opens the GPU), Q..B alternating inside one child in four rounds of 50 (5 warm-up launches each).  The tool stops at the first
child that fails."""
import argparse
import json
import math
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


def ring(scene, count):
    """`count` point lights on a horizontal ring around the scene's light, its radius a tenth of the scene's diagonal."""
    import numpy as np
    c = np.asarray(scene.light_point, np.float64)
    r = 0.1 * float(np.linalg.norm(np.asarray(scene.bbox_max, np.float64) - np.asarray(scene.bbox_min, np.float64)))
    return [(1, (c[0] + r * math.cos(2 * math.pi * i / count), c[1], c[2] + r * math.sin(2 * math.pi * i / count))) for i in range(count)]


def child(mode, config, root, nlights):
    sys.path.insert(0, root)
    import numpy as np
    from raytracedshadows_amd import api, workloads
    assert os.path.abspath(api.lib_path()).startswith(os.path.abspath(root)), api.lib_path()
    wl = workloads.prepare_config(config, cache=True)
    W, H = wl.W, wl.H
    row = {"config": config, "mode": mode, "lights": nlights, "lib": "this commit" if os.path.abspath(root) == ROOT else "parent commit",
           "steps": STEPS, "warmup": WARMUP}
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_mask = ctx.malloc(wl.positions.nbytes), ctx.malloc(W * H)
        ctx.h2d(d_pos, wl.positions)
        plain = lambda: ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_mask, light=wl.light)
        out = {}
        if mode == "plain":
            out["P"] = _timed(ctx, plain, STEPS, WARMUP)
            row["kernel_name"] = ctx.last_kernel_name()
        else:
            lights = api.LightList.make(ring(wl.scene, nlights))
            d_pos2, d_nrm, d_map, d_list = ctx.malloc(W * H * 16), ctx.malloc(W * H * 16), ctx.malloc(W * H), ctx.malloc(W * H)
            api.primary_gbuffer_device(ctx, wl.scene.eye, wl.scene.target, wl.scene.fovy, W, H, d_pos2, d_nrm)
            api.facing_lights_device(ctx, wl.constants, lights, d_pos, d_nrm, W, H, d_map)
            ones = [lights.light(l) for l in range(nlights)]
            d_acts, d_masks = [ctx.malloc(W * H) for _ in ones], [ctx.malloc(W * H) for _ in ones]
            for l, one in enumerate(ones):
                api.facing_active_device(ctx, wl.constants, one, d_pos, d_nrm, W, H, d_acts[l])
            ctx.synchronize()
            lights_map = np.empty((H, W), np.uint8)
            ctx.d2h(lights_map, d_map)
            row["marked_share_per_light"] = [float(((lights_map >> l) & 1).mean()) for l in range(nlights)]
            row["pixels_without_a_light"] = float((lights_map == 0).mean())

            def per_light():
                for l, one in enumerate(ones):
                    ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_masks[l], light=one, d_active=d_acts[l])

            one_list = lambda: ctx.trace_light_list_device(wl.constants, lights, d_pos, W, H, d_list, d_lights_map=d_map)
            # (variant: "kernel" and "soft_split" set once before its launches and outside the timed region, launch)
            launches = {"Q": (-1, 1, plain), "A": (3, 1, per_light), "A'": (-1, 1, per_light), "B4": (3, 1, one_list), "B1": (3, 0, one_list)}
            names = {}
            for r in range(ROUNDS):                      # alternating: Q A A' B4 B1 Q A ...; 20 warm-up launches per variant in all
                for v, (kernel, split, launch) in launches.items():
                    ctx.set_option("kernel", kernel)
                    ctx.set_option("soft_split", split)
                    out.setdefault(v, []).extend(_timed(ctx, launch, STEPS // ROUNDS, WARMUP // ROUNDS))
                    names[v] = ctx.last_kernel_name()
            row["kernel_names"] = names
            # parity at the size that was timed: bit l of both list traces against light l's own active trace
            ctx.set_option("kernel", 3)
            ctx.set_option("soft_split", 1)
            per_light()
            ctx.synchronize()
            want = np.zeros((H, W), np.uint8)
            one = np.empty((H, W), np.uint8)
            for l in range(nlights):
                ctx.d2h(one, d_masks[l])
                want |= (one << l).astype(np.uint8)
            bad = 0
            got = np.empty((H, W), np.uint8)
            for split in (1, 0):
                ctx.set_option("soft_split", split)
                one_list()
                ctx.synchronize()
                ctx.d2h(got, d_list)
                bad += int((got != want).sum())
            ctx.set_option("soft_split", 1)
            ctx.set_option("kernel", -1)
            row["mismatches_B"] = bad
            row["lit_share_per_light"] = [float(((want >> l) & 1).mean()) for l in range(nlights)]
        for v, ts in out.items():
            row[v] = {"median_ms": float(np.median(ts)), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts))}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,atrium_1080p")
    ap.add_argument("--lights", default="4,8")
    ap.add_argument("--out", default="profiles/r14/light_list_ab.jsonl")
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--nlights", type=int, default=4)
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=280)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.config, os.path.abspath(args.root), args.nlights)
    parent = os.path.abspath(args.parent_root)
    if not os.path.exists(os.path.join(parent, "raytracedshadows_amd", "librts.so")):
        sys.exit(f"light_list_ab: no built library under {parent} (export the parent commit there and build it)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k != "RTS_LIB"}
    with open(args.out, "a") as fh:
        for config in args.configs.split(","):
            for nlights in (int(v) for v in args.lights.split(",")):
                rows = {}
                for tag, mode, root in (("P1", "plain", parent), ("new", "variants", ROOT), ("P2", "plain", parent)):
                    cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child", mode,
                           "--config", config, "--nlights", str(nlights), "--root", root]
                    p = subprocess.run(cmd, env=env, capture_output=True, text=True)
                    line = next((l for l in p.stdout.splitlines() if l.startswith("ROW ")), None)
                    if p.returncode != 0 or line is None:
                        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                        sys.exit(f"light_list_ab: {config} {nlights} lights {tag} failed (exit {p.returncode}); nothing more is started")
                    rows[tag] = json.loads(line[4:])
                    rows[tag]["tag"] = tag
                    fh.write(json.dumps(rows[tag]) + "\n")
                    fh.flush()
                p1, p2, new = rows["P1"]["P"]["median_ms"], rows["P2"]["P"]["median_ms"], rows["new"]
                pm = 0.5 * (p1 + p2)
                spread = abs(p1 - p2) / pm
                bar = max(0.015, spread)
                q, a, a_, b4, b1 = (new[v]["median_ms"] for v in ("Q", "A", "A'", "B4", "B1"))
                summary = {"config": config, "lights": nlights, "tag": "summary", "P_ms": [p1, p2], "P_spread": spread, "Q_ms": q,
                           "Q_vs_P": q / pm - 1.0, "Q_bar": bar, "Q_holds": q <= pm * (1.0 + bar), "A_ms": a, "A'_ms": a_, "B4_ms": b4,
                           "B1_ms": b1, "B4_over_A": b4 / a, "B1_over_A": b1 / a, "B4_over_A'": b4 / a_, "B1_over_A'": b1 / a_,
                           "B4_over_B1": b4 / b1, "mismatches_B": new["mismatches_B"], "pixels_without_a_light": new["pixels_without_a_light"],
                           "kernel_names": new["kernel_names"]}
                fh.write(json.dumps(summary) + "\n")
                fh.flush()
                print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
