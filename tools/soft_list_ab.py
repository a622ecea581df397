"""What one soft light list dispatch costs against one soft mask dispatch per light (GPU box): point lights on a ring around the scene's
light, each of several samples, traced one after the other with the parent commit's active mask trace and in ONE list trace of this
commit, on the same frame; and the plain soft mask trace of this commit against the parent commit's library -- DESIGN.md 4.17.

    python tools/soft_list_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,courtyard_4k,atrium_1080p]
                                 [--out profiles/r19/soft_list_ab.jsonl]

Lists: "4x4" = 4 lights of 4 samples, "2x16" = 2 lights of 16, every light its own range of one 48-entry table, the radius 1 % of the
scene's diagonal; each without a map and ("f") through the facing map.  Variants, all at the untuned default launch ("kernel" -1, no
split table or order):
    S     plain soft mask trace, 16 samples, the parent commit's library   (twice, before and after: its own spread is the yardstick)
    A     one active mask trace per light, the parent commit's library     (twice; the baseline of the list)
    T     plain soft mask trace, 16 samples, this commit                   (no mask kernel changed: within max(1.5 %, spread) of S)
    L4    ONE list trace, "soft_split" 1                                   (four waves per tile, the pairs dealt over them)
    L1    the same with "soft_split" 0                                     (one wave walks every pair)
Every variant: 20 warm-up and 200 timed launches (of all the lights' traces, for A) between device events, the median reported.  The
parent's and this commit's variants run in child processes of this tool (a fresh process per library, each under its own time limit;
this process never opens the GPU), this commit's variants alternating inside one child in four rounds of 50 (5 warm-up launches each).
The tool stops at the first child that fails.  Beside the times: the planes of both list traces against the per-light traces of the
same process, byte for byte, at the size timed."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, ROUNDS = 200, 20, 4
LISTS = {"4x4": (4, 4), "2x16": (2, 16)}                 # name -> (lights, samples per light)


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


def entries(scene, count, samples):
    """`count` point lights on a horizontal ring around the scene's light (its radius a tenth of the scene's diagonal), light l the
    `samples` table entries from l * samples on, scaled to 1 % of the diagonal: (kind, xyz, nsamples, first, radius)."""
    import numpy as np
    c = np.asarray(scene.light_point, np.float64)
    diag = float(np.linalg.norm(np.asarray(scene.bbox_max, np.float64) - np.asarray(scene.bbox_min, np.float64)))
    r = 0.1 * diag
    return [(1, (c[0] + r * math.cos(2 * math.pi * i / count), c[1], c[2] + r * math.sin(2 * math.pi * i / count)), samples, i * samples,
             0.01 * diag) for i in range(count)]


def child(mode, config, root):
    sys.path.insert(0, root)
    import numpy as np
    from raytracedshadows_amd import api, scenes, workloads
    assert os.path.abspath(api.lib_path()).startswith(os.path.abspath(root)), api.lib_path()
    wl = workloads.prepare_config(config, cache=True)
    W, H = wl.W, wl.H
    table = scenes.jitter_offsets(48, 1.0, 19)
    row = {"config": config, "mode": mode, "lib": "this commit" if os.path.abspath(root) == ROOT else "parent commit", "steps": STEPS,
           "warmup": WARMUP}
    med = lambda ts: float(np.median(ts))
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_mask, d_nrm, d_map = ctx.malloc(wl.positions.nbytes), ctx.malloc(W * H), ctx.malloc(W * H * 16), ctx.malloc(W * H)
        d_pos2 = ctx.malloc(W * H * 16)
        ctx.h2d(d_pos, wl.positions)
        api.primary_gbuffer_device(ctx, wl.scene.eye, wl.scene.target, wl.scene.fovy, W, H, d_pos2, d_nrm)
        soft16 = workloads.relight(wl, "point", 16, 0.01, 0).light
        plain = lambda: ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_mask, light=soft16)
        d_acts, d_masks = [ctx.malloc(W * H) for _ in range(4)], [ctx.malloc(W * H) for _ in range(4)]
        d_counts = ctx.malloc(8 * W * H)
        out, names = {}, {}
        cases = {}
        for name, (count, samples) in LISTS.items():
            es = entries(wl.scene, count, samples)
            # the derived lights (include/rts.h), made here so that the parent commit's library can trace them: radius * table[first + j]
            ones = [api.Light.make(kind, xyz, np.float32(radius) * table[first:first + n, :3]) for kind, xyz, n, first, radius in es]
            cases[name] = (es, ones)

        def per_light(ones, facing):
            def run():
                for l, one in enumerate(ones):
                    ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_masks[l], light=one, d_active=d_acts[l] if facing else None)
            return run

        def facing_maps(es, ones):
            hard = api.LightList.make([(kind, xyz) for kind, xyz, _, _, _ in es])
            api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
            for l, one in enumerate(ones):
                api.facing_active_device(ctx, wl.constants, one, d_pos, d_nrm, W, H, d_acts[l])
            ctx.synchronize()

        if mode == "parent":
            out["S"] = _timed(ctx, plain, STEPS, WARMUP)
            names["S"] = ctx.last_kernel_name()
            for name, (es, ones) in cases.items():
                facing_maps(es, ones)
                for f in ("", "f"):
                    out["A_%s%s" % (name, f)] = _timed(ctx, per_light(ones, bool(f)), STEPS, WARMUP)
                    names["A_%s%s" % (name, f)] = ctx.last_kernel_name()
        else:
            for r in range(ROUNDS):                      # alternating: T, then per list L4 L1 L4f L1f; 20 warm-up launches per variant in all
                ctx.set_option("soft_split", 1)
                out.setdefault("T", []).extend(_timed(ctx, plain, STEPS // ROUNDS, WARMUP // ROUNDS))
                names["T"] = ctx.last_kernel_name()
                for name, (es, ones) in cases.items():
                    lights = api.SoftLightList.make(es, table)
                    facing_maps(es, ones)
                    for f in ("", "f"):
                        one_list = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts,
                                                                            d_lights_map=d_map if f else None)
                        for split in (1, 0):
                            v = "L%d_%s%s" % (4 if split else 1, name, f)
                            ctx.set_option("soft_split", split)
                            out.setdefault(v, []).extend(_timed(ctx, one_list, STEPS // ROUNDS, WARMUP // ROUNDS))
                            names[v] = ctx.last_kernel_name()
            # parity at the size that was timed: the planes of both list traces against each light's own active trace
            ctx.set_option("soft_split", 1)
            parity, shares = {}, {}
            one, planes = np.empty((H, W), np.uint8), None
            for name, (es, ones) in cases.items():
                lights = api.SoftLightList.make(es, table)
                facing_maps(es, ones)
                for f in ("", "f"):
                    per_light(ones, bool(f))()
                    ctx.synchronize()
                    want = []
                    for l in range(len(ones)):
                        ctx.d2h(one, d_masks[l])
                        want.append(one.copy())
                    want = np.stack(want)
                    bad = 0
                    for split in (1, 0):
                        ctx.set_option("soft_split", split)
                        ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_map if f else None)
                        ctx.synchronize()
                        planes = np.empty((8, H, W), np.uint8)
                        ctx.d2h(planes, d_counts)
                        bad += int((planes[:len(ones)] != want).sum())
                    parity["%s%s" % (name, f)] = bad
                    n = es[0][2]
                    shares["%s%s" % (name, f)] = {"penumbra_share_per_light": [float(((w > 0) & (w < n)).mean()) for w in want]}
                m = np.empty((H, W), np.uint8)
                ctx.d2h(m, d_map)
                shares[name]["marked_share_per_light"] = [float(((m >> l) & 1).mean()) for l in range(len(ones))]
            row["mismatches_against_the_per_light_traces"] = parity
            row["shares"] = shares
        row["kernel_names"] = names
        row.update({v: {"median_ms": med(ts), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts))} for v, ts in out.items()})
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r19/soft_list_ab.jsonl")
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=420)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.config, os.path.abspath(args.root))
    parent = os.path.abspath(args.parent_root)
    if not os.path.exists(os.path.join(parent, "raytracedshadows_amd", "librts.so")):
        sys.exit(f"soft_list_ab: no built library under {parent} (export the parent commit there and build it)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k != "RTS_LIB"}
    with open(args.out, "a") as fh:
        for config in args.configs.split(","):
            rows = {}
            for tag, mode, root in (("A1", "parent", parent), ("new", "variants", ROOT), ("A2", "parent", parent)):
                cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child", mode,
                       "--config", config, "--root", root]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True)
                line = next((l for l in p.stdout.splitlines() if l.startswith("ROW ")), None)
                if p.returncode != 0 or line is None:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    sys.exit(f"soft_list_ab: {config} {tag} failed (exit {p.returncode}); nothing more is started")
                rows[tag] = json.loads(line[4:])
                rows[tag]["tag"] = tag
                fh.write(json.dumps(rows[tag]) + "\n")
                fh.flush()
            a1, a2, new = rows["A1"], rows["A2"], rows["new"]
            s_ms = 0.5 * (a1["S"]["median_ms"] + a2["S"]["median_ms"])
            spread = abs(a1["S"]["median_ms"] - a2["S"]["median_ms"]) / s_ms
            bar = max(0.015, spread)
            t = new["T"]["median_ms"]
            s = {"config": config, "tag": "summary", "S_ms": [a1["S"]["median_ms"], a2["S"]["median_ms"]], "S_spread": spread, "T_ms": t,
                 "T_vs_S": t / s_ms - 1.0, "T_bar": bar, "T_holds": t <= s_ms * (1.0 + bar),
                 "mismatches_against_the_per_light_traces": new["mismatches_against_the_per_light_traces"]}
            for name in LISTS:
                for f in ("", "f"):
                    key = name + f
                    a = 0.5 * (a1["A_" + key]["median_ms"] + a2["A_" + key]["median_ms"])
                    s[key] = {"A_ms": [a1["A_" + key]["median_ms"], a2["A_" + key]["median_ms"]],
                              "L4_ms": new["L4_" + key]["median_ms"], "L1_ms": new["L1_" + key]["median_ms"],
                              "L4_over_A": new["L4_" + key]["median_ms"] / a, "L1_over_A": new["L1_" + key]["median_ms"] / a}
            fh.write(json.dumps(s) + "\n")
            fh.flush()
            print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
