"""What a per-pixel jitter table costs an adaptive soft light list dispatch, and what it buys (GPU box) -- DESIGN.md 4.19.

    python tools/soft_list_jitter_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,courtyard_4k,atrium_1080p]
                                        [--out profiles/r21/soft_list_jitter_ab.jsonl]

Lists and probes as in tools/soft_list_adaptive_ab.py ("4x4" with probe 2, "2x16" with probes 2 and 4), no light map, the untuned
default launch ("kernel" -1, "soft_split" 1).  n = the samples of every light of the list.  Variants:
    A     ONE adaptive list trace without tables, the parent commit's library            (twice, before and after: its spread is the yardstick)
    A1    one jittered adaptive soft mask trace per light (table 2n), the parent's library (twice)
    P     ONE plain soft light list trace, the parent's library                          (twice)
    B0    this commit, tables all 0                                                      (the same kernel as A: within A's spread)
    Bn    this commit, every table n                                                     (every sample, the start hashed)
    B2n   this commit, every table 2n                                                    (n of 2n entries)
    C     this commit, probes all 0 with every table 2n                                  (the full jittered list trace; against P)
Every variant: 10 warm-up and 100 timed launches between device events, the median reported; this commit's variants alternate in four
rounds.  The parent's and this commit's variants run in child processes of this tool (a fresh process per library, each under its own
time limit; this process never opens the GPU).  The tool stops at the first child that fails.  Quality, on the device results of this
commit at the size timed: the share of (pixel, light) bytes in which the adaptive jittered list (tables 2n, and n) differs from the
FULL jittered list trace (probes 0, the same tables), beside the share in which the untabled adaptive list differs from its own full
trace."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from soft_list_ab import LISTS, _timed, entries  # noqa: E402

CASES = [("4x4", 2), ("2x16", 2), ("2x16", 4)]           # (list, the probe of every light)
STEPS, WARMUP, ROUNDS = 100, 10, 4


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
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_counts, d_full, d_ref = ctx.malloc(wl.positions.nbytes), ctx.malloc(8 * W * H), ctx.malloc(8 * W * H), ctx.malloc(W * H)
        d_masks = [ctx.malloc(W * H) for _ in range(4)]
        ctx.h2d(d_pos, wl.positions)
        out, names, cases = {}, {}, {}
        for name, (count, samples) in LISTS.items():
            es = entries(wl.scene, count, samples)
            # the derived lights with a table of 2n, written out (the parent's SoftLightList.light has no table argument)
            ones = [api.Light.make(kind, xyz, np.float32(radius) * table[first:first + 2 * n, :3], nsamples=n) for kind, xyz, n, first, radius in es]
            cases[name] = (samples, ones, api.SoftLightList.make(es, table))
        if mode == "parent":
            for name, k in CASES:
                n, ones, lights = cases[name]
                key = "%s_k%d" % (name, k)
                out["A_" + key] = _timed(ctx, lambda: ctx.trace_soft_light_list_adaptive_device(
                    wl.constants, lights, (k,) * lights.count, d_pos, W, H, d_counts, d_refined=d_ref), STEPS, WARMUP)
                names["A_" + key] = ctx.last_kernel_name()

                def per_light():
                    for l, one in enumerate(ones):
                        ctx.trace_shadow_mask_adaptive_device(wl.constants, d_pos, W, H, d_masks[l], one, k)
                out["A1_" + key] = _timed(ctx, per_light, STEPS, WARMUP)
                names["A1_" + key] = ctx.last_kernel_name()
            for name in LISTS:
                lights = cases[name][2]
                out["P_" + name] = _timed(ctx, lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts), STEPS, WARMUP)
                names["P_" + name] = ctx.last_kernel_name()
        else:
            def jittered(lights, k, T):
                probes, tables = (k,) * lights.count, (T,) * lights.count
                return lambda: ctx.trace_soft_light_list_adaptive_device(wl.constants, lights, probes, d_pos, W, H, d_counts, d_refined=d_ref,
                                                                         tables=tables)
            for r in range(ROUNDS):
                for name, k in CASES:
                    n, ones, lights = cases[name]
                    for v, T in (("B0", 0), ("Bn", n), ("B2n", 2 * n)):
                        key = "%s_%s_k%d" % (v, name, k)
                        out.setdefault(key, []).extend(_timed(ctx, jittered(lights, k, T), STEPS // ROUNDS, WARMUP // ROUNDS + 1))
                        names[key] = ctx.last_kernel_name()
                for name in LISTS:
                    n, ones, lights = cases[name]
                    out.setdefault("C_" + name, []).extend(_timed(ctx, jittered(lights, 0, 2 * n), STEPS // ROUNDS, WARMUP // ROUNDS + 1))
                    names["C_" + name] = ctx.last_kernel_name()

            def planes(lights, k, T):
                jittered(lights, k, T)()
                ctx.synchronize()
                c = np.empty((8, H, W), np.uint8)
                ctx.d2h(c, d_counts)
                return c[:lights.count]
            quality = {}
            for name, k in CASES:
                n, ones, lights = cases[name]
                pairs = float(lights.count * W * H)
                quality["%s_k%d" % (name, k)] = {
                    "untabled_differs_from_its_full_trace": float((planes(lights, k, 0) != planes(lights, 0, 0)).sum()) / pairs,
                    "table_n_differs_from_its_full_trace": float((planes(lights, k, n) != planes(lights, 0, n)).sum()) / pairs,
                    "table_2n_differs_from_its_full_trace": float((planes(lights, k, 2 * n) != planes(lights, 0, 2 * n)).sum()) / pairs}
            row["quality"] = quality
        row["kernel_names"] = names
        row.update({v: {"median_ms": float(np.median(ts)), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts))} for v, ts in out.items()})
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r21/soft_list_jitter_ab.jsonl")
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=150, help="limit of a child, seconds")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.config, os.path.abspath(args.root))
    parent = os.path.abspath(args.parent_root)
    if not os.path.exists(os.path.join(parent, "raytracedshadows_amd", "librts.so")):
        sys.exit(f"soft_list_jitter_ab: no built library under {parent} (export the parent commit there and build it)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k != "RTS_LIB"}
    with open(args.out, "a") as fh:
        for config in args.configs.split(","):
            rows = {}
            for tag, mode, root in (("parent1", "parent", parent), ("new", "variants", ROOT), ("parent2", "parent", parent)):
                t0 = time.time()
                cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--child", mode,
                       "--config", config, "--root", root]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True)
                line = next((l for l in p.stdout.splitlines() if l.startswith("ROW ")), None)
                if p.returncode != 0 or line is None:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    sys.exit(f"soft_list_jitter_ab: {config} {tag} failed (exit {p.returncode}); nothing more is started")
                rows[tag] = json.loads(line[4:])
                rows[tag]["tag"] = tag
                rows[tag]["child_wall_s"] = round(time.time() - t0, 1)
                fh.write(json.dumps(rows[tag]) + "\n")
                fh.flush()
            p1, p2, new = rows["parent1"], rows["parent2"], rows["new"]
            both = lambda v: 0.5 * (p1[v]["median_ms"] + p2[v]["median_ms"])
            s = {"config": config, "tag": "summary", "quality": new["quality"]}
            for name, k in CASES:
                key = "%s_k%d" % (name, k)
                a, a1 = both("A_" + key), both("A1_" + key)
                b = {v: new["%s_%s" % (v, key)]["median_ms"] for v in ("B0", "Bn", "B2n")}
                s[key] = {"A_ms": [p1["A_" + key]["median_ms"], p2["A_" + key]["median_ms"]],
                          "A1_ms": [p1["A1_" + key]["median_ms"], p2["A1_" + key]["median_ms"]],
                          "A_spread": abs(p1["A_" + key]["median_ms"] - p2["A_" + key]["median_ms"]) / a,
                          "B0_ms": b["B0"], "Bn_ms": b["Bn"], "B2n_ms": b["B2n"], "B0_over_A": b["B0"] / a, "Bn_over_A": b["Bn"] / a,
                          "B2n_over_A": b["B2n"] / a, "B2n_over_A1": b["B2n"] / a1}
            for name in LISTS:
                s["C_" + name] = {"P_ms": [p1["P_" + name]["median_ms"], p2["P_" + name]["median_ms"]], "C_ms": new["C_" + name]["median_ms"],
                                  "C_over_P": new["C_" + name]["median_ms"] / both("P_" + name)}
            fh.write(json.dumps(s) + "\n")
            fh.flush()
            print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
