"""What ONE adaptive soft light list dispatch costs against the parent commit's two ways to trace the same lights (GPU box): its full
soft light list trace, and one adaptive soft mask trace per light; and the plain soft mask trace of this commit against the parent
commit's library -- DESIGN.md 4.18.

    python tools/soft_list_adaptive_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,courtyard_4k,atrium_1080p]
                                          [--out profiles/r20/soft_list_adaptive_ab.jsonl]

Lists as in tools/soft_list_ab.py ("4x4" = 4 lights of 4 samples, "2x16" = 2 lights of 16, the radius 1 % of the scene's diagonal),
each with the probes of CASES: 2 for the lights of 4, 2 and 4 for the lights of 16; each without a map and ("f") through the facing
map.  Variants, all at the untuned default launch ("kernel" -1, no split table or order):
    S     plain soft mask trace, 16 samples, the parent commit's library     (twice, before and after: its own spread is the yardstick)
    A     ONE soft light list trace, the parent commit's library             (twice; every sample of every light)
    A2    one adaptive soft mask trace per light, the parent commit's library (twice; "f": each light through its own facing mark)
    T     plain soft mask trace, 16 samples, this commit                     (no mask kernel changed: within max(1.5 %, spread) of S)
    B4    ONE adaptive list trace, "soft_split" 1                            (four waves per tile)
    B1    the same with "soft_split" 0                                       (one wave per tile)
Every variant: 20 warm-up and 200 timed launches (of all the lights' traces, for A2) between device events, the median reported.  The
parent's and this commit's variants run in child processes of this tool (a fresh process per library, each under its own time limit;
this process never opens the GPU), this commit's variants alternating inside one child in four rounds of 50 (5 warm-up launches each).
The tool stops at the first child that fails.  Beside the times, in a fourth child with a limit of its own (the host twin at 4K is the
slow part), at the size timed: both splits' planes and refined plane against the host twin, byte for byte; the share of (pixel,
light) pairs refined; and the share whose byte differs from this commit's full list trace -- the quality cost."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from soft_list_ab import LISTS, ROUNDS, STEPS, WARMUP, _timed, entries  # noqa: E402

CASES = [("4x4", 2), ("2x16", 2), ("2x16", 4)]           # (list, the probe of every light)


def child(mode, config, root, twin_threads):
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
        d_counts, d_full, d_ref = ctx.malloc(8 * W * H), ctx.malloc(8 * W * H), ctx.malloc(W * H)
        out, names = {}, {}
        cases = {}
        for name, (count, samples) in LISTS.items():
            es = entries(wl.scene, count, samples)
            ones = [api.Light.make(kind, xyz, np.float32(radius) * table[first:first + n, :3]) for kind, xyz, n, first, radius in es]
            cases[name] = (es, ones, api.SoftLightList.make(es, table))

        def facing_maps(es, ones):
            hard = api.LightList.make([(kind, xyz) for kind, xyz, _, _, _ in es])
            api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
            for l, one in enumerate(ones):
                api.facing_active_device(ctx, wl.constants, one, d_pos, d_nrm, W, H, d_acts[l])
            ctx.synchronize()

        if mode == "parent":
            out["S"] = _timed(ctx, plain, STEPS, WARMUP)
            names["S"] = ctx.last_kernel_name()
            for name, (es, ones, lights) in cases.items():
                facing_maps(es, ones)
                for f in ("", "f"):
                    full = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_map if f else None)
                    out["A_%s%s" % (name, f)] = _timed(ctx, full, STEPS, WARMUP)
                    names["A_%s%s" % (name, f)] = ctx.last_kernel_name()
                    for case, k in CASES:
                        if case != name:
                            continue

                        def per_light():
                            for l, one in enumerate(ones):
                                ctx.trace_shadow_mask_adaptive_device(wl.constants, d_pos, W, H, d_masks[l], one, k,
                                                                      d_active=d_acts[l] if f else None)
                        v = "A2_%s_k%d%s" % (name, k, f)
                        out[v] = _timed(ctx, per_light, STEPS, WARMUP)
                        names[v] = ctx.last_kernel_name()

        def adaptive(lights, k, f):
            probes = (k,) * lights.count
            return lambda: ctx.trace_soft_light_list_adaptive_device(wl.constants, lights, probes, d_pos, W, H, d_counts, d_refined=d_ref,
                                                                     d_lights_map=d_map if f else None)
        if mode == "variants":
            for r in range(ROUNDS):                      # alternating: T, then per case B4 B1 B4f B1f; 20 warm-up launches per variant in all
                ctx.set_option("soft_split", 1)
                out.setdefault("T", []).extend(_timed(ctx, plain, STEPS // ROUNDS, WARMUP // ROUNDS))
                names["T"] = ctx.last_kernel_name()
                for name, k in CASES:
                    es, ones, lights = cases[name]
                    facing_maps(es, ones)
                    for f in ("", "f"):
                        for split in (1, 0):
                            v = "B%d_%s_k%d%s" % (4 if split else 1, name, k, f)
                            ctx.set_option("soft_split", split)
                            out.setdefault(v, []).extend(_timed(ctx, adaptive(lights, k, f), STEPS // ROUNDS, WARMUP // ROUNDS))
                            names[v] = ctx.last_kernel_name()
        if mode == "parity":
            # at the size that was timed: both splits against the host twin; the shares refined and differing from the full list trace
            parity, shares = {}, {}
            m = np.empty((H, W), np.uint8)
            for name, k in CASES:
                es, ones, lights = cases[name]
                n = lights.count
                facing_maps(es, ones)
                ctx.d2h(m, d_map)
                for f in ("", "f"):
                    key = "%s_k%d%s" % (name, k, f)
                    want_c, want_r = api.soft_light_list_adaptive(wl.packed, wl.constants, lights, (k,) * n, wl.positions, W, H,
                                                                  lights_map=m if f else None, threads=twin_threads)
                    ctx.set_option("soft_split", 1)
                    ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_full, d_lights_map=d_map if f else None)
                    ctx.synchronize()
                    full = np.empty((8, H, W), np.uint8)
                    ctx.d2h(full, d_full)
                    bad = 0
                    for split in (1, 0):
                        ctx.set_option("soft_split", split)
                        adaptive(lights, k, f)()
                        ctx.synchronize()
                        planes, ref = np.empty((8, H, W), np.uint8), np.empty((H, W), np.uint8)
                        ctx.d2h(planes, d_counts)
                        ctx.d2h(ref, d_ref)
                        bad += int((planes[:n] != want_c).sum()) + int((ref != want_r).sum())
                    parity[key] = bad
                    marked = float(n * W * H) if not f else float(sum(int(((m >> l) & 1).sum()) for l in range(n)))
                    took = sum(int(((want_r >> l) & 1).sum()) for l in range(n))
                    shares[key] = {"refined_share_of_pixel_light_pairs": took / float(n * W * H),
                                   "refined_share_of_marked_pairs": took / max(1.0, marked),
                                   "differs_from_the_full_list_trace": float((want_c != full[:n]).sum()) / float(n * W * H)}
            row["mismatches_against_the_twin"] = parity
            row["shares"] = shares
        row["kernel_names"] = names
        row.update({v: {"median_ms": med(ts), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts))} for v, ts in out.items()})
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r20/soft_list_adaptive_ab.jsonl")
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=120, help="limit of a timing child, seconds (the slowest measured: courtyard_4k, 23 s)")
    ap.add_argument("--parity-timeout", type=int, default=120, help="limit of the parity child, seconds (the slowest measured: courtyard_4k, 16 s)")
    ap.add_argument("--twin-threads", type=int, default=16)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.config, os.path.abspath(args.root), args.twin_threads)
    parent = os.path.abspath(args.parent_root)
    if not os.path.exists(os.path.join(parent, "raytracedshadows_amd", "librts.so")):
        sys.exit(f"soft_list_adaptive_ab: no built library under {parent} (export the parent commit there and build it)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    env = {k: v for k, v in os.environ.items() if k != "RTS_LIB"}
    with open(args.out, "a") as fh:
        for config in args.configs.split(","):
            rows = {}
            for tag, mode, root in (("A1", "parent", parent), ("new", "variants", ROOT), ("A2", "parent", parent), ("parity", "parity", ROOT)):
                limit = args.parity_timeout if mode == "parity" else args.child_timeout
                t0 = time.time()
                cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", mode,
                       "--config", config, "--root", root, "--twin-threads", str(args.twin_threads)]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True)
                line = next((l for l in p.stdout.splitlines() if l.startswith("ROW ")), None)
                if p.returncode != 0 or line is None:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    sys.exit(f"soft_list_adaptive_ab: {config} {tag} failed (exit {p.returncode}); nothing more is started")
                rows[tag] = json.loads(line[4:])
                rows[tag]["tag"] = tag
                rows[tag]["child_wall_s"] = round(time.time() - t0, 1)
                fh.write(json.dumps(rows[tag]) + "\n")
                fh.flush()
            a1, a2, new, par = rows["A1"], rows["A2"], rows["new"], rows["parity"]
            both = lambda v: 0.5 * (a1[v]["median_ms"] + a2[v]["median_ms"])
            s_ms = both("S")
            spread = abs(a1["S"]["median_ms"] - a2["S"]["median_ms"]) / s_ms
            bar = max(0.015, spread)
            t = new["T"]["median_ms"]
            s = {"config": config, "tag": "summary", "S_ms": [a1["S"]["median_ms"], a2["S"]["median_ms"]], "S_spread": spread, "T_ms": t,
                 "T_vs_S": t / s_ms - 1.0, "T_bar": bar, "T_holds": t <= s_ms * (1.0 + bar),
                 "mismatches_against_the_twin": par["mismatches_against_the_twin"], "shares": par["shares"],
                 "child_wall_s": {t: rows[t]["child_wall_s"] for t in rows}}
            for name, k in CASES:
                for f in ("", "f"):
                    key, a, aa = "%s_k%d%s" % (name, k, f), "A_%s%s" % (name, f), "A2_%s_k%d%s" % (name, k, f)
                    b4, b1 = new["B4_" + key]["median_ms"], new["B1_" + key]["median_ms"]
                    s[key] = {"A_ms": [a1[a]["median_ms"], a2[a]["median_ms"]], "A2_ms": [a1[aa]["median_ms"], a2[aa]["median_ms"]],
                              "B4_ms": b4, "B1_ms": b1, "B4_over_A": b4 / both(a), "B1_over_A": b1 / both(a),
                              "B4_over_A2": b4 / both(aa), "B1_over_A2": b1 / both(aa)}
            fh.write(json.dumps(s) + "\n")
            fh.flush()
            print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
