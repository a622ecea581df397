"""What one soft light list distance dispatch costs against one soft distance dispatch per light, and against the soft light list
without distances (GPU box): point lights on a ring around the scene's light, each of several samples, on the same frame -- DESIGN.md 4.20.

    python tools/soft_list_distance_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,courtyard_4k,atrium_1080p]
                                          [--out profiles/r23/soft_list_distance_ab.jsonl]

Lists (tools/soft_list_ab.py: entries): "4x4" = 4 lights of 4 samples, "2x16" = 2 lights of 16, every light its own range of one
48-entry table, the radius 1 % of the scene's diagonal; each without a map and ("f") through the facing map.  Variants, all at the
untuned default launch ("kernel" -1, no split table or order):
    S     plain soft mask trace, 16 samples, the parent commit's library   (twice, before and after: its own spread is the yardstick)
    A     one rts_trace_soft_distance_device per light, distance and mask, the parent commit's library   (twice; the baseline)
    T     plain soft mask trace, 16 samples, this commit                   (no mask kernel changed: within max(1.5 %, spread) of S)
    B4    ONE list distance trace, distances and counts, "soft_split" 1    (four waves per tile, the pairs dealt over them)
    B1    the same with "soft_split" 0                                     (one wave walks every pair)
    C     this commit's rts_trace_soft_light_list_device on the same list, "soft_split" 1: counts alone, every walk ending at its
          first hit -- B / C is what the distances cost
Every variant: 20 warm-up and 200 timed launches (of all the lights' traces, for A) between device events, the median reported.  The
parent's and this commit's variants run in child processes of this tool (a fresh process per library, each under its own time limit;
this process never opens the GPU), this commit's variants alternating inside one child in four rounds of 50 (5 warm-up launches each).
The tool stops at the first child that fails.  Beside the times: both outputs of both list distance traces against the per-light
traces of the same process, bit for bit, at the size timed."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from soft_list_ab import LISTS, ROUNDS, STEPS, WARMUP, _timed, entries  # noqa: E402


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
        d_acts, d_masks, d_dists = ([ctx.malloc(W * H) for _ in range(4)], [ctx.malloc(W * H) for _ in range(4)],
                                    [ctx.malloc(W * H * 4) for _ in range(4)])
        out, names, cases = {}, {}, {}
        for name, (count, samples) in LISTS.items():
            es = entries(wl.scene, count, samples)
            # the derived lights (include/rts.h), made here so that the parent commit's library can trace them: radius * table[first + j]
            ones = [api.Light.make(kind, xyz, np.float32(radius) * table[first:first + n, :3]) for kind, xyz, n, first, radius in es]
            cases[name] = (es, ones)

        def per_light(ones, facing):
            def run():
                for l, one in enumerate(ones):
                    ctx.trace_soft_distance_device(wl.constants, d_pos, W, H, d_dists[l], d_masks[l], light=one,
                                                   d_active=d_acts[l] if facing else None)
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
            d_planes, d_counts = ctx.malloc(8 * W * H * 4), ctx.malloc(8 * W * H)
            for r in range(ROUNDS):                      # alternating: T, then per list B4 B1 C, without and with the map
                ctx.set_option("soft_split", 1)
                out.setdefault("T", []).extend(_timed(ctx, plain, STEPS // ROUNDS, WARMUP // ROUNDS))
                names["T"] = ctx.last_kernel_name()
                for name, (es, ones) in cases.items():
                    lights = api.SoftLightList.make(es, table)
                    facing_maps(es, ones)
                    for f in ("", "f"):
                        dist = lambda: ctx.trace_soft_light_list_distance_device(wl.constants, lights, d_pos, W, H, d_planes, d_counts,
                                                                                 d_lights_map=d_map if f else None)
                        counts = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts,
                                                                          d_lights_map=d_map if f else None)
                        for v, split, launch in (("B4", 1, dist), ("B1", 0, dist), ("C", 1, counts)):
                            v = "%s_%s%s" % (v, name, f)
                            ctx.set_option("soft_split", split)
                            out.setdefault(v, []).extend(_timed(ctx, launch, STEPS // ROUNDS, WARMUP // ROUNDS))
                            names[v] = ctx.last_kernel_name()
            # parity at the size that was timed: both outputs of both list distance traces against each light's own soft distance trace
            ctx.set_option("soft_split", 1)
            parity = {}
            for name, (es, ones) in cases.items():
                lights = api.SoftLightList.make(es, table)
                facing_maps(es, ones)
                for f in ("", "f"):
                    per_light(ones, bool(f))()
                    ctx.synchronize()
                    want_d, want_c = np.empty((len(ones), H, W), np.uint32), np.empty((len(ones), H, W), np.uint8)
                    one_d, one_c = np.empty((H, W), np.uint32), np.empty((H, W), np.uint8)
                    for l in range(len(ones)):
                        ctx.d2h(one_d, d_dists[l])
                        ctx.d2h(one_c, d_masks[l])
                        want_d[l], want_c[l] = one_d, one_c
                    bad = 0
                    for split in (1, 0):
                        ctx.set_option("soft_split", split)
                        ctx.trace_soft_light_list_distance_device(wl.constants, lights, d_pos, W, H, d_planes, d_counts,
                                                                  d_lights_map=d_map if f else None)
                        ctx.synchronize()
                        got_d, got_c = np.empty((8, H, W), np.uint32), np.empty((8, H, W), np.uint8)
                        ctx.d2h(got_d, d_planes)
                        ctx.d2h(got_c, d_counts)
                        bad += int((got_d[:len(ones)] != want_d).sum()) + int((got_c[:len(ones)] != want_c).sum())
                    parity["%s%s" % (name, f)] = bad
            row["mismatches_against_the_per_light_traces"] = parity
        row["kernel_names"] = names
        row.update({v: {"median_ms": med(ts), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts))} for v, ts in out.items()})
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r23/soft_list_distance_ab.jsonl")
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=420)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.config, os.path.abspath(args.root))
    parent = os.path.abspath(args.parent_root)
    if not os.path.exists(os.path.join(parent, "raytracedshadows_amd", "librts.so")):
        sys.exit(f"soft_list_distance_ab: no built library under {parent} (export the parent commit there and build it)")
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
                    sys.exit(f"soft_list_distance_ab: {config} {tag} failed (exit {p.returncode}); nothing more is started")
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
                    b4, b1, c = (new[v + "_" + key]["median_ms"] for v in ("B4", "B1", "C"))
                    s[key] = {"A_ms": [a1["A_" + key]["median_ms"], a2["A_" + key]["median_ms"]], "B4_ms": b4, "B1_ms": b1, "C_ms": c,
                              "B4_over_A": b4 / a, "B1_over_A": b1 / a, "B4_over_C": b4 / c, "B1_over_C": b1 / c}
            fh.write(json.dumps(s) + "\n")
            fh.flush()
            print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
