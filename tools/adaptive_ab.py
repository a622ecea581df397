"""What adaptive soft shadows gain and cost (GPU box): the soft mask trace of the parent commit's library, plain and through the facing
map, against this commit's adaptive trace with a probe of 4 and of 2 samples, on the same frame under 16 point-light samples with and
without a 16-entry per-pixel table -- DESIGN.md 4.16.

    python tools/adaptive_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,courtyard_4k,atrium_1080p] [--out profiles/r17/adaptive_ab.jsonl]

Variants, per table (0: every pixel the same 16 offsets in the same order; 16: the same offsets, the start hashed per pixel), all at the
untuned default launch ("kernel" -1, no split table or order):
    A     soft mask trace, the parent commit's library            (twice, before and after: its own spread is the yardstick)
    A'    the same through the facing active map                  (parent commit's library)
    B     soft mask trace, this commit                            (no mask kernel changed: within max(1.5 %, spread) of A)
    P4, P2        adaptive trace, probe 4 / 2, "soft_split" 1     (four waves per tile)
    P4s0, P2s0    the same with "soft_split" 0                    (one wave per tile)
    P4f, P2f, P4fs0, P2fs0   the four through the facing map
Every variant: 20 warm-up and 200 timed launches between device events, the median reported.  The parent's and this commit's variants
run in child processes of this tool (a fresh process per library, each under its own time limit; this process never opens the GPU),
this commit's variants alternating inside one child in four rounds of 50 (5 warm-up launches each).  The tool stops at the first
child that fails.  Beside the times: the share of refined pixels, the share of pixels whose byte differs from the full trace's (the
quality cost, from the GPU's own two results), the identity mask == full count on refined pixels, and a parity count against the host
twin at the size timed (under the table)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, ROUNDS = 200, 20, 4
SAMPLES, TABLES, PROBES = 16, (0, 16), (4, 2)


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


def _light(workloads, wl, table):
    """16 samples of a light of 1 % of the scene's diagonal (the soft16 configs); table 16: the same offsets, hashed start."""
    whole = workloads.relight(wl, "point", SAMPLES, 0.01, 0).light
    lt = type(whole).from_buffer_copy(whole)
    lt.table = table
    return lt


def child(mode, config, root):
    sys.path.insert(0, root)
    import numpy as np
    from raytracedshadows_amd import api, workloads
    assert os.path.abspath(api.lib_path()).startswith(os.path.abspath(root)), api.lib_path()
    wl = workloads.prepare_config(config, cache=True)
    W, H = wl.W, wl.H
    row = {"config": config, "mode": mode, "lib": "this commit" if os.path.abspath(root) == ROOT else "parent commit", "steps": STEPS,
           "warmup": WARMUP, "samples": SAMPLES}
    med = lambda ts: float(np.median(ts))
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_mask, d_facing = ctx.malloc(wl.positions.nbytes), ctx.malloc(W * H), ctx.malloc(W * H)
        ctx.h2d(d_pos, wl.positions)
        pos, nrm, _ = api.primary_gbuffer(wl.packed, wl.scene.eye, wl.scene.target, wl.scene.fovy, W, H)
        for table in TABLES:
            light = _light(workloads, wl, table)
            facing = api.facing_active(wl.constants, light, pos, nrm)
            ctx.h2d(d_facing, facing)
            plain = lambda a=None: (lambda: ctx.trace_shadow_mask_device(wl.constants, d_pos, W, H, d_mask, light=light, d_active=a))
            out, res = {}, {"inactive_pixel_share": float(1.0 - (facing != 0).mean())}
            if mode == "parent":
                out["A"] = _timed(ctx, plain(), STEPS, WARMUP)
                res["kernel_name"] = ctx.last_kernel_name()
                out["A'"] = _timed(ctx, plain(d_facing), STEPS, WARMUP)
            else:
                d_m2, d_ref = ctx.malloc(W * H), ctx.malloc(W * H)
                adaptive = lambda probe, a: (lambda: ctx.trace_shadow_mask_adaptive_device(wl.constants, d_pos, W, H, d_m2, light, probe,
                                                                                           d_refined=d_ref, d_active=a))
                launches = {"B": (1, plain())}
                for probe in PROBES:
                    for f, a in (("", None), ("f", d_facing)):
                        launches["P%d%s" % (probe, f)] = (1, adaptive(probe, a))
                        launches["P%d%ss0" % (probe, f)] = (0, adaptive(probe, a))
                names = {}
                for r in range(ROUNDS):                  # alternating: B P4 P4s0 P4f ... B P4 ...; 20 warm-up launches per variant in all
                    for v, (split, launch) in launches.items():
                        ctx.set_option("soft_split", split)
                        out.setdefault(v, []).extend(_timed(ctx, launch, STEPS // ROUNDS, WARMUP // ROUNDS))
                        names[v] = ctx.last_kernel_name()
                res["kernel_names"] = names
                # the shares and the identity, from the GPU's own results; both splits must agree byte for byte
                full, m, rf, m0, rf0 = (np.empty((H, W), np.uint8) for _ in range(5))
                for f, a, act in (("", None, None), ("f", d_facing, facing)):
                    ctx.set_option("soft_split", 1)
                    plain(a)()
                    ctx.synchronize()
                    ctx.d2h(full, d_mask)
                    for probe in PROBES:
                        adaptive(probe, a)()
                        ctx.synchronize()
                        ctx.d2h(m, d_m2); ctx.d2h(rf, d_ref)
                        ctx.set_option("soft_split", 0)
                        adaptive(probe, a)()
                        ctx.synchronize()
                        ctx.d2h(m0, d_m2); ctx.d2h(rf0, d_ref)
                        ctx.set_option("soft_split", 1)
                        res["shares_P%d%s" % (probe, f)] = {
                            "refined_share": float((rf == 1).mean()), "differs_from_full_share": float((m != full).mean()),
                            "mean_abs_count_error": float(np.abs(m.astype(np.int32) - full.astype(np.int32)).mean()),
                            "refined_pixels_unequal_to_full": int((m[rf == 1] != full[rf == 1]).sum()),
                            "unrefined_pixels_not_0_or_n": int((~np.isin(m[rf == 0], (0, SAMPLES))).sum()),
                            "split_1_vs_0_mismatches": int((m != m0).sum()) + int((rf != rf0).sum())}
                        if not f and table:              # parity with the host twin at the size timed (under the table)
                            hm, hr = api.shadow_mask_adaptive(wl.packed, wl.constants, light, wl.positions, W, H, probe)
                            res["shares_P%d" % probe]["host_twin_mismatches"] = int((hm != m).sum()) + int((hr != rf).sum())
                    res["full%s_penumbra_share" % f] = float(((full > 0) & (full < SAMPLES)).mean())
                ctx.free(d_m2); ctx.free(d_ref)
            res.update({v: {"median_ms": med(ts), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts))} for v, ts in out.items()})
            row["table_%d" % table] = res
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r17/adaptive_ab.jsonl")
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=480)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.config, os.path.abspath(args.root))
    parent = os.path.abspath(args.parent_root)
    if not os.path.exists(os.path.join(parent, "raytracedshadows_amd", "librts.so")):
        sys.exit(f"adaptive_ab: no built library under {parent} (export the parent commit there and build it)")
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
                    sys.exit(f"adaptive_ab: {config} {tag} failed (exit {p.returncode}); nothing more is started")
                rows[tag] = json.loads(line[4:])
                rows[tag]["tag"] = tag
                fh.write(json.dumps(rows[tag]) + "\n")
                fh.flush()
            for table in TABLES:
                t = "table_%d" % table
                a1, a2, new = rows["A1"][t], rows["A2"][t], rows["new"][t]
                a = 0.5 * (a1["A"]["median_ms"] + a2["A"]["median_ms"])
                af = 0.5 * (a1["A'"]["median_ms"] + a2["A'"]["median_ms"])
                spread = abs(a1["A"]["median_ms"] - a2["A"]["median_ms"]) / a
                bar = max(0.015, spread)
                b = new["B"]["median_ms"]
                s = {"config": config, "tag": "summary", "table": table, "A_ms": [a1["A"]["median_ms"], a2["A"]["median_ms"]],
                     "A_facing_ms": [a1["A'"]["median_ms"], a2["A'"]["median_ms"]], "A_spread": spread, "B_ms": b, "B_vs_A": b / a - 1.0,
                     "B_bar": bar, "B_holds": b <= a * (1.0 + bar), "inactive_pixel_share": new["inactive_pixel_share"],
                     "full_penumbra_share": new["full_penumbra_share"], "kernel_names": new["kernel_names"]}
                for v in new["kernel_names"]:
                    if v == "B":
                        continue
                    ms = new[v]["median_ms"]
                    s[v] = {"ms": ms, "over_A": ms / a, "over_A_facing": ms / af}
                for probe in PROBES:
                    for f in ("", "f"):
                        s["P%d%s" % (probe, f)].update(new["shares_P%d%s" % (probe, f)])
                fh.write(json.dumps(s) + "\n")
                fh.flush()
                print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
