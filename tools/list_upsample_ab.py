"""What a soft light list costs traced at half resolution and upsampled (GPU box), against the PARENT commit's library tracing the
same list at full resolution on the same frames.  DESIGN.md 4.32.

    python tools/list_upsample_ab.py --parent-root <tree of the parent commit, built>
                                     [--direct-lib <librts.so of this tree built with EXTRA=-DRTS_UPSAMPLE_DIRECT>]
                                     [--configs city_4k,courtyard_4k,atrium_1080p] [--out profiles/r37/list_upsample_ab.jsonl]

Rows: lists "4x4" = 4 lights of 4 samples and "2x16" = 2 lights of 16 (tools/soft_list_ab.py: entries), through the facing map.
  "parent": the parent commit's library -- trace_ms: rts_trace_soft_light_list_device at full resolution.
  "this" (and "direct": the same code with the low-resolution window read from the buffers, not staged in LDS), phase (0, 0),
            thresholds cos 0.9 and 0.5 % of the scene's diagonal:
            subsample_ms, retrace_map_ms, upsample_ms, upsample_keep_ms: each new pass alone;  lo_trace_ms: the trace at w x h;
            masked_trace_ms: the full-resolution trace under the retrace map;  trace_ms: this library's full-resolution trace;
            half_ms = subsample + lo_trace + upsample (no retrace: the fallback fills the edges);
            half_retrace_ms = subsample + lo_trace + retrace_map + masked_trace + upsample_keep;
            chain_ms / chain_retrace_ms: the same passes launched back to back and timed as one;
            retraced_share: the share of (pixel, light) pairs of the facing map that the retrace map marks.
            equal_rays: the same with 4 times the samples per light at half resolution (4x4 -> 4 lights of 16 sharing one table range;
            2x16 -> 2 lights of 48, the table's size: 0.75 of the parent's rays, named so in the row).
Each figure: 10 warm-up and 60 timed launches between device events, the median.  Every library runs in a child process of its own,
under its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.  After the rows of a
config: one "ratio" row per list, the sums over the parent's trace.  No threshold: every row is reported."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
LISTS = {"4x4": (4, 4), "2x16": (2, 16)}
EQUAL = {"4x4": (16, "equal"), "2x16": (48, "0.75 of the rays")}


def child(mode, config, root):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import numpy as np
    from raytracedshadows_amd import api, scenes, workloads
    from soft_list_ab import _timed, entries
    wl = workloads.prepare_config(config, cache=True)
    W, H, n = wl.W, wl.H, wl.W * wl.H
    sc = wl.scene
    med = lambda ts: float(np.median(ts))
    diag = float(np.linalg.norm(np.asarray(sc.bbox_max, np.float64) - np.asarray(sc.bbox_min, np.float64)))
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_map, d_counts = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n), ctx.malloc(4 * n)
        api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
        if mode != "parent":
            p = api.UpsampleParams.make(0, 0, 0.9, 0.005 * diag)
            w, h = api.subsampled_size(W, H, 0, 0)
            m = w * h
            d_lpos, d_lnrm, d_lmap, d_lo, d_keep = ctx.malloc(m * 16), ctx.malloc(m * 16), ctx.malloc(m), ctx.malloc(4 * m), ctx.malloc(n)
        table = scenes.jitter_offsets(48, 1.0, 19)
        for name, (count, spp) in LISTS.items():
            lights = api.SoftLightList.make(entries(sc, count, spp), table)
            hard = lights.hard_list()
            api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
            trace = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_map)
            row = {"config": config, "mode": mode, "list": name, "steps": STEPS, "warmup": WARMUP, "W": W, "H": H}
            row["trace_ms"] = med(_timed(ctx, trace, STEPS, WARMUP))
            if mode == "parent":
                print(json.dumps(row), flush=True)
                continue
            sub = lambda: api.subsample_gbuffer_device(ctx, p, d_pos, d_nrm, W, H, d_lpos, d_lnrm, d_lights_map=d_map, d_lo_lights_map=d_lmap)
            rmap = lambda: api.upsample_retrace_map_device(ctx, count, p, d_pos, d_nrm, d_lpos, d_lnrm, W, H, d_keep, d_lights_map=d_map,
                                                           d_lo_lights_map=d_lmap)
            masked = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, d_counts, d_lights_map=d_keep)
            sub(), rmap()
            ctx.synchronize()
            keep, fmap = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            ctx.d2h(keep, d_keep)
            ctx.d2h(fmap, d_map)
            pairs = lambda a: int(sum(((a >> l) & 1).sum(dtype=np.int64) for l in range(count)))
            row["retraced_share"] = pairs(keep) / max(1, pairs(fmap))
            row["subsample_ms"] = med(_timed(ctx, sub, STEPS, WARMUP))
            row["retrace_map_ms"] = med(_timed(ctx, rmap, STEPS, WARMUP))
            row["masked_trace_ms"] = med(_timed(ctx, masked, STEPS, WARMUP))
            for label, lo_lights in (("", lights), ("equal_rays_", None)):
                if lo_lights is None:
                    spp4, what = EQUAL[name]
                    lo_lights = api.SoftLightList.make([(k, xyz, spp4, 0, r) for k, xyz, _, _, r in entries(sc, count, spp)], table)
                    row["equal_rays"] = what
                lo_trace = lambda: ctx.trace_soft_light_list_device(wl.constants, lo_lights, d_lpos, w, h, d_lo, d_lights_map=d_lmap)
                up = lambda: api.upsample_soft_light_list_device(ctx, lo_lights, p, d_pos, d_nrm, d_lpos, d_lnrm, d_lo, W, H, d_counts,
                                                                 d_lights_map=d_map, d_lo_lights_map=d_lmap)
                up_keep = lambda: api.upsample_soft_light_list_device(ctx, lo_lights, p, d_pos, d_nrm, d_lpos, d_lnrm, d_lo, W, H, d_counts,
                                                                      d_lights_map=d_map, d_lo_lights_map=d_lmap, d_keep=d_keep)
                lo_trace()
                row[label + "lo_trace_ms"] = med(_timed(ctx, lo_trace, STEPS, WARMUP))
                row[label + "upsample_ms"] = med(_timed(ctx, up, STEPS, WARMUP))
                row[label + "upsample_keep_ms"] = med(_timed(ctx, up_keep, STEPS, WARMUP))
                row[label + "half_ms"] = row["subsample_ms"] + row[label + "lo_trace_ms"] + row[label + "upsample_ms"]
                row[label + "half_retrace_ms"] = (row["subsample_ms"] + row[label + "lo_trace_ms"] + row["retrace_map_ms"] + row["masked_trace_ms"] +
                                                  row[label + "upsample_keep_ms"])
                row[label + "chain_ms"] = med(_timed(ctx, lambda: (sub(), lo_trace(), up()), STEPS, WARMUP))
                # (the masked trace of the full-resolution list: at equal rays the retraced pixels take the list's own samples per light)
                row[label + "chain_retrace_ms"] = med(_timed(ctx, lambda: (sub(), lo_trace(), rmap(), masked(), up_keep()), STEPS, WARMUP))
            print(json.dumps(row), flush=True)


def ratios(rows, config):
    out = []
    for name in LISTS:
        pick = lambda mode, key: next((r[key] for r in rows if r["config"] == config and r["list"] == name and r["mode"] == mode and key in r), None)
        base = pick("parent", "trace_ms")
        if base is None:
            continue
        for mode in ("this", "direct"):
            if pick(mode, "half_ms") is None:
                continue
            r = {"config": config, "mode": "ratio", "of": mode, "list": name, "parent_trace_ms": base,
                 "own_trace_over_parent": pick(mode, "trace_ms") / base, "retraced_share": pick(mode, "retraced_share")}
            for key in ("half_ms", "half_retrace_ms", "chain_ms", "chain_retrace_ms", "equal_rays_half_ms", "equal_rays_half_retrace_ms",
                        "equal_rays_chain_ms", "equal_rays_chain_retrace_ms"):
                r[key[:-3] + "_over_parent"] = pick(mode, key) / base
            out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--direct-lib", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r37/list_upsample_ab.jsonl")
    ap.add_argument("--child", nargs=3, metavar=("MODE", "CONFIG", "ROOT"))
    args = ap.parse_args()
    if args.child:
        return child(*args.child)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        def emit(line):
            out.write(line + "\n")
            out.flush()
            print(line, flush=True)
        for config in args.configs.split(","):
            runs = [("this", ROOT, "")]
            if args.direct_lib:
                runs.append(("direct", ROOT, os.path.abspath(args.direct_lib)))
            if args.parent_root:
                runs.insert(0, ("parent", os.path.abspath(args.parent_root), ""))
            rows = []
            for mode, root, lib in runs:
                env = dict(os.environ)
                env.pop("RTS_LIB", None)
                if lib:
                    env["RTS_LIB"] = lib
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root], env=env, capture_output=True,
                                     text=True, timeout=400)
                if run.returncode != 0:
                    sys.exit(f"list_upsample_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                for line in run.stdout.splitlines():
                    if line.startswith("{"):
                        rows.append(json.loads(line))
                        emit(line)
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
