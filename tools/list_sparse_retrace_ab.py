"""What the retrace of a half-resolution soft light list costs through the compacted list of its pixels (GPU box), against the PARENT
commit's library tracing the same retrace map with the masked block trace.  DESIGN.md 4.33.

    python tools/list_sparse_retrace_ab.py --parent-root <tree of the parent commit, built>
                                           [--configs city_4k,courtyard_4k,atrium_1080p] [--out profiles/r38/list_sparse_retrace_ab.jsonl]

Rows: the six of DESIGN.md 4.32's table -- lists "4x4" = 4 lights of 4 samples and "2x16" = 2 lights of 16 (tools/soft_list_ab.py:
entries) through the facing map, phase (0, 0), thresholds cos 0.9 and 0.5 % of the scene's diagonal: the same retrace maps.
  "parent": the parent commit's library --
            masked_trace_ms (a): rts_trace_soft_light_list_device at full resolution under the retrace map;
            retrace_map_ms, lo_trace_ms: the passes around it;  chain_retrace_ms (e): subsample, trace at w x h, retrace map, masked
            trace, upsample with keep, launched back to back and timed as one.
  "this":   masked_trace_ms (a again, this library's: the kernel's text is the parent's);  compact_ms (b): rtsh_compact_light_map_device
            alone;  sparse_trace_ms (c): rts_trace_soft_light_list_sparse_device alone over the compacted list, capacity W * H;
            compact_sparse_ms (d) = (b) + (c);  chain_retrace_ms: the existing chain;  chain_sparse_ms (e): the chain with compact +
            sparse trace in the masked trace's place;  listed: the pixels of the list;  marked_share: listed / (W * H);
            mismatches: bytes of the final planes of the new chain that differ from the existing chain's (must be 0).
  "dense":  the same (a), (b), (c), (d) with the FACING MAP itself as the mark -- where the sparse path is expected to lose.
Each figure: 10 warm-up and 60 timed launches between device events, the median, ONE run of the tool: passes this small moved 18 %
between runs, so a difference inside that band is not a win.  Every library runs in a child process of its own, under
its own time limit; this process never opens the GPU, and the tool stops at the first child that fails.  After the rows of a config: one
"ratio" row per list, (d) of this library over (a) of the parent's.  No threshold: every row is reported."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 60, 10
LISTS = {"4x4": (4, 4), "2x16": (2, 16)}


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
        d_pos, d_nrm, d_map, d_counts, d_ref = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n), ctx.malloc(4 * n), ctx.malloc(4 * n)
        api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
        p = api.UpsampleParams.make(0, 0, 0.9, 0.005 * diag)
        w, h = api.subsampled_size(W, H, 0, 0)
        m = w * h
        d_lpos, d_lnrm, d_lmap, d_lo, d_keep = ctx.malloc(m * 16), ctx.malloc(m * 16), ctx.malloc(m), ctx.malloc(4 * m), ctx.malloc(n)
        if mode == "this":
            d_list, d_n, d_scratch = ctx.malloc(4 * n), ctx.malloc(4), ctx.malloc(api.compact_scratch_bytes(W, H))
        table = scenes.jitter_offsets(48, 1.0, 19)
        for name, (count, spp) in LISTS.items():
            lights = api.SoftLightList.make(entries(sc, count, spp), table)
            api.facing_lights_device(ctx, wl.constants, lights.hard_list(), d_pos, d_nrm, W, H, d_map)
            row = {"config": config, "mode": mode, "list": name, "steps": STEPS, "warmup": WARMUP, "runs": 1, "W": W, "H": H}
            sub = lambda: api.subsample_gbuffer_device(ctx, p, d_pos, d_nrm, W, H, d_lpos, d_lnrm, d_lights_map=d_map, d_lo_lights_map=d_lmap)
            lo_trace = lambda: ctx.trace_soft_light_list_device(wl.constants, lights, d_lpos, w, h, d_lo, d_lights_map=d_lmap)
            rmap = lambda: api.upsample_retrace_map_device(ctx, count, p, d_pos, d_nrm, d_lpos, d_lnrm, W, H, d_keep, d_lights_map=d_map,
                                                           d_lo_lights_map=d_lmap)
            masked = lambda out=d_counts, mark=d_keep: ctx.trace_soft_light_list_device(wl.constants, lights, d_pos, W, H, out, d_lights_map=mark)
            up_keep = lambda out=d_counts: api.upsample_soft_light_list_device(ctx, lights, p, d_pos, d_nrm, d_lpos, d_lnrm, d_lo, W, H, out,
                                                                               d_lights_map=d_map, d_lo_lights_map=d_lmap, d_keep=d_keep)
            sub(), lo_trace(), rmap()
            ctx.synchronize()
            row["retrace_map_ms"] = med(_timed(ctx, rmap, STEPS, WARMUP))
            row["lo_trace_ms"] = med(_timed(ctx, lo_trace, STEPS, WARMUP))
            row["masked_trace_ms"] = med(_timed(ctx, masked, STEPS, WARMUP))
            row["chain_retrace_ms"] = med(_timed(ctx, lambda: (sub(), lo_trace(), rmap(), masked(), up_keep()), STEPS, WARMUP))
            if mode == "parent":
                print(json.dumps(row), flush=True)
                continue
            compact = lambda mark=d_keep: api.compact_light_map_device(ctx, count, mark, W, H, d_list, n, d_n, d_scratch)
            sparse = lambda out=d_counts, mark=d_keep: ctx.trace_soft_light_list_sparse_device(wl.constants, lights, d_pos, W, H, d_list, d_n, n,
                                                                                               out, d_lights_map=mark)
            compact()
            ctx.synchronize()
            listed = np.zeros(1, np.uint32)
            ctx.d2h(listed, d_n)
            row["listed"], row["marked_share"] = int(listed[0]), int(listed[0]) / n
            row["compact_ms"] = med(_timed(ctx, compact, STEPS, WARMUP))
            row["sparse_trace_ms"] = med(_timed(ctx, sparse, STEPS, WARMUP))
            row["compact_sparse_ms"] = row["compact_ms"] + row["sparse_trace_ms"]
            row["chain_sparse_ms"] = med(_timed(ctx, lambda: (sub(), lo_trace(), rmap(), compact(), sparse(), up_keep()), STEPS, WARMUP))
            # the final planes of both chains over the same preset
            zero = np.zeros(count * n, np.uint8)
            ctx.h2d(d_counts, zero)
            ctx.h2d(d_ref, zero)
            sub(), lo_trace(), rmap(), masked(d_ref), up_keep(d_ref)
            compact(), sparse(), up_keep()
            ctx.synchronize()
            a, b = np.zeros(count * n, np.uint8), np.zeros(count * n, np.uint8)
            ctx.d2h(a, d_counts)
            ctx.d2h(b, d_ref)
            row["mismatches"] = int((a != b).sum())
            print(json.dumps(row), flush=True)
            # the dense mark: the facing map itself
            dense = {"config": config, "mode": "dense", "list": name, "steps": STEPS, "warmup": WARMUP, "runs": 1, "W": W, "H": H}
            compact(d_map)
            ctx.synchronize()
            ctx.d2h(listed, d_n)
            dense["listed"], dense["marked_share"] = int(listed[0]), int(listed[0]) / n
            dense["masked_trace_ms"] = med(_timed(ctx, lambda: masked(d_ref, d_map), STEPS, WARMUP))
            dense["compact_ms"] = med(_timed(ctx, lambda: compact(d_map), STEPS, WARMUP))
            dense["sparse_trace_ms"] = med(_timed(ctx, lambda: sparse(d_counts, d_map), STEPS, WARMUP))
            dense["compact_sparse_ms"] = dense["compact_ms"] + dense["sparse_trace_ms"]
            ctx.h2d(d_counts, zero)
            masked(d_ref, d_map), sparse(d_counts, d_map)
            ctx.synchronize()
            ctx.d2h(a, d_counts)
            ctx.d2h(b, d_ref)
            dense["mismatches"] = int((a != b).sum())
            dense["sparse_over_masked"] = dense["compact_sparse_ms"] / dense["masked_trace_ms"]
            print(json.dumps(dense), flush=True)


def ratios(rows, config):
    out = []
    for name in LISTS:
        pick = lambda mode, key: next((r[key] for r in rows if r["config"] == config and r["list"] == name and r["mode"] == mode and key in r), None)
        a, d = pick("parent", "masked_trace_ms"), pick("this", "compact_sparse_ms")
        if a is None or d is None:
            continue
        out.append({"config": config, "mode": "ratio", "list": name, "parent_masked_trace_ms": a, "compact_sparse_ms": d,
                    "compact_sparse_over_parent_masked": d / a, "sparse_not_below_masked": d >= a,
                    "compact_over_retrace_map": pick("this", "compact_ms") / pick("this", "retrace_map_ms"),
                    "parent_chain_retrace_ms": pick("parent", "chain_retrace_ms"), "chain_sparse_ms": pick("this", "chain_sparse_ms"),
                    "chain_sparse_over_parent_chain": pick("this", "chain_sparse_ms") / pick("parent", "chain_retrace_ms"),
                    "listed": pick("this", "listed"), "marked_share": pick("this", "marked_share"), "mismatches": pick("this", "mismatches")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r38/list_sparse_retrace_ab.jsonl")
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
            runs = [("this", ROOT)]
            if args.parent_root:
                runs.insert(0, ("parent", os.path.abspath(args.parent_root)))
            rows = []
            for mode, root in runs:
                env = dict(os.environ)
                env.pop("RTS_LIB", None)
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, config, root], env=env, capture_output=True,
                                     text=True, timeout=400)
                if run.returncode != 0:
                    sys.exit(f"list_sparse_retrace_ab: {mode} on {config} failed ({run.returncode}): {run.stderr[-1500:]}")
                for line in run.stdout.splitlines():
                    if line.startswith("{"):
                        rows.append(json.loads(line))
                        emit(line)
            for r in ratios(rows, config):
                emit(json.dumps(r))


if __name__ == "__main__":
    main()
