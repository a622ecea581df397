"""What lighting a frame from a light list's planes costs in ONE combine pass against one single-light combine pass per light (GPU
box) -- DESIGN.md 4.21.

    python tools/list_combine_ab.py --parent-root <tree of the parent commit, built> [--configs city_4k,courtyard_4k,atrium_1080p]
                                    [--out profiles/r24/list_combine_ab.jsonl]

Lists: "4x4" = 4 lights of 4 samples, "2x16" = 2 lights of 16 (tools/soft_list_ab.py's entries), "8h" = 8 hard lights on the same ring;
each without a map and ("f") with the facing map of rtsh_facing_lights_device given to the trace and to the combine pass.  Variants:
    A     the parent commit's library: one rtsh_combine_device per light over its count plane -- what tools/render.py did before this
          commit, without its read-back and its numpy average, so A never sums: the comparison flatters A.  For "8h" the eight passes
          all read the list's one mask plane as if it were a byte plane: the traffic of eight passes, not a meaningful image.  A has
          no map argument: its combine passes are the same with and without "f".  (Run twice, before and after B: its own spread.)
    B     this commit: ONE rtsh_combine_(soft_)light_list_device pass, all buffers as allocated
    B1    the same with rgb one byte into a larger allocation
(profiles/r24/list_combine_ab.jsonl was taken while the library still held a second kernel of four pixels per lane, which the launcher
took for aligned buffers and a pixel count that is a multiple of 4: its rows call that kernel Bq and the one-pixel-per-lane kernel,
forced by the shifted rgb, Bp.  Bq was slower and is gone -- EXPERIMENTS.md --, so B and B1 now run the same kernel and differ only in
the alignment of the byte stores.)
Each is timed alone ("combine") and behind the list's trace ("frame": rts_trace_soft_light_list_device / rts_trace_light_list_device,
then the combine passes, between one pair of device events).  Every variant: 20 warm-up and 200 timed rounds, the median reported; B
and B1 alternate inside one child in four rounds of 50, and the four round medians are kept: their spread is the yardstick for one against
the other.  The parent's and this commit's variants run in child processes of this tool (a fresh process per library, each under its own time
limit; this process never opens the GPU).  The tool stops at the first child that fails.  Beside the times: both B forms against the
host twin (rtsh_combine_soft_light_list / rtsh_combine_light_list) at the size timed, byte for byte."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
STEPS, WARMUP, ROUNDS = 200, 20, 4
LISTS = {"4x4": (4, 4), "2x16": (2, 16), "8h": (8, 1)}     # name -> (lights, samples per light; 1: a hard list)


def child(mode, config, root):
    sys.path.insert(0, root)
    import numpy as np
    from raytracedshadows_amd import api, scenes, workloads
    from soft_list_ab import _timed, entries
    assert os.path.abspath(api.lib_path()).startswith(os.path.abspath(root)), api.lib_path()
    wl = workloads.prepare_config(config, cache=True)
    W, H = wl.W, wl.H
    n = W * H
    table = scenes.jitter_offsets(48, 1.0, 19)
    row = {"config": config, "mode": mode, "lib": "this commit" if os.path.abspath(root) == ROOT else "parent commit", "steps": STEPS,
           "warmup": WARMUP, "pixels": n}
    med = lambda ts: float(np.median(ts))
    with api.ShadowContext(0) as ctx:
        ctx.set_bvh(wl.packed)
        d_pos, d_nrm, d_map = ctx.malloc(n * 16), ctx.malloc(n * 16), ctx.malloc(n)
        d_planes, d_rgb = ctx.malloc(8 * n), ctx.malloc(n * 3 + 16)
        api.primary_gbuffer_device(ctx, wl.scene.eye, wl.scene.target, wl.scene.fovy, W, H, d_pos, d_nrm)
        ctx.synchronize()
        out = {}

        def make(name):
            count, samples = LISTS[name]
            es = entries(wl.scene, count, samples)
            if samples == 1:
                lst = api.LightList.make([(kind, xyz) for kind, xyz, _, _, _ in es])
                return lst, lst, [lst.light(l) for l in range(count)]
            lst = api.SoftLightList.make(es, table)
            return lst, lst.hard_list(), [lst.light(l) for l in range(count)]

        def trace(lst, facing):
            fn = ctx.trace_light_list_device if isinstance(lst, api.LightList) else ctx.trace_soft_light_list_device
            return lambda: fn(wl.constants, lst, d_pos, W, H, d_planes, d_lights_map=d_map if facing else None)

        def after(first, second):
            def run():
                first()
                second()
            return run

        if mode == "parent":
            for name in LISTS:
                lst, hard, ones = make(name)
                api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
                shared = isinstance(lst, api.LightList)                  # "8h": every pass reads the one mask plane

                def per_light():
                    for l, one in enumerate(ones):
                        api.combine_device(ctx, wl.constants, one, d_pos, d_nrm, d_planes if shared else d_planes + l * n, W, H, d_rgb)
                for f in ("", "f"):
                    trace(lst, bool(f))()
                    ctx.synchronize()
                    out["A_combine_%s%s" % (name, f)] = _timed(ctx, per_light, STEPS, WARMUP)
                    out["A_frame_%s%s" % (name, f)] = _timed(ctx, after(trace(lst, bool(f)), per_light), STEPS, WARMUP)
            row.update({v: {"median_ms": med(ts), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts))} for v, ts in out.items()})
        else:
            rounds, parity = {}, {}
            nrm, pos = np.empty((H, W, 4), np.float32), np.empty((H, W, 4), np.float32)
            ctx.d2h(nrm, d_nrm)
            ctx.d2h(pos, d_pos)
            for name in LISTS:
                lst, hard, _ = make(name)
                count = lst.count
                colors = np.full((count, 3), 1.0 / count, np.float32)
                soft = not isinstance(lst, api.LightList)
                fn = api.combine_soft_light_list_device if soft else api.combine_light_list_device
                api.facing_lights_device(ctx, wl.constants, hard, d_pos, d_nrm, W, H, d_map)
                for f in ("", "f"):
                    forms = {"B": d_rgb, "B1": d_rgb + 1}
                    combine = {v: (lambda p=p: fn(ctx, wl.constants, lst, d_pos, d_nrm, d_planes, W, H, p, d_lights_map=d_map if f else None,
                                                  colors=colors)) for v, p in forms.items()}
                    trace(lst, bool(f))()
                    ctx.synchronize()
                    for r in range(ROUNDS):                              # alternating: B, B1, B frame, B1 frame; four rounds
                        for v in forms:
                            key = "%s_combine_%s%s" % (v, name, f)
                            ts = _timed(ctx, combine[v], STEPS // ROUNDS, WARMUP // ROUNDS)
                            out.setdefault(key, []).extend(ts)
                            rounds.setdefault(key, []).append(med(ts))
                        for v in forms:
                            key = "%s_frame_%s%s" % (v, name, f)
                            ts = _timed(ctx, after(trace(lst, bool(f)), combine[v]), STEPS // ROUNDS, WARMUP // ROUNDS)
                            out.setdefault(key, []).extend(ts)
                            rounds.setdefault(key, []).append(med(ts))
                    # parity at the size that was timed: both forms against the host twin
                    planes, lights_map = np.empty((count if soft else 1, H, W), np.uint8), np.empty((H, W), np.uint8)
                    ctx.d2h(planes, d_planes)
                    ctx.d2h(lights_map, d_map)
                    twin = api.combine_soft_light_list if soft else api.combine_light_list
                    want = twin(wl.constants, lst, pos, nrm, planes if soft else planes[0], lights_map if f else None, colors)
                    got = np.empty((H, W, 3), np.uint8)
                    for v, p in forms.items():
                        ctx.h2d(d_rgb, np.zeros(n * 3 + 16, np.uint8))
                        combine[v]()
                        ctx.synchronize()
                        ctx.d2h(got, p)
                        parity["%s_%s%s" % (v, name, f)] = int((got != want).sum())
            row["mismatches_against_the_host_twin"] = parity
            row.update({v: {"median_ms": med(ts), "mean_ms": float(np.mean(ts)), "min_ms": float(np.min(ts)), "round_medians_ms": rounds[v]}
                        for v, ts in out.items()})
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p")
    ap.add_argument("--out", default="profiles/r24/list_combine_ab.jsonl")
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--child-timeout", type=int, default=300)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.config, os.path.abspath(args.root))
    parent = os.path.abspath(args.parent_root)
    if not os.path.exists(os.path.join(parent, "raytracedshadows_amd", "librts.so")):
        sys.exit(f"list_combine_ab: no built library under {parent} (export the parent commit there and build it)")
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
                    sys.exit(f"list_combine_ab: {config} {tag} failed (exit {p.returncode}); nothing more is started")
                rows[tag] = json.loads(line[4:])
                rows[tag]["tag"] = tag
                fh.write(json.dumps(rows[tag]) + "\n")
                fh.flush()
            a1, a2, new = rows["A1"], rows["A2"], rows["new"]
            s = {"config": config, "tag": "summary", "mismatches_against_the_host_twin": new["mismatches_against_the_host_twin"]}
            for name in LISTS:
                for f in ("", "f"):
                    for what in ("combine", "frame"):
                        key = "%s_%s%s" % (what, name, f)
                        a = [a1["A_" + key]["median_ms"], a2["A_" + key]["median_ms"]]
                        am = 0.5 * (a[0] + a[1])
                        q, p = new["B_" + key], new["B1_" + key]
                        spread = lambda r: (max(r) - min(r)) / (sum(r) / len(r))
                        s[key] = {"A_ms": a, "A_spread": abs(a[0] - a[1]) / am, "B_ms": q["median_ms"], "B1_ms": p["median_ms"],
                                  "B_over_A": q["median_ms"] / am, "B1_over_A": p["median_ms"] / am,
                                  "B_over_B1": q["median_ms"] / p["median_ms"],
                                  "B_round_spread": max(spread(q["round_medians_ms"]), spread(p["round_medians_ms"])),
                                  "B_below_A": max(q["median_ms"], p["median_ms"]) < min(a)}
            fh.write(json.dumps(s) + "\n")
            fh.flush()
            print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
