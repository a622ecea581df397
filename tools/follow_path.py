"""Follow mode over a camera path: K frames with the eye moved `step` of eye -> target per frame, every mode traced on
every frame, the modes alternating inside one process.

  default        the everyday launch (no table, follow off)
  tuned_m0/m1    rts_ctx_autotune on frame 0 ("tune_for_motion" 0 / 1), its table and options reused on every later frame
  follow_bB_sS   option "follow" 1 with "follow_block" B and "follow_square" S (each mode its own context: its own state)

Each frame's G-buffer is made on the device, untimed (rtsh_primary_gbuffer_device).  Each trace is timed between two rts_timer_mark
slots on the default stream, so a follow mode's time includes its planner kernels.  Masks are checked against the oracle on
4 sampled frames per mode (and every mode against the default on every frame).  One JSON line per (config, step, mode): median and
spread of the per-frame time, and its ratio to the default's median.

  python tools/follow_path.py [--configs city_4k,...] [--steps 0.001,0.003] [--frames 60] [--modes default,follow_b8_s32,...]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STRIPE = (32, 8, 0)          # band_rows, n_stripes, stripe: one eighth of the frame
ALL_MODES = ["default", "tuned_m0", "tuned_m1"] + [f"follow_b{b}_s{s}" for s in (0, 32) for b in (1, 2, 4, 8, 16)]


def main():
    from raytracedshadows_amd import api, workloads
    import oracle
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="city_4k,courtyard_4k,atrium_1080p,city_4k_stripe")
    ap.add_argument("--steps", default="0.001,0.003")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--modes", default=",".join(ALL_MODES))
    ap.add_argument("--no-parity", action="store_true")
    args = ap.parse_args()
    modes = args.modes.split(",")
    for cfg in args.configs.split(","):
        stripes = STRIPE if cfg.endswith("_stripe") else None
        wl = workloads.prepare_config(cfg[:-len("_stripe")] if stripes else cfg, cache=True)
        W, H, sc = wl.W, wl.H, wl.scene
        for step in (float(s) for s in args.steps.split(",")):
            ctxs = {}
            try:
                for m in modes:
                    c = api.ShadowContext(0)
                    ctxs[m] = c
                    c.set_bvh(wl.packed)
                base = ctxs[modes[0]]
                d_pos, masks = base.malloc(W * H * 16), {m: base.malloc(W * H) for m in modes}

                def constants(i):
                    eye = (sc.eye + (sc.target - sc.eye) * np.float32(step * i)).astype(np.float32)
                    return eye, api.RayTracingConstants.make(eye, sc.light_direction, W, H, sc.target - eye)

                def trace(c, k, d_mask):
                    if stripes:
                        c.trace_shadow_mask_stripes_device(k, d_pos, W, H, d_mask, *stripes, light=wl.light)
                    else:
                        c.trace_shadow_mask_device(k, d_pos, W, H, d_mask, light=wl.light)

                eye0, k0 = constants(0)
                api.primary_gbuffer_device(base, eye0, sc.target, sc.fovy, W, H, d_pos)
                base.synchronize()
                for m, c in ctxs.items():
                    if m.startswith("tuned"):
                        c.set_option("tune_for_motion", 1 if m.endswith("m1") else 0)
                        c.autotune(k0, d_pos, W, H, masks[m], light=wl.light, stripes=stripes)
                    elif m.startswith("follow"):
                        b, s = m[len("follow_b"):].split("_s")
                        c.set_option("follow", 1)
                        c.set_option("follow_block", int(b))
                        c.set_option("follow_square", int(s))
                times = {m: [] for m in modes}
                bad = {m: 0 for m in modes}
                checked = {m: 0 for m in modes}
                sample = {0, args.frames // 3, 2 * args.frames // 3, args.frames - 1}
                rows = api.stripe_rows(H, *stripes) if stripes else H
                sel = np.ones((H, W), bool)                # the rows this dispatch writes
                if stripes:
                    sel[:] = False
                    for r0 in range(stripes[2] * stripes[0], H, stripes[0] * stripes[1]):
                        sel[r0:r0 + stripes[0]] = True
                sel = sel.reshape(-1)
                for i in range(args.frames):
                    eye, k = constants(i)
                    api.primary_gbuffer_device(base, eye, sc.target, sc.fovy, W, H, d_pos)
                    base.synchronize()
                    order = modes[i % len(modes):] + modes[:i % len(modes)]          # (alternating: each mode in every place)
                    for m in order:
                        c = ctxs[m]
                        c.timer_mark(0)
                        trace(c, k, masks[m])
                        c.timer_mark(1)
                        times[m].append(c.timer_between_ms(0, 1))
                    got = {}
                    for m in modes:
                        got[m] = np.empty(W * H, np.uint8)
                        ctxs[m].synchronize()
                        base.d2h(got[m], masks[m])
                    if i in sample and not args.no_parity:
                        pos = np.empty(W * H * 4, np.float32)
                        base.d2h(pos, d_pos)
                        want = oracle.shadow_mask(wl.packed, k.as_array(), oracle.light_from_product(wl.light, k), pos, W, H)[0].reshape(-1)
                        for m in modes:
                            bad[m] += int((got[m][sel] != want[sel]).sum())
                            checked[m] += 1
                    ref = got[modes[0]]
                    for m in modes[1:]:
                        bad[m] += int((got[m][sel] != ref[sel]).sum())
                med0 = float(np.median(times[modes[0]]))
                for m in modes:
                    t = np.array(times[m])
                    rec = {"config": cfg, "step": step, "mode": m, "frames": args.frames, "rows": rows,
                           "median_ms": round(float(np.median(t)), 5), "p10_ms": round(float(np.percentile(t, 10)), 5),
                           "p90_ms": round(float(np.percentile(t, 90)), 5), "steady_median_ms": round(float(np.median(t[2:])), 5),
                           "vs_default": round(float(np.median(t)) / med0 - 1.0, 4), "parity_frames": checked[m], "bad_bytes": bad[m]}
                    c = ctxs[m]
                    if m.startswith("follow"):
                        rec["ordered_traces"] = c.get_option("follow_ordered")
                    if m.startswith("tuned"):
                        rec["kernel"] = c.get_option("kernel")
                        rec["table_tiles"] = c.get_option("split_tiles") + c.get_option("front_tiles")
                    print(json.dumps(rec), flush=True)
                base.free(d_pos)
                for p in masks.values():
                    base.free(p)
            finally:
                for c in ctxs.values():
                    c.close()


if __name__ == "__main__":
    main()
