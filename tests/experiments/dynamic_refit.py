"""GPU box: a scene that changes every frame -- the whole frame on the device with a REFIT of the BVH per frame (the topology of
frame 0's SAH tree is kept; boxes and leaf data follow the vertices).  Same motion as dynamic_scene.py (which rebuilds).

Per frame: the vertices move (a travelling wave, computed on the host and uploaded), one device refit, G-buffer pass, shadow mask,
combine.  First and last frame: the refitted stream is read back and checked against the host refit's bytes, and mask and G-buffer
against the oracle on that stream.  Also printed: SAH and LBVH rebuild times of frame 0 (same run), the trace time at frame 0 and
at the last frame, the trace time over a fresh SAH build of the last frame's vertices (what the refitted tree costs), cost_ratio,
and whether a split table planned at frame 0 survived.
    python tests/experiments/dynamic_refit.py [city|courtyard|atrium] [frames] [WxH] [table: 0|1] [refit_treelet]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle
from raytracedshadows_amd import api, scenes

name = sys.argv[1] if len(sys.argv) > 1 else "city"
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 30
W, H = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "3840x2160").split("x")]
table = int(sys.argv[4]) if len(sys.argv) > 4 else 0
treelet = int(sys.argv[5]) if len(sys.argv) > 5 else 0
sc = scenes.SCENES[name]()
base, idx = sc.flat()
P = sc.triangle_count
amp = 0.002 * float(np.linalg.norm(sc.bbox_max - sc.bbox_min))
k = api.RayTracingConstants.make(sc.eye, sc.light_direction, W, H)
light = api.Light.make(api.Light.POINT, sc.light_point)


def frame_vertices(f):
    v = base.copy()
    v[:, 1] += (amp * np.sin(0.35 * base[:, 0] + 0.6 * f)).astype(np.float32)
    return v


def trace_ms(ctx, d_pos, d_mask, n=7):
    t = []
    for _ in range(n):
        ctx.timer_mark(10)
        ctx.trace_shadow_mask_device(k, d_pos, W, H, d_mask, light=light)
        ctx.timer_mark(11)
        t.append(ctx.timer_between_ms(10, 11))
    return float(np.median(t))


with api.ShadowContext(0) as ctx:
    d_pos, d_nrm, d_mask, d_rgb = ctx.malloc(W * H * 16), ctx.malloc(W * H * 16), ctx.malloc(W * H), ctx.malloc(W * H * 3)
    d_v, d_i = ctx.malloc(base.nbytes), ctx.malloc(idx.nbytes)
    if treelet:
        ctx.set_option("refit_treelet", treelet)
    ctx.h2d(d_i, idx)
    v0 = frame_vertices(0)
    ctx.h2d(d_v, v0)
    lb = [api.bvh_build_device(ctx, (d_v, v0.size), 8, d_i, P, install=True, want_packed=False, algorithm="lbvh")[1] for _ in range(5)]
    sah = [api.bvh_build_device(ctx, (d_v, v0.size), 8, d_i, P, install=True, want_packed=False)[1] for _ in range(5)]
    packed0, _ = api.bvh_build_device(ctx, (d_v, v0.size), 8, d_i, P, install=True)      # frame 0's tree: the topology kept
    print(f"{name}: {P} triangles, {W}x{H}; rebuild of frame 0 on the device, median of 5: SAH {np.median(sah):.2f} ms, "
          f"LBVH {np.median(lb):.2f} ms", flush=True)
    api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
    if table:
        tiles, records = ctx.plan_splits(k, d_pos, W, H, d_mask, light=light, front_share=1.0 / 3.0)
        print(f"split table planned at frame 0: {tiles} split tiles, {records} records", flush=True)
    splits0 = ctx.get_option("split_tiles") + ctx.get_option("front_tiles")
    rows, first_trace, ratio = [], None, 1.0
    for f in range(frames):
        v = frame_vertices(f)
        ctx.h2d(d_v, v)                                                        # the renderer's animation (not timed)
        check = f in (0, frames - 1)
        t0 = time.time()
        packed, refit_ms, ratio = api.bvh_refit_device(ctx, (d_v, v.size), 8, d_i, P, want_packed=check)
        t1 = time.time()
        ctx.timer_mark(0)
        api.primary_gbuffer_device(ctx, sc.eye, sc.target, sc.fovy, W, H, d_pos, d_nrm)
        ctx.timer_mark(1)
        ctx.trace_shadow_mask_device(k, d_pos, W, H, d_mask, light=light)
        ctx.timer_mark(2)
        api.combine_device(ctx, k, light, d_pos, d_nrm, d_mask, W, H, d_rgb)
        ctx.timer_mark(3)
        ctx.synchronize()
        t2 = time.time()
        rows.append(((t1 - t0) * 1e3, refit_ms, ctx.timer_between_ms(0, 1), ctx.timer_between_ms(1, 2), ctx.timer_between_ms(2, 3), (t2 - t0) * 1e3))
        if check:
            host = api.bvh_refit(packed0, v, 8, idx, P)
            pos, mask = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint8)
            ctx.d2h(pos, d_pos); ctx.d2h(mask, d_mask)
            want_pos = oracle.primary_gbuffer(packed, sc.eye, sc.target, sc.fovy, W, H)[0]
            want, _, _ = oracle.shadow_mask(packed, k.as_array(), oracle.light_from_product(light, k), pos, W, H)
            tm = trace_ms(ctx, d_pos, d_mask)
            if f == 0:
                first_trace = tm
            print(f"frame {f}: device refit == host refit: {bool(np.array_equal(packed, host))}, G-buffer == oracle: "
                  f"{bool((pos.view(np.uint32) == np.asarray(want_pos).view(np.uint32)).all())}, mask mismatches vs oracle on the frame's "
                  f"own stream: {int((mask != want).sum())}, lit {float(mask.mean()):.3f}, trace {tm:.3f} ms (median of 7), "
                  f"cost_ratio {ratio:.4f}", flush=True)
    last_trace = tm
    splits1 = ctx.get_option("split_tiles") + ctx.get_option("front_tiles")
    r = np.array(rows[2:])                                              # (the first frames grow the context's buffers)
    m = np.median(r, 0)
    print(f"{name}: {P} triangles refitted every frame (treelets of <= {ctx.get_option('refit_treelet')} nodes), {W}x{H}, {len(r)} frames, medians: refit call {m[0]:.3f} ms (device {m[1]:.3f}), "
          f"G-buffer {m[2]:.3f}, shadow mask {m[3]:.3f}, combine {m[4]:.3f}; whole frame {m[5]:.2f} ms = {1e3 / m[5]:.0f} frames/s "
          f"(host-side vertex animation and upload not counted)")
    print(f"split table / front tiles: {splits0} at frame 0, {splits1} after {frames} refits "
          f"({'kept' if splits0 == splits1 else 'changed'}{'' if splits0 else ', none planned'})")
    # what the refitted tree costs: the last frame's vertices built afresh (SAH), same G-buffer, same light
    ctx.clear_splits()
    nosplit_last = trace_ms(ctx, d_pos, d_mask)
    api.bvh_build_device(ctx, (d_v, v.size), 8, d_i, P, install=True, want_packed=False)
    fresh = trace_ms(ctx, d_pos, d_mask)
    print(f"trace: frame 0 {first_trace:.3f} ms, frame {frames - 1} {last_trace:.3f} ms (without a table {nosplit_last:.3f}), "
          f"fresh SAH build of frame {frames - 1}'s vertices {fresh:.3f} ms (no table): the refitted tree costs "
          f"{(nosplit_last / fresh - 1) * 100:+.1f} %; cost_ratio {ratio:.4f}")
    for d in (d_pos, d_nrm, d_mask, d_rgb, d_v, d_i):
        ctx.free(d)
