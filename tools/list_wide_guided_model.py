"""The synthetic model behind the variance guide of the wide filter, numpy alone -- no library, no GPU.

    python tools/list_wide_guided_model.py [--samples 4]

A frame of 128 x 96 pixels with a linear penumbra of width w pixels across its middle column, Binomial(n, p) counts, no geometry edges,
and the exact integer rule of include/rts_scene.h (rtsh_wide_filter_guided_soft_light_list): V_0 = c * (65535 // n), E = V_0 (n S - V_0),
G and D over the 3 x 3 neighbourhood with weights {1, 2, 1}^2, T = min(65535, isqrt(k4^2 G // (16 D n))), 5 x 5 passes of weights
{1, 4, 6, 4, 1}^2 with taps 1, 2, 4, ... pixels apart, the rounded mean.  Printed: the mean absolute error to the true visibility of the
raw counts, of the unguided filter and of the guided one at guide_k4 = 8, 12 and 16, at 2, 3 and 4 passes, for w = 1.5, 4, 30 and 80.
A model, not a measurement of the scenes: tools/list_filter_quality.py --wide --guide measures those, and disagrees with it for wide
lights under the jittered trace."""
import argparse

import numpy as np


def isqrt(a):
    r = np.floor(np.sqrt(a.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > a, r - 1, r)
    return np.where((r + 1) * (r + 1) <= a, r + 1, r)


def shifted(H, W, oy, ox):
    """Source and destination slices of a frame shifted by (oy, ox), the part inside the frame."""
    return (slice(max(0, oy), H + min(0, oy)), slice(max(0, ox), W + min(0, ox))), (slice(max(0, -oy), H + min(0, -oy)), slice(max(0, -ox), W + min(0, -ox)))


def run(rng, w, n, passes, k4, H=96, W=128):
    x = np.arange(W)[None, :] + 0 * np.arange(H)[:, None]
    p = np.clip((x - W / 2) / w + 0.5, 0, 1)
    S = 65535 // n
    V = rng.binomial(n, p).astype(np.int64) * S
    T = None
    if k4:
        E, G, D = V * (n * S - V), np.zeros_like(V), np.zeros_like(V)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                src, dst = shifted(H, W, dy, dx)
                G[dst] += (2 - abs(dy)) * (2 - abs(dx)) * E[src]
                D[dst] += (2 - abs(dy)) * (2 - abs(dx))
        T = np.minimum(isqrt((k4 * k4 * G) // (16 * D * n)), 65535)
    b = [6, 4, 1]
    for k in range(passes):
        num, den = np.zeros_like(V), np.zeros_like(V)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if abs(dy << k) >= H or abs(dx << k) >= W:
                    continue
                src, dst = shifted(H, W, dy << k, dx << k)
                q = V[src]
                acc = np.ones(q.shape, bool) if T is None else np.abs(q - V[dst]) <= T[dst]
                num[dst] += b[abs(dy)] * b[abs(dx)] * q * acc
                den[dst] += b[abs(dy)] * b[abs(dx)] * acc
        V = (2 * num + den) // (2 * den)
    return float(np.abs(V / (n * S) - p).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    n = args.samples
    for w in (1.5, 4, 30, 80):
        row = [f"w {w:g} n {n} raw {run(rng, w, n, 0, 0):.4f}"]
        for passes in (2, 3, 4):
            row.append(f"passes {passes}: unguided {run(rng, w, n, passes, 0):.4f} k4=8 {run(rng, w, n, passes, 8):.4f} "
                       f"k4=12 {run(rng, w, n, passes, 12):.4f} k4=16 {run(rng, w, n, passes, 16):.4f}")
        print(" | ".join(row))


if __name__ == "__main__":
    main()
