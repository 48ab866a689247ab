"""Rate of the order statistics and the range normalisation (include/microaligner_quantile.h) on device-resident images.

    python tools/quantile_rate.py [--size N] [--reps K] [--dtypes u8,u16,f32]

Images are `size`^2 (16384) in uint8 / uint16 / float32, of two kinds: (a) uniform noise, (b) 95 % one background value plus
a tissue-like remainder.  Per image it times, alternating the cases inside every repetition, as the median of `reps` calls
after a warm-up with the minimum and the maximum (wall clock around a synchronised call, inputs in HBM):
 - image_quantiles for 2 and for 8 ranks;
 - normalize_range_u8;
 - normalize_percentile end to end (on_device);
 - the yardstick: what the min-max scaling costs today, Context.minmax followed by Context.normalize_minmax_u8.
Beside the time: the bytes the case must move (passes x image bytes, + n for a u8 output) and the rate that makes against
the 8 TB/s peak."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from microaligner_amd import normalize_percentile
from microaligner_amd.device import get_context

PEAK = 8e12
PASSES = {"u8": 1, "u16": 2, "f32": 3}
DT = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
Q2 = [0.0, 0.999]
Q8 = [0.0, 0.001, 0.01, 0.25, 0.5, 0.75, 0.99, 0.999]


def make(kind, name, size, seed):
    """A size^2 image tiled from one 2048^2 tile (the statistics of a tile are those of the image)."""
    rng = np.random.default_rng(seed)
    t = min(size, 2048)
    if name == "u8":
        noise = rng.integers(0, 256, (t, t), dtype=np.uint8)
        tissue = (20 + rng.gamma(2.0, 18.0, (t, t))).clip(0, 255).astype(np.uint8)
        back = np.uint8(12)
    elif name == "u16":
        noise = rng.integers(0, 65536, (t, t)).astype(np.uint16)
        tissue = (200 + rng.gamma(2.0, 400.0, (t, t))).clip(0, 65535).astype(np.uint16)
        back = np.uint16(200)
    else:
        noise = rng.random((t, t), dtype=np.float32) * np.float32(4096.0) - np.float32(100.0)
        tissue = (200 + rng.gamma(2.0, 400.0, (t, t))).astype(np.float32)
        back = np.float32(200.0)
    tile = noise if kind == "a" else np.where(rng.random((t, t)) < 0.05, tissue, back).astype(DT[name])
    reps = -(-size // t)
    return np.ascontiguousarray(np.tile(tile, (reps, reps))[:size, :size])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", default="u8,u16,f32")
    a = ap.parse_args()
    ctx = get_context()
    n = a.size * a.size
    for name in a.dtypes.split(","):
        esz = np.dtype(DT[name]).itemsize
        imgs = {kind: ctx.asdevice(make(kind, name, a.size, 3)) for kind in ("a", "b")}
        ctx.forget_host_arrays()
        ctx.sync()
        found = {}

        def q2(d, k):
            found[k, "q2"] = ctx.image_quantiles(d, Q2)

        def q8(d, k):
            found[k, "q8"] = ctx.image_quantiles(d, Q8)

        def rng_u8(d, k):
            lo, hi = found[k, "q2"][0]
            ctx.normalize_range_u8(d, lo, hi)

        def pct(d, k):
            normalize_percentile(d, 0.0, 99.9, on_device=True)

        def yard(d, k):
            ctx.minmax(d)
            ctx.normalize_minmax_u8(d)

        cases = [("image_quantiles, 2 ranks", q2, PASSES[name] * n * esz), ("image_quantiles, 8 ranks", q8, PASSES[name] * n * esz),
                 ("normalize_range_u8", rng_u8, n * esz + n), ("normalize_percentile", pct, (PASSES[name] + 1) * n * esz + n),
                 ("yardstick minmax + normalize_minmax_u8", yard, 3 * n * esz + n)]
        times = {(kind, c[0]): [] for kind in imgs for c in cases}
        for rep in range(a.reps + 1):                      # repetition 0 is the warm-up
            for label, fn, _ in cases:
                for kind, d in imgs.items():
                    ctx.sync()
                    t0 = time.perf_counter()
                    fn(d, kind)
                    ctx.sync()
                    if rep:
                        times[kind, label].append((time.perf_counter() - t0) * 1e3)
        for kind in imgs:
            what = "uniform noise" if kind == "a" else "95 % background + tissue"
            vals, counts = found[kind, "q2"]
            print(f"{name} {a.size}x{a.size} ({kind}) {what}: q {Q2} -> {vals.tolist()}, pop {counts.pop}")
            yard_ms = float(np.median(times[kind, cases[-1][0]]))
            for label, _, nbytes in cases:
                v = times[kind, label]
                med = float(np.median(v))
                print(f"  {label:40s} {med:8.3f} ms median (min {min(v):.3f}, max {max(v):.3f})  {nbytes / 1e9:6.2f} GB  "
                      f"{nbytes / med / 1e9:6.2f} TB/s = {100 * nbytes / (med * 1e-3) / PEAK:5.1f} % of peak  "
                      f"{med / yard_ms:5.2f} x yardstick")
        for label, _, _ in cases:
            ma, mb = (float(np.median(times[k, label])) for k in ("a", "b"))
            print(f"  (b) / (a) {label:40s} {mb / ma:5.2f}")
        del imgs
        ctx.trim()


if __name__ == "__main__":
    main()
