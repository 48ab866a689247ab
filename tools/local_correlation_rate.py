"""Rate of the local correlation maps (Context.local_correlation), include/microaligner_localcorr.h.

    python tools/local_correlation_rate.py [--size N] [--reps K] [--parent DIR] [--no-bench]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident pair (the pattern of tools/texture_rate.py, a quarter of it exactly
   constant; the other image is 0.8 of it plus 0.05 with noise of its own, float32) with the reference as uint8, uint16 and
   float32.  Per case the median of `reps` HIP-event timings of one call after a warm-up call, with minimum and maximum:
   r = 12 (sigma 4) and r = 49 (the solver's window), score and weight planes, each without a weight and with a uint8 mask
   that drops 1 % of the image in blocks of 64; then once with the per-cell counts at cells of 1000.  Yardsticks on the
   same box with the same taps: Context.texture_maps (three planes through the same tile) and
   Context.smooth_flow(where="all").
2. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from flow_smooth_rate import block_mask, device_ms, flow_b, run
from texture_rate import image


def step_kernel(a):
    from microaligner_amd.device import gaussian_taps, get_context
    from microaligner_amd.shared_modules.texture import window_taps
    ctx = get_context()
    n = a.size
    windows = (("r 12 (sigma 4)   ", gaussian_taps(4.0)), ("r 49 (winsize 99)", window_taps(99)))
    v, _ = image(n, np.float32)
    rng = np.random.default_rng(1)
    keep = ctx.asdevice(block_mask(n))
    planes = ("score", "weight")
    for dtype in (np.uint8, np.uint16, np.float32):
        full = 1.0 if dtype is np.float32 else float(np.iinfo(dtype).max)
        d_ref = ctx.asdevice(v if dtype is np.float32 else np.rint(v * np.float32(full)).astype(dtype))
        other = np.empty((n, n), np.float32)
        for y0 in range(0, n, 1024):
            band = v[y0:y0 + 1024]
            other[y0:y0 + 1024] = (0.8 * band + 0.05 + 0.004 * rng.standard_normal(band.shape, dtype=np.float32)) * np.float32(full)
        d_img = ctx.asdevice(other)
        del other
        floor, center = 6.4e-5 * full * full, (0.5 * full, 0.45 * full)
        for name, taps in windows:
            cases = [(f"local_correlation {np.dtype(dtype).name:7s} {name} no weight   ",
                      lambda t=taps: ctx.local_correlation(d_ref, d_img, t, floor, center, want=planes)),
                     (f"local_correlation {np.dtype(dtype).name:7s} {name} uint8 mask  ",
                      lambda t=taps: ctx.local_correlation(d_ref, d_img, t, floor, center, keep, want=planes))]
            for label, fn in cases:
                r = fn()                                        # first launch, the buffers
                del r
                ms, lo, hi = device_ms(ctx, fn, a.reps)
                print(f"kernel {n}^2 {label}: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls), "
                      f"{n * n / ms / 1e6:7.2f} Gpx/s", flush=True)
        counts = ctx.local_correlation(d_ref, d_img, windows[0][1], floor, center, keep, cell_size=1000, want=())["counts"]
        print(f"classes at floor 6.4e-5 of squared full scale (agree, disagree, flat, unsupported): "
              f"{[int(c) for c in counts.sum((0, 1))]} of {n * n}", flush=True)
        del d_ref, d_img
    d = ctx.asdevice(v)
    del v
    for name, taps in windows:
        fn = lambda t=taps: ctx.texture_maps(d, t)              # noqa: E731
        r = fn()
        del r
        ms, lo, hi = device_ms(ctx, fn, a.reps)
        print(f"kernel {n}^2 texture_maps float32 eigenvalues {name} (yardstick): {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, "
              f"{a.reps} calls), {n * n / ms / 1e6:7.2f} Gpx/s", flush=True)
    del d
    f = ctx.asdevice(flow_b(n))
    for name, taps in windows:
        fn = lambda t=taps: ctx.smooth_flow(f, t)               # noqa: E731
        r = fn()
        del r
        ms, lo, hi = device_ms(ctx, fn, a.reps)
        print(f"kernel {n}^2 smooth_flow all, no weight       {name} (yardstick): {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, "
              f"{a.reps} calls), {n * n / ms / 1e6:7.2f} Gpx/s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", help="a built checkout of the parent commit, benchmarked in turns with this tree")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--step", choices=["kernel"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a)
    run([sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--reps", str(a.reps), "--step", "kernel"], 500)
    if a.no_bench:
        return
    bench = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]
    for _ in range(2):
        run(bench, 300)
        if a.parent:
            run(bench, 300, cwd=os.path.abspath(a.parent))


if __name__ == "__main__":
    main()
