"""Rate of the texture support maps (Context.texture_maps), include/microaligner_texture.h.

    python tools/texture_rate.py [--size N] [--reps K] [--parent DIR] [--no-bench]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident image (a smooth pattern plus noise, a quarter of it exactly constant) as
   uint8, uint16 and float32.  Per case the median of `reps` HIP-event timings of one call after a warm-up call, with minimum
   and maximum: the solver's window (r = 49) and sigma = 6 (r = 18), each with the two eigenvalue planes only and with the
   weight and the per-cell counts at cells of 1000 beside them; and Context.smooth_flow(where="all") with the same taps on
   the same box as the yardstick (the same filter over three planes, a flow in and a flow out).
2. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from flow_smooth_rate import device_ms, flow_b, run


def image(n, dtype):
    """a smooth pattern plus noise in [0, 1], exactly 0.5 in the last quarter of the rows, built in row bands"""
    rng = np.random.default_rng(0)
    out = np.empty((n, n), dtype)
    full = 1.0 if dtype is np.float32 else float(np.iinfo(dtype).max)
    xx = np.arange(n, dtype=np.float32)[None, :]
    for y0 in range(0, n, 1024):
        yy = np.arange(y0, min(y0 + 1024, n), dtype=np.float32)[:, None]
        v = 0.5 + 0.3 * np.sin(xx / 5) * np.cos(yy / 7) + 0.1 * (rng.random((len(yy), n), dtype=np.float32) - 0.5)
        v[np.broadcast_to(yy >= 3 * n // 4, v.shape)] = 0.5
        out[y0:y0 + 1024] = v if dtype is np.float32 else np.rint(v * full)
    return out, full


def step_kernel(a):
    from microaligner_amd.device import gaussian_taps, get_context
    from microaligner_amd.shared_modules.texture import window_taps
    ctx = get_context()
    n = a.size
    windows = (("r 49 (winsize 99)", window_taps(99)), ("r 18 (sigma 6)   ", gaussian_taps(6.0)))
    for dtype in (np.uint8, np.uint16, np.float32):
        host, full = image(n, dtype)
        d = ctx.asdevice(host)
        del host
        floor = 1e-4 * full * full
        for name, taps in windows:
            cases = [(f"texture_maps {np.dtype(dtype).name:7s} {name} eigenvalues          ", lambda t=taps: ctx.texture_maps(d, t)),
                     (f"texture_maps {np.dtype(dtype).name:7s} {name} + weight, cells 1000 ",
                      lambda t=taps: ctx.texture_maps(d, t, floor, 1000, ("lam_min", "lam_max", "weight")))]
            for label, fn in cases:
                r = fn()                                        # first launch, the buffers
                counts = r.get("counts")
                del r
                ms, lo, hi = device_ms(ctx, fn, a.reps)
                print(f"kernel {n}^2 {label}: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls), "
                      f"{n * n / ms / 1e6:7.2f} Gpx/s", flush=True)
            print(f"classes at floor 1e-4 of squared full scale (textured, edge, flat): "
                  f"{[int(v) for v in counts.sum((0, 1))]} of {n * n}", flush=True)
        del d
    f = ctx.asdevice(flow_b(n))
    for name, taps in windows:
        fn = lambda t=taps: ctx.smooth_flow(f, t)               # noqa: E731
        r = fn()
        del r
        ms, lo, hi = device_ms(ctx, fn, a.reps)
        print(f"kernel {n}^2 smooth_flow all, no weight {name} (yardstick)   : {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, "
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
