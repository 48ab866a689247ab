"""Rate of the connected components (Context.label_components, component_stats, remove_small_objects, fill_holes),
include/microaligner_components.h.

    python tools/components_rate.py [--size N] [--reps K] [--parent DIR] [--no-bench]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: N^2 (default 16384^2) device-resident uint8 masks -- random at density 0.593 (the site-percolation threshold),
   blobs (smooth noise above a threshold, a few thousand objects), all ones (one component: one atomic target for every
   tile) and the checkerboard (under 4 neighbours every foreground pixel its own component: the largest count, and the
   largest arrays of areas and boxes) -- under both connectivities.  Per case the median of `reps` HIP-event timings after
   a warm-up call, with minimum and maximum, of: label_components alone and followed by component_stats ("label with
   info"; the label call waits for the stream once, for its count), remove_small_objects(100), fill_holes(max_size=100), each with the
   number of components.  The yardsticks on the same box: Context.morphology("erode", 1) on the same mask, and
   scipy.ndimage.label on a 4096^2 crop of it on one CPU core (wall clock, one call).
2. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from flow_smooth_rate import device_ms, run

BAND = 1024


def random_mask(n, density=0.593, seed=0):
    rng = np.random.default_rng(seed)
    m = np.empty((n, n), np.uint8)
    for y0 in range(0, n, BAND):
        m[y0:y0 + BAND] = rng.random((min(BAND, n - y0), n), np.float32) < density
    return m


def blob_mask(n, cell=96, level=0.66, seed=1):
    """bilinear noise on a grid of `cell` pixels above `level`: separate smooth objects, about 0.2 per cell"""
    rng = np.random.default_rng(seed)
    g = n // cell + 2
    noise = rng.random((g, g), np.float32)
    x = np.arange(n, dtype=np.float32) / cell
    xi, xf = x.astype(np.int64), x - np.floor(x)
    m = np.empty((n, n), np.uint8)
    for y0 in range(0, n, BAND):
        y = np.arange(y0, min(y0 + BAND, n), dtype=np.float32) / cell
        yi, yf = y.astype(np.int64), (y - np.floor(y))[:, None]
        top = noise[yi][:, xi] * (1 - xf) + noise[yi][:, xi + 1] * xf
        bottom = noise[yi + 1][:, xi] * (1 - xf) + noise[yi + 1][:, xi + 1] * xf
        m[y0:y0 + BAND] = top * (1 - yf) + bottom * yf > level
    return m


def ones_mask(n):
    return np.ones((n, n), np.uint8)


def checkerboard(n):
    m = np.zeros((n, n), np.uint8)
    m[0::2, 0::2] = 1
    m[1::2, 1::2] = 1
    return m


def step_kernel(a):
    from microaligner_amd.device import get_context
    ctx = get_context()
    n = a.size
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for name, make in (("random 0.593", random_mask), ("blobs", blob_mask), ("all ones", ones_mask), ("checkerboard", checkerboard)):
        host = make(n)
        if ndimage is not None:
            crop = np.ascontiguousarray(host[:4096, :4096])
            for c in (1, 2):
                t0 = time.perf_counter()
                _, count = ndimage.label(crop, ndimage.generate_binary_structure(2, c))
                print(f"cpu    {crop.shape[0]}^2 {name:12s} connectivity {c} scipy.ndimage.label (yardstick): "
                      f"{(time.perf_counter() - t0) * 1e3:9.1f} ms, {count} components", flush=True)
        d = ctx.asdevice(host)
        del host
        ctx._resident.clear()
        out = ctx.empty((n, n), np.uint8)
        labels = ctx.empty((n, n), np.int32)
        for c in (1, 2):
            count = [0]

            def label():
                _, count[0] = ctx.label_components(d, c, out=labels)

            def label_info():
                label()
                return ctx.component_stats(labels, count[0])
            cases = (("label", label), ("label with info", label_info),
                     ("remove_small_objects 100", lambda: ctx.remove_small_objects(d, 100, c, out=out)),
                     ("fill_holes 100", lambda: ctx.fill_holes(d, 100, c, out=out)))
            for what, fn in cases:
                r = fn()                                    # first launch, the buffers
                del r
                ms, lo, hi = device_ms(ctx, fn, a.reps)
                print(f"kernel {n}^2 {name:12s} connectivity {c} {what:24s}: {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f}, "
                      f"{a.reps} calls), {n * n / ms / 1e6:7.2f} Gpx/s, {count[0]} components", flush=True)
        fn = lambda: ctx.morphology(d, "erode", 1, out=out)       # noqa: E731
        fn()
        ms, lo, hi = device_ms(ctx, fn, a.reps)
        print(f"kernel {n}^2 {name:12s} grey_erode r=1 (yardstick): {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls), "
              f"{n * n / ms / 1e6:7.2f} Gpx/s", flush=True)
        del d, out, labels
        ctx.trim()


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
    run([sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--reps", str(a.reps), "--step", "kernel"], 560)
    if a.no_bench:
        return
    bench = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]
    for _ in range(2):
        run(bench, 300)
        if a.parent:
            run(bench, 300, cwd=os.path.abspath(a.parent))


if __name__ == "__main__":
    main()
