"""Rate of the median filter of a flow (Context.median_flow), include/microaligner_flowmedian.h.

    python tools/flow_median_rate.py [--size N] [--reps K] [--parent DIR] [--no-bench]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident flow -- the test suite's smooth flow B of up to 25 px, +-0.05 px of
   pixel noise, and 20 px spikes on 1 % of the pixels.  Per case the median of `reps` HIP-event timings of one call after a
   warm-up call, with minimum and maximum: r = 1, 2, 3, 5, 7, each with where="all" and where="outliers" (thresh 1), with
   no weight and with a uint8 mask (1 % of the pixels dropped in 64 x 64 blocks).  At the radii of the register path its
   kernel and the generic one are timed in turns, call by call.  Context.compose_flows and Context.smooth_flow (sigma 2) on
   the same box are the yardsticks.
2. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from flow_smooth_rate import block_mask, flow_b, run  # noqa: E402

REGISTER_RADII = (1, 2, 3)


def spiked_flow_b(n):
    """flow B with +-0.05 px of pixel noise and 20 px spikes on 1 % of the pixels, built in row bands"""
    f = flow_b(n)
    rng = np.random.default_rng(0)
    for y0 in range(0, n, 1024):
        band = f[y0:y0 + 1024]
        band += rng.random(band.shape, dtype=np.float32) * np.float32(0.1) - np.float32(0.05)
        spikes = rng.random(band.shape[:2], dtype=np.float32) < 0.01
        band[spikes] += np.float32(20)
    return f


def device_ms_in_turns(ctx, fns, reps):
    """[(median, min, max)] of the calls fns, timed in turns: one call of each per round"""
    times = [[] for _ in fns]
    a, b = ctx.event(), ctx.event()
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ctx.record(a)
            r = fn()
            ctx.record(b)
            times[k].append(ctx.elapsed_ms(a, b))
            del r
    return [(float(np.median(t)), min(t), max(t)) for t in times]


def step_kernel(a):
    from microaligner_amd.device import gaussian_taps, get_context
    ctx = get_context()
    n = a.size
    d = ctx.asdevice(spiked_flow_b(n))
    keep = ctx.asdevice(block_mask(n))
    floor_ms = 16.0 * n * n / 8e12 * 1e3                 # 8 B/px read, 8 B/px written, at 8 TB/s

    def report(name, ms, lo, hi):
        print(f"kernel {n}^2 {name}: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls), "
              f"{n * n / ms / 1e6:7.2f} Gpx/s, {100 * floor_ms / ms:5.1f} % of the 16 B/px floor", flush=True)

    for r in (1, 2, 3, 5, 7):
        for where, thresh in (("all", None), ("outliers", 1.0)):
            for wname, w in (("no weight", None), ("u8 mask  ", keep)):
                kinds = (("registers", False), ("generic  ", True)) if r in REGISTER_RADII else (("generic  ", False),)
                fns = [lambda g=g, r=r, w=w, where=where, thresh=thresh: ctx.median_flow(d, r, w, None, where, thresh, generic=g)
                       for _, g in kinds]
                for fn in fns:                              # first launch, the buffers
                    res = fn()
                    del res
                for (kname, _), t in zip(kinds, device_ms_in_turns(ctx, fns, a.reps)):
                    report(f"median_flow r {r} {where:8s} {wname} {kname}", *t)
    _, info = ctx.median_flow(d, 2, keep, None, "outliers", 1.0, return_info=True)
    print(f"r 2, thresh 1, u8 mask: {info.outliers} outliers, {info.dropped} dropped, {info.unsupported} unsupported of {n * n}",
          flush=True)
    taps = gaussian_taps(2.0)
    for name, fn in (("smooth_flow sigma 2 (r 6) all, no weight (yardstick)", lambda: ctx.smooth_flow(d, taps)),
                     ("compose_flows (yardstick)                           ", lambda: ctx.compose_flows(d, d))):
        res = fn()
        del res
        report(name, *device_ms_in_turns(ctx, [fn], a.reps)[0])


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
