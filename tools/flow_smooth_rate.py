"""Rate of the weighted flow smoothing (Context.smooth_flow) and of the fold mask (Context.fold_mask),
include/microaligner_flowsmooth.h.

    python tools/flow_smooth_rate.py [--size N] [--reps K] [--parent DIR] [--no-bench]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident smooth flow of up to 25 px (the test suite's flow B).  Per case the median
   of `reps` HIP-event timings of one call after a warm-up call, with minimum and maximum: sigma = 6 (r = 18) and r = 128,
   each with where="all" and no weight, where="all" with a uint8 mask and where="blend" with the mask (1 % of the pixels
   dropped in 64 x 64 blocks); the fold mask at margin 4; and Context.compose_flows on the same box as the yardstick.
2. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def flow_b(n):
    """the test suite's flow B on an n^2 grid, built in row bands"""
    f = np.empty((n, n, 2), np.float32)
    xx = np.arange(n, dtype=np.float32)[None, :]
    for y0 in range(0, n, 1024):
        yy = np.arange(y0, min(y0 + 1024, n), dtype=np.float32)[:, None]
        f[y0:y0 + 1024, :, 0] = 20 * np.sin(xx / 90) * np.cos(yy / 70) + 5
        f[y0:y0 + 1024, :, 1] = 15 * np.cos(xx / 110 + yy / 80) - 3
    return f


def block_mask(n, share=0.01, block=64):
    rng = np.random.default_rng(0)
    g = -(-n // block)
    cells = (rng.random((g, g)) >= share).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(cells, block, 0), block, 1)[:n, :n])


def device_ms(ctx, fn, reps):
    out = []
    a, b = ctx.event(), ctx.event()
    for _ in range(reps):
        ctx.record(a)
        r = fn()
        ctx.record(b)
        out.append(ctx.elapsed_ms(a, b))
        del r
    return float(np.median(out)), min(out), max(out)


def step_kernel(a):
    from microaligner_amd.device import gaussian_taps, get_context
    ctx = get_context()
    n = a.size
    d = ctx.asdevice(flow_b(n))
    keep = ctx.asdevice(block_mask(n))
    wide = gaussian_taps(128 / 3.0, 127.5 / (128 / 3.0))
    assert len(wide) == 129
    cases = []
    for name, taps in (("sigma 6 (r 18)", gaussian_taps(6.0)), ("r 128        ", wide)):
        cases += [(f"smooth_flow {name} all, no weight ", lambda t=taps: ctx.smooth_flow(d, t)),
                  (f"smooth_flow {name} all, u8 mask   ", lambda t=taps: ctx.smooth_flow(d, t, keep)),
                  (f"smooth_flow {name} blend, u8 mask ", lambda t=taps: ctx.smooth_flow(d, t, keep, where="blend"))]
    cases += [("fold_mask margin 4                       ", lambda: ctx.fold_mask(d, 4)),
              ("compose_flows (yardstick)                ", lambda: ctx.compose_flows(d, d))]
    for name, fn in cases:
        r = fn()                                        # first launch, the buffers
        del r
        ms, lo, hi = device_ms(ctx, fn, a.reps)
        print(f"kernel {n}^2 {name}: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls), "
              f"{n * n / ms / 1e6:7.2f} Gpx/s", flush=True)
    _, info = ctx.smooth_flow(d, gaussian_taps(6.0), keep, where="blend", return_info=True)
    print(f"unsupported at sigma 6 with 64 x 64 holes: {info.unsupported} of {n * n}", flush=True)


def run(cmd, limit, cwd=ROOT):
    print("+", " ".join(cmd), f"(in {cwd})", flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd)
    if r.returncode != 0:
        print(f"step failed with status {r.returncode}: stopping", flush=True)
        sys.exit(r.returncode)


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
    run([sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--reps", str(a.reps), "--step", "kernel"], 400)
    if a.no_bench:
        return
    bench = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]
    for _ in range(2):
        run(bench, 300)
        if a.parent:
            run(bench, 300, cwd=os.path.abspath(a.parent))


if __name__ == "__main__":
    main()
