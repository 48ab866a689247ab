"""Rate of the affine moments of a flow (Context.flow_affine_moments) and of apply(flow, A) (Context.flow_affine_apply),
include/microaligner_flowaffine.h.

    python tools/flow_affine_rate.py [--size N] [--reps K] [--parent DIR] [--no-bench]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident smooth flow of up to 25 px (the test suite's flow B).  Per case the median
   of `reps` HIP-event timings of one call after a warm-up call, with minimum and maximum, and the bytes the case must move
   (8 B/px of flow, the weight's 4 or 1 B/px, 8 B/px more for apply's output) over that time against the 8 TB/s peak: the
   moments pass with no weight, a float32 map, a uint8 mask and a per-cell map (one cell, and cells of 1000), the pass at
   cell_size=1000 without a weight, the pass with a prior and a clip, and the apply pass out of place and in place;
   Context.qc_flow_grid at cells of 1000 -- the call behind flow_qc(), whose flow pass is qc_flow_tile_kernel -- and Context.compose_flows on the same box as the yardsticks.
2. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PEAK_TBS = 8.0


def flow_b(n):
    """the test suite's flow B on an n^2 grid, built in row bands"""
    f = np.empty((n, n, 2), np.float32)
    xx = np.arange(n, dtype=np.float32)[None, :]
    for y0 in range(0, n, 1024):
        yy = np.arange(y0, min(y0 + 1024, n), dtype=np.float32)[:, None]
        f[y0:y0 + 1024, :, 0] = 20 * np.sin(xx / 90) * np.cos(yy / 70) + 5
        f[y0:y0 + 1024, :, 1] = 15 * np.cos(xx / 110 + yy / 80) - 3
    return f


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
    from microaligner_amd.device import get_context
    ctx = get_context()
    n = a.size
    d = ctx.asdevice(flow_b(n))
    rng = np.random.default_rng(0)
    w32 = ctx.asdevice(rng.uniform(0.5, 1.5, (n, n)).astype(np.float32))
    w8 = ctx.asdevice((rng.random((n, n)) < 0.9).astype(np.uint8))
    g = -(-n // 1000)
    one, cells = ctx.asdevice(np.ones((1, 1), np.float32)), ctx.asdevice(rng.uniform(0.5, 1.5, (g, g)).astype(np.float32))
    prior = np.array([[1.0, 0.0, 5.0], [0.0, 1.0, -3.0]])
    mat = np.array([[1.001, -0.002, 3.0], [0.002, 0.999, -2.0]])
    out = ctx.empty((n, n, 2), np.float32)
    scratch = d.copy()
    cases = [("moments, no weight              ", 8, lambda: ctx.flow_affine_moments(d)),
             ("moments, float32 weight         ", 12, lambda: ctx.flow_affine_moments(d, w32)),
             ("moments, uint8 mask             ", 9, lambda: ctx.flow_affine_moments(d, w8)),
             ("moments, per-cell weight, 1 cell", 8, lambda: ctx.flow_affine_moments(d, one, (n, n))),
             ("moments, per-cell weight, 1000  ", 8, lambda: ctx.flow_affine_moments(d, cells, 1000)),
             ("moments, cell_size 1000         ", 8, lambda: ctx.flow_affine_moments(d, None, 1000)),
             ("moments, prior and clip 4 px    ", 8, lambda: ctx.flow_affine_moments(d, None, None, prior, 4.0)),
             ("apply, out of place             ", 16, lambda: ctx.flow_affine_apply(d, mat, out=out)),
             ("apply, in place                 ", 16, lambda: ctx.flow_affine_apply(scratch, mat, out=scratch)),
             ("qc_flow_grid 1000 (yardstick)   ", 8, lambda: ctx.qc_flow_grid(d, 1000, 1000)),
             ("compose_flows (yardstick)       ", 24, lambda: ctx.compose_flows(d, d))]
    for name, bpp, fn in cases:
        r = fn()                                        # first launch, the buffers
        del r
        ctx.sync()
        ms, lo, hi = device_ms(ctx, fn, a.reps)
        tbs = n * n * bpp / ms / 1e9
        print(f"kernel {n}^2 {name}: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls), "
              f"{n * n / ms / 1e6:7.2f} Gpx/s, {bpp:2d} B/px = {tbs:5.2f} TB/s = {100 * tbs / PEAK_TBS:4.1f} % of peak", flush=True)
    _, counts = ctx.flow_affine_moments(d, None, None, prior, 4.0)
    print(f"used / invalid / unweighted / trimmed with the prior: {counts[0, 0].tolist()}", flush=True)


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
