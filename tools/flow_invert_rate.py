"""Rate of the dense flow inverse (Context.invert_flow) and of the point transforms (Context.transform_points),
include/microaligner_flowinvert.h.

    python tools/flow_invert_rate.py [--size N] [--points P] [--reps K] [--no-prof] [--out DIR]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident smooth flow of up to 25 px (the test suite's flow B): median of `reps`
   HIP-event timings of one invert_flow call (max_iter 50, tol 1e-3) after a warm-up call; the pixels that did not
   converge; mean and maximum steps per pixel, exact, from not_converged at max_iter = 1, 2, ... (a pixel's iterates do
   not depend on max_iter, so not_converged(k) counts the pixels that need more than k steps); compose_flows on the same
   box, and steps_mean x that time: what one launch per step would cost.
2. points: P (default 10^7) random points in both directions, tol 1e-4: wall time of Context.transform_points (upload of
   the points, kernel, download of points and flags) and HIP-event time of the kernel alone.
3. prof: step 1's calls once more under `rocprofv3 --kernel-trace --stats`: the kernels' own times.
MICROALIGNER_HIP_LIB selects another build of the library (a -DFI_ROWS=n variant, MA_HIPCC_EXTRA at build time)."""
import argparse
import glob
import os
import subprocess
import sys
import time

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


def step_kernel(a, prof=False):
    from microaligner_amd.device import get_context
    ctx = get_context()
    n = a.size
    d = ctx.asdevice(flow_b(n))
    invert = lambda: ctx.invert_flow(d, 50, 1e-3)
    g = invert()                                        # first launch, the output buffer
    compose = lambda: ctx.compose_flows(d, g)
    compose()
    reps = 2 if prof else a.reps
    ms, lo, hi = device_ms(ctx, invert, reps)
    print(f"kernel {n}^2 invert_flow (max_iter 50, tol 1e-3): {ms:7.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} calls)", flush=True)
    cms, lo, hi = device_ms(ctx, compose, reps)
    print(f"kernel {n}^2 compose_flows                      : {cms:7.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} calls)", flush=True)
    if prof:
        return
    _, info = ctx.invert_flow(d, 50, 1e-3, return_info=True)
    print(f"not converged after 50 steps: {info.not_converged} of {n * n}", flush=True)
    del info
    more, k = [], 1                                     # more[k - 1]: pixels that need more than k steps
    while k <= 50:
        more.append(ctx.invert_flow(d, k, 1e-3, return_info=True)[1].not_converged)
        if more[-1] == 0:
            break
        k += 1
    mean = 1 + sum(more) / (n * n)
    print(f"steps per pixel: mean {mean:.2f}, max {len(more)}; a launch per step at compose_flows' rate: "
          f"{mean:.2f} x {cms:.3f} = {mean * cms:.2f} ms mean, {len(more)} x {cms:.3f} = {len(more) * cms:.2f} ms to the last pixel; "
          f"one launch: {ms:.3f} ms", flush=True)


def step_points(a):
    from microaligner_amd import _lib as L
    from microaligner_amd.device import get_context
    ctx = get_context()
    n, p = a.size, a.points
    d = ctx.asdevice(flow_b(n))
    rng = np.random.default_rng(0)
    pts = rng.uniform(0, n - 1, (p, 2))
    for direction, code in (("to_moving", L.MA_POINTS_TO_MOVING), ("to_reference", L.MA_POINTS_TO_REFERENCE)):
        ctx.transform_points(pts, d, direction)         # warm-up
        wall = []
        for _ in range(a.reps):
            ctx.sync()
            t0 = time.perf_counter()
            out, info = ctx.transform_points(pts, d, direction, return_info=True)
            wall.append((time.perf_counter() - t0) * 1e3)
        d_pts, d_out, d_cv, d_in = ctx._upload_raw(pts), ctx._raw(p * 16), ctx._raw(p), ctx._raw(p)
        kern = lambda: ctx._run(ctx.lib.ma_transform_points, d_pts.ptr, p, d.ptr, n, n, None, None, 0, 0, code, 50, 1e-4,
                                d_out.ptr, d_cv.ptr, d_in.ptr)
        kern()
        ms, lo, hi = device_ms(ctx, kern, a.reps)
        print(f"points {p} {direction:12s} on {n}^2: with transfers {np.median(wall):8.2f} ms (min {min(wall):.2f}, max "
              f"{max(wall):.2f}), kernel {ms:7.3f} ms (min {lo:.3f}, max {hi:.3f}), {a.reps} calls; converged "
              f"{info.converged.mean():.4f}, inside {info.inside.mean():.4f}", flush=True)


def run(cmd, limit):
    print("+", " ".join(cmd), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT)
    if r.returncode != 0:
        print(f"step failed with status {r.returncode}: stopping", flush=True)
        sys.exit(r.returncode)


def prof_stats(out):
    """average kernel times from the profile (rocpd database, or the CSV of older rocprofv3 versions)"""
    import sqlite3
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        c = sqlite3.connect(path)
        rows += c.execute("select name, count(*), avg(end - start) from kernels group by name").fetchall()
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        import csv
        rows += [(r["Name"], int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(path))]
    for name, calls, avg_ns in sorted(rows, key=lambda r: -r[2]):
        if "invert_flow" in name or "compose_flows" in name or "transform_points" in name:
            print(f"  {avg_ns / 1e6:8.3f} ms avg  {calls:4d} calls  {name[:110]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--points", type=int, default=10 ** 7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--no-points", action="store_true")
    ap.add_argument("--out", help="directory of the profile (default: a new temporary directory)")
    ap.add_argument("--step", choices=["kernel", "prof", "points"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a)
    if a.step == "prof":
        return step_kernel(a, prof=True)
    if a.step == "points":
        return step_points(a)
    me = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--points", str(a.points), "--reps", str(a.reps)]
    run(me + ["--step", "kernel"], 300)
    if not a.no_points:
        run(me + ["--step", "points"], 300)
    if not a.no_prof:
        if not a.out:
            import tempfile
            a.out = tempfile.mkdtemp(prefix="flow_invert_prof_")
        print(f"profile: {a.out}", flush=True)
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.out, "-o", "flow_invert", "--"] + me + ["--step", "prof"], 300)
        prof_stats(a.out)


if __name__ == "__main__":
    main()
