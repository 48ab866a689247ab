"""What grid flows (FlowGrid, include/microaligner_flowgrid.h) lose on real registrations and what they cost.

    python tools/flow_grid_rate.py [--size N] [--loss-size N] [--reps K] [--no-prof] [--out DIR]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. loss: register() on synthetic.make_pair(2048, 2048, seed=1) with the settings of the README's exact-composition table
   and on the cfg3 pair (--loss-size, default 16384), then flow_grid_error at strides 2 .. 64: the global max_err, the
   share of pixels above 1/32 px, the 99th percentile (sides up to 4096: it needs the expanded flow on the host) and the
   stride compress_flow picks at tol = 1/32.
2. warp: N^2 (default 16384^2) uint16 and float32, device resident, linear and nearest, identity matrix: (a) the dense
   Context.warp_affine_flow, (b) Context.flow_grid_expand followed by (a), (c) Context.warp_affine_grid at strides 8 and
   32.  HIP events around one call; a warm-up, then `reps` rounds with the four alternating; median (minimum - maximum).
3. points: transform_points of 10^7 points from a stride-8 grid against the dense flow, wall time of a call (upload,
   kernel, download), both directions, alternating.
4. prof: steps 2 and 3 once more with 2 rounds under `rocprofv3 --kernel-trace --stats`: the kernels' own times."""
import argparse
import glob
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

STRIDES = (2, 4, 8, 16, 32, 64)


def smooth_flow(n):
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32)
    return np.stack([2.7 + 1.5 * np.sin(xx / 300.0) * np.cos(yy / 500.0), -1.9 + 1.5 * np.cos(xx / 400.0)], -1).astype(np.float32)


def stats(ms):
    return f"{np.median(ms):8.3f} ms ({min(ms):.3f} - {max(ms):.3f})"


def step_loss(a):
    from microaligner_amd import OptFlowRegistrator, compress_flow, flow_grid_error, synthetic
    from microaligner_amd.device import get_context
    ctx = get_context()
    pairs = [("2048^2, exact composition, 3 levels, no DOG", 2048,
              dict(num_pyr_lvl=3, num_iterations=3, tile_size=1000, overlap=100, use_full_res_img=True, use_dog=False,
                   flow_composition="exact")),
             (f"{a.loss_size}^2, cfg3 (4 levels, full resolution, DOG)", a.loss_size,
              dict(num_pyr_lvl=4, use_full_res_img=True, use_dog=True))]
    for name, n, params in pairs:
        ref, mov = synthetic.make_pair(n, n, seed=1)
        reg = OptFlowRegistrator()
        for k, v in params.items():
            setattr(reg, k, v)
        reg.ref_img, reg.mov_img = ctx.asdevice(ref), ctx.asdevice(mov)
        flow = ctx.asdevice(reg.register())
        host = flow.numpy() if n <= 4096 else None
        print(f"loss {name}: max |flow| {float(np.abs(host).max()) if host is not None else float('nan'):.2f} px", flush=True)
        for s in STRIDES:
            grid, err = compress_flow(flow, stride=s, return_error=True)
            p99 = "not measured"
            if host is not None:
                p99 = f"{np.percentile(np.abs(grid.expand().numpy() - host).max(-1), 99):.5f} px"
            print(f"  stride {s:2d}: max_err {err.global_max_err:.5f} px, above 1/32 px {err.above.sum() / (n * n):.3e} of the "
                  f"pixels, invalid {int(err.invalid.sum())}, p99 {p99}, {grid.nbytes / 1e6:.2f} MB against "
                  f"{flow.nbytes / 1e6:.0f} MB", flush=True)
        t0 = time.perf_counter()
        grid, err = compress_flow(flow, return_error=True)
        print(f"  compress_flow at tol 1/32 picks stride {grid.stride} (max_err {err.global_max_err:.5f} px) in "
              f"{(time.perf_counter() - t0) * 1e3:.0f} ms", flush=True)
        del flow, reg


def step_warp(a, prof=False):
    from microaligner_amd.device import get_context
    ctx = get_context()
    n, reps = a.size, 2 if prof else a.reps
    rng = np.random.default_rng(0)
    dflow = ctx.asdevice(smooth_flow(n))
    grids = {s: ctx.flow_grid_sample(dflow, s) for s in (8, 32)}
    ident = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    ev0, ev1 = ctx.event(), ctx.event()

    def timed(fn):
        ctx.record(ev0)
        r = fn()
        ctx.record(ev1)
        ms = ctx.elapsed_ms(ev0, ev1)
        del r
        return ms

    for dt in (np.uint16, np.float32):
        dimg = ctx.asdevice(rng.integers(0, 65535, (n, n)).astype(dt))
        for mode in ("linear", "nearest"):
            calls = {"(a) dense": lambda: ctx.warp_affine_flow(dimg, dflow, ident, interpolation=mode),
                     "(b) expand 8 + dense": lambda: ctx.warp_affine_flow(dimg, ctx.flow_grid_expand(grids[8]), ident,
                                                                         interpolation=mode),
                     "(c) grid 8": lambda: ctx.warp_affine_grid(dimg, grids[8], interpolation=mode),
                     "(c) grid 32": lambda: ctx.warp_affine_grid(dimg, grids[32], interpolation=mode)}
            for fn in calls.values():
                timed(fn)                                     # tables, first launches, the pool's buffers
            ms = {k: [] for k in calls}
            for _ in range(reps):
                for k, fn in calls.items():
                    ms[k].append(timed(fn))
            for k in calls:
                print(f"warp {np.dtype(dt).name} {n}^2 {mode:8s} {k:22s} {stats(ms[k])}", flush=True)
            b, c = ms["(b) expand 8 + dense"], ms["(c) grid 8"]
            print(f"  (b) - (c) = {np.median(b) - np.median(c):.3f} ms, spread of (b) {max(b) - min(b):.3f} ms", flush=True)
        dimg.free()


def step_points(a, prof=False):
    from microaligner_amd import transform_points
    from microaligner_amd.device import get_context
    ctx = get_context()
    n, reps = a.size, 2 if prof else a.reps
    dflow = ctx.asdevice(smooth_flow(n))
    grid = ctx.flow_grid_sample(dflow, 8)
    rng = np.random.default_rng(2)
    pts = rng.uniform(0, n - 1, (10 ** 7, 2))
    for direction in ("to_moving", "to_reference"):
        calls = {"dense": lambda: transform_points(pts, dflow, direction), "grid 8": lambda: transform_points(pts, grid, direction)}
        outs = {k: fn() for k, fn in calls.items()}
        ms = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        for k in calls:
            print(f"points 1e7 {direction:12s} {k:8s} {stats(ms[k])}", flush=True)
        print(f"  max |grid - dense| = {np.abs(outs['grid 8'] - outs['dense']).max():.2e} px", flush=True)


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
        if any(k in name for k in ("compose", "fg_", "transform_points")):
            print(f"  {avg_ns / 1e6:8.3f} ms avg  {calls:4d} calls  {name[:130]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--loss-size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--out", help="directory of the profile (default: a new temporary directory)")
    ap.add_argument("--step", choices=["loss", "warp", "points", "prof"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "loss":
        return step_loss(a)
    if a.step == "warp":
        return step_warp(a)
    if a.step == "points":
        return step_points(a)
    if a.step == "prof":
        step_warp(a, prof=True)
        return step_points(a, prof=True)
    me = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--loss-size", str(a.loss_size), "--reps", str(a.reps)]
    run(me + ["--step", "loss"], 420)
    run(me + ["--step", "warp"], 300)
    run(me + ["--step", "points"], 300)
    if not a.no_prof:
        if not a.out:
            import tempfile
            a.out = tempfile.mkdtemp(prefix="flow_grid_prof_")
        print(f"profile: {a.out}", flush=True)
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.out, "-o", "flow_grid", "--"] + me + ["--step", "prof"], 420)
        prof_stats(a.out)


if __name__ == "__main__":
    main()
