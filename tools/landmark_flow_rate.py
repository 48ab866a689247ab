"""Rate of the thin-plate spline of landmark pairs on the device (Context.landmark_flow / landmark_points,
include/microaligner_landmarks.h).

    python tools/landmark_flow_rate.py [--size N] [--points P] [--reps K]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails.  Each
time is the median of `reps` HIP-event timings of the C entry alone (records uploaded before) after a warm-up call, with
minimum and maximum; beside it the pixel-landmark pairs per second and the share of the float64 issue rate of 39.3 T
instructions/s that the compiled loop's count of float64 instructions per pair implies:
1. dense: the N^2 (default 16384^2) dense flow with n = 64 and n = 1024 landmarks.
2. grid: the stride-16 nodes with n = 1024, then Context.flow_grid_expand of them, and flow_grid_error of that grid against
   the dense flow of step 1's kind: what the bilinear expansion loses for this landmark set.
3. points: P (default 10^7) random points with n = 1024.
The landmarks lie one per cell of a lattice over the frame and follow a smooth deformation of up to 25 px plus 1 px of scatter;
the fit is the host's (its time is printed).  MICROALIGNER_HIP_LIB selects another build of the library (a -DLM_ROWS=n
variant, MA_HIPCC_EXTRA at build time; pass its instruction count with --flow-instr)."""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

F64_ISSUE = 39.3e12      # float64 vector instructions per second, the rate README.md uses
# float64 instructions per pixel-landmark pair in the compiled loops (gfx950, build.FLAGS): landmark_flow_kernel<4> 334 per
# landmark for 4 pixels (372 instructions of any kind), landmark_points_kernel 85 per landmark (102)
FLOW_INSTR, POINTS_INSTR = 334 / 4, 85.0


def landmarks(size, n, seed=0):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    cy, cx = np.divmod(rng.permutation(side * side)[:n], side)
    r = np.stack([(cx + 0.25 + 0.5 * rng.random(n)), (cy + 0.25 + 0.5 * rng.random(n))], axis=1) * (size - 1) / side
    f = np.stack([20 * np.sin(r[:, 0] / (size / 7)) * np.cos(r[:, 1] / (size / 9)) + 5, 15 * np.cos(r[:, 0] / (size / 6) + r[:, 1] / (size / 8)) - 3],
                 axis=1)
    return r, r - f + rng.normal(0, 1.0, (n, 2))


def fit(size, n):
    from microaligner_amd import fit_landmarks
    t0 = time.perf_counter()
    f = fit_landmarks(*landmarks(size, n), smoothing=1.0)
    print(f"fit of {n} landmarks on the host: {(time.perf_counter() - t0) * 1e3:.1f} ms; {f}", flush=True)
    return f


def device_ms(ctx, fn, reps):
    fn()                                                # warm-up
    out = []
    a, b = ctx.event(), ctx.event()
    for _ in range(reps):
        ctx.record(a)
        fn()
        ctx.record(b)
        out.append(ctx.elapsed_ms(a, b))
    return float(np.median(out)), min(out), max(out)


def report(what, pairs, instr, ms, lo, hi, reps):
    rate = pairs / (ms * 1e-3)
    print(f"{what}: {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} calls); {rate:.3e} pairs/s; at {instr:.1f} float64 instructions per "
          f"pair {100 * rate * instr / F64_ISSUE:.1f} % of {F64_ISSUE / 1e12:.1f} T instructions/s", flush=True)


def flow_call(ctx, f, size, stride, out):
    d_cw = ctx._upload_raw(f.cw)
    a6 = (C.c_double * 6)(*f.a6)
    return d_cw, lambda: ctx._run(ctx.lib.ma_landmark_flow, d_cw.ptr, len(f), a6, float(f.c[0]), float(f.c[1]), f.k, size, size,
                                  stride, out.ptr)


def step_dense(a):
    from microaligner_amd.device import get_context
    ctx = get_context()
    out = ctx.empty((a.size, a.size, 2), np.float32)
    for n in (64, 1024):
        f = fit(a.size, n)
        keep, call = flow_call(ctx, f, a.size, 1, out)
        report(f"dense {a.size}^2, n = {n}", a.size * a.size * n, a.flow_instr, *device_ms(ctx, call, a.reps), a.reps)


def step_grid(a):
    from microaligner_amd.device import FlowGrid, get_context, grid_nodes
    ctx = get_context()
    f = fit(a.size, 1024)
    g = grid_nodes(a.size, 16)
    nodes = ctx.empty((g, g, 2), np.float32)
    keep, call = flow_call(ctx, f, a.size, 16, nodes)
    report(f"stride 16 of {a.size}^2 ({g}^2 nodes), n = 1024", g * g * 1024, a.flow_instr, *device_ms(ctx, call, a.reps), a.reps)
    grid = FlowGrid(nodes, 16, (a.size, a.size))
    ms, lo, hi = device_ms(ctx, lambda: ctx.flow_grid_expand(grid), a.reps)
    print(f"flow_grid_expand of those nodes: {ms:9.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls)", flush=True)
    dense = ctx.landmark_flow(f.cw, f.a6, f.c, f.k, (a.size, a.size), 1)
    max_err, above, invalid = ctx.flow_grid_error(dense, grid, 1024, 1024, 1.0 / 32)
    print(f"flow_grid_error of the stride-16 grid against the dense flow: max {float(max_err.max()):.5f} px, "
          f"{int(above.sum())} pixels above 1/32 px, {int(invalid.sum())} invalid", flush=True)


def step_points(a):
    from microaligner_amd.device import get_context
    ctx = get_context()
    f = fit(a.size, 1024)
    pts = np.random.default_rng(1).uniform(0, a.size - 1, (a.points, 2))
    d_cw, d_pts, d_out = ctx._upload_raw(f.cw), ctx._upload_raw(pts), ctx._raw(a.points * 16)
    a6 = (C.c_double * 6)(*f.a6)
    call = lambda: ctx._run(ctx.lib.ma_landmark_points, d_cw.ptr, len(f), a6, float(f.c[0]), float(f.c[1]), f.k, d_pts.ptr,
                            a.points, d_out.ptr)
    report(f"{a.points} points, n = 1024", a.points * 1024, a.points_instr, *device_ms(ctx, call, a.reps), a.reps)


def run(cmd, limit):
    print("+", " ".join(cmd), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT)
    if r.returncode != 0:
        print(f"step failed with status {r.returncode}: stopping", flush=True)
        sys.exit(r.returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--points", type=int, default=10 ** 7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--flow-instr", type=float, default=FLOW_INSTR, help="float64 instructions per pair of landmark_flow_kernel")
    ap.add_argument("--points-instr", type=float, default=POINTS_INSTR, help="float64 instructions per pair of landmark_points_kernel")
    ap.add_argument("--step", choices=["dense", "grid", "points"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return {"dense": step_dense, "grid": step_grid, "points": step_points}[a.step](a)
    me = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--points", str(a.points), "--reps", str(a.reps),
          "--flow-instr", str(a.flow_instr), "--points-instr", str(a.points_instr)]
    for step in ("dense", "grid", "points"):
        run(me + ["--step", step], 300)


if __name__ == "__main__":
    main()
