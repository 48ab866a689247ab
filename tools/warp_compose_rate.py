"""Rate of the one-resampling warp through a 2x3 matrix and a flow (Warper.tmat, include/microaligner_compose.h) against
the two-stage route it replaces (transform_img_with_tmat's affine warp, then Warper.warp()).

    python tools/warp_compose_rate.py [--size N] [--page-size N] [--reps K] [--no-prof] [--out DIR]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. device: N^2 (default 16384^2) uint16 and float32, device resident, every mode: Context.warp_affine_flow against
   Context.warp_affine + Context.warp (tile 1000, overlap 100), median of `reps` HIP-event timings of one call; for linear
   u16 also at 30 and 90 degrees (gather locality).  Bytes per pixel: flow 8 + source + output.
2. prof: step 1 once more under `rocprofv3 --kernel-trace --stats` (u16 and f32, linear, 3 degrees): the kernels' own
   times, to show what the float64 map costs beside the two-stage kernels.
3. pages: 8 uint16 host pages of N^2 (--page-size): Warper(tmat=...).warp_pages() against per-page transform_img_with_tmat
   followed by Warper.warp_pages(), wall time of one call, Gpix/s and the bytes that cross PCIe."""
import argparse
import glob
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

MODES = ["nearest", "linear", "cubic", "lanczos4"]


def tmat_deg(deg, n):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    cx = cy = n / 2
    return np.array([[c, -s, cx - c * cx + s * cy + 3.3], [s, c, cy - s * cx - c * cy - 2.1]])


def smooth_flow(n):
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32)
    return np.stack([2.7 + 1.5 * np.sin(xx / 300.0) * np.cos(yy / 500.0), -1.9 + 1.5 * np.cos(xx / 400.0)], -1).astype(np.float32)


def device_ms(ctx, fn, reps):
    out = []
    a, b = ctx.event(), ctx.event()
    for _ in range(reps):
        ctx.record(a)
        r = fn()
        ctx.record(b)
        out.append(ctx.elapsed_ms(a, b))
        del r
    return float(np.median(out))


def step_device(a, prof=False):
    from microaligner_amd.device import get_context
    ctx = get_context()
    n = a.size
    rng = np.random.default_rng(0)
    dflow = ctx.asdevice(smooth_flow(n))
    for dt in (np.uint16, np.float32):
        img = rng.integers(0, 65535, (n, n)).astype(dt)
        dimg = ctx.asdevice(img)
        del img
        bpp = 8 + 2 * np.dtype(dt).itemsize
        for mode in (["linear"] if prof else MODES):
            for deg in ([3] if prof or mode != "linear" or dt != np.uint16 else [3, 30, 90]):
                t = tmat_deg(deg, n)
                inv = np.linalg.pinv(np.append(t, [[0, 0, 1]], axis=0))
                one = lambda: ctx.warp_affine_flow(dimg, dflow, t, interpolation=mode)
                two = lambda: ctx.warp(ctx.warp_affine(dimg, inv), dflow, 1000, 100, interpolation=mode)
                one(), two()                                # tables, first launches
                reps = 2 if prof else a.reps
                ms1, ms2 = device_ms(ctx, one, reps), device_ms(ctx, two, reps)
                print(f"device {np.dtype(dt).name} {n}^2 {mode:8s} {deg:2d} deg: one resampling {ms1:7.2f} ms "
                      f"({n * n / ms1 / 1e6:5.1f} Gpix/s, {n * n * bpp / ms1 / 1e6:6.0f} GB/s at {bpp} B/px), "
                      f"two-stage {ms2:7.2f} ms, ratio {ms1 / ms2:.2f}", flush=True)
        dimg.free()


def step_pages(a):
    from microaligner_amd import Warper, transform_img_with_tmat
    from microaligner_amd.device import bind_to_device_numa, get_context
    bind_to_device_numa(0)
    ctx = get_context()
    P, n = a.page_size, 8
    rng = np.random.default_rng(1)
    page = rng.integers(0, 65535, (P, P), dtype=np.uint16)
    pages = [page ^ np.uint16(k) for k in range(n)]
    out = [np.ones_like(page) for _ in range(n)]
    t = tmat_deg(3, P)
    dflow = ctx.asdevice(smooth_flow(P))
    w = Warper()
    w.tmat, w.flow = t, dflow
    w.warp_pages(pages[:3], out[:3])
    t0 = time.perf_counter()
    w.warp_pages(pages, out)
    d1 = time.perf_counter() - t0
    w = Warper()
    w.flow = dflow
    w.warp_pages(pages[:3], out[:3])
    t0 = time.perf_counter()
    w.warp_pages(pages, out)
    dw = time.perf_counter() - t0
    t0 = time.perf_counter()
    aff = [transform_img_with_tmat(p, (P, P), t) for p in pages]
    w.warp_pages(aff, out)
    d2 = time.perf_counter() - t0
    gb = n * P * P * 2 / 1e9
    print(f"pages {n} u16 {P}^2: one resampling {d1 * 1e3:6.0f} ms = {n * P * P / d1 / 1e9:5.2f} Gpix/s, PCIe {2 * gb:.1f} GB; "
          f"two-stage {d2 * 1e3:6.0f} ms = {n * P * P / d2 / 1e9:5.2f} Gpix/s, PCIe {4 * gb:.1f} GB; "
          f"warp_pages alone {dw * 1e3:6.0f} ms = {n * P * P / dw / 1e9:5.2f} Gpix/s", flush=True)


def run(cmd, limit):
    print("+", " ".join(cmd), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT)
    if r.returncode != 0:
        print(f"step failed with status {r.returncode}: stopping", flush=True)
        sys.exit(r.returncode)


def prof_stats(out):
    """average kernel times of the warps from the profile (rocpd database, or the CSV of older rocprofv3 versions)"""
    import sqlite3
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        c = sqlite3.connect(path)
        rows += c.execute("select name, count(*), avg(end - start) from kernels group by name").fetchall()
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        import csv
        rows += [(r["Name"], int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(path))]
    for name, calls, avg_ns in sorted(rows, key=lambda r: -r[2]):
        if "compose" in name or "warp" in name:
            print(f"  {avg_ns / 1e6:8.3f} ms avg  {calls:4d} calls  {name[:110]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--page-size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--out", help="directory of the profile (default: a new temporary directory)")
    ap.add_argument("--step", choices=["device", "prof", "pages"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "device":
        return step_device(a)
    if a.step == "prof":
        return step_device(a, prof=True)
    if a.step == "pages":
        return step_pages(a)
    me = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--page-size", str(a.page_size), "--reps",
          str(a.reps)]
    run(me + ["--step", "device"], 300)
    if not a.no_prof:
        if not a.out:
            import tempfile
            a.out = tempfile.mkdtemp(prefix="warp_compose_prof_")
        print(f"profile: {a.out}", flush=True)
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.out, "-o", "warp_compose", "--"] + me + ["--step", "prof"], 300)
        prof_stats(a.out)
    run(me + ["--step", "pages"], 300)


if __name__ == "__main__":
    main()
