"""Rate of the flat grey morphology (Context.morphology), include/microaligner_morphology.h.

    python tools/morphology_rate.py [--size N] [--reps K] [--parent DIR] [--no-prof] [--no-bench] [--out DIR]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident image (the pattern of tools/texture_rate.py) as uint8, uint16 and
   float32; "erode" and "tophat" at r = 1, 8, 64 and 255.  Per case the median of `reps` HIP-event timings of one call after
   a warm-up call, with minimum and maximum, the bytes the call moves to and from memory (every launch reads a plane and
   writes a plane; the last launch of a hat reads the image as well) and their share of 8 TB/s.  The yardstick on the same
   box: Context.fold_mask (margin 4) of a flow of the same size, the package's other dilation.
2. prof: step 1 once more under `rocprofv3 --kernel-trace --stats`: the kernels' own times, largest first.
3. bench: `python bench.py --gpus 1 --steps 3 --warmup 1` for this tree and, with --parent DIR (a built checkout of the
   parent commit), for that tree, alternating, twice each: the JSON result lines as they come."""
import argparse
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from flow_smooth_rate import device_ms, flow_b, run
from texture_rate import image

PEAK = 8e12   # bytes per second


def moved_bytes(n, itemsize, op):
    """bytes read and written by the launches of one call on an n^2 image"""
    launches = 2 if op in ("erode", "dilate") else 4
    planes = 2 * launches + (1 if op in ("tophat", "blackhat") else 0)
    return planes * n * n * itemsize


def step_kernel(a):
    from microaligner_amd.device import get_context
    ctx = get_context()
    n = a.size
    for dtype in (np.uint8, np.uint16, np.float32):
        host, _ = image(n, dtype)
        d_img = ctx.asdevice(host)
        del host
        ctx._resident.clear()
        out = ctx.empty((n, n), dtype)
        for op in ("erode", "tophat"):
            for r in (1, 8, 64, 255):
                fn = lambda o=op, q=r: ctx.morphology(d_img, o, q, out=out)       # noqa: E731
                fn()                                        # first launch, the buffers
                ms, lo, hi = device_ms(ctx, fn, a.reps)
                nbytes = moved_bytes(n, np.dtype(dtype).itemsize, op)
                print(f"kernel {n}^2 morphology {np.dtype(dtype).name:7s} {op:6s} r={r:3d}: {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, "
                      f"{a.reps} calls), {n * n / ms / 1e6:7.2f} Gpx/s, {nbytes / 1e9:6.2f} GB moved, "
                      f"{nbytes / (ms * 1e-3) / PEAK:5.3f} of 8 TB/s", flush=True)
        del d_img, out
        ctx.trim()
    d = ctx.asdevice(flow_b(n))
    fn = lambda: ctx.fold_mask(d, 4)       # noqa: E731
    r = fn()
    del r
    ms, lo, hi = device_ms(ctx, fn, a.reps)
    print(f"kernel {n}^2 fold_mask margin 4 (yardstick): {ms:8.3f} ms (min {lo:.3f}, max {hi:.3f}, {a.reps} calls), "
          f"{n * n / ms / 1e6:7.2f} Gpx/s", flush=True)


def prof_stats(out):
    """calls, average and total time of the morphology kernels from the profile (rocpd database, or the CSV of older
    rocprofv3 versions)"""
    import sqlite3
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        c = sqlite3.connect(path)
        rows += c.execute("select name, count(*), avg(end - start) from kernels group by name").fetchall()
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        import csv
        rows += [(r["Name"], int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(path))]
    for name, calls, avg_ns in sorted(rows, key=lambda r: -r[1] * r[2]):
        if "mo_pass" in name or "fs_" in name:
            print(f"  {avg_ns / 1e6:8.4f} ms avg  {calls:4d} calls  {calls * avg_ns / 1e6:9.3f} ms in all  {name[:100]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent", help="a built checkout of the parent commit, benchmarked in turns with this tree")
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--out", help="directory of the profile (default: a new temporary directory)")
    ap.add_argument("--step", choices=["kernel"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a)
    me = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--reps", str(a.reps), "--step", "kernel"]
    run(me, 500)
    if not a.no_prof:
        if not a.out:
            import tempfile
            a.out = tempfile.mkdtemp(prefix="morphology_prof_")
        print(f"profile: {a.out}", flush=True)
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.out, "-o", "morphology", "--"] + me, 500)
        prof_stats(a.out)
    if a.no_bench:
        return
    bench = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]
    for _ in range(2):
        run(bench, 300)
        if a.parent:
            run(bench, 300, cwd=os.path.abspath(a.parent))


if __name__ == "__main__":
    main()
