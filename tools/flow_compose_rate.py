"""Rate of the exact flow composition (Context.compose_flows, include/microaligner_flowcompose.h) against the reference's
merge it stands in for (Context.merge_flows, tile 1000 / overlap 100), and what OptFlowRegistrator.flow_composition = "exact"
costs in register().

    python tools/flow_compose_rate.py [--size N] [--reps K] [--no-prof] [--no-register] [--accuracy] [--out DIR]

One command; every GPU step is a child process under its own time limit, and the steps stop at the first that fails:
1. kernel: an N^2 (default 16384^2) device-resident pair of smooth flows of a few px: median of `reps` HIP-event timings of
   one call after a warm-up call, ms, GB/s at 24 B/px (8 read of second, 8 gathered from first, 8 written) and the share
   of the 8 TB/s HBM peak, for compose_flows and for merge_flows.
2. prof: step 1 once more under `rocprofv3 --kernel-trace --stats`: the kernels' own times.
3. register: register() on the cfg3-shaped pair (N^2 f32, num_pyr_lvl=4, full-resolution level, DOG, device resident) with
   engine="c", engine="python" and flow_composition="exact", alternating, `reps` rounds after a warm-up round: median and
   range of the wall time of a call (synchronised).
4. accuracy (--accuracy): the endpoint-error table of the README on the GPU (synthetic.make_pair(seed=1), float32,
   num_iterations=3, tile 1000 / overlap 100, no DOG, 64 px border left out)."""
import argparse
import glob
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HBM_PEAK_GBS = 8000.0
BPP = 24


def smooth_flows(n):
    """two smooth flows of a few px, built in row bands (float64 temporaries of a whole 16384^2 grid are 2 GiB each)"""
    first, second = np.empty((n, n, 2), np.float32), np.empty((n, n, 2), np.float32)
    xx = np.arange(n, dtype=np.float32)[None, :]
    for y0 in range(0, n, 1024):
        yy = np.arange(y0, min(y0 + 1024, n), dtype=np.float32)[:, None]
        first[y0:y0 + 1024, :, 0] = 2.7 + 1.5 * np.sin(xx / 300.0) * np.cos(yy / 500.0)
        first[y0:y0 + 1024, :, 1] = -1.9 + 1.5 * np.cos(xx / 400.0) + 0 * yy
        second[y0:y0 + 1024, :, 0] = -1.2 + 2.0 * np.cos(xx / 350.0 + yy / 450.0)
        second[y0:y0 + 1024, :, 1] = 0.8 + 1.7 * np.sin(yy / 280.0) + 0 * xx
    return first, second


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
    first, second = smooth_flows(n)
    d1, d2 = ctx.asdevice(first), ctx.asdevice(second)
    del first, second
    compose = lambda: ctx.compose_flows(d1, d2)
    merge = lambda: ctx.merge_flows(d1, d2, 1000, 100)
    compose(), merge()                                  # first launches, the output buffers
    reps = 2 if prof else a.reps
    for name, fn in (("compose_flows", compose), ("merge_flows t1000/o100", merge)):
        ms, lo, hi = device_ms(ctx, fn, reps)
        gbs = n * n * BPP / ms / 1e6
        print(f"kernel {n}^2 {name:24s}: {ms:7.3f} ms (min {lo:.3f}, max {hi:.3f}, {reps} calls), {gbs:6.0f} GB/s at {BPP} B/px, "
              f"{100 * gbs / HBM_PEAK_GBS:4.1f} % of {HBM_PEAK_GBS / 1000:.0f} TB/s", flush=True)


def step_register(a):
    from microaligner_amd import OptFlowRegistrator, synthetic
    from microaligner_amd.device import get_context
    ctx = get_context()
    n = a.size
    ref, mov = synthetic.make_pair(n, n, seed=1)
    dref, dmov = ctx.asdevice(ref), ctx.asdevice(mov)
    del ref, mov
    modes = (("engine=c", dict(engine="c")), ("engine=python", dict(engine="python")),
             ("flow_composition=exact", dict(flow_composition="exact")))
    times = {name: [] for name, _ in modes}
    for rnd in range(a.reps + 1):                       # round 0 warms up
        for name, kw in modes:
            reg = OptFlowRegistrator()
            reg.verbose = False
            reg.num_pyr_lvl, reg.use_full_res_img, reg.use_dog = 4, True, True
            for k, v in kw.items():
                setattr(reg, k, v)
            reg.ref_img, reg.mov_img = dref, dmov
            ctx.sync()
            t0 = time.perf_counter()
            flow = reg.register()
            ctx.sync()
            dt = (time.perf_counter() - t0) * 1e3
            if rnd:
                times[name].append(dt)
            accepted = [r.accepted for r in reg.level_reports]
            del flow
        print(f"round {rnd}: " + ", ".join(f"{k} {v[-1]:.1f} ms" for k, v in times.items() if v), flush=True)
    for name, t in times.items():
        print(f"register {n}^2 {name:24s}: median {np.median(t):7.1f} ms (min {min(t):.1f}, max {max(t):.1f}, {len(t)} calls)",
              flush=True)
    print("accepted (last call):", accepted, flush=True)


def step_accuracy(a):
    from microaligner_amd import OptFlowRegistrator, synthetic

    def err(flow, truth, border=64):
        d = (flow.astype(np.float64) - truth)[border:-border, border:-border]
        e = np.hypot(d[..., 0], d[..., 1])
        return f"{np.median(e):.3f} / {np.percentile(e, 99):.3f} / {e.max():.3f}"

    for n, full in ((1024, True), (2048, True), (1024, False)):
        ref, mov = synthetic.make_pair(n, n, seed=1)
        truth = np.stack(synthetic.displacement(n, n, dtype=np.float64), -1)
        row = []
        for mode in ("reference", "exact"):
            reg = OptFlowRegistrator()
            reg.verbose = False
            reg.num_pyr_lvl, reg.num_iterations, reg.tile_size, reg.overlap, reg.use_full_res_img = 3, 3, 1000, 100, full
            reg.flow_composition = mode
            reg.ref_img, reg.mov_img = ref, mov
            row.append(f"{mode}: {err(reg.register(), truth)} px {[r.accepted for r in reg.level_reports]}")
        print(f"accuracy {n}^2 num_pyr_lvl=3 full_res={full}, median / p99 / max: " + "; ".join(row), flush=True)


def run(cmd, limit):
    print("+", " ".join(cmd), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT)
    if r.returncode != 0:
        print(f"step failed with status {r.returncode}: stopping", flush=True)
        sys.exit(r.returncode)


def prof_stats(out):
    """average kernel times of the two kernels from the profile (rocpd database, or the CSV of older rocprofv3 versions)"""
    import sqlite3
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*.db"), recursive=True):
        c = sqlite3.connect(path)
        rows += c.execute("select name, count(*), avg(end - start) from kernels group by name").fetchall()
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        import csv
        rows += [(r["Name"], int(r["Calls"]), float(r["AverageNs"])) for r in csv.DictReader(open(path))]
    for name, calls, avg_ns in sorted(rows, key=lambda r: -r[2]):
        if "compose_flows" in name or "merge_flows" in name or "cell_max" in name or "window_" in name:
            print(f"  {avg_ns / 1e6:8.3f} ms avg  {calls:4d} calls  {name[:110]}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--no-register", action="store_true")
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--out", help="directory of the profile (default: a new temporary directory)")
    ap.add_argument("--step", choices=["kernel", "prof", "register", "accuracy"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step == "kernel":
        return step_kernel(a)
    if a.step == "prof":
        return step_kernel(a, prof=True)
    if a.step == "register":
        return step_register(a)
    if a.step == "accuracy":
        return step_accuracy(a)
    me = [sys.executable, os.path.abspath(__file__), "--size", str(a.size), "--reps", str(a.reps)]
    run(me + ["--step", "kernel"], 300)
    if not a.no_prof:
        if not a.out:
            import tempfile
            a.out = tempfile.mkdtemp(prefix="flow_compose_prof_")
        print(f"profile: {a.out}", flush=True)
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.out, "-o", "flow_compose", "--"] + me + ["--step", "prof"], 300)
        prof_stats(a.out)
    if not a.no_register:
        run(me + ["--step", "register"], 420)
    if a.accuracy:
        run(me + ["--step", "accuracy"], 300)


if __name__ == "__main__":
    main()
