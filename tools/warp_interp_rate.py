"""Rate of the warp in each interpolation mode (nearest, linear, cubic, lanczos4).

    python tools/warp_interp_rate.py [--size N] [--page-size N] [--reps K] [--no-bind]

1. Device-resident Context.warp (tile 1000, overlap 100) of an N^2 (default 16384^2) uint16 and float32 image with a smooth
   subpixel flow: median of `reps` HIP-event timings of one call, ms and Gpix/s.
2. warp_pages on tools/page_rate.py's setup (8 uint16 pages of 16384^2, one flow (3.3, -2.1), pageable results): wall
   time of one call, Gpix/s, and the ratio to the linear mode."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from microaligner_amd import Warper
from microaligner_amd.device import bind_to_device_numa, get_context

MODES = ["nearest", "linear", "cubic", "lanczos4"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--page-size", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-bind", action="store_true")
    a = ap.parse_args()
    if not a.no_bind:
        bind_to_device_numa(0)
    ctx = get_context()
    H = W = a.size
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    flow = np.stack([2.7 + 1.5 * np.sin(xx / 300.0) * np.cos(yy / 500.0), -1.9 + 1.5 * np.cos(xx / 400.0)], -1).astype(np.float32)
    del yy, xx
    dflow = ctx.asdevice(flow)
    del flow
    for dt in (np.uint16, np.float32):
        img = rng.integers(0, 65535, (H, W)).astype(dt)
        dimg = ctx.asdevice(img)
        del img
        base = None
        for mode in MODES:
            ctx.warp(dimg, dflow, 1000, 100, interpolation=mode)     # tables, first launch
            ms = device_ms(ctx, lambda: ctx.warp(dimg, dflow, 1000, 100, interpolation=mode), a.reps)
            base = ms if mode == "linear" else base
            rel = f", {ms / base:.2f}x linear" if base and mode != "linear" else ""
            print(f"warp {np.dtype(dt).name} {H}x{W} {mode:9s}: {ms:7.2f} ms = {H * W / ms / 1e6:6.1f} Gpix/s{rel}", flush=True)
        dimg.free()
    dflow.free()
    ctx.trim()

    # warp_pages on tools/page_rate.py's setup
    P, n = a.page_size, 8
    page = rng.integers(0, 65535, (P, P), dtype=np.uint16)
    pages = [page ^ np.uint16(k) for k in range(n)]
    pflow = np.zeros((P, P, 2), np.float32)
    pflow[..., 0] = 3.3
    pflow[..., 1] = -2.1
    out = [np.zeros_like(page) for _ in range(n)]
    for o in out:
        o.fill(1)
    base = None
    for mode in MODES:
        w = Warper()
        w.interpolation = mode
        w.flow = ctx.asdevice(pflow)
        w.warp_pages(pages[:3], out[:3])
        t0 = time.perf_counter()
        w.warp_pages(pages, out)
        dt = time.perf_counter() - t0
        rate = n * P * P / dt / 1e9
        base = rate if mode == "linear" else base
        rel = f", {rate / base:.2f}x linear" if base and mode != "linear" else ""
        print(f"warp_pages {n} u16 pages {P}x{P} {mode:9s}: {dt * 1e3:6.0f} ms = {rate:5.1f} Gpix/s{rel}", flush=True)


if __name__ == "__main__":
    main()
