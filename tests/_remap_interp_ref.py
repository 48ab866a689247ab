"""Loader of tests/c_ref/remap_interp_ref.c, the CPU restatement of cv2.remap's four interpolation modes (generic remap and
the tiled warp of Warper.warp()).

It includes oracle/ma_oracle.c and is compiled with gcc and the flags of oracle/Makefile (-ffp-contract=off: the
restatement follows OpenCV's operation order) into a directory the caller owns, a pytest temporary directory."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_ref", "remap_interp_ref.c")
CFLAGS = ["-O3", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall", "-Wextra",
          "-Wno-unused-parameter", "-Wno-unused-function"]
_DT = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}
MODES = {"nearest": 0, "linear": 1, "cubic": 2, "lanczos4": 4}
KSIZE = {"cubic": 4, "lanczos4": 8}


class InterpRef:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libremap_interp_ref.so")
        subprocess.run(["gcc"] + CFLAGS + ["-shared", "-I", os.path.join(ROOT, "oracle"), SRC, "-o", so, "-lm"],
                       check=True, capture_output=True)
        self.lib = L = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int
        L.orcx_interp_tables.restype = i
        L.orcx_interp_tables.argtypes = [i, vp, vp, vp]
        L.orcx_remap_interp.restype = i
        L.orcx_remap_interp.argtypes = [vp, i, i, i, i, vp, i, i, i, vp]
        L.orcx_warp_tiled_interp.restype = i
        L.orcx_warp_tiled_interp.argtypes = [vp, i, i, i, vp, i, i, i, vp, i, vp]

    def tables(self, mode):
        """(1-D table (32, k), float 2-D table (1024, k*k), int16 2-D table (1024, k*k)) of "cubic" / "lanczos4"."""
        k = KSIZE[mode]
        t1 = np.empty((32, k), np.float32)
        tf = np.empty((1024, k * k), np.float32)
        ti = np.empty((1024, k * k), np.int16)
        assert self.lib.orcx_interp_tables(MODES[mode], t1.ctypes.data, tf.ctypes.data, ti.ctypes.data) == k
        return t1, tf, ti

    def remap(self, src, map_xy, mode):
        """cv2.remap(src, map_xy, None, mode) with BORDER_CONSTANT 0"""
        src = np.ascontiguousarray(src)
        map_xy = np.ascontiguousarray(map_xy, np.float32)
        cn = 1 if src.ndim == 2 else src.shape[2]
        sh, sw = src.shape[:2]
        dh, dw = map_xy.shape[:2]
        dst = np.empty((dh, dw) if src.ndim == 2 else (dh, dw, cn), src.dtype)
        rc = self.lib.orcx_remap_interp(src.ctypes.data, _DT[src.dtype], cn, sh, sw, map_xy.ctypes.data, dh, dw,
                                        MODES[mode], dst.ctypes.data)
        if rc:
            raise RuntimeError(f"orcx_remap_interp failed with status {rc}")
        return dst

    def warp(self, img, flow, tile, overlap, mode, rows=None):
        """Warper.warp() with `mode`; rows: compute only these output rows (returned as (len(rows), W))"""
        img = np.ascontiguousarray(img)
        flow = np.ascontiguousarray(flow, np.float32)
        H, W = img.shape
        assert flow.shape == (H, W, 2)
        r = None if rows is None else np.ascontiguousarray(rows, np.int32)
        out = np.empty((H if r is None else len(r), W), img.dtype)
        rc = self.lib.orcx_warp_tiled_interp(img.ctypes.data, _DT[img.dtype], H, W, flow.ctypes.data, int(tile),
                                             int(overlap), MODES[mode], None if r is None else r.ctypes.data,
                                             0 if r is None else len(r), out.ctypes.data)
        if rc:
            raise RuntimeError(f"orcx_warp_tiled_interp failed with status {rc}")
        return out
