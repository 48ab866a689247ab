"""Loader of tests/c_ref/farneback_levels_ref.c, the CPU restatement of cv2.calcOpticalFlowFarneback with levels > 0.

It includes oracle/ma_oracle.c and is compiled with gcc and the flags of oracle/Makefile (-ffp-contract=off: the
restatement follows OpenCV's operation order) into a directory the caller owns, a pytest temporary directory."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c_ref", "farneback_levels_ref.c")
CFLAGS = ["-O3", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall", "-Wextra",
          "-Wno-unused-parameter", "-Wno-unused-function"]
_DT = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}


class LevelsRef:
    def __init__(self, build_dir):
        so = os.path.join(str(build_dir), "libfb_levels_ref.so")
        subprocess.run(["gcc"] + CFLAGS + ["-shared", "-I", os.path.join(ROOT, "oracle"), SRC, "-o", so, "-lm"],
                       check=True, capture_output=True)
        self.lib = L = C.CDLL(so)
        ip, dp, vp, fp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_float)
        L.orcx_level_table.restype = C.c_int
        L.orcx_level_table.argtypes = [C.c_int, C.c_int, C.c_int, ip, ip, ip, dp]
        L.orcx_resize_linear_f32.restype = C.c_int
        L.orcx_resize_linear_f32.argtypes = [fp, C.c_int, C.c_int, C.c_int, fp, C.c_int, C.c_int, C.c_int]
        L.orcx_farneback_levels.restype = C.c_int
        L.orcx_farneback_levels.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_double, C.c_int, fp]
        L.orc_set_threads.restype = None
        L.orc_set_threads.argtypes = [C.c_int]

    def set_threads(self, n):
        self.lib.orc_set_threads(int(n))

    def level_table(self, H, W, levels):
        """[(w_k, h_k, ksize_k, sigma_k) for k = 0 .. kept levels]"""
        n = max(int(levels), 0) + 1
        w, h, k = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        s = (C.c_double * n)()
        kept = self.lib.orcx_level_table(H, W, levels, w, h, k, s)
        return [(w[i], h[i], k[i], s[i]) for i in range(kept + 1)]

    def resize_linear(self, src, dsize, fused=False):
        """cv2.resize(src, dsize=(dw, dh), interpolation=INTER_LINEAR) of a float32 (h, w) or (h, w, cn) image"""
        src = np.ascontiguousarray(src, np.float32)
        cn = 1 if src.ndim == 2 else src.shape[2]
        dw, dh = dsize
        dst = np.empty((dh, dw) + (() if src.ndim == 2 else (cn,)), np.float32)
        fp = C.POINTER(C.c_float)
        rc = self.lib.orcx_resize_linear_f32(src.ctypes.data_as(fp), cn, src.shape[0], src.shape[1],
                                             dst.ctypes.data_as(fp), dh, dw, int(fused))
        if rc:
            raise RuntimeError(f"orcx_resize_linear_f32 failed with status {rc}")
        return dst

    def farneback(self, prev, nxt, levels, winsize, iterations, poly_n=1, poly_sigma=1.7, fused=False):
        """cv2.calcOpticalFlowFarneback(prev, nxt, None, 0.5, levels, winsize, iterations, poly_n, poly_sigma,
        OPTFLOW_FARNEBACK_GAUSSIAN); a mixed-dtype pair is the float32 pair, as OpenCV converts each image"""
        prev, nxt = np.ascontiguousarray(prev), np.ascontiguousarray(nxt)
        if prev.dtype != nxt.dtype:
            prev, nxt = prev.astype(np.float32), nxt.astype(np.float32)
        h, w = prev.shape
        flow = np.empty((h, w, 2), np.float32)
        rc = self.lib.orcx_farneback_levels(prev.ctypes.data, nxt.ctypes.data, _DT[prev.dtype], h, w, int(levels),
                                            int(winsize), int(iterations), int(poly_n), float(poly_sigma), int(fused),
                                            flow.ctypes.data_as(C.POINTER(C.c_float)))
        if rc:
            raise RuntimeError(f"orcx_farneback_levels failed with status {rc}")
        return flow
