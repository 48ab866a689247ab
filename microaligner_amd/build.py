"""Build recipe for libmicroaligner_hip.so (hipcc, gfx950 only, in-tree).

    python -m microaligner_amd.build [--force]

-ffp-contract=off is load-bearing: the kernels follow OpenCV's operation order
(multiply and add as separate roundings) and must not be fused by the compiler;
fused multiply-adds are written explicitly where a mode asks for them.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmicroaligner_hip.so")
SOURCES = ["ma_api.hip", "farneback.hip", "remap.hip", "pyramid.hip", "dog.hip", "nmi.hip", "affine.hip", "knn.hip", "daisy.hip", "ransac.hip", "feature_round.hip", "register.hip", "probe.hip", "qc.hip", "remap_interp.hip", "warp_compose.hip", "page_pipeline.hip",
           "flow_compose.hip", "flow_invert.hip", "residual_shift.hip", "flow_grid.hip", "flow_smooth.hip", "flow_affine.hip", "texture.hip", "direct_affine.hip", "flow_refine.hip",
           "landmarks.hip", "translation.hip", "quantile.hip", "local_correlation.hip", "flow_median.hip", "flow_fill.hip", "debug_fill.hip",
           "local_norm.hip", "morphology.hip", "components.hip"]


def _inc(name):
    """a public header"""
    return os.path.join(HERE, "..", "include", name)


HEADERS = [os.path.join(CSRC, "ma_internal.h"), os.path.join(CSRC, "remap_common.h"), os.path.join(CSRC, "nmi_score.h"),
           _inc("microaligner_hip.h")]
# headers of single sources that are off the measured path (not in HEADERS, so not in source_hash())
_SMOOTH_H = _inc("microaligner_flowsmooth.h")            # the weight kinds, for the sources that take a weight
_INTERP_HEADERS = [_inc("microaligner_interp.h"), os.path.join(CSRC, "remap_interp.h")]
_CELL_GRID = os.path.join(CSRC, "cell_grid.h")
_FLOW_GRID = [_inc("microaligner_flowgrid.h"), os.path.join(CSRC, "flow_grid_eval.h")]
_FLOW_JACOBIAN = os.path.join(CSRC, "flow_jacobian.h")   # det J, stated once for the quality maps and the fold mask
# the separable FIR tile of the smoothing, the texture maps, the refinement, the local correlation maps and the local
# contrast normalisation
_WINDOW_FIR = os.path.join(CSRC, "window_fir.h")
# the weight argument of the eight calls that take one: its readers on the device, its check and dispatch at the C entry
_WEIGHT_MAP = os.path.join(CSRC, "weight_map.h")
# the per-call event counts: the wave tally of the kernels, the counters of the ctx workspace and their read-back
_CALL_COUNTS = os.path.join(CSRC, "call_counts.h")
# the fixed-order float64 reduction of the moment sums and their scatter into the caller's arrays
_MOMENT_SUMS = os.path.join(CSRC, "moment_sums.h")
SOURCE_HEADERS = {"qc.hip": [_inc("microaligner_qc.h"), _CELL_GRID, _FLOW_JACOBIAN],
                  "remap_interp.hip": _INTERP_HEADERS,
                  "warp_compose.hip": _INTERP_HEADERS + [_inc("microaligner_compose.h")],
                  "flow_compose.hip": [_inc("microaligner_flowcompose.h")],
                  "flow_invert.hip": [_inc("microaligner_flowinvert.h"), _CALL_COUNTS],
                  "residual_shift.hip": [_inc("microaligner_residual.h"), _CELL_GRID],
                  "flow_grid.hip": _FLOW_GRID + [_CELL_GRID],
                  "flow_smooth.hip": [_SMOOTH_H, _CELL_GRID, _FLOW_JACOBIAN, _WINDOW_FIR, _WEIGHT_MAP, _CALL_COUNTS],
                  "flow_affine.hip": [_inc("microaligner_flowaffine.h"), _SMOOTH_H, _CELL_GRID, _WEIGHT_MAP, _MOMENT_SUMS],
                  "texture.hip": [_inc("microaligner_texture.h"), _CELL_GRID, _WINDOW_FIR],
                  "direct_affine.hip": [_inc("microaligner_direct.h"), _SMOOTH_H, _WEIGHT_MAP, _CELL_GRID, _MOMENT_SUMS],
                  "flow_refine.hip": [_inc("microaligner_flowrefine.h"), _SMOOTH_H, _WINDOW_FIR, _WEIGHT_MAP, _CALL_COUNTS],
                  "landmarks.hip": [_inc("microaligner_landmarks.h")],
                  "translation.hip": [_inc("microaligner_translation.h")],
                  "quantile.hip": [_inc("microaligner_quantile.h")],
                  "local_correlation.hip": [_inc("microaligner_localcorr.h"), _SMOOTH_H, _CELL_GRID, _WINDOW_FIR, _WEIGHT_MAP],
                  "flow_median.hip": [_inc("microaligner_flowmedian.h"), _SMOOTH_H, _WEIGHT_MAP, _CALL_COUNTS],
                  "flow_fill.hip": [_inc("microaligner_flowfill.h"), _SMOOTH_H, _WEIGHT_MAP, _CALL_COUNTS],
                  "debug_fill.hip": [_inc("microaligner_debug.h")],
                  "local_norm.hip": [_inc("microaligner_localnorm.h"), _SMOOTH_H, _WINDOW_FIR, _WEIGHT_MAP, _CALL_COUNTS],
                  "morphology.hip": [_inc("microaligner_morphology.h")],
                  "components.hip": [_inc("microaligner_components.h")]}
# the grid-flow headers are also read by the two sources whose kernels take their flow from a grid: further dependencies of
# those sources, beside the headers of their own above
GRID_FLOW_USERS = {"warp_compose.hip": _FLOW_GRID, "flow_invert.hip": _FLOW_GRID}
# -fno-slp-vectorize: the SLP vectoriser packs the sliding-window blur into v_pk_* ops with a storm of
# register-pair shuffles (measured 1.65x slower on blur_h_solve, profiles/r01_*); packed math is written by hand
# where it pays.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC",
         "-fno-fast-math", "-Wall", "-Wno-unused-function"]


def _flags():
    # MA_HIPCC_EXTRA: extra compiler flags for experiments (e.g. "-fno-slp-vectorize")
    return FLAGS + os.environ.get("MA_HIPCC_EXTRA", "").split()


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.sep not in cand or os.path.exists(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def source_hash():
    """sha256 (first 16 hex digits) over every source file that holds kernels of the measured path, the internal header,
    the public header and the compiler flags: ma_version() carries it, the profile summaries under profiles/ record it, and bench.py only quotes PMC
    traffic from a summary whose hash is the loaded library's."""
    import hashlib
    h = hashlib.sha256()
    # register.hip decides which launches the measured path makes and on which stream, ma_api.hip how the buffer cache and
    # the streams behave: both are part of what a profile measures.  nmi_score.h holds the gate's score (HEADERS).
    # Left out, having no kernel on the measured path (cfg3: pyramid, DOG, Farneback, warp, merge, NMI):
    #   - the clock probe;
    #   - the feature stage (FAST / DAISY / 2-NN / affine warp), which has its own tests and timings;
    #   - the registration quality maps, which nothing on the path calls;
    #   - the nearest / cubic / Lanczos-4 warps, which only a non-default Warper.interpolation reaches;
    #   - the one-resampling warp through an affine matrix and a flow, which only a Warper.tmat reaches;
    #   - the page-warp driver, which holds no kernel and runs after the measured steps;
    #   - the exact flow composition, which only flow_composition="exact" reaches;
    #   - the flow inverse and the point transforms, which only invert_flow() / transform_points() reach;
    #   - the residual shift maps, which only residual_shift() reaches;
    #   - the grid flows (nodes, expansion, loss maps; flow_grid_eval.h, their evaluation inside the warp and the point
    #     kernels), which only compress_flow() / a FlowGrid reach;
    #   - the flow smoothing and the fold mask, which only smooth_flow() / fold_mask() / repair_flow() reach;
    #   - the affine moments of a flow and its re-expression relative to a matrix, which only fit_flow_affine() /
    #     split_flow() / join_flow() / local_affine() reach;
    #   - the texture support maps (structure-tensor eigenvalues of an image), which only texture_maps() reaches;
    #   - the Gauss-Newton moments of the intensity-based affine alignment, which only align_affine() reaches;
    #   - the regularised Lucas-Kanade step of a flow against the images, which only refine_flow() reaches;
    #   - the thin-plate spline of landmark pairs on a grid and at points, which only landmark_flow() / landmark_points()
    #     reach;
    #   - the moments of the global translation search (ZNCC at every shift of a window over that shift's overlap), which
    #     only align_translation() reaches;
    #   - the radix select of an image's order statistics and the scaling to u8 between two given values, which only
    #     image_quantiles() / normalize_percentile() / a `percentiles` argument reach;
    #   - the local correlation maps (windowed ZNCC of a registered pair), which only local_correlation() reaches;
    #   - the median filter of a flow and its outlier mask, which only median_flow() / outlier_mask() reach;
    #   - the push-pull fill of a flow (a weighted pyramid pulled to 1 x 1 and pushed back), which only fill_flow() reaches;
    #   - the local contrast normalisation (an image minus its windowed mean over its windowed standard deviation), which
    #     only normalize_local() reaches;
    #   - the flat grey morphology (running minimum and maximum over a rectangle, opening, closing, top-hats), which only
    #     grey_erode() / grey_dilate() / grey_open() / grey_close() / tophat() reach;
    #   - the connected components (labels, areas and boxes, the area filter and the hole filling), which only
    #     label_components() / remove_small_objects() / fill_holes() reach;
    #   - the test hook that fills a context's idle scratch memory, which only tests call and which launches no kernel;
    #   - cell_grid.h, the cell grid and batch loop of the quality and residual shift maps, flow_jacobian.h, det J of
    #     the quality maps and the fold mask, window_fir.h, the separable FIR tile of the flow smoothing, the texture
    #     maps, the flow refinement, the local correlation maps and the local contrast normalisation, weight_map.h, the
    #     weight argument of the eight calls above that take one, call_counts.h, the per-call event counts of the calls above that return some,
    #     and moment_sums.h, the fixed-order float64 reduction of the two kinds of affine moments (SOURCE_HEADERS).
    off_path = {"probe.hip", "knn.hip", "daisy.hip", "ransac.hip", "feature_round.hip", "affine.hip", "qc.hip",
                "remap_interp.hip", "warp_compose.hip", "page_pipeline.hip", "flow_compose.hip",
                "flow_invert.hip", "residual_shift.hip", "flow_grid.hip", "flow_smooth.hip", "flow_affine.hip",
                "texture.hip", "direct_affine.hip", "flow_refine.hip", "landmarks.hip", "translation.hip",
                "quantile.hip", "local_correlation.hip", "flow_median.hip", "flow_fill.hip", "debug_fill.hip",
                "local_norm.hip", "morphology.hip", "components.hip"}
    for path in [os.path.join(CSRC, s) for s in SOURCES if s not in off_path] + HEADERS:
        h.update(open(path, "rb").read())
    h.update(" ".join(_flags()).encode())
    return h.hexdigest()[:16]


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 and link the shared library in-tree."""
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hipcc = _hipcc()
    # the source hash reaches ma_version() through a generated header that is rewritten only when it changes
    hash_h = os.path.join(objdir, "ma_src_hash.h")
    text = f'#define MA_SRC_HASH "{source_hash()}"\n'
    if not os.path.exists(hash_h) or open(hash_h).read() != text:
        with open(hash_h, "w") as f:
            f.write(text)
    objs, jobs = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, s.replace(".hip", ".o"))
        objs.append(obj)
        deps = [src] + HEADERS + SOURCE_HEADERS.get(s, []) + GRID_FLOW_USERS.get(s, []) + ([hash_h] if s == "ma_api.hip" else [])
        if force or _stale(obj, deps):
            jobs.append([hipcc] + _flags() + ["-I", objdir, "-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        return r.stderr

    with ThreadPoolExecutor(max_workers=4) as ex:
        for err in ex.map(run, jobs):
            if verbose and err:
                print(err)
    if jobs or force or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
