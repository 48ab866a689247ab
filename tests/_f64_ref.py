"""Float64 statements of Farneback's displacement estimation (single scale and OpenCV's pyramid) and of the dog() chain,
made from scipy.ndimage, numpy and the published algorithms plus OpenCV's documented parameters, sharing no code with
oracle/ma_oracle.c or tests/c_ref/ and calling neither: the yardsticks of tests/test_oracle_independent.py (for the
oracle), tests/test_farneback_levels_ref.py (for the pyramid restatement) and tests/test_gpu_geometry_edges.py /
tests/test_gpu_farneback_levels_f64.py (for the kernels, which are bit-exact to those two).

Modelled, with opencv_borders=True and in farneback_pyramid_float64: an initial flow; OpenCV's out-of-range rule in
UpdateMatrices (the second expansion contributes nothing where the sample's top-left pixel is outside [0, w - 2] x
[0, h - 2]); the 5-px border attenuation of the matrices; the pyramid's level clamp, per-level Gaussian blur of the
full-resolution image (reflect-101), half-pixel bilinear resize of the level images and of the flow, and the x 2 on the
initial flow.  Not modelled: float32 storage anywhere (pixel and resize coordinates, expansions, matrices, sums) and
non-finite inputs; those are what the tolerances of the callers absorb, or are tested elsewhere."""
import numpy as np
from scipy import ndimage as ndi


def poly_expansion(img, n=1, sigma=1.7):
    """Farneback 2003, section 2: per pixel the weighted least-squares fit  f(x) ~ x'Ax + b'x + c  over a (2n+1)^2
    neighbourhood with a Gaussian applicability.  Returns c, bx, by, axx, ayy, axy (axy = coefficient of x*y)."""
    xs = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-xs ** 2 / (2 * sigma ** 2))
    X, Y = np.meshgrid(xs, xs)                                 # X varies along columns
    B = np.stack([np.ones_like(X), X, Y, X * X, Y * Y, X * Y], -1).reshape(-1, 6)
    Wa = np.outer(g, g).reshape(-1)
    proj = np.linalg.inv(B.T @ (Wa[:, None] * B)) @ (B.T * Wa)  # 6 x (2n+1)^2
    return [ndi.correlate(img, proj[k].reshape(2 * n + 1, 2 * n + 1), mode="nearest") for k in range(6)]


# OpenCV's FarnebackUpdateMatrices attenuates the matrices of the 5 pixels next to each edge by these weights, counted from
# the edge outwards; a pixel near two edges (or near both sides of an image under 10 px) takes the product
BORDER_WEIGHTS = (0.14, 0.14, 0.4472, 0.4472, 0.4472)


def _border_scale(n):
    s = np.ones(n)
    for i, b in enumerate(BORDER_WEIGHTS[:n]):
        s[i] *= b
        s[n - 1 - i] *= b
    return s


def _sample_in_range(planes, fx, fy):
    """Bilinear samples of `planes` at (fx, fy) and the mask of the samples OpenCV takes: those whose top-left pixel
    (floor(fx), floor(fy)) lies in [0, w - 2] x [0, h - 2].  Elsewhere the samples are meaningless."""
    h, w = fx.shape
    x1, y1 = np.floor(fx), np.floor(fy)
    ok = (x1 >= 0) & (x1 <= w - 2) & (y1 >= 0) & (y1 <= h - 2)
    ax, ay = fx - x1, fy - y1
    x0i, y0i = np.clip(x1, 0, w - 1).astype(np.intp), np.clip(y1, 0, h - 1).astype(np.intp)
    x1i, y1i = np.minimum(x0i + 1, w - 1), np.minimum(y0i + 1, h - 1)
    out = [(p[y0i, x0i] * (1 - ax) + p[y0i, x1i] * ax) * (1 - ay) + (p[y1i, x0i] * (1 - ax) + p[y1i, x1i] * ax) * ay
           for p in planes]
    return out, ok


def _displacement(r0, r1, winsize, iterations, det_eps, d0=None, opencv_borders=False):
    """Sections 4 - 5 of the paper on two expansions (c, bx, by, axx, ayy, axy), starting from the flow d0 (zero if None)"""
    _, bx0, by0, axx0, ayy0, axy0 = r0
    h, w = bx0.shape
    gx, gy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    m = winsize // 2
    k = np.exp(-np.arange(-m, m + 1) ** 2 / (2 * (m * 0.3) ** 2)) if m > 0 else np.ones(1)   # windows 1 and 2: no blur
    k /= k.sum()
    blur = lambda a: ndi.correlate1d(ndi.correlate1d(a, k, axis=0, mode="nearest"), k, axis=1, mode="nearest")
    if d0 is None:
        dx, dy = np.zeros((h, w)), np.zeros((h, w))
    else:
        dx, dy = np.asarray(d0[..., 0], np.float64), np.asarray(d0[..., 1], np.float64)
    att = _border_scale(h)[:, None] * _border_scale(w)[None, :] if opencv_borders else None
    for _ in range(iterations):
        if opencv_borders:
            # outside the sampling range OpenCV drops the second image: b terms 0, A the first image's alone
            (bx1, by1, axx1, ayy1, axy1), ok = _sample_in_range(r1[1:], gx + dx, gy + dy)
            a11, a22 = np.where(ok, (axx0 + axx1) / 2, axx0), np.where(ok, (ayy0 + ayy1) / 2, ayy0)
            a12 = np.where(ok, (axy0 + axy1) / 4, axy0 / 2)
            bx1, by1 = np.where(ok, bx1, 0.0), np.where(ok, by1, 0.0)
        else:
            s = [ndi.map_coordinates(p, [gy + dy, gx + dx], order=1, mode="nearest") for p in r1]
            _, bx1, by1, axx1, ayy1, axy1 = s
            a11, a22, a12 = (axx0 + axx1) / 2, (ayy0 + ayy1) / 2, (axy0 + axy1) / 4   # A = (A1 + A2) / 2, A12 = axy / 2
        dbx = -0.5 * (bx1 - bx0) + a11 * dx + a12 * dy                                # eq. 10 with the a-priori d
        dby = -0.5 * (by1 - by0) + a12 * dx + a22 * dy
        if opencv_borders:
            a11, a22, a12, dbx, dby = (v * att for v in (a11, a22, a12, dbx, dby))
        g11, g12, g22 = blur(a11 * a11 + a12 * a12), blur(a12 * (a11 + a22)), blur(a12 * a12 + a22 * a22)
        h1, h2 = blur(a11 * dbx + a12 * dby), blur(a12 * dbx + a22 * dby)
        det = g11 * g22 - g12 * g12 + det_eps
        dx, dy = (g22 * h1 - g12 * h2) / det, (g11 * h2 - g12 * h1) / det             # eq. 9: d = (sum w A'A)^-1 sum w A'db
    return np.stack([dx, dy], -1)


def _preblur(im):
    """OpenCV's fixed 3 x 3 binomial pre-smoothing at pyramid scale 1 (GaussianBlur, ksize 3, sigma 0; reflect-101)"""
    return ndi.correlate1d(ndi.correlate1d(np.asarray(im, np.float64), [0.25, 0.5, 0.25], axis=0, mode="mirror"),
                           [0.25, 0.5, 0.25], axis=1, mode="mirror")


def farneback_float64(prev, nxt, winsize, iterations, det_eps=0.0, flow0=None, opencv_borders=False):
    """Displacement estimation of the paper's sections 4 - 5 (eqs. 7 - 11 with the a-priori displacement of section 5,
    iterated), float64 throughout.  OpenCV specifics that are PARAMETERS of the call, not of the paper, taken from the
    call site: 3 x 3 binomial pre-smoothing of both images at pyramid scale 1, a Gaussian window of sigma = 0.3 * (winsize
    // 2), the second expansion sampled bilinearly at x + d.  det_eps: OpenCV adds 1e-3 to the determinant of the 2 x 2
    system (a regulariser the paper does not have); 0 is the paper.  flow0: the initial flow (h, w, 2), zero if None.
    opencv_borders=False (the paper): the second expansion is sampled with edge clamping everywhere and no border
    attenuation -- compare away from the borders.  opencv_borders=True: OpenCV's out-of-range rule and 5-px border
    attenuation, which makes the statement hold over the whole image."""
    return _displacement(poly_expansion(_preblur(prev)), poly_expansion(_preblur(nxt)), winsize, iterations, det_eps,
                         flow0, opencv_borders)


def level_table(H, W, levels, min_size=32):
    """OpenCV's pyramid (pyr_scale 0.5) from its definition: [(w_k, h_k, ksize_k, sigma_k) for k = 0 .. kept levels].
    A level is kept while both scaled sides stay >= min_size; sigma_k = (2^k - 1) / 2, ksize_k = max(round(5 sigma_k) | 1,
    3), sizes round(side / 2^k), every rounding half to even (Python's round, as cvRound)."""
    kept = 0
    while kept < levels and W / 2 ** (kept + 1) >= min_size and H / 2 ** (kept + 1) >= min_size:
        kept += 1
    table = []
    for k in range(kept + 1):
        sigma = (2 ** k - 1) / 2
        table.append((round(W / 2 ** k), round(H / 2 ** k), max(round(5 * sigma) | 1, 3), sigma))
    return table


def resize_bilinear64(src, dw, dh, corner_aligned=False, nearest=False):
    """cv2.resize(INTER_LINEAR) in float64: half-pixel centres, source coordinates clamped to the image.  The two switches
    are conventions OpenCV does NOT use, for the tests that show the comparisons can tell them apart."""
    def axis(a, n_src, n_dst, ax):
        d = np.arange(n_dst, dtype=np.float64)
        if nearest:
            return np.take(a, np.minimum(np.floor(d * n_src / n_dst).astype(np.intp), n_src - 1), axis=ax)
        if corner_aligned:
            x = d * ((n_src - 1) / (n_dst - 1)) if n_dst > 1 else np.zeros(1)
        else:
            x = np.clip((d + 0.5) * (n_src / n_dst) - 0.5, 0, n_src - 1)
        i0 = np.floor(x).astype(np.intp)
        i1 = np.minimum(i0 + 1, n_src - 1)
        f = (x - i0).reshape([-1 if i == ax else 1 for i in range(a.ndim)])
        return np.take(a, i0, axis=ax) * (1 - f) + np.take(a, i1, axis=ax) * f
    sh, sw = src.shape[:2]
    return axis(axis(np.asarray(src, np.float64), sw, dw, 1), sh, dh, 0)


def _gaussian_taps(ksize, sigma):
    x = np.arange(ksize) - (ksize - 1) / 2
    k = np.exp(-x ** 2 / (2 * sigma ** 2))
    return k / k.sum()


# Conventions OpenCV does not use, each a plausible slip in a restatement of its level loop; farneback_pyramid_float64
# applies one on request so that tests can show the comparison would catch it
PYRAMID_ERRORS = ("flow_resize_corner_aligned", "flow_resize_nearest", "flow_not_doubled", "level_ksize_plus_2",
                  "level_sigma_x1.1", "level_blur_reflect")


def farneback_pyramid_float64(prev, nxt, levels, winsize, iterations, det_eps=1e-3, error=None):
    """cv2.calcOpticalFlowFarneback(prev, nxt, None, 0.5, levels, winsize, iterations, 1, 1.7, GAUSSIAN) in float64,
    from OpenCV's documented level loop: for k = kept levels .. 0 (level_table), each image is blurred at full resolution
    with the level's Gaussian (taps from the definition, normalised, reflect-101), resized to the level's size
    (resize_bilinear64); at k = 0 the blur is the fixed 3 x 3 pre-smoothing and there is no resize.  The initial flow is
    zero on the coarsest level, elsewhere the previous level's flow resized (resize_bilinear64) and doubled.  Each level
    runs farneback's iterations with OpenCV's border rules (farneback_float64(opencv_borders=True)).  error: one of
    PYRAMID_ERRORS, or None for the faithful statement."""
    if error is not None and error not in PYRAMID_ERRORS:
        raise ValueError(f"unknown error {error!r}")
    H, W = prev.shape
    imgs = [np.asarray(prev, np.float64), np.asarray(nxt, np.float64)]
    table = level_table(H, W, levels)
    flow = None
    for k in range(len(table) - 1, -1, -1):
        wk, hk, ksize, sigma = table[k]
        if flow is None:
            d0 = np.zeros((hk, wk, 2))
        else:
            d0 = resize_bilinear64(flow, wk, hk, corner_aligned=error == "flow_resize_corner_aligned",
                                   nearest=error == "flow_resize_nearest")
            if error != "flow_not_doubled":
                d0 = d0 * 2
        if k == 0:
            lev = [_preblur(im) for im in imgs]
        else:
            if error == "level_ksize_plus_2":
                ksize += 2
            if error == "level_sigma_x1.1":
                sigma *= 1.1
            taps = _gaussian_taps(ksize, sigma)
            mode = "reflect" if error == "level_blur_reflect" else "mirror"
            lev = [resize_bilinear64(ndi.correlate1d(ndi.correlate1d(im, taps, axis=1, mode=mode), taps, axis=0, mode=mode),
                                     wk, hk) for im in imgs]
        flow = _displacement(poly_expansion(lev[0]), poly_expansion(lev[1]), winsize, iterations, det_eps, d0, True)
    return flow


def shifted_texture_pair(h, w, seed, shift, amp=200.0):
    """(prev, next) float32: smooth noise in [0, amp] and the same content moved by `shift` = (x, y) px (cubic spline),
    so that the flow prev -> next is +shift -- the input on which the float32 Farneback of the oracle and the kernels
    stays within 2e-5 px of farneback_float64(det_eps=1e-3) away from the borders."""
    rng = np.random.default_rng(seed)
    base = ndi.gaussian_filter(rng.standard_normal((h + 20, w + 20)), 2.0)
    base = (base - base.min()) / (base.max() - base.min()) * amp
    prev = base[10:-10, 10:-10].astype(np.float32)
    nxt = ndi.shift(base, (shift[1], shift[0]), order=3, mode="nearest")[10:-10, 10:-10].astype(np.float32)
    return prev, nxt


def dog_float64(img, low_sigma=5, high_sigma=9):
    """OptFlowRegistrator.dog (optflow_registrator.py:249-274) in float64: normalize to [0, 1] -> GaussianBlur(ksize =
    8 * low_sigma + 1 for BOTH sigmas, reflect-101 at any number of folds, which is scipy's mode="mirror") with the two
    sigmas -> high - low -> normalize to [0, 255] and round.  Kernel taps from the definition, truncated at the window and
    renormalised.  Returns float64 grey levels; NaN where a normalisation divides by a zero range."""
    f = np.asarray(img, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = (f - f.min()) / (f.max() - f.min())
    ksize = 8 * low_sigma + 1

    def blur(a, sigma):
        x = np.arange(ksize) - ksize // 2
        k = np.exp(-x ** 2 / (2.0 * sigma ** 2))
        k /= k.sum()
        return ndi.correlate1d(ndi.correlate1d(a, k, axis=0, mode="mirror"), k, axis=1, mode="mirror")
    d = blur(f, high_sigma) - blur(f, low_sigma)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.rint((d - d.min()) / (d.max() - d.min()) * 255)
