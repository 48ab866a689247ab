"""Float64 statements of Farneback's displacement estimation and of the dog() chain, made from scipy.ndimage and the
published algorithms, sharing no code with oracle/ma_oracle.c: the yardsticks of tests/test_oracle_independent.py (for the
oracle) and of tests/test_gpu_geometry_edges.py (for the kernels, which are bit-exact to the oracle)."""
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


def farneback_float64(prev, nxt, winsize, iterations, det_eps=0.0):
    """Displacement estimation of the paper's sections 4 - 5 (eqs. 7 - 11 with the a-priori displacement of section 5,
    iterated), float64 throughout.  OpenCV specifics that are PARAMETERS of the call, not of the paper, taken from the
    call site: 3 x 3 binomial pre-smoothing of both images at pyramid scale 1, a Gaussian window of sigma = 0.3 * (winsize
    // 2), the second expansion sampled bilinearly at x + d.  Not modelled: OpenCV's border attenuation (5 px) -- compare away
    from borders.  det_eps: OpenCV adds 1e-3 to the determinant of the 2 x 2 system (a regulariser the paper does not have);
    0 is the paper."""
    pre = lambda im: ndi.correlate1d(ndi.correlate1d(im.astype(np.float64), [0.25, 0.5, 0.25], axis=0, mode="mirror"),
                                     [0.25, 0.5, 0.25], axis=1, mode="mirror")
    c0, bx0, by0, axx0, ayy0, axy0 = poly_expansion(pre(prev))
    r1 = poly_expansion(pre(nxt))
    h, w = prev.shape
    gx, gy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    m = winsize // 2
    k = np.exp(-np.arange(-m, m + 1) ** 2 / (2 * (m * 0.3) ** 2))
    k /= k.sum()
    blur = lambda a: ndi.correlate1d(ndi.correlate1d(a, k, axis=0, mode="nearest"), k, axis=1, mode="nearest")
    dx, dy = np.zeros((h, w)), np.zeros((h, w))
    for _ in range(iterations):
        s = [ndi.map_coordinates(p, [gy + dy, gx + dx], order=1, mode="nearest") for p in r1]
        _, bx1, by1, axx1, ayy1, axy1 = s
        a11, a22, a12 = (axx0 + axx1) / 2, (ayy0 + ayy1) / 2, (axy0 + axy1) / 4       # A = (A1 + A2) / 2, A12 = axy / 2
        dbx = -0.5 * (bx1 - bx0) + a11 * dx + a12 * dy                                # eq. 10 with the a-priori d
        dby = -0.5 * (by1 - by0) + a12 * dx + a22 * dy
        g11, g12, g22 = blur(a11 * a11 + a12 * a12), blur(a12 * (a11 + a22)), blur(a12 * a12 + a22 * a22)
        h1, h2 = blur(a11 * dbx + a12 * dby), blur(a12 * dbx + a22 * dby)
        det = g11 * g22 - g12 * g12 + det_eps
        dx, dy = (g22 * h1 - g12 * h2) / det, (g11 * h2 - g12 * h1) / det             # eq. 9: d = (sum w A'A)^-1 sum w A'db
    return np.stack([dx, dy], -1)


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
