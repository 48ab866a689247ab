"""The numpy statement of include/microaligner_direct.h, written from its definitions: the per-pixel terms and classes of the
alignment moments, summed with math.fsum (the correctly rounded sum, which no order of summation reaches exactly but every
order approaches within the standard bound); align_affine's own level loop run over these moments and the oracle's
pyrDown; and the analytic image pairs the tests recover a matrix from.  Only the moments are restated here: the loop
(pyramid_plan, align_levels, solve_level, finish) is the package's, shared with the device path as fit_from_moments is in
the flow_affine tests, so the agreement of the device with align_ref checks the kernel's sums and the pyramids, not the
loop; the loop is checked by the recovery of known matrices and by the step against numpy.linalg.lstsq.  numpy rounds every float64 operation on its own, which is the
arithmetic the header asks of the kernel."""
import math

import numpy as np

from microaligner_amd.feature_reg import direct_affine as DA

F32, F64 = np.float32, np.float64
NS, NC = 31, 5
USED, OUTSIDE, INVALID, UNWEIGHTED, TRIMMED = range(5)


def pixel_weight(weight, shape):
    if weight is None:
        return np.ones(shape, F32)
    assert weight.shape == tuple(shape)
    if weight.dtype == np.uint8:
        return (weight != 0).astype(F32)
    assert weight.dtype == F32
    return weight


def pixel_fields(ref, mov, M, gain=1.0, bias=0.0, weight=None, clip=None):
    """what the header defines per pixel, (H, W) each: X, Y, m, gx, gy, I, e, w (float64) and cls (0 used, 1 outside,
    2 invalid, 3 unweighted, 4 trimmed); values of pixels that are not used have no meaning"""
    H, W = ref.shape
    assert mov.shape == (H, W)
    M = np.asarray(M, F64).reshape(2, 3)
    gain, bias = F64(gain), F64(bias)
    x = np.broadcast_to(np.arange(W, dtype=F64)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=F64)[:, None], (H, W))
    X, Y = x - (W - 1) / 2.0, y - (H - 1) / 2.0
    with np.errstate(invalid="ignore", over="ignore"):
        sx = (M[0, 0] * x + M[0, 1] * y) + M[0, 2]
        sy = (M[1, 0] * x + M[1, 1] * y) + M[1, 2]
        fx, fy = np.floor(sx), np.floor(sy)
        inside = (fx >= 0) & (fx <= W - 2) & (fy >= 0) & (fy <= H - 2)
        ix, iy = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
        tx, ty = sx - fx, sy - fy
        m64 = np.pad(mov.astype(F64), ((0, 1), (0, 1)))      # a side of 1: no pixel is inside, the taps read are the padding
        a00, a01, a10, a11 = m64[iy, ix], m64[iy, ix + 1], m64[iy + 1, ix], m64[iy + 1, ix + 1]
        d0, d1 = a01 - a00, a11 - a10
        top, bot = a00 + d0 * tx, a10 + d1 * tx
        gy = bot - top
        m = top + gy * ty
        gx = d0 + (d1 - d0) * ty
        I = ref.astype(F64)
        e = I - (gain * m + bias)
        finite = np.isfinite(I) & np.isfinite(a00) & np.isfinite(a01) & np.isfinite(a10) & np.isfinite(a11)
        wm = pixel_weight(weight, (H, W))
        weighted = np.isfinite(wm) & (wm > 0)
        trimmed = np.zeros((H, W), bool) if clip is None or not clip > 0 else ~(np.abs(e) <= clip)
        cls = np.where(~inside, OUTSIDE, np.where(~finite, INVALID, np.where(~weighted, UNWEIGHTED,
                                                                             np.where(trimmed, TRIMMED, USED))))
    return dict(X=X, Y=Y, m=m, gx=gx, gy=gy, I=I, e=e, w=wm.astype(F64), cls=cls)


def pixel_terms(ref, mov, M, gain=1.0, bias=0.0, weight=None, clip=None):
    """(terms (H, W, 31) float64, cls (H, W)); the terms of pixels that are not used are 0"""
    f = pixel_fields(ref, mov, M, gain, bias, weight, clip)
    X, Y, m, gx, gy, I, e, w, cls = (f[k] for k in ("X", "Y", "m", "gx", "gy", "I", "e", "w", "cls"))
    with np.errstate(invalid="ignore", over="ignore"):
        wgx, wgy = w * gx, w * gy
        A = (wgx * gx, wgx * gy, wgy * gy)
        G = (X * X, X * Y, X, Y * Y, Y)
        we = w * e
        ex, ey = we * gx, we * gy
        wmm, wI = w * m, w * I
        terms = [A[i] * G[j] if j < 5 else A[i] for i in range(3) for j in range(6)]
        terms += [ex * X, ex * Y, ex, ey * X, ey * Y, ey, we * e, w, wmm, wI, wmm * m, wmm * I, wI * I]
        terms = np.stack(terms, -1)
    terms[cls != USED] = 0.0
    return terms, cls


def moments_ref(ref, mov, M, gain=1.0, bias=0.0, weight=None, clip=None, with_abs=True):
    """(sums (31,) by math.fsum, counts (5,) of used / outside / invalid / unweighted / trimmed, abs_sums (31,) = sum |term|
    or None)"""
    terms, cls = pixel_terms(ref, mov, M, gain, bias, weight, clip)
    t = terms[cls == USED]
    sums = np.array([math.fsum(t[:, k]) for k in range(NS)])
    abs_sums = np.array([math.fsum(np.abs(t[:, k])) for k in range(NS)]) if with_abs else None
    counts = np.array([(cls == q).sum() for q in range(NC)], np.int64)
    return sums, counts, abs_sums


def pyramids(ref, mov, weight, plan):
    """per level of plan (ref, mov, weight), every level the oracle's pyrDown of the next finer one; a uint8 mask is a
    float32 map (nonzero = 1) below the full size"""
    from oracle import oracle as O
    steps = max(int(math.log2(f)) for f, _ in plan)
    refs, movs, ws = [ref], [mov], [weight]
    if weight is not None and weight.dtype == np.uint8 and steps:
        weight = (weight != 0).astype(F32)
    for _ in range(steps):
        refs.append(O.pyr_down(refs[-1]))
        movs.append(O.pyr_down(movs[-1]))
        weight = None if weight is None else O.pyr_down(weight)
        ws.append(weight)
    return [(refs[int(math.log2(f))], movs[int(math.log2(f))], ws[int(math.log2(f))]) for f, _ in plan]


def align_ref(ref, mov, model="affine", tmat=None, weight=None, num_pyr_lvl=3, use_full_res_img=True, max_iter=30, tol=1e-3,
              clip=None, photometric=True):
    """align_affine(..., return_info=True) with the moments of this statement in the place of the kernel's"""
    M0 = DA.start_matrix(tmat)
    plan = DA.pyramid_plan(ref.shape, num_pyr_lvl, use_full_res_img)
    pyr = pyramids(ref, mov, weight, plan)

    def moments(level, M, gain, bias, clip):
        r, m, w = pyr[level]
        return moments_ref(r, m, M, gain, bias, w, clip, with_abs=False)[:2]
    M, info = DA.align_levels(plan, moments, M0, model, max_iter, tol, clip, photometric)
    return DA.finish(tmat, M0, M, info, ref.shape)


# ---- analytic pairs ---------------------------------------------------------------------------------------------------------
def cosines(seed, n=10):
    """n plane waves of periods 9 to 40 px: (kx, ky, phase, amplitude), the amplitudes adding up to 1"""
    rng = np.random.default_rng(seed)
    period, ang = rng.uniform(9, 40, n), rng.uniform(0, math.pi, n)
    amp = rng.uniform(0.5, 1.0, n)
    return 2 * math.pi * np.cos(ang) / period, 2 * math.pi * np.sin(ang) / period, rng.uniform(0, 2 * math.pi, n), amp / amp.sum()


def texture(waves, x, y):
    """in [-1, 1]"""
    kx, ky, ph, amp = waves
    return sum(a * np.cos(u * x + v * y + p) for u, v, p, a in zip(kx, ky, ph, amp))


def true_matrix(shape, rot_deg, scale, shift, shear=0.0, aniso=1.0):
    """M (reference pixels -> moving pixels): about the image's centre a rotation, a scale (x by scale * aniso), a shear,
    then the shift"""
    H, W = shape
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    th = math.radians(rot_deg)
    R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    L = R @ np.array([[scale * aniso, shear], [0.0, scale]])
    return np.concatenate([L, (c - L @ c + np.asarray(shift, F64))[:, None]], 1)


def inverse(M):
    return np.linalg.inv(np.append(np.asarray(M, F64).reshape(2, 3), [[0, 0, 1]], axis=0))[:2]


def quantise(img, dtype):
    if dtype == F32:
        return img.astype(F32)
    return np.clip(np.rint(img), 0, np.iinfo(dtype).max).astype(dtype)


def make_pair(shape, M, seed, ref_dtype=F32, mov_dtype=F32, gain=1.0, bias=0.0, noise=0.0):
    """(ref, mov) with ref(p) = gain * mov(M p) + bias up to quantisation and noise: the texture is evaluated at the
    transformed coordinates, so M is exact.  The texture spans 0.15 to 0.45 of the reference dtype's range (255 for
    float32); bias and noise (sigma) are in units of that range's 1/255."""
    H, W = shape
    waves = cosines(seed)
    rng = np.random.default_rng(seed + 1)
    y, x = np.mgrid[0:H, 0:W].astype(F64)
    Mi = inverse(M)
    full = lambda dt: 255.0 if dt == F32 else float(np.iinfo(dt).max)       # noqa: E731
    f_ref = 0.30 + 0.15 * texture(waves, x, y)
    f_mov = 0.30 + 0.15 * texture(waves, Mi[0, 0] * x + Mi[0, 1] * y + Mi[0, 2], Mi[1, 0] * x + Mi[1, 1] * y + Mi[1, 2])
    ref = f_ref * full(ref_dtype) + rng.normal(0, 1, shape) * noise * full(ref_dtype) / 255.0
    mov = (f_mov - bias / 255.0) / gain * full(mov_dtype) + rng.normal(0, 1, shape) * noise * full(mov_dtype) / 255.0
    return quantise(ref, ref_dtype), quantise(mov, mov_dtype)


def corner_error(Ma, Mb, shape):
    """the largest distance between where two matrices send an image corner, px"""
    H, W = shape
    pts = np.array([[x, y, 1.0] for x in (0.0, W - 1.0) for y in (0.0, H - 1.0)])
    return float(np.hypot(*(pts @ (np.asarray(Ma, F64) - np.asarray(Mb, F64)).T).T).max())
