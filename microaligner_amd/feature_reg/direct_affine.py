"""Intensity-based affine alignment (include/microaligner_direct.h): a Gauss-Newton minimisation of the weighted squared
difference between the reference and the moving image sampled through a 2 x 3 matrix, coarse to fine, with a gain and a
bias between the two.  No counterpart in the reference.

    tmat = align_affine(ref, mov, model="affine", tmat=feature_tmat, weight=texture_maps(ref, floor=f).weight)
    Warper(tmat=tmat, ...)                         # or transform_points(..., tmat=tmat), split_flow(flow, tmat=tmat)

The sums of a pass come from one pass over the images on the device (Context.direct_affine_moments); the step is a few dozen
float64 operations on the host (gauss_newton_step).  Every argument is checked before any device work.  Images numpy or
DeviceArray; matrices are always numpy.

Frames.  M (2 x 3) takes absolute reference pixels to absolute moving-image pixels: mov is sampled at M (x, y, 1).  The
solver works on the centred parameters theta = (L00, L01, c0, L10, L11, c1), s = L P + c for P = p - centre, so that
M = [L | c - L centre]; the sums of the kernel are taken about the same centre.  Warper.tmat is inv([M; 0 0 1])[:2].

The method is local: it follows the gradient of the interpolated moving image, so the start has to be within a few pixels
(at the coarsest level used) of the optimum.  Start it from a feature matrix, not from nothing, where cycles are far apart.
"""
import collections
import math

import numpy as np

from ..device import _check_iteration, _real, direct_affine_moments_params, get_context
from . import affine_math

MODELS = ("affine", "similarity", "rigid", "translation")
LAMBDA_START, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-9, 1e9
RANK_EPS = 1e-12
MIN_LEVEL_SIDE = 100       # FeatureRegistrator's: a level is dropped once a side would fall below it


class LevelInfo(collections.namedtuple("LevelInfo", "factor shape passes rejected first_cost last_cost last_step counts "
                                                    "deficient empty converged")):
    """One level of align_affine: its factor against the full image and its (h, w); the number of moment passes of the
    Gauss-Newton loop (the photometric pass not counted) and how many of them were rejected; the cost sum w e^2 / sum w of
    the first pass and of the best; the largest movement of an image corner by the last step, in px of the level; the
    (used, outside, invalid, unweighted, trimmed) counts of the best pass; whether the level was skipped because its
    normal matrix was rank deficient, or because no pixel was used; whether the loop ended on a step within tol."""


class DirectAffineInfo(collections.namedtuple("DirectAffineInfo", "levels gain bias accepted converged used_share matrix "
                                                                  "start_cost final_cost")):
    """align_affine(..., return_info=True): a LevelInfo per level, coarsest first; the gain and bias of the finest level;
    whether the result was accepted (else the starting matrix came back); whether the finest level converged; the used
    pixels over h * w at the finest level; M (2 x 3 float64, reference pixels to moving-image pixels of the full image)
    behind the returned tmat; and the cost of the starting matrix and of the result at the finest level, both with the
    final gain and bias (costs compare only within a level)."""


def _check_model(model):
    if not isinstance(model, str) or model not in MODELS:
        raise ValueError(f"unknown model {model!r}: expected one of {list(MODELS)}")
    return model


def _centre(shape):
    return np.array([(shape[1] - 1) / 2.0, (shape[0] - 1) / 2.0])


def to_centred(M, shape):
    """theta (6,) of the absolute 2 x 3 matrix M: the same linear part, the translation c = L centre + t"""
    M = np.asarray(M, np.float64)
    out = M.copy()
    out[:, 2] = M[:, :2] @ _centre(shape) + M[:, 2]
    return out.ravel()


def to_absolute(theta, shape):
    """M (2 x 3) of theta: the same linear part (bit for bit), t = c - L centre"""
    out = np.array(theta, np.float64).reshape(2, 3)
    out[:, 2] = out[:, 2] - out[:, :2] @ _centre(shape)
    return out


def model_basis(model, theta):
    """B (6 x k): the directions of theta the model may move in.  "affine": all six.  "translation": c0, c1.
    "similarity": L + a I + b [[0, -1], [1, 0]] and the translation -- a start that is a similarity stays one.  "rigid":
    the rotation of the current linear part, d/dphi R(phi) L at phi = 0, and the translation -- linearised about the
    current matrix; the step is folded in as a rotation (fold_step), so det L is kept."""
    _check_model(model)
    B = np.zeros((6, {"affine": 6, "similarity": 4, "rigid": 3, "translation": 2}[model]))
    if model == "affine":
        B[:] = np.eye(6)
        return B
    B[2, -2] = B[5, -1] = 1.0
    if model == "similarity":
        B[0, 0] = B[4, 0] = 1.0
        B[1, 1], B[3, 1] = -1.0, 1.0
    elif model == "rigid":
        L00, L01, _, L10, L11, _ = theta
        B[:, 0] = (-L10, -L11, 0.0, L00, L01, 0.0)
    return B


def normal_equations(sums, gain):
    """(H (6 x 6), g (6,)) of a pass: H = gain^2 J^T W J from the 18 sums, g = gain J^T W e from the next six."""
    S = np.asarray(sums, np.float64)
    G = lambda a: np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])     # noqa: E731
    xx, xy, yy = G(S[0:6]), G(S[6:12]), G(S[12:18])
    H = np.block([[xx, xy], [xy, yy]]) * (gain * gain)
    return H, S[18:24] * gain


def gauss_newton_step(sums, gain, model, theta, lam=0.0):
    """The step D (6,) in theta of one pass: D = B (B^T H B + lam diag(B^T H B))^-1 B^T g.  -> (D, deficient).
    Deficient (D is then None): no weight (sums[25] <= 0), a diagonal entry of A = B^T H B that is not positive, or
    A scaled to a unit diagonal with a smallest eigenvalue <= 1e-12 times its largest -- solve_flow_affine's rule
    det <= 1e-12 tr^2, for k parameters."""
    B = model_basis(model, theta)
    H, g = normal_equations(sums, gain)
    A, b = B.T @ H @ B, B.T @ g
    d = np.diag(A)
    if not (sums[25] > 0 and np.all(np.isfinite(A)) and np.all(np.isfinite(b)) and np.all(d > 0)):
        return None, True
    sc = 1.0 / np.sqrt(d)
    An = A * sc[:, None] * sc[None, :]
    ev = np.linalg.eigvalsh(An)
    if not ev[0] > RANK_EPS * ev[-1]:
        return None, True
    dn = np.linalg.solve(An + lam * np.eye(len(d)), b * sc)
    return B @ (dn * sc), False


def fold_step(theta, D, model):
    """theta after the step D.  Additive, except "rigid": its linear part is turned by the step's angle, L <- R(phi) L."""
    theta = np.asarray(theta, np.float64)
    if model != "rigid":
        return theta + D
    L00, L01, _, L10, L11, _ = theta
    # D = B d with B[:, 0] = (-L10, -L11, 0, L00, L01, 0): the angle is the coefficient of that column
    col = np.array([-L10, -L11, L00, L01])
    phi = float(col @ np.array([D[0], D[1], D[3], D[4]]) / (col @ col))
    c, s = math.cos(phi), math.sin(phi)
    out = theta.copy()
    out[0], out[1] = c * L00 - s * L10, c * L01 - s * L11
    out[3], out[4] = s * L00 + c * L10, s * L01 + c * L11
    out[2], out[5] = theta[2] + D[2], theta[5] + D[5]
    return out


def corner_movement(theta_a, theta_b, shape):
    """the largest distance between the positions two thetas give an image corner, px"""
    d = (np.asarray(theta_b) - np.asarray(theta_a)).reshape(2, 3)
    cx, cy = _centre(shape)
    return float(max(np.hypot(*(d[:, 0] * X + d[:, 1] * Y + d[:, 2])) for X in (-cx, cx) for Y in (-cy, cy)))


def photometric_fit(sums, gain, bias):
    """(gain, bias) of the weighted least squares of I on m from sums[25..30]; the given pair where m has no variance or
    the slope is not positive and finite"""
    sw, swm, swi, swmm, swmi = (float(v) for v in sums[25:30])
    if not sw > 0:
        return gain, bias
    var, cov = swmm - swm * swm / sw, swmi - swm * swi / sw
    if not (var > RANK_EPS * abs(swmm) and cov > 0 and math.isfinite(cov / var)):
        return gain, bias
    g = cov / var
    return g, (swi - g * swm) / sw


def solve_level(moments, M0, shape, model="affine", max_iter=30, tol=1e-3, clip=None, photometric=True, gain=1.0, bias=0.0):
    """The loop of one level.  moments(M, gain, bias, clip) -> (sums (31,), counts (5,)).  -> (M, gain, bias, LevelInfo
    without factor).  One unclipped photometric pass sets (gain, bias); then passes of moments, step, fold; (gain, bias) for
    the next pass come from the sums the step was taken from.  Levenberg-Marquardt on the cost sum w e^2 / sum w: a pass whose
    cost is not below the best so far is rejected, the step is taken again from the best with lam * 10; an accepted pass
    divides lam by 10.  Ends on a step that moves no corner by more than tol (the step is applied), or after max_iter
    passes; the best measured matrix comes back unless the loop ended on such a step."""
    theta = to_centred(M0, shape)
    info = dict(shape=tuple(shape), passes=0, rejected=0, first_cost=float("nan"), last_cost=float("nan"),
                last_step=float("nan"), counts=(0, 0, 0, 0, 0), deficient=False, empty=False, converged=False)

    def done(th):
        return to_absolute(th, shape), gain, bias, info

    if photometric:
        sums, counts = moments(to_absolute(theta, shape), 1.0, 0.0, None)
        info["counts"] = tuple(int(v) for v in counts)
        if counts[0] == 0:
            info["empty"] = True
            return done(theta)
        gain, bias = photometric_fit(sums, 1.0, 0.0)
    best, lam = None, LAMBDA_START
    for _ in range(max_iter):
        sums, counts = moments(to_absolute(theta, shape), gain, bias, clip)
        info["passes"] += 1
        cost = sums[24] / sums[25] if counts[0] > 0 and sums[25] > 0 else float("nan")
        if best is None:
            info["first_cost"] = float(cost)
            info["counts"] = tuple(int(v) for v in counts)
            if not math.isfinite(cost):
                info["empty"] = True
                return done(theta)
        if best is None or cost < best["cost"]:
            if best is not None:
                lam = max(lam / 10.0, LAMBDA_MIN)
            best = dict(theta=theta, cost=float(cost), sums=sums, gain=gain, counts=counts)
            info["last_cost"], info["counts"] = float(cost), tuple(int(v) for v in counts)
        else:
            info["rejected"] += 1
            lam = lam * 10.0
            if lam > LAMBDA_MAX:
                break
        D, deficient = gauss_newton_step(best["sums"], best["gain"], model, best["theta"], lam)
        if deficient:
            info["deficient"] = True
            break
        theta = fold_step(best["theta"], D, model)
        info["last_step"] = corner_movement(best["theta"], theta, shape)
        if photometric:
            gain, bias = photometric_fit(best["sums"], gain, bias)
        if info["last_step"] <= tol:
            info["converged"] = True
            return done(theta)
    return done(best["theta"] if best is not None else theta)


def pyramid_plan(shape, num_pyr_lvl, use_full_res_img):
    """[(factor, (h, w))] coarsest first, FeatureRegistrator's plan: factors 2, 4, ... while both sides keep at least 100
    px, at most num_pyr_lvl of them, plus the image itself with use_full_res_img.  Level sizes are pyrDown's: (n + 1) // 2."""
    if isinstance(num_pyr_lvl, bool) or not isinstance(num_pyr_lvl, (int, np.integer)) or num_pyr_lvl < 0:
        raise ValueError(f"num_pyr_lvl must be a non-negative integer, got {num_pyr_lvl!r}")
    plan, hw = [], (int(shape[0]), int(shape[1]))
    for steps in range(1, int(num_pyr_lvl) + 1):
        if min(shape[0], shape[1]) / 2 ** steps < MIN_LEVEL_SIDE:
            break
        hw = ((hw[0] + 1) // 2, (hw[1] + 1) // 2)
        plan.append((2 ** steps, hw))
    plan.reverse()
    if use_full_res_img:
        plan.append((1, (int(shape[0]), int(shape[1]))))
    if not plan:
        raise ValueError("no level to work on: the image has no pyramid level of at least 100 px a side within num_pyr_lvl "
                         "and use_full_res_img is False")
    return plan


def start_matrix(tmat):
    """M0 = pinv([tmat; 0 0 1])[:2], formed as transform_img_with_tmat forms it; the identity for None.  ValueError unless
    tmat is a finite 2 x 3 matrix with a finite M0."""
    if tmat is None:
        return np.eye(2, 3)
    try:
        t = np.asarray(tmat, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"tmat must be a finite 2x3 matrix: {e}") from None
    if t.shape != (2, 3) or not np.all(np.isfinite(t)):
        raise ValueError(f"tmat must be a finite 2x3 matrix, got shape {t.shape}")
    m = np.linalg.pinv(np.append(t, [[0, 0, 1]], axis=0))[:2]
    if not np.all(np.isfinite(m)):
        raise ValueError("pinv([tmat; 0 0 1]) is not finite")
    return m


def _at_level(M, factor):
    """the full image's M in pixels of a level `factor` times coarser (coarse pixel k is fine pixel factor * k)"""
    out = np.array(M, np.float64)
    out[:, 2] = out[:, 2] / factor
    return out


def align_levels(plan, moments, M0, model="affine", max_iter=30, tol=1e-3, clip=None, photometric=True):
    """The level loop over any source of moments: moments(level, M, gain, bias, clip) -> (sums, counts) for level = index
    into plan ([(factor, (h, w))], coarsest first); M0 the start in pixels of the full image.  -> (M of the full image,
    DirectAffineInfo without the acceptance of the matrix's shape).  Between levels the 2 x 2 part carries over and the
    translation scales with the factor.  A level that is empty or rank deficient leaves the matrix as it was.  The result
    is accepted only if, at the finest level and with its final gain and bias, its cost is below the starting matrix's."""
    M0 = np.asarray(M0, np.float64)
    M, gain, bias, levels = M0.copy(), 1.0, 0.0, []
    for k, (factor, shape) in enumerate(plan):
        Ml, gain, bias, li = solve_level(lambda *a: moments(k, *a), _at_level(M, factor), shape, model, max_iter, tol, clip,
                                         photometric)
        if not (li["empty"] or li["deficient"]) and np.all(np.isfinite(Ml)):
            M = _at_level(Ml, 1.0 / factor)
        levels.append(LevelInfo(factor=factor, **li))
    k, (factor, shape) = len(plan) - 1, plan[-1]
    last = levels[-1]
    start_cost = final_cost = float("nan")
    used = 0
    if not last.empty:
        s0, c0 = moments(k, _at_level(M0, factor), gain, bias, clip)
        s1, c1 = moments(k, _at_level(M, factor), gain, bias, clip)
        if c0[0] > 0 and s0[25] > 0:
            start_cost = float(s0[24] / s0[25])
        if c1[0] > 0 and s1[25] > 0:
            final_cost = float(s1[24] / s1[25])
        used = int(c1[0])
    accepted = bool(final_cost < start_cost)
    return M, DirectAffineInfo(levels, float(gain), float(bias), accepted, bool(last.converged),
                               used / float(shape[0] * shape[1]), M, start_cost, final_cost)


def finish(tmat0, M0, M, info, shape):
    """(tmat, info): tmat = inv([M; 0 0 1])[:2] if the result was accepted and passes FeatureRegistrator's checks of a
    matrix (axis scales in [0.3, 3], the centre stays inside), else the start tmat0 as it was given (None: the identity) and
    accepted False."""
    accepted, out = info.accepted, None
    if accepted:
        with np.errstate(all="ignore"):
            try:
                out = np.linalg.inv(np.append(M, [[0, 0, 1]], axis=0))[:2]
            except np.linalg.LinAlgError:
                out = None
        accepted = out is not None and bool(np.all(np.isfinite(out))) and affine_math.scales_plausible(out) and \
            affine_math.centre_stays_inside(out, shape)
    if not accepted:
        M = np.asarray(M0, np.float64)
        out = np.eye(2, 3) if tmat0 is None else np.array(tmat0, dtype=np.float64)
    return out, info._replace(accepted=accepted, matrix=np.array(M, np.float64))


def check_arguments(ref_img, mov_img, model, tmat, weight, labels, num_pyr_lvl, use_full_res_img, max_iter, tol, clip):
    """Every check of align_affine, without touching a device -> (M0, plan, max_iter, tol, clip)."""
    _check_model(model)
    if labels is not None and labels != "dog":
        raise ValueError(f"labels must be None or 'dog', got {labels!r}")
    M0 = start_matrix(tmat)
    direct_affine_moments_params(ref_img, mov_img, M0, 1.0, 0.0, weight, clip)
    max_iter, tol = _check_iteration(max_iter, tol, np.float64)
    plan = pyramid_plan(ref_img.shape, num_pyr_lvl, bool(use_full_res_img))
    return M0, plan, max_iter, tol, None if clip is None else _real(clip, "clip")


def _device_pyramids(ctx, ref, mov, weight, plan):
    """per level of plan: (ref, mov, weight) on the device; every level is pyr_down of the next finer one.  A uint8 mask is
    used as it is at full size and as a float32 map (nonzero = 1) below."""
    steps = max(int(math.log2(f)) for f, _ in plan)
    refs, movs, ws = [ref], [mov], [weight]
    if weight is not None and weight.dtype == np.uint8 and steps:
        weight = ctx.mask_weight(weight)
    for _ in range(steps):
        refs.append(ctx.pyr_down(refs[-1]))
        movs.append(ctx.pyr_down(movs[-1]))
        weight = None if weight is None else ctx.pyr_down(weight)
        ws.append(weight)
    return [(refs[int(math.log2(f))], movs[int(math.log2(f))], ws[int(math.log2(f))]) for f, _ in plan]


def align_affine(ref_img, mov_img, model="affine", tmat=None, weight=None, labels=None, num_pyr_lvl=3,
                 use_full_res_img=True, max_iter=30, tol=1e-3, clip=None, photometric=True, return_info=False):
    """The 2 x 3 float64 matrix, in Warper.tmat's convention, that aligns mov_img to ref_img by their intensities: it
    minimises sum w (ref(p) - (gain * mov(M p) + bias))^2 over M = inv([tmat; 0 0 1])[:2], mov sampled bilinearly, by
    damped Gauss-Newton steps from coarse to fine.  Samples that fall outside the moving image take no part (no border
    mode), so a large shift shrinks the support: see info.used_share.

    ref_img, mov_img: (H, W) uint8, uint16 or float32, of one shape, numpy or DeviceArray; mov_img is the ORIGINAL moving
    image, not one already transformed.  model: "affine" (6 parameters), "similarity", "rigid" or "translation"; the
    restricted models move the start within the model (model_basis), they do not project it.  tmat: the start, e.g.
    FeatureRegistrator.register()'s; None is the identity.  The method is local: the start must be within a few px, at the
    coarsest level used, of the answer.  weight: None, an (H, W) float32 map (texture_maps(...).weight) or uint8 mask.
    labels: None -- the images as they are; "dog" -- the gate's labels of both first (sigmas 5 / 9), as texture_maps.
    num_pyr_lvl, use_full_res_img: the levels, as FeatureRegistrator's (a level is dropped below 100 px a side).
    max_iter, tol: per level, passes and the corner movement in px of the level at which a step ends the level.
    clip: residual in grey levels beyond which a pixel is left out (not in the photometric pass).  photometric: fit a
    gain and a bias between the images (they lag the matrix by one pass).

    The result is accepted only if its cost at the finest level is below the start's and it passes FeatureRegistrator's
    checks of a matrix; otherwise the start comes back and info.accepted is False.  Costs compare only within a level.
    return_info: (tmat, DirectAffineInfo)."""
    M0, plan, max_iter, tol, clip = check_arguments(ref_img, mov_img, model, tmat, weight, labels, num_pyr_lvl,
                                                    use_full_res_img, max_iter, tol, clip)
    ctx = get_context()
    d_ref, d_mov = ctx.asdevice(ref_img), ctx.asdevice(mov_img)
    d_weight = None if weight is None else ctx.asdevice(weight)
    if labels == "dog":
        from ..shared_modules.registration_qc import _labels
        d_ref, d_mov = _labels(ctx, d_ref, "dog", 0), _labels(ctx, d_mov, "dog", 0)
    pyr = _device_pyramids(ctx, d_ref, d_mov, d_weight, plan)

    def moments(level, M, gain, bias, clip):
        r, m, w = pyr[level]
        return ctx.direct_affine_moments(r, m, M, gain, bias, w, clip)

    M, info = align_levels(plan, moments, M0, model, max_iter, tol, clip, bool(photometric))
    out, info = finish(tmat, M0, M, info, tuple(ref_img.shape))
    return (out, info) if return_info else out


__all__ = ["align_affine", "DirectAffineInfo", "LevelInfo"]
