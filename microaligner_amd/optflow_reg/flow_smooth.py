"""Changing a flow (include/microaligner_flowsmooth.h): a confidence-weighted Gaussian smoothing that drops bad pixels,
fills them from their surroundings and feathers the result back into the untouched flow; the per-pixel mask of where a
flow folds or is not finite; and a short loop of the two that repairs a flow.  No counterpart in the reference.

    smooth_flow(f, sigma)                                  a denoised flow (every pixel smoothed)
    smooth_flow(f, sigma, weight=keep, where="blend")      the pixels with keep == 0 filled in, the rest untouched
    fold_mask(f, margin)                                   keep: 0 near a fold or a non-finite pixel
    repair_flow(f)                                         fold_mask and smooth_flow in rounds until nothing is bad

Every argument is checked before any device work.  numpy in, numpy out; DeviceArray in, DeviceArray out.  A FlowGrid is
expanded on the device first (device.dense_flow) and gives the kind of array its nodes are.
"""
import numpy as np

from ..device import DeviceArray, FlowGrid, RepairInfo, dense_flow, fold_mask_params, gaussian_taps, get_context, \
    smooth_flow_params


def _like(flow):
    return flow.nodes if isinstance(flow, FlowGrid) else flow


def _cell_weight(weight, cell_size):
    # per-cell maps arrive from FlowQC / RegistrationQC as float64, int64 or bool: a host map of any real dtype is
    # rounded to the float32 the kernel reads (a few numbers per cell)
    if cell_size is not None and isinstance(weight, np.ndarray) and weight.dtype != np.float32 and \
            weight.dtype.kind in "biuf":
        return weight.astype(np.float32)
    return weight


def smooth_flow(flow, sigma, weight=None, cell_size=None, where="all", truncate=3.0, min_support=0.0, return_info=False):
    """The (H, W, 2) float32 flow smoothed with a Gaussian of `sigma` px cut at r = max(1, ceil(truncate * sigma)) <= 128
    taps a side, normalised by the smoothed weights so that pixels of weight 0 -- and non-finite pixels, whatever their
    weight -- take no part and are filled from the others.

    weight: None (every finite pixel counts 1); an (H, W) float32 map; an (H, W) uint8 mask (nonzero keeps); or, with
    cell_size (an int or (cell_h, cell_w)), a (gy, gx) map on that cell grid, which is how FlowQC / RegistrationQC maps
    arrive (e.g. weight=(qc.folded == 0), cell_size=the one given to flow_qc).  A weight that is NaN, negative or 0 drops
    its pixel.  Weights above 1 are allowed; with where="blend" they saturate the feathering.
    where: "all" -- every pixel takes its smoothed value; "blend" -- dropped pixels take it, pixels with no dropped pixel
    within r keep their value bit for bit, and the ones between are feathered, continuously across the rim of a hole.
    A pixel whose smoothed weight is not above `min_support` (no kept pixel within r, for 0) comes back NaN.
    return_info: (flow, info) with info.unsupported, the number of such pixels."""
    like = _like(flow)
    taps = gaussian_taps(sigma, truncate)
    flow = dense_flow(flow)
    weight = _cell_weight(weight, cell_size)
    smooth_flow_params(flow, taps, weight, cell_size, where, min_support)
    ctx = get_context()
    res = ctx.smooth_flow(ctx.asdevice(flow), taps, None if weight is None else ctx.asdevice(weight), cell_size, where,
                          min_support, return_info)
    if isinstance(like, DeviceArray):
        return res
    return (res[0].numpy(), res[1]) if return_info else res.numpy()


def fold_mask(flow, margin=2, return_info=False):
    """keep, (H, W) uint8: 0 at every pixel within `margin` (0 .. 32, Chebyshev distance) of a pixel where the flow is
    not finite or folds -- det J <= 0, the determinant flow_qc() reports -- and 1 elsewhere: the weight that makes
    smooth_flow(where="blend") replace those pixels.  return_info: (keep, info) with info.folded and info.invalid, the
    sums of flow_qc's maps, and info.dropped, the number of zeros in keep."""
    like = _like(flow)
    flow = dense_flow(flow)
    fold_mask_params(flow, margin)
    ctx = get_context()
    res = ctx.fold_mask(ctx.asdevice(flow), margin, return_info)
    if isinstance(like, DeviceArray):
        return res
    return (res[0].numpy(), res[1]) if return_info else res.numpy()


def repair_flow(flow, sigma=6.0, margin=4, max_rounds=8, return_info=False):
    """A finite, fold-free version of `flow`, if the loop gets there: each round takes fold_mask(flow, margin) and stops
    if nothing is folded and nothing invalid; otherwise it replaces the dropped pixels by
    smooth_flow(flow, sigma, weight=keep, where="blend").  A hole wider than the kernel leaves unsupported pixels, which
    come back NaN and are filled from their rim in the next round.  At most `max_rounds` smoothing rounds.

    Convergence is NOT guaranteed: smoothing a fold away can leave a new, smaller one beside it, and with a sigma that is
    small against the folds the loop stalls (on the test field sigma <= 3 does).  return_info: (flow, info) with
    info.rounds, the (folded, invalid, dropped, unsupported) of every smoothing round, and info.converged, whether the
    flow that is returned has nothing folded and nothing invalid.  Raise sigma or margin where it does not converge."""
    like = _like(flow)
    taps = gaussian_taps(sigma)
    flow = dense_flow(flow)
    margin = fold_mask_params(flow, margin)[2]
    smooth_flow_params(flow, taps)
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or int(max_rounds) < 0:
        raise ValueError(f"max_rounds must be a non-negative integer, got {max_rounds!r}")
    ctx = get_context()
    cur = ctx.asdevice(flow)
    rounds, converged = [], None
    for _ in range(int(max_rounds)):
        keep, m = ctx.fold_mask(cur, margin, return_info=True)
        if m.folded == 0 and m.invalid == 0:
            converged = True
            break
        cur, s = ctx.smooth_flow(cur, taps, keep, None, "blend", 0.0, return_info=True)
        rounds.append((m.folded, m.invalid, m.dropped, s.unsupported))
    if converged is None:
        _, m = ctx.fold_mask(cur, margin, return_info=True)
        converged = m.folded == 0 and m.invalid == 0
    if cur is flow:                 # nothing to repair: still a new array, as from every other entry point
        cur = cur.copy()
    out = cur if isinstance(like, DeviceArray) else cur.numpy()
    return (out, RepairInfo(rounds, bool(converged))) if return_info else out
