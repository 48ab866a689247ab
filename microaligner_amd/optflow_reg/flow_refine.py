"""Refining a flow against the images (include/microaligner_flowrefine.h): regularised Lucas-Kanade steps at the scale of a
cell, below what the 99-tap window of register() resolves.  No counterpart in the reference.

    floor = float(np.median(texture_maps(ref, sigma=4.0).lam_min[:200, :200]))      # an empty corner
    flow = refine_flow(ref, mov, flow, floor=floor, tmat=tmat)

Each step warps the ORIGINAL moving image once through `tmat` and the current flow (the warp Warper(tmat=...) applies,
with its 1/32 px coordinate quantum), solves per pixel the 2 x 2 system of the Gaussian-windowed structure tensor of the
warped image plus `floor` on its diagonal against the windowed products of the gradients and warped - ref, and adds the
solution to the flow.  Where the warped image has structure the update follows it; where it has none -- glass -- the
floor makes the update vanish instead of returning noise, and along a straight edge it keeps the component along the edge
at zero.

It is a refinement: its capture range is about sigma, so run register() first.  The update is additive with a re-warp per
step, not a composition.  The warp's zero fill outside the moving image reads as a residual near borders where the flow
points outside: mask it with `weight`.  The smoothing's zero border lowers the tensor within r px of the image's edge, so
steps shrink there.  Gradients come from the warped image only.  Dense flows only (a FlowGrid is expanded first).

Every argument is checked before any device work.
"""
import numpy as np

from ..device import DeviceArray, FlowGrid, FlowRefineInfo, _check_image, _real, affine_flow_params, dense_flow, \
    flow_refine_step_params, gaussian_taps, get_context

_IDENTITY = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))


def refine_flow(ref_img, mov_img, flow=None, *, floor, tmat=None, sigma=4.0, truncate=3.0, num_iter=3, tol=0.0, max_step=1.0,
                weight=None, labels=None, return_info=False):
    """`flow` after up to `num_iter` regularised Lucas-Kanade steps of mov_img against ref_img.

    ref_img: (H, W) uint8, uint16 or float32.  mov_img: the original moving image, as Warper(tmat=...) takes it: (h, w) with
    h <= H and w <= W, padded to (H, W) as pad_to_shape does; tmat: None (the identity) or the 2 x 3 matrix of
    FeatureRegistrator.register().  flow: (H, W, 2) float32, None for zeros, or a FlowGrid, which is expanded first.
    floor: required, finite and > 0, in squared grey levels (of the labels, with labels="dog"): the floor of texture_maps
    for the same images and the same window -- the lam_min of a region known to be empty.  It is added to the diagonal
    of every pixel's system: a pixel no better supported than that region moves by half of what the images ask or less.
    sigma, truncate: the Gaussian window, cut at r = max(1, ceil(truncate * sigma)) <= 128 as in smooth_flow.
    tol: the loop stops after a step whose largest component is <= tol px.  max_step: every component of every step is
    clamped to +-max_step px.
    weight: None, an (H, W) float32 map or a uint8 mask; a weight that is NaN or <= 0 drops its pixel from every sum, as in
    smooth_flow.  labels: None -- the images as they are; "dog" -- both are replaced by the gate's labels first
    (dog(img, True), sigmas 5 / 9, as in assess_registration).
    return_info: (flow, FlowRefineInfo(steps, iterations, converged)), steps being the (step_max, clamped, invalid) of
    every step; the statistics cost a synchronisation per step, which a call with tol == 0 and no return_info does not pay.

    Output kind: that of `flow` (of its nodes, for a FlowGrid) when one is given, else that of ref_img: numpy in, numpy out;
    DeviceArray in, DeviceArray out."""
    if labels is not None and labels != "dog":
        raise ValueError(f"labels must be None or 'dog', got {labels!r}")
    _check_image(ref_img, "ref_img")
    _check_image(mov_img, "mov_img")
    H, W = (int(v) for v in ref_img.shape)
    if flow is None:
        like, flow_shape = ref_img, (H, W, 2)
    elif isinstance(flow, FlowGrid):
        like, flow_shape = flow.nodes, flow.shape + (2,)
    elif isinstance(flow, (np.ndarray, DeviceArray)) and flow.dtype == np.float32:
        like, flow_shape = flow, tuple(flow.shape)
    else:
        raise ValueError("flow must be None, an (H, W, 2) float32 numpy array or DeviceArray, or a FlowGrid")
    if flow_shape != (H, W, 2):
        raise ValueError(f"flow must have shape {(H, W, 2)} for a reference image of {(H, W)}, got {flow_shape}")
    taps = gaussian_taps(sigma, truncate)
    if isinstance(num_iter, bool) or not isinstance(num_iter, (int, np.integer)) or not 1 <= int(num_iter) < 1 << 31:
        raise ValueError(f"num_iter must be an integer >= 1, got {num_iter!r}")
    tol = _real(tol, "tol")
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError(f"tol must be finite and not negative, got {tol!r}")
    tmat = _IDENTITY if tmat is None else tmat
    affine_flow_params(mov_img.shape, np.float32, flow_shape, np.float32, tmat)
    stand_in = np.broadcast_to(np.float32(0), (H, W))      # the shapes and dtypes of what the step will get, no data
    flow_refine_step_params(ref_img, stand_in, np.broadcast_to(np.float32(0), flow_shape), taps, floor, weight, max_step)

    ctx = get_context()
    ref, mov = ctx.asdevice(ref_img), ctx.asdevice(mov_img)
    if labels == "dog":
        from ..shared_modules.registration_qc import _labels
        ref, mov = _labels(ctx, ref, "dog", 0), _labels(ctx, mov, "dog", 0)
    mov = ctx.to_f32(mov)
    weight = None if weight is None else ctx.asdevice(weight)
    if flow is None:
        cur = ctx.zeros((H, W, 2), np.float32)
    elif isinstance(flow, FlowGrid):
        cur = dense_flow(flow)
    else:
        cur = ctx.asdevice(flow).copy()        # the steps update in place, never the caller's array
    want_stats = bool(return_info) or tol > 0
    steps, converged = [], False
    for _ in range(int(num_iter)):
        warped = ctx.warp_affine_flow(mov, cur, tmat, "linear")
        res = ctx.flow_refine_step(ref, warped, cur, taps, floor, weight, max_step, return_info=want_stats, out=cur)
        if want_stats:
            steps.append(res[1])
            if res[1].step_max <= tol:
                converged = True
                break
    out = cur if isinstance(like, DeviceArray) else cur.numpy()
    return (out, FlowRefineInfo(steps, len(steps), converged)) if return_info else out


__all__ = ["refine_flow", "FlowRefineInfo"]
