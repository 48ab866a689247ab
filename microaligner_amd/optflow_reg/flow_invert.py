"""Coordinates through a registration (include/microaligner_flowinvert.h): the dense inverse of a flow and points mapped
between the registered frame (the flow's grid, where the reference lives) and the moving frame (the original moving
image).  No counterpart in the reference, which moves pixels only.  With warp(img, f)(p) = img(p - f(p)):

    invert_flow(f) = g with g(q) = -f(q - g(q)), so that compose_flows(f, g) ~ 0
    transform_points(p, f, "to_moving") = M . (p - f(p)) - padding       (the coordinate Warper samples at)
    transform_points(s, f, "to_reference") = the p with p - f(p) = tmat . (s + padding)

Every argument is checked before any device work.  A FlowGrid stands for its flow: transform_points samples its nodes
natively, invert_flow expands it on the device first (device.dense_flow).
"""
from ..device import DeviceArray, FlowGrid, dense_flow, get_context, invert_flow_params, transform_points_params


def invert_flow(flow, max_iter=50, tol=1e-3, return_info=False):
    """The inverse of an (H, W, 2) float32 flow by a per-pixel fixed-point iteration in one kernel: numpy in, numpy out;
    DeviceArray in, DeviceArray out.  The iteration stops at a pixel when a step moves it by at most `tol` px in x and y,
    or after `max_iter` steps.  It converges where the flow is a contraction (adjacent differences below 1 px per px in
    sum) and not where the flow folds.  return_info: (inverse, info) with info.not_converged, the number of pixels that
    used all max_iter steps, and info.residual, the (H, W) float32 size of every pixel's last step.  A FlowGrid is expanded
    on the device first and gives the kind of array its nodes are."""
    like = flow.nodes if isinstance(flow, FlowGrid) else flow
    flow = dense_flow(flow)
    invert_flow_params(flow, max_iter, tol)
    ctx = get_context()
    res = ctx.invert_flow(ctx.asdevice(flow), max_iter, tol, return_info)
    if isinstance(like, DeviceArray):
        return res
    if not return_info:
        return res.numpy()
    out, info = res
    return out.numpy(), info._replace(residual=info.residual.numpy())


def transform_points(points, flow, direction, tmat=None, image_shape=None, max_iter=50, tol=1e-4, return_info=False):
    """(N, 2) float64 points (x, y) through the registration `flow` (numpy or device resident, (H, W, 2) float32, or a
    FlowGrid, whose nodes the kernel samples in float64 without building the flow) and,
    optionally, the 2x3 `tmat` that Warper.tmat takes, with `image_shape` the (h, w) of the moving image it resamples
    (default: the flow's).  direction "to_moving": registered frame -> moving image, one pass; "to_reference": moving
    image -> registered frame, a fixed-point iteration per point in float64 that stops when a step is at most `tol` px
    or after `max_iter` steps.  Returns the points as a new float64 array; with return_info also info.converged and
    info.inside, bool arrays of length N (inside: the registered-frame coordinate lies within the flow's grid)."""
    transform_points_params(points, flow, direction, tmat, image_shape, max_iter, tol)
    return get_context().transform_points(points, flow, direction, tmat, image_shape, max_iter, tol, return_info)
