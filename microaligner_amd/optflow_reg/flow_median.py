"""Median-filtering a flow (include/microaligner_flowmedian.h): the exact windowed median of each component, which removes
isolated wrong vectors, keeps motion edges and leaves an affine flow untouched, and the mask of the vectors that lie far
from the median of their surroundings.  No counterpart in the reference.

    median_flow(f, radius=2)                                    every pixel takes the median of its 5 x 5 window
    median_flow(f, radius=2, where="outliers", thresh=1.0)      only vectors more than 1 px from it do; the rest untouched
    outlier_mask(f, radius=2, thresh=1.0)                       keep: 0 at those vectors, the weight smooth_flow() takes

Every argument is checked before any device work.  numpy in, numpy out; DeviceArray in, DeviceArray out.  A FlowGrid is
expanded on the device first (device.dense_flow) and gives the kind of array its nodes are.
"""
from ..device import DeviceArray, MedianInfo, dense_flow, get_context, median_flow_params  # noqa: F401
from .flow_smooth import _cell_weight, _like


def _run(flow, radius, weight, cell_size, where, thresh, return_info, out, keep):
    like = _like(flow)
    flow = dense_flow(flow)
    weight = _cell_weight(weight, cell_size)
    median_flow_params(flow, radius, weight, cell_size, where, thresh)
    ctx = get_context()
    res = ctx.median_flow(ctx.asdevice(flow), radius, None if weight is None else ctx.asdevice(weight), cell_size, where,
                          thresh, return_info, out=out, keep=keep)
    if isinstance(like, DeviceArray):
        return res
    return (res[0].numpy(), res[1]) if return_info else res.numpy()


def median_flow(flow, radius=2, weight=None, cell_size=None, where="all", thresh=None, return_info=False):
    """The (H, W, 2) float32 flow with each component replaced by the median of its (2 radius + 1)^2 window, radius 1 .. 7.
    The window is cut at the image's border, not padded; of an even number of values the lower median is taken, so the
    result is always one of the input values, bit for bit.

    weight: what it is for smooth_flow -- None; an (H, W) float32 map or uint8 mask; or, with cell_size (an int or
    (cell_h, cell_w)), a (gy, gx) map on that cell grid -- read as a mask: a pixel whose weight is NaN, negative or 0, or
    whose flow is not finite, takes no part in any window and always takes its window's median.
    where: "all" -- every pixel takes the median; "outliers" -- only pixels that take no part and pixels farther than
    `thresh` px (the larger of the two components' distances) from the median do, every other pixel comes back bit for
    bit.  where="outliers" needs a thresh; with where="all" a thresh only feeds the counts.
    A pixel with no participating pixel in its window comes back NaN.
    return_info: (flow, info) with info.outliers, info.dropped and info.unsupported."""
    return _run(flow, radius, weight, cell_size, where, thresh, return_info, None, False)


def outlier_mask(flow, radius=2, thresh=1.0, weight=None, cell_size=None, return_info=False):
    """keep, (H, W) uint8: 0 at every pixel that is farther than `thresh` px from the median of its (2 radius + 1)^2 window
    (the larger of the two components' distances) or that takes no part (weight NaN, negative or 0, or a flow that is not
    finite), and 1 elsewhere: a subset of the `weight` it was given, and itself a weight for smooth_flow(where="blend").
    return_info: (keep, info) with info.outliers, info.dropped and info.unsupported."""
    if thresh is None:
        raise ValueError("outlier_mask needs a thresh")
    return _run(flow, radius, weight, cell_size, "all", thresh, return_info, False, True)
