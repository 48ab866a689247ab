"""Filling a flow across holes of any size (include/microaligner_flowfill.h): a push-pull fill.  A weighted pyramid of the
kept vectors is pulled to 1 x 1 and pushed back, kept pixels overriding, so the result is finite everywhere one vector was
kept, at a cost that does not depend on the size of the holes.  No counterpart in the reference.

    fill_flow(f)                                               non-finite vectors are filled from the finite ones
    fill_flow(f, weight=keep)                                  and so is every pixel whose keep is 0
    fill_flow(f, weight=local_correlation(...).weight)         soft weights blend the flow with the fill

Every argument is checked before any device work.  numpy in, numpy out; DeviceArray in, DeviceArray out.  A FlowGrid is
expanded on the device first (device.dense_flow) and gives the kind of array its nodes are.
"""
from ..device import DeviceArray, FillInfo, dense_flow, fill_flow_params, get_context  # noqa: F401
from .flow_smooth import _cell_weight, _like


def fill_flow(flow, weight=None, cell_size=None, return_info=False):
    """The (H, W, 2) float32 flow with every pixel that is not kept replaced by an extrapolation of the kept ones, however
    far away they are: each kept pixel enters a pyramid of weighted 2 x 2 means that ends at 1 x 1, and the pyramid is
    expanded back bilinearly, a level's own values overriding what comes from above.

    weight: what it is for smooth_flow -- None; an (H, W) float32 map or uint8 mask; or, with cell_size (an int or
    (cell_h, cell_w)), a (gy, gx) map on that cell grid.  A pixel whose weight is NaN, negative or 0, or whose flow is not
    finite, is dropped and filled.  A pixel of weight >= 1 comes back bit for bit; weights saturate at 1.  A weight in
    (0, 1) blends: out = fill + weight * (flow - fill).
    With every pixel dropped the result is NaN everywhere.
    return_info: (flow, info) with info.dropped, info.blended, info.unsupported (output pixels that are not finite) and
    info.levels (pyramid levels above the flow)."""
    like = _like(flow)
    flow = dense_flow(flow)
    weight = _cell_weight(weight, cell_size)
    fill_flow_params(flow, weight, cell_size)
    ctx = get_context()
    res = ctx.fill_flow(ctx.asdevice(flow), None if weight is None else ctx.asdevice(weight), cell_size, return_info)
    if isinstance(like, DeviceArray):
        return res
    return (res[0].numpy(), res[1]) if return_info else res.numpy()
