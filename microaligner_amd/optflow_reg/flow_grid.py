"""Grid flows (include/microaligner_flowgrid.h): keep a registration at 1 / stride^2 of its size and use it from there.

    grid = compress_flow(flow)                       # the largest stride that loses at most 1/32 px
    grid.save("cycle002.npz"); grid = FlowGrid.load("cycle002.npz")
    warper.flow = grid; warper.warp_pages(pages)     # the nodes are evaluated inside the warp kernel
    transform_points(points, grid, "to_moving")

A Farneback flow is smooth at the scale of its window, so its values on a coarse grid of nodes and bilinear interpolation
between them give it back to a small fraction of a pixel; flow_grid_error() says how small, per cell and in pixels.  No
counterpart in the reference.  Every argument is checked before any device work.
"""
from dataclasses import dataclass

import numpy as np

from ..device import DeviceArray, FlowGrid, _check_flow, _check_stride, get_context
from ..shared_modules.registration_qc import cell_bounds, cell_size_hw

STRIDES = (64, 32, 16, 8, 4, 2, 1)   # what compress_flow() tries, in this order
DEFAULT_TOL = 1.0 / 32               # the warps' own coordinate quantum: cv2.remap and every warp here quantise the map to it


@dataclass
class FlowGridError:
    """What a grid loses against the dense flow, per cell (flow_grid_error()); every map is (gy, gx)."""
    cell_bounds: np.ndarray
    max_err: np.ndarray     # float32: max over the cell's valid pixels of max(|E.x - f.x|, |E.y - f.y|) (NaN if none)
    above: np.ndarray       # int64: valid pixels whose error exceeds tol
    invalid: np.ndarray     # int64: pixels where either difference is NaN
    stride: int
    tol: float

    @property
    def global_max_err(self) -> float:
        """The largest max_err of all cells; NaN when no cell has a valid pixel."""
        return global_max_err(self.max_err)

    def summary(self) -> dict:
        return {"cells": int(self.max_err.size), "stride": self.stride, "tol": self.tol, "max_err": self.global_max_err,
                "above": int(self.above.sum()), "invalid": int(self.invalid.sum())}


def global_max_err(max_err):
    valid = max_err[~np.isnan(max_err)]
    return float(valid.max()) if valid.size else float("nan")


def qualifies(max_err, invalid, tol):
    """compress_flow()'s test of one stride's maps: no invalid pixel and no cell above tol."""
    return int(np.sum(invalid)) == 0 and global_max_err(max_err) <= tol


def choose_stride(maps_of, tol, strides=STRIDES):
    """The first stride of `strides` whose maps qualify, with those maps: (stride, (max_err, above, invalid)).
    maps_of(stride) gives the three maps.  The last stride is taken whatever its maps say: stride 1 is the flow itself."""
    for s in strides[:-1]:
        maps = maps_of(s)
        if qualifies(maps[0], maps[2], tol):
            return s, maps
    return strides[-1], maps_of(strides[-1])


def _check_tol(tol):
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not float(tol) >= 0:
        raise ValueError(f"tol must be a number >= 0, got {tol!r}")
    return float(np.float32(tol))


def _host_nodes(grid, like):
    """numpy flow in, numpy nodes out; device flow in, device nodes out"""
    return grid if isinstance(like, DeviceArray) else FlowGrid(grid.nodes.numpy(), grid.stride, grid.shape)


def flow_grid_error(flow, grid, cell_size=1000, tol=DEFAULT_TOL) -> FlowGridError:
    """Per cell of `cell_size` (an int or (cell_h, cell_w)): the largest error of `grid` against the (H, W, 2) float32
    `flow` in pixels, the number of pixels above `tol` and the number of invalid ones.  A maximum and two counts, so the
    maps do not depend on the order of the reduction."""
    H, W = _check_flow(flow)
    if not isinstance(grid, FlowGrid):
        raise ValueError(f"grid must be a FlowGrid, got {type(grid).__name__}")
    if grid.shape != (H, W):
        raise ValueError(f"the grid belongs to a flow of shape {grid.shape}, got {(H, W)}")
    ch, cw = cell_size_hw(cell_size)
    tol = _check_tol(tol)
    ctx = get_context()
    max_err, above, invalid = ctx.flow_grid_error(ctx.asdevice(flow), grid, ch, cw, tol)
    return FlowGridError(cell_bounds((H, W), (ch, cw)), max_err, above, invalid, grid.stride, tol)


def compress_flow(flow, stride=None, tol=DEFAULT_TOL, cell_size=1000, return_error=False):
    """The FlowGrid of an (H, W, 2) float32 flow: numpy in, numpy nodes; DeviceArray in, device nodes.  With `stride` the
    flow is sampled there.  Without, the largest stride of 64, 32, 16, 8, 4, 2, 1 whose error is at most `tol` px everywhere
    with no invalid pixel is taken (stride 1, the flow itself, when none is).  return_error: (grid, FlowGridError)."""
    H, W = _check_flow(flow)
    if stride is not None:
        stride = _check_stride(stride)
    ch, cw = cell_size_hw(cell_size)
    tol = _check_tol(tol)
    ctx = get_context()
    d_flow = ctx.asdevice(flow)
    grids = {}

    def maps_of(s):
        grids[s] = ctx.flow_grid_sample(d_flow, s)
        return ctx.flow_grid_error(d_flow, grids[s], ch, cw, tol)

    if stride is None:
        stride, maps = choose_stride(maps_of, tol)
    elif return_error:
        maps = maps_of(stride)
    else:
        grids[stride] = ctx.flow_grid_sample(d_flow, stride)
    grid = _host_nodes(grids[stride], flow)
    if not return_error:
        return grid
    return grid, FlowGridError(cell_bounds((H, W), (ch, cw)), *maps, stride, tol)
