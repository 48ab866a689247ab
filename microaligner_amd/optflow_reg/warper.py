"""Tiled backward warp (counterpart of microaligner/optflow_reg/warper.py:29-76).

One HIP kernel evaluates, per output pixel, the window the reference would have cut
(tile_size + 2*overlap, zero padded), the window-local map float32(x_local - flow) and the
cv2.remap arithmetic of `interpolation`: INTER_LINEAR by default, as the reference calls it (fixed point
for uint8, float for uint16/float32), or INTER_NEAREST / INTER_CUBIC / INTER_LANCZOS4
(include/microaligner_interp.h).

With `tmat` set to a 2x3 matrix (FeatureRegistrator.register()'s, the one transform_img_with_tmat takes) the image is
the ORIGINAL moving image and is resampled once, through the matrix and the flow together
(include/microaligner_compose.h): the result has the flow's shape, covers the whole image (tile_size / overlap do not
apply) and differs from transform_img_with_tmat followed by a plain warp, which interpolates twice.

`flow` may be a FlowGrid (include/microaligner_flowgrid.h): the nodes are evaluated inside that same whole-image warp,
with `tmat` or, when it is None, the identity and no padding.  This is the whole-image warp of `tmat`, NOT the tiled one
of a dense flow without a matrix, which zeroes samples beyond a tile's window: the result is
warp_affine_flow(image, grid.expand(), tmat) bit for bit.
"""
import numpy as np

from .._lib import MA_INTER_LINEAR as INTER_LINEAR
from ..device import DeviceArray, FlowGrid, affine_flow_params, affine_grid_params, get_context, interp_code


def _mode(interp):
    """keyword arguments of the Context calls: none for the default linear mode, whose calls stay exactly as they were"""
    return {} if interp == INTER_LINEAR else {"interpolation": interp}


class Warper:
    HOST_BANDED_MIN = 64 << 20   # bytes; below this a page is a band or two and the plain upload / warp / download is as fast

    def __init__(self):
        self.image = np.array([])
        self.flow = np.array([])
        self.tile_size = 1000
        self.overlap = 100
        # "nearest", "linear", "cubic", "lanczos4" or cv2's codes 0, 1, 2, 4; checked before any device work
        self.interpolation = "linear"
        # None, or the 2x3 affine initialisation of `image`: one resampling through it and the flow (module docstring)
        self.tmat = None

    def warp(self):
        if len(self.image) == 0:
            raise ValueError("No image provided")
        if len(self.flow) == 0:
            raise ValueError("No flow provided")
        interp = interp_code(self.interpolation)
        if self.tmat is not None or isinstance(self.flow, FlowGrid):
            return self._warp_affine_flow()
        ctx = get_context()
        like = self.image
        if np.ndim(like) != 2:
            raise ValueError(f"Expected 2D grayscale image, got shape {np.shape(like)}")
        if isinstance(like, np.ndarray) and like.nbytes >= self.HOST_BANDED_MIN:
            like = np.ascontiguousarray(like)      # a strided view is gathered once, here
        if isinstance(like, np.ndarray) and like.nbytes >= self.HOST_BANDED_MIN and not ctx.is_resident(like):
            # a large host page that is not in HBM yet (the reference's own per-page loop, __main__.py:288-302, kept by a
            # caller who only swapped the import): the page-warp driver moves it in bands of tile rows, so upload,
            # kernel and download of the one page overlap
            flow = ctx.asdevice(self.flow)
            out = ctx.host_empty(like.shape, like.dtype)
            ctx.warp_pages([like], flow, self.tile_size, self.overlap, [out], **_mode(interp))
            self.image = np.array([])
            self.flow = np.array([])
            return out
        img, flow = ctx.asdevice(like), ctx.asdevice(self.flow)
        out = ctx.warp(img, flow, self.tile_size, self.overlap, **_mode(interp))
        # like the reference (warper.py:41,45) the inputs are consumed
        self.image = np.array([])
        self.flow = np.array([])
        return out if isinstance(like, DeviceArray) else out.numpy()

    def _params(self, like):
        """affine_flow_params of `like` against the flow and tmat: every check before any device work"""
        if np.ndim(like) != 2:
            raise ValueError(f"Expected 2D grayscale image, got shape {np.shape(like)}")
        if isinstance(self.flow, FlowGrid):
            return affine_grid_params(np.shape(like), like.dtype, self.flow, self.tmat, self.interpolation)
        return affine_flow_params(np.shape(like), like.dtype, np.shape(self.flow), self.flow.dtype, self.tmat,
                                  self.interpolation)

    def _warp_affine_flow(self):
        like = self.image
        self._params(like)
        interp, tmat = interp_code(self.interpolation), self.tmat
        ctx = get_context()
        # a dense flow or a grid: the same two calls, the resident and the page driver's
        if isinstance(self.flow, FlowGrid):
            flow, warp, warp_pages = self.flow, ctx.warp_affine_grid, ctx.warp_affine_grid_pages
        else:
            flow, warp, warp_pages = ctx.asdevice(self.flow), ctx.warp_affine_flow, ctx.warp_affine_flow_pages
        if isinstance(like, np.ndarray) and like.nbytes >= self.HOST_BANDED_MIN:
            like = np.ascontiguousarray(like)
        if isinstance(like, np.ndarray) and like.nbytes >= self.HOST_BANDED_MIN and not ctx.is_resident(like):
            # a large host page: the page driver uploads it whole and downloads the result in bands under the kernel
            out = ctx.host_empty(flow.shape[:2], like.dtype)
            warp_pages([like], flow, tmat, [out], interpolation=interp)
        else:
            out = warp(ctx.asdevice(like), flow, tmat, interpolation=interp)
            if not isinstance(like, DeviceArray):
                out = out.numpy()
        # the matrix is consumed with the image and the flow
        self.image = np.array([])
        self.flow = np.array([])
        self.tmat = None
        return out

    def warp_pages(self, pages, out=None):
        """Apply `self.flow` to many pages (the channel x z pages of a cycle, __main__.py:288-302,427-433) with the
        flow uploaded once and the page transfers overlapped.  Unlike warp() this keeps `self.flow` (and `self.tmat`:
        with a matrix every page is resampled once through it and the flow, and `out` holds arrays of the flow's shape)."""
        if len(self.flow) == 0:
            raise ValueError("No flow provided")
        interp = interp_code(self.interpolation)
        grid = self.flow if isinstance(self.flow, FlowGrid) else None
        if self.tmat is not None or grid is not None:
            pages = [np.ascontiguousarray(p) for p in pages]
            for p in pages:
                self._params(p)
        ctx = get_context()
        if grid is not None:
            # the nodes stay resident for further calls, as a flow does
            self.flow = grid = FlowGrid(ctx.asdevice(grid.nodes), grid.stride, grid.shape)
            return ctx.warp_affine_grid_pages(pages, grid, self.tmat, out, interpolation=interp)
        flow = ctx.asdevice(self.flow)
        self.flow = flow  # stays resident for further calls
        if self.tmat is not None:
            return ctx.warp_affine_flow_pages(pages, flow, self.tmat, out, interpolation=interp)
        return ctx.warp_pages(pages, flow, self.tile_size, self.overlap, out, **_mode(interp))
