"""Flat grey morphology of an image on the GPU (include/microaligner_morphology.h): the running minimum and maximum over a
rectangle cut at the border, and opening, closing and the two top-hats built from them.  Exact: an order statistic has no
rounding, so every result but a hat's is one of the input values, bit for bit.

Editing a mask before it becomes a weight:

    keep = outlier_mask(flow)                          # uint8, 1 = keep
    keep = grey_erode(keep, 10)                        # stay 10 px off every hole's rim
    keep = grey_open(keep, 3)                          # drop specks narrower than 7 px
    tissue = grey_close((img > t).astype(np.uint8), 5) # bridge gaps of up to 10 px
    flow = fill_flow(flow, weight=keep)

Removing an uneven additive background before a registration:

    oreg.ref_img, oreg.mov_img = tophat(ref, 25), tophat(mov, 25)   # radius above the widest nucleus
"""
import numpy as np


def _call(img, op, radius, on_device):
    from ..device import DeviceArray, get_context, morphology_params
    if not isinstance(on_device, (bool, np.bool_)):
        raise ValueError(f"on_device must be a bool, got {on_device!r}")
    morphology_params(img, op, radius)                     # refusals before a context is made
    ctx = get_context()
    dev = img if isinstance(img, DeviceArray) else ctx.asdevice(np.ascontiguousarray(img))
    out = ctx.morphology(dev, op, radius)
    return out if on_device else out.numpy()


def grey_erode(img, radius, *, on_device=False):
    """The smallest value of img (uint8 / uint16 / float32, numpy or DeviceArray, 2-D) in the rectangle of
    (2 ry + 1) x (2 rx + 1) pixels around each pixel, radius = r or (ry, rx), each an int in 0 .. 255.  The window is cut at
    the border; float32 NaNs take no part, and a window of NaNs only gives NaN.  On a mask: shrinks it by the radius.  numpy
    in, numpy out; a DeviceArray comes back with on_device=True."""
    return _call(img, "erode", radius, on_device)


def grey_dilate(img, radius, *, on_device=False):
    """The largest value of img in the rectangle around each pixel: grey_erode with the order reversed.  On a mask: grows it
    by the radius."""
    return _call(img, "dilate", radius, on_device)


def grey_open(img, radius, *, on_device=False):
    """grey_dilate(grey_erode(img)): removes what is brighter than its surroundings and does not hold the rectangle, and
    leaves the rest where it was.  On a mask: deletes specks lower than 2 ry + 1 or narrower than 2 rx + 1."""
    return _call(img, "open", radius, on_device)


def grey_close(img, radius, *, on_device=False):
    """grey_erode(grey_dilate(img)): fills what is darker than its surroundings and does not hold the rectangle.  On a mask:
    closes gaps and holes narrower than the rectangle."""
    return _call(img, "close", radius, on_device)


def tophat(img, radius, black=False, *, on_device=False):
    """The white top-hat img - grey_open(img): what is brighter than its surroundings and narrower than the rectangle, at
    its own grey levels, with everything wider -- an uneven additive background -- removed.  black=True: the black top-hat
    grey_close(img) - img, the same for dark structures.  Exact and >= 0 for uint8 and uint16; one rounded subtraction for
    float32, NaN where the pixel is NaN."""
    if not isinstance(black, (bool, np.bool_)):
        raise ValueError(f"black must be a bool, got {black!r}")
    return _call(img, "blackhat" if black else "tophat", radius, on_device)
