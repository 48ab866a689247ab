"""Connected components of an image on the GPU (include/microaligner_components.h): labels, the areas and boxes of the
components, and the two filters built from them.  Everything is integer and defined without a traversal order: the same
bits on every run.

What no local filter can do to a mask before it becomes a weight:

    tissue = grey_close((img > t).astype(np.uint8), 5)
    tissue = fill_holes(remove_small_objects(tissue, 500), max_size=10_000)   # specks of any shape out, enclosed gaps in
    flow = fill_flow(flow, weight=tissue)

Finding the fragments a nearest-neighbour warp tore a label image into:

    pieces, info = label_components(warped_labels, by_value=True, return_info=True)
"""
import collections

import numpy as np


class ComponentInfo(collections.namedtuple("ComponentInfo", "count areas bboxes")):
    """label_components(..., return_info=True): count, the number n of components; areas, int64 (n + 1,), areas[0] the
    number of background pixels; bboxes, int32 (n + 1, 4), y0, x0, y1, x1 of every component with the ends exclusive
    (scipy.ndimage.find_objects as numbers), row 0 zeros."""


def _prepare(img, on_device, check, *args):
    from ..device import get_context
    if not isinstance(on_device, (bool, np.bool_)):
        raise ValueError(f"on_device must be a bool, got {on_device!r}")
    check(img, *args)                                     # refusals before a context is made
    ctx = get_context()
    return ctx, ctx.components_asdevice(img)


def label_components(img, connectivity=1, by_value=False, *, on_device=False, return_info=False):
    """The connected components of img, an (H, W) uint8, uint16 or int32 image (numpy or DeviceArray; a numpy bool array is
    taken as uint8; H * W <= 2^31 - 1): int32 labels (H, W), 0 for background -- the pixels that are 0 -- and k = 1 .. n for
    the k-th component in ascending order of the components' smallest linear index y * W + x.  connectivity=1 joins the 4
    edge neighbours, 2 the 8 neighbours; by_value=True joins neighbours only where their values are equal, so a label
    image falls into the connected pieces of its labels.  With by_value=False the result is scipy.ndimage.label(img != 0,
    generate_binary_structure(2, connectivity))[0].  return_info=True: (labels, ComponentInfo).  numpy in, numpy out; a
    DeviceArray comes back with on_device=True (the ComponentInfo is always on the host)."""
    from ..device import components_params
    if not isinstance(return_info, (bool, np.bool_)):
        raise ValueError(f"return_info must be a bool, got {return_info!r}")
    ctx, dev = _prepare(img, on_device, components_params, connectivity, by_value)
    labels, n = ctx.label_components(dev, connectivity, by_value)
    info = None
    if return_info:
        areas, bboxes = ctx.component_stats(labels, n)
        info = ComponentInfo(n, areas.numpy(), bboxes.numpy())
    out = labels if on_device else labels.numpy()
    return (out, info) if return_info else out


def remove_small_objects(img, min_size, connectivity=1, by_value=False, *, on_device=False):
    """img with every foreground pixel set to 0 whose component -- label_components' components under the same connectivity
    and by_value -- has fewer than min_size pixels, whatever its shape; every other pixel comes back bit for bit, in img's
    dtype.  min_size: an int >= 0; 0 and 1 return the image unchanged."""
    from ..device import remove_small_params
    ctx, dev = _prepare(img, on_device, remove_small_params, min_size, connectivity, by_value)
    out = ctx.remove_small_objects(dev, min_size, connectivity, by_value)
    return out if on_device else out.numpy()


def fill_holes(img, max_size=None, connectivity=1, value=1, *, on_device=False):
    """img with every enclosed hole set to `value` (an int in 1 .. the largest value of img's dtype); every other pixel comes
    back bit for bit, in img's dtype.  The components are those of the background, the pixels that are 0, joined under
    `connectivity`; one is a hole when it has no pixel in row 0, row H - 1, column 0 or column W - 1 and, with max_size
    given, at most max_size pixels.  With max_size=None on a 0/1 mask this is scipy.ndimage.binary_fill_holes(img != 0,
    generate_binary_structure(2, connectivity))."""
    from ..device import fill_holes_params
    ctx, dev = _prepare(img, on_device, fill_holes_params, max_size, connectivity, value)
    out = ctx.fill_holes(dev, max_size, connectivity, value)
    return out if on_device else out.numpy()
