"""Robust intensity normalisation (include/microaligner_quantile.h): an image scaled to uint8 between two of its percentiles
instead of between its minimum and its maximum, so that one hot pixel, a speck of dust or saturated debris no longer decides
how many grey levels the tissue gets.  No counterpart in the reference, whose read_and_max_project_pages scales between the
extremes; that stays the default everywhere.

The percentiles are exact order statistics of the whole image (numpy's method="lower"), found by a radix select on the
device; the scaling is the rule of the min-max normalisation with (lo, hi) in place of (min, max), values outside clamped."""
import collections
import math

import numpy as np


class NormalizeInfo(collections.namedtuple("NormalizeInfo", "lo hi pop nonfinite zeros degenerate")):
    """normalize_percentile(..., return_info=True): the two values the image was scaled between (NaN when the population is
    empty), the pixels of the population, the NaN / +-Inf pixels and -- with ignore_zeros -- the zeros left out of it, and
    whether the output is all zeros because hi <= lo or because nothing was left to take a percentile of."""


def percentile_params(low, high, ignore_zeros=False):
    """Checks of normalize_percentile without touching a device: (low / 100, high / 100) as float64 quantiles.  low and high
    are percentages with 0 <= low < high <= 100; ignore_zeros is a bool.  ValueError otherwise."""
    vals = []
    for v, name in ((low, "low"), (high, "high")):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a percentage, got {v!r}")
        vals.append(float(v))
    low, high = vals
    if not (0.0 <= low < high <= 100.0):                   # false for a NaN
        raise ValueError(f"percentiles must satisfy 0 <= low < high <= 100, got {low!r} and {high!r}")
    if not isinstance(ignore_zeros, (bool, np.bool_)):
        raise ValueError(f"ignore_zeros must be a bool, got {ignore_zeros!r}")
    return low / 100.0, high / 100.0


def percentile_ranks(low, high, pop):
    """The zero-based ranks of the two percentiles in a population of pop > 0 pixels: floor(q * (pop - 1)), q = p / 100."""
    qlo, qhi = percentile_params(low, high)
    return int(math.floor(qlo * float(pop - 1))), int(math.floor(qhi * float(pop - 1)))


def normalize_percentile(img, low=0.0, high=99.9, ignore_zeros=False, on_device=False, return_info=False):
    """img (uint8 / uint16 / float32, numpy or DeviceArray) scaled to uint8 so that its low-th percentile maps to 0 and its
    high-th to 255; values outside are clamped, NaN becomes 0.  The percentiles are order statistics q = p / 100 of the
    finite pixels (without the zeros with ignore_zeros: padded mosaics, sparse nuclei).  numpy in, numpy out; a DeviceArray
    comes back with on_device=True.  Data never raises: where hi <= lo or no pixel is left the output is all zeros and
    NormalizeInfo.degenerate is set.  With return_info: (image, NormalizeInfo)."""
    from ..device import DeviceArray, get_context
    qlo, qhi = percentile_params(low, high, ignore_zeros)
    ctx = get_context()
    dev = img if isinstance(img, DeviceArray) else ctx.asdevice(np.ascontiguousarray(img))
    (lo, hi), counts = ctx.image_quantiles(dev, [qlo, qhi], ignore_zeros=bool(ignore_zeros))
    lo, hi = float(lo), float(hi)
    degenerate = counts.pop == 0 or not hi > lo
    if counts.pop == 0:
        out = ctx.zeros(dev.shape, np.uint8)
    else:
        out = ctx.normalize_range_u8(dev, lo, hi)
    if not on_device:
        out = out.numpy()
    if return_info:
        return out, NormalizeInfo(lo, hi, counts.pop, counts.nonfinite, counts.zeros, bool(degenerate))
    return out
