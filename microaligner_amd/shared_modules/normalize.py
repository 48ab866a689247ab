"""Robust intensity normalisation (include/microaligner_quantile.h): an image scaled to uint8 between two of its percentiles
instead of between its minimum and its maximum, so that one hot pixel, a speck of dust or saturated debris no longer decides
how many grey levels the tissue gets.  No counterpart in the reference, whose read_and_max_project_pages scales between the
extremes; that stays the default everywhere.

The percentiles are exact order statistics of the whole image (numpy's method="lower"), found by a radix select on the
device; the scaling is the rule of the min-max normalisation with (lo, hi) in place of (min, max), values outside clamped."""
import collections
import math

import numpy as np

from ..device import LocalNormInfo  # noqa: F401  (what normalize_local(..., return_info=True) returns)


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


# ---- local contrast normalisation (include/microaligner_localnorm.h) --------------------------------------------------------
# A gain and an offset that vary slowly over the image -- bleaching between the cycles, uneven stripping, the illumination
# of mosaic tiles -- are what neither normalisation above removes: both fix one gain for the whole image.  Here every pixel
# is taken relative to the Gaussian-windowed mean and standard deviation around it, so two images of one structure come out
# with one grey level, which is what Farneback assumes of its inputs:
#
#     oreg.ref_img, oreg.mov_img = normalize_local(ref, floor=f), normalize_local(mov, floor=f)
LOCALNORM_DTYPES = {"uint8": "u8", "float32": "f32"}


def local_norm_call_params(sigma, truncate, dtype, on_device, return_info):
    """Checks of normalize_local that are its own, without touching a device: (taps, the plane's name).  The image, floor,
    clip, weight and min_support are device.local_norm_params'."""
    from ..device import gaussian_taps
    taps = gaussian_taps(sigma, truncate)
    if isinstance(dtype, type) or isinstance(dtype, np.dtype):
        dtype = np.dtype(dtype).name
    if not isinstance(dtype, str) or dtype not in LOCALNORM_DTYPES:
        raise ValueError(f'dtype must be "uint8" or "float32", got {dtype!r}')
    for v, name in ((on_device, "on_device"), (return_info, "return_info")):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, got {v!r}")
    return taps, LOCALNORM_DTYPES[dtype]


def normalize_local(img, sigma=16.0, *, floor, clip=4.0, weight=None, truncate=3.0, min_support=0.0, dtype="uint8",
                    on_device=False, return_info=False):
    """img (uint8 / uint16 / float32, numpy or DeviceArray) with its local mean taken out and divided by its local standard
    deviation: z = (x - mu) / sqrt(v + floor), mu and v the mean and the variance under a Gaussian window of `sigma` px cut
    at truncate * sigma (at most 128 px).  dtype "uint8": z * 127 / clip + 128 rounded into 0 .. 255, what register() takes;
    "float32": z clipped to +-clip (clip may be inf).  floor, in squared grey levels of img, is the variance below which a
    window counts as empty (bare glass: its noise variance); there z goes to 0 instead of amplifying the noise.  weight:
    None, or an (H, W) float32 map or uint8 mask (numpy or DeviceArray); pixels without weight, NaN / Inf pixels and pixels
    whose window holds no more than min_support of weight give 0.0 / 128 and put no edge at the mask's rim.  Choose sigma
    above the size of the structures and below the scale of the gain field.  numpy in, numpy out; a DeviceArray comes back
    with on_device=True.  With return_info: (image, LocalNormInfo(dropped, unsupported, flat, clipped))."""
    from ..device import DeviceArray, get_context, local_norm_params
    taps, plane = local_norm_call_params(sigma, truncate, dtype, on_device, return_info)
    local_norm_params(img, taps, floor, clip, weight, min_support, (plane,))        # refusals before a context is made
    ctx = get_context()
    dev = img if isinstance(img, DeviceArray) else ctx.asdevice(np.ascontiguousarray(img))
    wdev = weight if weight is None or isinstance(weight, DeviceArray) else ctx.asdevice(np.ascontiguousarray(weight))
    res = ctx.normalize_local(dev, taps, floor, clip, wdev, min_support, (plane,), return_info=bool(return_info))
    out, info = res if return_info else (res, None)
    out = out[plane] if on_device else out[plane].numpy()
    return (out, info) if return_info else out
