/* Intensity-based affine alignment: the Gauss-Newton moments of the weighted squared difference between a reference image
 * and a moving image sampled through a 2 x 3 matrix, with a gain and a bias between the two.  An extension of
 * libmicroaligner_hip.so with no counterpart in the reference.  Off the measured path (build.source_hash() does not cover
 * it).  Whole image, no tile windows.
 *
 * All arithmetic is float64 and every operation is rounded on its own: nothing is fused.  ref and mov are (H, W) images of
 * one dtype each (MA_U8, MA_U16 or MA_F32, independently of each other), 1 <= H, W <= 2^24; pixel values are widened to
 * float64 (exact).
 *
 * Inputs: M (6 doubles, row-major 2 x 3) takes absolute reference pixel coordinates to absolute coordinates of the moving
 * image; gain, bias; a weight by weight_kind (enum ma_smooth_weight_kind of microaligner_flowsmooth.h):
 *      MA_SMOOTH_WEIGHT_NONE : weight(p) = 1 (the pointer is ignored);
 *      MA_SMOOTH_WEIGHT_F32  : an (H, W) float32 map;
 *      MA_SMOOTH_WEIGHT_U8   : an (H, W) uint8 mask, nonzero = 1.0, zero = 0.0;
 *      MA_SMOOTH_WEIGHT_CELLS is refused;
 * clip: a residual in grey levels beyond which a pixel is left out; clip <= 0 or NaN means no clipping.
 *
 * Per pixel p = (x, y), with c = ((W - 1) / 2, (H - 1) / 2), X = x - c_x, Y = y - c_y (exact):
 *      sx = (M[0] * x + M[1] * y) + M[2],  sy = (M[3] * x + M[4] * y) + M[5];
 *      x0 = floor(sx), y0 = floor(sy);
 *      the pixel is inside iff 0 <= x0 <= W - 2 and 0 <= y0 <= H - 2 (a NaN fails): no border mode is applied, and an
 *      image with a side of 1 has no inside pixel;
 *      tx = sx - x0, ty = sy - y0 (exact); the taps a00 = mov(x0, y0), a01 = mov(x0 + 1, y0), a10 = mov(x0, y0 + 1),
 *      a11 = mov(x0 + 1, y0 + 1);
 *      d0 = a01 - a00, d1 = a11 - a10;
 *      top = a00 + d0 * tx, bot = a10 + d1 * tx;
 *      gy = bot - top, m = top + gy * ty, gx = d0 + (d1 - d0) * ty:
 *      m is the bilinear sample and (gx, gy) the exact gradient of the interpolant at (sx, sy), so no neighbours beyond
 *      the four taps are read;
 *      I = ref(p), e = I - (gain * m + bias).
 *    Effective weight, the rule of microaligner_flowsmooth.h: w(p) = weight(p) widened to float64 if weight(p) is finite and
 *    > 0, else w(p) = 0.
 *    Every pixel falls in exactly one class, tested in this order:
 *      outside    : not inside;
 *      invalid    : I or one of the four taps is not finite;
 *      unweighted : w = 0;
 *      trimmed    : clipping is on and not |e| <= clip;
 *      used       : the rest.
 *    Over the used pixels, with wgx = w * gx, wgy = w * gy, we = w * e, wm = w * m, wI = w * I rounded once each, the
 *    31 sums, in this order:
 *      A = (wgx * gx, wgx * gy, wgy * gy),  G = (X * X, X * Y, X, Y * Y, Y, 1):
 *      sums[6 i + j] = A_i * G_j, i = 0 .. 2, j = 0 .. 5 (j = 5 is A_i itself): the 18 distinct products of J^T J for
 *                      J = (gx X, gx Y, gx, gy X, gy Y, gy), the derivative of m by the entries of M in the centred frame;
 *      sums[18..23]  : with ex = we * gx, ey = we * gy: ex * X, ex * Y, ex, ey * X, ey * Y, ey  (w J_k e);
 *      sums[24]      : we * e;
 *      sums[25..30]  : w, wm, wI, wm * m, wm * I, wI * I;
 *    and the five counts, in this order: used, outside, invalid, unweighted, trimmed; they add up to H * W.
 *    The terms are defined bit for bit; the order of summation is not, but it is fixed -- per thread in pixel order, the
 *    lanes of a wave by a shuffle tree, the waves of a tile in sequence, the tiles in a fixed order and tree by a second
 *    kernel, no floating-point atomics -- so two calls on the same input return the same bits. */
#ifndef MICROALIGNER_DIRECT_H
#define MICROALIGNER_DIRECT_H

#include "microaligner_flowsmooth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MA_DIRECT_AFFINE_SUMS 31
#define MA_DIRECT_AFFINE_COUNTS 5

/* The 31 sums and 5 counts defined above into the host arrays sums_host and counts_host.  ref, mov and weight are device
 * pointers, M a host pointer to 6 doubles that is read before the call returns.  The call synchronises the ctx stream.
 * MA_EINVAL for a NULL ctx, ref, mov, M, sums_host or counts_host, a NULL weight of a kind other than NONE, an unknown dtype
 * or weight kind (MA_SMOOTH_WEIGHT_CELLS included), H or W outside [1, 2^24], a non-finite entry of M, gain or bias, or an
 * image of more than 2^31 - 1 tiles of 256 x 64 pixels. */
int ma_direct_affine_moments(ma_ctx* ctx, const void* ref, int ref_dtype, const void* mov, int mov_dtype, int H, int W,
                             const double* M, double gain, double bias, const void* weight, int weight_kind, double clip,
                             double* sums_host, long long* counts_host);

/* out[i] = mask[i] != 0 ? 1.0f : 0.0f for i < n: a uint8 mask as the float32 map of the same weights, for the pyramid of
 * a weight (a mask has no pyramid of its own).  mask and out are device pointers; enqueued on the ctx stream, no
 * synchronisation.  MA_EINVAL for a NULL ctx, mask or out, or n outside [1, (2^31 - 1) * 1024]. */
int ma_direct_mask_weight(ma_ctx* ctx, const unsigned char* mask, size_t n, float* out);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_DIRECT_H */
