/* Texture support maps: the eigenvalues of the Gaussian-windowed structure tensor of an image (Shi-Tomasi; the G matrix of
 * Lucas-Kanade and Farneback), a per-pixel weight made from the smaller one, and per-cell counts of textured, edge and flat
 * pixels.  They say where a flow computed on the image is founded on image content: both components where the smaller
 * eigenvalue is large, one component (across an edge) where only the larger is, none where both are small.  An extension
 * of libmicroaligner_hip.so with no counterpart in the reference.  Off the measured path (build.source_hash() does not
 * cover it).  Whole image, no tile windows.
 *
 * All arithmetic is float32 and every operation is rounded on its own: nothing is fused, the division and the square root
 * are the correctly rounded ones, denormals are kept, and the arithmetic is IEEE's throughout.
 *
 * Input: img (H, W) uint8, uint16 or float32 (MA_U8, MA_U16, MA_F32), 1 <= H, W <= 2^24; I = float32(img).
 * Gradients, central differences with a replicated border:
 *   gx(x, y) = 0.5f * (I(min(x + 1, W - 1), y) - I(max(x - 1, 0), y)),
 *   gy(x, y) = 0.5f * (I(x, min(y + 1, H - 1)) - I(x, max(y - 1, 0)));
 *   along an axis of one pixel both reads are the pixel itself, which gives 0 for a finite pixel.
 * Products: P0 = gx * gx, P1 = gx * gy, P2 = gy * gy.
 * Smoothing: taps t[0 .. r] (host, float32), the centre and one side of a symmetric kernel, 1 <= r <= 128, every tap finite
 *   and >= 0, t[0] > 0.  A row pass, then a column pass over the row pass's output, both by the rule of
 *   microaligner_flowsmooth.h along their axis, samples outside the image being 0:
 *     A(x) = t[0] * P(x); then for k = 1 .. r ascending: A = A + t[k] * (P(x - k) + P(x + k)).
 *   The results are Sxx, Sxy, Syy (of P0, P1, P2).
 * Eigenvalues: h = 0.5f * (Sxx + Syy), d = 0.5f * (Sxx - Syy), q = sqrt(d * d + Sxy * Sxy);
 *   lam_max = h + q;  m = h - q, lam_min = (m < 0) ? 0 : m  (a NaN stays NaN).
 * Weight, with floor finite and > 0 (in squared grey levels): weight = (lam_min > 0) ? lam_min / (lam_min + floor) : 0, so
 *   that a NaN lam_min gives 0.  It is in [0, 1) and feeds ma_smooth_flow / ma_flow_affine_moments as it is.
 * Classes, with the same floor: textured: lam_min > floor; edge: lam_min <= floor and lam_max > floor; flat: the rest, which
 *   includes every pixel with a NaN lam_min.
 * Per-cell counts: on the cell grid of microaligner_qc.h (cells of cell_h x cell_w pixels from (0, 0), gy = ceil(H / cell_h)
 *   rows and gx = ceil(W / cell_w) columns of cells, the last row and column ragged; a cell larger than the image is the
 *   whole axis), counts[cy][cx][0 .. 3) = the textured, edge and flat pixels of the cell, which sum to its pixel count.
 *   Integer adds: the result does not depend on their order.
 * Non-finite float32 input is not special-cased: such a pixel makes the gradients of its four neighbours non-finite, and the
 *   smoothing carries them r px further, so that within r + 1 px (Chebyshev distance) of the pixel, the four corners of
 *   that box apart, lam_min is NaN and lam_max is NaN or +Inf; the weight there is 0 and the class flat.  The sign and
 *   payload of a computed NaN are not promised.
 * The zero border of the smoothing lowers both eigenvalues within r px of the image's edge. */
#ifndef MICROALIGNER_TEXTURE_H
#define MICROALIGNER_TEXTURE_H

#include "microaligner_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MA_TEXTURE_MAX_RADIUS 128
#define MA_TEXTURE_CLASSES 3

/* The maps of img as defined above: a row pass that forms the products from the image into a 12 B/px workspace from the ctx
 * cache (its three planes transposed), then a column pass that ends in the eigenvalues.  img, lam_min, lam_max and weight
 * ((H, W) float32 each) are device pointers, taps_host and counts_host (gy * gx * 3 entries) host pointers; taps_host is read
 * before the call returns.  Any of the four outputs may be NULL, not all of them; only the planes given are written.
 * floor is read only when weight or counts_host is given, cell_h and cell_w only when counts_host is.  Enqueued on the ctx
 * stream; with counts_host == NULL the call only enqueues, otherwise it synchronises the stream.
 * MA_EINVAL, before any device work, for a NULL ctx, img or taps_host, no output at all, H or W outside [1, 2^24], r outside
 * [1, 128], a tap that is not finite or is negative, t[0] == 0, an unknown dtype, a floor that is not finite and positive
 * when it is read, or a cell size < 1 when it is read. */
int ma_texture_maps(ma_ctx* ctx, const void* img, int dtype, int H, int W, const float* taps_host, int r, float floor,
                    float* lam_min, float* lam_max, float* weight, int cell_h, int cell_w, long long* counts_host);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_TEXTURE_H */
