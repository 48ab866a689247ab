/* Registration quality maps: per-cell similarity of two label images against a reference and per-cell statistics of a
 * dense flow (Jacobian determinant, folding, magnitude).  An extension of libmicroaligner_hip.so with no counterpart in
 * the reference; off the measured path (build.source_hash() does not cover it).
 *
 * Cells: a grid from (0, 0) of cell_h x cell_w pixels over an (h, w) image, gy = ceil(h / cell_h) rows and
 * gx = ceil(w / cell_w) columns of cells; the last row / column of cells is ragged.  Every output array has gy * gx
 * entries in row-major cell order.  Work is done in batches of cells so that the device workspace stays within
 * ma_ctx_set_workspace_limit; results do not depend on the batching.  Both calls synchronise the ctx stream. */
#ifndef MICROALIGNER_QC_H
#define MICROALIGNER_QC_H

#include "microaligner_hip.h"
/* Device pointers follow the alignment rule of microaligner_hip.h ("Device pointers"): an array is aligned to its element,
 * a flow, a map or the nodes of a grid flow to 8 bytes, float64 points to 16 bytes, unless an entry below names a stricter
 * figure for one argument; below the rule an entry returns MA_EINVAL before it launches anything. */

#ifdef __cplusplus
extern "C" {
#endif

/* Per cell: sklearn normalized_mutual_info_score (arithmetic mean) of the u8 labels ref and b0, and of ref and b1 (b1 may
 * be NULL: nmi1 / ncc1 are then not written), computed by the gate's own code (same doubles as ma_nmi_u8 on the
 * cropped cell), and the Pearson correlation of the same labels from the exact integer moments of the joint histogram
 * (NaN where either label set is constant).  Every cell must hold fewer than 2^32 pixels. */
int ma_qc_nmi_grid(ma_ctx* ctx, const uint8_t* ref, const uint8_t* b0, const uint8_t* b1, int h, int w, int cell_h, int cell_w,
                   double* nmi0_host, double* nmi1_host, double* ncc0_host, double* ncc1_host);

/* Per cell of an (h, w, 2) float32 flow (u = [..., 0], v = [..., 1]) with the map phi(p) = p + flow(p):
 *   jac_min : min of det J = (1 + du/dx)(1 + dv/dy) - (du/dy)(dv/dx) in f64 without fused multiply-adds, the derivatives
 *             numpy.gradient's (central differences inside, one-sided at the edges, 0 along an axis of length 1), over the
 *             pixels whose stencil reads only finite values (+inf if none);
 *   folded  : number of those pixels with det J <= 0;
 *   invalid : number of pixels with a non-finite u or v;
 *   flow_mean, flow_max : mean and max of sqrt(u^2 + v^2) in f64 over the pixels with finite u and v (NaN if none). */
int ma_qc_flow_grid(ma_ctx* ctx, const float* flow, int h, int w, int cell_h, int cell_w, double* jac_min_host,
                    long long* folded_host, long long* invalid_host, double* flow_mean_host, double* flow_max_host);

#ifdef __cplusplus
}
#endif

#endif /* MICROALIGNER_QC_H */
