// det J of the map phi(p) = p + flow(p) at one pixel, the one statement of it: the flow statistics of the quality maps
// (qc.hip) and the fold mask (flow_smooth.hip) both call it.  Off the measured path (a header of single sources,
// build.SOURCE_HEADERS).
//
// det J = (1 + du/dx)(1 + dv/dy) - (du/dy)(dv/dx) in f64, every operation rounded on its own, the derivatives
// numpy.gradient's at edge_order 1: central differences / 2 inside, one-sided at the edges, 0 along an axis of length 1.
// det is finite exactly when every value its stencil reads is: finite f32 values give finite differences and products in
// f64, and a non-finite operand of +, -, * never yields a finite result.
#pragma once
#include <hip/hip_runtime.h>

// at(dx, dy): the float2 (u, v) of the pixel (x + dx, y + dy); called only for neighbours inside the (H, W) image, with
// (dx, dy) one of (0, 0), (+-1, 0), (0, +-1).
template <class At>
__device__ __forceinline__ double ma_flow_det_j(const At& at, int x, int y, int W, int H)
{
    double dudx = 0.0, dvdx = 0.0, dudy = 0.0, dvdy = 0.0;
    if (W > 1) {
        if (x == 0) {
            const float2 c = at(0, 0), p = at(1, 0);
            dudx = __dsub_rn((double)p.x, (double)c.x); dvdx = __dsub_rn((double)p.y, (double)c.y);
        } else if (x == W - 1) {
            const float2 c = at(0, 0), m = at(-1, 0);
            dudx = __dsub_rn((double)c.x, (double)m.x); dvdx = __dsub_rn((double)c.y, (double)m.y);
        } else {
            const float2 p = at(1, 0), m = at(-1, 0);
            dudx = __dsub_rn((double)p.x, (double)m.x) / 2.0;
            dvdx = __dsub_rn((double)p.y, (double)m.y) / 2.0;
        }
    }
    if (H > 1) {
        if (y == 0) {
            const float2 c = at(0, 0), p = at(0, 1);
            dudy = __dsub_rn((double)p.x, (double)c.x); dvdy = __dsub_rn((double)p.y, (double)c.y);
        } else if (y == H - 1) {
            const float2 c = at(0, 0), m = at(0, -1);
            dudy = __dsub_rn((double)c.x, (double)m.x); dvdy = __dsub_rn((double)c.y, (double)m.y);
        } else {
            const float2 p = at(0, 1), m = at(0, -1);
            dudy = __dsub_rn((double)p.x, (double)m.x) / 2.0;
            dvdy = __dsub_rn((double)p.y, (double)m.y) / 2.0;
        }
    }
    return __dsub_rn(__dmul_rn(__dadd_rn(1.0, dudx), __dadd_rn(1.0, dvdy)), __dmul_rn(dudy, dvdx));
}
