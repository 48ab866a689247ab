// Thin-plate spline of a set of landmark pairs, evaluated on the nodes of a grid flow (stride 1: the dense flow) and at
// points (include/microaligner_landmarks.h).  The fit is the host's.
//
// Both kernels spread positions over lanes and walk the landmarks in one ascending loop that is the same for every lane
// of a wave: the 32-byte record (u.x, u.y, w.x, w.y) is addressed from kernel arguments and the loop counter alone, so it
// arrives by one scalar 32-byte load per landmark per wave, never by per-lane loads.  The work per pair is a double
// logarithm (about three quarters of the ~100 instructions) and a dozen float64 operations; nothing else touches memory
// until the float2 store of the result, one column per lane, so a wave stores 512 contiguous bytes per row.
// landmark_flow_kernel takes LM_ROWS rows of one column per thread: the record, d = X - u.x and d * d serve all of them, and
// their logarithms are independent chains.
#include "../../include/microaligner_landmarks.h"
#include "ma_internal.h"

#include <cmath>

namespace {

#ifndef LM_ROWS
#define LM_ROWS 4      // rows per thread of landmark_flow_kernel
#endif
constexpr int LM_SIDE_MAX = 1 << 24;
constexpr int LM_BLOCK = 256;     // columns per block

struct __attribute__((aligned(32))) Rec { double ux, uy, wx, wy; };
struct Mat6 { double v[6]; };

// U of the header, q > 0 ? (0.5 * q) * log(q) : 0, without a branch around the logarithm: at q == 0 (and for a NaN) it is
// (0.5 * 1) * log(1), and log(1) is +0 exactly.  A branch costs about 8 instructions per pair and keeps the rows of a
// thread from overlapping.
__device__ __forceinline__ double tps_u(double q)
{
    const double p = q > 0.0 ? q : 1.0;
    return (0.5 * p) * log(p);
}

template <int R>
__global__ __launch_bounds__(LM_BLOCK) void landmark_flow_kernel(const Rec* __restrict__ cw, int n, Mat6 A, double cx,
                                                                 double cy, double k, int H, int W, int stride, int gh,
                                                                 int gw, int nby, float2* __restrict__ out)
{
    const int i = blockIdx.x * LM_BLOCK + threadIdx.x;      // node column
    const bool col = i < gw;
    // node positions in 64 bits: i * stride may pass 2^31
    const long long px = min((long long)i * stride, (long long)(W - 1));
    const double x = (double)px, X = (x - cx) * k;
    // more row blocks than gridDim.y holds: a block strides over them
    for (int by = blockIdx.y; by < nby; by += gridDim.y) {
        const int j0 = by * R;
        double y[R], Y[R], sx[R], sy[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const long long py = min((long long)min(j0 + r, gh - 1) * stride, (long long)(H - 1));
            y[r] = (double)py;
            Y[r] = (y[r] - cy) * k;
            sx[r] = 0.0;
            sy[r] = 0.0;
        }
        for (int l = 0; l < n; l++) {       // wave-uniform: cw[l] is a scalar load
            const Rec c = cw[l];
            const double d = X - c.ux, dd = d * d;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const double e = Y[r] - c.uy;
                const double u = tps_u(dd + e * e);
                sx[r] = sx[r] + c.wx * u;
                sy[r] = sy[r] + c.wy * u;
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (!(col && j0 + r < gh)) continue;
            const double fx = ((A.v[0] * X + A.v[1] * Y[r]) + A.v[2]) + sx[r];
            const double fy = ((A.v[3] * X + A.v[4] * Y[r]) + A.v[5]) + sy[r];
            out[(size_t)(j0 + r) * gw + i] = make_float2((float)(x - fx), (float)(y[r] - fy));
        }
    }
}

// `pts` and `out` may be one array: neither is __restrict__, and a thread reads only the point it writes.
__global__ __launch_bounds__(LM_BLOCK) void landmark_points_kernel(const Rec* __restrict__ cw, int n, Mat6 A, double cx,
                                                                   double cy, double k, const double2* pts, int m,
                                                                   double2* out)
{
    const long long i = (long long)blockIdx.x * LM_BLOCK + threadIdx.x;
    const bool live = i < m;
    // no early return: the landmark loop stays the same for every lane of the wave
    const double2 p = live ? pts[i] : make_double2(0.0, 0.0);
    const double X = (p.x - cx) * k, Y = (p.y - cy) * k;
    double sx = 0.0, sy = 0.0;
    for (int l = 0; l < n; l++) {
        const Rec c = cw[l];
        const double d = X - c.ux, e = Y - c.uy;
        const double u = tps_u(d * d + e * e);
        sx = sx + c.wx * u;
        sy = sy + c.wy * u;
    }
    if (!live) return;
    if (!(__builtin_isfinite(p.x) && __builtin_isfinite(p.y))) {
        out[i] = make_double2((double)NAN, (double)NAN);
        return;
    }
    out[i] = make_double2(((A.v[0] * X + A.v[1] * Y) + A.v[2]) + sx, ((A.v[3] * X + A.v[4] * Y) + A.v[5]) + sy);
}

bool finite_spline(const double* a6, double cx, double cy, double k)
{
    for (int i = 0; i < 6; i++)
        if (!std::isfinite(a6[i])) return false;
    return std::isfinite(cx) && std::isfinite(cy) && std::isfinite(k);
}

int grid_nodes(int n, int s) { return n == 1 ? 1 : (int)(((long long)n - 2) / s) + 2; }   // ceil((n - 1) / s) + 1

} // namespace

extern "C" int ma_landmark_flow(ma_ctx* ctx, const double* cw, int n, const double* a6, double cx, double cy, double k, int H,
                                int W, int stride, float* out)
{
    MA_REQUIRE(ctx && cw && a6 && out, "NULL argument");
    MA_REQUIRE(n >= 0 && n <= MA_LANDMARK_MAX, "the number of landmarks must be in [0, 2^20]");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= LM_SIDE_MAX && W <= LM_SIDE_MAX, "flow sides must be in [1, 2^24]");
    MA_REQUIRE(stride >= 1, "the stride must be at least 1");
    MA_REQUIRE(finite_spline(a6, cx, cy, k), "the affine part, the centre and the scale must be finite");
    MA_REQUIRE_ALIGNED(cw, 32, "cw");
    MA_REQUIRE_ALIGNED(out, 8, "out");
    Mat6 A;
    for (int i = 0; i < 6; i++) A.v[i] = a6[i];
    const int gh = grid_nodes(H, stride), gw = grid_nodes(W, stride);
    const int nby = (gh + LM_ROWS - 1) / LM_ROWS;
    MA_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(landmark_flow_kernel<LM_ROWS>, dim3((gw + LM_BLOCK - 1) / LM_BLOCK, nby < MA_GRID_Y_MAX ? nby : MA_GRID_Y_MAX),
                       dim3(LM_BLOCK), 0, ctx->stream, (const Rec*)cw, n, A, cx, cy, k, H, W, stride, gh, gw, nby,
                       (float2*)out);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

extern "C" int ma_landmark_points(ma_ctx* ctx, const double* cw, int n, const double* a6, double cx, double cy, double k,
                                  const double* pts, int m, double* out)
{
    MA_REQUIRE(ctx && cw && a6 && pts && out, "NULL argument");
    MA_REQUIRE(n >= 0 && n <= MA_LANDMARK_MAX, "the number of landmarks must be in [0, 2^20]");
    MA_REQUIRE(m >= 0, "the number of points must not be negative");
    MA_REQUIRE(finite_spline(a6, cx, cy, k), "the affine part, the centre and the scale must be finite");
    MA_REQUIRE_ALIGNED(cw, 32, "cw");
    MA_REQUIRE_ALIGNED(pts, 16, "pts");
    MA_REQUIRE_ALIGNED(out, 16, "out");
    if (m == 0) return MA_OK;
    Mat6 A;
    for (int i = 0; i < 6; i++) A.v[i] = a6[i];
    MA_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(landmark_points_kernel, dim3((unsigned)(((long long)m + LM_BLOCK - 1) / LM_BLOCK)), dim3(LM_BLOCK), 0,
                       ctx->stream, (const Rec*)cw, n, A, cx, cy, k, (const double2*)pts, m, (double2*)out);
    MA_HIP(hipGetLastError());
    return MA_OK;
}
