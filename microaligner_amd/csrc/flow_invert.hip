// Dense inverse of a flow and point transforms between the registered and the moving frame
// (include/microaligner_flowinvert.h).
//
// invert_flow_kernel: the fixed point g(q) = -f(q - g(q)) of one pixel, iterated in registers in one launch.  Shaped like
// compose_flows_kernel (flow_compose.hip): one column per lane, FI_ROWS rows per thread; the sampler is the unquantised
// bilinear one of the header, not remap_common.h's.  Per pixel one 8-byte write (plus 4 for the residual) and four
// gathered float2 taps per step; the taps of a step lie within |g| px of the pixel, so neighbouring lanes share their
// cache lines.  Lanes finish at different steps: a wave runs until its last lane stops.  The pixels that did not converge
// are counted as call_counts.h states.
#include "../../include/microaligner_flowinvert.h"
#include "../../include/microaligner_flowgrid.h"
#include "call_counts.h"
#include "flow_grid_eval.h"
#include "ma_internal.h"

#include <cmath>

namespace {

// Measured on 16384^2 with a smooth flow of up to 25 px (6.5 steps per pixel in the mean, 9 at most), alternating builds
// on one box: the kernel is bound by the gather instructions it issues, not by registers or bytes.  With four float2 loads
// per step, 1, 2 and 4 rows per thread (29 / 36 / 46 VGPRs, 8 waves per SIMD each) all take 4.1 ms.  FI_PAIR fetches the two
// taps of a row with one 16-byte load: 3.37 ms with 1 row (FI_ROWS, 38 VGPRs), 3.15 ms with 2 (46), 3.19 ms with 4 (56).
#ifndef FI_ROWS
#define FI_ROWS 2      // rows per thread; they step together so that their gathers are in flight together
#endif
#ifndef FI_PAIR
#define FI_PAIR 1
#endif
constexpr int FI_SIDE_MAX = 1 << 24;   // pixel coordinates exact in float32

struct __attribute__((aligned(8))) Pair { float2 lo, hi; };   // two neighbouring pixels of a row

__device__ __forceinline__ float2 sample_f32(const float2* __restrict__ f, int H, int W, float wmax, float hmax, float mx,
                                             float my)
{
    // fmaxf / fminf return the other operand for a NaN: a NaN coordinate clamps to 0
    const float cx = fminf(fmaxf(mx, 0.f), wmax), cy = fminf(fmaxf(my, 0.f), hmax);
    const float x0 = floorf(cx), y0 = floorf(cy);
    const float ax = cx - x0, ay = cy - y0, bx = 1.f - ax, by = 1.f - ay;
    const int ix = (int)x0, iy = (int)y0;
    const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
    const float2* r0 = f + (size_t)iy * W;
    const float2* r1 = f + (size_t)iy1 * W;
#if FI_PAIR
    float2 v00, v01, v10, v11;
    if (W >= 2) {       // wave-uniform
        // the two taps of a row in one 16-byte load (8-byte aligned): columns xb, xb + 1 with xb = min(ix, W - 2)
        const int xb = min(ix, W - 2);
        const Pair a = *(const Pair*)(r0 + xb), b = *(const Pair*)(r1 + xb);
        const bool last = ix != xb;    // ix == W - 1: both taps are the last column
        v00 = last ? a.hi : a.lo, v01 = a.hi, v10 = last ? b.hi : b.lo, v11 = b.hi;
    } else {
        v00 = r0[ix], v01 = r0[ix1], v10 = r1[ix], v11 = r1[ix1];
    }
#else
    const float2 v00 = r0[ix], v01 = r0[ix1], v10 = r1[ix], v11 = r1[ix1];
#endif
    const float topx = v00.x * bx + v01.x * ax, botx = v10.x * bx + v11.x * ax;
    const float topy = v00.y * bx + v01.y * ax, boty = v10.y * bx + v11.y * ax;
    return make_float2(topx * by + botx * ay, topy * by + boty * ay);
}

template <int R>
__global__ __launch_bounds__(256) void invert_flow_kernel(const float2* __restrict__ f, int H, int W, int nby, int max_iter,
                                                          float tol, float2* __restrict__ out, float* __restrict__ residual,
                                                          unsigned long long* __restrict__ not_converged)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const bool col = x < W;                 // no early return: every lane takes part in the wave's count below
    const float xf = (float)x, wmax = (float)(W - 1), hmax = (float)(H - 1);
    unsigned int missed = 0;
    // more row blocks than gridDim.y holds (H > MA_GRID_Y_MAX * R): a block strides over them
    for (int by = blockIdx.y; by < nby; by += gridDim.y) {
        const int y0 = by * R;
        float2 g[R];
        float res[R];
        bool live[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            g[r] = make_float2(0.f, 0.f);
            res[r] = 0.f;
            live[r] = col && y0 + r < H;
        }
        for (int k = 0; k < max_iter; k++) {
            bool any = false;
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (!live[r]) continue;
                const float2 s = sample_f32(f, H, W, wmax, hmax, xf - g[r].x, (float)(y0 + r) - g[r].y);
                const float nx = -s.x, ny = -s.y;
                const float dx = fabsf(nx - g[r].x), dy = fabsf(ny - g[r].y);
                g[r] = make_float2(nx, ny);
                res[r] = (dx != dx || dy != dy) ? NAN : fmaxf(dx, dy);
                if (dx <= tol && dy <= tol) live[r] = false;      // false for a NaN: it never stops the loop
                else any = true;
            }
            if (!any) break;
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (!(col && y0 + r < H)) continue;
            const size_t i = (size_t)(y0 + r) * W + x;
            out[i] = g[r];
            if (residual) residual[i] = res[r];
            missed += live[r] ? 1u : 0u;
        }
    }
    if (not_converged) d_wave_tally(not_converged, {missed});        // wave-uniform
}

struct Mat6 { double v[6]; };

__device__ __forceinline__ double2 sample_f64(const float2* __restrict__ f, int H, int W, double mx, double my)
{
    const double cx = fmin(fmax(mx, 0.0), (double)(W - 1)), cy = fmin(fmax(my, 0.0), (double)(H - 1));
    const double x0 = floor(cx), y0 = floor(cy);
    const double ax = cx - x0, ay = cy - y0, bx = 1.0 - ax, by = 1.0 - ay;
    const int ix = (int)x0, iy = (int)y0;
    const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
    const float2* r0 = f + (size_t)iy * W;
    const float2* r1 = f + (size_t)iy1 * W;
    const float2 v00 = r0[ix], v01 = r0[ix1], v10 = r1[ix], v11 = r1[ix1];
    const double topx = (double)v00.x * bx + (double)v01.x * ax, botx = (double)v10.x * bx + (double)v11.x * ax;
    const double topy = (double)v00.y * bx + (double)v01.y * ax, boty = (double)v10.y * bx + (double)v11.y * ax;
    return make_double2(topx * by + botx * ay, topy * by + boty * ay);
}

// the float64 sampler of the dense flow, S64 of the header; the one of a grid flow is flow_grid_eval.h's FgSampler64
struct DenseSampler64 {
    const float2* __restrict__ f;
    int H, W;
    __device__ __forceinline__ double2 operator()(double mx, double my) const { return sample_f64(f, H, W, mx, my); }
};

// `pts` and `out` may be one array: neither is __restrict__, and a thread reads only the point it writes.  S: the sampler
// of the (H, W) flow.
template <class S>
__global__ __launch_bounds__(256) void transform_points_kernel(const double2* pts, int n, S sample, int H,
                                                               int W, Mat6 A, double padx, double pady, int direction,
                                                               int max_iter, double tol, double2* out,
                                                               unsigned char* __restrict__ converged,
                                                               unsigned char* __restrict__ inside)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double2 p = pts[i];
    if (!(__builtin_isfinite(p.x) && __builtin_isfinite(p.y))) {
        out[i] = make_double2((double)NAN, (double)NAN);
        converged[i] = 0;
        inside[i] = 0;
        return;
    }
    const double wmax = (double)(W - 1), hmax = (double)(H - 1);
    if (direction == MA_POINTS_TO_MOVING) {
        const double2 s = sample(p.x, p.y);
        const double ux = p.x - s.x, uy = p.y - s.y;
        out[i] = make_double2(((A.v[0] * ux + A.v[1] * uy) + A.v[2]) - padx, ((A.v[3] * ux + A.v[4] * uy) + A.v[5]) - pady);
        converged[i] = 1;
        inside[i] = (p.x >= 0.0 && p.x <= wmax && p.y >= 0.0 && p.y <= hmax) ? 1 : 0;
        return;
    }
    const double sx = p.x + padx, sy = p.y + pady;
    const double ax = (A.v[0] * sx + A.v[1] * sy) + A.v[2], ay = (A.v[3] * sx + A.v[4] * sy) + A.v[5];
    double qx = ax, qy = ay;
    unsigned char ok = 0;
    for (int k = 0; k < max_iter; k++) {
        const double2 s = sample(qx, qy);
        const double nx = ax + s.x, ny = ay + s.y;
        const double dx = fabs(nx - qx), dy = fabs(ny - qy);
        qx = nx;
        qy = ny;
        if (dx <= tol && dy <= tol) {
            ok = 1;
            break;
        }
    }
    out[i] = make_double2(qx, qy);
    converged[i] = ok;
    inside[i] = (qx >= 0.0 && qx <= wmax && qy >= 0.0 && qy <= hmax) ? 1 : 0;
}

bool finite6(const double* m)
{
    for (int i = 0; i < 6; i++)
        if (!std::isfinite(m[i])) return false;
    return true;
}

} // namespace

extern "C" int ma_invert_flow(ma_ctx* ctx, const float* flow, int H, int W, int max_iter, float tol, float* out,
                              float* residual, long long* not_converged_host)
{
    MA_REQUIRE(ctx && flow && out, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE_ALIGNED(out, 8, "out");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FI_SIDE_MAX && W <= FI_SIDE_MAX, "flow sides must be in [1, 2^24]");
    MA_REQUIRE(max_iter >= 1, "max_iter must be at least 1");
    MA_REQUIRE(std::isfinite(tol) && tol >= 0.f, "tol must be finite and not negative");
    MA_REQUIRE(out != flow && residual != flow && (const float*)residual != out, "out, residual and flow must be distinct arrays");
    MA_HIP(hipSetDevice(ctx->device));
    unsigned long long* counter;
    MA_TRY(ma_call_counts(ctx, not_converged_host != nullptr, 1, &counter));
    const int nby = (H + FI_ROWS - 1) / FI_ROWS;
    hipLaunchKernelGGL(invert_flow_kernel<FI_ROWS>, dim3((W + 255) / 256, nby < MA_GRID_Y_MAX ? nby : MA_GRID_Y_MAX), dim3(256),
                       0, ctx->stream, (const float2*)flow, H, W, nby, max_iter, tol, (float2*)out, residual, counter);
    MA_HIP(hipGetLastError());
    if (not_converged_host) MA_TRY(ma_read_call_counts(ctx, counter, 1, not_converged_host));
    return MA_OK;
}

// the checks and the launch that the two point entries share
template <class S>
static int transform_points(ma_ctx* ctx, const double* pts, int n, const S& sample, int H, int W, const double* m6,
                            const double* t6, int pad_left, int pad_top, int direction, int max_iter, double tol,
                            double* out, unsigned char* converged, unsigned char* inside)
{
    MA_REQUIRE(ctx && pts && out && converged && inside, "NULL argument");
    MA_REQUIRE_ALIGNED(pts, 16, "pts");
    MA_REQUIRE_ALIGNED(out, 16, "out");
    MA_REQUIRE(n >= 0, "the number of points must not be negative");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FI_SIDE_MAX && W <= FI_SIDE_MAX, "flow sides must be in [1, 2^24]");
    MA_REQUIRE(direction == MA_POINTS_TO_MOVING || direction == MA_POINTS_TO_REFERENCE, "unknown direction");
    MA_REQUIRE(max_iter >= 1, "max_iter must be at least 1");
    MA_REQUIRE(std::isfinite(tol) && tol >= 0.0, "tol must be finite and not negative");
    MA_REQUIRE(pad_left >= 0 && pad_top >= 0, "the padding must not be negative");
    MA_REQUIRE((!m6 || finite6(m6)) && (!t6 || finite6(t6)), "the matrices must be finite");
    if (n == 0) return MA_OK;
    const double* a = direction == MA_POINTS_TO_MOVING ? m6 : t6;
    Mat6 A = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0}};
    if (a)
        for (int i = 0; i < 6; i++) A.v[i] = a[i];
    MA_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(transform_points_kernel<S>, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const double2*)pts, n, sample, H, W, A, (double)pad_left, (double)pad_top, direction,
                       max_iter, tol, (double2*)out, converged, inside);
    MA_HIP(hipGetLastError());
    return MA_OK;
}

extern "C" int ma_transform_points(ma_ctx* ctx, const double* pts, int n, const float* flow, int H, int W, const double* m6,
                                   const double* t6, int pad_left, int pad_top, int direction, int max_iter, double tol,
                                   double* out, unsigned char* converged, unsigned char* inside)
{
    MA_REQUIRE(flow, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    return transform_points(ctx, pts, n, DenseSampler64{(const float2*)flow, H, W}, H, W, m6, t6, pad_left, pad_top, direction,
                            max_iter, tol, out, converged, inside);
}

extern "C" int ma_transform_points_grid(ma_ctx* ctx, const double* pts, int n, const float* nodes, int H, int W, int s,
                                        const double* m6, const double* t6, int pad_left, int pad_top, int direction,
                                        int max_iter, double tol, double* out, unsigned char* converged,
                                        unsigned char* inside)
{
    MA_REQUIRE(nodes, "NULL argument");
    MA_REQUIRE_ALIGNED(nodes, 8, "nodes");
    MA_REQUIRE(s >= 1, "the stride must be at least 1");
    MA_REQUIRE(H >= 1 && W >= 1, "flow sides must be in [1, 2^24]");
    return transform_points(ctx, pts, n, FgSampler64{fg_grid(nodes, H, W, s)}, H, W, m6, t6, pad_left, pad_top, direction,
                            max_iter, tol, out, converged, inside);
}
