// Exact composition of two flows (include/microaligner_flowcompose.h): out(p) = second(p) + first sampled at
// (p - second(p)), the sample cv2.remap's linear one with a replicate border and no 16-bit saturation.  Shaped like
// merge_flows_kernel (remap.hip), the kernel it stands in for when OptFlowRegistrator.flow_composition is "exact": one
// column per lane, FC_ROWS rows per thread with the loads of `second` issued up front, float2 loads and stores.  24 B per
// pixel: 8 read of second, 8 gathered from first (the four taps of neighbouring lanes share cache lines), 8 written.
#include "../../include/microaligner_flowcompose.h"
#include "remap_common.h"

namespace {

// rows per thread: 4 (64 VGPRs, 8 waves per SIMD) measured 1.28 ms on 16384^2 against 1.35 ms with merge_flows_kernel's 8
// (122 VGPRs, 4 waves) and 1.60 ms with 16: the gathers want waves in flight more than loads in flight per wave
constexpr int FC_ROWS = 4;
constexpr int FC_SIDE_MAX = 1 << 24;   // pixel coordinates exact in float32

// `second` and `out` may be one array: neither is __restrict__, and a thread reads second only where it writes out
__global__ __launch_bounds__(256) void compose_flows_kernel(const float2* __restrict__ first, const float2* second, int H,
                                                            int W, int nby, float2* out)
{
    constexpr int R = FC_ROWS;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const float xf = (float)x, wmax = (float)(W - 1), hmax = (float)(H - 1);
    // more row blocks than gridDim.y holds (H > MA_GRID_Y_MAX * R): a block strides over them
    for (int by = blockIdx.y; by < nby; by += gridDim.y) {
        const int y0 = by * R;
        float2 t[R], res[R];
#pragma unroll
        for (int r = 0; r < R; r++) t[r] = second[(size_t)min(y0 + r, H - 1) * W + x];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int y = min(y0 + r, H - 1);
            const float mx = xf - t[r].x, my = (float)y - t[r].y;
            // fmaxf / fminf return the other operand for a NaN: a NaN coordinate clamps to 0
            const float cx = fminf(fmaxf(mx, 0.f), wmax), cy = fminf(fmaxf(my, 0.f), hmax);
            // remap_common.h's quantise() without d_sat_short: cx * 32 < 2^29
            const int qx = d_cvround(cx * 32.f), qy = d_cvround(cy * 32.f);
            const int ix = qx >> 5, iy = qy >> 5, fx = qx & 31, fy = qy & 31;
            const int ix1 = min(ix + 1, W - 1), iy1 = min(iy + 1, H - 1);
            const float2* r0 = first + (size_t)iy * W;
            const float2* r1 = first + (size_t)iy1 * W;
            const float2 v0 = r0[ix], v1 = r0[ix1], v2 = r1[ix], v3 = r1[ix1];
            const float sx = Interp<float>::run(v0.x, v1.x, v2.x, v3.x, fx, fy);
            const float sy = Interp<float>::run(v0.y, v1.y, v2.y, v3.y, fx, fy);
            res[r] = make_float2(t[r].x + sx, t[r].y + sy);
        }
#pragma unroll
        for (int r = 0; r < R; r++)
            if (y0 + r < H) out[(size_t)(y0 + r) * W + x] = res[r];
    }
}

} // namespace

extern "C" int ma_compose_flows(ma_ctx* ctx, const float* first, const float* second, int H, int W, float* out)
{
    MA_REQUIRE(ctx && first && second && out, "NULL argument");
    MA_REQUIRE_ALIGNED(first, 8, "first");
    MA_REQUIRE_ALIGNED(second, 8, "second");
    MA_REQUIRE_ALIGNED(out, 8, "out");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FC_SIDE_MAX && W <= FC_SIDE_MAX, "flow sides must be in [1, 2^24]");
    MA_REQUIRE(out != first, "out must not be first (it may be second)");
    MA_HIP(hipSetDevice(ctx->device));
    const int nby = (H + FC_ROWS - 1) / FC_ROWS;
    hipLaunchKernelGGL(compose_flows_kernel, dim3((W + 255) / 256, nby < MA_GRID_Y_MAX ? nby : MA_GRID_Y_MAX), dim3(256), 0,
                       ctx->stream, (const float2*)first, (const float2*)second, H, W, nby, (float2*)out);
    MA_HIP(hipGetLastError());
    return MA_OK;
}
