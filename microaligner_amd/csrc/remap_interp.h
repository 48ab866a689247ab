// Tap and weight code of cv2.remap's INTER_NEAREST / INTER_CUBIC / INTER_LANCZOS4 shared by the kernels of
// remap_interp.hip and warp_compose.hip: the 1-D weight tables in constant memory (one copy per source file that includes
// this header, filled by its own ensure_tables()), their LDS staging, and the sample of N x N taps in OpenCV's summation
// order; the 5-bit quantisation is remap_common.h's.  The semantics are those of include/microaligner_interp.h.
#ifndef MA_REMAP_INTERP_H
#define MA_REMAP_INTERP_H

#include "remap_common.h"
#include "../../include/microaligner_interp.h"

#include <climits>
#include <cmath>
#include <mutex>
#include <vector>

namespace {

constexpr int TAB = 32;   // INTER_TAB_SIZE

__constant__ float c_tab_cubic[TAB * 4];
__constant__ float c_tab_lanczos[TAB * 8];
// per fraction pair fy * 32 + fx: tap index | (delta << 8) of initInterTab2D's fix-up of the u8 table (delta 0: none)
__constant__ int c_fix_cubic[TAB * TAB];
__constant__ int c_fix_lanczos[TAB * TAB];

template <int MODE> struct Mode;
template <> struct Mode<MA_INTER_NEAREST> { static constexpr int N = 1, OFF = 0, R = 8; };
template <> struct Mode<MA_INTER_CUBIC> { static constexpr int N = 4, OFF = 1, R = 4; };
template <> struct Mode<MA_INTER_LANCZOS4> { static constexpr int N = 8, OFF = 3, R = 2; };

template <int N> __device__ __forceinline__ const float* d_tab1() { return N == 4 ? c_tab_cubic : c_tab_lanczos; }
template <int N> __device__ __forceinline__ const int* d_fix() { return N == 4 ? c_fix_cubic : c_fix_lanczos; }

// (unsigned)v < max(n, 0): OpenCV's width1 tests
__device__ __forceinline__ bool d_below(int v, int n) { return n > 0 && (unsigned)v < (unsigned)n; }

// stage the 1-D table of the mode in LDS (every thread of the block takes part: before any early return)
template <int N>
__device__ __forceinline__ void load_tab(float* s_tab)
{
    if (N > 1) {
        for (int i = threadIdx.x; i < TAB * N; i += blockDim.x) s_tab[i] = d_tab1<N>()[i];
        __syncthreads();
    }
}

// One sample from its N x N taps v (0 where a tap is not read).  fast: every tap lies inside the source (OpenCV's
// straight path); otherwise rmask / cmask hold the rows / columns of taps inside the source, and only those are summed.
template <typename T, int N>
__device__ __forceinline__ T combine(const T (&v)[N][N], const float* s_tab, int fx, int fy, bool fast, unsigned rmask,
                                     unsigned cmask)
{
    float wx[N], wy[N];
#pragma unroll
    for (int k = 0; k < N; k++) { wx[k] = s_tab[fx * N + k]; wy[k] = s_tab[fy * N + k]; }
    if constexpr (sizeof(T) == 1) {
        // integer sum: the order does not matter, and taps outside the source hold 0
        const int fix = d_fix<N>()[fy * TAB + fx], ftap = fix & 255, fdel = fix >> 8;
        int acc = 0;
#pragma unroll
        for (int k1 = 0; k1 < N; k1++)
#pragma unroll
            for (int k2 = 0; k2 < N; k2++) {
                const float p = wy[k1] * wx[k2];
                const int w = d_sat_short(d_cvround(p * 32768.f)) + (k1 * N + k2 == ftap ? fdel : 0);
                acc += (int)v[k1][k2] * w;
            }
        return (T)d_clamp((acc + (1 << 14)) >> 15, 0, 255);
    } else {
        float sum = 0.f;
        if (fast) {
#pragma unroll
            for (int k1 = 0; k1 < N; k1++) {
                float r = (float)v[k1][0] * (wy[k1] * wx[0]);
#pragma unroll
                for (int k2 = 1; k2 < N; k2++) r = r + (float)v[k1][k2] * (wy[k1] * wx[k2]);
                // remapBicubic starts from the first row sum, remapLanczos4 from 0
                sum = (N == 4 && k1 == 0) ? r : sum + r;
            }
        } else {
#pragma unroll
            for (int k1 = 0; k1 < N; k1++)
#pragma unroll
                for (int k2 = 0; k2 < N; k2++)
                    if ((rmask >> k1) & (cmask >> k2) & 1u) sum = sum + (float)v[k1][k2] * (wy[k1] * wx[k2]);
        }
        if constexpr (sizeof(T) == 2) return (T)d_clamp(d_cvround(sum), 0, 65535);
        else return sum;
    }
}

// ---- host tables ----------------------------------------------------------------------------------------------------
int h_cvround(float v)
{
    if (!(fabsf(v) < 2147483648.0f)) return INT_MIN;
    return (int)lrintf(v);
}
short h_sat_short(int v) { return (short)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// imgwarp.cpp interpolateCubic / interpolateLanczos4
void interpolate_cubic(float x, float* coeffs)
{
    const float A = -0.75f;
    coeffs[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    coeffs[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    coeffs[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    coeffs[3] = 1.f - coeffs[0] - coeffs[1] - coeffs[2];
}
void interpolate_lanczos4(float x, float* coeffs)
{
    static const double s45 = 0.70710678118654752440084436210485;
    static const double cs[][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
    const double PI = 3.1415926535897932384626433832795;
    float sum = 0;
    double y0 = -(x + 3) * PI * 0.25, s0 = std::sin(y0), c0 = std::cos(y0);
    for (int i = 0; i < 8; i++) {
        float y0_ = (x + 3 - i);
        if (fabs(y0_) >= 1e-6f) {
            double y = -y0_ * PI * 0.25;
            coeffs[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
        } else {
            coeffs[i] = 1e30f;
        }
        sum += coeffs[i];
    }
    sum = 1.f / sum;
    for (int i = 0; i < 8; i++) coeffs[i] *= sum;
}

// initInterTab2D's u8 table for an N-tap 1-D table, reduced to the one entry its sum fix-up changes per fraction pair
template <int N>
void fix_table(const float* tab1, int* fix)
{
    for (int i = 0; i < TAB; i++)
        for (int j = 0; j < TAB; j++) {
            short itab[N * N], raw[N * N];
            int isum = 0;
            for (int k1 = 0; k1 < N; k1++) {
                const float vy = tab1[i * N + k1];
                for (int k2 = 0; k2 < N; k2++) {
                    const float v = vy * tab1[j * N + k2];
                    isum += itab[k1 * N + k2] = raw[k1 * N + k2] = h_sat_short(h_cvround(v * 32768));
                }
            }
            if (isum != 32768) {
                const int diff = isum - 32768, k = N / 2;
                int Mk1 = k, Mk2 = k, mk1 = k, mk2 = k;
                for (int k1 = k; k1 < k + 2; k1++)
                    for (int k2 = k; k2 < k + 2; k2++) {
                        if (itab[k1 * N + k2] < itab[mk1 * N + mk2]) mk1 = k1, mk2 = k2;
                        else if (itab[k1 * N + k2] > itab[Mk1 * N + Mk2]) Mk1 = k1, Mk2 = k2;
                    }
                if (diff < 0) itab[Mk1 * N + Mk2] = (short)(itab[Mk1 * N + Mk2] - diff);
                else itab[mk1 * N + mk2] = (short)(itab[mk1 * N + mk2] - diff);
            }
            int f = 0;
            for (int t = 0; t < N * N; t++)
                if (itab[t] != raw[t]) f = t | ((itab[t] - raw[t]) * 256);
            fix[i * TAB + j] = f;
        }
}

struct HostTables {
    float cubic[TAB * 4], lanczos[TAB * 8];
    int fix_cubic[TAB * TAB], fix_lanczos[TAB * TAB];
    HostTables()
    {
        const float scale = 1.f / TAB;
        for (int i = 0; i < TAB; i++) {
            interpolate_cubic(i * scale, cubic + i * 4);
            interpolate_lanczos4(i * scale, lanczos + i * 8);
        }
        fix_table<4>(cubic, fix_cubic);
        fix_table<8>(lanczos, fix_lanczos);
    }
};

// the tables reach a device's constant memory once, on the stream of the first ctx that needs them there
int ensure_tables(ma_ctx* ctx)
{
    static const HostTables tabs;
    static std::mutex mu;
    static std::vector<char> ready;
    std::lock_guard<std::mutex> lk(mu);
    if ((int)ready.size() <= ctx->device) ready.resize(ctx->device + 1, 0);
    if (ready[ctx->device]) return MA_OK;
    MA_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_tab_cubic), tabs.cubic, sizeof(tabs.cubic), 0, hipMemcpyHostToDevice, ctx->stream));
    MA_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_tab_lanczos), tabs.lanczos, sizeof(tabs.lanczos), 0, hipMemcpyHostToDevice, ctx->stream));
    MA_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_fix_cubic), tabs.fix_cubic, sizeof(tabs.fix_cubic), 0, hipMemcpyHostToDevice, ctx->stream));
    MA_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_fix_lanczos), tabs.fix_lanczos, sizeof(tabs.fix_lanczos), 0, hipMemcpyHostToDevice, ctx->stream));
    MA_HIP(hipStreamSynchronize(ctx->stream));
    ready[ctx->device] = 1;
    return MA_OK;
}

bool interp_known(int interp)
{
    return interp == MA_INTER_NEAREST || interp == MA_INTER_LINEAR || interp == MA_INTER_CUBIC || interp == MA_INTER_LANCZOS4;
}

} // namespace

#endif // MA_REMAP_INTERP_H
