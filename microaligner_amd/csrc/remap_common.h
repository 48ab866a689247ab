// Device code of cv2.remap's arithmetic that every warp kernel shares: the 1/32 px quantisation of
// a map coordinate, the bilinear sample, and the window origins of the tiled warps.  Included by remap.hip (the linear
// kernels of the measured path), remap_interp.h (nearest / cubic / Lanczos-4) and warp_compose.hip; no tables, no host code.
#ifndef MA_REMAP_COMMON_H
#define MA_REMAP_COMMON_H

#include "ma_internal.h"

namespace {

struct Tap {
    int sx, sy;   // integer source coordinate of the top-left tap (before a mode's tap offset)
    int fx, fy;   // 5-bit fractions
};

__device__ __forceinline__ short d_sat_short(int v) { return (short)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

__device__ __forceinline__ Tap quantise(float mx, float my)
{
    int sxq = d_cvround(mx * 32.f), syq = d_cvround(my * 32.f);
    Tap t;
    t.fx = sxq & 31; t.fy = syq & 31;
    t.sx = d_sat_short(sxq >> 5); t.sy = d_sat_short(syq >> 5);
    return t;
}

// 15-bit fixed-point bilinear weights of OpenCV's BilinearTab_i (A.2), including the
// [32767,0,0,1] entry that the table's sum fix-up produces at zero fraction.
__device__ __forceinline__ void weights_i(int fx, int fy, int w[4])
{
    if ((fx | fy) == 0) { w[0] = 32767; w[1] = 0; w[2] = 0; w[3] = 1; return; }
    w[0] = (32 - fy) * (32 - fx) * 32; w[1] = (32 - fy) * fx * 32;
    w[2] = fy * (32 - fx) * 32;        w[3] = fy * fx * 32;
}
__device__ __forceinline__ void weights_f(int fx, int fy, float w[4])
{
    // products of the exact 1-D weights (1 - f/32, f/32): exact in float
    const float s = 1.f / 32.f;
    float x1 = fx * s, x0 = 1.f - x1, y1 = fy * s, y0 = 1.f - y1;
    w[0] = y0 * x0; w[1] = y0 * x1; w[2] = y1 * x0; w[3] = y1 * x1;
}

// the four taps (top left, top right, bottom left, bottom right) summed in that order; taps outside the source hold 0
template <typename T> struct Interp;
template <> struct Interp<uint8_t> {
    __device__ static uint8_t run(uint8_t v0, uint8_t v1, uint8_t v2, uint8_t v3, int fx, int fy)
    {
        int w[4];
        weights_i(fx, fy, w);
        int acc = v0 * w[0] + v1 * w[1] + v2 * w[2] + v3 * w[3];
        return (uint8_t)d_clamp((acc + (1 << 14)) >> 15, 0, 255);
    }
};
template <> struct Interp<uint16_t> {
    __device__ static uint16_t run(uint16_t v0, uint16_t v1, uint16_t v2, uint16_t v3, int fx, int fy)
    {
        float w[4];
        weights_f(fx, fy, w);
        float acc = (float)v0 * w[0] + (float)v1 * w[1] + (float)v2 * w[2] + (float)v3 * w[3];
        return (uint16_t)d_clamp(d_cvround(acc), 0, 65535);
    }
};
template <> struct Interp<float> {
    __device__ static float run(float v0, float v1, float v2, float v3, int fx, int fy)
    {
        float w[4];
        weights_f(fx, fy, w);
        return v0 * w[0] + v1 * w[1] + v2 * w[2] + v3 * w[3];
    }
};

// Window origin along x of column `x` (ox = (x / T) T - ov) without a division per lane: the 64 columns of a wave lie in at
// most two windows when T >= 64 -- the wave's first column decides (a scalar division), the columns at or beyond the next
// window's first take that one.
__device__ __forceinline__ int warp_window_origin_x(int x, const MaTiling& g)
{
    if (g.T <= 0) return 0;
    if (g.T < 64) return (x / g.T) * g.T - g.ov;
    const int x_first = __builtin_amdgcn_readfirstlane(x - (int)(threadIdx.x & 63));
    const int t0 = x_first / g.T, next = (t0 + 1) * g.T;
    return (x >= next ? next : t0 * g.T) - g.ov;
}
// Window origins along y of the rows y0 .. y0 + R of a block: one division, the rows at or beyond the next window's first
// row take that one (T >= R; smaller tiles divide per row)
struct WarpRowsY {
    int t0T, next, T, ov;
    __device__ __forceinline__ WarpRowsY(int y0, const MaTiling& g) : T(g.T), ov(g.ov)
    {
        const int t0 = g.T > 0 ? y0 / g.T : 0;
        t0T = t0 * g.T; next = t0T + g.T;
    }
    __device__ __forceinline__ int origin(int y) const
    {
        if (T <= 0) return 0;
        if (T < 16) return (y / T) * T - ov;
        return (y >= next ? next : t0T) - ov;
    }
};

} // namespace

#endif // MA_REMAP_COMMON_H
