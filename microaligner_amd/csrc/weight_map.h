// The weight argument of the calls that take one (flow_smooth.hip, flow_median.hip, flow_fill.hip, flow_affine.hip,
// direct_affine.hip, flow_refine.hip, local_correlation.hip, local_norm.hip), stated once: how a kernel reads weight(p) of include/microaligner_flowsmooth.h and
// how a C entry checks and passes it.  Off the measured path (a header of single sources, build.SOURCE_HEADERS).
#pragma once
#include "../../include/microaligner_flowsmooth.h"
#include "ma_internal.h"

#include <cmath>
#include <initializer_list>
#include <type_traits>

namespace {

// a weight as a kernel takes it: per pixel, or for MA_SMOOTH_WEIGHT_CELLS the (gy, gx) map of ch x cw cells
struct MaWeight {
    const void* p;
    int ch, cw, gx;
};

__device__ __forceinline__ bool d_finite(float v) { return fabsf(v) < INFINITY; }

// does a pixel of this weight take part?  local_correlation.hip states the test in place: with this function the float32
// instantiation of its row kernel compiles to other code.
__device__ __forceinline__ bool d_weight_counts(float w) { return w > 0.f && w < INFINITY; }

// weight(p) of the header for a kind known at compile time; i = y * W + x
template <int KIND>
__device__ __forceinline__ float d_weight_at(const MaWeight& wt, size_t i, int x, int y)
{
    if (KIND == MA_SMOOTH_WEIGHT_F32) return ((const float*)wt.p)[i];
    if (KIND == MA_SMOOTH_WEIGHT_U8) return ((const unsigned char*)wt.p)[i] ? 1.f : 0.f;
    if (KIND == MA_SMOOTH_WEIGHT_CELLS) return ((const float*)wt.p)[(size_t)(y / wt.ch) * wt.gx + x / wt.cw];
    return 1.f;
}

// weight(p) of a per-pixel weight whose kind is a kernel argument (wave-uniform branches); 1 for every other kind.
// flow_affine.hip reads a per-cell map itself, one entry per block: its cells are the cells of the call, not a lookup by pixel.
__device__ __forceinline__ float d_weight_px(const void* p, int kind, size_t i)
{
    if (kind == MA_SMOOTH_WEIGHT_F32) return ((const float*)p)[i];
    if (kind == MA_SMOOTH_WEIGHT_U8) return ((const unsigned char*)p)[i] ? 1.f : 0.f;
    return 1.f;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// The weight of a C entry: a kind the entry accepts (cells: a per-cell map among them), not NULL unless the kind is NONE, none
// of the arrays the entry writes, and for a per-cell map a cell size.
inline int ma_weight_check(const void* weight, int kind, bool cells, std::initializer_list<const void*> outs, int cell_h,
                           int cell_w)
{
    MA_REQUIRE(kind >= MA_SMOOTH_WEIGHT_NONE && kind <= (cells ? MA_SMOOTH_WEIGHT_CELLS : MA_SMOOTH_WEIGHT_U8),
               cells ? "unknown weight kind" : "the weight must be none or per pixel, float32 or uint8");
    if (kind == MA_SMOOTH_WEIGHT_NONE) return MA_OK;
    MA_REQUIRE(weight, "NULL weight");
    for (const void* out : outs) MA_REQUIRE(weight != out, "the weight must be none of the arrays written");
    MA_REQUIRE(kind != MA_SMOOTH_WEIGHT_CELLS || (cell_h >= 1 && cell_w >= 1), "cell size must be >= 1");
    return MA_OK;
}

// the checked weight of an (H, W) call as its kernels take it
inline MaWeight ma_weight_map(const void* weight, int kind, int W, int cell_h, int cell_w)
{
    if (kind != MA_SMOOTH_WEIGHT_CELLS) return MaWeight{weight, 1, 1, 1};
    return MaWeight{weight, cell_h, cell_w, (int)(((long long)W + cell_w - 1) / cell_w)};
}

// f(std::integral_constant<int, KIND>) for a checked kind
template <class F>
auto ma_weight_dispatch(int kind, F&& f)
{
    switch (kind) {
    case MA_SMOOTH_WEIGHT_F32: return f(std::integral_constant<int, MA_SMOOTH_WEIGHT_F32>{});
    case MA_SMOOTH_WEIGHT_U8: return f(std::integral_constant<int, MA_SMOOTH_WEIGHT_U8>{});
    case MA_SMOOTH_WEIGHT_CELLS: return f(std::integral_constant<int, MA_SMOOTH_WEIGHT_CELLS>{});
    default: return f(std::integral_constant<int, MA_SMOOTH_WEIGHT_NONE>{});
    }
}

} // namespace
