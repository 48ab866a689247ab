// Push-pull fill of a flow (include/microaligner_flowfill.h).  Off the measured path: nothing in register() or warp() calls
// it.
//
// A level above level 0 is stored as one 16-byte entry (a_u, a_v, t, unused) per pixel, so that a child or a tap is one
// load; the push writes G over a in place (8 bytes of the entry).  Level 0 is never stored: t0 and a0 are read from the flow
// and the weight, in the first pull and again in the last push.
//
// Every kernel gives a thread one PARENT (j, i) and the 2 x 2 quad of children (2j + dy, 2i + dx) below it; a block of 256
// threads is 4 parent rows of 64 parents, lane = column, so a wave reads two runs of 128 children and writes one row of 64
// parents, all coalesced:
//   - ff_pull0<KIND>: the quad of level 0 from float2 flow loads, the weight read beside them -> the entry of level 1;
//   - ff_pull       : the quad of level l -> the entry of level l + 1;
//   - ff_push       : the 3 x 3 neighbourhood of the parent in G_{l+1} serves the four outputs of the quad: three rows of
//                     two row interpolations each, then four column interpolations, then the blend with (a, t) of level l;
//   - ff_push0<KIND>: the same over the flow and the weight, out, and the three counts (call_counts.h).
// The pull that makes the 1 x 1 level applies the header's "top" rule (NaN where nothing was kept).  No LDS, no scratch.
#include "../../include/microaligner_flowfill.h"
#include "call_counts.h"
#include "weight_map.h"

#include <cmath>

namespace {

constexpr int FF_SIDE_MAX = 1 << 24;
constexpr int FF_PW = 64, FF_PH = 4;            // the parents of a block: a tile of 2 FF_PH x 2 FF_PW children
constexpr size_t FF_LEVELS_AT = 256;            // the levels' offset in the workspace, behind the three counters
constexpr int FF_MAX_LEVELS = 25;

struct FfSample {   // (a, t) of the header
    float2 a;
    float t;
};

__device__ __forceinline__ float ff_nan() { return __int_as_float(0x7fc00000); }

// (a0, t0) of pixel (x, y) of level 0; i = y * W + x
template <int KIND>
__device__ __forceinline__ FfSample ff_level0(const float2* flow, const MaWeight& wt, size_t i, int x, int y)
{
    const float2 f = flow[i];
    const float w = d_weight_at<KIND>(wt, i, x, y);
    const bool kept = d_weight_counts(w) && d_finite(f.x) && d_finite(f.y);
    FfSample s;
    s.t = kept ? fminf(w, 1.f) : 0.f;
    s.a = kept ? f : make_float2(0.f, 0.f);
    return s;
}

// the parent entry of the four children c[dy][dx]; top: the level made is the 1 x 1 one
__device__ __forceinline__ float4 ff_parent(const FfSample (&c)[2][2], bool top)
{
    const float sw = (c[0][0].t + c[0][1].t) + (c[1][0].t + c[1][1].t);
    const float su = (c[0][0].t * c[0][0].a.x + c[0][1].t * c[0][1].a.x) + (c[1][0].t * c[1][0].a.x + c[1][1].t * c[1][1].a.x);
    const float sv = (c[0][0].t * c[0][0].a.y + c[0][1].t * c[0][1].a.y) + (c[1][0].t * c[1][0].a.y + c[1][1].t * c[1][1].a.y);
    const float none = top ? ff_nan() : 0.f;
    float4 e;
    e.x = sw > 0.f ? __fdiv_rn(su, sw) : none;
    e.y = sw > 0.f ? __fdiv_rn(sv, sw) : none;
    e.z = fminf(sw, 1.f);
    e.w = 0.f;
    return e;
}

// the parent (j, i) of this thread; false beyond the hc x wc parents
__device__ __forceinline__ bool ff_thread_parent(int hc, int wc, int nbx, int* j, int* i)
{
    *i = (int)(blockIdx.x % nbx) * FF_PW + (int)(threadIdx.x & 63);
    *j = (int)(blockIdx.x / nbx) * FF_PH + (int)(threadIdx.x >> 6);
    return *i < wc && *j < hc;
}

template <int KIND>
__global__ __launch_bounds__(256) void ff_pull0(const float2* __restrict__ flow, int H, int W, MaWeight wt,
                                                float4* __restrict__ dst, int hc, int wc, int nbx, int top)
{
    int j, i;
    if (!ff_thread_parent(hc, wc, nbx, &j, &i)) return;
    FfSample c[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const int y = 2 * j + dy, x = 2 * i + dx;
            c[dy][dx].a = make_float2(0.f, 0.f);
            c[dy][dx].t = 0.f;
            if (y < H && x < W) c[dy][dx] = ff_level0<KIND>(flow, wt, (size_t)y * W + x, x, y);
        }
    dst[(size_t)j * wc + i] = ff_parent(c, top != 0);
}

__global__ __launch_bounds__(256) void ff_pull(const float4* __restrict__ src, int h, int w, float4* __restrict__ dst, int hc,
                                               int wc, int nbx, int top)
{
    int j, i;
    if (!ff_thread_parent(hc, wc, nbx, &j, &i)) return;
    FfSample c[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const int y = 2 * j + dy, x = 2 * i + dx;
            c[dy][dx].a = make_float2(0.f, 0.f);
            c[dy][dx].t = 0.f;
            if (y < h && x < w) {
                const float4 e = src[(size_t)y * w + x];
                c[dy][dx].a = make_float2(e.x, e.y);
                c[dy][dx].t = e.z;
            }
        }
    dst[(size_t)j * wc + i] = ff_parent(c, top != 0);
}

// up[dy][dx] of the header for the quad below parent (j, i), from the 3 x 3 neighbourhood of (j, i) in G (hc x wc entries)
__device__ __forceinline__ void ff_expand(const float4* __restrict__ G, int hc, int wc, int j, int i, float2 (&up)[2][2])
{
    const int jj[3] = {j > 0 ? j - 1 : 0, j, j + 1 < hc ? j + 1 : hc - 1};
    const int ii[3] = {i > 0 ? i - 1 : 0, i, i + 1 < wc ? i + 1 : wc - 1};
    float2 hrow[3][2];       // [parent row][dx]
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float2* row = reinterpret_cast<const float2*>(G + (size_t)jj[r] * wc);      // (G_u, G_v) leads an entry
        const float2 g0 = row[2 * (size_t)ii[0]], g1 = row[2 * (size_t)ii[1]], g2 = row[2 * (size_t)ii[2]];
        hrow[r][0] = make_float2(0.25f * g0.x + 0.75f * g1.x, 0.25f * g0.y + 0.75f * g1.y);      // x even: (i - 1, i)
        hrow[r][1] = make_float2(0.75f * g1.x + 0.25f * g2.x, 0.75f * g1.y + 0.25f * g2.y);      // x odd : (i, i + 1)
    }
#pragma unroll
    for (int dx = 0; dx < 2; dx++) {
        up[0][dx] = make_float2(0.25f * hrow[0][dx].x + 0.75f * hrow[1][dx].x, 0.25f * hrow[0][dx].y + 0.75f * hrow[1][dx].y);
        up[1][dx] = make_float2(0.75f * hrow[1][dx].x + 0.25f * hrow[2][dx].x, 0.75f * hrow[1][dx].y + 0.25f * hrow[2][dx].y);
    }
}

// G_l(p) of the header from up and (a, t) of the level
__device__ __forceinline__ float2 ff_blend(const float2 up, const float2 a, const float t)
{
    if (t >= 1.f) return a;
    if (t == 0.f) return up;
    return make_float2(up.x + t * (a.x - up.x), up.y + t * (a.y - up.y));
}

// lvl: the h x w entries of level l, G written over a; G: the hc x wc entries of level l + 1, pushed already
__global__ __launch_bounds__(256) void ff_push(float4* __restrict__ lvl, int h, int w, const float4* __restrict__ G, int hc,
                                               int wc, int nbx)
{
    int j, i;
    if (!ff_thread_parent(hc, wc, nbx, &j, &i)) return;
    float2 up[2][2];
    ff_expand(G, hc, wc, j, i, up);
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const int y = 2 * j + dy, x = 2 * i + dx;
            if (y < h && x < w) {
                float4* e = lvl + (size_t)y * w + x;
                const float4 v = *e;
                *reinterpret_cast<float2*>(e) = ff_blend(up[dy][dx], make_float2(v.x, v.y), v.z);
            }
        }
}

// G == NULL: a flow of one pixel, which is its own top.  flow and out may be the same array: a thread reads the pixels it
// writes and no other.  counts: NULL, or {dropped, blended, unsupported}.
template <int KIND>
__global__ __launch_bounds__(256) void ff_push0(const float2* flow, int H, int W, MaWeight wt, const float4* __restrict__ G,
                                                int hc, int wc, int nbx, float2* out, unsigned long long* __restrict__ counts)
{
    int j, i;
    const bool active = ff_thread_parent(G ? hc : 1, G ? wc : 1, nbx, &j, &i);
    unsigned int dropped = 0, blended = 0, unsupported = 0;
    if (active) {
        float2 up[2][2];
        if (G) ff_expand(G, hc, wc, j, i, up);
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
            for (int dx = 0; dx < 2; dx++) {
                const int y = 2 * j + dy, x = 2 * i + dx;
                if (y < H && x < W) {
                    const size_t p = (size_t)y * W + x;
                    const FfSample s = ff_level0<KIND>(flow, wt, p, x, y);
                    float2 o;
                    if (G) o = ff_blend(up[dy][dx], s.a, s.t);
                    else o = s.t > 0.f ? s.a : make_float2(ff_nan(), ff_nan());
                    out[p] = o;
                    dropped += s.t == 0.f ? 1u : 0u;
                    blended += s.t > 0.f && s.t < 1.f ? 1u : 0u;
                    unsupported += d_finite(o.x) && d_finite(o.y) ? 0u : 1u;
                }
            }
    }
    if (counts) d_wave_tally(counts, {dropped, blended, unsupported});     // wave-uniform
}

// the blocks of a launch over hc x wc parents
inline long long ff_blocks(int hc, int wc, int* nbx)
{
    *nbx = (wc + FF_PW - 1) / FF_PW;
    return (long long)*nbx * ((hc + FF_PH - 1) / FF_PH);
}

} // namespace

extern "C" int ma_fill_flow(ma_ctx* ctx, const float* flow, int H, int W, const void* weight, int weight_kind, int cell_h,
                            int cell_w, float* out, long long* counts_host)
{
    MA_REQUIRE(ctx && flow && out, "NULL argument");
    MA_REQUIRE_ALIGNED(flow, 8, "flow");
    MA_REQUIRE_ALIGNED(out, 8, "out");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= FF_SIDE_MAX && W <= FF_SIDE_MAX, "flow sides must be in [1, 2^24]");
    MA_TRY(ma_weight_check(weight, weight_kind, true, {out}, cell_h, cell_w));
    // level l has hs[l] x ws[l] entries; level l >= 1 starts at entry at[l] of the stored levels
    int hs[FF_MAX_LEVELS + 1], ws[FF_MAX_LEVELS + 1], L = 0;
    size_t at[FF_MAX_LEVELS + 2];
    hs[0] = H;
    ws[0] = W;
    at[1] = 0;
    while (hs[L] > 1 || ws[L] > 1) {
        hs[L + 1] = (hs[L] + 1) / 2;
        ws[L + 1] = (ws[L] + 1) / 2;
        L++;
        at[L + 1] = at[L] + (size_t)hs[L] * ws[L];
    }
    int nbx;
    MA_REQUIRE(ff_blocks(L ? hs[1] : 1, L ? ws[1] : 1, &nbx) <= 0x7fffffffLL,
               "flow too large: more than 2^31 - 1 tiles of 8 x 128 pixels");
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ma_ws_reserve(ctx, FF_LEVELS_AT + at[L + 1] * sizeof(float4)));
    unsigned long long* counts;
    MA_TRY(ma_call_counts(ctx, counts_host != nullptr, 3, &counts));      // behind the reserve of the levels: ctx->ws is final
    float4* levels = (float4*)((char*)ctx->ws + FF_LEVELS_AT);
    auto level = [&](int l) { return levels + at[l]; };
    const MaWeight wt = ma_weight_map(weight, weight_kind, W, cell_h, cell_w);
    if (L >= 1) {
        const unsigned grid = (unsigned)ff_blocks(hs[1], ws[1], &nbx);
        ma_weight_dispatch(weight_kind, [&](auto kind) {
            hipLaunchKernelGGL((ff_pull0<kind()>), dim3(grid), dim3(256), 0, ctx->stream, (const float2*)flow, H, W, wt, level(1),
                               hs[1], ws[1], nbx, L == 1 ? 1 : 0);
        });
    }
    for (int l = 1; l < L; l++) {
        const unsigned grid = (unsigned)ff_blocks(hs[l + 1], ws[l + 1], &nbx);
        hipLaunchKernelGGL(ff_pull, dim3(grid), dim3(256), 0, ctx->stream, (const float4*)level(l), hs[l], ws[l], level(l + 1),
                           hs[l + 1], ws[l + 1], nbx, l + 1 == L ? 1 : 0);
    }
    for (int l = L - 1; l >= 1; l--) {
        const unsigned grid = (unsigned)ff_blocks(hs[l + 1], ws[l + 1], &nbx);
        hipLaunchKernelGGL(ff_push, dim3(grid), dim3(256), 0, ctx->stream, level(l), hs[l], ws[l], (const float4*)level(l + 1),
                           hs[l + 1], ws[l + 1], nbx);
    }
    {
        const int hc = L ? hs[1] : 1, wc = L ? ws[1] : 1;
        const unsigned grid = (unsigned)ff_blocks(hc, wc, &nbx);
        const float4* G = L ? level(1) : nullptr;
        ma_weight_dispatch(weight_kind, [&](auto kind) {
            hipLaunchKernelGGL((ff_push0<kind()>), dim3(grid), dim3(256), 0, ctx->stream, (const float2*)flow, H, W, wt, G, hc, wc,
                               nbx, (float2*)out, counts);
        });
    }
    MA_HIP(hipGetLastError());
    if (counts_host) MA_TRY(ma_read_call_counts(ctx, counts, 3, counts_host));
    return MA_OK;
}
