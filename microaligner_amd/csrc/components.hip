// Connected components: labels, areas and boxes, and the two filters built from them (include/microaligner_components.h).
// Off the measured path: nothing in register() or warp() calls it.
//
// The state of every call is one int32 plane, `parent`: parent[p] is a pixel of p's component with a linear index <= p, or
// CC_NONE where p is in no component.  A pixel with parent[p] == p is a root; at the end the only root of a component is its
// smallest pixel, which is what the numbering of the header sorts by.
//   1. cc_tile_kernel: a block of 256 threads labels a tile of 64 x 64 pixels in LDS.  A wave takes a row: one ballot gives
//      every lane the start of its run of joined pixels, which is the run's first label.  A run is then united with the runs
//      above it by union-find on the LDS labels (atomicMin on the larger root), only where the pair is not implied by the
//      pair to its left, and the labels are flattened.  The smallest local index of a local component is its smallest
//      linear index, so parent[p] = the linear index of p's local root.  For the filters the block also counts every local
//      root's pixels, run by run, and notes in bit 31 whether a run lies on the image border: `area`, a second plane, gets
//      that word at the local roots and 0 elsewhere.  For ma_cc_stats the same kernel runs on the finished labels (joined by
//      value under 8 neighbours) and adds every local root's count and box to the arrays of its label: one global atomic of each kind per
//      piece of a component in a tile, none per pixel.
//   2. cc_seam_kernel: a thread per pixel beside a tile border joins it to its neighbours in the next tile: find both roots
//      (agent-scope relaxed atomic loads: other XCDs write these words during the launch), atomicMin the larger root's word
//      to the smaller root, go on from the value the atomic returned.  Parents only decrease and every value stored is a
//      pixel of the same component, so the loops end and the last root is the smallest pixel whatever the order.  A pair is
//      left out where the pair one pixel back along the seam and the two tile-local joins imply it (an all-ones image: one
//      union per tile side, not 64), and a diagonal pair where the pixel above its lower end joins both.
//      No thread waits for another one anywhere: no flags, no spinning, no cooperative launch.
//   3. cc_flatten_kernel: parent[p] = root(p).  For the filters it also adds the word of every local root that is no root to
//      its root's (the counts with atomicAdd, bit 31 with atomicOr: at most 2^31 - 1 pixels, so no carry reaches the bit);
//      for the labels it counts the roots of every segment of 1024 pixels instead.
//   4. labels: cc_scan_kernel (one block) turns the counts of the segments into their exclusive sums and the total,
//      cc_rank_kernel gives every root 1 + the number of roots before it (segment sum + ballot and popcount) in a second
//      plane, cc_relabel_kernel writes labels[p] = rank[parent[p]].  A thread of the last kernel reads and writes only its
//      own word of `labels` (the parent plane) and reads the other plane: no race.
//      filters: cc_select_kernel writes dst[p] from src[p] and the word of p's root.
// Every sum is an integer, so nothing depends on the order the atomics arrive in.
#include "../../include/microaligner_components.h"
#include "ma_internal.h"

#include <algorithm>
#include <climits>

namespace {

constexpr int CC_SIDE_MAX = 1 << 24;
constexpr int CC_T = MA_CC_TILE, CC_PIX = CC_T * CC_T, CC_THREADS = 256, CC_ROWS = CC_T / (CC_THREADS / 64);
constexpr int CC_SEG = 1024;                      // pixels of a segment of the pixel-linear kernels: 256 threads x 4
constexpr int CC_NONE = -1;                       // the parent of a pixel that is in no component
constexpr unsigned CC_BORDER = 0x80000000u, CC_COUNT = 0x7fffffffu;   // the word of a root: bit 31 and the pixel count
static_assert(CC_T == 64 && CC_ROWS == 16, "a wave holds one row of a tile");

enum { CC_KEY_FG = 0, CC_KEY_VALUE = 1, CC_KEY_HOLES = 2 };             // what joins two pixels
enum { CC_OUT_PARENT = 0, CC_OUT_AREA = 1, CC_OUT_STATS = 2 };          // what the tile kernel leaves

// the key of a pixel: 0 where it is in no component, otherwise equal for pixels that may be joined
template <typename T>
__device__ __forceinline__ int cc_key(T v, int mode)
{
    if (mode == CC_KEY_HOLES) return v == 0 ? 1 : 0;
    if (mode == CC_KEY_VALUE) return (int)v;
    return v != 0 ? 1 : 0;
}

// ---- union-find on the labels of a tile in LDS ----------------------------------------------------------------------------
__device__ __forceinline__ int cc_lds_find(const volatile int* lab, int a)
{
    for (int t; (t = lab[a]) != a;) a = t;
    return a;
}

__device__ __forceinline__ void cc_lds_union(int* lab, int a, int b)
{
    for (;;) {
        a = cc_lds_find(lab, a);
        b = cc_lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lab[a], b);      // a was a root when it was read; old != a: another union moved it
        if (old == a) return;
        a = old;
    }
}

// ---- union-find on the parent plane ---------------------------------------------------------------------------------------
__device__ __forceinline__ int cc_load(int* parent, int a) { return __hip_atomic_load(&parent[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int cc_find(int* parent, int a)
{
    for (int t; (t = cc_load(parent, a)) != a;) a = t;
    return a;
}

__device__ __forceinline__ void cc_union(int* parent, int a, int b)
{
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&parent[a], b);   // agent scope
        if (old == a) return;
        a = old;                                    // smaller than a and in the same component: go on from there
    }
}

// The run of equal labels of a row of the tile that `lane` starts: its last column, or -1 where the lane starts none.
// After the flattening two neighbours of a row have one label exactly where the tile pass put them in one run.  Every lane
// of the wave calls it.
__device__ __forceinline__ int cc_run_end(int l, int lane)
{
    const int left = __shfl_up(l, 1);
    const bool same = lane > 0 && l >= 0 && left == l;
    const unsigned long long b = __ballot(same);
    if (l < 0 || same) return -1;
    const unsigned long long above = lane == 63 ? 0ull : (~b & (~0ull << (lane + 1)));
    return above ? __ffsll((long long)above) - 2 : 63;
}

// One tile.  OUT = CC_OUT_PARENT: parent;  CC_OUT_AREA: parent and area;  CC_OUT_STATS: src holds labels, pixels of one
// value in 1 .. nmax are joined under 8 neighbours (the widest relation, so the fewest local roots, whatever made the labels),
// and areas / bboxes take every local root's count and box.
template <typename T, int OUT>
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const T* src, int H, int W, int ntx, int mode, int conn8, int nmax,
                                                             int* parent, unsigned* area, unsigned long long* areas, int* bboxes)
{
    __shared__ int s_key[CC_PIX];      // the keys; afterwards the scratch words of the local roots
    __shared__ int s_lab[CC_PIX];
    __shared__ int s_bg;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int x0 = (int)(blockIdx.x % (unsigned)ntx) * CC_T, y0 = (int)(blockIdx.x / (unsigned)ntx) * CC_T;
    const int gx = x0 + lane;
    if (OUT == CC_OUT_STATS && tid == 0) s_bg = 0;
    // keys, and every pixel's label: the first pixel of its run
    int nbg = 0;
    for (int j = 0; j < CC_ROWS; j++) {
        const int ly = j * 4 + wv, gy = y0 + ly, p = ly * CC_T + lane;
        int k = 0;
        bool zero = false;
        if (gy < H && gx < W) {
            const T v = src[(size_t)gy * W + gx];
            if (OUT == CC_OUT_STATS) {
                k = (v >= 1 && v <= nmax) ? (int)v : 0;
                zero = v == 0;
            } else {
                k = cc_key(v, mode);
            }
        }
        if (OUT == CC_OUT_STATS) nbg += __popcll(__ballot(zero));
        const int kl = __shfl_up(k, 1);
        const bool same = lane > 0 && k != 0 && kl == k;
        const unsigned long long breaks = ~__ballot(same) & (~0ull >> (63 - lane));   // bit 0 is always one
        s_key[p] = k;
        s_lab[p] = k ? ly * CC_T + 63 - __clzll((long long)breaks) : CC_NONE;
    }
    __syncthreads();
    if (OUT == CC_OUT_STATS && lane == 0 && nbg) atomicAdd(&s_bg, nbg);
    // unite a pixel with the row above.  The pair straight up is implied where the pixel to the left and the one above that
    // are of the same key (runs join them, and that pair is united or implied in turn); a diagonal pair where the pixel
    // straight up is of the same key.
    for (int j = 0; j < CC_ROWS; j++) {
        const int ly = j * 4 + wv, p = ly * CC_T + lane;
        const int k = s_key[p];
        if (ly == 0 || k == 0) continue;
        if (s_key[p - CC_T] == k) {
            if (!(lane > 0 && s_key[p - 1] == k && s_key[p - CC_T - 1] == k)) cc_lds_union(s_lab, p, p - CC_T);
        } else if (conn8) {
            if (lane > 0 && s_key[p - CC_T - 1] == k) cc_lds_union(s_lab, p, p - CC_T - 1);
            if (lane < 63 && s_key[p - CC_T + 1] == k) cc_lds_union(s_lab, p, p - CC_T + 1);
        }
    }
    __syncthreads();
    // flatten.  Other threads store roots over labels meanwhile: a chain read half way still ends at the root.
    for (int j = 0; j < CC_ROWS; j++) {
        const int p = (j * 4 + wv) * CC_T + lane;
        if (s_lab[p] >= 0) {
            const int r = cc_lds_find(s_lab, p);
            reinterpret_cast<volatile int*>(s_lab)[p] = r;
        }
    }
    __syncthreads();
    if (OUT != CC_OUT_STATS) {
        for (int j = 0; j < CC_ROWS; j++) {
            const int ly = j * 4 + wv, gy = y0 + ly, l = s_lab[ly * CC_T + lane];
            if (gy < H && gx < W) parent[(size_t)gy * W + gx] = l < 0 ? CC_NONE : (y0 + (l >> 6)) * W + x0 + (l & 63);
        }
    }
    unsigned* scr = reinterpret_cast<unsigned*>(s_key);
    if (OUT == CC_OUT_AREA) {
        for (int j = 0; j < CC_ROWS; j++) scr[(j * 4 + wv) * CC_T + lane] = 0;
        __syncthreads();
        for (int j = 0; j < CC_ROWS; j++) {
            const int ly = j * 4 + wv, gy = y0 + ly, l = s_lab[ly * CC_T + lane];
            const int end = cc_run_end(l, lane);
            if (end < 0) continue;
            atomicAdd(&scr[l], (unsigned)(end - lane + 1));
            if (gy == 0 || gy == H - 1 || gx == 0 || x0 + end == W - 1) atomicOr(&scr[l], CC_BORDER);
        }
        __syncthreads();
        for (int j = 0; j < CC_ROWS; j++) {
            const int ly = j * 4 + wv, gy = y0 + ly, p = ly * CC_T + lane;
            if (gy < H && gx < W) area[(size_t)gy * W + gx] = s_lab[p] == p ? scr[p] : 0u;
        }
    }
    if (OUT == CC_OUT_STATS) {
        // four rounds over one scratch word per local root: count, first column, last column + 1, last row + 1; the first
        // row of a local component is its root's.  After each the thread of the root adds it to the label's entry.
        for (int round = 0; round < 4; round++) {
            for (int j = 0; j < CC_ROWS; j++) scr[(j * 4 + wv) * CC_T + lane] = round == 1 ? (unsigned)CC_T : 0u;
            __syncthreads();
            for (int j = 0; j < CC_ROWS; j++) {
                const int ly = j * 4 + wv, l = s_lab[ly * CC_T + lane];
                const int end = cc_run_end(l, lane);
                if (end < 0) continue;
                if (round == 0) atomicAdd(&scr[l], (unsigned)(end - lane + 1));
                else if (round == 1) atomicMin(&scr[l], (unsigned)lane);
                else if (round == 2) atomicMax(&scr[l], (unsigned)(end + 1));
                else atomicMax(&scr[l], (unsigned)(ly + 1));
            }
            __syncthreads();
            for (int j = 0; j < CC_ROWS; j++) {
                const int ly = j * 4 + wv, p = ly * CC_T + lane;
                if (s_lab[p] != p) continue;
                const size_t k = (size_t)src[(size_t)(y0 + ly) * W + gx];      // in 1 .. nmax: the pixel has a key
                const int v = (int)scr[p];
                if (round == 0) {
                    atomicAdd(&areas[k], (unsigned long long)v);
                    atomicMin(&bboxes[4 * k], y0 + ly);
                } else if (round == 1) {
                    atomicMin(&bboxes[4 * k + 1], x0 + v);
                } else if (round == 2) {
                    atomicMax(&bboxes[4 * k + 3], x0 + v);
                } else {
                    atomicMax(&bboxes[4 * k + 2], y0 + v);
                }
            }
            __syncthreads();
        }
        if (tid == 0 && s_bg) atomicAdd(&areas[0], (unsigned long long)s_bg);
    }
}

// One thread per pixel below a row seam (rows 64, 128, ...: i < nrs * W) and per pixel right of a column seam (columns 64,
// 128, ...: the next ncs * H).
template <typename T>
__global__ __launch_bounds__(256) void cc_seam_kernel(const T* src, int H, int W, int mode, int conn8, int nrs, int ncs, int* parent)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nrow = (long long)nrs * W;
    auto key = [&](int y, int x) { return cc_key(src[(size_t)y * W + x], mode); };
    if (i < nrow) {
        const int y = ((int)(i / W) + 1) * CC_T, x = (int)(i % W);
        const int k = key(y, x);
        if (k == 0) return;
        const int p = y * W + x;
        if (key(y - 1, x) == k) {
            if (!((x & (CC_T - 1)) != 0 && key(y - 1, x - 1) == k && key(y, x - 1) == k)) cc_union(parent, p, p - W);
        } else if (conn8) {
            if (x > 0 && key(y - 1, x - 1) == k) cc_union(parent, p, p - W - 1);
            if (x + 1 < W && key(y - 1, x + 1) == k) cc_union(parent, p, p - W + 1);
        }
    } else if (i < nrow + (long long)ncs * H) {
        const long long c = i - nrow;
        const int x = ((int)(c / H) + 1) * CC_T, y = (int)(c % H);
        const int k = key(y, x), kl = key(y, x - 1);
        const int p = y * W + x;
        if (k != 0 && kl == k) {
            if (!((y & (CC_T - 1)) != 0 && key(y - 1, x - 1) == k && key(y - 1, x) == k)) cc_union(parent, p, p - 1);
        }
        if (conn8) {
            // down to the right across the seam: (y - 1, x - 1) and (y, x), implied where (y - 1, x) joins both
            if (k != 0 && y > 0 && key(y - 1, x - 1) == k && key(y - 1, x) != k) cc_union(parent, p, p - W - 1);
            // down to the left across the seam: (y, x) and (y + 1, x - 1), implied where (y, x - 1) joins both
            if (k != 0 && y + 1 < H && kl != k && key(y + 1, x - 1) == k) cc_union(parent, p, p + W - 1);
        }
    }
}

// parent[p] = root(p).  AREA: the word of a local root that is no root goes to its root's; otherwise segs[block] = the roots
// of the block's segment.  Roots are never written here and the words of the others are only read, so the sums are exact.
template <bool AREA>
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* parent, unsigned N, unsigned* area, int* segs)
{
    __shared__ int s_cnt[4];
    const unsigned base = blockIdx.x * (unsigned)CC_SEG;
    int roots = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned p = base + i * 256 + threadIdx.x;
        bool root = false;
        if (p < N) {
            const int t = cc_load(parent, (int)p);
            if (t >= 0) {
                const int r = t == (int)p ? t : cc_find(parent, t);
                if (r != t) __hip_atomic_store(&parent[p], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                root = r == (int)p;
                if (AREA && !root) {
                    const unsigned a = area[p];
                    if (a) {
                        atomicAdd(&area[r], a & CC_COUNT);
                        if (a & CC_BORDER) atomicOr(&area[r], CC_BORDER);
                    }
                }
            }
        }
        if (!AREA) roots += __popcll(__ballot(root));
    }
    if (!AREA) {
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = roots;
        __syncthreads();
        if (threadIdx.x == 0) segs[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
}

// segs[0 .. nseg) -> their exclusive sums, segs[nseg] = the total.  One block: a thread sums a stretch, the block scans
// the 1024 sums, the thread writes its stretch.
__global__ __launch_bounds__(1024) void cc_scan_kernel(int* segs, int nseg)
{
    __shared__ int s_sum[1024];
    const int tid = threadIdx.x, per = (nseg + 1023) / 1024;
    const int b = min(tid * per, nseg), e = min(b + per, nseg);
    int s = 0;
    for (int i = b; i < e; i++) s += segs[i];
    s_sum[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? s_sum[tid - off] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    int run = s_sum[tid] - s;
    for (int i = b; i < e; i++) {
        const int c = segs[i];
        segs[i] = run;
        run += c;
    }
    if (tid == 1023) segs[nseg] = s_sum[1023];
}

// rank[p] = 1 + the number of roots below p, for every root p; the other words of rank are not written and never read
__global__ __launch_bounds__(256) void cc_rank_kernel(const int* parent, unsigned N, const int* segs, int* rank)
{
    __shared__ int s_c[16];
    const unsigned base = blockIdx.x * (unsigned)CC_SEG;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    bool root[4];
    unsigned long long bal[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned p = base + i * 256 + threadIdx.x;
        root[i] = p < N && parent[p] == (int)p;
        bal[i] = __ballot(root[i]);
        if (lane == 0) s_c[i * 4 + wv] = __popcll(bal[i]);
    }
    __syncthreads();
    int before = segs[blockIdx.x];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        for (int q = 0; q < 4; q++) {
            if (q == wv && root[i]) rank[base + i * 256 + threadIdx.x] = before + __popcll(bal[i] & ((1ull << lane) - 1ull)) + 1;
            before += s_c[i * 4 + q];
        }
    }
}

// labels is the parent plane: a thread reads its own word, then rank, and writes its own word
__global__ __launch_bounds__(256) void cc_relabel_kernel(int* labels, unsigned N, const int* rank)
{
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= N) return;
    const int r = labels[p];
    labels[p] = r < 0 ? 0 : rank[r];
}

// dst from src and the word of the pixel's root (the header's ma_cc_filter)
template <typename T>
__global__ __launch_bounds__(256) void cc_select_kernel(const T* src, unsigned N, const int* parent, const unsigned* area, int holes,
                                                        unsigned lo, unsigned hi, T value, T* dst)
{
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= N) return;
    T v = src[p];
    const int r = parent[p];
    if (r >= 0) {
        const unsigned a = area[r], n = a & CC_COUNT;
        const bool selected = n >= lo && n <= hi && !(holes && (a & CC_BORDER));
        if (holes) {
            if (selected) v = value;
        } else if (!selected) {
            v = 0;
        }
    }
    dst[p] = v;
}

__global__ __launch_bounds__(256) void cc_stats_init_kernel(long long rows, unsigned long long* areas, int* bboxes)
{
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < rows; k += (long long)gridDim.x * 256) {
        areas[k] = 0;
        bboxes[4 * k] = INT_MAX;
        bboxes[4 * k + 1] = INT_MAX;
        bboxes[4 * k + 2] = 0;
        bboxes[4 * k + 3] = 0;
    }
}

// row 0 and the rows of values no pixel has: zeros
__global__ __launch_bounds__(256) void cc_stats_final_kernel(long long rows, const unsigned long long* areas, int* bboxes)
{
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < rows; k += (long long)gridDim.x * 256) {
        if (k == 0 || areas[k] == 0) {
            bboxes[4 * k] = 0;
            bboxes[4 * k + 1] = 0;
        }
    }
}

inline unsigned cc_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

static int cc_check_image(const void* ctx, int H, int W)
{
    MA_REQUIRE(ctx, "NULL argument");
    MA_REQUIRE(H >= 1 && W >= 1 && H <= CC_SIDE_MAX && W <= CC_SIDE_MAX, "image sides must be in [1, 2^24]");
    MA_REQUIRE((long long)H * W <= (long long)MA_CC_MAX_PIXELS, "image too large: H * W must be at most 2^31 - 1");
    return MA_OK;
}

// the tile pass and the seams of src into parent (and area)
template <typename T, int OUT>
static void cc_build(ma_ctx* ctx, const T* src, int H, int W, int mode, int conn8, int* parent, unsigned* area)
{
    const int ntx = (W + CC_T - 1) / CC_T, nty = (H + CC_T - 1) / CC_T;
    hipLaunchKernelGGL((cc_tile_kernel<T, OUT>), dim3((unsigned)ntx * (unsigned)nty), dim3(CC_THREADS), 0, ctx->stream, src, H, W,
                       ntx, mode, conn8, 0, parent, area, (unsigned long long*)nullptr, (int*)nullptr);
    const long long seam = (long long)(nty - 1) * W + (long long)(ntx - 1) * H;
    if (seam > 0)
        hipLaunchKernelGGL((cc_seam_kernel<T>), dim3(cc_blocks(seam, 256)), dim3(256), 0, ctx->stream, src, H, W, mode, conn8,
                           nty - 1, ntx - 1, parent);
}

template <typename T>
static void cc_filter_run(ma_ctx* ctx, const T* src, int H, int W, int mode, int conn8, long long lo, long long hi, long long value,
                          int* parent, unsigned* area, T* dst)
{
    const unsigned N = (unsigned)((long long)H * W);
    cc_build<T, CC_OUT_AREA>(ctx, src, H, W, mode, conn8, parent, area);
    hipLaunchKernelGGL((cc_flatten_kernel<true>), dim3(cc_blocks(N, CC_SEG)), dim3(256), 0, ctx->stream, parent, N, area, (int*)nullptr);
    hipLaunchKernelGGL((cc_select_kernel<T>), dim3(cc_blocks(N, 256)), dim3(256), 0, ctx->stream, src, N, parent, area,
                       mode == CC_KEY_HOLES ? 1 : 0, (unsigned)lo, (unsigned)hi, (T)value, dst);
}

static int cc_launch_check(const char* what)
{
    if (hipGetLastError() != hipSuccess) {
        ma_set_error("a launch of %s failed", what);
        return MA_EHIP;
    }
    return MA_OK;
}

static bool cc_dtype_ok(int dtype) { return dtype == MA_U8 || dtype == MA_U16 || dtype == MA_CC_I32; }

} // namespace

extern "C" int ma_cc_label(ma_ctx* ctx, const void* src, int dtype, int H, int W, int flags, int* labels, long long* count)
{
    MA_REQUIRE(ctx && src && labels && count, "NULL argument");
    MA_REQUIRE(cc_dtype_ok(dtype), "dtype must be uint8, uint16 or int32");
    MA_TRY(cc_check_image(ctx, H, W));
    MA_REQUIRE((flags & ~(MA_CC_CONN8 | MA_CC_BY_VALUE)) == 0, "unknown flags");
    const long long N = (long long)H * W;
    {
        const uintptr_t s = (uintptr_t)src, l = (uintptr_t)labels;
        MA_REQUIRE(l + (uintptr_t)N * 4 <= s || s + (uintptr_t)N * ma_esize(dtype) <= l, "labels must not overlap src");
    }
    const int nseg = (int)((N + CC_SEG - 1) / CC_SEG);
    MA_HIP(hipSetDevice(ctx->device));
    MA_TRY(ma_pinned_reserve(ctx, sizeof(int)));
    int* rank = (int*)ma_pool_alloc(ctx, ((size_t)N + (size_t)nseg + 1) * sizeof(int));
    if (!rank) return MA_ENOMEM;
    int* segs = rank + N;
    const int mode = (flags & MA_CC_BY_VALUE) ? CC_KEY_VALUE : CC_KEY_FG, conn8 = (flags & MA_CC_CONN8) ? 1 : 0;
    switch (dtype) {
    case MA_U8: cc_build<unsigned char, CC_OUT_PARENT>(ctx, (const unsigned char*)src, H, W, mode, conn8, labels, nullptr); break;
    case MA_U16: cc_build<unsigned short, CC_OUT_PARENT>(ctx, (const unsigned short*)src, H, W, mode, conn8, labels, nullptr); break;
    default: cc_build<int, CC_OUT_PARENT>(ctx, (const int*)src, H, W, mode, conn8, labels, nullptr); break;
    }
    hipLaunchKernelGGL((cc_flatten_kernel<false>), dim3((unsigned)nseg), dim3(256), 0, ctx->stream, labels, (unsigned)N,
                       (unsigned*)nullptr, segs);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, segs, nseg);
    hipLaunchKernelGGL(cc_rank_kernel, dim3((unsigned)nseg), dim3(256), 0, ctx->stream, labels, (unsigned)N, segs, rank);
    hipLaunchKernelGGL(cc_relabel_kernel, dim3(cc_blocks(N, 256)), dim3(256), 0, ctx->stream, labels, (unsigned)N, rank);
    int rc = cc_launch_check("ma_cc_label");
    if (rc == MA_OK) {
        hipError_t e = hipMemcpyAsync(ctx->pinned, segs + nseg, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            ma_set_error("reading the count of ma_cc_label failed: %s", hipGetErrorString(e));
            rc = MA_EHIP;
        } else {
            *count = *(const int*)ctx->pinned;
        }
    }
    // stream-ordered reuse: the next call on this ctx that takes the buffer runs behind the kernels launched here
    ma_pool_free(ctx, rank);
    return rc;
}

extern "C" int ma_cc_stats(ma_ctx* ctx, const int* labels, int H, int W, long long n, long long* areas, int* bboxes)
{
    MA_REQUIRE(ctx && labels && areas && bboxes, "NULL argument");
    MA_TRY(cc_check_image(ctx, H, W));
    MA_REQUIRE(n >= 0 && n <= (long long)MA_CC_MAX_PIXELS - 1, "n must be in [0, 2^31 - 2]");
    MA_HIP(hipSetDevice(ctx->device));
    const long long rows = n + 1;
    const unsigned nb = (unsigned)std::min<long long>((rows + 255) / 256, 65536);
    hipLaunchKernelGGL(cc_stats_init_kernel, dim3(nb), dim3(256), 0, ctx->stream, rows, (unsigned long long*)areas, bboxes);
    const int ntx = (W + CC_T - 1) / CC_T, nty = (H + CC_T - 1) / CC_T;
    hipLaunchKernelGGL((cc_tile_kernel<int, CC_OUT_STATS>), dim3((unsigned)ntx * (unsigned)nty), dim3(CC_THREADS), 0, ctx->stream,
                       labels, H, W, ntx, CC_KEY_VALUE, 1, (int)n, (int*)nullptr, (unsigned*)nullptr, (unsigned long long*)areas,
                       bboxes);
    hipLaunchKernelGGL(cc_stats_final_kernel, dim3(nb), dim3(256), 0, ctx->stream, rows, (const unsigned long long*)areas, bboxes);
    return cc_launch_check("ma_cc_stats");
}

extern "C" int ma_cc_filter(ma_ctx* ctx, const void* src, int dtype, int H, int W, int flags, long long min_area, long long max_area,
                            long long value, void* dst)
{
    MA_REQUIRE(ctx && src && dst, "NULL argument");
    MA_REQUIRE(cc_dtype_ok(dtype), "dtype must be uint8, uint16 or int32");
    MA_TRY(cc_check_image(ctx, H, W));
    MA_REQUIRE((flags & ~(MA_CC_CONN8 | MA_CC_BY_VALUE | MA_CC_HOLES)) == 0, "unknown flags");
    const bool holes = (flags & MA_CC_HOLES) != 0;
    MA_REQUIRE(!(holes && (flags & MA_CC_BY_VALUE)), "MA_CC_HOLES and MA_CC_BY_VALUE exclude each other");
    MA_REQUIRE(min_area >= 0 && min_area <= MA_CC_MAX_PIXELS && max_area >= 0 && max_area <= MA_CC_MAX_PIXELS,
               "min_area and max_area must be in [0, 2^31 - 1]");
    if (holes) {
        const long long top = dtype == MA_U8 ? 255 : (dtype == MA_U16 ? 65535 : (long long)INT_MAX);
        MA_REQUIRE(value >= 1 && value <= top, "value must be in [1, the largest value of the dtype]");
    }
    const size_t N = (size_t)H * W;
    MA_HIP(hipSetDevice(ctx->device));
    int* parent = (int*)ma_pool_alloc(ctx, 2 * N * sizeof(int));
    if (!parent) return MA_ENOMEM;
    unsigned* area = (unsigned*)(parent + N);
    const int mode = holes ? CC_KEY_HOLES : ((flags & MA_CC_BY_VALUE) ? CC_KEY_VALUE : CC_KEY_FG), conn8 = (flags & MA_CC_CONN8) ? 1 : 0;
    switch (dtype) {
    case MA_U8:
        cc_filter_run<unsigned char>(ctx, (const unsigned char*)src, H, W, mode, conn8, min_area, max_area, value, parent, area,
                                     (unsigned char*)dst);
        break;
    case MA_U16:
        cc_filter_run<unsigned short>(ctx, (const unsigned short*)src, H, W, mode, conn8, min_area, max_area, value, parent, area,
                                      (unsigned short*)dst);
        break;
    default: cc_filter_run<int>(ctx, (const int*)src, H, W, mode, conn8, min_area, max_area, value, parent, area, (int*)dst); break;
    }
    const int rc = cc_launch_check("ma_cc_filter");
    ma_pool_free(ctx, parent);
    return rc;
}
