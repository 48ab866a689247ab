/* CPU restatement of cv2.remap with INTER_NEAREST / INTER_LINEAR / INTER_CUBIC / INTER_LANCZOS4 and BORDER_CONSTANT 0,
 * for the generic remap and for the tiled warp of Warper.warp() (include/microaligner_interp.h states the semantics).
 *
 * Written from OpenCV 4.5.5 imgwarp.cpp as remembered: interpolateCubic / interpolateLanczos4, initInterTab1D /
 * initInterTab2D (including the u8 table's sum fix-up), remapNearest, remapBicubic and remapLanczos4 with their two
 * summation paths, the casts of their CastOps.  The linear mode reuses the oracle's bilinear tables and states the
 * tiled window the same way as the other modes.  Compiled with -ffp-contract=off: every product and sum is rounded on
 * its own, as in the SSE2 baseline build. */
#include "ma_oracle.c"

#define MODE_NEAREST 0
#define MODE_LINEAR 1
#define MODE_CUBIC 2
#define MODE_LANCZOS4 4

static float g_cubic1[INTER_TAB_SIZE][4], g_lanczos1[INTER_TAB_SIZE][8];
static float g_cubic_f[INTER_TAB_SIZE * INTER_TAB_SIZE][16], g_lanczos_f[INTER_TAB_SIZE * INTER_TAB_SIZE][64];
static short g_cubic_i[INTER_TAB_SIZE * INTER_TAB_SIZE][16], g_lanczos_i[INTER_TAB_SIZE * INTER_TAB_SIZE][64];
static int g_interp_ready = 0;

static void interpolate_cubic(float x, float* coeffs)
{
    const float A = -0.75f;
    coeffs[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    coeffs[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    coeffs[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    coeffs[3] = 1.f - coeffs[0] - coeffs[1] - coeffs[2];
}

static void interpolate_lanczos4(float x, float* coeffs)
{
    static const double s45 = 0.70710678118654752440084436210485;
    static const double cs[][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
    const double CV_PI = 3.1415926535897932384626433832795;
    float sum = 0;
    double y0 = -(x + 3) * CV_PI * 0.25, s0 = sin(y0), c0 = cos(y0);
    for (int i = 0; i < 8; i++) {
        float y0_ = (x + 3 - i);
        if (fabs(y0_) >= 1e-6f) {
            double y = -y0_ * CV_PI * 0.25;
            coeffs[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
        } else {
            coeffs[i] = 1e30f;   /* x ~ 0: the tap at distance 0 takes (nearly) everything after the normalisation */
        }
        sum += coeffs[i];
    }
    sum = 1.f / sum;
    for (int i = 0; i < 8; i++) coeffs[i] *= sum;
}

/* initInterTab2D for one ksize: float products and the 15-bit table with its sum fix-up */
static void init_tab2d(const float* tab1, int ksize, float* tabf, short* tabi)
{
    for (int i = 0; i < INTER_TAB_SIZE; i++)
        for (int j = 0; j < INTER_TAB_SIZE; j++) {
            float* tab = tabf + (size_t)(i * INTER_TAB_SIZE + j) * ksize * ksize;
            short* itab = tabi + (size_t)(i * INTER_TAB_SIZE + j) * ksize * ksize;
            int isum = 0;
            for (int k1 = 0; k1 < ksize; k1++) {
                float vy = tab1[i * ksize + k1];
                for (int k2 = 0; k2 < ksize; k2++) {
                    float v = vy * tab1[j * ksize + k2];
                    tab[k1 * ksize + k2] = v;
                    isum += itab[k1 * ksize + k2] = sat_short(cv_round_f(v * INTER_REMAP_COEF_SCALE));
                }
            }
            if (isum != INTER_REMAP_COEF_SCALE) {
                int diff = isum - INTER_REMAP_COEF_SCALE;
                int ksize2 = ksize / 2, Mk1 = ksize2, Mk2 = ksize2, mk1 = ksize2, mk2 = ksize2;
                for (int k1 = ksize2; k1 < ksize2 + 2; k1++)
                    for (int k2 = ksize2; k2 < ksize2 + 2; k2++) {
                        if (itab[k1 * ksize + k2] < itab[mk1 * ksize + mk2]) mk1 = k1, mk2 = k2;
                        else if (itab[k1 * ksize + k2] > itab[Mk1 * ksize + Mk2]) Mk1 = k1, Mk2 = k2;
                    }
                if (diff < 0) itab[Mk1 * ksize + Mk2] = (short)(itab[Mk1 * ksize + Mk2] - diff);
                else itab[mk1 * ksize + mk2] = (short)(itab[mk1 * ksize + mk2] - diff);
            }
        }
}

static void init_interp_tabs(void)
{
    if (g_interp_ready) return;
    init_bilinear_tab();
    const float scale = 1.f / INTER_TAB_SIZE;
    for (int i = 0; i < INTER_TAB_SIZE; i++) {
        interpolate_cubic(i * scale, g_cubic1[i]);
        interpolate_lanczos4(i * scale, g_lanczos1[i]);
    }
    init_tab2d(&g_cubic1[0][0], 4, &g_cubic_f[0][0], &g_cubic_i[0][0]);
    init_tab2d(&g_lanczos1[0][0], 8, &g_lanczos_f[0][0], &g_lanczos_i[0][0]);
    g_interp_ready = 1;
}

/* 1-D table (32 x ksize) and 2-D tables (1024 x ksize^2) of a mode; returns ksize (0: unknown mode) */
int orcx_interp_tables(int interp, float* tab1, float* tab2f, short* tab2i)
{
    init_interp_tabs();
    if (interp == MODE_CUBIC) {
        if (tab1) memcpy(tab1, g_cubic1, sizeof(g_cubic1));
        if (tab2f) memcpy(tab2f, g_cubic_f, sizeof(g_cubic_f));
        if (tab2i) memcpy(tab2i, g_cubic_i, sizeof(g_cubic_i));
        return 4;
    }
    if (interp == MODE_LANCZOS4) {
        if (tab1) memcpy(tab1, g_lanczos1, sizeof(g_lanczos1));
        if (tab2f) memcpy(tab2f, g_lanczos_f, sizeof(g_lanczos_f));
        if (tab2i) memcpy(tab2i, g_lanczos_i, sizeof(g_lanczos_i));
        return 8;
    }
    return 0;
}

/* The source of a sample: an SW x SH image whose pixel (x, y) is pixel (ox + x, oy + y) of the (H, W, cn) array `base`,
 * channel c, and 0 where that lies outside the array (the zero padding of a tiled warp's window) */
typedef struct {
    const void* base;
    int dtype, cn, c;
    int SW, SH;
    int ox, oy, W, H;
} Src;

static float src_get(const Src* s, int x, int y)
{
    const int jx = s->ox + x, jy = s->oy + y;
    if (jx < 0 || jx >= s->W || jy < 0 || jy >= s->H) return 0.f;
    const size_t i = ((size_t)jy * s->W + jx) * s->cn + s->c;
    if (s->dtype == ORC_U8) return ((const uint8_t*)s->base)[i];
    if (s->dtype == ORC_U16) return ((const uint16_t*)s->base)[i];
    return ((const float*)s->base)[i];
}

static void put(int dtype, void* dst, size_t i, int iv, float fv)
{
    if (dtype == ORC_U8) ((uint8_t*)dst)[i] = (uint8_t)iv;
    else if (dtype == ORC_U16) ((uint16_t*)dst)[i] = (uint16_t)iv;
    else ((float*)dst)[i] = fv;
}

/* one output element at map (mx, my) into dst[i] */
static void sample(const Src* s, int interp, float mx, float my, void* dst, size_t i)
{
    const int dt = s->dtype;
    if (interp == MODE_NEAREST) {
        int X = sat_short(cv_round_f(mx)), Y = sat_short(cv_round_f(my));
        float v = (X >= 0 && X < s->SW && Y >= 0 && Y < s->SH) ? src_get(s, X, Y) : 0.f;
        put(dt, dst, i, (int)v, v);
        return;
    }
    const int sxq = cv_round_f(mx * INTER_TAB_SIZE), syq = cv_round_f(my * INTER_TAB_SIZE);
    const int a = (syq & (INTER_TAB_SIZE - 1)) * INTER_TAB_SIZE + (sxq & (INTER_TAB_SIZE - 1));
    if (interp == MODE_LINEAR) {
        /* remapBilinear, BORDER_CONSTANT: outside taps read cval, one 4-term sum on both paths */
        const int sx = sat_short(sxq >> INTER_BITS), sy = sat_short(syq >> INTER_BITS);
        if (sx >= s->SW || sx + 1 < 0 || sy >= s->SH || sy + 1 < 0) { put(dt, dst, i, 0, 0.f); return; }
        float v[4];
        for (int k = 0; k < 4; k++) {
            const int x = sx + (k & 1), y = sy + (k >> 1);
            v[k] = (x >= 0 && x < s->SW && y >= 0 && y < s->SH) ? src_get(s, x, y) : 0.f;
        }
        if (dt == ORC_U8) {
            const short* w = g_tab_i[a];
            int acc = (int)v[0] * w[0] + (int)v[1] * w[1] + (int)v[2] * w[2] + (int)v[3] * w[3];
            put(dt, dst, i, clampi((acc + (1 << (INTER_REMAP_COEF_BITS - 1))) >> INTER_REMAP_COEF_BITS, 0, 255), 0.f);
        } else {
            const float* w = g_tab_f[a];
            float acc = v[0] * w[0] + v[1] * w[1] + v[2] * w[2] + v[3] * w[3];
            put(dt, dst, i, dt == ORC_U16 ? clampi(cv_round_f(acc), 0, 65535) : 0, acc);
        }
        return;
    }
    const int N = interp == MODE_CUBIC ? 4 : 8, OFF = interp == MODE_CUBIC ? 1 : 3;
    const int sx = sat_short(sxq >> INTER_BITS) - OFF, sy = sat_short(syq >> INTER_BITS) - OFF;
    if (sx >= s->SW || sx + N <= 0 || sy >= s->SH || sy + N <= 0) { put(dt, dst, i, 0, 0.f); return; }
    const unsigned width1 = (unsigned)(s->SW - N + 1 > 0 ? s->SW - N + 1 : 0);
    const unsigned height1 = (unsigned)(s->SH - N + 1 > 0 ? s->SH - N + 1 : 0);
    const int fast = (unsigned)sx < width1 && (unsigned)sy < height1;
    if (dt == ORC_U8) {
        const short* w = interp == MODE_CUBIC ? g_cubic_i[a] : g_lanczos_i[a];
        int sum = 0;
        for (int k1 = 0; k1 < N; k1++) {
            if (sy + k1 < 0 || sy + k1 >= s->SH) continue;
            for (int k2 = 0; k2 < N; k2++)
                if (sx + k2 >= 0 && sx + k2 < s->SW) sum += ((int)src_get(s, sx + k2, sy + k1) - 0) * w[k1 * N + k2];
        }
        put(dt, dst, i, clampi((sum + (1 << (INTER_REMAP_COEF_BITS - 1))) >> INTER_REMAP_COEF_BITS, 0, 255), 0.f);
        return;
    }
    const float* w = interp == MODE_CUBIC ? g_cubic_f[a] : g_lanczos_f[a];
    float sum;
    if (fast) {
        /* remapBicubic: sum = row 0, then sum += row k; remapLanczos4: sum = 0, then sum += row k */
        sum = 0.f;
        for (int k1 = 0; k1 < N; k1++) {
            float r = src_get(s, sx, sy + k1) * w[k1 * N];
            for (int k2 = 1; k2 < N; k2++) r = r + src_get(s, sx + k2, sy + k1) * w[k1 * N + k2];
            if (N == 4 && k1 == 0) sum = r;
            else sum += r;
        }
    } else {
        const float cv = 0.f;
        sum = cv * 1;
        for (int k1 = 0; k1 < N; k1++) {
            if (sy + k1 < 0 || sy + k1 >= s->SH) continue;
            for (int k2 = 0; k2 < N; k2++)
                if (sx + k2 >= 0 && sx + k2 < s->SW) sum += (src_get(s, sx + k2, sy + k1) - cv) * w[k1 * N + k2];
        }
    }
    put(dt, dst, i, dt == ORC_U16 ? clampi(cv_round_f(sum), 0, 65535) : 0, sum);
}

static int mode_ok(int interp)
{
    return interp == MODE_NEAREST || interp == MODE_LINEAR || interp == MODE_CUBIC || interp == MODE_LANCZOS4;
}

/* cv2.remap(src, map, None, interp): src (sh, sw, cn), map (dh, dw, 2) float32, dst (dh, dw, cn) */
int orcx_remap_interp(const void* src, int dtype, int cn, int sh, int sw, const float* map, int dh, int dw, int interp,
                      void* dst)
{
    if (sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0 || cn < 1 || cn > 4 || !mode_ok(interp)) return ORC_EINVAL;
    if (dtype != ORC_U8 && dtype != ORC_U16 && dtype != ORC_F32) return ORC_EINVAL;
    if (sh >= 32767 || sw >= 32767 || dh >= 32767 || dw >= 32767) return ORC_EINVAL;
    init_interp_tabs();
    #pragma omp parallel for schedule(static)
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++)
            for (int c = 0; c < cn; c++) {
                Src s = {src, dtype, cn, c, sw, sh, 0, 0, sw, sh};
                const float* m = map + ((size_t)y * dw + x) * 2;
                sample(&s, interp, m[0], m[1], dst, ((size_t)y * dw + x) * cn + c);
            }
    return ORC_OK;
}

/* Warper.warp() with interp: windows of tile + 2 * overlap from (tx * tile - overlap, ty * tile - overlap), zero padded,
 * map float32(x_local - flow); the output pixel (x, y) comes from the window of its tile.  rows: the output rows to
 * compute (NULL: all H), out: (nrows, W) -- row r of out is image row rows[r]. */
int orcx_warp_tiled_interp(const void* img, int dtype, int H, int W, const float* flow, int tile, int overlap, int interp,
                           const int* rows, int nrows, void* out)
{
    if (H <= 0 || W <= 0 || tile < 0 || overlap < 0 || !mode_ok(interp)) return ORC_EINVAL;
    if (dtype != ORC_U8 && dtype != ORC_U16 && dtype != ORC_F32) return ORC_EINVAL;
    const int P_h = tile > 0 ? tile + 2 * overlap : H, P_w = tile > 0 ? tile + 2 * overlap : W;
    if (P_h >= 32767 || P_w >= 32767) return ORC_EINVAL;
    if (!rows) nrows = H;
    for (int r = 0; rows && r < nrows; r++)
        if (rows[r] < 0 || rows[r] >= H) return ORC_EINVAL;
    init_interp_tabs();
    #pragma omp parallel for schedule(static)
    for (int r = 0; r < nrows; r++) {
        const int y = rows ? rows[r] : r;
        const int oy = tile > 0 ? (y / tile) * tile - overlap : 0;
        for (int x = 0; x < W; x++) {
            const int ox = tile > 0 ? (x / tile) * tile - overlap : 0;
            const float* f = flow + ((size_t)y * W + x) * 2;
            Src s = {img, dtype, 1, 0, P_w, P_h, ox, oy, W, H};
            /* warper.py:57-59: float32(float64(-flow) + arange) == the correctly rounded x_local - flow */
            sample(&s, interp, (float)(x - ox) - f[0], (float)(y - oy) - f[1], out, (size_t)r * W + x);
        }
    }
    return ORC_OK;
}
