/* CPU restatement of cv2.calcOpticalFlowFarneback with levels > 0 (FarnebackOpticalFlow::calc, CPU path, OpenCV 4.x):
 * the reference the GPU pyramid (ma_farneback_levels) is compared against bit for bit.  Built on top of the oracle
 * (compiled with its flags, -ffp-contract=off), whose static Farneback pieces it reuses unmodified: poly_exp, preblur3,
 * update_matrices, update_flow_gaussian, orc_gaussian_blur_f32_ex, cv_round_d.
 *
 * The rules, as restated here (unpinned against OpenCV until tests/golden/cv2_levels_4.5.5.npz exists):
 *  1. Level clamp: scale = 1; for k in 0..levels-1: scale *= 0.5, stop at the first k with W*scale < 32 or H*scale < 32;
 *     levels = k.  The dropped levels are not an error.
 *  2. For k = levels .. 0, scale = 0.5^k by repeated multiplication in double:
 *     sigma = (1/scale - 1) * 0.5, ksize = max(cvRound(5 sigma) | 1, 3)   (k = 1..4: 3, 9, 19, 39);
 *     w_k = cvRound(W scale), h_k = cvRound(H scale)                        (cvRound: half to even);
 *     initial flow: zeros on the coarsest level, else resize(flow_{k+1}, (w_k, h_k), INTER_LINEAR) * 2, where the
 *     scaling is convertTo's x * 2 + 0;
 *     each image: convertTo(CV_32F), GaussianBlur(ksize, sigma) on the FULL-resolution image (reflect-101; the row
 *     filter accumulates left to right, the column filter symmetrically), resize to (w_k, h_k), FarnebackPolyExp with
 *     no further pre-blur.  At k = 0 the blur is the fixed [1/4 1/2 1/4] pre-blur of the single-scale oracle (preblur3)
 *     and the resize is the identity;
 *     FarnebackUpdateMatrices(R0, R1, flow), then `iterations` UpdateFlow_GaussianBlur, the matrices not rebuilt
 *     after the last one (update_flow_gaussian).
 *  3. cv::resize INTER_LINEAR on float data (resize_linear_f32):
 *     - both inverse scales exactly 2 (an even-sized level 1): the INTER_AREA fast path, the 2x2 mean summed as
 *       ((s00 + s01) + (s10 + s11)) * 0.25f;
 *     - otherwise the generic path with half-pixel centres, scale = 1 / (dsize / ssize) in double:
 *       f = (float)((d + 0.5) * scale - 0.5), s = cvFloor(f), f -= s, weights (1 - f, f) in float.
 *       Columns: s < 0 -> s = 0, f = 0; from the first dx with s + 1 >= sw on the value is S[sw - 1] alone.
 *       Rows: weights kept, both source rows clamped into [0, sh).
 *       Horizontal pass per source row: h = S[s] * a0 + S[s + 1] * a1 (multiply, multiply, add).
 *       Vertical pass: muladd(h0, b0, h1 * b1) -- v_muladd, an FMA in the fused model.
 *  The rounding model `fused` (MA_FB_MULADD_FUSED) applies to the window blur (as in the oracle), to both passes of
 *  the level GaussianBlur (as orc_gaussian_blur_f32_ex) and to the vertical resize pass. */
#include "ma_oracle.c"

#define ORCX_MIN_SIZE 32

/* Level table: returns the number of levels kept (<= levels); w, h, ksize, sigma of levels 0..returned value. */
int orcx_level_table(int H, int W, int levels, int* w, int* h, int* ksize, double* sigma)
{
    const double pyr_scale = 0.5;
    int k;
    double scale = 1;
    for (k = 0; k < levels; k++) {
        scale *= pyr_scale;
        if (W * scale < ORCX_MIN_SIZE || H * scale < ORCX_MIN_SIZE) break;
    }
    levels = k;
    for (k = 0; k <= levels; k++) {
        double s = 1;
        for (int i = 0; i < k; i++) s *= pyr_scale;
        const double sg = (1. / s - 1) * 0.5;
        int ks = cv_round_d(sg * 5) | 1;
        if (ks < 3) ks = 3;
        if (w) w[k] = cv_round_d(W * s);
        if (h) h[k] = cv_round_d(H * s);
        if (ksize) ksize[k] = ks;
        if (sigma) sigma[k] = sg;
    }
    return levels;
}

/* cv::resize(src, dst, (dw, dh), 0, 0, INTER_LINEAR) of an interleaved float image with cn channels (rule 3). */
int orcx_resize_linear_f32(const float* src, int cn, int sh, int sw, float* dst, int dh, int dw, int fused)
{
    if (sh <= 0 || sw <= 0 || dh <= 0 || dw <= 0 || cn < 1) return ORC_EINVAL;
    if (sh == dh && sw == dw) {
        memcpy(dst, src, sizeof(float) * (size_t)sh * sw * cn);
        return ORC_OK;
    }
    if (sw == 2 * dw && sh == 2 * dh) {
        for (int dy = 0; dy < dh; dy++)
            for (int dx = 0; dx < dw; dx++)
                for (int c = 0; c < cn; c++) {
                    const float* s0 = src + ((size_t)(2 * dy) * sw + 2 * dx) * cn + c;
                    const float* s1 = s0 + (size_t)sw * cn;
                    dst[((size_t)dy * dw + dx) * cn + c] = ((s0[0] + s0[cn]) + (s1[0] + s1[cn])) * 0.25f;
                }
        return ORC_OK;
    }
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    int* xs = (int*)malloc(sizeof(int) * dw);
    float* xa = (float*)malloc(sizeof(float) * dw * 2);
    int* xtail = (int*)malloc(sizeof(int) * dw);
    if (!xs || !xa || !xtail) { free(xs); free(xa); free(xtail); return ORC_ENOMEM; }
    for (int dx = 0; dx < dw; dx++) {
        float f = (float)((dx + 0.5) * scale_x - 0.5);
        int s = cv_floor_f(f);
        f -= s;
        if (s < 0) { s = 0; f = 0.f; }
        xtail[dx] = s + 1 >= sw;
        if (xtail[dx]) { s = sw - 1; f = 0.f; }
        xs[dx] = s;
        xa[dx * 2] = 1.f - f;
        xa[dx * 2 + 1] = f;
    }
    for (int dy = 0; dy < dh; dy++) {
        float f = (float)((dy + 0.5) * scale_y - 0.5);
        const int s = cv_floor_f(f);
        f -= s;
        const float b0 = 1.f - f, b1 = f;
        const float* r0 = src + (size_t)clampi(s, 0, sh - 1) * sw * cn;
        const float* r1 = src + (size_t)clampi(s + 1, 0, sh - 1) * sw * cn;
        for (int dx = 0; dx < dw; dx++)
            for (int c = 0; c < cn; c++) {
                const size_t i0 = (size_t)xs[dx] * cn + c, i1 = i0 + cn;
                float h0, h1;
                if (xtail[dx]) {
                    h0 = r0[i0];
                    h1 = r1[i0];
                } else {
                    h0 = r0[i0] * xa[dx * 2] + r0[i1] * xa[dx * 2 + 1];
                    h1 = r1[i0] * xa[dx * 2] + r1[i1] * xa[dx * 2 + 1];
                }
                dst[((size_t)dy * dw + dx) * cn + c] = muladd_f(h0, b0, h1 * b1, fused);
            }
    }
    free(xs); free(xa); free(xtail);
    return ORC_OK;
}

/* cv2.calcOpticalFlowFarneback(prev, next, None, 0.5, levels, winsize, iters, poly_n, poly_sigma, GAUSSIAN).
 * prev/next: dtype u8/u16/f32, h x w contiguous.  flow_out: h*w*2 float. */
int orcx_farneback_levels(const void* prev, const void* next, int dtype, int h, int w, int levels, int winsize,
                          int iters, int poly_n, double poly_sigma, int fused, float* flow_out)
{
    if (h <= 0 || w <= 0 || levels < 0 || iters < 0 || poly_n < 1 || winsize < 1) return ORC_EINVAL;
    int lw[64], lh[64], lk[64];
    double ls[64];
    if (levels > 62) levels = 62;  /* the 32-px clamp keeps at most 26 levels of a 2^31-px side */
    levels = orcx_level_table(h, w, levels, lw, lh, lk, ls);
    if (levels == 0)
        return orc_farneback(prev, next, dtype, h, w, winsize, iters, poly_n, poly_sigma, fused, flow_out, NULL, NULL, NULL);
    const size_t npx = (size_t)h * w;
    float* fimg = (float*)malloc(sizeof(float) * npx);
    float* blur = (float*)malloc(sizeof(float) * npx);
    float* tmp = (float*)malloc(sizeof(float) * npx);
    float* R[2];
    R[0] = (float*)malloc(sizeof(float) * npx * 5);
    R[1] = (float*)malloc(sizeof(float) * npx * 5);
    float* M = (float*)malloc(sizeof(float) * npx * 5);
    float* flow = (float*)malloc(sizeof(float) * npx * 2);
    float* prevflow = (float*)malloc(sizeof(float) * npx * 2);
    const void* img[2] = { prev, next };
    int rc = ORC_OK;
    if (!fimg || !blur || !tmp || !R[0] || !R[1] || !M || !flow || !prevflow) { rc = ORC_ENOMEM; goto done; }
    for (int k = levels; k >= 0; k--) {
        const int wk = lw[k], hk = lh[k];
        const size_t n = (size_t)wk * hk;
        if (k == levels) {
            memset(flow, 0, sizeof(float) * n * 2);
        } else {
            rc = orcx_resize_linear_f32(prevflow, 2, lh[k + 1], lw[k + 1], flow, hk, wk, fused);
            if (rc) goto done;
            for (size_t i = 0; i < n * 2; i++) flow[i] = flow[i] * 2.f + 0.f;
        }
        for (int i = 0; i < 2; i++) {
            for (size_t p = 0; p < npx; p++) fimg[p] = load_as_f32(img[i], dtype, p);
            if (k == 0) {
                preblur3(fimg, blur, h, w, tmp);
            } else {
                rc = orc_gaussian_blur_f32_ex(fimg, h, w, lk[k], ls[k], fused, tmp);
                if (rc) goto done;
                rc = orcx_resize_linear_f32(tmp, 1, h, w, blur, hk, wk, fused);
                if (rc) goto done;
            }
            rc = poly_exp(blur, R[i], hk, wk, poly_n, poly_sigma);
            if (rc) goto done;
        }
        update_matrices(R[0], R[1], flow, M, hk, wk, 0, hk);
        for (int i = 0; i < iters; i++) {
            rc = update_flow_gaussian(R[0], R[1], flow, M, hk, wk, winsize, i < iters - 1, fused);
            if (rc) goto done;
        }
        memcpy(prevflow, flow, sizeof(float) * n * 2);
    }
    memcpy(flow_out, flow, sizeof(float) * npx * 2);
done:
    free(fimg); free(blur); free(tmp); free(R[0]); free(R[1]); free(M); free(flow); free(prevflow);
    return rc;
}
