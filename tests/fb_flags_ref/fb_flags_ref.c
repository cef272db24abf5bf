/*
 * tests/fb_flags_ref/fb_flags_ref.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Plain-C restatement of DESIGN.md appendix F.7 and F.8: the two stages that cv2.calcOpticalFlowFarneback's flags
 * OPTFLOW_FARNEBACK_GAUSSIAN and OPTFLOW_USE_INITIAL_FLOW put in place of the box window and of the zero start.  Every
 * other stage is tests/fb_general_ref's; tests/fb_flags_ref.py composes the level driver from both.
 *   - F.7: taps k[0..m] (m = winsize / 2, sigma = 0.3 m), the separable float Gaussian of the five M planes (vertical pass
 *     first, REPLICATE), the 2x2 solve in double, no 1 / winsize^2 scale;
 *   - F.8: resize(seed, lw x lh, INTER_AREA) * (float)scale of a 2-channel float field: (a) the same size, (b) whole-number
 *     ratios (block sums), (c) per-axis coefficient tables.
 * Compile with -ffp-contract=off (tests/fb_flags_ref.py does).  Parity with cv2 itself is unpinned.
 */
#include <float.h>
#include <math.h>
#include <stdlib.h>

#define FFR_API __attribute__((visibility("default")))

static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* F.7 taps: k[0..winsize/2] */
FFR_API void ffr_taps(int winsize, float *k) {
    const int m = winsize / 2;
    const double sigma = m * 0.3;
    double s = 1.0;
    k[0] = (float)s;
    for (int i = 1; i <= m; i++) {
        float t = (float)exp(-(i * i) / (2 * sigma * sigma));
        k[i] = t;
        s += t * 2;
    }
    s = 1. / s;
    for (int i = 0; i <= m; i++) k[i] = (float)(k[i] * s);
}

/* F.7: M (5 planes, h x w) -> flow (h, w, 2) */
FFR_API int ffr_gauss_solve(const float *M, int w, int h, int winsize, float *flow) {
    const int m = winsize / 2;
    float k[64];
    if (m < 1 || m > 63) return -1;
    ffr_taps(winsize, k);
    size_t pl = (size_t)w * h;
    float *vs = malloc(sizeof(float) * 5 * pl), *hs = malloc(sizeof(float) * 5 * pl);
    if (!vs || !hs) return -1;
    for (int c = 0; c < 5; c++) {
        const float *P = M + c * pl;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                float v = P[(size_t)y * w + x] * k[0];
                for (int i = 1; i <= m; i++)
                    v = v + (P[(size_t)clampi(y + i, 0, h - 1) * w + x] + P[(size_t)clampi(y - i, 0, h - 1) * w + x]) * k[i];
                vs[c * pl + (size_t)y * w + x] = v;
            }
        for (int y = 0; y < h; y++) {
            const float *row = vs + c * pl + (size_t)y * w;
            for (int x = 0; x < w; x++) {
                float g = row[x] * k[0];
                for (int i = 1; i <= m; i++) g = g + k[i] * (row[clampi(x - i, 0, w - 1)] + row[clampi(x + i, 0, w - 1)]);
                hs[c * pl + (size_t)y * w + x] = g;
            }
        }
    }
    for (size_t i = 0; i < pl; i++) {
        double g11 = hs[i], g12 = hs[pl + i], g22 = hs[2 * pl + i], h1 = hs[3 * pl + i], h2 = hs[4 * pl + i];
        double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
        flow[i * 2] = (float)((g11 * h2 - g12 * h1) * idet);
        flow[i * 2 + 1] = (float)((g22 * h1 - g12 * h2) * idet);
    }
    free(vs);
    free(hs);
    return 0;
}

/* F.8 (c): the table of one axis (S source, D destination positions): entries (dst, src, alpha) in order; returns their
 * number, at most S + 2 * D (every source position is a whole cell of one destination at most). */
FFR_API int ffr_area_table(int S, int D, int *di, int *si, float *alpha) {
    const double s = (double)S / D;
    int k = 0;
    for (int d = 0; d < D; d++) {
        double f1 = d * s, f2 = f1 + s, cw = fmin(s, S - f1);
        int s1 = (int)ceil(f1), s2 = (int)floor(f2);
        if (s2 > S - 1) s2 = S - 1;
        if (s1 > s2) s1 = s2;
        if (s1 - f1 > 1e-3) {
            di[k] = d; si[k] = s1 - 1; alpha[k++] = (float)((s1 - f1) / cw);
        }
        for (int q = s1; q < s2; q++) {
            di[k] = d; si[k] = q; alpha[k++] = (float)(1.0 / cw);
        }
        if (f2 - s2 > 1e-3) {
            di[k] = d; si[k] = s2; alpha[k++] = (float)(fmin(fmin(f2 - s2, 1.0), cw) / cw);
        }
    }
    return k;
}

/* F.8: seed (H, W, 2) -> out (lh, lw, 2) = area(seed) * (float)scale; returns the path taken: 0 (a), 1 (b), 2 (c); -1 on
 * failure */
FFR_API int ffr_area_init(const float *seed, int W, int H, int lw, int lh, double scale, float *out) {
    const float fs = (float)scale;
    if (lw == W && lh == H) {
        for (size_t i = 0; i < (size_t)W * H * 2; i++) out[i] = seed[i] * fs;
        return 0;
    }
    const double sx = (double)W / lw, sy = (double)H / lh;
    const int ix = (int)lrint(sx), iy = (int)lrint(sy);
    if (fabs(sx - ix) < DBL_EPSILON && fabs(sy - iy) < DBL_EPSILON) {
        const float inv = 1.f / (ix * iy);
        for (int y = 0; y < lh; y++)
            for (int x = 0; x < lw; x++)
                for (int c = 0; c < 2; c++) {
                    float sum = 0.f;
                    for (int j = 0; j < iy; j++)
                        for (int i = 0; i < ix; i++) sum = sum + seed[((size_t)(y * iy + j) * W + x * ix + i) * 2 + c];
                    out[((size_t)y * lw + x) * 2 + c] = sum * inv * fs;
                }
        return 1;
    }
    const int nx = W + 2 * lw, ny = H + 2 * lh;
    int *xd = malloc(sizeof(int) * nx), *xs = malloc(sizeof(int) * nx), *yd = malloc(sizeof(int) * ny), *ys = malloc(sizeof(int) * ny);
    float *xa = malloc(sizeof(float) * nx), *ya = malloc(sizeof(float) * ny);
    float *buf = malloc(sizeof(float) * 2 * lw), *sum = malloc(sizeof(float) * 2 * lw);
    if (!xd || !xs || !yd || !ys || !xa || !ya || !buf || !sum) return -1;
    const int kx = ffr_area_table(W, lw, xd, xs, xa), ky = ffr_area_table(H, lh, yd, ys, ya);
    for (int e = 0; e < ky;) {
        const int dy = yd[e];
        for (int first = 1; e < ky && yd[e] == dy; e++, first = 0) {
            const float *S = seed + (size_t)ys[e] * W * 2;
            const float beta = ya[e];
            for (int i = 0; i < 2 * lw; i++) buf[i] = 0.f;
            for (int q = 0; q < kx; q++)
                for (int c = 0; c < 2; c++) buf[xd[q] * 2 + c] = buf[xd[q] * 2 + c] + S[xs[q] * 2 + c] * xa[q];
            for (int i = 0; i < 2 * lw; i++) {
                if (first) sum[i] = beta * buf[i];
                else sum[i] = sum[i] + beta * buf[i];
            }
        }
        for (int i = 0; i < 2 * lw; i++) out[(size_t)dy * lw * 2 + i] = sum[i] * fs;
    }
    free(xd); free(xs); free(yd); free(ys); free(xa); free(ya); free(buf); free(sum);
    return 2;
}
