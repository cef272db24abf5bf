/*
 * tests/fb_general_ref/fb_general_ref.c -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Plain-C restatement of DESIGN.md appendix F: Farneback with the six numeric parameters of
 * cv2.calcOpticalFlowFarneback made parameters of the call.  At the reference's values (0.5, 3, 15, 3, 5, 1.2, 0) every
 * operation and every summation order is that of oracle/farneback_oracle.c (flags == 0), so the two agree bit for bit;
 * elsewhere the orders are the oracle's generalised as appendix F states:
 *   - pyr_scale and poly_sigma arrive as float and are widened to the double of their shortest decimal form (F.0);
 *   - level k: scale = pyr_scale^k by repeated multiplication, sigma = (1/scale - 1) / 2,
 *     ksize = max(cvRound(5 sigma) | 1, 3), the fixed 3-tap table at sigma = 0 (F.1, F.2);
 *   - the Gaussian is the symmetric form k[r]*c + sum_j k[r+j]*(x[-j]+x[+j]) in float, rows then columns, REFLECT_101;
 *     INTER_LINEAR through the oracle's coordinate tables at every scale (F.2);
 *   - PolyExp with n = poly_n: the oracle's loops with n as their bound (F.3);
 *   - the (2m+1)^2 box, m = winsize/2: blocks of L = 2m+2 positions anchored at L*j - (m+1); the window of position
 *     L*j + t is (suffix of block j from t, summed from its end) + (prefix of block j+1 up to t-1, summed from its
 *     start).  L = 16 and m = 7 are the oracle's box15_block16 (F.5).
 * Compile with -ffp-contract=off (tests/fb_general_ref.py does).  Parity with cv2 itself is unpinned.
 * Layouts as the oracle: images row-major, R and M 5 planes, flow interleaved (h, w, 2).
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define FBR_API __attribute__((visibility("default")))
#define MIN_SIZE 32
#define MAX_POLY_N 7
#define MAX_KSIZE 191  /* the largest level Gaussian (F.2); larger ones are refused */

typedef struct {
    float pyr_scale;
    int levels, winsize, iterations, poly_n;
    float poly_sigma;
    int flags;
} fbr_params;

static inline int cv_round(double v) { return (int)lrint(v); }
static inline int cv_floorf(float v) { return (int)floorf(v); }
static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static inline int reflect101(int p, int n) {
    if (n == 1) return 0;
    while (p < 0 || p >= n) {
        if (p < 0) p = -p;
        else p = 2 * (n - 1) - p;
    }
    return p;
}

/* F.0: the double a caller meant by a float parameter -- the shortest decimal that reads back as the same float */
FBR_API double fbr_widen(float f) {
    char buf[32];
    for (int d = 1; d <= 9; d++) {
        snprintf(buf, sizeof buf, "%.*g", d, (double)f);
        double v = strtod(buf, 0);
        if ((float)v == f) return v;
    }
    return (double)f;
}

/* F.1 parameter rules; 0 or a message */
FBR_API const char *fbr_check(const fbr_params *p) {
    if (!p) return "params is NULL";
    if (!(p->pyr_scale > 0.f && p->pyr_scale < 1.f)) return "pyr_scale must be in (0, 1)";
    if (p->levels < 0 || p->levels > 12) return "levels must be 0..12";
    if (p->winsize < 3 || p->winsize > 63 || !(p->winsize & 1)) return "winsize must be odd, 3..63";
    if (p->iterations < 1 || p->iterations > 10) return "iterations must be 1..10";
    if (p->poly_n != 5 && p->poly_n != 7) return "poly_n must be 5 or 7";
    if (!(p->poly_sigma > 0.f && p->poly_sigma <= 3.f)) return "poly_sigma must be in (0, 3]";
    if (p->flags & 4) return "OPTFLOW_USE_INITIAL_FLOW is not supported";
    if (p->flags & 256) return "OPTFLOW_FARNEBACK_GAUSSIAN is not supported";
    if (p->flags) return "flags must be 0";
    return 0;
}

FBR_API int fbr_num_levels(int w, int h, const fbr_params *p) {
    const double ps = fbr_widen(p->pyr_scale);
    double scale = 1.0;
    int k;
    for (k = 0; k < p->levels; k++) {
        scale *= ps;
        if (w * scale < MIN_SIZE || h * scale < MIN_SIZE) break;
    }
    return k;
}

FBR_API void fbr_level_params(int w, int h, const fbr_params *p, int k, int *lw, int *lh, double *sigma, int *ksize) {
    const double ps = fbr_widen(p->pyr_scale);
    double scale = 1.0;
    for (int i = 0; i < k; i++) scale *= ps;
    double s = (1.0 / scale - 1.0) * 0.5;
    int sm = cv_round(s * 5) | 1;
    if (sm < 3) sm = 3;
    *lw = cv_round(w * scale);
    *lh = cv_round(h * scale);
    *sigma = s;
    *ksize = sm;
}

/* 0 when the parameters are valid and every level's Gaussian fits MAX_KSIZE; *n_scales = levels actually used + 1 */
FBR_API int fbr_geometry(int w, int h, const fbr_params *p, int *n_scales) {
    if (fbr_check(p) || w < 16 || h < 16) return 1;
    const int nl = fbr_num_levels(w, h, p);
    for (int k = 0; k <= nl; k++) {
        int lw, lh, ks;
        double s;
        fbr_level_params(w, h, p, k, &lw, &lh, &s, &ks);
        if (ks > MAX_KSIZE) return 1;
    }
    *n_scales = nl + 1;
    return 0;
}

FBR_API void fbr_gaussian_kernel(int n, double sigma, float *out) {
    static const float tab1[] = {1.f};
    static const float tab3[] = {0.25f, 0.5f, 0.25f};
    static const float tab5[] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    static const float tab7[] = {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f};
    const float *fixed = 0;
    if (sigma <= 0 && (n & 1) && n <= 7) fixed = n == 1 ? tab1 : n == 3 ? tab3 : n == 5 ? tab5 : tab7;
    double sg = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    double scale2x = -0.5 / (sg * sg);
    double sum = 0;
    for (int i = 0; i < n; i++) {
        double x = i - (n - 1) * 0.5;
        double t = fixed ? (double)fixed[i] : exp(scale2x * x * x);
        out[i] = (float)t;
        sum += out[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < n; i++) out[i] = (float)(out[i] * sum);
}

static void resize_table(int src, int dst, int *i0, int *i1, float *f) {
    double scale = (double)src / dst;
    for (int d = 0; d < dst; d++) {
        float fx = (float)((d + 0.5) * scale - 0.5);
        int sx = cv_floorf(fx);
        fx -= sx;
        if (sx < 0) { sx = 0; fx = 0.f; }
        if (sx >= src - 1) { sx = src - 1; fx = 0.f; }
        i0[d] = sx;
        i1[d] = sx + 1 < src ? sx + 1 : src - 1;
        f[d] = fx;
    }
}

/* F.2: level k of an 8-bit frame -> I (lh x lw) */
FBR_API int fbr_pyr_level(const uint8_t *img, int w, int h, const fbr_params *p, int k, float *I) {
    int lw, lh, ks;
    double sigma;
    fbr_level_params(w, h, p, k, &lw, &lh, &sigma, &ks);
    if (ks > MAX_KSIZE) return -1;
    const int r = ks / 2;
    float kern[MAX_KSIZE];
    fbr_gaussian_kernel(ks, sigma, kern);
    float *tmp = malloc(sizeof(float) * (size_t)w * h), *blur = malloc(sizeof(float) * (size_t)w * h);
    int *x0 = malloc(sizeof(int) * lw), *x1 = malloc(sizeof(int) * lw), *y0 = malloc(sizeof(int) * lh),
        *y1 = malloc(sizeof(int) * lh);
    float *fx = malloc(sizeof(float) * lw), *fy = malloc(sizeof(float) * lh);
    if (!tmp || !blur || !x0 || !x1 || !y0 || !y1 || !fx || !fy) return -1;
    for (int y = 0; y < h; y++) {
        const uint8_t *s = img + (size_t)y * w;
        for (int x = 0; x < w; x++) {
            float acc = kern[r] * (float)s[x];
            for (int j = 1; j <= r; j++) {
                float a = (float)s[reflect101(x - j, w)];
                float b = (float)s[reflect101(x + j, w)];
                acc = acc + kern[r + j] * (a + b);
            }
            tmp[(size_t)y * w + x] = acc;
        }
    }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float acc = kern[r] * tmp[(size_t)y * w + x];
            for (int j = 1; j <= r; j++) {
                float a = tmp[(size_t)reflect101(y - j, h) * w + x];
                float b = tmp[(size_t)reflect101(y + j, h) * w + x];
                acc = acc + kern[r + j] * (a + b);
            }
            blur[(size_t)y * w + x] = acc;
        }
    resize_table(w, lw, x0, x1, fx);
    resize_table(h, lh, y0, y1, fy);
    for (int y = 0; y < lh; y++) {
        const float *r0 = blur + (size_t)y0[y] * w, *r1 = blur + (size_t)y1[y] * w;
        float b1 = fy[y], b0 = 1.f - b1;
        for (int x = 0; x < lw; x++) {
            float a1 = fx[x], a0 = 1.f - a1;
            float t0 = r0[x0[x]] * a0 + r0[x1[x]] * a1;
            float t1 = r1[x0[x]] * a0 + r1[x1[x]] * a1;
            I[(size_t)y * lw + x] = t0 * b0 + t1 * b1;
        }
    }
    free(tmp); free(blur); free(x0); free(x1); free(y0); free(y1); free(fx); free(fy);
    return 0;
}

/* F.3 FarnebackPrepareGaussian(n, sigma): g, xg, xxg of n+1 floats; ig = {ig11, ig03, ig33, ig55} */
FBR_API void fbr_polyexp_prepare(int n, double sigma, float *g, float *xg, float *xxg, double *ig) {
    float gg[2 * MAX_POLY_N + 1];
    double s = 0;
    for (int x = -n; x <= n; x++) {
        gg[x + n] = (float)exp(-x * x / (2 * sigma * sigma));
        s += gg[x + n];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) gg[x + n] = (float)(gg[x + n] * s);
    for (int x = 0; x <= n; x++) {
        g[x] = gg[x + n];
        xg[x] = (float)(x * gg[x + n]);
        xxg[x] = (float)(x * x * gg[x + n]);
    }
    double G[6][6];
    memset(G, 0, sizeof(G));
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            float pp = gg[y + n] * gg[x + n];
            G[0][0] += pp;
            G[1][1] += pp * x * x;
            G[3][3] += pp * x * x * x * x;
            G[5][5] += pp * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    double A[6][12];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 12; j++) A[i][j] = j < 6 ? G[i][j] : (j - 6 == i ? 1.0 : 0.0);
    for (int c = 0; c < 6; c++) {
        int pv = c;
        for (int r = c + 1; r < 6; r++)
            if (fabs(A[r][c]) > fabs(A[pv][c])) pv = r;
        if (pv != c)
            for (int j = 0; j < 12; j++) { double t = A[c][j]; A[c][j] = A[pv][j]; A[pv][j] = t; }
        double d = 1.0 / A[c][c];
        for (int j = 0; j < 12; j++) A[c][j] *= d;
        for (int r = 0; r < 6; r++)
            if (r != c) {
                double f = A[r][c];
                if (f != 0)
                    for (int j = 0; j < 12; j++) A[r][j] -= f * A[c][j];
            }
    }
    ig[0] = A[1][7];
    ig[1] = A[0][9];
    ig[2] = A[3][9];
    ig[3] = A[5][11];
}

/* F.3 FarnebackPolyExp: I (h, w) -> R 5 planes; f32 vertical part, f64 horizontal accumulators */
FBR_API int fbr_polyexp(const float *I, int w, int h, int n, double sigma, float *R) {
    float g[MAX_POLY_N + 1], xg[MAX_POLY_N + 1], xxg[MAX_POLY_N + 1];
    double ig[4];
    fbr_polyexp_prepare(n, sigma, g, xg, xxg, ig);
    const double ig11 = ig[0], ig03 = ig[1], ig33 = ig[2], ig55 = ig[3];
    size_t plane = (size_t)w * h;
    float *row = malloc(sizeof(float) * 3 * (size_t)w);
    if (!row) return -1;
    for (int y = 0; y < h; y++) {
        const float *s0 = I + (size_t)y * w;
        for (int x = 0; x < w; x++) {
            row[x * 3] = s0[x] * g[0];
            row[x * 3 + 1] = row[x * 3 + 2] = 0.f;
        }
        for (int k = 1; k <= n; k++) {
            const float *a = I + (size_t)(y - k < 0 ? 0 : y - k) * w;
            const float *b = I + (size_t)(y + k > h - 1 ? h - 1 : y + k) * w;
            for (int x = 0; x < w; x++) {
                float pp = a[x] + b[x];
                float t0 = row[x * 3] + g[k] * pp;
                float t1 = row[x * 3 + 1] + xg[k] * (b[x] - a[x]);
                float t2 = row[x * 3 + 2] + xxg[k] * pp;
                row[x * 3] = t0;
                row[x * 3 + 1] = t1;
                row[x * 3 + 2] = t2;
            }
        }
        for (int x = 0; x < w; x++) {
            float g0 = g[0];
            double b1 = row[x * 3] * g0, b2 = 0, b3 = row[x * 3 + 1] * g0, b4 = 0, b5 = row[x * 3 + 2] * g0, b6 = 0;
            for (int k = 1; k <= n; k++) {
                int pp = x + k > w - 1 ? w - 1 : x + k;
                int m = x - k < 0 ? 0 : x - k;
                double tg = row[pp * 3] + row[m * 3];
                g0 = g[k];
                b1 += tg * g0;
                b4 += tg * xxg[k];
                b2 += (row[pp * 3] - row[m * 3]) * xg[k];
                b3 += (row[pp * 3 + 1] + row[m * 3 + 1]) * g0;
                b6 += (row[pp * 3 + 1] - row[m * 3 + 1]) * xg[k];
                b5 += (row[pp * 3 + 2] + row[m * 3 + 2]) * g0;
            }
            size_t o = (size_t)y * w + x;
            R[0 * plane + o] = (float)(b3 * ig11);
            R[1 * plane + o] = (float)(b2 * ig11);
            R[2 * plane + o] = (float)(b1 * ig03 + b5 * ig33);
            R[3 * plane + o] = (float)(b1 * ig03 + b4 * ig33);
            R[4 * plane + o] = (float)(b6 * ig55);
        }
    }
    free(row);
    return 0;
}

/* F.2 flow upsample: resize(prev, (w, h), INTER_LINEAR) * mul, mul = (float)(1 / pyr_scale) */
FBR_API int fbr_flow_upsample(const float *prev, int pw, int ph, float *flow, int w, int h, float mul) {
    int *x0 = malloc(sizeof(int) * w), *x1 = malloc(sizeof(int) * w), *y0 = malloc(sizeof(int) * h),
        *y1 = malloc(sizeof(int) * h);
    float *fx = malloc(sizeof(float) * w), *fy = malloc(sizeof(float) * h);
    if (!x0 || !x1 || !y0 || !y1 || !fx || !fy) return -1;
    resize_table(pw, w, x0, x1, fx);
    resize_table(ph, h, y0, y1, fy);
    for (int y = 0; y < h; y++) {
        const float *r0 = prev + (size_t)y0[y] * pw * 2, *r1 = prev + (size_t)y1[y] * pw * 2;
        float b1 = fy[y], b0 = 1.f - b1;
        for (int x = 0; x < w; x++) {
            float a1 = fx[x], a0 = 1.f - a1;
            for (int c = 0; c < 2; c++) {
                float t0 = r0[x0[x] * 2 + c] * a0 + r0[x1[x] * 2 + c] * a1;
                float t1 = r1[x0[x] * 2 + c] * a0 + r1[x1[x] * 2 + c] * a1;
                flow[((size_t)y * w + x) * 2 + c] = (t0 * b0 + t1 * b1) * mul;
            }
        }
    }
    free(x0); free(x1); free(y0); free(y1); free(fx); free(fy);
    return 0;
}

/* F.4 FarnebackUpdateMatrices (no parameter enters it) */
FBR_API void fbr_update_matrices(const float *R0, const float *R1, const float *flow, int w, int h, float *M) {
    static const float border[5] = {0.14f, 0.14f, 0.4472f, 0.4472f, 0.4472f};
    const int BORDER = 5;
    size_t pl = (size_t)w * h;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            size_t o = (size_t)y * w + x;
            float dx = flow[o * 2], dy = flow[o * 2 + 1];
            float fx = x + dx, fy = y + dy;
            int x1 = cv_floorf(fx), y1 = cv_floorf(fy);
            float r2, r3, r4, r5, r6;
            fx -= x1;
            fy -= y1;
            if ((unsigned)x1 < (unsigned)(w - 1) && (unsigned)y1 < (unsigned)(h - 1)) {
                float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
                size_t q = (size_t)y1 * w + x1;
#define BIL(c) (a00 * R1[(c)*pl + q] + a01 * R1[(c)*pl + q + 1] + a10 * R1[(c)*pl + q + w] + a11 * R1[(c)*pl + q + w + 1])
                r2 = BIL(0);
                r3 = BIL(1);
                r4 = BIL(2);
                r5 = BIL(3);
                r6 = BIL(4);
#undef BIL
                r4 = (R0[2 * pl + o] + r4) * 0.5f;
                r5 = (R0[3 * pl + o] + r5) * 0.5f;
                r6 = (R0[4 * pl + o] + r6) * 0.25f;
            } else {
                r2 = r3 = 0.f;
                r4 = R0[2 * pl + o];
                r5 = R0[3 * pl + o];
                r6 = R0[4 * pl + o] * 0.5f;
            }
            r2 = (R0[0 * pl + o] - r2) * 0.5f;
            r3 = (R0[1 * pl + o] - r3) * 0.5f;
            r2 += r4 * dy + r6 * dx;
            r3 += r6 * dy + r5 * dx;
            if ((unsigned)(x - BORDER) >= (unsigned)(w - BORDER * 2) || (unsigned)(y - BORDER) >= (unsigned)(h - BORDER * 2)) {
                float scale = (x < BORDER ? border[x] : 1.f) * (x >= w - BORDER ? border[w - x - 1] : 1.f) *
                              (y < BORDER ? border[y] : 1.f) * (y >= h - BORDER ? border[h - y - 1] : 1.f);
                r2 *= scale; r3 *= scale; r4 *= scale; r5 *= scale; r6 *= scale;
            }
            M[0 * pl + o] = r4 * r4 + r6 * r6;
            M[1 * pl + o] = (r4 + r5) * r6;
            M[2 * pl + o] = r5 * r5 + r6 * r6;
            M[3 * pl + o] = r4 * r2 + r6 * r3;
            M[4 * pl + o] = r6 * r2 + r5 * r3;
        }
}

/* F.5 window sums of one block: v[0 .. 4m+1] = positions L*j - m .. L*j + 3m + 1 (L = 2m+2), out[t] = window of L*j + t.
 * Suffix s[t] = v[t] + s[t+1] (s[2m] = v[2m]); prefix p = v[2m+1] + v[2m+2] + ... left to right. */
static void box_block(const double *v, int m, double *out) {
    double s[64];
    s[2 * m] = v[2 * m];
    for (int j = 2 * m - 1; j >= 0; j--) s[j] = v[j] + s[j + 1];
    double p = v[2 * m + 1];
    out[0] = s[0];
    for (int t = 1; t <= 2 * m; t++) {
        out[t] = s[t] + p;
        p = p + v[2 * m + 1 + t];
    }
    out[2 * m + 1] = p;
}

/* F.5 (2m+1)^2 box (REPLICATE, double, columns first) + the 2x2 solve */
FBR_API int fbr_blur_solve(const float *M, int w, int h, int winsize, float *flow) {
    const int m = winsize / 2, L = 2 * m + 2;
    const double scale = 1. / (winsize * winsize);
    size_t pl = (size_t)w * h;
    double *vs = malloc(sizeof(double) * 5 * pl);
    if (!vs) return -1;
    double v[128], o[64];
    for (int c = 0; c < 5; c++)
        for (int x = 0; x < w; x++)
            for (int yb = 0; yb < h; yb += L) {
                for (int j = 0; j < 4 * m + 2; j++) v[j] = (double)M[c * pl + (size_t)clampi(yb - m + j, 0, h - 1) * w + x];
                box_block(v, m, o);
                for (int t = 0; t < L && yb + t < h; t++) vs[c * pl + (size_t)(yb + t) * w + x] = o[t];
            }
    double *hs = malloc(sizeof(double) * 5 * pl);
    if (!hs) return -1;
    for (int c = 0; c < 5; c++)
        for (int y = 0; y < h; y++)
            for (int xb = 0; xb < w; xb += L) {
                for (int j = 0; j < 4 * m + 2; j++) v[j] = vs[c * pl + (size_t)y * w + clampi(xb - m + j, 0, w - 1)];
                box_block(v, m, o);
                for (int t = 0; t < L && xb + t < w; t++) hs[c * pl + (size_t)y * w + xb + t] = o[t];
            }
    for (size_t i = 0; i < pl; i++) {
        double g11 = hs[i] * scale, g12 = hs[pl + i] * scale, g22 = hs[2 * pl + i] * scale, h1 = hs[3 * pl + i] * scale,
               h2 = hs[4 * pl + i] * scale;
        double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
        flow[i * 2] = (float)((g11 * h2 - g12 * h1) * idet);
        flow[i * 2 + 1] = (float)((g22 * h1 - g12 * h2) * idet);
    }
    free(vs);
    free(hs);
    return 0;
}

/* F.1 driver.  dump_level >= 0: level dump_level's I0, I1 (lh*lw), R0, R1 (5 planes), and M and the flow as they stand
 * before blur iteration dump_iter (dump_iter >= iterations: end of the level); NULL pointers are skipped. */
FBR_API int fbr_flow(const uint8_t *prev, const uint8_t *next, int w, int h, const fbr_params *p, float *flow_out,
                     int dump_level, int dump_iter, float *dI0, float *dI1, float *dR0, float *dR1, float *dM, float *dflow) {
    int ns;
    if (fbr_geometry(w, h, p, &ns)) return -2;
    const int levels = ns - 1;
    const double sig = fbr_widen(p->poly_sigma);
    const float mul = (float)(1.0 / fbr_widen(p->pyr_scale));
    size_t N = (size_t)w * h;
    float *I = malloc(sizeof(float) * N), *R0 = malloc(sizeof(float) * 5 * N), *R1 = malloc(sizeof(float) * 5 * N);
    float *M = malloc(sizeof(float) * 5 * N), *flow = malloc(sizeof(float) * 2 * N), *prevflow = malloc(sizeof(float) * 2 * N);
    if (!I || !R0 || !R1 || !M || !flow || !prevflow) return -1;
    int pw = 0, ph = 0, rc = 0;
    for (int k = levels; k >= 0; k--) {
        int lw, lh, ks;
        double sigma;
        fbr_level_params(w, h, p, k, &lw, &lh, &sigma, &ks);
        size_t n = (size_t)lw * lh;
        if (pw == 0) memset(flow, 0, sizeof(float) * 2 * n);
        else rc |= fbr_flow_upsample(prevflow, pw, ph, flow, lw, lh, mul);
        rc |= fbr_pyr_level(prev, w, h, p, k, I);
        if (k == dump_level && dI0) memcpy(dI0, I, sizeof(float) * n);
        rc |= fbr_polyexp(I, lw, lh, p->poly_n, sig, R0);
        rc |= fbr_pyr_level(next, w, h, p, k, I);
        if (k == dump_level && dI1) memcpy(dI1, I, sizeof(float) * n);
        rc |= fbr_polyexp(I, lw, lh, p->poly_n, sig, R1);
        if (rc) return -1;
        if (k == dump_level && dR0) memcpy(dR0, R0, sizeof(float) * 5 * n);
        if (k == dump_level && dR1) memcpy(dR1, R1, sizeof(float) * 5 * n);
        fbr_update_matrices(R0, R1, flow, lw, lh, M);
        int dumped = 0;
        for (int it = 0; it < p->iterations; it++) {
            if (k == dump_level && it == dump_iter) {
                if (dM) memcpy(dM, M, sizeof(float) * 5 * n);
                if (dflow) memcpy(dflow, flow, sizeof(float) * 2 * n);
                dumped = 1;
            }
            if (fbr_blur_solve(M, lw, lh, p->winsize, flow)) return -1;
            if (it < p->iterations - 1) fbr_update_matrices(R0, R1, flow, lw, lh, M);
        }
        if (k == dump_level && !dumped) {
            if (dM) memcpy(dM, M, sizeof(float) * 5 * n);
            if (dflow) memcpy(dflow, flow, sizeof(float) * 2 * n);
        }
        memcpy(prevflow, flow, sizeof(float) * 2 * n);
        pw = lw;
        ph = lh;
    }
    memcpy(flow_out, flow, sizeof(float) * 2 * N);
    free(I); free(R0); free(R1); free(M); free(flow); free(prevflow);
    return 0;
}
