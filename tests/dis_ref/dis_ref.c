/*
 * dis_ref.c -- plain-C restatement of the DIS optical-flow path (DESIGN.md "DIS path", appendix D).
 *
 * Test-only: tests/dis_ref.py builds it with `cc -O2 -ffp-contract=off -fno-fast-math -shared` and loads it
 * through ctypes.  The product (funscript_flow_amd/csrc/kernels_dis.hip) restates the same rules for gfx950 and
 * must agree with this file bit for bit, so every floating-point expression below is written in the order the
 * kernels evaluate it, and every sum over the 64 pixels of a patch uses the butterfly tree of wave_sum().
 * Rule numbers (D1 ...) refer to the appendix.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int finest_scale, patch_size, patch_stride, grad_descent_iters, var_refine_iters;
    float vr_alpha, vr_gamma, vr_delta;
    int use_mean_norm, use_spatial_prop, stripes;
} dis_params;

#define PS 8          /* D1: patch size (the only one accepted) */
#define NPIX 64       /* pixels per patch = lanes per wave */
#define DET_EPS 0.001f
#define VR_ZETA2 0.01f   /* zeta^2, zeta = 0.1 */
#define VR_EPS2 1e-6f    /* eps^2,  eps = 0.001 */
#define VR_OMEGA 1.6f
#define VR_SOR 5

static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* D2: geometry; 0 = supported, 1 = refused */
int dis_geometry(int w, int h, const dis_params *p, int *coarsest, int *finest) {
    if (!p || w < 1 || h < 1) return 1;
    if (p->patch_size != PS || p->patch_stride < 1 || p->patch_stride > PS || p->finest_scale < 0 ||
        p->grad_descent_iters < 1 || p->var_refine_iters < 0 || p->stripes < 0)
        return 1;
    int mx = w > h ? w : h, mn = w < h ? w : h;
    int a = (int)(log2((double)mx / (4.0 * PS)) + 0.5), b = (int)log2((double)mn / PS);
    int c = a < b ? a : b;
    if (c < p->finest_scale || c - p->finest_scale + 1 > 12) return 1;
    if ((w % (1 << c)) || (h % (1 << c))) return 1;
    long pyr = 0;
    for (int s = p->finest_scale; s <= c; s++) {
        int lw = w >> s, lh = h >> s;
        if (lw < PS || lh < PS || (lw - PS) % p->patch_stride || (lh - PS) % p->patch_stride) return 1;
        if ((1 + (lw - PS) / p->patch_stride) * (1 + (lh - PS) / p->patch_stride) > 4096) return 1;  /* patches per scale */
        pyr += (long)lw * lh;
    }
    /* a pair's working set on the device (4 pyramids + 20 finest-scale planes) within 5 * W * H floats */
    if (4 * pyr + 20L * (w >> p->finest_scale) * (h >> p->finest_scale) > 5L * w * h) return 1;
    if (coarsest) *coarsest = c;
    if (finest) *finest = p->finest_scale;
    return 0;
}

/* D3: u8 INTER_AREA reduction by an integer factor f (sides divisible by f).  f == 2: (sum + 2) >> 2 (OpenCV's
 * fast 2x2 path); f > 2: sum / f^2 rounded half to even (cvRound of sum * scale). */
void dis_area_down(const uint8_t *src, int w, int h, int f, uint8_t *dst) {
    int ow = w / f, oh = h / f, a = f * f;
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++) {
            int s = 0;
            for (int j = 0; j < f; j++)
                for (int i = 0; i < f; i++) s += src[(y * f + j) * w + x * f + i];
            int q;
            if (f == 1) q = s;
            else if (f == 2) q = (s + 2) >> 2;
            else {
                q = s / a;
                int r = s - q * a;
                if (2 * r > a || (2 * r == a && (q & 1))) q++;
            }
            dst[y * ow + x] = (uint8_t)q;
        }
}

/* D4: 3x3 Sobel, replicated border (integers, exact in float) */
static void sobel(const float *I, int w, int h, float *gx, float *gy) {
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int ym = clampi(y - 1, 0, h - 1), yp = clampi(y + 1, 0, h - 1);
            int xm = clampi(x - 1, 0, w - 1), xp = clampi(x + 1, 0, w - 1);
            float a = I[ym * w + xm], b = I[ym * w + x], c = I[ym * w + xp];
            float d = I[y * w + xm], f = I[y * w + xp];
            float g = I[yp * w + xm], k = I[yp * w + x], l = I[yp * w + xp];
            gx[y * w + x] = ((c + 2.0f * f) + l) - ((a + 2.0f * d) + g);
            gy[y * w + x] = ((g + 2.0f * k) + l) - ((a + 2.0f * b) + c);
        }
}

/* D0: the fixed reduction order of 64 values (lane l of a wave = patch pixel (l / 8, l % 8)) */
static float wave_sum(const float *v) {
    float t[NPIX];
    memcpy(t, v, sizeof(t));
    for (int off = 32; off >= 1; off >>= 1)
        for (int i = 0; i < off; i++) t[i] = t[i] + t[i + off];
    return t[0];
}

/* D5: bilinear sample of I1 with clamp-to-edge indices and float weights */
static inline float bilin(const float *I, int w, int h, int x0, int y0, float ax, float ay) {
    int c0 = clampi(x0, 0, w - 1), c1 = clampi(x0 + 1, 0, w - 1);
    int r0 = clampi(y0, 0, h - 1), r1 = clampi(y0 + 1, 0, h - 1);
    float w00 = (1.0f - ax) * (1.0f - ay), w01 = ax * (1.0f - ay), w10 = (1.0f - ax) * ay, w11 = ax * ay;
    return ((w00 * I[r0 * w + c0] + w01 * I[r0 * w + c1]) + w10 * I[r1 * w + c0]) + w11 * I[r1 * w + c1];
}

typedef struct {
    float i0[NPIX], gx[NPIX], gy[NPIX];
    float sx, sy, ih11, ih12, ih22;
    int x, y;
} patch_t;

/* D6: per-patch constants */
static void patch_prepare(patch_t *P, const float *I0, const float *GX, const float *GY, int w, int x, int y, int mean_norm) {
    float xx[NPIX], xy[NPIX], yy[NPIX];
    P->x = x;
    P->y = y;
    for (int l = 0; l < NPIX; l++) {
        int o = (y + l / 8) * w + x + l % 8;
        P->i0[l] = I0[o];
        P->gx[l] = GX[o];
        P->gy[l] = GY[o];
        xx[l] = P->gx[l] * P->gx[l];
        xy[l] = P->gx[l] * P->gy[l];
        yy[l] = P->gy[l] * P->gy[l];
    }
    float sx = wave_sum(P->gx), sy = wave_sum(P->gy), sxx = wave_sum(xx), sxy = wave_sum(xy), syy = wave_sum(yy);
    float h11 = sxx, h12 = sxy, h22 = syy;
    if (mean_norm) {
        h11 = sxx - sx * sx / 64.0f;
        h12 = sxy - sx * sy / 64.0f;
        h22 = syy - sy * sy / 64.0f;
    }
    float det = h11 * h22 - h12 * h12;
    if (fabsf(det) < DET_EPS) det = DET_EPS;
    P->sx = sx;
    P->sy = sy;
    P->ih11 = h22 / det;
    P->ih12 = -h12 / det;
    P->ih22 = h11 / det;
}

/* D7: residual of the patch warped by (ux, uy): d[l] = I1(patch pixel + u) - I0(patch pixel) */
static void patch_diff(const patch_t *P, const float *I1, int w, int h, float ux, float uy, float *d) {
    float x1 = fminf(fmaxf((float)P->x + ux, -7.0f), (float)(w - 1));
    float y1 = fminf(fmaxf((float)P->y + uy, -7.0f), (float)(h - 1));
    float fx = floorf(x1), fy = floorf(y1);
    int ix = (int)fx, iy = (int)fy;
    float ax = x1 - fx, ay = y1 - fy;
    for (int l = 0; l < NPIX; l++) d[l] = bilin(I1, w, h, ix + l % 8, iy + l / 8, ax, ay) - P->i0[l];
}

static float patch_ssd(const patch_t *P, const float *I1, int w, int h, float ux, float uy, int mean_norm) {
    float d[NPIX], dd[NPIX];
    patch_diff(P, I1, w, h, ux, uy, d);
    for (int l = 0; l < NPIX; l++) dd[l] = d[l] * d[l];
    float sdd = wave_sum(dd);
    if (!mean_norm) return sdd;
    float sd = wave_sum(d);
    return sdd - sd * sd / 64.0f;
}

/* D8: one inverse-compositional Gauss-Newton step */
static void patch_step(const patch_t *P, const float *I1, int w, int h, float *ux, float *uy, int mean_norm) {
    float d[NPIX], dx[NPIX], dy[NPIX];
    patch_diff(P, I1, w, h, *ux, *uy, d);
    for (int l = 0; l < NPIX; l++) {
        dx[l] = d[l] * P->gx[l];
        dy[l] = d[l] * P->gy[l];
    }
    float bx = wave_sum(dx), by = wave_sum(dy);
    if (mean_norm) {
        float sd = wave_sum(d);
        bx = bx - sd * P->sx / 64.0f;
        by = by - sd * P->sy / 64.0f;
    }
    float ddx = P->ih11 * bx + P->ih12 * by, ddy = P->ih12 * bx + P->ih22 * by;
    *ux = *ux - ddx;
    *uy = *uy - ddy;
}

/* D9: patch search of one level.  U0: start field (w*h*2), S: patch flows (hs*ws*2); S1 (optional) gets the pass-1
 * flows. */
static void patch_search(const float *I0, const float *GX, const float *GY, const float *I1, int w, int h, const float *U0,
                         const dis_params *p, float *S, float *S1) {
    const int st = p->patch_stride, ws = 1 + (w - PS) / st, hs = 1 + (h - PS) / st;
    const int ns = p->stripes == 0 ? hs : (p->stripes < hs ? p->stripes : hs);
    const int rps = (hs + ns - 1) / ns;
    const int mn = p->use_mean_norm, sp = p->use_spatial_prop;
    const int inner = sp ? p->grad_descent_iters / 2 : p->grad_descent_iters;
    const float lim = (float)(PS * PS);
    for (int r0 = 0; r0 < hs; r0 += rps) {
        const int r1 = r0 + rps < hs ? r0 + rps : hs;
        for (int pass = 0; pass < (sp ? 2 : 1); pass++) {
            for (int k = 0; k < (r1 - r0) * ws; k++) {
                const int q = pass == 0 ? k : (r1 - r0) * ws - 1 - k;
                const int is = r0 + q / ws, js = q % ws;
                patch_t P;
                patch_prepare(&P, I0, GX, GY, w, js * st, is * st, mn);
                const int c = (is * st + PS / 2) * w + js * st + PS / 2;
                const float u0 = U0[2 * c], v0 = U0[2 * c + 1];
                float ux, uy;
                if (pass == 0) {
                    ux = u0;
                    uy = v0;
                } else {
                    ux = S[2 * (is * ws + js)];
                    uy = S[2 * (is * ws + js) + 1];
                }
                if (sp) {
                    float best = patch_ssd(&P, I1, w, h, ux, uy, mn);
                    for (int n = 0; n < 2; n++) {
                        int ci, cj;
                        if (pass == 0) {
                            ci = n == 0 ? is : is - 1;
                            cj = n == 0 ? js - 1 : js;
                            if (cj < 0 || ci < r0) continue;
                        } else {
                            ci = n == 0 ? is : is + 1;
                            cj = n == 0 ? js + 1 : js;
                            if (cj >= ws || ci >= r1) continue;
                        }
                        const float cx = S[2 * (ci * ws + cj)], cy = S[2 * (ci * ws + cj) + 1];
                        const float e = patch_ssd(&P, I1, w, h, cx, cy, mn);
                        if (e < best) {
                            best = e;
                            ux = cx;
                            uy = cy;
                        }
                    }
                }
                for (int it = 0; it < inner; it++) patch_step(&P, I1, w, h, &ux, &uy, mn);
                const float ex = ux - u0, ey = uy - v0;
                if (ex * ex + ey * ey > lim) {
                    ux = u0;
                    uy = v0;
                }
                S[2 * (is * ws + js)] = ux;
                S[2 * (is * ws + js) + 1] = uy;
            }
            if (pass == 0 && S1)
                for (int i = r0; i < r1; i++)
                    for (int j = 0; j < ws; j++) {
                        S1[2 * (i * ws + j)] = S[2 * (i * ws + j)];
                        S1[2 * (i * ws + j) + 1] = S[2 * (i * ws + j) + 1];
                    }
        }
    }
}

/* D10: densification: u(x) = sum lambda_i u_i / sum lambda_i, patches in raster order, lambda = 1/max(1,|I1(x+u_i)-I0(x)|) */
void dis_densify(const float *I0, const float *I1, int w, int h, const float *S, int stride, float *U) {
    const int ws = 1 + (w - PS) / stride, hs = 1 + (h - PS) / stride;
    for (int i = 0; i < h; i++)
        for (int j = 0; j < w; j++) {
            int is0 = i - PS + 1 < 0 ? 0 : (i - PS + 1 + stride - 1) / stride, is1 = i / stride < hs - 1 ? i / stride : hs - 1;
            int js0 = j - PS + 1 < 0 ? 0 : (j - PS + 1 + stride - 1) / stride, js1 = j / stride < ws - 1 ? j / stride : ws - 1;
            float su = 0.0f, sv = 0.0f, sl = 0.0f;
            const float i0 = I0[i * w + j];
            for (int is = is0; is <= is1; is++)
                for (int js = js0; js <= js1; js++) {
                    const float ux = S[2 * (is * ws + js)], uy = S[2 * (is * ws + js) + 1];
                    const float x1 = fminf(fmaxf((float)j + ux, -1.0f), (float)w);
                    const float y1 = fminf(fmaxf((float)i + uy, -1.0f), (float)h);
                    const float fx = floorf(x1), fy = floorf(y1);
                    const float d = bilin(I1, w, h, (int)fx, (int)fy, x1 - fx, y1 - fy) - i0;
                    const float lam = 1.0f / fmaxf(1.0f, fabsf(d));
                    su = su + lam * ux;
                    sv = sv + lam * uy;
                    sl = sl + lam;
                }
            U[2 * (i * w + j)] = su / sl;
            U[2 * (i * w + j) + 1] = sv / sl;
        }
}

/* D11: 5-tap derivative (1, -8, 0, 8, -1) / 12 along x (dx = 1) or y (dx = 0), replicated border */
static void deriv5(const float *f, int w, int h, int along_x, float *out) {
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            float a, b, c, d;
            if (along_x) {
                a = f[y * w + clampi(x - 2, 0, w - 1)];
                b = f[y * w + clampi(x - 1, 0, w - 1)];
                c = f[y * w + clampi(x + 1, 0, w - 1)];
                d = f[y * w + clampi(x + 2, 0, w - 1)];
            } else {
                a = f[clampi(y - 2, 0, h - 1) * w + x];
                b = f[clampi(y - 1, 0, h - 1) * w + x];
                c = f[clampi(y + 1, 0, h - 1) * w + x];
                d = f[clampi(y + 2, 0, h - 1) * w + x];
            }
            out[y * w + x] = (((a - 8.0f * b) + 8.0f * c) - d) / 12.0f;
        }
}

/* D12: variational refinement of U in place */
static void var_refine(const float *I0, const float *I1, int w, int h, float *U, const dis_params *p) {
    const int n = w * h;
    float *buf = (float *)calloc((size_t)n * 24, sizeof(float));
    float *I1w = buf, *I0x = buf + n, *I0y = buf + 2 * n, *I1x = buf + 3 * n, *I1y = buf + 4 * n, *t0 = buf + 5 * n, *t1 = buf + 6 * n;
    float *Ix = buf + 7 * n, *Iy = buf + 8 * n, *Iz = buf + 9 * n, *Ixx = buf + 10 * n, *Ixy = buf + 11 * n, *Iyy = buf + 12 * n,
          *Ixz = buf + 13 * n, *Iyz = buf + 14 * n;
    float *A11 = buf + 15 * n, *A12 = buf + 16 * n, *A22 = buf + 17 * n, *B1 = buf + 18 * n, *B2 = buf + 19 * n, *WS = buf + 20 * n;
    float *dU = buf + 21 * n;  /* 2n, interleaved */
    for (int i = 0; i < h; i++)
        for (int j = 0; j < w; j++) {
            const float x1 = fminf(fmaxf((float)j + U[2 * (i * w + j)], -1.0f), (float)w);
            const float y1 = fminf(fmaxf((float)i + U[2 * (i * w + j) + 1], -1.0f), (float)h);
            const float fx = floorf(x1), fy = floorf(y1);
            I1w[i * w + j] = bilin(I1, w, h, (int)fx, (int)fy, x1 - fx, y1 - fy);
        }
    deriv5(I0, w, h, 1, I0x);
    deriv5(I0, w, h, 0, I0y);
    deriv5(I1w, w, h, 1, I1x);
    deriv5(I1w, w, h, 0, I1y);
    for (int k = 0; k < n; k++) {
        Ix[k] = 0.5f * (I0x[k] + I1x[k]);
        Iy[k] = 0.5f * (I0y[k] + I1y[k]);
        Iz[k] = I1w[k] - I0[k];
        Ixz[k] = I1x[k] - I0x[k];
        Iyz[k] = I1y[k] - I0y[k];
    }
    deriv5(I0x, w, h, 1, t0);
    deriv5(I1x, w, h, 1, t1);
    for (int k = 0; k < n; k++) Ixx[k] = 0.5f * (t0[k] + t1[k]);
    deriv5(I0x, w, h, 0, t0);
    deriv5(I1x, w, h, 0, t1);
    for (int k = 0; k < n; k++) Ixy[k] = 0.5f * (t0[k] + t1[k]);
    deriv5(I0y, w, h, 0, t0);
    deriv5(I1y, w, h, 0, t1);
    for (int k = 0; k < n; k++) Iyy[k] = 0.5f * (t0[k] + t1[k]);

    const float alpha = p->vr_alpha, gamma = p->vr_gamma, delta = p->vr_delta;
    for (int it = 0; it < p->var_refine_iters; it++) {
        /* smoothness weights of U + dU (forward differences, 0 past the last column / row) */
        for (int i = 0; i < h; i++)
            for (int j = 0; j < w; j++) {
                const int k = i * w + j, kr = j < w - 1 ? k + 1 : k, kd = i < h - 1 ? k + w : k;
                const float u = U[2 * k] + dU[2 * k], v = U[2 * k + 1] + dU[2 * k + 1];
                const float ux = (U[2 * kr] + dU[2 * kr]) - u, vx = (U[2 * kr + 1] + dU[2 * kr + 1]) - v;
                const float uy = (U[2 * kd] + dU[2 * kd]) - u, vy = (U[2 * kd + 1] + dU[2 * kd + 1]) - v;
                const float s2 = ((ux * ux + uy * uy) + vx * vx) + vy * vy;
                WS[k] = alpha * (0.5f / sqrtf(s2 + VR_EPS2));
            }
        /* data term linearised at dU */
        for (int k = 0; k < n; k++) {
            const float du = dU[2 * k], dv = dU[2 * k + 1];
            const float ix = Ix[k], iy = Iy[k], iz = Iz[k], ixx = Ixx[k], ixy = Ixy[k], iyy = Iyy[k], ixz = Ixz[k], iyz = Iyz[k];
            const float nd = (ix * ix + iy * iy) + VR_ZETA2;
            const float r = (iz + ix * du) + iy * dv;
            const float wd = delta * (0.5f / sqrtf(r * r / nd + VR_EPS2)) / nd;
            const float bx = 1.0f / ((ixx * ixx + ixy * ixy) + VR_ZETA2), by = 1.0f / ((ixy * ixy + iyy * iyy) + VR_ZETA2);
            const float rx = (ixz + ixx * du) + ixy * dv, ry = (iyz + ixy * du) + iyy * dv;
            const float wg = gamma * (0.5f / sqrtf((bx * rx * rx + by * ry * ry) + VR_EPS2));
            A11[k] = wd * ix * ix + wg * (bx * ixx * ixx + by * ixy * ixy);
            A12[k] = wd * ix * iy + wg * (bx * ixx * ixy + by * ixy * iyy);
            A22[k] = wd * iy * iy + wg * (bx * ixy * ixy + by * iyy * iyy);
            B1[k] = -(wd * ix * iz + wg * (bx * ixx * ixz + by * ixy * iyz));
            B2[k] = -(wd * iy * iz + wg * (bx * ixy * ixz + by * iyy * iyz));
        }
        /* red-black SOR on dU */
        for (int sweep = 0; sweep < VR_SOR; sweep++)
            for (int color = 0; color < 2; color++)
                for (int i = 0; i < h; i++)
                    for (int j = (i + color) & 1; j < w; j += 2) {
                        const int k = i * w + j;
                        const int kl = j > 0 ? k - 1 : k, kr = j < w - 1 ? k + 1 : k, ku = i > 0 ? k - w : k, kd = i < h - 1 ? k + w : k;
                        const float wl = j > 0 ? WS[k - 1] : 0.0f, wr = j < w - 1 ? WS[k] : 0.0f;
                        const float wu = i > 0 ? WS[k - w] : 0.0f, wdn = i < h - 1 ? WS[k] : 0.0f;
                        const float sw = ((wl + wr) + wu) + wdn;
                        const float u = U[2 * k], v = U[2 * k + 1];
                        const float su = ((wl * ((U[2 * kl] - u) + dU[2 * kl]) + wr * ((U[2 * kr] - u) + dU[2 * kr])) +
                                          wu * ((U[2 * ku] - u) + dU[2 * ku])) + wdn * ((U[2 * kd] - u) + dU[2 * kd]);
                        const float sv = ((wl * ((U[2 * kl + 1] - v) + dU[2 * kl + 1]) + wr * ((U[2 * kr + 1] - v) + dU[2 * kr + 1])) +
                                          wu * ((U[2 * ku + 1] - v) + dU[2 * ku + 1])) + wdn * ((U[2 * kd + 1] - v) + dU[2 * kd + 1]);
                        const float du = dU[2 * k], dv = dU[2 * k + 1];
                        const float den1 = A11[k] + sw, den2 = A22[k] + sw;
                        const float du2 = den1 > 0.0f ? (1.0f - VR_OMEGA) * du + VR_OMEGA * (((B1[k] + su) - A12[k] * dv) / den1) : du;
                        const float dv2 = den2 > 0.0f ? (1.0f - VR_OMEGA) * dv + VR_OMEGA * (((B2[k] + sv) - A12[k] * du2) / den2) : dv;
                        dU[2 * k] = du2;
                        dU[2 * k + 1] = dv2;
                    }
    }
    for (int k = 0; k < 2 * n; k++) U[k] = U[k] + dU[k];
    free(buf);
}

/* D13: INTER_LINEAR resize of a 2-channel float field by an integer factor f (half-pixel centres, OpenCV's edge rule),
 * each component multiplied by `mul` */
void dis_upsample(const float *src, int w, int h, int f, float mul, float *dst) {
    const int ow = w * f, oh = h * f;
    const float inv = 1.0f / (float)f;
    for (int y = 0; y < oh; y++) {
        const float syf = ((float)y + 0.5f) * inv - 0.5f;
        int y0 = (int)floorf(syf);
        float fy = syf - floorf(syf);
        if (y0 < 0) { y0 = 0; fy = 0.0f; }
        if (y0 >= h - 1) { y0 = h - 1; fy = 0.0f; }
        const int y1 = y0 + 1 < h ? y0 + 1 : h - 1;
        for (int x = 0; x < ow; x++) {
            const float sxf = ((float)x + 0.5f) * inv - 0.5f;
            int x0 = (int)floorf(sxf);
            float fx = sxf - floorf(sxf);
            if (x0 < 0) { x0 = 0; fx = 0.0f; }
            if (x0 >= w - 1) { x0 = w - 1; fx = 0.0f; }
            const int x1 = x0 + 1 < w ? x0 + 1 : w - 1;
            for (int c = 0; c < 2; c++) {
                const float r0 = src[2 * (y0 * w + x0) + c] * (1.0f - fx) + src[2 * (y0 * w + x1) + c] * fx;
                const float r1 = src[2 * (y1 * w + x0) + c] * (1.0f - fx) + src[2 * (y1 * w + x1) + c] * fx;
                dst[2 * (y * ow + x) + c] = (r0 * (1.0f - fy) + r1 * fy) * mul;
            }
        }
    }
}

/* The whole pair.  flow: (h, w, 2).  Debug capture: when dbg != NULL, the field of (dbg_scale, dbg_stage) is copied
 * to it -- stage 0 patch flows after pass 1, 1 after pass 2 (hs*ws*2), 2 densified, 3 after VR (lh*lw*2);
 * stage 4: the level images I0, I1 as floats (2 * lh * lw). */
int dis_flow(const uint8_t *f0, const uint8_t *f1, int w, int h, const dis_params *p, float *flow, int dbg_scale,
             int dbg_stage, float *dbg) {
    int c, f;
    if (dis_geometry(w, h, p, &c, &f)) return 1;
    const int fw = w >> f, fh = h >> f, nf = fw * fh;
    uint8_t *pyr = (uint8_t *)malloc((size_t)2 * nf);
    uint8_t *tmp = (uint8_t *)malloc((size_t)2 * nf);
    float *I0 = (float *)malloc(sizeof(float) * nf), *I1 = (float *)malloc(sizeof(float) * nf);
    float *GX = (float *)malloc(sizeof(float) * nf), *GY = (float *)malloc(sizeof(float) * nf);
    float *U0 = (float *)calloc((size_t)2 * nf, sizeof(float)), *U = (float *)malloc(sizeof(float) * 2 * nf);
    float *S = (float *)malloc(sizeof(float) * 2 * nf), *S1 = (float *)malloc(sizeof(float) * 2 * nf);
    for (int s = c; s >= f; s--) {
        const int lw = w >> s, lh = h >> s, n = lw * lh;
        /* level images: area reduction of the frame by 2^f, then 2x steps up to scale s */
        for (int k = 0; k < 2; k++) {
            dis_area_down(k ? f1 : f0, w, h, 1 << f, pyr + k * nf);
            for (int t = f; t < s; t++) {
                dis_area_down(pyr + k * nf, w >> t, h >> t, 2, tmp);
                memcpy(pyr + k * nf, tmp, (size_t)(w >> (t + 1)) * (h >> (t + 1)));
            }
        }
        for (int k = 0; k < n; k++) {
            I0[k] = pyr[k];
            I1[k] = pyr[nf + k];
        }
        sobel(I0, lw, lh, GX, GY);
        if (dbg && dbg_scale == s && dbg_stage == 4) {
            memcpy(dbg, I0, sizeof(float) * n);
            memcpy(dbg + n, I1, sizeof(float) * n);
        }
        patch_search(I0, GX, GY, I1, lw, lh, U0, p, S, S1);
        const int ns = (1 + (lw - PS) / p->patch_stride) * (1 + (lh - PS) / p->patch_stride);
        if (dbg && dbg_scale == s && dbg_stage == 0) memcpy(dbg, S1, sizeof(float) * 2 * ns);
        if (dbg && dbg_scale == s && dbg_stage == 1) memcpy(dbg, S, sizeof(float) * 2 * ns);
        dis_densify(I0, I1, lw, lh, S, p->patch_stride, U);
        if (dbg && dbg_scale == s && dbg_stage == 2) memcpy(dbg, U, sizeof(float) * 2 * n);
        if (p->var_refine_iters > 0) var_refine(I0, I1, lw, lh, U, p);
        if (dbg && dbg_scale == s && dbg_stage == 3) memcpy(dbg, U, sizeof(float) * 2 * n);
        if (s > f) dis_upsample(U, lw, lh, 2, 2.0f, U0);
        else dis_upsample(U, lw, lh, 1 << f, (float)(1 << f), flow);
    }
    free(pyr); free(tmp); free(I0); free(I1); free(GX); free(GY); free(U0); free(U); free(S); free(S1);
    return 0;
}
