// Farneback with caller-chosen parameters (ffl_flow_pairs_farneback).
//
// The arithmetic is the oracle's (oracle/farneback_oracle.c) with pyr_scale, levels, winsize, iterations, poly_n and
// poly_sigma as parameters; at the reference's values every result is bit-identical to it, elsewhere to the plain-C
// restatement tests/fb_general_ref.  These kernels are correct first: one launch per stage, 64-lane waves, separable
// passes staged in LDS, f64 wherever the appendix says double.  The tuned kernels (kernels_farneback.hip) are not used.
//
// A batch runs eagerly on its lane's stream:
//   per level k (all unique frames, z = frame):  blur rows (u8 -> T)  ->  blur columns (T -> B)  ->  resize (B -> I)
//                                                ->  PolyExp<poly_n> (I -> R_k)
//   per level k, coarse to fine (z = pair):      flow init (zero / upsample x 1/pyr_scale)  ->  UpdateMatrices
//                                                ->  iterations x (box + solve [-> UpdateMatrices])
// Under ffl_flow_pairs_farneback_ex's modes the window is the float Gaussian of F.7 (k_fbg_gauss_solve) and the coarsest
// level starts from the pair's flow slot reduced by INTER_AREA (F.8, k_fbg_flow_area) instead of zero.
// T and B live in the M area and I in flow buffer fa: none of them is live once the frames are expanded.
#include "ffl_kernels.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int BH_W = 256;            // k_fbg_blur_h: outputs per workgroup (one row)
constexpr int BV_W = 64, BV_H = 32;  // k_fbg_blur_v: 64 x 32 outputs per workgroup
constexpr int PE_W = 64, PE_H = 16;  // k_fbg_polyexp / k_fbg_box_solve tiles
constexpr int BS_W = 64, BS_H = 16;

// Gaussian, horizontal pass: one row segment of BH_W outputs, its 2r-wide halo staged in LDS (REFLECT_101)
__global__ __launch_bounds__(256) void k_fbg_blur_h(const uint8_t *gray, size_t gray_stride, const UTab *ut, int w, int h,
                                                    FbgGauss gk, float *T, size_t T_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *s = reinterpret_cast<float *>(smem);
    const int u = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * BH_W, r = gk.r;
    const uint8_t *row = gray + (size_t)ut->fslot[u] * gray_stride + (size_t)y * w;
    for (int i = threadIdx.x; i < BH_W + 2 * r; i += blockDim.x) s[i] = (float)row[ffl_reflect101(x0 - r + i, w)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    const float *c = s + r + threadIdx.x;
    float acc = gk.k[0] * c[0];
    for (int j = 1; j <= r; j++) acc = acc + gk.k[j] * (c[-j] + c[j]);
    T[(size_t)u * T_stride + (size_t)y * w + x] = acc;
}

// Gaussian, vertical pass: a 64 x 32 tile, its 2r rows of halo staged in LDS (REFLECT_101)
__global__ __launch_bounds__(256) void k_fbg_blur_v(const float *T, size_t stride, int w, int h, FbgGauss gk, float *B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *s = reinterpret_cast<float *>(smem);
    const int u = blockIdx.z, x0 = blockIdx.x * BV_W, y0 = blockIdx.y * BV_H, r = gk.r, rows = BV_H + 2 * r;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = min(x0 + tx, w - 1);
    const float *src = T + (size_t)u * stride;
    for (int i = ty; i < rows; i += 4) s[i * BV_W + tx] = src[(size_t)ffl_reflect101(y0 - r + i, h) * w + x];
    __syncthreads();
    if (x0 + tx >= w) return;
    for (int t = ty; t < BV_H && y0 + t < h; t += 4) {
        const float *c = s + (t + r) * BV_W + tx;
        float acc = gk.k[0] * c[0];
        for (int j = 1; j <= r; j++) acc = acc + gk.k[j] * (c[-j * BV_W] + c[j * BV_W]);
        B[(size_t)u * stride + (size_t)(y0 + t) * w + x0 + tx] = acc;
    }
}

// blurred full-resolution frame -> level image (lw x lh)
__global__ __launch_bounds__(64) void k_fbg_resize(const float *B, size_t B_stride, int w, int h, float *I, size_t I_stride,
                                                   int lw, int lh) {
    const int u = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 64 + threadIdx.x;
    if (x >= lw) return;
    int x0, x1, y0, y1;
    float a1, b1;
    ffl_resize_coord(x, w, (double)w / lw, x0, x1, a1);
    ffl_resize_coord(y, h, (double)h / lh, y0, y1, b1);
    const float *r0 = B + (size_t)u * B_stride + (size_t)y0 * w, *r1 = B + (size_t)u * B_stride + (size_t)y1 * w;
    const float a0 = 1.f - a1, b0 = 1.f - b1;
    const float t0 = r0[x0] * a0 + r0[x1] * a1;
    const float t1 = r1[x0] * a0 + r1[x1] * a1;
    I[(size_t)u * I_stride + (size_t)y * lw + x] = t0 * b0 + t1 * b1;
}

// PolyExp with n = N: the 64 x 16 tile's (16 + 2N) x (64 + 2N) neighbourhood (rows and columns clamped) in LDS, the f32
// vertical part for 16 x (64 + 2N) positions in LDS, then the f64 horizontal part per output
template <int N>
__global__ __launch_bounds__(256) void k_fbg_polyexp(const float *I, size_t I_stride, float *R, size_t R_stride, int w, int h,
                                                     FbgPoly pc) {
    constexpr int TW = PE_W + 2 * N, TH = PE_H + 2 * N;
    __shared__ float sI[TH][TW];
    __shared__ float s0[PE_H][TW], s1[PE_H][TW], s2[PE_H][TW];
    const int u = blockIdx.z, x0 = blockIdx.x * PE_W, y0 = blockIdx.y * PE_H;
    const float *src = I + (size_t)u * I_stride;
    for (int i = threadIdx.x; i < TW * TH; i += blockDim.x) {
        const int ty = i / TW, tx = i - ty * TW;
        sI[ty][tx] = src[(size_t)ffl_clampi(y0 - N + ty, 0, h - 1) * w + ffl_clampi(x0 - N + tx, 0, w - 1)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TW * PE_H; i += blockDim.x) {
        const int t = i / TW, c = i - t * TW;
        float r0 = sI[t + N][c] * pc.g[0], r1 = 0.f, r2 = 0.f;
#pragma unroll
        for (int k = 1; k <= N; k++) {
            const float a = sI[t + N - k][c], b = sI[t + N + k][c];
            const float p = a + b;
            const float t0 = r0 + pc.g[k] * p;
            const float t1 = r1 + pc.xg[k] * (b - a);
            const float t2 = r2 + pc.xxg[k] * p;
            r0 = t0;
            r1 = t1;
            r2 = t2;
        }
        s0[t][c] = r0;
        s1[t][c] = r1;
        s2[t][c] = r2;
    }
    __syncthreads();
    const size_t plane = (size_t)w * h;
    float *dst = R + (size_t)u * R_stride;
    for (int i = threadIdx.x; i < PE_W * PE_H; i += blockDim.x) {
        const int t = i / PE_W, xi = i - t * PE_W, x = x0 + xi, y = y0 + t;
        if (x >= w || y >= h) continue;
        const int c = xi + N;
        float g0 = pc.g[0];
        double b1 = s0[t][c] * g0, b2 = 0, b3 = s1[t][c] * g0, b4 = 0, b5 = s2[t][c] * g0, b6 = 0;
#pragma unroll
        for (int k = 1; k <= N; k++) {
            const float p0 = s0[t][c + k], m0 = s0[t][c - k];
            const double tg = p0 + m0;
            g0 = pc.g[k];
            b1 += tg * g0;
            b4 += tg * pc.xxg[k];
            b2 += (p0 - m0) * pc.xg[k];
            b3 += (s1[t][c + k] + s1[t][c - k]) * g0;
            b6 += (s1[t][c + k] - s1[t][c - k]) * pc.xg[k];
            b5 += (s2[t][c + k] + s2[t][c - k]) * g0;
        }
        const size_t o = (size_t)y * w + x;
        dst[0 * plane + o] = (float)(b3 * pc.ig11);
        dst[1 * plane + o] = (float)(b2 * pc.ig11);
        dst[2 * plane + o] = (float)(b1 * pc.ig03 + b5 * pc.ig33);
        dst[3 * plane + o] = (float)(b1 * pc.ig03 + b4 * pc.ig33);
        dst[4 * plane + o] = (float)(b6 * pc.ig55);
    }
}

// the pair's flow at level k: its flow slot at level 0, else its region of the level's ping-pong buffer
__device__ __forceinline__ float *fbg_flow(const PairTab *pt, float *buf, size_t stride, int b, bool slot) {
    return slot ? pt->flow[0][b] : buf + (size_t)b * stride;
}

// the level's initial flow: zero at the coarsest level, else resize(prev, INTER_LINEAR) * mul
__global__ __launch_bounds__(64) void k_fbg_flow_init(const PairTab *pt, const float *prev, float *cur, size_t stride,
                                                      bool slot, int pw, int ph, int lw, int lh, float mul) {
    const int b = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 64 + threadIdx.x;
    if (x >= lw) return;
    float *f = fbg_flow(pt, cur, stride, b, slot) + ((size_t)y * lw + x) * 2;
    if (pw == 0) {
        f[0] = 0.f;
        f[1] = 0.f;
        return;
    }
    int x0, x1, y0, y1;
    float a1, b1;
    ffl_resize_coord(x, pw, (double)pw / lw, x0, x1, a1);
    ffl_resize_coord(y, ph, (double)ph / lh, y0, y1, b1);
    const float *p = prev + (size_t)b * stride;
    const float *r0 = p + (size_t)y0 * pw * 2, *r1 = p + (size_t)y1 * pw * 2;
    const float a0 = 1.f - a1, b0 = 1.f - b1;
    for (int c = 0; c < 2; c++) {
        const float t0 = r0[x0 * 2 + c] * a0 + r0[x1 * 2 + c] * a1;
        const float t1 = r1[x0 * 2 + c] * a0 + r1[x1 * 2 + c] * a1;
        f[c] = (t0 * b0 + t1 * b1) * mul;
    }
}

// FarnebackUpdateMatrices (A.4; nothing in it depends on the parameters)
__global__ __launch_bounds__(64) void k_fbg_update_matrices(const PairTab *pt, const float *R, size_t R_stride, float *flowbuf,
                                                            size_t f_stride, bool slot, float *M, size_t M_stride, int w,
                                                            int h) {
    const int b = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 64 + threadIdx.x;
    if (x >= w) return;
    const size_t pl = (size_t)w * h, o = (size_t)y * w + x;
    const float *R0 = R + (size_t)pt->u0[b] * R_stride, *R1 = R + (size_t)pt->u1[b] * R_stride;
    const float *f = fbg_flow(pt, flowbuf, f_stride, b, slot);
    const float dx = f[o * 2], dy = f[o * 2 + 1];
    const UmLoc L = ffl_um_locate(w, h, x, y, dx, dy);
    float r0[5], bl[5], out[5];
    for (int c = 0; c < 5; c++) {
        r0[c] = R0[c * pl + o];
        bl[c] = 0.f;
        if (L.inside) {
            const size_t q = c * pl + (size_t)L.y1 * w + L.x1;
            bl[c] = L.a00 * R1[q] + L.a01 * R1[q + 1] + L.a10 * R1[q + w] + L.a11 * R1[q + w + 1];
        }
    }
    ffl_um_finish(r0, bl, L.inside, w, h, x, y, dx, dy, out);
    float *dst = M + (size_t)b * M_stride;
    for (int c = 0; c < 5; c++) dst[c * pl + o] = out[c];
}

// The (2m+1)-term window sum at position q of a sequence v (v(i) = the value at position i, REPLICATE-clamped by the
// caller's staging), in appendix F.5's order: blocks of L = 2m + 2 positions anchored at L*j - (m+1); with q = L*j + t,
// the suffix of block j (positions q-m .. L*j+m, summed from its end) plus the prefix of block j+1 (positions
// L*j+m+1 .. q+m, summed from its start).  Identical to the restatement's block-at-a-time form, one output at a time.
template <typename F>
__device__ __forceinline__ double fbg_box_sum(int q, int m, F v) {
    const int L = 2 * m + 2, j = q / L, t = q - j * L, e = j * L + m;  // e: last position of block j
    double s = 0.0;
    if (t <= 2 * m) {
        s = v(e);
        for (int i = e - 1; i >= q - m; i--) s = v(i) + s;
    }
    if (t == 0) return s;
    double p = v(e + 1);
    for (int i = e + 2; i <= q + m; i++) p = p + v(i);
    return t <= 2 * m ? s + p : p;
}

// FarnebackUpdateFlow_Blur: (2m+1)^2 box in double (columns, then rows) + the 2x2 solve, one 64 x 16 tile, channel by
// channel: M_c's (16 + 2m) x (64 + 2m) neighbourhood (REPLICATE) in LDS, the column sums of 16 x (64 + 2m) positions in
// LDS (double), then the row sums per output
__global__ __launch_bounds__(256) void k_fbg_box_solve(const PairTab *pt, const float *M, size_t M_stride, float *flowbuf,
                                                       size_t f_stride, bool slot, int w, int h, int m) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int TW = BS_W + 2 * m, TH = BS_H + 2 * m;
    double *sV = reinterpret_cast<double *>(smem);                        // [BS_H][TW]
    float *sM = reinterpret_cast<float *>(smem + sizeof(double) * BS_H * TW);  // [TH][TW]
    const int b = blockIdx.z, x0 = blockIdx.x * BS_W, y0 = blockIdx.y * BS_H;
    const size_t pl = (size_t)w * h;
    const float *Mb = M + (size_t)b * M_stride;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    double g[5][4];
    for (int c = 0; c < 5; c++) {
        const float *src = Mb + c * pl;
        __syncthreads();  // the previous channel's row sums are done with sV / sM
        for (int i = threadIdx.x; i < TW * TH; i += blockDim.x) {
            const int r = i / TW, cc = i - r * TW;
            sM[i] = src[(size_t)ffl_clampi(y0 - m + r, 0, h - 1) * w + ffl_clampi(x0 - m + cc, 0, w - 1)];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < TW * BS_H; i += blockDim.x) {
            const int t = i / TW, cc = i - t * TW;
            // rows of the tile's LDS copy are positions y0 - m + r; only window positions of y0 + t are read
            sV[i] = fbg_box_sum(y0 + t, m, [&](int q) { return (double)sM[(q - (y0 - m)) * TW + cc]; });
        }
        __syncthreads();
        for (int k = 0; k < 4; k++) {
            const int t = ty + 4 * k;
            const double *row = sV + t * TW;
            g[c][k] = fbg_box_sum(x0 + tx, m, [&](int q) { return row[q - (x0 - m)]; });
        }
    }
    const int x = x0 + tx;
    if (x >= w) return;
    const double scale = 1. / ((2 * m + 1) * (2 * m + 1));
    float *f = fbg_flow(pt, flowbuf, f_stride, b, slot);
    for (int k = 0; k < 4; k++) {
        const int y = y0 + ty + 4 * k;
        if (y >= h) break;
        const double g11 = g[0][k] * scale, g12 = g[1][k] * scale, g22 = g[2][k] * scale, h1 = g[3][k] * scale,
                     h2 = g[4][k] * scale;
        const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
        f[((size_t)y * w + x) * 2] = (float)((g11 * h2 - g12 * h1) * idet);
        f[((size_t)y * w + x) * 2 + 1] = (float)((g22 * h1 - g12 * h2) * idet);
    }
}

static int cv_round(double v) { return (int)lrint(v); }  // cvRound: the whole-number ratios of F.8 (b)

static size_t box_lds_bytes(int m) {
    return sizeof(double) * BS_H * (BS_W + 2 * m) + sizeof(float) * (BS_H + 2 * m) * (BS_W + 2 * m);
}

static size_t gauss_lds_bytes(int m) { return sizeof(float) * ((BS_H + 2 * m) + BS_H) * (BS_W + 2 * m); }

// FarnebackUpdateFlow_GaussianBlur (F.7): the separable float Gaussian of the five M planes (rows of the window first, then
// columns; REPLICATE) + the 2x2 solve in double, one 64 x 16 tile, channel by channel: M_c's (16 + 2m) x (64 + 2m)
// neighbourhood in LDS, the vertical sums of 16 x (64 + 2m) positions in LDS (float), then the horizontal sums per output.
// No 1 / winsize^2 scale: the taps sum to one.
__global__ __launch_bounds__(256) void k_fbg_gauss_solve(const PairTab *pt, const float *M, size_t M_stride, float *flowbuf,
                                                         size_t f_stride, bool slot, int w, int h, FbgWin win) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int m = win.m, TW = BS_W + 2 * m, TH = BS_H + 2 * m;
    float *sM = reinterpret_cast<float *>(smem);  // [TH][TW]
    float *sV = sM + TH * TW;                     // [BS_H][TW]
    const int b = blockIdx.z, x0 = blockIdx.x * BS_W, y0 = blockIdx.y * BS_H;
    const size_t pl = (size_t)w * h;
    const float *Mb = M + (size_t)b * M_stride;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    float g[5][4];
    for (int c = 0; c < 5; c++) {
        const float *src = Mb + c * pl;
        __syncthreads();  // the previous channel's horizontal sums are done with sV / sM
        for (int i = threadIdx.x; i < TW * TH; i += blockDim.x) {
            const int r = i / TW, cc = i - r * TW;
            sM[i] = src[(size_t)ffl_clampi(y0 - m + r, 0, h - 1) * w + ffl_clampi(x0 - m + cc, 0, w - 1)];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < TW * BS_H; i += blockDim.x) {
            const int t = i / TW, cc = i - t * TW;
            const float *col = sM + (t + m) * TW + cc;  // row y0 + t of the tile's LDS copy
            float v = col[0] * win.k[0];
            for (int j = 1; j <= m; j++) v = v + (col[j * TW] + col[-j * TW]) * win.k[j];
            sV[i] = v;
        }
        __syncthreads();
        for (int k = 0; k < 4; k++) {
            const float *row = sV + (ty + 4 * k) * TW + tx + m;
            float a = row[0] * win.k[0];
            for (int j = 1; j <= m; j++) a = a + win.k[j] * (row[-j] + row[j]);
            g[c][k] = a;
        }
    }
    const int x = x0 + tx;
    if (x >= w) return;
    float *f = fbg_flow(pt, flowbuf, f_stride, b, slot);
    for (int k = 0; k < 4; k++) {
        const int y = y0 + ty + 4 * k;
        if (y >= h) break;
        const double g11 = g[0][k], g12 = g[1][k], g22 = g[2][k], h1 = g[3][k], h2 = g[4][k];
        const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
        f[((size_t)y * w + x) * 2] = (float)((g11 * h2 - g12 * h1) * idet);
        f[((size_t)y * w + x) * 2 + 1] = (float)((g22 * h1 - g12 * h2) * idet);
    }
}

// F.8 (c): the entries of destination index d on an axis of S source and D destination positions (s = S / D), in order:
// an optional left partial cell (s1 - 1, al), the whole cells s1 .. s2 - 1 (af each), an optional right partial cell (s2, ar)
struct FbgAreaAxis {
    int s1, s2, n;
    bool left, right;
    float al, af, ar;
};
__device__ __forceinline__ FbgAreaAxis fbg_area_axis(int d, double s, int S) {
    FbgAreaAxis a;
    const double f1 = d * s, f2 = f1 + s, cw = fmin(s, S - f1);
    int s1 = (int)ceil(f1), s2 = min((int)floor(f2), S - 1);
    s1 = min(s1, s2);
    a.s1 = s1;
    a.s2 = s2;
    a.left = s1 - f1 > 1e-3;
    a.right = f2 - s2 > 1e-3;
    a.al = (float)((s1 - f1) / cw);
    a.af = (float)(1.0 / cw);
    a.ar = (float)(fmin(fmin(f2 - s2, 1.0), cw) / cw);
    a.n = (int)a.left + (s2 - s1) + (int)a.right;
    return a;
}
__device__ __forceinline__ void fbg_area_entry(const FbgAreaAxis &a, int e, int S, int &idx, float &alpha) {
    const int j = e - (int)a.left;
    if (j < 0) {
        idx = a.s1 - 1;
        alpha = a.al;
    } else if (j < a.s2 - a.s1) {
        idx = a.s1 + j;
        alpha = a.af;
    } else {
        idx = a.s2;
        alpha = a.ar;
    }
    idx = ffl_clampi(idx, 0, S - 1);  // the rule keeps every index inside; this keeps the read inside whatever the rule gives
}

// F.8: the coarsest level's initial flow from the pair's full-resolution flow slot: resize(seed, lw x lh, INTER_AREA) *
// scale.  ix, iy > 0: both ratios are whole numbers (1 x 1: the seed itself; else the ix x iy block sum, row-major, times
// 1.f / (ix * iy)); ix = iy = 0: the per-axis coefficient entries, row sums first.
__global__ __launch_bounds__(64) void k_fbg_flow_area(const PairTab *pt, float *cur, size_t stride, int w, int h, int lw,
                                                      int lh, int ix, int iy, float scale) {
    const int b = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 64 + threadIdx.x;
    if (x >= lw) return;
    const float *seed = pt->flow[0][b];
    float *f = cur + (size_t)b * stride + ((size_t)y * lw + x) * 2;
    float s0 = 0.f, s1 = 0.f;
    if (ix == 1 && iy == 1) {  // (a) the same size: the seed itself
        s0 = seed[((size_t)y * w + x) * 2];
        s1 = seed[((size_t)y * w + x) * 2 + 1];
    } else if (ix > 0) {       // (b)
        for (int j = 0; j < iy; j++) {
            const float *row = seed + ((size_t)min(y * iy + j, h - 1) * w) * 2;
            for (int i = 0; i < ix; i++) {
                const int sx = min(x * ix + i, w - 1);
                s0 = s0 + row[sx * 2];
                s1 = s1 + row[sx * 2 + 1];
            }
        }
        const float inv = 1.f / (ix * iy);
        s0 = s0 * inv;
        s1 = s1 * inv;
    } else {                   // (c)
        const FbgAreaAxis ax = fbg_area_axis(x, (double)w / lw, w), ay = fbg_area_axis(y, (double)h / lh, h);
        for (int ey = 0; ey < ay.n; ey++) {
            int sy;
            float beta;
            fbg_area_entry(ay, ey, h, sy, beta);
            const float *row = seed + (size_t)sy * w * 2;
            float b0 = 0.f, b1 = 0.f;
            for (int ex = 0; ex < ax.n; ex++) {
                int sx;
                float alpha;
                fbg_area_entry(ax, ex, w, sx, alpha);
                b0 = b0 + row[sx * 2] * alpha;
                b1 = b1 + row[sx * 2 + 1] * alpha;
            }
            if (ey == 0) {
                s0 = beta * b0;
                s1 = beta * b1;
            } else {
                s0 = s0 + beta * b0;
                s1 = s1 + beta * b1;
            }
        }
    }
    f[0] = s0 * scale;
    f[1] = s1 * scale;
}

}  // namespace

void ffl_launch_fb_general(const UTab *ut, const PairTab *pt, int n, int nU, const uint8_t *gray, size_t gray_stride, int w,
                           int h, const FbgPlan &plan, const FbgWork &wk, hipStream_t st) {
    const size_t N = (size_t)w * h;
    float *T = wk.M, *B = wk.M + N * nU;  // 2 * nU * N floats of the M area (n * 5N >= nU * 2N: nU <= 2n)
    // frames: every level of every unique frame
    for (int k = plan.levels; k >= 0; k--) {
        const FbgGauss &gk = plan.gk[k];
        const int lw = plan.lw[k], lh = plan.lh[k];
        const size_t lpl = (size_t)lw * lh;
        k_fbg_blur_h<<<dim3((w + BH_W - 1) / BH_W, h, nU), 256, sizeof(float) * (BH_W + 2 * gk.r), st>>>(gray, gray_stride, ut, w, h, gk, T, N);
        k_fbg_blur_v<<<dim3((w + BV_W - 1) / BV_W, (h + BV_H - 1) / BV_H, nU), 256, sizeof(float) * BV_W * (BV_H + 2 * gk.r), st>>>(
            T, N, w, h, gk, B);
        k_fbg_resize<<<dim3((lw + 63) / 64, lh, nU), 64, 0, st>>>(B, N, w, h, wk.fa, lpl, lw, lh);
        const dim3 pg((lw + PE_W - 1) / PE_W, (lh + PE_H - 1) / PE_H, nU);
        float *Rk = wk.R + plan.r_off[k];
        if (plan.poly_n == 7)
            k_fbg_polyexp<7><<<pg, 256, 0, st>>>(wk.fa, lpl, Rk, plan.r_frame, lw, lh, plan.poly);
        else
            k_fbg_polyexp<5><<<pg, 256, 0, st>>>(wk.fa, lpl, Rk, plan.r_frame, lw, lh, plan.poly);
    }
    // pairs: the level chain, coarse to fine; level k's flow in fa / fb alternately, level 0's in the flow slot
    const size_t fs = 2 * N;
    int pw = 0, ph = 0;
    float *prev = nullptr;
    for (int k = plan.levels; k >= 0; k--) {
        const int lw = plan.lw[k], lh = plan.lh[k];
        const bool slot = k == 0;
        float *cur = ((plan.levels - k) & 1) ? wk.fb : wk.fa;
        const float *Rk = wk.R + plan.r_off[k];
        const dim3 pg((lw + 63) / 64, lh, n);
        if (k == plan.levels && (plan.mode & FBG_USE_INITIAL_FLOW)) {
            // F.8: the coarsest level starts from the pair's flow slot.  With one scale the slot is the seed as it stands.
            // Otherwise this read of the slot is queued here, on the stream that level 0 below writes the slot on, so it
            // precedes that write; the slot's earlier writer is behind the batch's wait for ev_slot_done.
            if (k > 0) {
                const double sx = (double)w / lw, sy = (double)h / lh;
                const int ix = cv_round(sx), iy = cv_round(sy);
                const bool whole = fabs(sx - ix) < DBL_EPSILON && fabs(sy - iy) < DBL_EPSILON;
                k_fbg_flow_area<<<pg, 64, 0, st>>>(pt, cur, fs, w, h, lw, lh, whole ? ix : 0, whole ? iy : 0, plan.seed_scale);
            }
        } else {
            k_fbg_flow_init<<<pg, 64, 0, st>>>(pt, prev, cur, fs, slot, pw, ph, lw, lh, plan.mul);
        }
        k_fbg_update_matrices<<<pg, 64, 0, st>>>(pt, Rk, plan.r_frame, cur, fs, slot, wk.M, 5 * N, lw, lh);
        const dim3 bg((lw + BS_W - 1) / BS_W, (lh + BS_H - 1) / BS_H, n);
        for (int it = 0; it < plan.iterations; it++) {
            if (plan.mode & FBG_GAUSSIAN_WINDOW)
                k_fbg_gauss_solve<<<bg, 256, gauss_lds_bytes(plan.m), st>>>(pt, wk.M, 5 * N, cur, fs, slot, lw, lh, plan.win);
            else
                k_fbg_box_solve<<<bg, 256, box_lds_bytes(plan.m), st>>>(pt, wk.M, 5 * N, cur, fs, slot, lw, lh, plan.m);
            if (it < plan.iterations - 1)
                k_fbg_update_matrices<<<pg, 64, 0, st>>>(pt, Rk, plan.r_frame, cur, fs, slot, wk.M, 5 * N, lw, lh);
        }
        prev = cur;
        pw = lw;
        ph = lh;
    }
}
