// DIS optical flow (Kroeger et al., ECCV 2016; the parameters of OpenCV's DISOpticalFlow PRESET_FAST) for gfx950:
// the reference's "DNN" backend, FunscriptFlow.pyw:948-980.  The rules are frozen in DESIGN.md appendix D (D0-D13);
// tests/dis_ref/dis_ref.c restates them in plain C and this file must agree with it bit for bit.  Every
// floating-point expression is written in the order the restatement evaluates it (no FMA contraction: the Makefile's
// -ffp-contract=off), and every sum over the 64 pixels of a patch is the xor butterfly of dis_wave_sum (D0).
//
// Shape: ONE workgroup of 1024 threads per pair runs the whole pair -- the u8 pyramid of both frames, Sobel gradients,
// and per scale (coarsest first) the patch search (one wave per stripe, one lane per patch pixel), densification,
// variational refinement and the x2 upsample into the next scale's start field; the last scale's field is resized
// x 2^finest straight into the pair's flow slot, where the unchanged k_pass1 picks it up.  At 1/4 resolution a pair
// is small (64x64 at 256x256): its planes live in a per-pair region of the lane's work buffer (L2 / MALL resident),
// only the patch flows of the current scale live in LDS.  Phases are separated by __syncthreads().
#include "ffl_kernels.h"

#define DIS_THREADS 1024
#define DIS_WAVES (DIS_THREADS / 64)
#define DIS_PS 8
#define DIS_DET_EPS 0.001f
#define DIS_ZETA2 0.01f
#define DIS_EPS2 1e-6f
#define DIS_OMEGA 1.6f
#define DIS_SOR 5

// D0: lane l ends with ((v_l + v_{l^32}) + ...) -- the same value in every lane (each step adds commutatively equal
// pairs), equal to the restatement's t[0]
__device__ __forceinline__ float dis_wave_sum(float v) {
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// D5
__device__ __forceinline__ float dis_bilin(const float *__restrict__ I, int w, int h, int x0, int y0, float ax, float ay) {
    const int c0 = ffl_clampi(x0, 0, w - 1), c1 = ffl_clampi(x0 + 1, 0, w - 1);
    const int r0 = ffl_clampi(y0, 0, h - 1), r1 = ffl_clampi(y0 + 1, 0, h - 1);
    const float w00 = (1.0f - ax) * (1.0f - ay), w01 = ax * (1.0f - ay), w10 = (1.0f - ax) * ay, w11 = ax * ay;
    return ((w00 * I[r0 * w + c0] + w01 * I[r0 * w + c1]) + w10 * I[r1 * w + c0]) + w11 * I[r1 * w + c1];
}

// D11
__device__ __forceinline__ float dis_deriv5(const float *__restrict__ f, int w, int h, int x, int y, int along_x) {
    float a, b, c, d;
    if (along_x) {
        a = f[y * w + ffl_clampi(x - 2, 0, w - 1)];
        b = f[y * w + ffl_clampi(x - 1, 0, w - 1)];
        c = f[y * w + ffl_clampi(x + 1, 0, w - 1)];
        d = f[y * w + ffl_clampi(x + 2, 0, w - 1)];
    } else {
        a = f[ffl_clampi(y - 2, 0, h - 1) * w + x];
        b = f[ffl_clampi(y - 1, 0, h - 1) * w + x];
        c = f[ffl_clampi(y + 1, 0, h - 1) * w + x];
        d = f[ffl_clampi(y + 2, 0, h - 1) * w + x];
    }
    return (((a - 8.0f * b) + 8.0f * c) - d) / 12.0f;
}

// D10 / D12 sampler of I1 at a pixel displaced by (ux, uy)
__device__ __forceinline__ float dis_sample_px(const float *__restrict__ I1, int w, int h, int j, int i, float ux, float uy) {
    const float x1 = fminf(fmaxf((float)j + ux, -1.0f), (float)w);
    const float y1 = fminf(fmaxf((float)i + uy, -1.0f), (float)h);
    const float fx = floorf(x1), fy = floorf(y1);
    return dis_bilin(I1, w, h, (int)fx, (int)fy, x1 - fx, y1 - fy);
}

struct DisPatch {  // one lane's pixel of the wave's patch + the patch constants (wave-uniform)
    float i0, gx, gy, sx, sy, ih11, ih12, ih22;
    int x, y;
};

// D7: this lane's residual for flow (ux, uy)
__device__ __forceinline__ float dis_patch_diff(const DisPatch &P, const float *__restrict__ I1, int w, int h, float ux, float uy,
                                                int px, int py) {
    const float x1 = fminf(fmaxf((float)P.x + ux, -7.0f), (float)(w - 1));
    const float y1 = fminf(fmaxf((float)P.y + uy, -7.0f), (float)(h - 1));
    const float fx = floorf(x1), fy = floorf(y1);
    const int ix = (int)fx, iy = (int)fy;
    return dis_bilin(I1, w, h, ix + px, iy + py, x1 - fx, y1 - fy) - P.i0;
}

__device__ __forceinline__ float dis_patch_ssd(const DisPatch &P, const float *__restrict__ I1, int w, int h, float ux, float uy,
                                               int px, int py, int mean_norm) {
    const float d = dis_patch_diff(P, I1, w, h, ux, uy, px, py);
    const float sdd = dis_wave_sum(d * d);
    if (!mean_norm) return sdd;
    const float sd = dis_wave_sum(d);
    return sdd - sd * sd / 64.0f;
}

// ---- phases --------------------------------------------------------------------------------------------------------

// D9: the wave's stripes of one scale; S (LDS) holds the scale's patch flows
__device__ void dis_patch_search(const DisKParams &p, int lw, int lh, const float *__restrict__ I0, const float *__restrict__ GX,
                                 const float *__restrict__ GY, const float *__restrict__ I1, const float *__restrict__ U0, float2 *S,
                                 float *dbg1) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, px = lane & 7, py = lane >> 3;
    const int st = p.stride, ws = 1 + (lw - DIS_PS) / st, hs = 1 + (lh - DIS_PS) / st;
    const int ns = p.stripes == 0 ? hs : (p.stripes < hs ? p.stripes : hs);
    const int rps = (hs + ns - 1) / ns, nstripes = (hs + rps - 1) / rps;
    const int mn = p.mean_norm, sp = p.spatial_prop;
    const int inner = sp ? p.gd_iters / 2 : p.gd_iters;
    const float lim = (float)(DIS_PS * DIS_PS);
    #pragma unroll 1
    for (int stripe = wv; stripe < nstripes; stripe += DIS_WAVES) {
        const int r0 = stripe * rps, r1 = r0 + rps < hs ? r0 + rps : hs, np = (r1 - r0) * ws;
        #pragma unroll 1
        for (int pass = 0; pass < (sp ? 2 : 1); pass++) {
            #pragma unroll 1
            for (int k = 0; k < np; k++) {
                const int q = pass == 0 ? k : np - 1 - k;
                const int is = r0 + q / ws, js = q % ws;
                // D6
                DisPatch P;
                P.x = js * st;
                P.y = is * st;
                const int o = (P.y + py) * lw + P.x + px;
                P.i0 = I0[o];
                P.gx = GX[o];
                P.gy = GY[o];
                const float sx = dis_wave_sum(P.gx), sy = dis_wave_sum(P.gy);
                const float sxx = dis_wave_sum(P.gx * P.gx), sxy = dis_wave_sum(P.gx * P.gy), syy = dis_wave_sum(P.gy * P.gy);
                float h11 = sxx, h12 = sxy, h22 = syy;
                if (mn) {
                    h11 = sxx - sx * sx / 64.0f;
                    h12 = sxy - sx * sy / 64.0f;
                    h22 = syy - sy * sy / 64.0f;
                }
                float det = h11 * h22 - h12 * h12;
                if (fabsf(det) < DIS_DET_EPS) det = DIS_DET_EPS;
                P.sx = sx;
                P.sy = sy;
                P.ih11 = h22 / det;
                P.ih12 = -h12 / det;
                P.ih22 = h11 / det;
                const int c = (P.y + DIS_PS / 2) * lw + P.x + DIS_PS / 2;
                const float u0 = U0[2 * c], v0 = U0[2 * c + 1];
                float ux, uy;
                if (pass == 0) {
                    ux = u0;
                    uy = v0;
                } else {
                    const float2 s = S[is * ws + js];
                    ux = s.x;
                    uy = s.y;
                }
                if (sp) {
                    float best = dis_patch_ssd(P, I1, lw, lh, ux, uy, px, py, mn);
                    #pragma unroll 1
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
                        const float2 cand = S[ci * ws + cj];
                        const float e = dis_patch_ssd(P, I1, lw, lh, cand.x, cand.y, px, py, mn);
                        if (e < best) {
                            best = e;
                            ux = cand.x;
                            uy = cand.y;
                        }
                    }
                }
                #pragma unroll 1
                for (int it = 0; it < inner; it++) {  // D8
                    const float d = dis_patch_diff(P, I1, lw, lh, ux, uy, px, py);
                    float bx = dis_wave_sum(d * P.gx), by = dis_wave_sum(d * P.gy);
                    if (mn) {
                        const float sd = dis_wave_sum(d);
                        bx = bx - sd * P.sx / 64.0f;
                        by = by - sd * P.sy / 64.0f;
                    }
                    const float ddx = P.ih11 * bx + P.ih12 * by, ddy = P.ih12 * bx + P.ih22 * by;
                    ux = ux - ddx;
                    uy = uy - ddy;
                }
                const float ex = ux - u0, ey = uy - v0;
                if (ex * ex + ey * ey > lim) {
                    ux = u0;
                    uy = v0;
                }
                // the next patch's lanes read this entry (pass-1 left / pass-2 right neighbour): a wavefront-scope
                // release/acquire orders lane 0's LDS store before those loads (one wave's LDS operations also
                // complete in order on CDNA; the fence states the requirement rather than relying on it silently)
                if (lane == 0) S[is * ws + js] = make_float2(ux, uy);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            if (pass == 0 && dbg1)
                #pragma unroll 1
                for (int q = lane; q < np; q += 64) {
                    const float2 s = S[r0 * ws + q];
                    dbg1[2 * (r0 * ws + q)] = s.x;
                    dbg1[2 * (r0 * ws + q) + 1] = s.y;
                }
        }
    }
}

// The pair's scratch region (floats; nf = pixels of the finest scale): the two u8 pyramids and I0's Sobel gradients as
// float pyramids (scales finest..coarsest at p.pyr_off), the start field U0, the field U and VR's increment dU (2 nf each),
// then 14 planes for the refinement.
#define DIS_PAIR_REGION                                                                                              \
    const int b = blockIdx.x, tid = threadIdx.x;                                                                     \
    const int f = p.finest, W = p.w, H = p.h, nf = (W >> f) * (H >> f);                                              \
    float *const P0 = scratch + (size_t)b * p.pair_floats, *const P1 = P0 + p.pyr_floats;                            \
    float *const GX = P1 + p.pyr_floats, *const GY = GX + p.pyr_floats;                                              \
    float *const U0 = GY + p.pyr_floats, *const U = U0 + 2 * nf, *const dU = U + 2 * nf, *const V = dU + 2 * nf;     \
    const bool dbg_here = p.dbg && b == 0;                                                                           \
    (void)U;                                                                                                         \
    (void)dU;                                                                                                        \
    (void)V;                                                                                                         \
    (void)dbg_here

// phase 1: the u8 pyramid of both frames (D3), Sobel gradients of I0 (D4), zero start field of the coarsest scale
__global__ __launch_bounds__(DIS_THREADS) void k_dis_prep(const UTab *__restrict__ ut, const PairTab *__restrict__ pt,
                                                          const uint8_t *__restrict__ gray, size_t gray_stride, float *scratch,
                                                          DisKParams p) {
    DIS_PAIR_REGION;

    const int c = p.coarsest, fw = W >> f;
    // D3: level f of both frames straight from the frames, then 2x steps
    {
        const uint8_t *g0 = gray + (size_t)ut->fslot[pt->u0[b]] * gray_stride, *g1 = gray + (size_t)ut->fslot[pt->u1[b]] * gray_stride;
        const int fac = 1 << f, area = fac * fac;
        #pragma unroll 1
        for (int k = tid; k < 2 * nf; k += DIS_THREADS) {
            const int fr = k >= nf, q = fr ? k - nf : k, y = q / fw, x = q - y * fw;
            const uint8_t *g = fr ? g1 : g0;
            int s = 0;
            for (int j = 0; j < fac; j++)
                for (int i = 0; i < fac; i++) s += g[(size_t)(y * fac + j) * W + x * fac + i];
            int v;
            if (fac == 1) v = s;
            else if (fac == 2) v = (s + 2) >> 2;
            else {
                v = s / area;
                const int r = s - v * area;
                if (2 * r > area || (2 * r == area && (v & 1))) v++;
            }
            (fr ? P1 : P0)[q] = (float)v;
        }
        __syncthreads();
        #pragma unroll 1
        for (int s = f + 1; s <= c; s++) {
            const int pw = W >> (s - 1), lw = W >> s, lh = H >> s, n = lw * lh;
            const float *s0 = P0 + p.pyr_off[s - 1 - f], *s1 = P1 + p.pyr_off[s - 1 - f];
            float *d0 = P0 + p.pyr_off[s - f], *d1 = P1 + p.pyr_off[s - f];
            #pragma unroll 1
            for (int k = tid; k < 2 * n; k += DIS_THREADS) {
                const int fr = k >= n, q = fr ? k - n : k, y = q / lw, x = q - y * lw;
                const float *sp = fr ? s1 : s0;
                const int sum = (int)sp[2 * y * pw + 2 * x] + (int)sp[2 * y * pw + 2 * x + 1] + (int)sp[(2 * y + 1) * pw + 2 * x] +
                                (int)sp[(2 * y + 1) * pw + 2 * x + 1];
                (fr ? d1 : d0)[q] = (float)((sum + 2) >> 2);
            }
            __syncthreads();
        }
        // D4: Sobel of every I0 level
        #pragma unroll 1
        for (int s = f; s <= c; s++) {
            const int lw = W >> s, lh = H >> s, n = lw * lh;
            const float *I = P0 + p.pyr_off[s - f];
            #pragma unroll 1
            for (int k = tid; k < n; k += DIS_THREADS) {
                const int y = k / lw, x = k - y * lw;
                const int ym = ffl_clampi(y - 1, 0, lh - 1), yp = ffl_clampi(y + 1, 0, lh - 1);
                const int xm = ffl_clampi(x - 1, 0, lw - 1), xp = ffl_clampi(x + 1, 0, lw - 1);
                const float a = I[ym * lw + xm], bb = I[ym * lw + x], cc = I[ym * lw + xp];
                const float d = I[y * lw + xm], ff = I[y * lw + xp];
                const float g = I[yp * lw + xm], kk = I[yp * lw + x], l = I[yp * lw + xp];
                GX[p.pyr_off[s - f] + k] = ((cc + 2.0f * ff) + l) - ((a + 2.0f * d) + g);
                GY[p.pyr_off[s - f] + k] = ((g + 2.0f * kk) + l) - ((a + 2.0f * bb) + cc);
            }
        }
        const int lc = (W >> c) * (H >> c);
        #pragma unroll 1
        for (int k = tid; k < 2 * lc; k += DIS_THREADS) U0[k] = 0.0f;
        __syncthreads();
    }

}

// phase 2 of scale s: patch search (D9) and densification (D10)
__global__ __launch_bounds__(DIS_THREADS) void k_dis_search(float *scratch, DisKParams p, int s) {
    __shared__ float2 S[DIS_MAX_PATCHES];
    DIS_PAIR_REGION;
    const int lw = W >> s, lh = H >> s, n = lw * lh;
    const float *I0 = P0 + p.pyr_off[s - f], *I1 = P1 + p.pyr_off[s - f];
    const float *gx = GX + p.pyr_off[s - f], *gy = GY + p.pyr_off[s - f];
    const bool dbg_s = dbg_here && p.dbg_scale == s;
    if (dbg_s && p.dbg_stage == 4)
        #pragma unroll 1
        for (int k = tid; k < n; k += DIS_THREADS) {
            p.dbg[k] = I0[k];
            p.dbg[n + k] = I1[k];
        }
    dis_patch_search(p, lw, lh, I0, gx, gy, I1, U0, S, dbg_s && p.dbg_stage == 0 ? p.dbg : nullptr);
    __syncthreads();
    const int stride = p.stride, ws = 1 + (lw - DIS_PS) / stride, hs = 1 + (lh - DIS_PS) / stride;
    if (dbg_s && p.dbg_stage == 1)
        #pragma unroll 1
        for (int k = tid; k < ws * hs; k += DIS_THREADS) {
            p.dbg[2 * k] = S[k].x;
            p.dbg[2 * k + 1] = S[k].y;
        }
    // D10
    #pragma unroll 1
    for (int k = tid; k < n; k += DIS_THREADS) {
        const int i = k / lw, j = k - i * lw;
        const int is0 = i - DIS_PS + 1 < 0 ? 0 : (i - DIS_PS + 1 + stride - 1) / stride, is1 = i / stride < hs - 1 ? i / stride : hs - 1;
        const int js0 = j - DIS_PS + 1 < 0 ? 0 : (j - DIS_PS + 1 + stride - 1) / stride, js1 = j / stride < ws - 1 ? j / stride : ws - 1;
        float su = 0.0f, sv = 0.0f, sl = 0.0f;
        const float i0 = I0[k];
        #pragma unroll 1
        for (int is = is0; is <= is1; is++)
            #pragma unroll 1
            for (int js = js0; js <= js1; js++) {
                const float2 u = S[is * ws + js];
                const float d = dis_sample_px(I1, lw, lh, j, i, u.x, u.y) - i0;
                const float lam = 1.0f / fmaxf(1.0f, fabsf(d));
                su = su + lam * u.x;
                sv = sv + lam * u.y;
                sl = sl + lam;
            }
        U[2 * k] = su / sl;
        U[2 * k + 1] = sv / sl;
    }
    __syncthreads();
    if (dbg_s && p.dbg_stage == 2)
        #pragma unroll 1
        for (int k = tid; k < 2 * n; k += DIS_THREADS) p.dbg[k] = U[k];

}

// phase 3 of scale s: variational refinement (D12), then the upsample (D13) into the next scale's start field or
// into the pair's flow slot
__global__ __launch_bounds__(DIS_THREADS) void k_dis_refine(const PairTab *__restrict__ pt, float *scratch, DisKParams p, int s) {
    DIS_PAIR_REGION;
    const int lw = W >> s, lh = H >> s, n = lw * lh;
    const float *I0 = P0 + p.pyr_off[s - f], *I1 = P1 + p.pyr_off[s - f];
    const bool dbg_s = dbg_here && p.dbg_scale == s;
    if (p.vr_iters > 0) {  // D12
        float *I1w = V, *I0x = V + n, *I0y = V + 2 * n, *I1x = V + 3 * n, *I1y = V + 4 * n;
        float *Ix = V + 6 * n, *Iy = V + 7 * n, *Iz = V + 8 * n, *Ixx = V + 9 * n, *Ixy = V + 10 * n, *Iyy = V + 11 * n,
              *Ixz = V + 12 * n, *Iyz = V + 13 * n;
        float *A11 = V, *A12 = V + n, *A22 = V + 2 * n, *B1 = V + 3 * n, *B2 = V + 4 * n, *WS = V + 5 * n;  // over the sources
        #pragma unroll 1
        for (int k = tid; k < n; k += DIS_THREADS) {
            const int i = k / lw, j = k - i * lw;
            I1w[k] = dis_sample_px(I1, lw, lh, j, i, U[2 * k], U[2 * k + 1]);
        }
        __syncthreads();
        #pragma unroll 1
        for (int k = tid; k < n; k += DIS_THREADS) {
            const int i = k / lw, j = k - i * lw;
            I0x[k] = dis_deriv5(I0, lw, lh, j, i, 1);
            I0y[k] = dis_deriv5(I0, lw, lh, j, i, 0);
            I1x[k] = dis_deriv5(I1w, lw, lh, j, i, 1);
            I1y[k] = dis_deriv5(I1w, lw, lh, j, i, 0);
        }
        __syncthreads();
        #pragma unroll 1
        for (int k = tid; k < n; k += DIS_THREADS) {
            const int i = k / lw, j = k - i * lw;
            Ix[k] = 0.5f * (I0x[k] + I1x[k]);
            Iy[k] = 0.5f * (I0y[k] + I1y[k]);
            Iz[k] = I1w[k] - I0[k];
            Ixz[k] = I1x[k] - I0x[k];
            Iyz[k] = I1y[k] - I0y[k];
            Ixx[k] = 0.5f * (dis_deriv5(I0x, lw, lh, j, i, 1) + dis_deriv5(I1x, lw, lh, j, i, 1));
            Ixy[k] = 0.5f * (dis_deriv5(I0x, lw, lh, j, i, 0) + dis_deriv5(I1x, lw, lh, j, i, 0));
            Iyy[k] = 0.5f * (dis_deriv5(I0y, lw, lh, j, i, 0) + dis_deriv5(I1y, lw, lh, j, i, 0));
            dU[2 * k] = 0.0f;
            dU[2 * k + 1] = 0.0f;
        }
        __syncthreads();
        const float alpha = p.alpha, gamma = p.gamma, delta = p.delta;
        #pragma unroll 1
        for (int it = 0; it < p.vr_iters; it++) {
            #pragma unroll 1
            for (int k = tid; k < n; k += DIS_THREADS) {
                const int i = k / lw, j = k - i * lw;
                const int kr = j < lw - 1 ? k + 1 : k, kd = i < lh - 1 ? k + lw : k;
                const float u = U[2 * k] + dU[2 * k], v = U[2 * k + 1] + dU[2 * k + 1];
                const float ux = (U[2 * kr] + dU[2 * kr]) - u, vx = (U[2 * kr + 1] + dU[2 * kr + 1]) - v;
                const float uy = (U[2 * kd] + dU[2 * kd]) - u, vy = (U[2 * kd + 1] + dU[2 * kd + 1]) - v;
                const float s2 = ((ux * ux + uy * uy) + vx * vx) + vy * vy;
                WS[k] = alpha * (0.5f / sqrtf(s2 + DIS_EPS2));
                const float du = dU[2 * k], dv = dU[2 * k + 1];
                const float ix = Ix[k], iy = Iy[k], iz = Iz[k], ixx = Ixx[k], ixy = Ixy[k], iyy = Iyy[k], ixz = Ixz[k], iyz = Iyz[k];
                const float nd = (ix * ix + iy * iy) + DIS_ZETA2;
                const float r = (iz + ix * du) + iy * dv;
                const float wd = delta * (0.5f / sqrtf(r * r / nd + DIS_EPS2)) / nd;
                const float bx = 1.0f / ((ixx * ixx + ixy * ixy) + DIS_ZETA2), by = 1.0f / ((ixy * ixy + iyy * iyy) + DIS_ZETA2);
                const float rx = (ixz + ixx * du) + ixy * dv, ry = (iyz + ixy * du) + iyy * dv;
                const float wg = gamma * (0.5f / sqrtf((bx * rx * rx + by * ry * ry) + DIS_EPS2));
                A11[k] = wd * ix * ix + wg * (bx * ixx * ixx + by * ixy * ixy);
                A12[k] = wd * ix * iy + wg * (bx * ixx * ixy + by * ixy * iyy);
                A22[k] = wd * iy * iy + wg * (bx * ixy * ixy + by * iyy * iyy);
                B1[k] = -(wd * ix * iz + wg * (bx * ixx * ixz + by * ixy * iyz));
                B2[k] = -(wd * iy * iz + wg * (bx * ixy * ixz + by * iyy * iyz));
            }
            __syncthreads();
            #pragma unroll 1
            for (int sweep = 0; sweep < 2 * DIS_SOR; sweep++) {
                const int color = sweep & 1;
                #pragma unroll 1
                for (int k = tid; k < n; k += DIS_THREADS) {
                    const int i = k / lw, j = k - i * lw;
                    if (((i + j + color) & 1) != 0) continue;
                    const int kl = j > 0 ? k - 1 : k, kr = j < lw - 1 ? k + 1 : k, ku = i > 0 ? k - lw : k, kd = i < lh - 1 ? k + lw : k;
                    const float wl = j > 0 ? WS[k - 1] : 0.0f, wr = j < lw - 1 ? WS[k] : 0.0f;
                    const float wu = i > 0 ? WS[k - lw] : 0.0f, wdn = i < lh - 1 ? WS[k] : 0.0f;
                    const float sw = ((wl + wr) + wu) + wdn;
                    const float u = U[2 * k], v = U[2 * k + 1];
                    const float su = ((wl * ((U[2 * kl] - u) + dU[2 * kl]) + wr * ((U[2 * kr] - u) + dU[2 * kr])) +
                                      wu * ((U[2 * ku] - u) + dU[2 * ku])) + wdn * ((U[2 * kd] - u) + dU[2 * kd]);
                    const float sv = ((wl * ((U[2 * kl + 1] - v) + dU[2 * kl + 1]) + wr * ((U[2 * kr + 1] - v) + dU[2 * kr + 1])) +
                                      wu * ((U[2 * ku + 1] - v) + dU[2 * ku + 1])) + wdn * ((U[2 * kd + 1] - v) + dU[2 * kd + 1]);
                    const float du = dU[2 * k], dv = dU[2 * k + 1];
                    const float den1 = A11[k] + sw, den2 = A22[k] + sw;
                    const float du2 = den1 > 0.0f ? (1.0f - DIS_OMEGA) * du + DIS_OMEGA * (((B1[k] + su) - A12[k] * dv) / den1) : du;
                    const float dv2 = den2 > 0.0f ? (1.0f - DIS_OMEGA) * dv + DIS_OMEGA * (((B2[k] + sv) - A12[k] * du2) / den2) : dv;
                    dU[2 * k] = du2;
                    dU[2 * k + 1] = dv2;
                }
                __syncthreads();
            }
        }
        #pragma unroll 1
        for (int k = tid; k < 2 * n; k += DIS_THREADS) U[k] = U[k] + dU[k];
        __syncthreads();
    }
    if (dbg_s && p.dbg_stage == 3)
        #pragma unroll 1
        for (int k = tid; k < 2 * n; k += DIS_THREADS) p.dbg[k] = U[k];

    // D13: x2 into the next scale's start field, or x 2^finest into the flow slot
    const int fac = s > f ? 2 : (1 << f);
    const float mul = s > f ? 2.0f : (float)(1 << f), inv = 1.0f / (float)fac;
    const int ow = lw * fac, oh = lh * fac;
    float *dst = s > f ? U0 : pt->flow[0][b];
    #pragma unroll 1
    for (int k = tid; k < ow * oh; k += DIS_THREADS) {
        const int y = k / ow, x = k - y * ow;
        const float syf = ((float)y + 0.5f) * inv - 0.5f;
        int y0 = (int)floorf(syf);
        float fy = syf - floorf(syf);
        if (y0 < 0) { y0 = 0; fy = 0.0f; }
        if (y0 >= lh - 1) { y0 = lh - 1; fy = 0.0f; }
        const int y1 = y0 + 1 < lh ? y0 + 1 : lh - 1;
        const float sxf = ((float)x + 0.5f) * inv - 0.5f;
        int x0 = (int)floorf(sxf);
        float fx = sxf - floorf(sxf);
        if (x0 < 0) { x0 = 0; fx = 0.0f; }
        if (x0 >= lw - 1) { x0 = lw - 1; fx = 0.0f; }
        const int x1 = x0 + 1 < lw ? x0 + 1 : lw - 1;
        float o2[2];
        for (int ch = 0; ch < 2; ch++) {
            const float r0 = U[2 * (y0 * lw + x0) + ch] * (1.0f - fx) + U[2 * (y0 * lw + x1) + ch] * fx;
            const float r1 = U[2 * (y1 * lw + x0) + ch] * (1.0f - fx) + U[2 * (y1 * lw + x1) + ch] * fx;
            o2[ch] = (r0 * (1.0f - fy) + r1 * fy) * mul;
        }
        dst[2 * k] = o2[0];
        dst[2 * k + 1] = o2[1];
    }
    __syncthreads();
}

void ffl_launch_dis(const UTab *ut, const PairTab *pt, int nB, const uint8_t *gray, size_t gray_stride, float *scratch,
                    const DisKParams &p, hipStream_t st) {
    hipLaunchKernelGGL(k_dis_prep, dim3(nB), dim3(DIS_THREADS), 0, st, ut, pt, gray, gray_stride, scratch, p);
    for (int s = p.coarsest; s >= p.finest; s--) {
        hipLaunchKernelGGL(k_dis_search, dim3(nB), dim3(DIS_THREADS), 0, st, scratch, p, s);
        hipLaunchKernelGGL(k_dis_refine, dim3(nB), dim3(DIS_THREADS), 0, st, pt, scratch, p, s);
    }
}
