// Template-matching drift correction for tracked regions (ffl_track_template, ffl_track_match).
// A file of its own: the kernels of kernels_track.hip and kernels_post.hip keep the code objects, and the offsets inside
// them, that they had before these were added (see the note above k_texture in kernels_post.hip).
#include <cstdint>
#include <hip/hip_runtime.h>

#include "ffl_kernels.h"

#define MCH_THREADS 256
#define MCH_TSIDE (2 * FFL_MATCH_MAX_P + 1)                          // 33: a template's side at most
#define MCH_CSIDE (2 * FFL_MATCH_MAX_S + 1)                          // 33: the candidates' side at most
#define MCH_WSIDE (2 * (FFL_MATCH_MAX_P + FFL_MATCH_MAX_S) + 1)      // 65: the search window's side at most
#define MCH_PER_LANE ((MCH_CSIDE * MCH_CSIDE + MCH_THREADS - 1) / MCH_THREADS)   // 5 candidates per lane at most

__device__ __forceinline__ double ffl_match_clamp(double c, double hi) {   // rule Q1: two selects, a NaN gives 0
    return c >= 0.0 ? (c <= hi ? c : hi) : 0.0;
}

__device__ __forceinline__ int ffl_match_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// rule N1: the sanitised centre of the two doubles at `cen` and its rounding.  After Q1's selects x is in [0, w-1] whatever
// the bits were, so ix = floor(x + 0.5) is in 0..w-1 (w <= 32768: x + 0.5 is exact); y alike.
__device__ __forceinline__ void ffl_match_anchor(const double *cen, int w, int h, double *x, double *y, int *ix, int *iy) {
    *x = ffl_match_clamp(cen[0], (double)(w - 1));
    *y = ffl_match_clamp(cen[1], (double)(h - 1));
    *ix = (int)floor(*x + 0.5);
    *iy = (int)floor(*y + 0.5);
}

// the whole workgroup's sum / minimum of one value per lane, through s_red[MCH_THREADS] (index tid and tid + k < 256 only);
// every lane returns the result.  Integers: no order of summation to pin.
__device__ __forceinline__ unsigned long long mch_block_min(unsigned long long v, unsigned long long *s_red, int tid) {
    __syncthreads();   // the previous use of s_red is over
    s_red[tid] = v;
    __syncthreads();
    for (int k = MCH_THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) {
            const unsigned long long a = s_red[tid], b = s_red[tid + k];
            s_red[tid] = b < a ? b : a;
        }
        __syncthreads();
    }
    return s_red[0];
}

__device__ __forceinline__ unsigned long long mch_block_sum(unsigned long long v, unsigned long long *s_red, int tid) {
    __syncthreads();
    s_red[tid] = v;
    __syncthreads();
    for (int k = MCH_THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) s_red[tid] += s_red[tid + k];
        __syncthreads();
    }
    return s_red[0];
}

// Phase C of k_track_match for NQ candidates per lane: the template once, (j, i) row-major; per template pixel one LDS byte of
// the template (the same for every lane) and one of the window per candidate, consecutive bytes over the lanes of a wave.  The
// body holds no branch, so a pixel's NQ + 1 reads are in flight together.  Reading four pixels as one word was measured and is
// slower by up to 6x: the addresses are not word-aligned and the lanes' words overlap.
template <int NQ>
__device__ __forceinline__ void mch_walk(const unsigned char *s_win, const unsigned char *s_tm, const int *base, int P, int WS,
                                         int *S1, int *S2) {
    for (int j = 0; j < P; j++) {
        for (int i = 0; i < P; i++) {
            const int tv = (int)s_tm[j * P + i];
            const int o = j * WS + i;
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                const int d = (int)s_win[base[q] + o] - tv;
                S1[q] += d;
                S2[q] += d * d;
            }
        }
    }
}

// ---- k_track_match (appendix N) ---------------------------------------------------------------------------------------
// One workgroup per (track t, item i): grid = (n_tracks, n).  With P = 2p + 1, C = 2s + 1, WS = 2(p + s) + 1:
//   A  every lane reads the centre (the same 16 bytes) and forms the anchor of rule N1;
//   B  the lanes stage the clamped search window (WS x WS bytes, rows WS apart) and the template (P x P bytes) into LDS;
//   C  candidate c = cy * C + cx stands for (dx, dy) = (cx - s, cy - s); lane tid owns c = tid + 256 q, q < 5.  It walks the
//      template once, (j, i) row-major, and adds d and d * d of all its candidates per template pixel (the template byte is read
//      once for the five; the lanes of a wave read consecutive window bytes); the costs of rule N3 go to LDS;
//   D  a minimum over packed keys gives N4: cost < 2^37 in bits 22.., dx^2 + dy^2 <= 512 in bits 12..21, dy + s <= 32 in bits
//      6..11, dx + s <= 32 in bits 0..5 -- the key's order is the lexicographic order of (cost, dist^2, dy, dx);
//   E  a second minimum over the candidates more than one step (Chebyshev) from the best gives N5; all ones: there are none;
//   F  the template's own sums for FLAT, by two integer block sums;
//   G  lane 0 forms the verdict (N6), the record (N7) and the write-back (N8).
// Every index against N1 / N2, with p in 1..16 and s in 1..16 (host-checked, and clamped again below):
//   global reads: the frame slot fr.slot[i] < n_fslots is host-checked; a staged pixel is row clamp(iy - p - s + wy, 0, h - 1),
//     column clamp(ix - p - s + wx, 0, w - 1): inside the w x h frame whatever ix, iy are.  The template bytes are
//     tmpl[t * P * P + k], k < P * P, inside the T * P * P bytes the host checked.  The centre is the 16 bytes at
//     cen + i * cstride + t * 48, inside the (n - 1) * cstride + 48 * (T - 1) + 16 bytes the host checked;
//   s_win[wy * WS + wx], wx, wy < WS <= 65: below 65 * 65.  s_tm[k], k < P * P <= 33 * 33;
//   a candidate's sample: row cy + j <= 2s + 2p = WS - 1, column cx + i <= WS - 1: inside the staged window.  A lane whose
//     c is not below C * C computes on candidate 0 (in bounds) and stores nothing;
//   s_cost[c], c < C * C <= 33 * 33.  s_red[tid], s_red[tid + k] with tid < k, k <= 128: below 256;
//   global writes: out[i * n_tracks + t], i < n, t < n_tracks: inside the n * T records the host checked; the write-back goes
//     to the two doubles the centre was read from.
// Candidate (dx, dy)'s sample (i, j) of rule N2 is I[clamp(iy + dy + j - p)][clamp(ix + dx + i - p)]: with dy = cy - s that is
// staged row wy = cy + j, since iy - p - s + wy = iy + dy + j - p; columns alike.
__global__ __launch_bounds__(MCH_THREADS) void k_track_match(const unsigned char *__restrict__ gray, size_t N, const ExportTab fr,
                                                              int n_tracks, int w, int h, int p_in, int s_in, int mode,
                                                              double min_var, double max_mse, double ratio,
                                                              const unsigned char *__restrict__ tmpl, char *cen, long long cstride,
                                                              int write_back, MatchRecord *__restrict__ out) {
    __shared__ unsigned char s_win[MCH_WSIDE * MCH_WSIDE + 3];
    __shared__ unsigned char s_tm[MCH_TSIDE * MCH_TSIDE + 3];
    __shared__ long long s_cost[MCH_CSIDE * MCH_CSIDE];
    __shared__ unsigned long long s_red[MCH_THREADS];
    const int t = blockIdx.x, item = blockIdx.y, tid = threadIdx.x;
    const int p = ffl_match_clampi(p_in, FFL_MATCH_MAX_P), s = ffl_match_clampi(s_in, FFL_MATCH_MAX_S);
    const int P = 2 * p + 1, C = 2 * s + 1, WS = 2 * (p + s) + 1, NP = P * P, NC = C * C;
    // A
    double *cp = reinterpret_cast<double *>(cen + (long long)item * cstride + (long long)t * 48);
    double x, y;
    int ix, iy;
    ffl_match_anchor(cp, w, h, &x, &y, &ix, &iy);
    // B
    const unsigned char *I = gray + (size_t)fr.slot[item] * N;
    for (int k = tid; k < WS * WS; k += MCH_THREADS) {
        const int wy = k / WS, wx = k - wy * WS;
        const int gy = ffl_match_clampi(iy - p - s + wy, h - 1), gx = ffl_match_clampi(ix - p - s + wx, w - 1);
        s_win[k] = I[(size_t)gy * (size_t)w + (size_t)gx];
    }
    const unsigned char *Tm = tmpl + (size_t)t * (size_t)NP;
    for (int k = tid; k < NP; k += MCH_THREADS) s_tm[k] = Tm[k];
    __syncthreads();
    // C
    int base[MCH_PER_LANE], S1[MCH_PER_LANE], S2[MCH_PER_LANE];
#pragma unroll
    for (int q = 0; q < MCH_PER_LANE; q++) {
        const int c = tid + MCH_THREADS * q;
        const int cc = c < NC ? c : 0;
        const int cy = cc / C, cx = cc - cy * C;
        base[q] = cy * WS + cx;
        S1[q] = 0;
        S2[q] = 0;
    }
    // The rounds q a wave walks are the same for its 64 lanes (tid & ~63 is the wave's first lane), so the switch does not
    // diverge: a lane without a candidate in a round its wave walks adds up candidate 0's differences and drops them.
    switch ((NC - (tid & ~63) + MCH_THREADS - 1) / MCH_THREADS) {   // 0..5 (NC - 192 + 255 > 0: the division never sees a negative)
    case 0: break;
    case 1: mch_walk<1>(s_win, s_tm, base, P, WS, S1, S2); break;
    case 2: mch_walk<2>(s_win, s_tm, base, P, WS, S1, S2); break;
    case 3: mch_walk<3>(s_win, s_tm, base, P, WS, S1, S2); break;
    case 4: mch_walk<4>(s_win, s_tm, base, P, WS, S1, S2); break;
    default: mch_walk<MCH_PER_LANE>(s_win, s_tm, base, P, WS, S1, S2); break;
    }
    unsigned long long key = ~0ull;
#pragma unroll
    for (int q = 0; q < MCH_PER_LANE; q++) {
        const int c = tid + MCH_THREADS * q;
        if (c < NC) {
            long long cost = (long long)NP * (long long)S2[q];                     // N3
            if (mode == MCH_ZSSD) cost -= (long long)S1[q] * (long long)S1[q];
            s_cost[c] = cost;
            const int cy = c / C, cx = c - cy * C, dx = cx - s, dy = cy - s;
            const unsigned long long k = ((unsigned long long)cost << 22) | ((unsigned long long)(dx * dx + dy * dy) << 12) |
                                         ((unsigned long long)cy << 6) | (unsigned long long)cx;
            key = k < key ? k : key;
        }
    }
    // D
    const unsigned long long best = mch_block_min(key, s_red, tid);
    const int bcx = (int)(best & 63ull), bcy = (int)((best >> 6) & 63ull);
    const long long bcost = (long long)(best >> 22);
    // E
    unsigned long long k2 = ~0ull;
#pragma unroll
    for (int q = 0; q < MCH_PER_LANE; q++) {
        const int c = tid + MCH_THREADS * q;
        if (c < NC) {
            const int cy = c / C, cx = c - cy * C;
            const int ax = cx > bcx ? cx - bcx : bcx - cx, ay = cy > bcy ? cy - bcy : bcy - cy;
            if (ax > 1 || ay > 1) {
                const unsigned long long k = (unsigned long long)s_cost[c];       // this lane wrote it
                k2 = k < k2 ? k : k2;
            }
        }
    }
    const unsigned long long sec = mch_block_min(k2, s_red, tid);
    // F
    unsigned long long t1 = 0, t2 = 0;
    for (int k = tid; k < NP; k += MCH_THREADS) {
        const unsigned long long v = s_tm[k];
        t1 += v;
        t2 += v * v;
    }
    const long long T1 = (long long)mch_block_sum(t1, s_red, tid);
    const long long T2 = (long long)mch_block_sum(t2, s_red, tid);
    // G
    if (tid == 0) {
        const double dN = (double)NP;
        const long long second = sec == ~0ull ? -1ll : (long long)sec;
        const long long tvar = (long long)NP * T2 - T1 * T1;
        int status = 0;
        if ((double)tvar < min_var * dN * dN) status |= MCH_FLAT;                 // N6
        if ((double)bcost > max_mse * dN * dN) status |= MCH_POOR;
        if (second >= 0 && (double)bcost > ratio * (double)second) status |= MCH_AMBIGUOUS;
        const int bdx = bcx - s, bdy = bcy - s;
        MatchRecord rec;
        rec.x = x;
        rec.y = y;
        if (status == 0) {                                                        // N7
            rec.x = ffl_match_clamp((double)(ix + bdx), (double)(w - 1));
            rec.y = ffl_match_clamp((double)(iy + bdy), (double)(h - 1));
        }
        rec.dx = bdx;
        rec.dy = bdy;
        rec.cost = bcost;
        rec.second = second;
        rec.status = status;
        rec.pad = 0;
        out[(size_t)item * (size_t)n_tracks + (size_t)t] = rec;
        if (write_back && status == 0) {                                          // N8
            cp[0] = rec.x;
            cp[1] = rec.y;
        }
    }
}

void ffl_launch_track_match(const unsigned char *gray, size_t N, const ExportTab &fr, int n, int n_tracks, int w, int h, int p,
                            int s, int mode, double min_var, double max_mse, double ratio, const unsigned char *tmpl, char *cen,
                            long long cstride, int write_back, MatchRecord *out, hipStream_t st) {
    hipLaunchKernelGGL(k_track_match, dim3(n_tracks, n), dim3(MCH_THREADS), 0, st, gray, N, fr, n_tracks, w, h, p, s, mode, min_var,
                       max_mse, ratio, tmpl, cen, cstride, write_back, out);
}

// ---- k_track_template (rule N10) --------------------------------------------------------------------------------------
// One workgroup per track: Tm[j][i] = I[clamp(iy + j - p)][clamp(ix + i - p)] about the anchor of rule N1.  The reads are
// clamped into the frame; the writes are tmpl[t * P * P + k], k < P * P, inside the T * P * P bytes the host checked.
__global__ __launch_bounds__(MCH_THREADS) void k_track_template(const unsigned char *__restrict__ I, int w, int h, int p_in,
                                                                 const char *__restrict__ cen, unsigned char *__restrict__ tmpl) {
    const int t = blockIdx.x, tid = threadIdx.x;
    const int p = ffl_match_clampi(p_in, FFL_MATCH_MAX_P), P = 2 * p + 1, NP = P * P;
    double x, y;
    int ix, iy;
    ffl_match_anchor(reinterpret_cast<const double *>(cen + (long long)t * 48), w, h, &x, &y, &ix, &iy);
    for (int k = tid; k < NP; k += MCH_THREADS) {
        const int j = k / P, i = k - j * P;
        const int gy = ffl_match_clampi(iy + j - p, h - 1), gx = ffl_match_clampi(ix + i - p, w - 1);
        tmpl[(size_t)t * (size_t)NP + (size_t)k] = I[(size_t)gy * (size_t)w + (size_t)gx];
    }
}

void ffl_launch_track_template(const unsigned char *frame, int n_tracks, int w, int h, int p, const char *cen, unsigned char *tmpl,
                               hipStream_t st) {
    hipLaunchKernelGGL(k_track_template, dim3(n_tracks), dim3(MCH_THREADS), 0, st, frame, w, h, p, cen, tmpl);
}
