// Whole-frame template re-detection for tracked regions (ffl_track_redetect).
// A file of its own, for the reason kernels_match.hip gives at its head: the kernels of the other files keep the code objects,
// and the offsets inside them, that they had before these were added.
#include <cstdint>
#include <hip/hip_runtime.h>

#include "ffl_kernels.h"

#define RDT_THREADS 256
#define RDT_TW 64                                                    // the candidate tile: 64 x 16, four rows per wave
#define RDT_TH 16
#define RDT_PER_LANE (RDT_TW * RDT_TH / RDT_THREADS)                 // 4 candidates of one column per lane
#define RDT_TSIDE (2 * FFL_MATCH_MAX_P + 1)                          // 33: a template's side at most
#define RDT_WW (RDT_TW + 2 * FFL_MATCH_MAX_P)                        // 96: the staged window's width at most
#define RDT_WH (RDT_TH + 2 * FFL_MATCH_MAX_P)                        // 48: its height at most
#define RDT_NONE (~0ull)                                             // the key of "no candidate"

__device__ __forceinline__ double rdt_clamp(double c, double hi) {   // rule Q1: two selects, a NaN gives 0
    return c >= 0.0 ? (c <= hi ? c : hi) : 0.0;
}

__device__ __forceinline__ int rdt_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// What every kernel of a call forms again for its search (item, track t) from the same bytes, which no kernel but the last
// (k_redetect_final, lane 0, at its very end) writes: the trigger and the anchor of rule L1, the candidate rectangle of rule L2
// clipped to the frame, [x0, x1] x [y0, y1], and the tiles that touch it, [tx0, tx1] x [ty0, ty1], cut to the sweep's grid.
struct RdtSearch {
    double *cp;
    double x, y;
    int ix, iy, active;
    int x0, x1, y0, y1;
    int tx0, tx1, ty0, ty1;
};

__device__ __forceinline__ RdtSearch rdt_search(const RedetectArgs &a, int item, int t) {
    RdtSearch s;
    s.cp = reinterpret_cast<double *>(a.cen + (long long)item * a.cstride + (long long)t * 48);
    s.x = rdt_clamp(s.cp[0], (double)(a.w - 1));   // in [0, w - 1] whatever the bits were
    s.y = rdt_clamp(s.cp[1], (double)(a.h - 1));
    s.ix = (int)floor(s.x + 0.5);                  // in 0..w-1 (x + 0.5 is exact below 2^52)
    s.iy = (int)floor(s.y + 0.5);
    s.active = 1;
    if (a.trig) s.active = (*reinterpret_cast<const int *>(a.trig + (long long)item * a.tstride + (long long)t * 48) & a.mask) != 0;
    const int reach = a.reach < 0 ? 0 : (a.reach > 32768 ? 32768 : a.reach);
    s.x0 = reach ? (s.ix - reach > 0 ? s.ix - reach : 0) : 0;              // ix < 2^28 and reach <= 2^15: no overflow
    s.x1 = reach ? (s.ix + reach < a.w - 1 ? s.ix + reach : a.w - 1) : a.w - 1;
    s.y0 = reach ? (s.iy - reach > 0 ? s.iy - reach : 0) : 0;
    s.y1 = reach ? (s.iy + reach < a.h - 1 ? s.iy + reach : a.h - 1) : a.h - 1;
    s.tx0 = s.x0 / RDT_TW;
    s.ty0 = s.y0 / RDT_TH;
    s.tx1 = s.x1 / RDT_TW;
    s.ty1 = s.y1 / RDT_TH;
    if (s.tx1 > s.tx0 + a.gx - 1) s.tx1 = s.tx0 + a.gx - 1;   // never beyond what the sweep's grid wrote (the host sizes the grid
    if (s.ty1 > s.ty0 + a.gy - 1) s.ty1 = s.ty0 + a.gy - 1;   // so that these two never cut anything)
    return s;
}

// the tiles that touch the exclusion square of rule L5 about (bx, by), clipped to the frame and cut to the exclusion grid
struct RdtExcl {
    int e, ex0, ex1, ey0, ey1, nx, ny;
};

__device__ __forceinline__ RdtExcl rdt_excl(const RedetectArgs &a, int bx, int by) {
    RdtExcl q;
    q.e = a.exclude < 1 ? 1 : (a.exclude > FFL_REDETECT_MAX_EXCLUDE ? FFL_REDETECT_MAX_EXCLUDE : a.exclude);
    q.nx = a.ex < 1 ? 1 : (a.ex > RDT_EXCL_NX ? RDT_EXCL_NX : a.ex);
    q.ny = a.ey < 1 ? 1 : (a.ey > RDT_EXCL_NY ? RDT_EXCL_NY : a.ey);
    q.ex0 = (bx - q.e > 0 ? bx - q.e : 0) / RDT_TW;
    q.ey0 = (by - q.e > 0 ? by - q.e : 0) / RDT_TH;
    q.ex1 = (bx + q.e < a.w - 1 ? bx + q.e : a.w - 1) / RDT_TW;
    q.ey1 = (by + q.e < a.h - 1 ? by + q.e : a.h - 1) / RDT_TH;
    if (q.ex1 > q.ex0 + q.nx - 1) q.ex1 = q.ex0 + q.nx - 1;
    if (q.ey1 > q.ey0 + q.ny - 1) q.ey1 = q.ey0 + q.ny - 1;
    return q;
}

// the whole workgroup's minimum of one key per lane, through s_red[RDT_THREADS] (index tid and tid + k < 256 only); every lane
// returns the result
__device__ __forceinline__ unsigned long long rdt_block_min(unsigned long long v, unsigned long long *s_red, int tid) {
    __syncthreads();   // the previous use of s_red is over
    s_red[tid] = v;
    __syncthreads();
    for (int k = RDT_THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) {
            const unsigned long long a = s_red[tid], b = s_red[tid + k];
            s_red[tid] = b < a ? b : a;
        }
        __syncthreads();
    }
    return s_red[0];
}

__device__ __forceinline__ unsigned long long rdt_block_sum(unsigned long long v, unsigned long long *s_red, int tid) {
    __syncthreads();
    s_red[tid] = v;
    __syncthreads();
    for (int k = RDT_THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) s_red[tid] += s_red[tid + k];
        __syncthreads();
    }
    return s_red[0];
}

// The scratch of search s = item * n_tracks + t, `sstride` 64-bit words at scr + s * sstride (ffl_kernels.h):
//   [0, TX * TY)                    the tile keys of the sweep, tile (tx, ty) of the FRAME at ty * TX + tx;
//   [TX * TY, TX * TY + 2)          the pick: the best cost and its row-major position by * w + bx;
//   [TX * TY + 2, TX * TY + 2 + 18) the keys of the re-walked tiles, exclusion-grid block b at b.
// A key is cost << 10 | local index (ly * 64 + lx), or RDT_NONE: costs are below 2^37 (N3: 1089 * 70812225 < 2^37).

// ---- k_redetect_sweep<EXCL> (rules L1 to L3, and the masks of L2 and L5) ------------------------------------------------
// One workgroup per (tile, search): grid = (tiles of the launch, n * n_tracks).  EXCL false: block b is tile (tx0 + b % gx,
// ty0 + b / gx) of the search's own tile range; EXCL true: tile (ex0 + b % nx, ey0 + b / nx) of the tiles about the pick.
//   A  every lane forms rule L1's trigger and anchor (the same bytes); a skipped search, or a tile beyond the range, leaves:
//      the condition is the same for all 256 lanes, and no barrier has been passed;
//   B  the lanes stage the clamped window, (64 + 2p) x (16 + 2p) bytes with rows WW = 64 + 2p apart, and the template;
//   C  lane tid owns column lx = tid & 63 and rows ly = 4 * (tid >> 6) + q, q < 4: the lanes of a wave read consecutive window
//      bytes.  It walks the template once, (j, i) row-major, and adds d and d * d of its four candidates per template pixel;
//   D  a candidate outside rule L2 (and, EXCL, inside the square of rule L5) gets RDT_NONE; one block minimum over the keys; lane 0
//      stores the tile's key.
// Every index against L1 to L3, with p in 1..16 (host-checked, and clamped again below):
//   global reads: the frame slot fr.slot[item] < n_fslots is host-checked; item = blockIdx.y / n_tracks < n.  A staged pixel is
//     row clamp(ty * 16 - p + wy, 0, h - 1), column clamp(tx * 64 - p + wx, 0, w - 1): inside the w x h frame whatever tx, ty
//     are.  The template bytes are tmpl[t * P * P + k], k < P * P; the centre and the trigger word are the bytes the host
//     checked ((n - 1) * stride + 48 * (T - 1) + 16, or + 4);
//   s_win[wy * WW + wx], wx < WW <= 96, wy < WH <= 48: below 96 * 48.  s_tm[k], k < P * P <= 33 * 33;
//   a candidate's sample: row ly + j <= 15 + 2p = WH - 1, column lx + i <= 63 + 2p = WW - 1: inside the staged window, also for
//     a candidate beyond the frame's edge or the reach, whose sums are formed and dropped;
//   s_red[tid], s_red[tid + k] with tid < k, k <= 128: below 256;
//   global writes: EXCL false: scr[s * sstride + ty * TX + tx] with tx0 <= tx <= tx1 <= (w - 1) / 64 < TX, ty alike < TY;
//     EXCL true: scr[s * sstride + TX * TY + 2 + b], b < nx * ny <= 18; s < n * n_tracks <= max_batch * 8, which the
//     allocation is sized for.
// Candidate (cx, cy) = (tx * 64 + lx, ty * 16 + ly): its sample (i, j) of rule L3 is I[clamp(cy + j - p)][clamp(cx + i - p)],
// and cy + j - p = (ty * 16 - p) + (ly + j): staged row ly + j; columns alike.
template <bool EXCL>
__global__ __launch_bounds__(RDT_THREADS) void k_redetect_sweep(const RedetectArgs a) {
    __shared__ unsigned char s_win[RDT_WW * RDT_WH];
    __shared__ unsigned char s_tm[RDT_TSIDE * RDT_TSIDE + 3];
    __shared__ unsigned long long s_red[RDT_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x, srch = blockIdx.y;
    const int item = srch / a.n_tracks, t = srch - item * a.n_tracks;
    const int p = rdt_clampi(a.p, FFL_MATCH_MAX_P) < 1 ? 1 : rdt_clampi(a.p, FFL_MATCH_MAX_P);
    const int P = 2 * p + 1, NP = P * P, WW = RDT_TW + 2 * p, WH = RDT_TH + 2 * p;
    // A
    const RdtSearch s = rdt_search(a, item, t);
    if (!s.active) return;
    unsigned long long *scr = a.scr + (size_t)srch * (size_t)a.sstride;
    const size_t ntiles = (size_t)a.TX * (size_t)a.TY;
    int tx, ty, bx = 0, by = 0, e = 0;
    if (EXCL) {
        const unsigned long long pos = scr[ntiles + 1];
        by = (int)(pos / (unsigned long long)a.w);
        bx = (int)(pos - (unsigned long long)by * (unsigned long long)a.w);
        const RdtExcl q = rdt_excl(a, bx, by);
        e = q.e;
        if (b >= q.nx * q.ny) return;
        tx = q.ex0 + b % q.nx;
        ty = q.ey0 + b / q.nx;
        if (tx > q.ex1 || ty > q.ey1) return;
    } else {
        tx = s.tx0 + b % a.gx;
        ty = s.ty0 + b / a.gx;
        if (tx > s.tx1 || ty > s.ty1) return;
    }
    // B
    const unsigned char *I = a.gray + (size_t)a.fr.slot[item] * a.N;
    const int gx0 = tx * RDT_TW - p, gy0 = ty * RDT_TH - p;
    for (int k = tid; k < WW * WH; k += RDT_THREADS) {
        const int wy = k / WW, wx = k - wy * WW;
        const int gy = rdt_clampi(gy0 + wy, a.h - 1), gx = rdt_clampi(gx0 + wx, a.w - 1);
        s_win[k] = I[(size_t)gy * (size_t)a.w + (size_t)gx];
    }
    const unsigned char *Tm = a.tmpl + (size_t)t * (size_t)NP;
    for (int k = tid; k < NP; k += RDT_THREADS) s_tm[k] = Tm[k];
    __syncthreads();
    // C: mch_walk's branch-free form (kernels_match.hip) with the round count fixed: every lane has its four candidates
    const int lx = tid & (RDT_TW - 1), ly0 = (tid >> 6) * RDT_PER_LANE;
    int S1[RDT_PER_LANE], S2[RDT_PER_LANE];
#pragma unroll
    for (int q = 0; q < RDT_PER_LANE; q++) S1[q] = S2[q] = 0;
    // The pragma keeps the reads bytes: left alone, the compiler reads two template pixels per candidate as one 16-bit LDS word at
    // an unaligned address whose words overlap between lanes -- the form DESIGN.md section 24 measured as up to 6x slower, and 6.3x
    // slower here (section 25).  Unrolled by four, the byte reads of a row share one address and differ in their immediate offset.
    const unsigned char *wp = s_win + ly0 * WW + lx;
    for (int j = 0; j < P; j++) {
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(4)
        for (int i = 0; i < P; i++) {
            const int tv = (int)s_tm[j * P + i];
            const int o = j * WW + i;
#pragma unroll
            for (int q = 0; q < RDT_PER_LANE; q++) {
                const int d = (int)wp[o + q * WW] - tv;
                S1[q] += d;
                S2[q] += d * d;
            }
        }
    }
    // D
    unsigned long long key = RDT_NONE;
    const int cx = tx * RDT_TW + lx;
#pragma unroll
    for (int q = 0; q < RDT_PER_LANE; q++) {
        const int ly = ly0 + q, cy = ty * RDT_TH + ly;
        bool ok = cx >= s.x0 && cx <= s.x1 && cy >= s.y0 && cy <= s.y1;   // rule L2 (x1 <= w - 1, y1 <= h - 1)
        if (EXCL) {
            const int ax = cx > bx ? cx - bx : bx - cx, ay = cy > by ? cy - by : by - cy;
            ok = ok && (ax > e || ay > e);                               // rule L5
        }
        long long cost = (long long)NP * (long long)S2[q];               // N3
        if (a.mode == MCH_ZSSD) cost -= (long long)S1[q] * (long long)S1[q];
        const unsigned long long k = ((unsigned long long)cost << 10) | (unsigned long long)(ly * RDT_TW + lx);
        if (ok && k < key) key = k;
    }
    const unsigned long long best = rdt_block_min(key, s_red, tid);
    if (tid == 0) scr[EXCL ? ntiles + 2 + (size_t)b : (size_t)ty * (size_t)a.TX + (size_t)tx] = best;
}

// ---- k_redetect_pick (rule L4) ----------------------------------------------------------------------------------------
// One workgroup per search.  The lanes stride over the tiles of the search's range, unpack every key into (cost, cy, cx) and
// keep the lexicographic minimum of (cost, cy * w + cx) -- the row-major order of the FRAME, which the tile order is not; a
// reduction over the pairs follows (the position is below 2^28: cost and position do not fit one 64-bit key together).
//   reads: scr[s * sstride + ty * TX + tx], tx0 <= tx <= tx1, ty0 <= ty <= ty1: exactly the words the sweep wrote;
//   s_cost / s_pos[tid], [tid + k], tid < k <= 128: below 256;
//   writes: scr[s * sstride + TX * TY + {0, 1}].
// The range holds the anchor's tile, whose candidate (ix, iy) is inside rule L2: there is always a key that is not RDT_NONE.
__global__ __launch_bounds__(RDT_THREADS) void k_redetect_pick(const RedetectArgs a) {
    __shared__ unsigned long long s_cost[RDT_THREADS], s_pos[RDT_THREADS];
    const int tid = threadIdx.x, srch = blockIdx.x;
    const int item = srch / a.n_tracks, t = srch - item * a.n_tracks;
    const RdtSearch s = rdt_search(a, item, t);
    if (!s.active) return;
    unsigned long long *scr = a.scr + (size_t)srch * (size_t)a.sstride;
    const size_t ntiles = (size_t)a.TX * (size_t)a.TY;
    const int nx = s.tx1 - s.tx0 + 1, ny = s.ty1 - s.ty0 + 1;
    unsigned long long bc = RDT_NONE, bp = RDT_NONE;
    for (long long k = tid; k < (long long)nx * ny; k += RDT_THREADS) {
        const int ty = s.ty0 + (int)(k / nx), tx = s.tx0 + (int)(k % nx);
        const unsigned long long key = scr[(size_t)ty * (size_t)a.TX + (size_t)tx];
        if (key == RDT_NONE) continue;
        const unsigned long long cost = key >> 10;
        const int loc = (int)(key & 1023ull);
        const unsigned long long pos = (unsigned long long)(ty * RDT_TH + (loc >> 6)) * (unsigned long long)a.w +
                                       (unsigned long long)(tx * RDT_TW + (loc & 63));
        if (cost < bc || (cost == bc && pos < bp)) {
            bc = cost;
            bp = pos;
        }
    }
    s_cost[tid] = bc;
    s_pos[tid] = bp;
    __syncthreads();
    for (int k = RDT_THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) {
            const unsigned long long c2 = s_cost[tid + k], p2 = s_pos[tid + k];
            if (c2 < s_cost[tid] || (c2 == s_cost[tid] && p2 < s_pos[tid])) {
                s_cost[tid] = c2;
                s_pos[tid] = p2;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        scr[ntiles] = s_cost[0];
        scr[ntiles + 1] = s_pos[0];
    }
}

// ---- k_redetect_final (rules L5 to L8, and L7's skipped form) -----------------------------------------------------------
// One workgroup per search.  second = the minimum over the stored keys of the range's tiles that do not touch the exclusion
// square (every candidate of such a tile is further than `exclude` from the best) and over the re-walked keys of those that do;
// the template's own sums for FLAT by two block sums; lane 0 forms the verdict, the record and the write-back.
//   reads: the tile keys as k_redetect_pick; the pick; scr[s * sstride + TX * TY + 2 + b] for the blocks b = (ty - ey0) * nx +
//     (tx - ex0) with ex0 <= tx <= ex1, ey0 <= ty <= ey1 -- exactly the words the exclusion sweep wrote; tmpl[t * P * P + k],
//     k < P * P;
//   writes: out[item * n_tracks + t], inside the n * T records the host checked; the two doubles the centre was read from.
__global__ __launch_bounds__(RDT_THREADS) void k_redetect_final(const RedetectArgs a) {
    __shared__ unsigned long long s_red[RDT_THREADS];
    const int tid = threadIdx.x, srch = blockIdx.x;
    const int item = srch / a.n_tracks, t = srch - item * a.n_tracks;
    const RdtSearch s = rdt_search(a, item, t);
    MatchRecord *out = a.out + (size_t)item * (size_t)a.n_tracks + (size_t)t;
    if (!s.active) {   // rule L1: no frame byte read, no centre stored
        if (tid == 0) {
            MatchRecord rec;
            rec.x = s.x;
            rec.y = s.y;
            rec.dx = rec.dy = 0;
            rec.cost = rec.second = -1;
            rec.status = RDT_SKIPPED;
            rec.pad = 0;
            *out = rec;
        }
        return;
    }
    const int p = rdt_clampi(a.p, FFL_MATCH_MAX_P) < 1 ? 1 : rdt_clampi(a.p, FFL_MATCH_MAX_P);
    const int P = 2 * p + 1, NP = P * P;
    const unsigned long long *scr = a.scr + (size_t)srch * (size_t)a.sstride;
    const size_t ntiles = (size_t)a.TX * (size_t)a.TY;
    const long long bcost = (long long)scr[ntiles];
    const unsigned long long pos = scr[ntiles + 1];
    const int by = (int)(pos / (unsigned long long)a.w), bx = (int)(pos - (unsigned long long)by * (unsigned long long)a.w);
    const RdtExcl q = rdt_excl(a, bx, by);
    const int nx = s.tx1 - s.tx0 + 1, ny = s.ty1 - s.ty0 + 1;
    unsigned long long k2 = RDT_NONE;
    for (long long k = tid; k < (long long)nx * ny; k += RDT_THREADS) {
        const int ty = s.ty0 + (int)(k / nx), tx = s.tx0 + (int)(k % nx);
        if (tx >= q.ex0 && tx <= q.ex1 && ty >= q.ey0 && ty <= q.ey1) continue;   // re-walked below
        const unsigned long long key = scr[(size_t)ty * (size_t)a.TX + (size_t)tx];
        if (key != RDT_NONE && (key >> 10) < k2) k2 = key >> 10;
    }
    const int enx = q.ex1 - q.ex0 + 1, eny = q.ey1 - q.ey0 + 1;
    if (tid < enx * eny) {
        const unsigned long long key = scr[ntiles + 2 + (size_t)((tid / enx) * q.nx + tid % enx)];
        if (key != RDT_NONE && (key >> 10) < k2) k2 = key >> 10;
    }
    const unsigned long long sec = rdt_block_min(k2, s_red, tid);
    const unsigned char *Tm = a.tmpl + (size_t)t * (size_t)NP;
    unsigned long long t1 = 0, t2 = 0;
    for (int k = tid; k < NP; k += RDT_THREADS) {
        const unsigned long long v = Tm[k];
        t1 += v;
        t2 += v * v;
    }
    const long long T1 = (long long)rdt_block_sum(t1, s_red, tid);
    const long long T2 = (long long)rdt_block_sum(t2, s_red, tid);
    if (tid == 0) {
        const double dN = (double)NP;
        const long long second = sec == RDT_NONE ? -1ll : (long long)sec;
        const long long tvar = (long long)NP * T2 - T1 * T1;
        int status = 0;
        if ((double)tvar < a.min_var * dN * dN) status |= MCH_FLAT;               // L6: FLAT and POOR are N6's
        if ((double)bcost > a.max_mse * dN * dN) status |= MCH_POOR;
        if (second >= 0 && (double)bcost >= a.ratio * (double)second) status |= MCH_AMBIGUOUS;   // >=, not N6's >
        MatchRecord rec;
        rec.x = s.x;
        rec.y = s.y;
        if (status == 0) {                                                        // L7
            rec.x = rdt_clamp((double)bx, (double)(a.w - 1));
            rec.y = rdt_clamp((double)by, (double)(a.h - 1));
        }
        rec.dx = bx - s.ix;
        rec.dy = by - s.iy;
        rec.cost = bcost;
        rec.second = second;
        rec.status = status;
        rec.pad = 0;
        *out = rec;
        if (a.write_back && status == 0) {                                        // L8
            s.cp[0] = rec.x;
            s.cp[1] = rec.y;
        }
    }
}

// The four launches of one call, in stream order: sweep, pick, the exclusion sweep, final.  a.gx, a.gy, a.ex, a.ey are the
// host's grid sizes (ffl_redetect_grid); every kernel derives its tiles from them and from the anchor again.
void ffl_launch_track_redetect(const RedetectArgs &a, int n, hipStream_t st) {
    const unsigned searches = (unsigned)(n * a.n_tracks);
    hipLaunchKernelGGL(k_redetect_sweep<false>, dim3((unsigned)(a.gx * a.gy), searches), dim3(RDT_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_redetect_pick, dim3(searches), dim3(RDT_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_redetect_sweep<true>, dim3((unsigned)(a.ex * a.ey), searches), dim3(RDT_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_redetect_final, dim3(searches), dim3(RDT_THREADS), 0, st, a);
}
