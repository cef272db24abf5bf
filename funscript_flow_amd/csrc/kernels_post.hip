// gfx950 kernels for the reference's numpy post path on a resident flow field:
//   pass 1: max_divergence (FunscriptFlow.pyw:748-758) + mean flow magnitude (FF:889-890)
//   pass 2: radial_motion_weighted (FF:761-785)
// Both are single-read streaming reductions over the (h, w, 2) float flow: HBM-bound, 8 B per pixel.
// Reductions are wave-shuffle -> LDS -> one partial per workgroup -> a small second kernel, so sums
// are reproducible run to run (no float atomics).
#include "ffl_kernels.h"
#include <cassert>
#include <cfloat>
#include <type_traits>

#define P1_THREADS 256
#define P1_RG 16          // rows a wave walks down (its row group)
#ifndef P1_G
#define P1_G 16            // rows of it whose loads are in flight together in k_pass1 (4: 118 us, 8: 111, 16: 105 at 1080p B = 32)
#endif
#define P1_STRIP 126      // useful pixels of a pass-1 strip: 64 lanes x 2 pixels minus one halo pixel per side
#define P2_STRIP 128      // pass 2 needs no halo
#ifndef P2_AXES_G
#define P2_AXES_G 2        // rows in flight per lane in the four-component RadialSums: 48 VGPRs, 8 waves per SIMD (8 rows, the single
                           // component's: 80 VGPRs, 6 waves); chosen by measurement over 8 and 4 rows -- DESIGN.md section 15
#endif

// Both passes walk the flow field in column strips: a wave owns 128 consecutive pixels of a row (two per
// lane, one 16-byte load) and walks down P1_RG rows, so every pixel is read once with full-width loads,
// the vertical neighbours of pass 1 are the previous / next row already in registers and the horizontal
// ones come from the adjacent lanes.  No per-pixel index division, no neighbour gathers.
static inline int ffl_strip_waves(int w, int h, int strip) {
    return ((w + strip - 1) / strip) * ((h + P1_RG - 1) / P1_RG);
}
// workgroups (= partial results) per item: four waves each.  Pass 1's count is the larger one (P1_STRIP < P2_STRIP), so
// scratch sized by it serves both passes.
int ffl_pass1_blocks(int w, int h) { return (ffl_strip_waves(w, h, P1_STRIP) + 3) / 4; }
int ffl_radial_blocks(int w, int h) { return (ffl_strip_waves(w, h, P2_STRIP) + 3) / 4; }

// np.gradient along one axis: central difference /2 inside, one-sided at the ends (FF:754)
__device__ __forceinline__ float ffl_grad(float lo, float hi, int idx, int n) {
    return (idx == 0 || idx == n - 1) ? hi - lo : (hi - lo) / 2.0f;
}

__device__ __forceinline__ float ffl_div_at(const float2 *__restrict__ flow, int w, int h, int x, int y) {
    int ya = y == 0 ? 0 : y - 1, yb = y == h - 1 ? h - 1 : y + 1;
    int xa = x == 0 ? 0 : x - 1, xb = x == w - 1 ? w - 1 : x + 1;
    float du = ffl_grad(ffl_gload2(flow, 8u * ((size_t)ya * w + x)).x, ffl_gload2(flow, 8u * ((size_t)yb * w + x)).x, y, h);   // d(u)/dy
    float dv = ffl_grad(ffl_gload2(flow, 8u * ((size_t)y * w + xa)).y, ffl_gload2(flow, 8u * ((size_t)y * w + xb)).y, x, w);   // d(v)/dx
    return du + dv;
}

// the lane's two pixels (x, x+1) of row y, each clamped into the image, with one 16-byte load
__device__ __forceinline__ void ffl_load_pair(const float2 *__restrict__ flow, int w, int h, int x, int y, float2 &p0,
                                              float2 &p1) {
    const int yc = min(max(y, 0), h - 1);
    const int xa = min(max(x, 0), w - 2);  // pair start inside the row
    const float4 t = ffl_gload4(flow, 8u * ((unsigned)yc * (unsigned)w + (unsigned)xa))  /* < 2^32: ffl_create */;
    const float2 A = make_float2(t.x, t.y), B = make_float2(t.z, t.w);
    p0 = (min(max(x, 0), w - 1) == xa) ? A : B;
    p1 = (min(max(x + 1, 0), w - 1) == xa) ? A : B;
}

__device__ __forceinline__ unsigned long long ffl_wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ double ffl_wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Where pass 1 reads its field.  load(yc, xa) is the 16-byte window of pixels (xa, xa + 1) of row yc as float4 (u, v, u,
// v); store() hands over the pixels a lane owns (the importing loader writes them into their flow slot).
struct P1SlotSrc {   // a flow slot: (h, w, 2) float32, one 16-byte load
    const float2 *flow;
    int w;
    __device__ __forceinline__ float4 load(int yc, int xa) const {
        return ffl_gload4(flow, 8u * ((unsigned)yc * (unsigned)w + (unsigned)xa));  // < 2^32: ffl_create
    }
    __device__ __forceinline__ void store(int, int, float2, float2, bool, bool) const {}
};

// Whether and where a pass reads per-pixel weights.  WtNone compiles every weighted
// statement away: k_pass1, k_import_pass1 and the k_strip_sums instantiations without maps carry no trace of it.  WtBytes is
// one item's (h, w) uint8 map with any base and row pitch: a lane reads the weight of each of its two pixels with a byte
// load at the pixel's clamped (x, y), so no byte outside the `w` bytes of a row is read and nothing is asked of alignment
// (pass 1's strips start at odd x).
struct WtNone {
    static constexpr bool on = false;
    __device__ __forceinline__ unsigned load(int, int) const { return 1u; }
};
struct WtBytes {
    static constexpr bool on = true;
    const char *item;    // the map's (0, 0)
    long long pitch;     // bytes
    __device__ __forceinline__ unsigned load(int yc, int xc) const {   // 0 <= yc < h, 0 <= xc < w
        return *(const FFL_GLOBAL unsigned char *)(item + (long long)yc * pitch + xc);
    }
};

// key = (bits(|div|) << 32) | (0xFFFFFFFF - flat index): the maximum key is the largest |div| and,
// among equals, the smallest row-major index -- np.argmax's first-occurrence rule, order independent.
// np.argmax ranks every NaN above every number and takes the first one, whatever its payload: a NaN |div| enters the
// key as one bit pattern (above +inf), so among NaNs the index decides as it does among equal numbers.
__device__ __forceinline__ unsigned ffl_key_bits(float absdiv) {
    return absdiv != absdiv ? 0x7FC00000u : __float_as_uint(absdiv);
}
// The body of k_pass1 and k_import_pass1: one summation order whatever the source, so an imported field's record is
// bit-identical to the record of the same float32 field in a slot.
// Wt::on (k_pass1_weighted, rules W1-W3): a pixel is a candidate of the argmax and a term of the sums only where its weight
// is > 0 -- by the selects that already exclude halo pixels, so nothing of an excluded pixel's flow reaches a key or a sum;
// its magnitude enters as (double)mag * (double)weight (exact) and SW = sum of the weights travels as one more float64
// partial per workgroup (psw; ssw: 4 doubles of LDS).  The divergence itself is today's, from today's neighbours.
template <class Src, class Wt>
__device__ __forceinline__ void ffl_pass1_body(const Src &src, const Wt &wt, int w, int h, int pov_mode, int b,
                                               unsigned long long *__restrict__ pkey, double *__restrict__ psum,
                                               unsigned long long *skey, double *ssum, double *__restrict__ psw = nullptr,
                                               double *ssw = nullptr) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nstrips = (w + P1_STRIP - 1) / P1_STRIP, ngroups = (h + P1_RG - 1) / P1_RG;
    const int wid = blockIdx.x * (P1_THREADS / 64) + wv;  // wave-uniform
    unsigned long long key = 0;
    double sum = 0.0;
    [[maybe_unused]] double sw = 0.0;
    if (wid < nstrips * ngroups) {
        const int grp = wid / nstrips, strip = wid - grp * nstrips;
        const int x = strip * P1_STRIP - 1 + 2 * lane, y0 = grp * P1_RG;  // the lane's pixels: x, x+1
        // a pixel counts if it is inside the image and not one of the strip's two halo pixels
        const bool ok0 = lane > 0 && x < w, ok1 = lane < 63 && x + 1 < w;
        // Two groups of 8 rows.  All 10 rows a group needs are requested before anything is computed: written as one
        // loop (load row y + 1, use rows y - 1 .. y + 1) the compiler put a full wait behind every load -- the uniform
        // `pov_mode` branch and the lane exchanges sit between them -- and a wave paid 18 dependent round trips.
        const int xa = min(max(x, 0), w - 2);   // the lane's 16-byte window starts here (inside the row)
        const bool first0 = min(max(x, 0), w - 1) == xa, first1 = min(max(x + 1, 0), w - 1) == xa;
#pragma unroll 1
        for (int g = 0; g < P1_RG; g += P1_G) {
            float4 raw[P1_G + 2];
            [[maybe_unused]] unsigned q0[P1_G], q1[P1_G];   // the weights of the group's own rows (the halo rows need none)
#pragma unroll
            for (int r = 0; r < P1_G + 2; r++) {
                const int yc = min(max(y0 + g - 1 + r, 0), h - 1);   // clamped: rows past the end repeat row h-1
                raw[r] = src.load(yc, xa);
                if constexpr (Wt::on) {
                    if (r >= 1 && r <= P1_G) {   // in flight with the flow rows
                        q0[r - 1] = wt.load(yc, min(max(x, 0), w - 1));
                        q1[r - 1] = wt.load(yc, min(max(x + 1, 0), w - 1));
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < P1_G; r++) {
                const int y = y0 + g + r;
                const float4 tu = raw[r], tc = raw[r + 1], td = raw[r + 2];
                const float2 up0 = first0 ? make_float2(tu.x, tu.y) : make_float2(tu.z, tu.w), up1 = first1 ? make_float2(tu.x, tu.y) : make_float2(tu.z, tu.w);
                const float2 c0 = first0 ? make_float2(tc.x, tc.y) : make_float2(tc.z, tc.w), c1 = first1 ? make_float2(tc.x, tc.y) : make_float2(tc.z, tc.w);
                const float2 dn0 = first0 ? make_float2(td.x, td.y) : make_float2(td.z, td.w), dn1 = first1 ? make_float2(td.x, td.y) : make_float2(td.z, td.w);
                const bool row_ok = y < h;
                src.store(y, x, c0, c1, ok0 && row_ok, ok1 && row_ok);
                bool in0 = ok0 && row_ok, in1 = ok1 && row_ok;
                if constexpr (Wt::on) {
                    in0 = in0 && q0[r] > 0u;
                    in1 = in1 && q1[r] > 0u;
                    sum += in0 ? (double)sqrtf(c0.x * c0.x + c0.y * c0.y) * (double)q0[r] : 0.0;
                    sum += in1 ? (double)sqrtf(c1.x * c1.x + c1.y * c1.y) * (double)q1[r] : 0.0;
                    sw += in0 ? (double)q0[r] : 0.0;
                    sw += in1 ? (double)q1[r] : 0.0;
                } else {
                    sum += in0 ? (double)sqrtf(c0.x * c0.x + c0.y * c0.y) : 0.0;
                    sum += in1 ? (double)sqrtf(c1.x * c1.x + c1.y * c1.y) : 0.0;
                }
                if (!pov_mode) {
                    // horizontal neighbours: the adjacent lanes' pixels (clamped loads make x = 0 / w-1 see themselves)
                    const float left0 = __shfl_up(c1.y, 1, 64), right1 = __shfl_down(c0.y, 1, 64);
                    const float d0 = fabsf(ffl_grad(up0.x, dn0.x, y, h) + ffl_grad(left0, c1.y, x, w));
                    const float d1 = fabsf(ffl_grad(up1.x, dn1.x, y, h) + ffl_grad(c0.y, right1, x + 1, w));
                    const unsigned i0 = (unsigned)y * (unsigned)w + (unsigned)x;
                    if (in0) {
                        const unsigned long long k = ((unsigned long long)ffl_key_bits(d0) << 32) | (unsigned long long)(0xFFFFFFFFu - i0);
                        key = k > key ? k : key;
                    }
                    if (in1) {
                        const unsigned long long k = ((unsigned long long)ffl_key_bits(d1) << 32) | (unsigned long long)(0xFFFFFFFFu - (i0 + 1u));
                        key = k > key ? k : key;
                    }
                }
            }
        }
    }
    key = ffl_wave_max_u64(key);
    sum = ffl_wave_sum_f64(sum);
    if constexpr (Wt::on) sw = ffl_wave_sum_f64(sw);
    if (lane == 0) {
        skey[wv] = key;
        ssum[wv] = sum;
        if constexpr (Wt::on) ssw[wv] = sw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < P1_THREADS / 64; i++) {
            key = skey[i] > key ? skey[i] : key;
            sum += ssum[i];
            if constexpr (Wt::on) sw += ssw[i];
        }
        pkey[(size_t)b * gridDim.x + blockIdx.x] = key;
        psum[(size_t)b * gridDim.x + blockIdx.x] = sum;
        if constexpr (Wt::on) psw[(size_t)b * gridDim.x + blockIdx.x] = sw;
    }
}

__global__ __launch_bounds__(P1_THREADS) void k_pass1(const PairTab *__restrict__ pt, int w, int h, int pov_mode,
                                                      unsigned long long *__restrict__ pkey,
                                                      double *__restrict__ psum) {
    __shared__ unsigned long long skey[P1_THREADS / 64];
    __shared__ double ssum[P1_THREADS / 64];
    const int b = blockIdx.y;
    const P1SlotSrc src{reinterpret_cast<const float2 *>(pt->flow[0][b]), w};
    ffl_pass1_body(src, WtNone{}, w, h, pov_mode, b, pkey, psum, skey, ssum);
}

// The body of k_pass1_final and k_pass1_weighted_final: item b's nblk partials in one order, then its record.  The record
// under a map (WT) is marked `weighted` and holds the quotient by SW instead of the sum (rule W5 when SW == 0).
template <bool WT>
__device__ __forceinline__ void ffl_pass1_final_body(const PairTab *__restrict__ pt, int w, int h, int pov_mode, int nblk,
                                                     const unsigned long long *__restrict__ pkey,
                                                     const double *__restrict__ psum, const double *__restrict__ psw,
                                                     unsigned long long *skey, double *ssum, double *ssw) {
    const int b = blockIdx.x;
    unsigned long long key = 0;
    double sum = 0.0;
    [[maybe_unused]] double sw = 0.0;
    for (int i = threadIdx.x; i < nblk; i += P1_THREADS) {
        unsigned long long k = pkey[(size_t)b * nblk + i];
        key = k > key ? k : key;
        sum += psum[(size_t)b * nblk + i];
        if constexpr (WT) sw += psw[(size_t)b * nblk + i];
    }
    key = ffl_wave_max_u64(key);
    sum = ffl_wave_sum_f64(sum);
    if constexpr (WT) sw = ffl_wave_sum_f64(sw);
    int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        skey[wv] = key;
        ssum[wv] = sum;
        if constexpr (WT) ssw[wv] = sw;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < P1_THREADS / 64; i++) {
            key = skey[i] > key ? skey[i] : key;
            sum += ssum[i];
            if constexpr (WT) sw += ssw[i];
        }
        Pass1Result r;
        bool empty = false;
        if constexpr (WT) empty = sw == 0.0;
        if (empty) {  // rule W5: no candidate, no term; mag_sum / divisor = +0.0 without a division by zero
            r.x = w / 2;
            r.y = h / 2;
            r.div_val = 0.f;
        } else if (pov_mode) {  // FF:880-882: centre of the bottom edge, value 0
            r.x = w / 2;
            r.y = h - 1;
            r.div_val = 0.f;
        } else {
            unsigned idx = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
            r.y = idx / w;
            r.x = idx - r.y * w;
            r.div_val = ffl_div_at(reinterpret_cast<const float2 *>(pt->flow[0][b]), w, h, r.x, r.y);
        }
        r.weighted = WT ? 1 : 0;
        r.mag_sum = sum;
        if constexpr (WT) r.mag_sum = empty ? 0.0 : sum / (empty ? 1.0 : sw);   // one IEEE division; none by zero
        *pt->res[b] = r;
    }
}

__global__ __launch_bounds__(P1_THREADS) void k_pass1_final(const PairTab *__restrict__ pt, int w, int h, int pov_mode,
                                                            int nblk, const unsigned long long *__restrict__ pkey,
                                                            const double *__restrict__ psum) {
    __shared__ unsigned long long skey[P1_THREADS / 64];
    __shared__ double ssum[P1_THREADS / 64];
    ffl_pass1_final_body<false>(pt, w, h, pov_mode, nblk, pkey, psum, nullptr, skey, ssum, nullptr);
}

void ffl_launch_pass1(const PairTab *pt, int nB, int w, int h, int pov_mode, unsigned long long *pkey, double *psum,
                      hipStream_t st) {
    const int nblk = ffl_pass1_blocks(w, h);
    hipLaunchKernelGGL(k_pass1, dim3(nblk, nB), dim3(P1_THREADS), 0, st, pt, w, h, pov_mode, pkey, psum);
    hipLaunchKernelGGL(k_pass1_final, dim3(nB), dim3(P1_THREADS), 0, st, pt, w, h, pov_mode, nblk, pkey, psum);
}

// ---- pass 2: radial_motion_weighted, float64 ------------------------------------------------------
// wytab[y] = (double)(h - y) / h, wytab[h + y] = (double)y / h: the two row weights of FF:780-783, formed once per
// context on the host (IEEE division, the value the device's division yields).  The row index is wave-uniform, so the
// weight comes with a scalar load instead of a 15-instruction f64 division per lane and row -- the kernel had
// hoisted all 16 of them and needed 198 VGPRs (2 waves per SIMD).

// One pixel's terms into the lane's sums without maps: radial ((u dx + v dy) wx) wy and, with NC = FFL_NAXES, the three further
// components.  A pixel outside the image (`in` false) adds 0.0 by a select.
template <int NC>
__device__ __forceinline__ void ffl_radial_terms(double (&sum)[NC], bool in, float2 f, double dx, double dy, double wx, double wy) {
    const double u = (double)f.x, v = (double)f.y;
    sum[0] += in ? (u * dx + v * dy) * wx * wy : 0.0;
    if constexpr (NC > 1) {
        sum[1] += in ? (v * dx - u * dy) * wx * wy : 0.0;
        sum[2] += in ? u * wx * wy : 0.0;
        sum[3] += in ? v * wx * wy : 0.0;
    }
}

// What a launch takes as its maps: WeightArgs, or NoWeights for the forms without.  ffl_item_weights is item b's policy.
struct NoWeights {};
__device__ __forceinline__ WtNone ffl_item_weights(const NoWeights &, int) { return WtNone{}; }
__device__ __forceinline__ WtBytes ffl_item_weights(const WeightArgs &wa, int b) {
    return WtBytes{wa.base + (long long)b * wa.item, wa.pitch};   // rows wa.pitch bytes apart
}

// ---- the partial protocol of the strip sums: NS float64 sums per item, one partial of each per workgroup ----------------
// Sum c of workgroup g of item b of nblk workgroups: sum-major per item, so a collecting kernel reads a sum's partials with
// consecutive lanes.
template <int NS>
__device__ __forceinline__ size_t ffl_partial_index(int b, int c, int nblk, int g) {
    return ((size_t)b * NS + c) * nblk + g;
}

// The workgroup's tree: the wave sum of each of the lane's sums, then the four waves' through LDS (ssum: NS * 4 doubles), added
// in wave order by thread 0, which ends up holding the totals.
template <int NS, class WaveSum>
__device__ __forceinline__ void ffl_block_sums(double (&sum)[NS], double *ssum, WaveSum wave_sum) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NS; c++) {
        sum[c] = wave_sum(sum[c]);
        if (lane == 0) ssum[c * (P1_THREADS / 64) + wv] = sum[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NS; c++)
            for (int i = 1; i < P1_THREADS / 64; i++) sum[c] += ssum[c * (P1_THREADS / 64) + i];
    }
}

// A main kernel's end: the workgroup's sums become its partials of item b.
template <int NS, class WaveSum>
__device__ __forceinline__ void ffl_block_partials(double (&sum)[NS], double *ssum, double *__restrict__ psum, int b,
                                                   WaveSum wave_sum) {
    ffl_block_sums<NS>(sum, ssum, wave_sum);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < NS; c++) psum[ffl_partial_index<NS>(b, c, gridDim.x, blockIdx.x)] = sum[c];
    }
}

// A collecting kernel's start (one workgroup per item): item b's nblk partials of each sum strided over the workgroup's threads
// into sum[], which enters zeroed, then the same tree.
template <int NS>
__device__ __forceinline__ void ffl_collect_partials(double (&sum)[NS], double *ssum, const double *__restrict__ psum, int b,
                                                     int nblk) {
    for (int i = threadIdx.x; i < nblk; i += P1_THREADS) {
#pragma unroll
        for (int c = 0; c < NS; c++) sum[c] += psum[ffl_partial_index<NS>(b, c, nblk, i)];
    }
    ffl_block_sums<NS>(sum, ssum, ffl_wave_sum_f64);
}

// ---- the strip-sum walk: the main kernel of pass 2 (RadialSums) and of the motion fit (MotionSums, further down) --------------
// A wave owns P2_STRIP columns of a row group of P1_RG rows; a lane its two pixels x, x + 1 (one 16-byte load per row), whose
// terms enter the lane's P::NS float64 sums pixel x, then x + 1, row by row.  P::G rows of the row group have their loads in
// flight together: all G flow loads and, under maps, the byte loads at the flow's clamps are issued before any arithmetic.
// The policy P states what differs: skip(b), a workgroup-uniform way out before anything of the item is loaded; the item's
// field(b, w, h), weights(b) (WtNone / WtBytes) and scalars item(b, w, h), read with the wave-uniform item index; columns(), the
// per-column terms of the lane's two pixels, formed once; row(), row y's terms (ok0 / ok1: the column is in the image); wave_sum.
// It is a plain struct of what the launcher has to hand and is itself the kernel's argument: built inside the kernel or handed
// to a helper, the single-component form compiled to 5 waves per SIMD instead of 8 (profiles/r24_strip_sums_single_source.md).
template <class P>
__global__ __launch_bounds__(P1_THREADS) void k_strip_sums(const P p, int w, int h, double *__restrict__ psum) {
    constexpr int NS = P::NS, G = P::G;
    __shared__ double ssum[NS * (P1_THREADS / 64)];
    const int b = blockIdx.y;
    if (p.skip(b)) return;
    const float2 *flow = p.field(b, w, h);
    const auto wt = p.weights(b);
    const auto item = p.item(b, w, h);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nstrips = (w + P2_STRIP - 1) / P2_STRIP, ngroups = (h + P1_RG - 1) / P1_RG;
    const int wid = blockIdx.x * (P1_THREADS / 64) + wv;  // wave-uniform
    double sum[NS] = {};
    if (wid < nstrips * ngroups) {
        const int grp = wid / nstrips, strip = wid - grp * nstrips;
        const int x = strip * P2_STRIP + 2 * lane, y0 = grp * P1_RG;  // the lane's pixels: x, x+1
        const bool ok0 = x < w, ok1 = x + 1 < w;
        const auto col = p.columns(item, x, w);
#pragma unroll 1
        for (int g = 0; g < P1_RG; g += G) {
            float2 f0[G], f1[G];
            unsigned q0[G], q1[G];
#pragma unroll
            for (int r = 0; r < G; r++) {
                ffl_load_pair(flow, w, h, x, y0 + g + r, f0[r], f1[r]);
                const int yq = min(y0 + g + r, h - 1);   // the flow's clamps; in flight with the flow rows
                q0[r] = wt.load(yq, min(x, w - 1));
                q1[r] = wt.load(yq, min(x + 1, w - 1));
            }
            // Nothing is scheduled across this line.  Without it the compiler sinks row 1's loads of the fit's kernels behind row 0's
            // arithmetic, and the prior forms measured 2 to 5 % behind; pass 2's kernels compile to the same code either way.
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < G; r++) p.row(sum, item, col, y0 + g + r, h, ok0, ok1, f0[r], f1[r], q0[r], q1[r]);
        }
    }
    ffl_block_partials<NS>(sum, ssum, psum, b, P::wave_sum);
}

template <class P>
static void ffl_launch_strip_sums(const P &p, int n, int w, int h, double *psum, hipStream_t st) {
    hipLaunchKernelGGL(k_strip_sums<P>, dim3(ffl_radial_blocks(w, h), n), dim3(P1_THREADS), 0, st, p, w, h, psum);
}

// Pass 2's sums over a WindowItem table in device memory: ffl_radial copies one there, ffl_radial_window has k_window_plan write
// it.  Three instantiations: <1, 8, NoWeights> (ffl_radial, ffl_radial_window), <FFL_NAXES, P2_AXES_G, NoWeights> (DESIGN.md
// section 15) and <FFL_NAXES, P2_AXES_G, WeightArgs> (section 16).  One per-lane order and one wave / workgroup reduction order
// for every component, so the single- and the four-component forms give the same bits in component 0 for the same slot, centre
// and pov_mode.  Components 1..3 reuse the pixel's u, v, dx, dy and weights: tangential ((v dx - u dy) wx)
// wy, shift_x (u wx) wy, shift_y (v wx) wy.
// Under maps (rule W4) SW = sum of the weights is one more component, index NC: NS = NC + 1 sums per item and workgroup.  A cut
// item is skipped (FF:766-767, rule W6), and the final kernel answers it +0.0.
// G = 8 for the single component, two groups of 8 rows: 8 row loads in flight per lane are enough to cover the latency, and the
// unrolled body holds 8 waves per SIMD (64 VGPRs; all 16 rows hoisted needed 191).
template <int NC, int G_, class WA>
struct RadialSums {
    using Wt = decltype(ffl_item_weights(WA{}, 0));
    static constexpr int G = G_, NS = NC + (Wt::on ? 1 : 0);   // sums per lane
    const WindowItem *tab;
    int pov_mode;
    const double *wytab;
    WA wa;
    struct Item { double cx, cy; };
    struct Columns { double dx0, dx1, wx0, wx1; };   // dx and the quadrant weight (w - x) / w or x / w (FF:776-779)
    __device__ __forceinline__ bool skip(int b) const { return tab[b].cut; }
    __device__ __forceinline__ const float2 *field(int b, int, int) const { return reinterpret_cast<const float2 *>(tab[b].flow); }
    __device__ __forceinline__ Wt weights(int b) const { return ffl_item_weights(wa, b); }
    __device__ __forceinline__ Item item(int b, int, int) const { return Item{tab[b].cx, tab[b].cy}; }
    __device__ __forceinline__ Columns columns(const Item &it, int x, int w) const {
        const double cx = it.cx, dw = (double)w;
        return Columns{(double)x - cx, (double)(x + 1) - cx,
                       pov_mode ? 1.0 : (((double)x > cx) ? (double)(w - x) / dw : (double)x / dw),
                       pov_mode ? 1.0 : (((double)(x + 1) > cx) ? (double)(w - x - 1) / dw : (double)(x + 1) / dw)};
    }
    __device__ __forceinline__ void row(double (&sum)[NS], const Item &it, const Columns &c, int y, int h, bool ok0, bool ok1,
                                        float2 f0, float2 f1, unsigned q0, unsigned q1) const {
        const int yc = min(y, h - 1);  // rows past the image contribute nothing (selected out in the terms)
        const double dx0 = c.dx0, dx1 = c.dx1, wx0 = c.wx0, wx1 = c.wx1, cy = it.cy;
        const double dy = (double)y - cy;
        const double wy = pov_mode ? 1.0 : (((double)y > cy) ? wytab[yc] : wytab[h + yc]);
        if constexpr (Wt::on) {
            // Rule W4, written out: stated through ffl_radial_terms with the predicate and the factor hoisted, this
            // instantiation measured behind at 256 items of 256x256 (profiles/r22_pass2_single_source.md).  Every term
            // is the unweighted one times (double)weight as its last factor, and enters only where the weight is > 0.
            static_assert(NC == FFL_NAXES, "the weighted form is the four-component one");
            const bool in0 = ok0 && y < h && q0 > 0u, in1 = ok1 && y < h && q1 > 0u;
            const double p0 = (double)q0, p1 = (double)q1;
            const double t0 = ((double)f0.x * dx0 + (double)f0.y * dy) * wx0 * wy;
            const double t1 = ((double)f1.x * dx1 + (double)f1.y * dy) * wx1 * wy;
            const double u0 = (double)f0.x, v0 = (double)f0.y, u1 = (double)f1.x, v1 = (double)f1.y;
            const double a0 = (v0 * dx0 - u0 * dy) * wx0 * wy, a1 = (v1 * dx1 - u1 * dy) * wx1 * wy;
            sum[0] += in0 ? t0 * p0 : 0.0;
            sum[0] += in1 ? t1 * p1 : 0.0;
            sum[1] += in0 ? a0 * p0 : 0.0;
            sum[1] += in1 ? a1 * p1 : 0.0;
            sum[2] += in0 ? u0 * wx0 * wy * p0 : 0.0;
            sum[2] += in1 ? u1 * wx1 * wy * p1 : 0.0;
            sum[3] += in0 ? v0 * wx0 * wy * p0 : 0.0;
            sum[3] += in1 ? v1 * wx1 * wy * p1 : 0.0;
            sum[NC] += in0 ? p0 : 0.0;
            sum[NC] += in1 ? p1 : 0.0;
        } else {
            ffl_radial_terms<NC>(sum, ok0 && y < h, f0, dx0, dy, wx0, wy);
            ffl_radial_terms<NC>(sum, ok1 && y < h, f1, dx1, dy, wx1, wy);
        }
    }
    static __device__ __forceinline__ double wave_sum(double v) { return ffl_wave_sum_f64(v); }
};

// The final kernel of the pair: each component's nblk partials of item b in one order, then its means into out[b] -- `dot` of a
// Pass2Record (NC = 1), or the four components of an AxesRecord and reserved = +0.0; whoever planned the item wrote the rest of
// the record.  A cut item's partials were never written: its means are +0.0.
// WT: NS = NC + 1 sums per item, the last one SW, which replaces the pixel count as the one divisor; SW == 0 (rule W5) divides
// the all-zero sums by 1.0 instead, +0.0 without a division by zero.
template <int NC, bool WT, class Rec>
__global__ __launch_bounds__(P1_THREADS) void k_radial_final(const WindowItem *__restrict__ tab, int w, int h, int nblk,
                                                             const double *__restrict__ psum, Rec *__restrict__ out) {
    constexpr int NS = NC + (WT ? 1 : 0);
    __shared__ double ssum[NS * (P1_THREADS / 64)];
    const int b = blockIdx.x;
    double sum[NS] = {};
    if (!tab[b].cut) {   // workgroup-uniform
        ffl_collect_partials<NS>(sum, ssum, psum, b, nblk);
        if (threadIdx.x == 0) {
            double divisor = (double)w * (double)h;
            if constexpr (WT) divisor = sum[NC] == 0.0 ? 1.0 : sum[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) sum[c] = sum[c] / divisor;
        }
    }
    if (threadIdx.x == 0) {
        if constexpr (NC == 1) {
            out[b].dot = sum[0];
        } else {
            out[b].base.dot = sum[0];
            out[b].tangential = sum[1];
            out[b].shift_x = sum[2];
            out[b].shift_y = sum[3];
            out[b].reserved = 0.0;
        }
    }
}

template <int NC, int G, class Rec, class WA>
static void ffl_radial_pair(const WindowItem *tab, int n, int w, int h, int pov_mode, const double *wytab, const WA &wa,
                            double *psum, void *out, hipStream_t st) {
    ffl_launch_strip_sums(RadialSums<NC, G, WA>{tab, pov_mode, wytab, wa}, n, w, h, psum, st);
    hipLaunchKernelGGL((k_radial_final<NC, std::is_same<WA, WeightArgs>::value, Rec>), dim3(n), dim3(P1_THREADS), 0, st, tab, w, h,
                       ffl_radial_blocks(w, h), psum, (Rec *)out);
}

void ffl_launch_radial(const WindowItem *tab, int n, int w, int h, int pov_mode, const double *wytab, const RadialForm &form,
                       double *psum, void *out, hipStream_t st) {
    assert((form.nc == 1 && !form.maps) || form.nc == FFL_NAXES);   // the three forms that exist
    if (form.maps)
        ffl_radial_pair<FFL_NAXES, P2_AXES_G, AxesRecord>(tab, n, w, h, pov_mode, wytab, *form.maps, psum, out, st);
    else if (form.nc == FFL_NAXES)
        ffl_radial_pair<FFL_NAXES, P2_AXES_G, AxesRecord>(tab, n, w, h, pov_mode, wytab, NoWeights{}, psum, out, st);
    else
        ffl_radial_pair<1, 8, Pass2Record>(tab, n, w, h, pov_mode, wytab, NoWeights{}, psum, out, st);
}

// ---- pass 2 behind the batches, host-free (ffl_radial_window) ---------------------------------
// k_window_plan<STRIDE, CEN>, then the radial pair.  One thread per item forms the clipped centre window, mean_mag and cut out of
// the pass-1 records and writes the device-resident WindowItem table plus every field of the record but `dot` (STRIDE: bytes
// from one record to the next; each starts with a Pass2Record).  The records
// are mapped pinned memory: a workgroup stages the (x, y) of the <= 64 + 2 * radius records its items' windows span in
// LDS, so the window costs one (x, y) read per record and workgroup instead of 2 * radius + 1 per item; each item then
// reads mag_sum and div_val of its own record once more.  Nothing of a record is read by the radial grid.
#define W2_THREADS 64

// CEN (k_window_plan<80, true>, DESIGN.md section 17 rule G6): the window's centres are the caller's, two doubles at the head
// of each of n_seq entries cstride bytes apart at cen, staged the same way and added in the order numpy adds the rows of
// FF:1205-1213's list -- item j, then j - i before j + i for i = 1..radius.  x and y of the record are still the slot's.
template <int STRIDE, bool CEN>
__global__ __launch_bounds__(W2_THREADS) void k_window_plan(const WindowSeq seq, int n_seq, int first, int n, int radius,
                                                            float cut_threshold, double npx, const Pass1Result *__restrict__ res,
                                                            const float *__restrict__ flow, size_t N, const char *__restrict__ cen,
                                                            long long cstride, WindowItem *__restrict__ tab,
                                                            char *__restrict__ out) {
    using T = typename std::conditional<CEN, double, int>::type;
    __shared__ T sx[W2_THREADS + 2 * FFL_WINDOW_MAX_RADIUS], sy[W2_THREADS + 2 * FFL_WINDOW_MAX_RADIUS];
    const int i0 = blockIdx.x * W2_THREADS;                      // the workgroup's first item
    const int j0 = first + i0, j1 = first + min(i0 + W2_THREADS, n) - 1;   // its items in seq, inclusive
    const int lo = max(0, j0 - radius), hi = min(n_seq - 1, j1 + radius);  // the records their windows span
    for (int k = lo + (int)threadIdx.x; k <= hi; k += W2_THREADS) {
        if constexpr (CEN) {
            const double *c = reinterpret_cast<const double *>(cen + (long long)k * cstride);
            sx[k - lo] = c[0];
            sy[k - lo] = c[1];
        } else {
            const Pass1Result *r = res + seq.slot[k];
            sx[k - lo] = r->x;
            sy[k - lo] = r->y;
        }
    }
    __syncthreads();
    const int i = i0 + (int)threadIdx.x;
    if (i >= n) return;
    const int j = first + i, slot = seq.slot[j];
    const int a = max(0, j - radius), b = min(n_seq - 1, j + radius);
    const double cnt = (double)(b - a + 1);
    double cx, cy;
    if constexpr (CEN) {
        double ax = sx[j - lo], ay = sy[j - lo];
        for (int d = 1; d <= radius; d++) {
            if (j - d >= 0) {
                ax += sx[j - d - lo];
                ay += sy[j - d - lo];
            }
            if (j + d < n_seq) {
                ax += sx[j + d - lo];
                ay += sy[j + d - lo];
            }
        }
        cx = ax / cnt;
        cy = ay / cnt;
    } else {
        long long tx = 0, ty = 0;                                // exact integer sums (np.mean of the int64 pairs)
        for (int k = a; k <= b; k++) {
            tx += sx[k - lo];
            ty += sy[k - lo];
        }
        cx = (double)tx / cnt;                                   // one IEEE division each: pipeline.smooth_centers
        cy = (double)ty / cnt;
    }
    const Pass1Result *r = res + slot;
    const float mm = (float)ffl_record_mean(*r, npx);            // ffl_pass1_results' expressions
    const int cut = mm > cut_threshold ? 1 : 0;                  // NaN > threshold is false
    WindowItem it;
    it.flow = flow + (size_t)slot * 2 * N;
    it.cx = cx;
    it.cy = cy;
    it.cut = cut;
    it.pad = 0;
    tab[i] = it;
    Pass2Record *o = reinterpret_cast<Pass2Record *>(out + (size_t)i * STRIDE);
    o->cx = cx;
    o->cy = cy;
    o->mean_mag = mm;
    o->div_val = r->div_val;
    if constexpr (CEN) {
        o->x = r->x;
        o->y = r->y;
    } else {
        o->x = sx[j - lo];
        o->y = sy[j - lo];
    }
    o->cut = cut;
    o->pad = 0;
}

// cen NULL: the centres are the records' argmax, rec_stride sizeof(Pass2Record) or sizeof(AxesRecord); else the caller's, the
// records AxesRecord
void ffl_launch_window_plan(const WindowSeq &seq, int n_seq, int first, int n, int radius, float cut_threshold,
                            const Pass1Result *res, const float *flow, int w, int h, const void *cen, long long cstride,
                            WindowItem *tab, void *out, int rec_stride, hipStream_t st) {
    constexpr int P2 = (int)sizeof(Pass2Record), AX = (int)sizeof(AxesRecord);
    const auto plan = cen ? k_window_plan<AX, true> : rec_stride == AX ? k_window_plan<AX, false> : k_window_plan<P2, false>;
    hipLaunchKernelGGL(plan, dim3((n + W2_THREADS - 1) / W2_THREADS), dim3(W2_THREADS), 0, st, seq, n_seq, first, n, radius,
                       cut_threshold, (double)w * (double)h, res, flow, (size_t)w * h, (const char *)cen, cstride, tab,
                       (char *)out);
}

// ---- per-cell statistics and the variance centre (ffl_cell_stats) ------------------
// center_of_mass_variance (FF:721-746) and its intermediate grid.  A reduction segmented by cell: workgroup (i, b) owns cell
// row i of item b and walks its G * gw columns in the 256-column blocks of rule G3, one column per lane.  A lane sums its
// column's gh rows top to bottom (CS_G rows of loads in flight), the column sums go through LDS, and one lane per cell
// segment of the block adds its columns left to right and then adds that block partial to the cell's sums, which stay in
// LDS from block to block: ascending block order without scratch partials, atomics or a ticket.  After the last block one
// lane per cell forms its record (rule G4) and lane 0 the row's t_i and x_i of rule G5, sequentially over j.
// k_grid_centre (the second launch) adds the G rows of an item in order and writes its centre record.
#define CS_THREADS 256   // = the column block of rule G3
#ifndef CS_G
#define CS_G 4           // rows whose loads are in flight together per lane (1080p n = 32, G = 32, gh = 33: 140 us with 4, 144 with 8,
                         // 153 with 16 -- a group re-reads the cell's last row for the rows it has past the cell's end: 3, 7, 15 of them)
#endif

__global__ __launch_bounds__(CS_THREADS) void k_cell_stats(const float *__restrict__ flow, const ExportTab tab, int w, int h, int G,
                                                           int gw, int gh, CellRecord *__restrict__ cells,
                                                           double *__restrict__ rowsum) {
    __shared__ double scol[CS_THREADS][4];      // the block's column sums: S_u, S_v, S_d, S_dd of a column side by side
    __shared__ double scell[4][FFL_CELLS_MAX];  // the row's cell sums so far
    __shared__ double svar[FFL_CELLS_MAX];
    const int i = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const float *f = flow + (size_t)tab.slot[b] * 2 * ((size_t)w * h);
    const int y0 = i * gh, wc = G * gw;         // rows y0 .. y0 + gh - 1; columns >= wc belong to no cell (rule G1)
    if (t < G) {
#pragma unroll
        for (int c = 0; c < 4; c++) scell[c][t] = 0.0;
    }
    const int nblk = (wc + CS_THREADS - 1) / CS_THREADS;
#pragma unroll 1
    for (int blk = 0; blk < nblk; blk++) {
        const int x = blk * CS_THREADS + t;
        const int xc = min(x, wc - 1);          // lanes past the last cell column repeat it; their sums are never read
        const int j = xc / gw;
        // K: the magnitude of the cell's top-left pixel (rule G2).  Byte offsets < 2^32: ffl_create
        const float2 k2 = ffl_gload2(f, 8u * ((unsigned)y0 * (unsigned)w + (unsigned)(j * gw)));
        const double K = (double)sqrtf(k2.x * k2.x + k2.y * k2.y);
        double su = 0.0, sv = 0.0, sd = 0.0, sdd = 0.0;
#pragma unroll 1
        for (int g = 0; g < gh; g += CS_G) {
            float2 p[CS_G];
#pragma unroll
            for (int r = 0; r < CS_G; r++) {    // rows past the cell repeat its last row (selected out below)
                const int y = y0 + min(g + r, gh - 1);
                p[r] = ffl_gload2(f, 8u * ((unsigned)y * (unsigned)w + (unsigned)xc));
            }
#pragma unroll
            for (int r = 0; r < CS_G; r++) {
                const bool in = g + r < gh;     // workgroup-uniform
                const double d = (double)sqrtf(p[r].x * p[r].x + p[r].y * p[r].y) - K;
                su += in ? (double)p[r].x : 0.0;
                sv += in ? (double)p[r].y : 0.0;
                sd += in ? d : 0.0;
                sdd += in ? d * d : 0.0;
            }
        }
        scol[t][0] = su;
        scol[t][1] = sv;
        scol[t][2] = sd;
        scol[t][3] = sdd;
        __syncthreads();
        // the cells that have columns in this block: jf .. jl (at most FFL_CELLS_MAX = CS_THREADS / 4 of them), one lane per
        // cell and sum.  The additions are sequential by rule G3; the LDS reads are not, so they go eight at a time.
        const int xb = blk * CS_THREADS, xl = min(xb + CS_THREADS, wc);
        const int jf = xb / gw, jl = (xl - 1) / gw;
        const int seg = t >> 2, c = t & 3;
        if (seg <= jl - jf) {
            const int jc = jf + seg;
            const int xs = max(jc * gw, xb) - xb, xe = min((jc + 1) * gw, xl) - xb;
            double part = 0.0;
            int k = xs;
            for (; k + 8 <= xe; k += 8) {
                double v[8];
#pragma unroll
                for (int r = 0; r < 8; r++) v[r] = scol[k + r][c];
#pragma unroll
                for (int r = 0; r < 8; r++) part += v[r];
            }
            for (; k < xe; k++) part += scol[k][c];
            scell[c][jc] += part;
        }
        __syncthreads();
    }
    if (t < G) {
        const float2 k2 = ffl_gload2(f, 8u * ((unsigned)y0 * (unsigned)w + (unsigned)(t * gw)));
        const double K = (double)sqrtf(k2.x * k2.x + k2.y * k2.y);
        const double n = (double)gh * (double)gw;
        const double sd = scell[2][t];
        double var = (scell[3][t] - sd * sd / n) / n;
        var = var < 0.0 ? 0.0 : var;            // a NaN stays a NaN (rule G4)
        svar[t] = var;
        if (cells) {
            CellRecord r;
            r.mean_u = scell[0][t] / n;
            r.mean_v = scell[1][t] / n;
            r.mean_mag = K + sd / n;
            r.var_mag = var;
            cells[((size_t)b * G + i) * G + t] = r;
        }
    }
    __syncthreads();
    if (t < 2) {                                // lane 0: t_i, lane 1: x_i, each over j in order (rule G5)
        double acc = 0.0;
        int j = 0;
        for (; j + 8 <= G; j += 8) {
            double v[8];
#pragma unroll
            for (int r = 0; r < 8; r++) v[r] = svar[j + r];
#pragma unroll
            for (int r = 0; r < 8; r++) acc += t ? (double)(j + r) * v[r] : v[r];
        }
        for (; j < G; j++) acc += t ? (double)j * svar[j] : svar[j];
        rowsum[((size_t)b * G + i) * 2 + t] = acc;
    }
}

__global__ __launch_bounds__(64) void k_grid_centre(const double *__restrict__ rowsum, int n, int w, int h, int G, int gw, int gh,
                                                    GridCentre *__restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    double T = 0.0, X = 0.0, Y = 0.0;
    for (int i = 0; i < G; i++) {
        const double ti = rowsum[((size_t)b * G + i) * 2], xi = rowsum[((size_t)b * G + i) * 2 + 1];
        T += ti;
        X += xi;
        Y += (double)i * ti;
    }
    GridCentre r;
    if (T == 0.0) {                             // FF:741-742; a NaN T takes the other branch and gives NaN centres
        r.cx = (double)(w / 2);
        r.cy = (double)(h / 2);
        r.empty = 1;
    } else {                                    // FF:744-745, left to right
        r.cx = X * (double)gw / T + (double)gw / 2.0;
        r.cy = Y * (double)gh / T + (double)gh / 2.0;
        r.empty = 0;
    }
    r.total_var = T;
    r.cells = G;
    out[b] = r;
}

void ffl_launch_cell_stats(const float *flow, const ExportTab &tab, int n, int w, int h, int G, CellRecord *cells,
                           GridCentre *centres, double *rowsum, hipStream_t st) {
    const int gw = w / G, gh = h / G;
    hipLaunchKernelGGL(k_cell_stats, dim3(G, n), dim3(CS_THREADS), 0, st, flow, tab, w, h, G, gw, gh, cells, rowsum);
    if (centres)
        hipLaunchKernelGGL(k_grid_centre, dim3((n + 63) / 64), dim3(64), 0, st, rowsum, n, w, h, G, gw, gh, centres);
}

// ---- flow export -----------------------------------------------------------------------------
// k_export_flows gathers flow slots into caller memory: (H, W, 2) with 16-byte copies, or (2, H, W) de-interleaved with
// 16-byte loads and stores on both sides.  Pure bandwidth.
// grid = (blocks per item, items); a lane handles FFL_EXP_UNROLL units of one item, 256 units apart.  Units: NHWC vec one
// float4 (2 pixels), NCHW vec 4 pixels (two float4 in, one float4 per plane out), scalar paths one pixel.
#define FFL_EXP_UNROLL 4

__global__ __launch_bounds__(256) void k_export_flows(const float *__restrict__ flow, ExportTab tab, size_t N,
                                                      char *__restrict__ dst, long long item_stride, int layout, int vec) {
    const float *src = flow + (size_t)tab.slot[blockIdx.y] * 2 * N;
    char *out = dst + (long long)blockIdx.y * item_stride;
    const size_t base = (size_t)blockIdx.x * (256 * FFL_EXP_UNROLL) + threadIdx.x;
    if (layout == 0) {
        if (vec) {  // 2N floats = N / 2 float4
            const float4 *s4 = (const float4 *)src;
            float4 *o4 = (float4 *)out;
            const size_t units = N / 2;
#pragma unroll
            for (int k = 0; k < FFL_EXP_UNROLL; k++) {
                const size_t u = base + (size_t)k * 256;
                if (u < units) o4[u] = s4[u];
            }
        } else {
            const float2 *s2 = (const float2 *)src;
            float *o = (float *)out;
#pragma unroll
            for (int k = 0; k < FFL_EXP_UNROLL; k++) {
                const size_t u = base + (size_t)k * 256;
                if (u < N) {
                    const float2 f = s2[u];
                    o[2 * u] = f.x;
                    o[2 * u + 1] = f.y;
                }
            }
        }
    } else {
        float *ou = (float *)out, *ov = ou + N;
        if (vec) {  // N % 4 == 0: 4 pixels = two float4 in, one float4 to each plane
            const float4 *s4 = (const float4 *)src;
            const size_t units = N / 4;
#pragma unroll
            for (int k = 0; k < FFL_EXP_UNROLL; k++) {
                const size_t u = base + (size_t)k * 256;
                if (u < units) {
                    const float4 a = s4[2 * u], b = s4[2 * u + 1];
                    ((float4 *)ou)[u] = make_float4(a.x, a.z, b.x, b.z);
                    ((float4 *)ov)[u] = make_float4(a.y, a.w, b.y, b.w);
                }
            }
        } else {
            const float2 *s2 = (const float2 *)src;
#pragma unroll
            for (int k = 0; k < FFL_EXP_UNROLL; k++) {
                const size_t u = base + (size_t)k * 256;
                if (u < N) {
                    const float2 f = s2[u];
                    ou[u] = f.x;
                    ov[u] = f.y;
                }
            }
        }
    }
}

void ffl_launch_export_flows(const float *flow, const ExportTab &tab, int n, size_t N, char *dst, long long item_stride,
                             int layout, hipStream_t st) {
    // 16-byte paths: every item base (and the v plane) 16-byte aligned; slot bases are (8N bytes apart) when N is even
    const bool aligned = ((uintptr_t)dst | (unsigned long long)item_stride) % 16 == 0;
    const int vec = aligned && (layout == 0 ? N % 2 == 0 : N % 4 == 0);
    const size_t units = vec ? (layout == 0 ? N / 2 : N / 4) : N;
    dim3 grid((unsigned)((units + 256 * FFL_EXP_UNROLL - 1) / (256 * FFL_EXP_UNROLL)), n);
    hipLaunchKernelGGL(k_export_flows, grid, dim3(256), 0, st, flow, tab, N, dst, item_stride, layout, vec);
}

// ---- forward-backward consistency maps -------------------------------------------
// k_consistency writes one uint8 weight per pixel from a forward field F and the backward field B sampled where F lands.
// grid = (blocks per item, items); a lane owns 4 consecutive pixels of a row (a quad): F is 32 streamed bytes (two 16-byte
// loads where the quad's address allows, four 8-byte loads otherwise), the four corners of B are two gathered 16-byte loads
// (the corners of a row are neighbours; 6 % faster than four float2 loads at 1080p), the gate is 4 bytes, the output one 4-byte
// store where its address allows.  No LDS, no loop, plain vector stores.  Rule K1: a pixel that lands outside reads nothing of
// B.  Bound by the address path of the gathers (TA 78 % busy, VALU 48 %, HBM at 2.7 TB/s).
struct __attribute__((aligned(8))) FlowPair {   // two neighbouring pixels of a field: 16 bytes at any pixel address
    float x, y, z, w;
};
__device__ __forceinline__ unsigned ffl_consistency_pixel(const float2 *__restrict__ B, float2 f, int x, int y, int w, int h,
                                                          float alpha, float beta, int soft) {
    const float u = f.x, v = f.y;
    const float px = (float)x + u, py = (float)y + v;
    const bool inside = px >= 0.0f && px <= (float)(w - 1) && py >= 0.0f && py <= (float)(h - 1);   // K1: NaN / inf fail
    if (!inside) return 0u;
    const float fx = floorf(px), fy = floorf(py);                                                     // K2
    const int x0 = (int)fx, y0 = (int)fy;
    const int y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;   // x1 = min(x0 + 1, w - 1): see the loads
    const float ax = px - fx, ay = py - fy;
    // The two corners of a row are neighbours in memory: one 16-byte load of pixels xs, xs + 1 with xs = min(x0, w - 2), so that
    // it never leaves the row.  x0 < w - 1: they are (x0, x1).  x0 = w - 1: x1 = x0 is the second of the two, for both corners.
    const unsigned r0 = (unsigned)y0 * (unsigned)w, r1 = (unsigned)y1 * (unsigned)w;   // 32-bit pixel offsets: 20 * w * h < 2^32
    const int xs = x0 < w - 2 ? x0 : w - 2;
    const FlowPair p0 = *(const FlowPair *)(B + (r0 + (unsigned)xs)), p1 = *(const FlowPair *)(B + (r1 + (unsigned)xs));
    const bool first = xs == x0;
    const float2 b01 = make_float2(p0.z, p0.w), b00 = first ? make_float2(p0.x, p0.y) : b01;
    const float2 b11 = make_float2(p1.z, p1.w), b10 = first ? make_float2(p1.x, p1.y) : b11;
    const float tu = b00.x + ax * (b01.x - b00.x), su = b10.x + ax * (b11.x - b10.x);
    const float bu = tu + ay * (su - tu);
    const float tv = b00.y + ax * (b01.y - b00.y), sv = b10.y + ax * (b11.y - b10.y);
    const float bv = tv + ay * (sv - tv);
    const float ex = u + bu, ey = v + bv, e2 = ex * ex + ey * ey;                                     // K3
    const float thr = alpha * ((u * u + v * v) + (bu * bu + bv * bv)) + beta;
    if (!soft) return e2 < thr ? 255u : 0u;                                                           // K5: no division
    float q = 1.0f - e2 / thr;                                                                        // K4
    q = q > 0.0f ? q : 0.0f;   // a select: a NaN gives 0
    return (unsigned)(int)(q * 255.0f + 0.5f);
}

__global__ __launch_bounds__(256) void k_consistency(const float *__restrict__ flow, ExportTab fwd, ExportTab bwd, int w, int h,
                                                     float alpha, float beta, int soft, WeightArgs gate, char *__restrict__ out,
                                                     long long out_item, long long out_pitch) {
    const int qw = (w + 3) >> 2;   // quads per row
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= (unsigned)qw * (unsigned)h) return;
    const int y = (int)(q / (unsigned)qw), x = (int)(q % (unsigned)qw) * 4;
    const int b = blockIdx.y, np = w - x < 4 ? w - x : 4;   // pixels of this quad
    const size_t N = (size_t)w * h;
    const float2 *F = (const float2 *)(flow + (size_t)fwd.slot[b] * 2 * N) + ((unsigned)y * (unsigned)w + (unsigned)x);
    const float2 *B = (const float2 *)(flow + (size_t)bwd.slot[b] * 2 * N);
    float2 f[4];
    if (np == 4 && ((uintptr_t)F & 15) == 0) {
        const float4 a = ((const float4 *)F)[0], c = ((const float4 *)F)[1];
        f[0] = make_float2(a.x, a.y), f[1] = make_float2(a.z, a.w), f[2] = make_float2(c.x, c.y), f[3] = make_float2(c.z, c.w);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) f[k] = k < np ? F[k] : make_float2(0.0f, 0.0f);
    }
    unsigned wt[4];
#pragma unroll
    for (int k = 0; k < 4; k++) wt[k] = k < np ? ffl_consistency_pixel(B, f[k], x + k, y, w, h, alpha, beta, soft) : 0u;
    if (gate.base) {   // K6
        const unsigned char *g = (const unsigned char *)gate.base + (long long)b * gate.item + (long long)y * gate.pitch + x;
        if (np == 4 && ((uintptr_t)g & 3) == 0) {
            const unsigned s = *(const unsigned *)g;
#pragma unroll
            for (int k = 0; k < 4; k++) wt[k] = min(wt[k], (s >> (8 * k)) & 255u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < np) wt[k] = min(wt[k], (unsigned)g[k]);
        }
    }
    unsigned char *o = (unsigned char *)out + (long long)b * out_item + (long long)y * out_pitch + x;
    if (np == 4 && ((uintptr_t)o & 3) == 0) {
        *(unsigned *)o = wt[0] | (wt[1] << 8) | (wt[2] << 16) | (wt[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < np) o[k] = (unsigned char)wt[k];
    }
}

void ffl_launch_consistency(const float *flow, const ExportTab &fwd, const ExportTab &bwd, int n, int w, int h, float alpha,
                            float beta, int soft, const WeightArgs *gate, char *out, long long out_item, long long out_pitch,
                            hipStream_t st) {
    const size_t quads = (size_t)((w + 3) / 4) * h;   // below 2^30: 20 * w * h < 2^32
    const WeightArgs g = gate ? *gate : WeightArgs{nullptr, 0, 0};
    hipLaunchKernelGGL(k_consistency, dim3((unsigned)((quads + 255) / 256), n), dim3(256), 0, st, flow, fwd, bwd, w, h, alpha, beta,
                       soft, g, out, out_item, out_pitch);
}

// ---- photometric-residual maps ---------------------------------------------------
// k_residual writes one uint8 weight per pixel from the gray operands I0, I1 of a pair and its forward field F: I1 sampled
// where F lands, against I0's pixel, measured by I0's local gradient.  k_consistency's form: grid = (blocks per item, items), a
// lane owns a quad of a row, F is 32 streamed bytes, gate and output 4 bytes each where their addresses allow.  The uint8 side:
// I0's centre quad and the quads of the rows above and below are one 4-byte load each where the address allows (bytes
// otherwise; a frame slot's rows are w bytes apart, so a width that is no multiple of 4 takes the byte form on most rows), its
// left and right neighbours one byte each, all with clamped edges; the four corners of I1 are four byte gathers at clamped
// coordinates, so that no access leaves the frame (rule P1: a pixel that lands outside reads nothing of I1).  No LDS, no loop,
// plain vector loads and stores, 32-bit pixel offsets inside a frame.  Bound by the address path of the byte gathers and
// loads, with the arithmetic close behind (1080p n = 32: TA 82 % busy, VALU 69 %, 2.1 TB/s fetched; 1.29 x k_export_flows'
// time, 0.71 x k_consistency's).
__device__ __forceinline__ unsigned ffl_load_quad_u8(const unsigned char *__restrict__ p, int np) {   // bytes p[0..np) packed
    if (np == 4 && ((uintptr_t)p & 3) == 0) return *(const unsigned *)p;
    unsigned r = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k < np) r |= (unsigned)p[k] << (8 * k);
    return r;
}

__device__ __forceinline__ unsigned ffl_residual_pixel(const unsigned char *__restrict__ I1, float2 f, int i0, int gx, int gy, int x,
                                                       int y, int w, int h, float alpha, float beta, int soft) {
    const float px = (float)x + f.x, py = (float)y + f.y;
    const bool inside = px >= 0.0f && px <= (float)(w - 1) && py >= 0.0f && py <= (float)(h - 1);   // P1: NaN / inf fail
    if (!inside) return 0u;
    const float fx = floorf(px), fy = floorf(py);                                                     // P2
    const int x0 = (int)fx, y0 = (int)fy;
    const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
    const float ax = px - fx, ay = py - fy;
    const unsigned r0 = (unsigned)y0 * (unsigned)w, r1 = (unsigned)y1 * (unsigned)w;   // 0 <= x0 <= x1 <= w-1, 0 <= y0 <= y1 <= h-1
    const float i00 = (float)I1[r0 + (unsigned)x0], i01 = (float)I1[r0 + (unsigned)x1];
    const float i10 = (float)I1[r1 + (unsigned)x0], i11 = (float)I1[r1 + (unsigned)x1];
    const float t = i00 + ax * (i01 - i00), s = i10 + ax * (i11 - i10);
    const float ic = t + ay * (s - t);
    const float a = fabsf(ic - (float)i0);                                                            // P3
    const float g = fabsf((float)gx) + fabsf((float)gy);
    const float thr = alpha * g + beta;
    if (!soft) return a < thr ? 255u : 0u;                                                            // P5: no division
    float q = 1.0f - a / thr;                                                                         // P4
    q = q > 0.0f ? q : 0.0f;   // a select: a NaN gives 0
    return (unsigned)(int)(q * 255.0f + 0.5f);
}

__global__ __launch_bounds__(256) void k_residual(const unsigned char *__restrict__ gray, const float *__restrict__ flow, ExportTab fr0,
                                                  ExportTab fr1, ExportTab fl, int w, int h, float alpha, float beta, int soft,
                                                  WeightArgs gate, char *__restrict__ out, long long out_item, long long out_pitch) {
    const int qw = (w + 3) >> 2;   // quads per row
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= (unsigned)qw * (unsigned)h) return;
    const int y = (int)(q / (unsigned)qw), x = (int)(q % (unsigned)qw) * 4;
    const int b = blockIdx.y, np = w - x < 4 ? w - x : 4;   // pixels of this quad
    const size_t N = (size_t)w * h;
    const float2 *F = (const float2 *)(flow + (size_t)fl.slot[b] * 2 * N) + ((unsigned)y * (unsigned)w + (unsigned)x);
    const unsigned char *I0 = gray + (size_t)fr0.slot[b] * N, *I1 = gray + (size_t)fr1.slot[b] * N;
    float2 f[4];
    if (np == 4 && ((uintptr_t)F & 15) == 0) {
        const float4 a = ((const float4 *)F)[0], c = ((const float4 *)F)[1];
        f[0] = make_float2(a.x, a.y), f[1] = make_float2(a.z, a.w), f[2] = make_float2(c.x, c.y), f[3] = make_float2(c.z, c.w);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) f[k] = k < np ? F[k] : make_float2(0.0f, 0.0f);
    }
    // I0: rows max(y-1, 0), y, min(y+1, h-1) at columns x .. x+np-1, and row y's columns max(x-1, 0) and min(x+np, w-1)
    const unsigned row = (unsigned)y * (unsigned)w + (unsigned)x;
    const unsigned up = (unsigned)(y > 0 ? y - 1 : 0) * (unsigned)w + (unsigned)x;
    const unsigned dn = (unsigned)(y + 1 < h ? y + 1 : h - 1) * (unsigned)w + (unsigned)x;
    const unsigned c4 = ffl_load_quad_u8(I0 + row, np), u4 = ffl_load_quad_u8(I0 + up, np), d4 = ffl_load_quad_u8(I0 + dn, np);
    const int left = x > 0 ? (int)I0[row - 1] : (int)(c4 & 255u);
    const int right = x + np < w ? (int)I0[row + (unsigned)np] : (int)((c4 >> (8 * (np - 1))) & 255u);
    int ce[6];   // row y at columns x-1 .. x+4, clamped
    ce[0] = left;
#pragma unroll
    for (int k = 0; k < 4; k++) ce[k + 1] = (int)((c4 >> (8 * k)) & 255u);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (k == np) ce[k + 1] = right;
    ce[5] = right;
    unsigned wt[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int gx = ce[k + 2] - ce[k], gy = (int)((d4 >> (8 * k)) & 255u) - (int)((u4 >> (8 * k)) & 255u);
        wt[k] = k < np ? ffl_residual_pixel(I1, f[k], ce[k + 1], gx, gy, x + k, y, w, h, alpha, beta, soft) : 0u;
    }
    if (gate.base) {   // P6
        const unsigned char *g = (const unsigned char *)gate.base + (long long)b * gate.item + (long long)y * gate.pitch + x;
        if (np == 4 && ((uintptr_t)g & 3) == 0) {
            const unsigned s = *(const unsigned *)g;
#pragma unroll
            for (int k = 0; k < 4; k++) wt[k] = min(wt[k], (s >> (8 * k)) & 255u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < np) wt[k] = min(wt[k], (unsigned)g[k]);
        }
    }
    unsigned char *o = (unsigned char *)out + (long long)b * out_item + (long long)y * out_pitch + x;
    if (np == 4 && ((uintptr_t)o & 3) == 0) {
        *(unsigned *)o = wt[0] | (wt[1] << 8) | (wt[2] << 16) | (wt[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < np) o[k] = (unsigned char)wt[k];
    }
}

void ffl_launch_residual(const unsigned char *gray, const float *flow, const ExportTab &fr0, const ExportTab &fr1, const ExportTab &fl,
                         int n, int w, int h, float alpha, float beta, int soft, const WeightArgs *gate, char *out,
                         long long out_item, long long out_pitch, hipStream_t st) {
    const size_t quads = (size_t)((w + 3) / 4) * h;   // below 2^30: 20 * w * h < 2^32
    const WeightArgs g = gate ? *gate : WeightArgs{nullptr, 0, 0};
    hipLaunchKernelGGL(k_residual, dim3((unsigned)((quads + 255) / 256), n), dim3(256), 0, st, gray, flow, fr0, fr1, fl, w, h, alpha, beta,
                       soft, g, out, out_item, out_pitch);
}

// ---- flow import -----------------------------------------------------------------------------
// k_import_pass1 reads n caller fields once: every pixel is widened to float32, stored into its flow slot by the lane that
// owns it in pass 1's walk (halo loads never store), and fed to the pass-1 body in k_pass1's order, so the partials -- and
// after k_pass1_final the records -- are bit-identical to ffl_upload_flow's for the float32 widening of the field.
template <int DT>
__device__ __forceinline__ float ffl_widen_bits(unsigned short bits) {  // exact: every f16 / bf16 value is a float32
    if (DT == FFL_IMP_BF16) return __uint_as_float((unsigned)bits << 16);
    return (float)__builtin_bit_cast(_Float16, bits);
}

template <int DT, int MODE>
struct P1ImportSrc {
    const char *item;          // the field's (0, 0, u)
    long long pitch, ps, cs;   // bytes
    float *slot;               // its flow slot
    int w;
    // the element at byte offset `off` of row `row`, widened
    __device__ __forceinline__ float elem(const char *row, long long off) const {
        if (DT == FFL_IMP_F32) return *(const FFL_GLOBAL float *)(row + off);
        return ffl_widen_bits<DT>(*(const FFL_GLOBAL unsigned short *)(row + off));
    }
    __device__ __forceinline__ float4 load(int yc, int xa) const {
        const char *row = item + (long long)yc * pitch;   // wave-uniform
        if (MODE == FFL_IMP_NHWC && DT == FFL_IMP_F32) {  // (u, v, u, v): one 16-byte load
            const ffl_v4f v = *(const FFL_GLOBAL ffl_v4f *)(row + (long long)xa * 8);
            return make_float4(v.x, v.y, v.z, v.w);
        } else if (MODE == FFL_IMP_NHWC) {                // 16-bit (u, v, u, v): one 8-byte load (4-byte aligned)
            const ffl_v2f v = *(const FFL_GLOBAL ffl_v2f *)(row + (long long)xa * 4);
            const unsigned a = __float_as_uint(v.x), b = __float_as_uint(v.y);
            return make_float4(ffl_widen_bits<DT>(a & 0xFFFFu), ffl_widen_bits<DT>(a >> 16), ffl_widen_bits<DT>(b & 0xFFFFu),
                               ffl_widen_bits<DT>(b >> 16));
        } else if (MODE == FFL_IMP_NCHW && DT == FFL_IMP_F32) {  // (u, u) and (v, v): one 8-byte load per plane
            const ffl_v2f u = *(const FFL_GLOBAL ffl_v2f *)(row + (long long)xa * 4);
            const ffl_v2f v = *(const FFL_GLOBAL ffl_v2f *)(row + cs + (long long)xa * 4);
            return make_float4(u.x, v.x, u.y, v.y);
        } else {                                          // any strides: element by element
            const long long o = (long long)xa * ps;
            return make_float4(elem(row, o), elem(row, o + cs), elem(row, o + ps), elem(row, o + ps + cs));
        }
    }
    __device__ __forceinline__ void store(int y, int x, float2 c0, float2 c1, bool s0, bool s1) const {
        // signed: x = -1 (the halo pixel of strip 0) forms an address one pixel before the slot that only s1 offsets past
        char *p = (char *)slot + 8 * ((long long)y * w + x);
        if (s0 && s1) {
            ffl_v4f v = {c0.x, c0.y, c1.x, c1.y};
            *(FFL_GLOBAL ffl_v4f *)p = v;
        } else if (s0) {
            ffl_v2f v = {c0.x, c0.y};
            *(FFL_GLOBAL ffl_v2f *)p = v;
        } else if (s1) {
            ffl_v2f v = {c1.x, c1.y};
            *(FFL_GLOBAL ffl_v2f *)(p + 8) = v;
        }
    }
};

// workgroup (0, b) also names item b's slot and record in `pt` for k_pass1_final (read after this launch, same stream)
__device__ __forceinline__ void ffl_import_publish(const ImportArgs &a, const ExportTab &tab, size_t N, PairTab *pt, int b) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        pt->flow[0][b] = a.flow + (size_t)tab.slot[b] * 2 * N;
        pt->res[b] = a.res + tab.slot[b];
    }
}

template <int DT, int MODE>
__global__ __launch_bounds__(P1_THREADS) void k_import_pass1(const ImportArgs a, const ExportTab tab, int w, int h,
                                                             int pov_mode, PairTab *__restrict__ pt,
                                                             unsigned long long *__restrict__ pkey,
                                                             double *__restrict__ psum) {
    __shared__ unsigned long long skey[P1_THREADS / 64];
    __shared__ double ssum[P1_THREADS / 64];
    const int b = blockIdx.y;
    const size_t N = (size_t)w * h;
    ffl_import_publish(a, tab, N, pt, b);
    const P1ImportSrc<DT, MODE> src{a.base + (long long)b * a.item, a.pitch, a.ps, a.cs, a.flow + (size_t)tab.slot[b] * 2 * N, w};
    ffl_pass1_body(src, WtNone{}, w, h, pov_mode, b, pkey, psum, skey, ssum);
}

template <int DT, int MODE>
static void ffl_import_launch(const ImportArgs &a, const ExportTab &tab, int n, int w, int h, int pov_mode, PairTab *pt,
                              unsigned long long *pkey, double *psum, hipStream_t st) {
    const int nblk = ffl_pass1_blocks(w, h);
    hipLaunchKernelGGL((k_import_pass1<DT, MODE>), dim3(nblk, n), dim3(P1_THREADS), 0, st, a, tab, w, h, pov_mode, pt, pkey,
                       psum);
    hipLaunchKernelGGL(k_pass1_final, dim3(n), dim3(P1_THREADS), 0, st, pt, w, h, pov_mode, nblk, pkey, psum);
}

void ffl_launch_import_pass1(const ImportArgs &a, const ExportTab &tab, int n, int dtype, int mode, int w, int h, int pov_mode,
                             PairTab *pt, unsigned long long *pkey, double *psum, hipStream_t st) {
#define FFL_IMP_CASE(DT, MODE)                                                                                   \
    if (dtype == DT && mode == MODE) return ffl_import_launch<DT, MODE>(a, tab, n, w, h, pov_mode, pt, pkey, psum, st);
    FFL_IMP_CASE(FFL_IMP_F32, FFL_IMP_NHWC)
    FFL_IMP_CASE(FFL_IMP_F32, FFL_IMP_NCHW)
    FFL_IMP_CASE(FFL_IMP_F32, FFL_IMP_ANY)
    FFL_IMP_CASE(FFL_IMP_F16, FFL_IMP_NHWC)
    FFL_IMP_CASE(FFL_IMP_F16, FFL_IMP_ANY)
    FFL_IMP_CASE(FFL_IMP_BF16, FFL_IMP_NHWC)
    FFL_IMP_CASE(FFL_IMP_BF16, FFL_IMP_ANY)
#undef FFL_IMP_CASE
}

// ---- pass 1 under weight maps (ffl_pass1_weighted) ----------------------------------------------
// k_pass1's walk over flow slots tab.slot[0..n) with item b's map at wa.base + b * wa.item; workgroup (0, b) names the slot
// and its record in `pt` for the final kernel, as the import does.
__global__ __launch_bounds__(P1_THREADS) void k_pass1_weighted(const ImportArgs a, const ExportTab tab, int w, int h, int pov_mode,
                                                               PairTab *__restrict__ pt, unsigned long long *__restrict__ pkey,
                                                               double *__restrict__ psum, double *__restrict__ psw) {
    __shared__ unsigned long long skey[P1_THREADS / 64];
    __shared__ double ssum[P1_THREADS / 64], ssw[P1_THREADS / 64];
    const int b = blockIdx.y;
    const size_t N = (size_t)w * h;
    ffl_import_publish(a, tab, N, pt, b);
    const P1SlotSrc src{reinterpret_cast<const float2 *>(a.flow + (size_t)tab.slot[b] * 2 * N), w};
    const WtBytes wt{a.base + (long long)b * a.item, a.pitch};
    ffl_pass1_body(src, wt, w, h, pov_mode, b, pkey, psum, skey, ssum, psw, ssw);
}

__global__ __launch_bounds__(P1_THREADS) void k_pass1_weighted_final(const PairTab *__restrict__ pt, int w, int h, int pov_mode,
                                                                     int nblk, const unsigned long long *__restrict__ pkey,
                                                                     const double *__restrict__ psum,
                                                                     const double *__restrict__ psw) {
    __shared__ unsigned long long skey[P1_THREADS / 64];
    __shared__ double ssum[P1_THREADS / 64], ssw[P1_THREADS / 64];
    ffl_pass1_final_body<true>(pt, w, h, pov_mode, nblk, pkey, psum, psw, skey, ssum, ssw);
}

void ffl_launch_pass1_weighted(const WeightArgs &wa, float *flow, Pass1Result *res, const ExportTab &tab, int n, int w, int h,
                               int pov_mode, PairTab *pt, unsigned long long *pkey, double *psum, double *psw, hipStream_t st) {
    const int nblk = ffl_pass1_blocks(w, h);
    const ImportArgs a{wa.base, wa.item, wa.pitch, 1, 0, flow, res};
    hipLaunchKernelGGL(k_pass1_weighted, dim3(nblk, n), dim3(P1_THREADS), 0, st, a, tab, w, h, pov_mode, pt, pkey, psum, psw);
    hipLaunchKernelGGL(k_pass1_weighted_final, dim3(n), dim3(P1_THREADS), 0, st, pt, w, h, pov_mode, nblk, pkey, psum, psw);
}

// ---- global-motion fit and compensation (ffl_motion_fit, ffl_motion_subtract) --------
// The fit's main kernel is k_strip_sums<MotionSums<WA, PRIOR>>: pass 2's walk with the twelve float64 sums of rule C4 per lane
// instead of four, in four instantiations, {NoWeights, WeightArgs} x {no prior, prior}.  MOT_G: rows of the row group whose loads
// are in flight together; 2 as for the four-component RadialSums (the compiler's report for gfx950, no scratch: DESIGN.md
// section 19).
#ifndef MOT_G
#define MOT_G 2
#endif

// One pixel's twelve terms (rules C3, C4) into the lane's sums.  mux, mvx: (a0 + a1 * xc) and (b0 + b1 * xc) of the prior, formed
// once per column.  The exclusion is three selects, not twelve: `in` false replaces the pixel's omega, u and v by +0.0 BEFORE
// any term is formed, so nothing of its flow or of its weight reaches a term, each of its twelve terms is +0.0 or -0.0 (a zero
// times a coordinate), and adding either to a sum that started at +0.0 leaves the sum's bits as they were -- the sums are
// those of adding +0.0.  (Selecting each term instead cost 24 v_cndmask per pixel in a kernel that is VALU-bound: DESIGN.md
// section 19.)
template <bool PRIOR>
__device__ __forceinline__ void ffl_motion_terms(double (&sum)[FFL_MOTION_NSUMS], bool in, float2 f, double wt, double xc, double yc,
                                                 double mux, double mvx, double a2, double b2, double t2) {
    double om = wt;
    if constexpr (PRIOR) {
        const double ru = (double)f.x - (mux + a2 * yc), rv = (double)f.y - (mvx + b2 * yc);
        const double r2 = ru * ru + rv * rv;
        const double rho = t2 / (t2 + r2);   // the one division of rule C3
        om = wt * rho;
    }
    om = in ? om : 0.0;
    const double u = (double)(in ? f.x : 0.0f), v = (double)(in ? f.y : 0.0f);
    const double ox = om * xc, oy = om * yc, ou = om * u, ov = om * v;
    sum[MOT_S] += om;
    sum[MOT_SX] += ox;
    sum[MOT_SY] += oy;
    sum[MOT_SXX] += ox * xc;
    sum[MOT_SXY] += ox * yc;
    sum[MOT_SYY] += oy * yc;
    sum[MOT_SU] += ou;
    sum[MOT_SUX] += ou * xc;
    sum[MOT_SUY] += ou * yc;
    sum[MOT_SV] += ov;
    sum[MOT_SVX] += ov * xc;
    sum[MOT_SVY] += ov * yc;
}

// ffl_wave_sum_f64's tree -- offsets 32, 16, 8, 4, 2, 1, hence its bits -- with the four steps inside a row of 16 lanes as DPP
// row shifts (lane i reads lane i + N of its row; a lane past the row's end reads 0 and feeds nothing lane 0 consumes) instead
// of ds_bpermute: twelve sums cost 144 ds_bpermute_b32 per wave the plain way, a third of a wave's life in the fit's k_strip_sums.
template <int N>
__device__ __forceinline__ double ffl_row_down(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b & 0xFFFFFFFFull), 0x100 | N, 0xF, 0xF, false);   // row_shl:N
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), 0x100 | N, 0xF, 0xF, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo));
}
__device__ __forceinline__ double ffl_wave_sum_f64_rows(double v) {
    v += __shfl_down(v, 32, 64);
    v += __shfl_down(v, 16, 64);
    v += ffl_row_down<8>(v);
    v += ffl_row_down<4>(v);
    v += ffl_row_down<2>(v);
    v += ffl_row_down<1>(v);
    return v;
}

__device__ __forceinline__ bool ffl_flow_finite(float2 f) { return fabsf(f.x) <= FLT_MAX && fabsf(f.y) <= FLT_MAX; }

template <class WA, bool PRIOR>
struct MotionSums {
    using Wt = decltype(ffl_item_weights(WA{}, 0));
    static constexpr int G = MOT_G, NS = FFL_MOTION_NSUMS;
    const float *flow;
    ExportTab tab;
    WA wa;
    MotionPrior prior;
    double t2;
    struct Item { double a0, a1, a2, b0, b1, b2, hx, hy; };
    struct Columns { double xc0, xc1, mux0, mvx0, mux1, mvx1; };   // centred x and the prior's (a0 + a1 * xc), (b0 + b1 * xc)
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ const float2 *field(int b, int w, int h) const {
        return reinterpret_cast<const float2 *>(flow + (size_t)tab.slot[b] * 2 * ((size_t)w * h));
    }
    __device__ __forceinline__ Wt weights(int b) const { return ffl_item_weights(wa, b); }
    __device__ __forceinline__ Item item(int b, int w, int h) const {
        const double hx = (double)(w - 1) / 2.0, hy = (double)(h - 1) / 2.0;   // rule C1
        const double *p = reinterpret_cast<const double *>(prior.base + (long long)b * prior.stride);   // wave-uniform
        if constexpr (PRIOR) return Item{p[0], p[1], p[2], p[3], p[4], p[5], hx, hy};
        return Item{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, hx, hy};
    }
    __device__ __forceinline__ Columns columns(const Item &it, int x, int) const {
        const double xc0 = (double)x - it.hx, xc1 = (double)(x + 1) - it.hx;
        return Columns{xc0, xc1, it.a0 + it.a1 * xc0, it.b0 + it.b1 * xc0, it.a0 + it.a1 * xc1, it.b0 + it.b1 * xc1};
    }
    __device__ __forceinline__ void row(double (&sum)[NS], const Item &it, const Columns &c, int y, int h, bool ok0, bool ok1,
                                        float2 f0, float2 f1, unsigned q0, unsigned q1) const {
        const double yc = (double)y - it.hy;
        // without maps q0 = q1 = 1 (WtNone): the weight's test and its factor fold away
        const bool in0 = ok0 && y < h && ffl_flow_finite(f0) && q0 > 0u, in1 = ok1 && y < h && ffl_flow_finite(f1) && q1 > 0u;
        ffl_motion_terms<PRIOR>(sum, in0, f0, (double)q0, c.xc0, yc, c.mux0, c.mvx0, it.a2, it.b2, t2);
        ffl_motion_terms<PRIOR>(sum, in1, f1, (double)q1, c.xc1, yc, c.mux1, c.mvx1, it.a2, it.b2, t2);
    }
    static __device__ __forceinline__ double wave_sum(double v) { return ffl_wave_sum_f64_rows(v); }
};

// One workgroup per item: its nblk partials of every sum in k_radial_final's tree, then thread 0 runs the solve of rules C5 and
// C6 (ffl_motion_solve_body, the source ffl_motion_solve compiles for the host) and writes the record, and the sums when asked.
__global__ __launch_bounds__(P1_THREADS) void k_motion_solve(int nblk, int model, const double *__restrict__ psum,
                                                             MotionRecord *__restrict__ models, double *__restrict__ sums) {
    constexpr int NS = FFL_MOTION_NSUMS;
    __shared__ double ssum[NS * (P1_THREADS / 64)];
    const int b = blockIdx.x;
    double sum[NS] = {};
    ffl_collect_partials<NS>(sum, ssum, psum, b, nblk);
    if (threadIdx.x == 0) {
        MotionRecord r;
        ffl_motion_solve_body(sum, model, &r);
        models[b] = r;
        if (sums) {
#pragma unroll
            for (int c = 0; c < NS; c++) sums[(size_t)b * NS + c] = sum[c];
        }
    }
}

void ffl_launch_motion_fit(const float *flow, const ExportTab &tab, int n, int w, int h, const WeightArgs *maps,
                           const MotionPrior &prior, float tau, int model, double *psum, MotionRecord *models, double *sums,
                           hipStream_t st) {
    const double t2 = (double)tau * (double)tau;
    if (maps && prior.base)
        ffl_launch_strip_sums(MotionSums<WeightArgs, true>{flow, tab, *maps, prior, t2}, n, w, h, psum, st);
    else if (maps)
        ffl_launch_strip_sums(MotionSums<WeightArgs, false>{flow, tab, *maps, prior, t2}, n, w, h, psum, st);
    else if (prior.base)
        ffl_launch_strip_sums(MotionSums<NoWeights, true>{flow, tab, NoWeights{}, prior, t2}, n, w, h, psum, st);
    else
        ffl_launch_strip_sums(MotionSums<NoWeights, false>{flow, tab, NoWeights{}, prior, t2}, n, w, h, psum, st);
    hipLaunchKernelGGL(k_motion_solve, dim3(n), dim3(P1_THREADS), 0, st, ffl_radial_blocks(w, h), model, psum, models, sums);
}

// Rule C8, element-wise: grid = (blocks per item, items) in k_export_flows' style, a lane handles FFL_EXP_UNROLL units of one
// item 256 units apart.  A unit is two consecutive pixels of the row-major field (one 16-byte load and store) where the field
// has an even number of pixels -- every slot is then 16-byte aligned -- else one pixel.  Each pixel is read and written by the
// same lane only, so dst may be src (in place).  Workgroup (0, b) names the dst slot and its record in `pt` for the k_pass1 /
// k_pass1_final pair that follows on the stream, as the import does.
__device__ __forceinline__ float2 ffl_motion_sub(float2 f, int x, int y, double hx, double hy, const double (&m)[6]) {
    const double xc = (double)x - hx, yc = (double)y - hy;
    const double mu = (m[0] + m[1] * xc) + m[2] * yc, mv = (m[3] + m[4] * xc) + m[5] * yc;
    return make_float2((float)((double)f.x - mu), (float)((double)f.y - mv));
}

__global__ __launch_bounds__(256) void k_motion_subtract(float *__restrict__ flow, Pass1Result *__restrict__ res, const ExportTab src,
                                                         const ExportTab dst, int w, int h, const char *__restrict__ models,
                                                         long long stride, int vec, PairTab *__restrict__ pt) {
    const int b = blockIdx.y;
    const size_t N = (size_t)w * h;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        pt->flow[0][b] = flow + (size_t)dst.slot[b] * 2 * N;
        pt->res[b] = res + dst.slot[b];
    }
    const float *s = flow + (size_t)src.slot[b] * 2 * N;   // may alias d: no __restrict__
    float *d = flow + (size_t)dst.slot[b] * 2 * N;
    const double *mp = reinterpret_cast<const double *>(models + (long long)b * stride);   // wave-uniform
    const double m[6] = {mp[0], mp[1], mp[2], mp[3], mp[4], mp[5]};
    const double hx = (double)(w - 1) / 2.0, hy = (double)(h - 1) / 2.0;   // rule C1
    const unsigned base = blockIdx.x * (256u * FFL_EXP_UNROLL) + threadIdx.x;   // units < 2^31: 20 * w * h < 2^32
    const unsigned units = (unsigned)(vec ? N / 2 : N);
#pragma unroll
    for (int k = 0; k < FFL_EXP_UNROLL; k++) {
        const unsigned u = base + (unsigned)k * 256u;
        if (u >= units) continue;
        if (vec) {
            const unsigned p = 2u * u;
            const int y = (int)(p / (unsigned)w), x = (int)(p - (unsigned)y * (unsigned)w);
            const int x1 = x + 1 == w ? 0 : x + 1, y1 = x + 1 == w ? y + 1 : y;   // an odd width: the pair may end a row
            const float4 t = ((const float4 *)s)[u];
            const float2 a = ffl_motion_sub(make_float2(t.x, t.y), x, y, hx, hy, m);
            const float2 c = ffl_motion_sub(make_float2(t.z, t.w), x1, y1, hx, hy, m);
            ((float4 *)d)[u] = make_float4(a.x, a.y, c.x, c.y);
        } else {
            const int y = (int)(u / (unsigned)w), x = (int)(u - (unsigned)y * (unsigned)w);
            ((float2 *)d)[u] = ffl_motion_sub(((const float2 *)s)[u], x, y, hx, hy, m);
        }
    }
}

void ffl_launch_motion_subtract(float *flow, Pass1Result *res, const ExportTab &src, const ExportTab &dst, int n, int w, int h,
                                const char *models, long long stride, PairTab *pt, hipStream_t st) {
    const size_t N = (size_t)w * h;
    const int vec = N % 2 == 0;   // slot bases are 8N bytes apart
    const size_t units = vec ? N / 2 : N;
    dim3 grid((unsigned)((units + 256 * FFL_EXP_UNROLL - 1) / (256 * FFL_EXP_UNROLL)), n);
    hipLaunchKernelGGL(k_motion_subtract, grid, dim3(256), 0, st, flow, res, src, dst, w, h, models, stride, vec, pt);
}

// ---- texture (structure-tensor) maps ---------------------------------------------
// (This section stands at the end of the file on purpose: the kernels above keep the order, and with it the offsets inside the
// code object, that they had before it was added.  With it behind k_residual the plain 1080p chunk, which launches none of it,
// ran 3 % low against the parent build; here it does not: profiles/texture_unchanged_paths.md.)
// k_texture writes one uint8 weight per pixel from the gray operand I of one frame slot: Noble's cornerness det / tr of the
// structure tensor summed over a (2R+1)^2 window, against tau.  Unlike its two siblings it has a stencil, so it goes through
// LDS.  grid = (tiles per item, items); a workgroup of 256 lanes owns a tile of 64 x 16 output pixels and runs four steps
// with a barrier between them:
//   1  the tile's gray bytes plus a halo of R + 1, (66 + 2R) x (18 + 2R), read once from global memory at clamped coordinates;
//   2  (gx, gy) of rule T1 at every position of the (64 + 2R) x (16 + 2R) window region, taken AT THE CLAMPED POSITION (rule T2
//      -- not the gradient of the clamped image, which would be 0 outside the frame), packed as two int16 in one dword;
//   3  per row of that region and quad of columns the three horizontal window sums: 4 + 2R packed gradients come in as
//      ceil((4 + 2R) / 4) 16-byte LDS reads (conflict-free: consecutive lanes read consecutive 16 bytes), the first window is
//      summed, the other three slide; three int4 go out;
//   4  lane (quad, row) adds the 2R + 1 rows above and below as int4, applies T3 to T6 and stores 4 bytes where the address
//      allows and bytes otherwise, as k_residual does.
// The sums are integers, so their order is free (rule T2) and the bits do not depend on R being a template parameter.  det is
// a 64-bit product (rule T3: at R = 8 Sxx * Syy reaches 3.5e14).  gate may alias out exactly (ffl_texture_weights' in-place
// form): a lane reads the gate bytes of its own quad before it writes them, so out carries no __restrict__.
#define FFL_TEX_TW 64
#define FFL_TEX_TH 16

template <int R>
__global__ __launch_bounds__(256) void k_texture(const unsigned char *__restrict__ gray, ExportTab fr, int w, int h, int tiles_x,
                                                 double tn, int soft, WeightArgs gate, char *out, long long out_item,
                                                 long long out_pitch) {
    constexpr int TW = FFL_TEX_TW, TH = FFL_TEX_TH;
    constexpr int GW = TW + 2 * R + 2, GH = TH + 2 * R + 2, GP = (GW + 3) & ~3;   // gray tile and its pitch in bytes
    constexpr int PW = TW + 2 * R, PH = TH + 2 * R;                               // window region
    constexpr int NV = (4 + 2 * R + 3) / 4;                                       // 16-byte reads per quad in step 3
    constexpr int PP = TW - 4 + 4 * NV;                                           // pitch of the region in dwords, >= PW
    __shared__ unsigned char s_gray[GH * GP];
    __shared__ __attribute__((aligned(16))) unsigned s_grad[PH * PP];
    __shared__ __attribute__((aligned(16))) int s_h[3][PH][TW];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int ox = (int)(blockIdx.x % (unsigned)tiles_x) * TW, oy = (int)(blockIdx.x / (unsigned)tiles_x) * TH;
    const unsigned char *I = gray + (size_t)fr.slot[b] * ((size_t)w * h);
    // 1: gray, clamped: no access leaves the frame
    for (int i = tid; i < GW * GH; i += 256) {
        const int ty = i / GW, tx = i - ty * GW;
        int sx = ox - (R + 1) + tx, sy = oy - (R + 1) + ty;
        sx = sx < 0 ? 0 : sx > w - 1 ? w - 1 : sx;
        sy = sy < 0 ? 0 : sy > h - 1 ? h - 1 : sy;
        s_gray[ty * GP + tx] = I[(unsigned)sy * (unsigned)w + (unsigned)sx];
    }
    __syncthreads();
    // 2: gradients at the clamped position.  The region contains a pixel of the frame (the tile's origin), so the clamped
    // position stays inside the region and its four neighbours inside the gray tile.
    for (int i = tid; i < PW * PH; i += 256) {
        const int py = i / PW, px = i - py * PW;
        int X = ox - R + px, Y = oy - R + py;
        X = X < 0 ? 0 : X > w - 1 ? w - 1 : X;
        Y = Y < 0 ? 0 : Y > h - 1 ? h - 1 : Y;
        const int tx = X - (ox - (R + 1)), ty = Y - (oy - (R + 1));   // 1 <= tx <= GW - 2, 1 <= ty <= GH - 2
        const int gx = (int)s_gray[ty * GP + tx + 1] - (int)s_gray[ty * GP + tx - 1];
        const int gy = (int)s_gray[(ty + 1) * GP + tx] - (int)s_gray[(ty - 1) * GP + tx];
        s_grad[py * PP + px] = ((unsigned)gx & 0xffffu) | ((unsigned)gy << 16);
    }
    __syncthreads();
    // 3: horizontal window sums of gx^2, gx*gy, gy^2 for the quad's four columns
    for (int t = tid; t < PH * (TW / 4); t += 256) {
        const int q = t & (TW / 4 - 1), j = t / (TW / 4);
        unsigned g[4 * NV];
#pragma unroll
        for (int m = 0; m < NV; m++) {
            const uint4 v = *(const uint4 *)&s_grad[j * PP + 4 * q + 4 * m];   // words past 4q + 3 + 2R are read and never used
            g[4 * m] = v.x, g[4 * m + 1] = v.y, g[4 * m + 2] = v.z, g[4 * m + 3] = v.w;
        }
        int sxx[4], sxy[4], syy[4];   // only the packed words stay in registers: the products are formed where they are added
        sxx[0] = sxy[0] = syy[0] = 0;
#pragma unroll
        for (int k = 0; k <= 2 * R; k++) {
            const int gx = (int)(short)(g[k] & 0xffffu), gy = (int)g[k] >> 16;
            sxx[0] += gx * gx, sxy[0] += gx * gy, syy[0] += gy * gy;
        }
#pragma unroll
        for (int k = 1; k < 4; k++) {
            const int ax = (int)(short)(g[k - 1] & 0xffffu), ay = (int)g[k - 1] >> 16;               // leaves the window
            const int bx = (int)(short)(g[k + 2 * R] & 0xffffu), by = (int)g[k + 2 * R] >> 16;       // enters it
            sxx[k] = sxx[k - 1] - ax * ax + bx * bx;
            sxy[k] = sxy[k - 1] - ax * ay + bx * by;
            syy[k] = syy[k - 1] - ay * ay + by * by;
        }
        *(int4 *)&s_h[0][j][4 * q] = make_int4(sxx[0], sxx[1], sxx[2], sxx[3]);
        *(int4 *)&s_h[1][j][4 * q] = make_int4(sxy[0], sxy[1], sxy[2], sxy[3]);
        *(int4 *)&s_h[2][j][4 * q] = make_int4(syy[0], syy[1], syy[2], syy[3]);
    }
    __syncthreads();
    // 4: vertical sums, T3 to T6, the store
    const int q = tid & (TW / 4 - 1), ly = tid / (TW / 4);
    const int x = ox + 4 * q, y = oy + ly;
    if (x >= w || y >= h) return;
    int4 a = make_int4(0, 0, 0, 0), c = a, d = a;
#pragma unroll 3   // a full unroll keeps all 3 * (2R + 1) int4 in flight: 196 VGPRs at R = 7 against 2 waves per SIMD
    for (int j = 0; j <= 2 * R; j++) {
        const int4 u = *(const int4 *)&s_h[0][ly + j][4 * q], v = *(const int4 *)&s_h[1][ly + j][4 * q],
                   z = *(const int4 *)&s_h[2][ly + j][4 * q];
        a.x += u.x, a.y += u.y, a.z += u.z, a.w += u.w;
        c.x += v.x, c.y += v.y, c.z += v.z, c.w += v.w;
        d.x += z.x, d.y += z.y, d.z += z.z, d.w += z.w;
    }
    const int Sxx[4] = {a.x, a.y, a.z, a.w}, Sxy[4] = {c.x, c.y, c.z, c.w}, Syy[4] = {d.x, d.y, d.z, d.w};
    const int np = w - x < 4 ? w - x : 4;   // pixels of this quad
    unsigned wt[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int tr = Sxx[k] + Syy[k];                                                               // T3
        const long long det = (long long)Sxx[k] * (long long)Syy[k] - (long long)Sxy[k] * (long long)Sxy[k];
        if (!soft) {
            wt[k] = (double)det >= tn * (double)tr && tr != 0 ? 255u : 0u;                            // T5: no division
        } else if (tr == 0) {
            wt[k] = 0u;
        } else {
            double qv = ((double)det / (double)tr) / tn;                                              // T4
            qv = qv < 1.0 ? qv : 1.0;
            wt[k] = (unsigned)(int)(qv * 255.0 + 0.5);
        }
    }
    if (gate.base) {   // T6
        const unsigned char *g = (const unsigned char *)gate.base + (long long)b * gate.item + (long long)y * gate.pitch + x;
        if (np == 4 && ((uintptr_t)g & 3) == 0) {
            const unsigned s = *(const unsigned *)g;
#pragma unroll
            for (int k = 0; k < 4; k++) wt[k] = min(wt[k], (s >> (8 * k)) & 255u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < np) wt[k] = min(wt[k], (unsigned)g[k]);
        }
    }
    unsigned char *o = (unsigned char *)out + (long long)b * out_item + (long long)y * out_pitch + x;
    if (np == 4 && ((uintptr_t)o & 3) == 0) {
        *(unsigned *)o = wt[0] | (wt[1] << 8) | (wt[2] << 16) | (wt[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < np) o[k] = (unsigned char)wt[k];
    }
}

template <int R>
static void ffl_launch_texture_r(const unsigned char *gray, const ExportTab &fr, int n, int w, int h, double tn, int soft,
                                 const WeightArgs &g, char *out, long long out_item, long long out_pitch, hipStream_t st) {
    const int tx = (w + FFL_TEX_TW - 1) / FFL_TEX_TW, ty = (h + FFL_TEX_TH - 1) / FFL_TEX_TH;   // at most 512 * 2048 tiles
    hipLaunchKernelGGL(k_texture<R>, dim3((unsigned)tx * (unsigned)ty, n), dim3(256), 0, st, gray, fr, w, h, tx, tn, soft, g, out,
                       out_item, out_pitch);
}

void ffl_launch_texture(const unsigned char *gray, const ExportTab &fr, int n, int w, int h, int radius, float tau, int soft,
                        const WeightArgs *gate, char *out, long long out_item, long long out_pitch, hipStream_t st) {
    const WeightArgs g = gate ? *gate : WeightArgs{nullptr, 0, 0};
    const double tn = (double)tau * (double)((2 * radius + 1) * (2 * radius + 1));   // rule T4's tn, formed once
    switch (radius) {   // 1..8, host-checked
#define FFL_TEX_CASE(R) \
    case R: ffl_launch_texture_r<R>(gray, fr, n, w, h, tn, soft, g, out, out_item, out_pitch, st); break;
        FFL_TEX_CASE(1) FFL_TEX_CASE(2) FFL_TEX_CASE(3) FFL_TEX_CASE(4) FFL_TEX_CASE(5) FFL_TEX_CASE(6) FFL_TEX_CASE(7) FFL_TEX_CASE(8)
#undef FFL_TEX_CASE
    }
}
