// Region tracking through the flow and ROI weight maps (ffl_track_advance, ffl_roi_weights; DESIGN.md section 23, appendices
// Q and E).  A file of its own: the kernels of kernels_post.hip keep the code object, and the offsets inside it, that they had
// before these were added (see the note above k_texture there).
#include <cfloat>
#include <cstdint>
#include <hip/hip_runtime.h>

#include "ffl_kernels.h"

// ---- k_track (appendix Q) ---------------------------------------------------------------------------------------------
// One workgroup per track walks the n items in order: item i + 1's window depends on item i's step, so the chain is
// sequential by nature and the kernel is latency-bound by construction (n_tracks workgroups, n dependent steps).  Per item,
// with a barrier between the phases:
//   A  every lane reads the position and the item's cut flag from LDS and forms the clipped window of rule Q2;
//   B  all 256 lanes stage the window's (u, v), and its map bytes if there are any, into LDS: a wave per row (64 contiguous
//      pixels), four rows per pass, every load issued before the first store; a cut item has an empty window and stages
//      nothing (rule Q6: none of its flow or map is read);
//   C  one lane per window column adds its column from LDS top to bottom (rule Q4; the LDS rows are 65 float2 apart, so the
//      lanes of a wave read consecutive words);
//   D  lane 0 adds the <= 65 column sums left to right, forms the step (Q6), writes the record (Q7) and moves (Q8).
// The cut flags of all n items (rule Q5) are formed once, in parallel, before the walk: the pass-1 records are mapped host
// memory, and n dependent reads of it would cost more than the walk.
// Every index against Q1 and Q2: the position is in [0, w-1] x [0, h-1] after Q1's selects whatever the state held (a NaN
// fails c >= 0 and becomes 0), and it stays there because Q8 passes every new position through the same selects.  So
// ix = floor(x + 0.5) is in 0..w-1 (w <= 32768: x + 0.5 is exact), x0 = max(ix - r, 0) <= ix <= x1 = min(ix + r, w - 1), hence
// 1 <= ww = x1 - x0 + 1 <= 2r + 1 <= 65 with r <= 32 (host-checked, and clamped again below); rows alike.  A staged pixel
// (x0 + rx, y0 + ry) has rx < ww, ry < hh: inside the field, and its LDS index ry * 65 + rx <= 64 * 65 + 63 is inside the
// 65 x 65 arrays; the 65th column is staged only when ww == 65, at (x0 + 64 = x1, y0 + tid) with tid < hh, LDS index
// tid * 65 + 64 <= 64 * 65 + 64.  Column lanes are tid < ww <= 65, s_cut is indexed by i < n <= FFL_MAXB, record (i, t) by i < n, t < n_tracks.
#define TRK_THREADS 256
#define TRK_SIDE (2 * FFL_TRACK_MAX_R + 1)
#define TRK_PASSES ((TRK_SIDE + 3) / 4)   // staging passes of four rows

__device__ __forceinline__ double ffl_track_clamp(double c, double hi) {   // rule Q1: two selects, a NaN gives 0
    return c >= 0.0 ? (c <= hi ? c : hi) : 0.0;
}

__global__ __launch_bounds__(TRK_THREADS) void k_track(const float *__restrict__ flow, const Pass1Result *__restrict__ res,
                                                        const ExportTab tab, int n, int n_tracks, int w, int h, int radius,
                                                        int on_cut, float cut_threshold, double npx, WeightArgs maps,
                                                        TrackState *__restrict__ state, TrackRecord *__restrict__ out) {
    __shared__ float2 s_f[TRK_SIDE * TRK_SIDE];
    __shared__ unsigned char s_w[TRK_SIDE * TRK_SIDE + 7];
    __shared__ double s_col[3][TRK_SIDE];
    __shared__ int s_cnt[TRK_SIDE];
    __shared__ int s_cut[FFL_MAXB];
    __shared__ double s_pos[2];
    const int t = blockIdx.x, tid = threadIdx.x;
    const int r = radius < FFL_TRACK_MAX_R ? radius : FFL_TRACK_MAX_R;
    const double xmax = (double)(w - 1), ymax = (double)(h - 1);
    const size_t N = (size_t)w * h;
    for (int k = tid; k < n; k += TRK_THREADS) {   // rule Q5, ffl_pass1_results' expressions
        const float mm = (float)ffl_record_mean(res[tab.slot[k]], npx);
        s_cut[k] = mm > cut_threshold ? 1 : 0;     // NaN > threshold is false
    }
    TrackState st{};
    if (tid == 0) {
        st = state[t];
        st.x = ffl_track_clamp(st.x, xmax);        // Q1
        st.y = ffl_track_clamp(st.y, ymax);
        st.home_x = ffl_track_clamp(st.home_x, xmax);
        st.home_y = ffl_track_clamp(st.home_y, ymax);
        s_pos[0] = st.x;
        s_pos[1] = st.y;
    }
    for (int i = 0; i < n; i++) {
        __syncthreads();   // A: the position of item i (and, for i = 0, the cut flags)
        const int cut = s_cut[i];
        const int ix = (int)floor(s_pos[0] + 0.5), iy = (int)floor(s_pos[1] + 0.5);   // Q2
        const int x0 = max(ix - r, 0), x1 = min(ix + r, w - 1), y0 = max(iy - r, 0), y1 = min(iy + r, h - 1);
        const int ww = cut ? 0 : x1 - x0 + 1, hh = cut ? 0 : y1 - y0 + 1;
        // B: the window into LDS
        const float2 *F = reinterpret_cast<const float2 *>(flow + (size_t)tab.slot[i] * 2 * N);
        const unsigned char *M = reinterpret_cast<const unsigned char *>(maps.base) + (long long)i * maps.item;
        // A wave takes a row's first 64 columns, the four waves four rows per pass; the 65th column (only an unclipped window
        // of radius 32 has one) goes one row per lane.  All loads are issued before the first LDS store, so an item pays one
        // global round trip, not one per pass (256x256, n = 256, r = 32: 3.67 -> 2.44 ms per call).
        const int rx = tid & 63, r4 = tid >> 6;
        const bool last = ww == TRK_SIDE && tid < hh;
        float2 fv[TRK_PASSES + 1];
        unsigned char mv[TRK_PASSES + 1];
#pragma unroll
        for (int j = 0; j < TRK_PASSES; j++) {
            const int ry = 4 * j + r4;
            if (rx < ww && ry < hh) {
                fv[j] = F[(unsigned)(y0 + ry) * (unsigned)w + (unsigned)(x0 + rx)];   // 20 * w * h < 2^32
                if (maps.base) mv[j] = M[(long long)(y0 + ry) * maps.pitch + (x0 + rx)];
            }
        }
        if (last) {
            fv[TRK_PASSES] = F[(unsigned)(y0 + tid) * (unsigned)w + (unsigned)(x0 + TRK_SIDE - 1)];
            if (maps.base) mv[TRK_PASSES] = M[(long long)(y0 + tid) * maps.pitch + (x0 + TRK_SIDE - 1)];
        }
#pragma unroll
        for (int j = 0; j < TRK_PASSES; j++) {
            const int ry = 4 * j + r4;
            if (rx < ww && ry < hh) {
                s_f[ry * TRK_SIDE + rx] = fv[j];
                if (maps.base) s_w[ry * TRK_SIDE + rx] = mv[j];
            }
        }
        if (last) {
            s_f[tid * TRK_SIDE + TRK_SIDE - 1] = fv[TRK_PASSES];
            if (maps.base) s_w[tid * TRK_SIDE + TRK_SIDE - 1] = mv[TRK_PASSES];
        }
        __syncthreads();
        // C: one lane per column, top to bottom (Q3, Q4)
        if (tid < ww) {
            double cS = 0.0, cU = 0.0, cV = 0.0;
            int cnt = 0;
#pragma unroll 8   // the LDS reads of eight rows in flight ahead of the one chain of additions
            for (int ry = 0; ry < hh; ry++) {
                const float2 f = s_f[ry * TRK_SIDE + tid];
                const unsigned wb = maps.base ? (unsigned)s_w[ry * TRK_SIDE + tid] : 1u;
                const bool keep = wb != 0u && fabsf(f.x) <= FLT_MAX && fabsf(f.y) <= FLT_MAX;
                const double wt = (double)wb;
                const double nS = cS + wt, nU = cU + wt * (double)f.x, nV = cV + wt * (double)f.y;
                cS = keep ? nS : cS;   // selects: nothing of a dropped member reaches a sum
                cU = keep ? nU : cU;
                cV = keep ? nV : cV;
                cnt += keep ? 1 : 0;
            }
            s_col[0][tid] = cS;
            s_col[1][tid] = cU;
            s_col[2][tid] = cV;
            s_cnt[tid] = cnt;
        }
        __syncthreads();
        // D: the columns left to right, the step, the record, the move
        if (tid == 0) {
            double S = 0.0, U = 0.0, V = 0.0;
            int count = 0;
#pragma unroll 8
            for (int c = 0; c < ww; c++) {
                S += s_col[0][c];
                U += s_col[1][c];
                V += s_col[2][c];
                count += s_cnt[c];
            }
            TrackRecord rec;
            rec.x = st.x;   // Q7: the position before the step
            rec.y = st.y;
            rec.du = 0.0;
            rec.dv = 0.0;
            rec.sw = S;     // +0.0 for a cut item
            rec.count = count;
            int status = TRK_OK;
            if (cut) {      // Q6
                status |= TRK_CUT;
            } else if (S == 0.0) {
                status |= TRK_LOST;
                st.lost_run = (int)((unsigned)st.lost_run + 1u);
            } else {
                rec.du = U / S;
                rec.dv = V / S;
                st.lost_run = 0;
            }
            if (cut && on_cut == TRK_HOME) {   // Q8
                st.x = st.home_x;
                st.y = st.home_y;
            } else {
                const double nx = st.x + rec.du, ny = st.y + rec.dv;
                const double qx = ffl_track_clamp(nx, xmax), qy = ffl_track_clamp(ny, ymax);
                if (!(qx == nx) || !(qy == ny)) status |= TRK_CLAMPED;
                st.x = qx;
                st.y = qy;
            }
            st.steps = (long long)((unsigned long long)st.steps + 1ull);
            rec.status = status;
            out[(size_t)i * n_tracks + t] = rec;
            s_pos[0] = st.x;
            s_pos[1] = st.y;
        }
    }
    if (tid == 0) state[t] = st;
}

void ffl_launch_track(const float *flow, const Pass1Result *res, const ExportTab &tab, int n, int n_tracks, int w, int h,
                      int radius, int on_cut, float cut_threshold, const WeightArgs *maps, TrackState *state, TrackRecord *out,
                      hipStream_t st) {
    const WeightArgs m = maps ? *maps : WeightArgs{nullptr, 0, 0};
    hipLaunchKernelGGL(k_track, dim3(n_tracks), dim3(TRK_THREADS), 0, st, flow, res, tab, n, n_tracks, w, h, radius, on_cut,
                       cut_threshold, (double)w * (double)h, m, state, out);
}

// ---- k_roi_weights (appendix E) ---------------------------------------------------------------------------------------
// k_consistency's form without a gather: grid = (blocks per item, items), a lane owns a quad of a row, reads the item's centre
// (two doubles, the same address for the whole workgroup), forms dy once and dx per pixel (dx depends on the column alone, dy
// on the row alone: forming dy * dy once changes no bit), and stores 4 bytes where the address allows and bytes otherwise.
// gate may alias out exactly (the in-place form): a lane reads the gate bytes of its own quad before it writes them, so out
// carries no __restrict__.  No LDS, no loop, plain vector stores; bytes between rows and between items are never written.
__global__ __launch_bounds__(256) void k_roi_weights(const char *__restrict__ cen, long long cstride, int w, int h, double ax,
                                                     double ay, int soft, WeightArgs gate, char *out, long long out_item,
                                                     long long out_pitch) {
    const int qw = (w + 3) >> 2;   // quads per row
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= (unsigned)qw * (unsigned)h) return;
    const int y = (int)(q / (unsigned)qw), x = (int)(q % (unsigned)qw) * 4;
    const int b = blockIdx.y, np = w - x < 4 ? w - x : 4;   // pixels of this quad
    const double *c = reinterpret_cast<const double *>(cen + (long long)b * cstride);   // E1
    const double cx = c[0], cy = c[1];
    const double dy = ((double)y - cy) / ay, dy2 = dy * dy;                               // E2
    unsigned wt[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double dx = ((double)(x + k) - cx) / ax;
        const double e = dx * dx + dy2;
        if (soft) {                                                                       // E3
            double qv = 1.0 - e;
            qv = qv > 0.0 ? qv : 0.0;   // a select: a NaN gives 0
            wt[k] = (unsigned)(int)(qv * 255.0 + 0.5);
        } else {
            wt[k] = e <= 1.0 ? 255u : 0u;                                                 // E4
        }
    }
    if (gate.base) {   // E5
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

void ffl_launch_roi_weights(const char *cen, long long cstride, int n, int w, int h, float ax, float ay, int soft,
                            const WeightArgs *gate, char *out, long long out_item, long long out_pitch, hipStream_t st) {
    const size_t quads = (size_t)((w + 3) / 4) * h;   // below 2^30: 20 * w * h < 2^32
    const WeightArgs g = gate ? *gate : WeightArgs{nullptr, 0, 0};
    hipLaunchKernelGGL(k_roi_weights, dim3((unsigned)((quads + 255) / 256), n), dim3(256), 0, st, cen, cstride, w, h, (double)ax,
                       (double)ay, soft, g, out, out_item, out_pitch);
}
