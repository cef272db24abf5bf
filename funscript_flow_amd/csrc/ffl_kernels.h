// Shared declarations of the gfx950 kernels behind include/ffl.h.
//
// Data layout in HBM (all tightly packed, row-major, sized for level 0 and reused per level):
//   gray   : uint8  [frame slot][h][w]
//   I      : float  [unique frame u][lh][lw]                     level image (blur + resize)
//   R      : float  [unique frame u][5 planes][lh][lw]           polynomial expansion, SoA planes
//   M      : float  [pair b][5 planes][lh][lw]  (two buffers)    G11,G12,G22,h1,h2 before the box blur
//   flow   : float2 [pair b][lh][lw]            interleaved (u,v) exactly as cv2 returns it
// SoA planes (not 20-byte AoS records) so that 64 consecutive lanes read 256 contiguous bytes of
// one channel; the bilinear gather of R1 in UpdateMatrices then hits mostly-shared cache lines.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#define FFL_MAXB 256                 // pairs per batch (= FFL_MAX_BATCH of include/ffl.h)
#define FFL_MAXU (2 * FFL_MAXB)      // unique frames per batch
#define FFL_MAX_LEVELS 4             // pyramid scales (FarnebackOpticalFlowImpl::calc: levels = 3 -> 4 scales)
#define FFL_POLY_N 5
#define FFL_WIN 15
#define FFL_WIN_R 7

struct PolyConsts {
    float g[FFL_POLY_N + 1], xg[FFL_POLY_N + 1], xxg[FFL_POLY_N + 1];
    double gd[FFL_POLY_N + 1], xxgd[FFL_POLY_N + 1];  // (double)g[k], (double)xxg[k]: widened once on the host
    double ig11, ig03, ig33, ig55;
};

struct GaussKernel {
    float k[32];  // full symmetric kernel, ksize taps, centre at k[ksize/2]
    int ksize;
};

// Per-batch tables live in device memory (one copy per compute lane, refreshed by a small stream-ordered H2D
// copy before the batch's first launch): a batch may hold hundreds of pairs (the reference's own operating point
// is 256x256, where only large batches fill the device), far more than fits kernel arguments, and kernels that
// take only pointers and geometry can be replayed from a captured hipGraph.  Every entry is read with a
// wave-uniform index (scalar loads).
struct UTab {  // unique frame u of the batch -> resident frame slot
    int fslot[FFL_MAXU];
};

struct PairTab {  // per pair of the batch
    int u0[FFL_MAXB], u1[FFL_MAXB];          // unique-frame indices of prev / next
    float *flow[FFL_MAX_LEVELS][FFL_MAXB];   // the pair's flow field at every level (level 0: its flow slot);
                                             // level k + 1 is the input of level k's x2 upsample
    struct Pass1Result *res[FFL_MAXB];       // where the pair's pass-1 record goes (mapped pinned memory)
};

struct BatchTab {
    UTab ut;
    PairTab pt;
};

struct Pass1Result {  // written by k_pass1_final, mirrored to pinned host memory
    int x, y;
    float div_val;
    int weighted;     // 0: an ordinary record.  1 (k_pass1_weighted_final): mag_sum is already the mean, see below
    double mag_sum;   // sum of sqrt(u^2+v^2) over the image (mean = mag_sum / (w*h)); under a weight map the record carries
                      // its own divisor by holding the quotient: (sum of mag * weight) / SW, +0.0 when SW == 0
};
// the mean magnitude of a record as a double, before its one rounding to float (npx = (double)w * (double)h)
__host__ __device__ inline double ffl_record_mean(const Pass1Result &r, double npx) {
    return r.weighted ? r.mag_sum : r.mag_sum / npx;
}

// The input front-end (k_frontend, k_frontend_dev): a decoded frame -> the gray crop window of its (virtual) resize.
enum { FFL_FRONT_GENERIC = 0, FFL_FRONT_AREA2 = 1, FFL_FRONT_IDENTITY = 2 };
enum { FFL_SRC_GRAY = 0, FFL_SRC_BGR = 1, FFL_SRC_YUV = 2, FFL_SRC_YUV16 = 3, FFL_SRC_ANY = -1 };  // YUV16: 4:2:0 in 16-bit
                                                                                       // samples; ANY: the kernels' own use
struct FrameDesc {  // where one source frame's bytes lie on the device
    const uint8_t *p0, *p1, *p2;  // packed / first channel / Y; chroma: U and V (NV12: p2 = p1 + 1)
    long long pitch0, pitch1, pitch2;
    long long ps, cs;             // plane 0: bytes between horizontal neighbours / between the channels of a pixel
    int c_step;                   // 4:2:0: bytes between horizontally adjacent chroma samples (1 I420, 2 NV12; YUV16: 2, 4)
    int wx, wy;                   // origin of the window the planes hold inside the STORED frame (even; 0, 0: the whole frame)
    int fslot;                    // k_frontend_dev: destination frame slot
};
struct FrontParams {  // what the frames of one launch share
    int kind, rgb;               // FFL_SRC_*; rgb: channel 0 is R
    int sw, sh;                  // full UPRIGHT source size (rule Y6): source coordinates and their clamps stay in these terms
    int cx, cy, ow, oh;          // crop origin inside the resized image, output size
    double scale_x, scale_y;     // 1. / ((double)resize / src), formed on the host
    int mode;                    // FFL_FRONT_*
    int shift16, round16;        // FFL_SRC_YUV16, rule Y5: v8 = min(255, (raw + round16) >> shift16)
    int src;                     // the launch carries stream metadata: a map other than the identity, or full range
    int ax, bx, cx0, ay, by, cy0;  // rule Y6: upright (x, y) is stored (ax x + bx y + cx0, ay x + by y + cy0)
    int full;                    // rule Y7: full-range 4:2:0
};
// k_frontend_remap, k_frontend_remap_dev: what a map-driven launch carries beside FrontParams, of
// which it reads only the source description -- nothing here is seen by the resize kernels.
#define FFL_REMAP_NONE (-2147483647 - 1)  // qx of a sample without a source (rule R1; FFL_REMAP_NO_SOURCE of include/ffl.h)
struct RemapParams {
    const int2 *map;  // [ss * oh][ss * ow] entries (qx, qy): upright source coordinates in 1/32 px
    int ss, lg;       // supersampling per axis (1, 2, 4) and its log2
};
// k_export_flows: the flow slots of one launch (at most FFL_MAXB) travel as a kernel argument
struct ExportTab {
    int slot[FFL_MAXB];
};

// ffl_import_flows (k_import_pass1): item b, pixel (x, y), component c lies at base + b*item + y*pitch + x*ps + c*cs
enum { FFL_IMP_F32 = 0, FFL_IMP_F16 = 1, FFL_IMP_BF16 = 2 };   // = FFL_F32, FFL_F16, FFL_BF16 of include/ffl.h
enum { FFL_IMP_ANY = 0,    // element by element
       FFL_IMP_NHWC = 1,   // ps = 2 * element, cs = element; 16-bit: base and pitch also 4-byte aligned
       FFL_IMP_NCHW = 2 }; // float32, ps = 4
struct ImportArgs {
    const char *base;
    long long item, pitch, ps, cs;   // bytes
    float *flow;                     // the context's flow slots (2N floats each)
    Pass1Result *res;                // their records
};

// weight maps: item b's (h, w) uint8 map starts at base + b * item, its rows pitch bytes apart
struct WeightArgs {
    const char *base;
    long long item, pitch;   // bytes; item 0: one map for every item
};

// merged launches: one 1-D grid cut into per-job block ranges
#define FFL_MAX_JOBS 4
// kernel forms of a level: fused 3-tap x1 / x2, or the H and V passes of a pair of radius 4 / 9 / 1 (V = H + 2; the
// radius-1 pair is launched per level only, k_pyr_multi has no case for it)
enum { FFL_PYR_NONE = -1, FFL_PYR_F1 = 0, FFL_PYR_F2, FFL_PYR_H4, FFL_PYR_H9, FFL_PYR_V4, FFL_PYR_V9, FFL_PYR_H1 };
struct PyrJob {  // one level of the pyramid (caller fills w, h, lw, lh, sx, sy, gk, tmp, tmp_stride, I, I_stride)
    int kind, w, h, lw, lh;
    unsigned gx, gy, first, count;  // grid of one frame, first block of the job, tiles of the job (all frames)
    double sx, sy;                  // (double)w / lw, (double)h / lh
    float *tmp, *I;
    size_t tmp_stride, I_stride;
    GaussKernel gk;
};
struct PyrJobs {
    PyrJob j[FFL_MAX_JOBS];
    int n;
};
struct PolyJob {  // one level of PolyExp (caller fills I, I_stride, R, R_stride, plane, w, h)
    const float *I;
    float *R;
    size_t I_stride, R_stride, plane;
    int w, h;
    unsigned gx, gy, first, count;
    int from_gray;   // the image is formed from the gray frame (level 0's 3-tap blur, taps gk0 / gk1) instead of read from I
    float gk0, gk1;
};
struct PolyJobs {
    PolyJob j[FFL_MAX_JOBS];
    int n;
};

// Tuning knobs (ffl_set_option / ffl_ctx_set_option; results never depend on them).  The process-wide set holds the
// defaults of contexts created afterwards; every context keeps its OWN copy, taken at ffl_create, so two contexts of one
// process (one per GPU, or several on one device) neither share a knob nor invalidate each other's captured graphs.
struct FflOptions {
    int lanes = 2;          // compute lanes (co-scheduled batches) -- fixed once the context exists
    int fuse_first = 10000; // minimum tiles x pairs of a level for the folded first blur+solve launch (0: never)
    int use_graph = 1;      // replay a batch's launches from a captured hipGraph
    int copy_threads = 4;   // host threads sharing a staging copy
    int blur_rows = 0;      // tiles a k_blur_solve workgroup walks down (0: automatic)
    int blur_min_wgs = 3500; // automatic strip length: the longest strips that still give this many workgroups
    int tile_order = 0;     // 0 pair-major, 1 tile-major (ffl_tile_coord)
    int blur_taper = 1;     // 1: the pairs a k_blur_solve launch deals last get shorter strips (ffl_blur_plan), sized from the slots
    int blur_taper_pairs = 0; // > 0: that many pairs in each of the two taper segments, whatever blur_taper says (tests, sweeps)
    int pyr_coarse = 1;     // one-pass kernel for the x1/4 and x1/8 pyramid levels where sizes allow
    int fuse_l0_blur = 1;   // merged expansion: PolyExp forms level 0's image from the gray frame itself; its I plane is not written
    int fb_general = 0;     // 1: ffl_flow_pairs_farneback runs the reference's parameters through the general kernels too
};
// The knobs by name (host only; ffl_api.hip sets and reads them through this table): accepted values lo..hi, and `flag`
// when any value is accepted and stored as != 0.  A new knob is a member above and a row here.
struct FflOptionRow {
    const char *name;
    int FflOptions::*member;
    int lo, hi;
    bool flag;
};
inline constexpr FflOptionRow kFflOptionRows[] = {
    {"lanes", &FflOptions::lanes, 1, 4, false},
    {"fuse_first", &FflOptions::fuse_first, 0, INT_MAX, false},
    {"graph", &FflOptions::use_graph, INT_MIN, INT_MAX, true},
    {"copy_threads", &FflOptions::copy_threads, 1, 16, false},
    {"blur_rows", &FflOptions::blur_rows, 0, 64, false},
    {"blur_min_wgs", &FflOptions::blur_min_wgs, 1, INT_MAX, false},
    {"tile_order", &FflOptions::tile_order, 0, 1, false},
    {"blur_taper", &FflOptions::blur_taper, 0, 1, false},
    {"blur_taper_pairs", &FflOptions::blur_taper_pairs, 0, FFL_MAXB, false},
    {"pyr_coarse", &FflOptions::pyr_coarse, INT_MIN, INT_MAX, true},
    {"fuse_l0_blur", &FflOptions::fuse_l0_blur, INT_MIN, INT_MAX, true},
    {"fb_general", &FflOptions::fb_general, 0, 1, false},
};

// The launch plan of k_blur_solve (ffl_blur_plan, kernels_farneback.hip): up to three segments of consecutive pairs, each
// a uniform grid of strips dealt by ffl_tile_map.  The bulk walks strips of `nrb` tiles; with taper on, the pairs dealt
// last walk strips of ceil(nrb / 2) and then ceil(nrb / 4) tiles, so the workgroups that start last are also the shortest
// and the launch drains faster.  Every segment starts at a multiple of 8 workgroups (the XCD round-robin).  One segment
// is the launch without taper: same grid, same mapping.  Passed to the kernel by value.
#define FFL_BLUR_SEGS 3
struct BlurSeg {
    int first_block, first_pair, pairs, nrb, strips;  // strips: per tile column
};
struct BlurPlan {
    BlurSeg s[FFL_BLUR_SEGS];
    int n;
};
// workgroup slots of the device per k_blur_solve instantiation (occupancy x compute units), cached by the context
struct BlurSlots {
    int first, first_zero, update, last;  // folded first launch (upsampled / zero initial flow), fused update, a level's last
};

// ---- launchers (each enqueues on `st` and returns; no synchronisation) ----------------------
// all pyramid levels in two launches; false (nothing launched) when a level needs the generic kernels
bool ffl_launch_pyr_multi(const uint8_t *gray_base, size_t gray_stride, const UTab *ut, int nU, const PyrJob *levels, int n,
                          const FflOptions &opt, hipStream_t st);
// l0 != nullptr: the last level is level 0 and is formed from the gray frames (ffl_polyexp_from_gray_ok(*l0) must hold)
bool ffl_polyexp_from_gray_ok(const PyrJob &l0);
void ffl_launch_polyexp_multi(const PolyJob *levels, int n, int nU, PolyConsts pc, const uint8_t *gray_base, size_t gray_stride,
                              const UTab *ut, const PyrJob *l0, hipStream_t st);
// host paths: one frame, its descriptor a kernel argument; device path: n frames, descriptors tab[0..n) in device memory
void ffl_launch_frontend(const FrameDesc &d, uint8_t *gray, const FrontParams &p, hipStream_t st);
void ffl_launch_frontend_dev(const FrameDesc *tab, int n, uint8_t *gray_base, size_t N, const FrontParams &p, hipStream_t st);
void ffl_launch_frontend_remap(const FrameDesc &d, uint8_t *gray, const FrontParams &p, const RemapParams &r, hipStream_t st);
void ffl_launch_frontend_remap_dev(const FrameDesc *tab, int n, uint8_t *gray_base, size_t N, const FrontParams &p,
                                   const RemapParams &r, hipStream_t st);
// n (<= FFL_MAXB) flow slots of `flow` (2N floats each) -> dst + i * item_stride bytes; layout 0 (H, W, 2), 1 (2, H, W)
void ffl_launch_export_flows(const float *flow, const ExportTab &tab, int n, size_t N, char *dst, long long item_stride,
                             int layout, hipStream_t st);
// n (<= FFL_MAXB) caller fields -> flow slots tab.slot[0..n) + their pass-1 records (through pt, which the import fills);
// dtype FFL_IMP_*, mode FFL_IMP_* (host-checked)
void ffl_launch_import_pass1(const ImportArgs &a, const ExportTab &tab, int n, int dtype, int mode, int w, int h, int pov_mode,
                             PairTab *pt, unsigned long long *pkey, double *psum, hipStream_t st);
void ffl_launch_gray(const uint8_t *bgr, uint8_t *gray, int n_pixels, hipStream_t st);
size_t ffl_pyr_tmp_floats(int w, int h, int lw);  // per-frame size of the level's horizontal-pass buffer
// one level on its own; ffl_pyr_level_ok: the level has one of the forms this serves (checked by ffl_create)
bool ffl_pyr_level_ok(int w, int h, int lw, int lh, int ksize);
void ffl_launch_pyr_level(const uint8_t *gray_base, size_t gray_stride, const UTab *ut, int nU, const PyrJob &level,
                          hipStream_t st);
// pw > 0: the level's initial flow = x2 bilinear upsample of pt.prev (pw x ph), used from registers (and written
// to pt.flow only when store_flow != 0: nothing but the debug capture reads it);
// pw == 0: the flow is read from pt.flow, or taken as zero without touching memory when zero_flow != 0
void ffl_launch_update_matrices(const float *R, size_t R_stride, size_t plane, const PairTab *pt, int level, int nB, float *M,
                                size_t M_stride, int lw, int lh, int pw, int ph, int zero_flow, int store_flow,
                                const FflOptions &opt, hipStream_t st);
// update != 0: the next UpdateMatrices is fused in; the solved flow then only reaches memory when store_flow != 0
// (it is dead until the level's last iteration, which always stores it)
void ffl_launch_blur_solve(const float *Min, float *Mout, size_t M_stride, const float *R, size_t R_stride,
                           size_t plane, const PairTab *pt, int level, int nB, int lw, int lh, int update, int store_flow,
                           const FflOptions &opt, const BlurSlots &slots, hipStream_t st);


void ffl_launch_blur_solve_first(float *Mout, size_t M_stride, const float *R, size_t R_stride, size_t plane,
                                 const PairTab *pt, int level, int nB, int lw, int lh, int pw, int ph, const FflOptions &opt,
                                 const BlurSlots &slots, hipStream_t st);
// the slots of the current device; false when the occupancy query fails
bool ffl_blur_slots(BlurSlots *out);
// the plan of one launch over tiles_x x tiles_y tiles and nB pairs on `slots` workgroup slots (host only, no device);
// returns the grid size
unsigned ffl_blur_plan(int tiles_x, int tiles_y, int nB, int slots, const FflOptions &opt, BlurPlan *plan);

// ---- DIS (kernels_dis.hip) ----------------------------------------------------------------
#define DIS_MAX_PATCHES 4096   // patch flows of one scale in LDS (float2 each)
#define DIS_MAX_SCALES 12
struct DisKParams {
    int w, h, finest, coarsest, stride, gd_iters, vr_iters, mean_norm, spatial_prop, stripes;
    float alpha, gamma, delta;
    size_t pair_floats;              // per-pair scratch region (floats)
    size_t pyr_floats;               // floats of one pyramid (scales finest..coarsest)
    size_t pyr_off[DIS_MAX_SCALES];  // offset of scale finest + i inside a pyramid
    float *dbg;                      // ffl_debug_dis_pair: pair 0's field of (dbg_scale, dbg_stage), else nullptr
    int dbg_scale, dbg_stage;
};
// one workgroup per pair: pyramid, patch search, densification, refinement per scale, then the full-size field into
// pt->flow[0][b]; `scratch` holds nB regions of p.pair_floats floats
void ffl_launch_dis(const UTab *ut, const PairTab *pt, int nB, const uint8_t *gray, size_t gray_stride, float *scratch,
                    const DisKParams &p, hipStream_t st);

int ffl_pass1_blocks(int w, int h);
// pass 1 of the level-0 flows pt->flow[0][b]; records go to pt->res[b]
void ffl_launch_pass1(const PairTab *pt, int nB, int w, int h, int pov_mode, unsigned long long *pkey, double *psum,
                      hipStream_t st);

// pass 2 (k_strip_sums<RadialSums<..>>, k_radial_final) and the plan of ffl_radial_window (k_window_plan)
#define FFL_WINDOW_MAX_RADIUS 32     // = FFL_MAX_RADIUS of include/ffl.h
struct WindowSeq {   // the flow slots of the call's consecutive pairs; travels as a kernel argument (1280 bytes)
    int slot[FFL_MAXB + 2 * FFL_WINDOW_MAX_RADIUS];
};
struct WindowItem {  // one item of the radial grid, in device memory: from the host (ffl_radial) or from k_window_plan
    const float *flow;
    double cx, cy;
    int cut, pad;
};
struct Pass2Record { // = ffl_pass2_record of include/ffl.h (ffl_api.hip asserts the layout)
    double dot, cx, cy;
    float mean_mag, div_val;
    int x, y, cut, pad;
};
struct AxesRecord {  // = ffl_axes_record of include/ffl.h (ffl_api.hip asserts the layout)
    Pass2Record base;   // base.dot = component 0
    double tangential, shift_x, shift_y, reserved;
};
#define FFL_NAXES 4                  // = FFL_N_AXES of include/ffl.h
// workgroups (= partial results per component) of a pass-2 grid per item
int ffl_radial_blocks(int w, int h);
// wytab: 2 * h doubles, [y] = (double)(h - y) / h, [h + y] = (double)y / h (the row weights of FF:780-783)
// The form of a radial launch: nc = 1 -> out is Pass2Record[n] and out[i].dot is written; nc = FFL_NAXES (DESIGN.md section
// 15) -> AxesRecord[n]: base.dot, tangential, shift_x, shift_y and reserved = +0.0.  maps (with nc = FFL_NAXES; section 16,
// appendix W): the items' weight maps, or NULL.  A cut item's means are +0.0.  psum holds ffl_radial_blocks(w, h) doubles per
// sum and item, NS = nc (+ 1 under maps, SW) sums per item: sum c of item b at psum[(b * NS + c) * nblk ..].
struct RadialForm {
    int nc;
    const WeightArgs *maps;
};
void ffl_launch_radial(const WindowItem *tab, int n, int w, int h, int pov_mode, const double *wytab, const RadialForm &form,
                       double *psum, void *out, hipStream_t st);
// Pass 1 under maps: the records of flow slots tab.slot[0..n) of `flow` recomputed under the maps `wa`; psw: one more double
// per workgroup and item next to pkey / psum.
void ffl_launch_pass1_weighted(const WeightArgs &wa, float *flow, Pass1Result *res, const ExportTab &tab, int n, int w, int h,
                               int pov_mode, PairTab *pt, unsigned long long *pkey, double *psum, double *psw, hipStream_t st);
// items first .. first+n-1 of seq -> tab[0..n) and every field but `dot` of the Pass2Record at the head of each of the n
// records that start rec_stride bytes apart at out (sizeof(Pass2Record) or sizeof(AxesRecord)).  cen NULL: the window's
// centres are the records' argmax; else (rule G6; AxesRecord only) they are read from n_seq entries of
// device memory, two doubles (cx, cy) at the head of each, cstride bytes apart.
void ffl_launch_window_plan(const WindowSeq &seq, int n_seq, int first, int n, int radius, float cut_threshold,
                            const Pass1Result *res, const float *flow, int w, int h, const void *cen, long long cstride,
                            WindowItem *tab, void *out, int rec_stride, hipStream_t st);

// per-cell statistics and the variance centre (k_cell_stats, k_grid_centre)
#define FFL_CELLS_MAX 64             // = FFL_MAX_CELLS of include/ffl.h
struct CellRecord {  // = ffl_cell_record of include/ffl.h (ffl_api.hip asserts the layout)
    double mean_u, mean_v, mean_mag, var_mag;
};
struct GridCentre {  // = ffl_grid_centre
    double cx, cy, total_var;
    int cells, empty;
};
// flow slots tab.slot[0..n) of `flow` under a G x G grid -> cells[(b * G + i) * G + j] (may be NULL) and centres[b] (may be
// NULL); rowsum: 2 * G doubles per item (t_i, x_i of rule G5)
void ffl_launch_cell_stats(const float *flow, const ExportTab &tab, int n, int w, int h, int G, CellRecord *cells,
                           GridCentre *centres, double *rowsum, hipStream_t st);

// forward-backward consistency maps (k_consistency): item b's map, from the forward field
// in flow slot fwd.slot[b] and the backward field in bwd.slot[b], goes to out + b * out_item, rows out_pitch bytes apart; gate
// (may be NULL): the maps of rule K6
void ffl_launch_consistency(const float *flow, const ExportTab &fwd, const ExportTab &bwd, int n, int w, int h, float alpha,
                            float beta, int soft, const WeightArgs *gate, char *out, long long out_item, long long out_pitch,
                            hipStream_t st);

// photometric-residual maps (k_residual): item b's map, from the gray frames in frame slots
// fr0.slot[b] and fr1.slot[b] of `gray` (N = w * h bytes each) and the forward field in flow slot fl.slot[b], goes to
// out + b * out_item, rows out_pitch bytes apart; gate (may be NULL): the maps of rule P6
void ffl_launch_residual(const unsigned char *gray, const float *flow, const ExportTab &fr0, const ExportTab &fr1, const ExportTab &fl,
                         int n, int w, int h, float alpha, float beta, int soft, const WeightArgs *gate, char *out,
                         long long out_item, long long out_pitch, hipStream_t st);

// texture (structure-tensor) maps (k_texture): item b's map, from the gray frame in frame slot
// fr.slot[b] of `gray` (w * h bytes each), goes to out + b * out_item, rows out_pitch bytes apart; radius 1..8 (host-checked)
// picks the instantiation; gate (may be NULL): the maps of rule T6, which may be exactly `out` (min-combined in place)
void ffl_launch_texture(const unsigned char *gray, const ExportTab &fr, int n, int w, int h, int radius, float tau, int soft,
                        const WeightArgs *gate, char *out, long long out_item, long long out_pitch, hipStream_t st);

// ---- region tracking and ROI maps (kernels_track.hip; DESIGN.md section 23, appendices Q and E) --------------------
#define FFL_TRACK_MAX_R 32           // = FFL_MAX_TRACK_RADIUS of include/ffl.h
#define FFL_TRACK_MAX_T 8            // = FFL_MAX_TRACKS
enum { TRK_HOLD = 0, TRK_HOME = 1 };                             // = FFL_TRACK_HOLD, FFL_TRACK_HOME
enum { TRK_OK = 0, TRK_CUT = 1, TRK_LOST = 2, TRK_CLAMPED = 4 }; // = FFL_TRACK_* status bits
struct TrackState {  // = ffl_track_state of include/ffl.h (ffl_api.hip asserts the layout)
    double x, y, home_x, home_y;
    long long steps;
    int lost_run, pad;
};
struct TrackRecord { // = ffl_track_record
    double x, y, du, dv, sw;
    int count, status;
};
// n_tracks points through flow slots tab.slot[0..n) of `flow` in order (k_track, one workgroup per track): record (i, t) to
// out[i * n_tracks + t], state[t] read and written.  res: the slots' pass-1 records (rule Q5).  maps.base NULL: no map.
void ffl_launch_track(const float *flow, const Pass1Result *res, const ExportTab &tab, int n, int n_tracks, int w, int h,
                      int radius, int on_cut, float cut_threshold, const WeightArgs *maps, TrackState *state, TrackRecord *out,
                      hipStream_t st);
// item b's elliptical map about the two doubles at cen + b * cstride (k_roi_weights) goes to out + b * out_item, rows
// out_pitch bytes apart; gate (may be NULL): the maps of rule E5, which may be exactly `out` (min-combined in place)
void ffl_launch_roi_weights(const char *cen, long long cstride, int n, int w, int h, float ax, float ay, int soft,
                            const WeightArgs *gate, char *out, long long out_item, long long out_pitch, hipStream_t st);

// ---- template matching about tracked centres (kernels_match.hip) ------------------
#define FFL_MATCH_MAX_P 16           // = FFL_MAX_MATCH_P of include/ffl.h
#define FFL_MATCH_MAX_S 16           // = FFL_MAX_MATCH_S
enum { MCH_SSD = 0, MCH_ZSSD = 1 };                     // = FFL_MATCH_SSD, FFL_MATCH_ZSSD
enum { MCH_FLAT = 1, MCH_POOR = 2, MCH_AMBIGUOUS = 4 }; // = FFL_MATCH_* status bits
struct MatchRecord { // = ffl_match_record of include/ffl.h (ffl_api.hip asserts the layout)
    double x, y;
    int dx, dy;
    long long cost, second;
    int status, pad;
};
// item i searches frame slot fr.slot[i] of `gray` (N bytes each) for n_tracks templates of (2p+1)^2 bytes at tmpl, about the
// two doubles at cen + i * cstride + t * 48 (k_track_match, one workgroup per (track, item)): record (i, t) to
// out[i * n_tracks + t]; write_back 1: an accepted match also overwrites those two doubles
void ffl_launch_track_match(const unsigned char *gray, size_t N, const ExportTab &fr, int n, int n_tracks, int w, int h, int p,
                            int s, int mode, double min_var, double max_mse, double ratio, const unsigned char *tmpl, char *cen,
                            long long cstride, int write_back, MatchRecord *out, hipStream_t st);
// n_tracks templates of (2p+1)^2 bytes out of one frame about the two doubles at cen + t * 48 (k_track_template, rule N10)
void ffl_launch_track_template(const unsigned char *frame, int n_tracks, int w, int h, int p, const char *cen, unsigned char *tmpl,
                               hipStream_t st);

// ---- whole-frame template re-detection (kernels_redetect.hip) ----------------------
#define FFL_REDETECT_MAX_EXCLUDE 32  // = FFL_MAX_REDETECT_EXCLUDE of include/ffl.h
#define RDT_SKIPPED 8                // = FFL_REDETECT_SKIPPED
#define RDT_EXCL_NX 3                // a square of 2 * 32 + 1 columns touches at most 3 tile columns of 64
#define RDT_EXCL_NY 6                // and at most 6 tile rows of 16
// the candidate tiles of a w x h frame (64 x 16), and the 64-bit words of scratch one search takes: a key per tile of the
// frame, the pick's two words, a key per re-walked tile
static inline int ffl_redetect_tiles_x(int w) { return (w + 63) / 64; }
static inline int ffl_redetect_tiles_y(int h) { return (h + 15) / 16; }
static inline size_t ffl_redetect_words(int w, int h) {
    return (size_t)ffl_redetect_tiles_x(w) * (size_t)ffl_redetect_tiles_y(h) + 2 + RDT_EXCL_NX * RDT_EXCL_NY;
}
struct RedetectArgs {   // one call's arguments, the same for its four launches
    const unsigned char *gray;      // the frame slots, N bytes each; item i reads slot fr.slot[i]
    size_t N;
    ExportTab fr;
    int n_tracks, w, h, p, mode, exclude, reach, mask, write_back;
    double min_var, max_mse, ratio;
    const unsigned char *tmpl;      // n_tracks templates of (2p+1)^2 bytes
    char *cen;                      // the two doubles of (item i, track t) at cen + i * cstride + t * 48
    long long cstride;
    const char *trig;               // NULL, or the int32 of (i, t) at trig + i * tstride + t * 48 (rule L1)
    long long tstride;
    unsigned long long *scr;        // sstride words per search i * n_tracks + t
    long long sstride;
    int TX, TY;                     // ffl_redetect_tiles_x / _y of the frame
    int gx, gy;                     // the sweep's grid per search: TX x TY, or what 2 * reach + 1 columns / rows can touch
    int ex, ey;                     // the exclusion sweep's grid per search: what 2 * exclude + 1 columns / rows can touch
    MatchRecord *out;
};
// the four launches of ffl_track_redetect for n items (k_redetect_sweep, k_redetect_pick, k_redetect_sweep masked, k_redetect_final)
void ffl_launch_track_redetect(const RedetectArgs &a, int n, hipStream_t st);

// ---- global-motion fit and compensation (kernels_post.hip) -----------------------
#define FFL_MOTION_NSUMS 12          // = FFL_MOTION_N_SUMS of include/ffl.h; the order of rule C4
enum { MOT_S = 0, MOT_SX, MOT_SY, MOT_SXX, MOT_SXY, MOT_SYY, MOT_SU, MOT_SUX, MOT_SUY, MOT_SV, MOT_SVX, MOT_SVY };
enum { MOT_TRANSLATION = 0, MOT_RIGID = 1, MOT_SIMILARITY = 2, MOT_AFFINE = 3 };   // = FFL_MOTION_* of include/ffl.h
enum { MOT_OK = 0, MOT_EMPTY = 1, MOT_DEGENERATE = 2 };
struct MotionRecord {  // = ffl_motion_record of include/ffl.h (ffl_api.hip asserts the layout)
    double a0, a1, a2, b0, b1, b2;   // rule C2
    double sw;                       // S of the last pass
    int model, status;
};
struct MotionPrior {   // the six doubles of n priors in device memory, `stride` bytes apart (NULL base: none)
    const char *base;
    long long stride;
};

// Rules C5 and C6: the weighted least-squares model of `model` out of the twelve sums s[] (rule C4's order), line for line the
// text of DESIGN.md appendix C.  ONE body for ffl_motion_solve on the host and k_motion_solve on the device; both are compiled
// with -ffp-contract=off, so every line is one rounding per written operation on either side.  A pivot passes when it is
// > 1e-12 * its diagonal entry before elimination (a NaN does not).
__host__ __device__ inline void ffl_motion_solve_body(const double *s, int model, MotionRecord *out) {
    const double S = s[MOT_S], Sx = s[MOT_SX], Sy = s[MOT_SY], Sxx = s[MOT_SXX], Sxy = s[MOT_SXY], Syy = s[MOT_SYY];
    const double Su = s[MOT_SU], Sux = s[MOT_SUX], Suy = s[MOT_SUY], Sv = s[MOT_SV], Svx = s[MOT_SVX], Svy = s[MOT_SVY];
    MotionRecord r;
    r.a0 = r.a1 = r.a2 = r.b0 = r.b1 = r.b2 = 0.0;
    r.sw = S;
    r.model = model;
    r.status = MOT_EMPTY;
    if (S == 0.0) {   // C6: no division is executed
        *out = r;
        return;
    }
    const double ta = Su / S, tb = Sv / S;   // C5.T
    r.a0 = ta;
    r.b0 = tb;
    r.status = MOT_OK;
    const double eps = 1e-12;
    if (model == MOT_RIGID || model == MOT_SIMILARITY) {   // C5.R / C5.S: one pivot D behind the two pivots S
        const double Q = Sxx + Syy;
        const double q = Sx / S, p = Sy / S;
        const double D = (Q - q * Sx) - p * Sy;
        if (!(S > eps * S) || !(D > eps * Q)) {
            r.status = MOT_DEGENERATE;
        } else {
            const double g3 = Svx - Suy;
            const double z3 = (g3 + p * Su) - q * Sv;
            const double rot = z3 / D;
            double sc = 0.0;
            if (model == MOT_SIMILARITY) {
                const double g2 = Sux + Svy;
                const double z2 = (g2 - q * Su) - p * Sv;
                sc = z2 / D;
            }
            r.a0 = (ta - q * sc) + p * rot;
            r.b0 = (tb - p * sc) - q * rot;
            r.a1 = sc;
            r.a2 = -rot;
            r.b1 = rot;
            r.b2 = sc;
        }
    } else if (model == MOT_AFFINE) {   // C5.A: LDL^T of [[S, Sx, Sy], [Sx, Sxx, Sxy], [Sy, Sxy, Syy]], two right-hand sides
        bool ok = S > eps * S;
        double l10 = 0.0, l20 = 0.0, l21 = 0.0, d1 = 0.0, d2 = 0.0;
        if (ok) {
            l10 = Sx / S;
            l20 = Sy / S;
            d1 = Sxx - l10 * Sx;
            ok = d1 > eps * Sxx;
        }
        if (ok) {
            const double m21 = Sxy - l20 * Sx;
            l21 = m21 / d1;
            d2 = (Syy - l20 * Sy) - l21 * m21;
            ok = d2 > eps * Syy;
        }
        if (!ok) {
            r.status = MOT_DEGENERATE;
        } else {
            const double za1 = Sux - l10 * Su, za2 = (Suy - l20 * Su) - l21 * za1;
            const double zb1 = Svx - l10 * Sv, zb2 = (Svy - l20 * Sv) - l21 * zb1;
            r.a2 = za2 / d2;
            r.a1 = za1 / d1 - l21 * r.a2;
            r.a0 = (ta - l10 * r.a1) - l20 * r.a2;
            r.b2 = zb2 / d2;
            r.b1 = zb1 / d1 - l21 * r.b2;
            r.b0 = (tb - l10 * r.b1) - l20 * r.b2;
        }
    }
    *out = r;
}

// One fit pass: the twelve sums of rule C4 of flow slots tab.slot[0..n) into psum (FFL_MOTION_NSUMS * ffl_radial_blocks(w, h)
// doubles per item), then per item the solve into the record at models + b * sizeof(MotionRecord) and, when sums != NULL, its
// twelve sums at sums + 12 * b.  maps NULL: no map.  prior.base NULL: no prior; else item b's prior is six doubles at
// prior.base + b * prior.stride.
void ffl_launch_motion_fit(const float *flow, const ExportTab &tab, int n, int w, int h, const WeightArgs *maps,
                           const MotionPrior &prior, float tau, int model, double *psum, MotionRecord *models, double *sums,
                           hipStream_t st);
// Rule C8: slot dst.slot[b] = slot src.slot[b] minus the model of item b (six doubles at models + b * stride); dst.slot[b] ==
// src.slot[b] is in place.  The launch also names the dst slots and their records (res + slot) in pt, for the ffl_launch_pass1
// the caller queues behind it.
void ffl_launch_motion_subtract(float *flow, Pass1Result *res, const ExportTab &src, const ExportTab &dst, int n, int w, int h,
                                const char *models, long long stride, PairTab *pt, hipStream_t st);

// ---- index rules shared by the kernel files ----------------------------------------------------------------------
__device__ __forceinline__ int ffl_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int ffl_reflect101(int p, int n) {  // BORDER_REFLECT_101
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// INTER_LINEAR coordinate rule of the oracle's resize tables, for destination index d.
// `scale` = (double)src / dst (IEEE division: the same double the oracle forms)
__device__ __forceinline__ void ffl_resize_coord(int d, int src, double scale, int &i0, int &i1, float &f) {
    // (the x2 upsample of an even-sized level takes ffl_resize_coord_half of kernels_farneback.hip; useless while the
    // phase waited for its loads, -1.5 % once it did not)
    float fx = (float)((d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= src - 1) { sx = src - 1; fx = 0.f; }
    i0 = sx;
    i1 = sx + 1 < src ? sx + 1 : src - 1;
    f = fx;
}

// XCD-aware order of a 1-D run of `count` tiles: the l-th workgroup of the run (l and l+8 share an XCD under the
// observed round-robin placement; the run must start at a multiple of 8) takes tile (l % 8) * chunk + l / 8, so every
// XCD walks one contiguous piece of the run.  ffl_xcd_blocks(count) workgroups cover the run (up to 7 idle ones).
static inline unsigned ffl_xcd_blocks(unsigned count) { return ((count + 7) / 8) * 8; }
__device__ __forceinline__ bool ffl_xcd_tile(unsigned l, unsigned count, unsigned &t) {
    const unsigned chunk = (count + 7) >> 3;
    t = (l & 7u) * chunk + (l >> 3);
    return (l >> 3) < chunk && t < count;
}

// XCD-aware tile order (speed only, never correctness).  Workgroups are dealt round-robin over the 8
// XCDs, so linear ids l and l+8 share an L2.  Each XCD gets one contiguous run of tiles, walked in
// panels of FFL_PANEL_W tile columns, row-major inside a panel: a tile's left/right neighbour runs
// right next to it in time and its upper/lower neighbour FFL_PANEL_W tiles later, all on the same L2,
// so stencil halos and gather neighbourhoods are re-read from L2 instead of over the fabric.
// Grid: ffl_tile_grid(tiles_x, tiles_y, nB) workgroups, 1-D.  Returns false for padding workgroups.
#ifndef FFL_PANEL_W
#define FFL_PANEL_W 4
#endif
static inline unsigned ffl_tile_grid(int tiles_x, int tiles_y, int nB) {
    const int T = tiles_x * tiles_y;
    return (unsigned)(((T + 7) / 8) * 8 * nB);
}
// order 0 (pair-major): all tiles of pair 0, then all tiles of pair 1, ...
// order 1 (tile-major): an XCD walks its run of tiles and runs every tile for ALL nB pairs back to back.  In a
//   stream, frame j's expansion R is R1 of pair j-1 and R0 of pair j: with the same tile of consecutive pairs
//   resident on one XCD at the same time, the second of those reads is served by that XCD's L2 instead of the
//   fabric (the R planes are 40 of the 68 bytes per pixel an UpdateMatrices pass moves).
// ffl_tile_map: the same for workgroup `blk` of the grid, on the host as well (ffl_debug_blur_plan enumerates a launch).
__host__ __device__ __forceinline__ bool ffl_tile_map(unsigned blk, int tiles_x, int tiles_y, int nB, int order, int &b,
                                                      int &tile_x, int &tile_y) {
    const int T = tiles_x * tiles_y, chunk = (T + 7) >> 3;
    int t;
    if (order == 0) {
        b = blk / (chunk * 8);
        const int l = blk - b * (chunk * 8);
        t = (l & 7) * chunk + (l >> 3);
    } else {
        const int pos = blk >> 3, tt = pos / nB;
        b = pos - tt * nB;
        t = (blk & 7) * chunk + tt;
    }
    if (t >= T) return false;
    const int per_panel = FFL_PANEL_W * tiles_y;
    const int panel = t / per_panel, within = t - panel * per_panel;
    const int left = tiles_x - panel * FFL_PANEL_W;
    const int pw = left < FFL_PANEL_W ? left : FFL_PANEL_W;  // the last panel may be narrower
    tile_y = within / pw;
    tile_x = panel * FFL_PANEL_W + (within - tile_y * pw);
    return true;
}
__device__ __forceinline__ bool ffl_tile_coord(int tiles_x, int tiles_y, int nB, int order, int &b, int &tile_x,
                                               int &tile_y) {
    return ffl_tile_map(blockIdx.x, tiles_x, tiles_y, nB, order, b, tile_x, tile_y);
}

// workgroup `blk` of a planned k_blur_solve launch (BlurPlan) -> its pair, tile column, first tile row and strip length (rows past tiles_y are the
// caller's to clip); false for a padding workgroup.  The segment is found with scalar compares, as k_polyexp_multi's job.
__host__ __device__ __forceinline__ bool ffl_blur_block(const BlurPlan &p, unsigned blk, int tiles_x, int order, int &b,
                                                        int &tile_x, int &row0, int &nrb) {
    int first = 0, pair0 = 0, pairs = p.s[0].pairs, strips = p.s[0].strips;
    nrb = p.s[0].nrb;
#pragma unroll
    for (int i = 1; i < FFL_BLUR_SEGS; i++)
        if (i < p.n && blk >= (unsigned)p.s[i].first_block) {
            first = p.s[i].first_block;
            pair0 = p.s[i].first_pair;
            pairs = p.s[i].pairs;
            strips = p.s[i].strips;
            nrb = p.s[i].nrb;
        }
    int strip_y;
    if (!ffl_tile_map(blk - first, tiles_x, strips, pairs, order, b, tile_x, strip_y)) return false;
    b += pair0;
    row0 = strip_y * nrb;
    return true;
}

// A pointer read from a device-resident table (PairTab / WindowItem) is a generic pointer to the compiler: it
// emits flat_load with per-lane 64-bit address arithmetic and waits on two counters.  Every such pointer is a
// hipMalloc'ed buffer, so its accesses go through these helpers, which name the global address space:
// global_load, saddr form when the base is wave-uniform.  Vectors need 4-byte alignment only.
// Used by the post kernels (k_pass1 -5 %, k_radial -2 %).  NOT by k_blur_solve / k_update_matrices: there the same
// change made the folded launch 3 % slower (1826 -> 1880 us, same-box A/B) -- their coarse-flow gathers stay flat.
#define FFL_GLOBAL __attribute__((address_space(1)))
typedef float ffl_v2f __attribute__((ext_vector_type(2), aligned(4)));
typedef float ffl_v4f __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ float2 ffl_gload2(const void *base, size_t byte_off) {
    const ffl_v2f v = *(const FFL_GLOBAL ffl_v2f *)((const char *)base + byte_off);
    return make_float2(v.x, v.y);
}
__device__ __forceinline__ float4 ffl_gload4(const void *base, size_t byte_off) {
    const ffl_v4f v = *(const FFL_GLOBAL ffl_v4f *)((const char *)base + byte_off);
    return make_float4(v.x, v.y, v.z, v.w);
}

// 8- and 16-byte vectors that are only 4-byte aligned: gfx950 global loads/stores of dwordx2/x4 need
// dword alignment only.  What a wave64 global load costs the CU's vector-memory path (cache-resident data, lanes
// contiguous; profiles/tools/micro/vmem_issue.hip): 4 bytes per lane 6.3 cycles, 16 bytes 16.7, 8 bytes 19.5 -- so
// streams use 16-byte accesses (byte taps of the pyramid fetched as words: 54 -> 22 us; PolyExp tiles, flow rows),
// gathers use dwords, and 8-byte loads are avoided (phase V of k_blur_solve with 8-byte loads was slower than with
// dwords; the R1 corner pairs as two dwords instead of one dwordx2: folded launch -3.4 %).
struct __attribute__((packed, aligned(4))) ffl_f2u { float x, y; };
struct __attribute__((packed, aligned(4))) ffl_f4u { float x, y, z, w; };

// Element `idx` of a plane whose base is wave-uniform: base in scalar registers + a 32-bit per-lane byte offset -- the
// global_load / global_store "saddr" form, no per-lane 64-bit address arithmetic (a tenth of UpdateMatrices' vector
// instructions were 64-bit adds).  Offsets fit 32 bits: ffl_create rejects sizes with 20 * w * h >= 2^32.
template <typename T>
__device__ __forceinline__ const T *ffl_at(const float *base, unsigned idx) {
    return reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + idx * 4u);
}
template <typename T>
__device__ __forceinline__ T *ffl_at(float *base, unsigned idx) {
    return reinterpret_cast<T *>(reinterpret_cast<char *>(base) + idx * 4u);
}

// The two horizontally adjacent corners of a bilinear gather / one coarse-flow vector.  A wave64 global load of 8 bytes
// per lane occupies the CU's vector-memory path for ~19 cycles, one of 4 bytes for ~6 and one of 16 bytes for ~17
// (cache-resident data, profiles/tools/micro/vmem_issue.hip): two dword loads are cheaper than one dwordx2.
__device__ __forceinline__ ffl_f2u ffl_ld_corner(const float *plane_base, unsigned idx) {
    ffl_f2u v;
    v.x = *ffl_at<float>(plane_base, idx);
    v.y = *ffl_at<float>(plane_base, idx + 1u);
    return v;
}

// update-matrices body shared by the standalone kernel and the fused blur+solve+update kernel, in three
// steps so that the R1 neighbourhood can be fetched in more than one way:
//   ffl_um_locate   where pixel (x, y) displaced by (dx, dy) lands in R1 and its bilinear weights
//   (gather)        b[c] = a00 * R1c(x1, y1) + a01 * R1c(x1+1, y1) + a10 * R1c(x1, y1+1) + a11 * R1c(x1+1, y1+1)
//   ffl_um_finish   the polynomial-difference terms, border scaling and the 5 products
struct UmLoc {
    int x1, y1;
    float a00, a01, a10, a11;
    bool inside;  // all four corners inside the image
};
__device__ __forceinline__ UmLoc ffl_um_locate(int w, int h, int x, int y, float dx, float dy) {
    UmLoc L;
    float fx = x + dx, fy = y + dy;
    L.x1 = (int)floorf(fx);
    L.y1 = (int)floorf(fy);
    fx -= L.x1;
    fy -= L.y1;
    L.inside = (unsigned)L.x1 < (unsigned)(w - 1) && (unsigned)L.y1 < (unsigned)(h - 1);
    L.a00 = (1.f - fx) * (1.f - fy);
    L.a01 = fx * (1.f - fy);
    L.a10 = (1.f - fx) * fy;
    L.a11 = fx * fy;
    return L;
}

// The inside / outside cases are selects, not a branch: a divergent branch around loaded values makes the compiler wait
// for every outstanding load (vmcnt(0)), the next item's prefetched ones included.
__device__ __forceinline__ void ffl_um_finish(const float (&r0)[5], const float (&b)[5], bool inside, int w, int h, int x,
                                              int y, float dx, float dy, float (&out)[5]) {
    // border[5] = {0.14, 0.14, 0.4472, 0.4472, 0.4472} as selects (no runtime-indexed array)
#define FFL_BORDER(i) ((i) < 2 ? 0.14f : 0.4472f)
    float r2 = inside ? b[0] : 0.f;
    float r3 = inside ? b[1] : 0.f;
    float r4 = inside ? (r0[2] + b[2]) * 0.5f : r0[2];
    float r5 = inside ? (r0[3] + b[3]) * 0.5f : r0[3];
    float r6 = inside ? (r0[4] + b[4]) * 0.25f : r0[4] * 0.5f;
    r2 = (r0[0] - r2) * 0.5f;
    r3 = (r0[1] - r3) * 0.5f;
    r2 += r4 * dy + r6 * dx;
    r3 += r6 * dy + r5 * dx;
    if ((unsigned)(x - 5) >= (unsigned)(w - 10) || (unsigned)(y - 5) >= (unsigned)(h - 10)) {
        float scale = (x < 5 ? FFL_BORDER(x) : 1.f) * (x >= w - 5 ? FFL_BORDER(w - x - 1) : 1.f) *
                      (y < 5 ? FFL_BORDER(y) : 1.f) * (y >= h - 5 ? FFL_BORDER(h - y - 1) : 1.f);
#undef FFL_BORDER
        r2 *= scale; r3 *= scale; r4 *= scale; r5 *= scale; r6 *= scale;
    }
    out[0] = r4 * r4 + r6 * r6;
    out[1] = (r4 + r5) * r6;
    out[2] = r5 * r5 + r6 * r6;
    out[3] = r4 * r2 + r6 * r3;
    out[4] = r6 * r2 + r5 * r3;
}

// ---- Farneback with caller-chosen parameters (kernels_farneback_general.hip) ----------------
#define FBG_MAX_R 95          // widest level Gaussian: 2 * 95 + 1 = 191 taps (larger ones are refused)
#define FBG_MAX_SCALES 13     // levels 0..12
#define FBG_MAX_M 31          // winsize 63
struct FbgGauss {             // getGaussianKernel(2r + 1, sigma) as the symmetric half: k[j] = kernel[r + j]
    float k[FBG_MAX_R + 1];
    int r;
};
struct FbgPoly {              // FarnebackPrepareGaussian(poly_n, poly_sigma)
    float g[8], xg[8], xxg[8];
    double ig11, ig03, ig33, ig55;
};
#define FBG_USE_INITIAL_FLOW 4u   // = FFL_FB_USE_INITIAL_FLOW, FFL_FB_GAUSSIAN_WINDOW of include/ffl.h
#define FBG_GAUSSIAN_WINDOW 256u
struct FbgWin {               // F.7: the Gaussian window's taps k[0..m] (m = winsize / 2, sigma = 0.3 m), host-computed
    float k[FBG_MAX_M + 1];
    int m;
};
struct FbgPlan {              // one parameter set on one frame size (host-side; kernels take pieces of it by value)
    int levels, iterations, poly_n, m;  // levels actually used (A.1's min_size rule), window half-width m = winsize / 2
    float mul;                          // (float)(1 / pyr_scale): the flow upsample factor
    unsigned mode;                      // FBG_* bits of ffl_flow_pairs_farneback_ex (0: box window, zero initial flow)
    FbgWin win;                         // the window's taps when mode has FBG_GAUSSIAN_WINDOW
    float seed_scale;                   // F.8: (float)pyr_scale^levels, the factor of the coarsest level's seeded flow
    int lw[FBG_MAX_SCALES], lh[FBG_MAX_SCALES];
    FbgGauss gk[FBG_MAX_SCALES];
    FbgPoly poly;
    size_t r_off[FBG_MAX_SCALES];       // float offset of level k inside one frame's R region
    size_t r_frame;                     // floats of one frame's R region (5 planes of every level)
};
struct FbgWork {              // where a batch's working set lives (the lane's buffers or the general-path work area)
    float *R;                 // nU regions of plan.r_frame floats
    float *M;                 // n * 5N floats; the full-resolution blur planes (2 * nU * N floats) use it first
    float *fa, *fb;           // n * 2N floats each: the level flows (ping-pong); fa holds the level images first
};
// the whole batch: every level of every unique frame, then the level chain of every pair into pt->flow[0][b]
void ffl_launch_fb_general(const UTab *ut, const PairTab *pt, int n, int nU, const uint8_t *gray, size_t gray_stride, int w,
                           int h, const FbgPlan &plan, const FbgWork &wk, hipStream_t st);
