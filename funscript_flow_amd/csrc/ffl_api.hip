// C ABI (include/ffl.h) of the gfx950 pair-motion path: context, slots, streams, batch schedule.
//
// Streams: `copy` carries the pinned H2D frame transfers (+ the BGR->gray kernel); every compute lane
// has its own stream and work buffers; `post` carries pass 2.  A batch waits on its frames' upload
// events; an upload into a frame slot waits on the batch events of the lanes that last read it; each
// batch records ONE event that stands for "slots ready / frames released / lane buffers free".  Result
// records are stored by the reduction kernels straight into mapped pinned memory, so no tiny D2H
// copies are queued.  No host synchronisation happens inside ffl_upload_frame / ffl_flow_pairs, so
// uploads of the next frames overlap the kernels of the previous batch (north_star: "staged to HBM via
// pinned hipMemcpyAsync on a side stream").
#include "../../include/ffl.h"
#include "ffl_kernels.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#define FFL_EV_RING 16
#define FFL_RAW_RING 4

// Every runtime resource of a context belongs to one of these move-only handles (the only callers of hipFree, hipHostFree
// and the *Destroy calls): a null handle destroys as a no-op, reset() frees now and reports what the runtime answered.
// They read like the raw handle wherever one is expected; put() is the out-parameter of a create call.
template <class H, class Arg, hipError_t (*Free)(Arg)>
struct Owned {
    H h = H();
    Owned() = default;
    explicit Owned(H take) : h(take) {}
    Owned(Owned &&o) noexcept : h(o.release()) {}  // move-only: no copies are generated
    Owned &operator=(Owned &&o) noexcept { std::swap(h, o.h); return *this; }  // o frees what *this held
    ~Owned() { reset(); }
    hipError_t reset() { return h ? Free(release()) : hipSuccess; }
    H release() { H t = h; h = H(); return t; }
    H *put() { reset(); return &h; }
    operator H() const { return h; }
    H operator->() const { return h; }
};
template <class T> struct DevBuf : Owned<T *, void *, hipFree> {  // hipMalloc'ed array of T
    hipError_t alloc(size_t count) { return hipMalloc(this->put(), sizeof(T) * count); }
};
template <class T> struct PinBuf : Owned<T *, void *, hipHostFree> {  // page-locked host array of T
    hipError_t alloc(size_t count, unsigned flags) { return hipHostMalloc(this->put(), sizeof(T) * count, flags); }
};
typedef Owned<hipEvent_t, hipEvent_t, hipEventDestroy> Event;
typedef Owned<hipStream_t, hipStream_t, hipStreamDestroy> Stream;
typedef Owned<hipGraph_t, hipGraph_t, hipGraphDestroy> Graph;
typedef Owned<hipGraphExec_t, hipGraphExec_t, hipGraphExecDestroy> GraphExec;

static thread_local std::string g_create_error = "";
// The process-wide option set (ffl_set_option): the defaults of contexts created AFTERWARDS.  Every context copies it at
// ffl_create (ffl_ctx::opt) and is from then on only changed through ffl_ctx_set_option, which bumps that context's own
// graph epoch -- two contexts of one process (one per GPU) share no knob and do not invalidate each other's graphs.
//   fuse_first  a level's initial UpdateMatrices runs inside its first blur+solve launch when the level has at least this
//               many 64x16 tiles over the batch (0: never).  The folded launch saves an M write + read but runs its extra
//               phase at 3 workgroups per CU: worth it only where the launch is long enough to be bandwidth-bound (1080p,
//               B = 32: level 0 2093 vs 1018 + 1217 us; level 2 157 vs 65 + 68 us; level 3 138 vs 34 + 45 us)
//   use_graph   a batch's ~20 launches are captured once per (lane, batch shape, option epoch) into a hipGraph and
//               replayed: the kernels take only pointers and geometry (per-batch indices live in the lane's device table),
//               so nothing in the graph changes from batch to batch.  Host time per batch drops from one launch call per
//               kernel to one graph launch -- what matters at the reference's 256x256 operating point, where a whole
//               batch is a fraction of a ms.
static FflOptions g_opts;
static std::mutex g_opt_mu;

// Events come from small rings, one per stream (a lane's "batch finished" events, the upload events of stream `copy`, the
// events of stream `post`), and what the slot tables hold are REFERENCES to ring entries: (ring, ticket).  An entry is
// recorded again once the ring has gone round.  A reference that outlived its entry must not be waited on any more: the
// event it names now stands for a much LATER operation of that stream -- possibly one that is still running -- and waiting
// for it serialises things that have nothing to do with each other.  (Rounds 1-3 kept bare hipEvent_t handles.  Harmless
// for correctness, since "later work of the same stream" is a conservative wait, but not for speed: with 131 or 132 frame
// slots at B = 32 a slot's last-use handle of the OTHER lane went 33 batches without being refreshed, and from the moment
// the lanes' 16-entry rings wrapped every upload waited for the batch in flight: 5.1 -> 8.9 ms per batch from batch 33 on,
// profiles/r04_pcie_chunk_length.txt.)  So: record() waits on the host for the entry it is about to hand out again -- that
// operation is `size` operations old and practically always long finished -- which makes "stale" imply "completed", and
// EvRef::get() answers nullptr for a stale reference: nothing to wait for.  A ticket is handed out only once its entry has
// been recorded, so no reference ever names an entry that still holds an older operation.
struct EvRef;
struct EvRing {
    std::vector<Event> ev;
    unsigned long long next = 0;     // tickets handed out so far
    unsigned long long settled = 0;  // settle_next() has succeeded for every ticket below this
    hipError_t create(int n) {
        ev = std::vector<Event>(n);
        for (auto &e : ev) {
            hipError_t r = hipEventCreateWithFlags(e.put(), hipEventDisableTiming);
            if (r != hipSuccess) return r;
        }
        return hipSuccess;
    }
    // the entry the next record() hands out: its previous operation (`size` operations ago) must be over.  Waits at most
    // once per ticket, so a caller may settle early (run_batch, before it writes the entry's table) and record later.
    hipError_t settle_next() {
        if (next < ev.size() || next < settled) return hipSuccess;
        const hipError_t r = hipEventSynchronize(ev[next % ev.size()]);
        if (r == hipSuccess) settled = next + 1;
        return r;
    }
    // the next entry recorded on `st`; *out names it and `next` advances only once the record has succeeded
    hipError_t record(hipStream_t st, EvRef *out);
};
struct EvRef {
    const EvRing *ring = nullptr;
    unsigned long long ticket = 0;
    // the event to wait on, or nullptr when there is nothing (never set, or the entry has been handed out again: completed)
    hipEvent_t get() const { return (ring && ring->next - ticket <= ring->ev.size()) ? ring->ev[ticket % ring->ev.size()].h : nullptr; }
};
inline hipError_t EvRing::record(hipStream_t st, EvRef *out) {
    hipError_t r = settle_next();
    if (r == hipSuccess) r = hipEventRecord(ev[next % ev.size()], st);
    if (r == hipSuccess) *out = EvRef{this, next++};
    return r;
}
static inline EvRef ev_latest(const EvRing &r) { return r.next ? EvRef{&r, r.next - 1} : EvRef{}; }

struct ProfRec {
    int cls;
    hipEvent_t a, b;
    bool shared_start;  // `a` is the previous record's `b`
};

struct LevelGeom {
    int lw, lh, ksize;
    double sigma;
    GaussKernel gk;
};
struct Geometry { int levels = 0; LevelGeom lv[8]; };  // level_geometry(width, height)

// What a context of (width, height, n_frame_slots, n_flow_slots, max_batch) allocates, in elements (context_layout):
// ffl_create allocates from it, ffl_estimate_bytes sums it and ffl_farneback_extra_bytes reads R.  The small tables (and the
// 16 padding bytes of d_gray) are not listed: the estimate covers them with an allowance.
struct Layout {
    // per lane (the same for every lane)
    size_t i_off[8], t_off[8], r_off[8];  // float offset of level k inside d_I / d_T (pyramid horizontal-pass buffer) / d_R
    size_t I, T, R;                       // floats of d_I, d_T, d_R: all levels of the 2 * max_batch unique frames of a batch
    size_t M, flow;                       // floats of each of d_M[0], d_M[1] / of each of d_flowA, d_flowB
    size_t p1, tab;                       // pass-1 partial keys, and as many sums / entries of the pinned table ring h_tab
    // per context
    size_t gray, bgr;   // bytes of d_gray / d_bgr, and of their pinned staging areas
    size_t slots, res;  // floats of d_flow / result records h_res
};

// Staging copies (caller's pageable ndarray -> pinned memory) bound the PCIe-inclusive rate from 3-channel frames:
// one host thread moves ~22 GB/s, a 1080p BGR stream at 5 k pairs/s needs 31.  A few persistent helper threads share
// each large copy by rows (created on first use, joined in ffl_destroy).
struct CopyPool {
    // one share of a staging copy: global rows g0 .. g1-1 of a run of `nf` equally shaped frames (row g belongs to frame
    // g / rows); frame f is read from srcs[f] (row pitch src_pitch) and lands at dst + f * dst_frame (rows packed)
    struct Job {
        uint8_t *dst;
        const uint8_t *const *srcs;
        size_t row_bytes, dst_frame;
        ptrdiff_t src_pitch;
        int rows, g0, g1;
    };
    std::vector<std::thread> workers;
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::vector<Job> jobs;   // one slot per worker
    std::vector<char> busy;
    bool stop = false;

    static void run(const Job &j) {
        int g = j.g0;
        while (g < j.g1) {
            const int f = g / j.rows, y0 = g - f * j.rows;
            const int y1 = (j.g1 - f * j.rows) < j.rows ? (j.g1 - f * j.rows) : j.rows;  // rows y0 .. y1-1 of frame f
            uint8_t *d = j.dst + (size_t)f * j.dst_frame + (size_t)y0 * j.row_bytes;
            const uint8_t *s = j.srcs[f] + (ptrdiff_t)y0 * j.src_pitch;
            if (j.src_pitch == (ptrdiff_t)j.row_bytes)
                memcpy(d, s, j.row_bytes * (size_t)(y1 - y0));
            else
                for (int y = y0; y < y1; y++, d += j.row_bytes, s += j.src_pitch) memcpy(d, s, j.row_bytes);
            g += y1 - y0;
        }
    }
    void start(int n) {
        jobs.resize(n);
        busy.assign(n, 0);
        for (int i = 0; i < n; i++)
            workers.emplace_back([this, i] {
                std::unique_lock<std::mutex> lk(mu);
                for (;;) {
                    cv_work.wait(lk, [&] { return stop || busy[i]; });
                    if (stop) return;
                    Job j = jobs[i];
                    lk.unlock();
                    run(j);
                    lk.lock();
                    busy[i] = 0;
                    cv_done.notify_all();
                }
            });
    }
    // `nf` frames of rows x row_bytes (source row pitch src_pitch) into consecutive packed frames at dst, the run's rows
    // split evenly over the helpers + the caller.  A run of many SMALL frames (257 frames of 64 KB per batch at the
    // reference's 256x256 operating point) is shared like one large frame: copied frame by frame on the calling thread it
    // cost 0.7 ms per batch -- half of what the device needs for the batch -- and made the host the bottleneck.
    void copy(uint8_t *dst, const uint8_t *const *srcs, int nf, ptrdiff_t src_pitch, size_t row_bytes, int rows, int threads) {
        const int total = nf * rows;
        const int parts = (row_bytes * (size_t)total < (size_t)(1 << 20) || threads < 2) ? 1 : (threads < total ? threads : total);
        if (parts > 1 && (int)workers.size() < parts - 1) {
            // (re)size once; helpers are idle here because copy() is only called under the context's upload lock (up_mu)
            shutdown();
            stop = false;
            start(parts - 1);
        }
        const int per = (total + parts - 1) / parts;
        const size_t dst_frame = row_bytes * (size_t)rows;
        if (parts > 1) {
            std::unique_lock<std::mutex> lk(mu);
            for (int p = 1; p < parts; p++) {
                const int g0 = p * per, g1 = g0 + per < total ? g0 + per : total;
                if (g0 >= g1) continue;
                jobs[p - 1] = {dst, srcs, row_bytes, dst_frame, src_pitch, rows, g0, g1};
                busy[p - 1] = 1;
            }
            cv_work.notify_all();
        }
        run({dst, srcs, row_bytes, dst_frame, src_pitch, rows, 0, per < total ? per : total});
        if (parts > 1) {
            std::unique_lock<std::mutex> lk(mu);
            cv_done.wait(lk, [&] {
                for (char b : busy)
                    if (b) return false;
                return true;
            });
        }
    }
    void shutdown() {
        {
            std::unique_lock<std::mutex> lk(mu);
            stop = true;
            cv_work.notify_all();
        }
        for (auto &t : workers) t.join();
        workers.clear();
    }
};

struct ffl_ctx {
    int device = 0, w = 0, h = 0;
    FflOptions opt;      // this context's own option set (copied from the process-wide defaults at ffl_create)
    int opt_epoch = 0;   // bumped by every applied ffl_ctx_set_option: a graph is only replayed under the options it was captured with
    int graph_captured = 0, graph_replayed = 0, graph_failed = 0;  // ffl_graph_stats
    BlurSlots blur_slots = {};  // resident workgroups of the k_blur_solve instantiations on this device (ffl_blur_plan's taper)
    CopyPool pool;
    int n_fslots = 0, n_slots = 0, max_batch = 0;
    size_t N = 0;
    Geometry geo;
    Layout lay;
    PolyConsts pc;
    Stream s_copy, s_post;  // uploads (+gray) / pass 2 and flow uploads
    // Compute lanes: each ffl_flow_pairs batch runs on the next lane (stream + its own work buffers),
    // so consecutive batches execute concurrently and the device overlaps one batch's f64-bound box
    // filter with another's bandwidth-bound UpdateMatrices / PolyExp.
    struct Lane {
        Stream st;
        EvRing ring;  // one "batch finished" event per batch (FFL_EV_RING entries)
        DevBuf<float> d_gen;  // general-path work area (ffl_flow_pairs_farneback), allocated when d_R is too small
        size_t gen_cap = 0;   // its floats: the largest request seen
        DevBuf<float> d_I, d_T, d_R, d_M[2], d_flowA, d_flowB;  // Layout: I, T, R, M, flow
        DevBuf<unsigned long long> d_pkey;
        DevBuf<double> d_psum;
        // per-batch index tables: device copy + a ring of pinned host copies (entry e belongs to ring entry e)
        DevBuf<BatchTab> d_tab; PinBuf<BatchTab> h_tab;
        // the frame-only work of every level on this lane's buffers, coarsest level first (the order of the merged
        // launches): level k is entry geo.levels - k.  Filled once by ffl_create
        PyrJob pyr[FFL_MAX_JOBS] = {};
        PolyJob poly[FFL_MAX_JOBS] = {};
        int n_jobs = 0;
        struct GraphEntry {
            int n, nU, pov, epoch;
            Graph graph;
            GraphExec exec;
        };
        std::vector<GraphEntry> graphs;
    };
    std::vector<Lane> lanes;
    unsigned next_lane = 0;
    // frames
    DevBuf<uint8_t> d_gray;        // [n_fslots][N]
    DevBuf<uint8_t> d_bgr;         // [n_fslots][3N] staging for 3-channel uploads
    PinBuf<uint8_t> h_stage_gray;  // pinned [n_fslots][N]   (separate, so that runs of slots are contiguous)
    PinBuf<uint8_t> h_stage_bgr;   // pinned [n_fslots][3N]
    std::vector<EvRef> ev_uploaded;  // per frame slot: the upload call that filled it (one event per call, up_ring)
    EvRing up_ring;                  // 2 * FFL_EV_RING entries
    // [frame slot * frame_readers() + r]: the last reader of the slot on stream r -- r < n_lanes: that lane's last batch (the
    // lane's ring); r = n_lanes: the last ffl_residual_weights or ffl_texture_weights call, on stream `post` (post_ring).  An upload waits for all
    std::vector<EvRef> ev_last_use;
    size_t frame_readers() const { return lanes.size() + 1; }
    std::vector<char> frame_valid;
    std::vector<int> u_of_fslot;      // scratch of run_batch: frame slot -> index among the batch's unique frames (-1 outside)
    std::vector<char> slot_mark;      // scratch of check_flow_slots: flow slot already named in this call
    // ffl_upload_frames_raw: decoded source frames pass through a small ring of pinned + device buffers
    // (grown on demand to the largest source seen); `ev` = the frame's k_frontend has consumed the buffer
    struct RawBuf {
        PinBuf<uint8_t> h;
        DevBuf<uint8_t> d;
        size_t cap = 0;
        Event ev;
        bool busy = false;
    };
    RawBuf raw[FFL_RAW_RING];
    unsigned raw_next = 0;
    EvRing post_ring;  // events of the calls that queue on stream `post` (publish_post), FFL_EV_RING entries
    // device-memory I/O (ffl_upload_frames_device / ffl_export_flows / ffl_import_flows / ffl_radial_window): the event
    // recorded on the caller's stream (waited for at once, so one is enough), and, allocated on first use, the per-call
    // frame descriptor tables -- a pinned copy per up_ring entry (n_fslots descriptors each) and the device table
    // k_frontend_dev reads (`copy`)
    Event ev_caller;
    PinBuf<FrameDesc> h_dtab; DevBuf<FrameDesc> d_dtab;
    // the source maps of ffl_remap_create: the device copy, what the upload calls check a source
    // against, the upright bounding box of its taps (rule R6) and the upload call that read it last (ffl_remap_destroy
    // waits for it).  Users hold up_mu, as every uploader does.
    struct Remap {
        DevBuf<int2> d;
        int ss = 0, sw = 0, sh = 0;   // supersampling; the upright source size
        int ux[2] = {0, 0}, uy[2] = {0, 0};
        EvRef last;
    };
    Remap remaps[FFL_MAX_REMAPS];
    // flow slots
    DevBuf<float> d_flow;             // [n_slots][2N]
    // Result records live in pinned, device-mapped host memory: the reduction kernels store their
    // 24-byte record straight into it (visible after the slot's event), so no D2H copies are queued.
    PinBuf<Pass1Result> h_res;        // pinned [n_slots]
    Pass1Result *d_res = nullptr;     // device alias of h_res
    std::vector<EvRef> ev_slot_done;  // per flow slot: the batch (a lane's ring) or pass-2 / flow-upload call (post_ring) that used it last
    std::vector<char> slot_state;     // 1: queued/ready, 0: empty or its batch failed
    // Stream `post`'s tables and scratch: ONE copy of each, shared by ffl_upload_flow, ffl_import_flows, ffl_radial and
    // ffl_radial_window.  That is safe because every kernel and copy that touches them is queued on stream `post`, by a
    // call that holds post_mu while it queues: a user runs after the previous one has finished, so nothing read from a
    // buffer was left there by another call and nothing is overwritten while it is still read.  The host writes only the
    // two pinned tables, each while the stream holds no copy out of it: h_ptab after ffl_upload_flow has drained the
    // stream, h_wtab by ffl_radial, the one call that copies it and that returns only once the stream has drained.
    DevBuf<PairTab> d_ptab; PinBuf<PairTab> h_ptab;    // pass 1: flow[0][b] and res[b] of the call's items (host: item 0, ffl_upload_flow)
    DevBuf<unsigned long long> d_pskey;                // pass-1 partial keys of max_batch items (lay.p1)
    DevBuf<double> d_rpsum;                            // partial sums of either pass: p1_blocks per item, FFL_MAXB items (pass 2
                                                       // takes up to FFL_MAXB whatever max_batch is, and never more blocks than pass 1)
    DevBuf<WindowItem> d_wtab; PinBuf<WindowItem> h_wtab;  // pass-2 items, FFL_MAXB entries (host: ffl_radial; device: k_window_plan)
    DevBuf<double> d_wytab;                            // pass-2 row weights (h - y) / h and y / h
    PinBuf<Pass2Record> h_radial; Pass2Record *d_radial = nullptr;  // ffl_radial's mapped pinned records (only `dot` is used) and their device alias
    // The extra scratch of stream `post`, one buffer per row of kPostScratch: allocated by the first call that needs it
    // (post_scratch) and held to ffl_destroy, under the single-copy rule above -- stream `post` alone touches them, so a call
    // of another form queued between two users of a buffer never sees or disturbs it.
    // The four-component calls (ffl_radial_axes, ffl_radial_window_axes, ffl_radial_window_axes_centres; DESIGN.md section
    // 15): FFL_NAXES * ffl_radial_blocks partials per item.
    DevBuf<double> d_apsum;
    // ffl_radial_axes' mapped pinned records and their device alias, allocated with d_apsum.
    PinBuf<AxesRecord> h_axes;
    AxesRecord *d_axes = nullptr;
    // The weighted calls (ffl_pass1_weighted, ffl_radial_window_axes_weighted): pass 1's SW per
    // workgroup, or pass 2's FFL_NAXES + 1 sums per workgroup.
    DevBuf<double> d_wpsum;
    // ffl_cell_stats: t_i and x_i of rule G5 per cell row, FFL_MAX_CELLS rows per item.
    DevBuf<double> d_cellrow;
    // ffl_motion_fit: FFL_MOTION_NSUMS partials per workgroup of the radial grid.
    DevBuf<double> d_mpsum;
    // ffl_track_redetect: ffl_redetect_words 64-bit words per search, max_batch x FFL_MAX_TRACKS searches.
    DevBuf<double> d_rdscr;
    int p1_blocks = 0;
    // profiling
    unsigned prof_mask = 0;   // bit k set: bracket every launch of kernel class k with HIP events
    // caller-visible page-locked buffers (ffl_host_alloc): uploads out of them skip the staging copy
    std::vector<std::pair<PinBuf<uint8_t>, size_t>> host_bufs;
    std::vector<ProfRec> prof_recs;
    std::vector<Event> prof_pool;        // recycled timing events
    hipEvent_t prof_last_end = nullptr;  // end event of the latest timed launch, while nothing followed it
    int prof_last_cls = -1;
    hipStream_t prof_last_stream = nullptr;
    int prof_launches[FFL_K_COUNT] = {0};
    double prof_ms[FFL_K_COUNT] = {0};
    std::string err;
    // Every entry point takes this lock, so calls from several host threads are safe (submit / pass1 / radial on
    // distinct slots may come from different host threads).  The rule: a host wait for the device runs WITHOUT the lock,
    // through wait_unlocked(), and only ever waits on EVENTS, never on a lane's stream -- another thread may be inside
    // hipStreamBeginCapture / EndCapture on that stream (a new batch shape), and synchronising a capturing stream is an
    // error that also invalidates the capture; hipEventSynchronize on an event recorded outside the capture is legal.  The
    // staging memcpy of the uploads and the waits for streams `copy` and `post`, on which nothing is captured, also run
    // without it.  A wait under the lock is rare or a test hook: a ring's settle_next() (its entry is FFL_EV_RING
    // operations old), the eviction of a captured graph, ffl_debug_pair, ffl_download_frame and ffl_profile_read.
    // Two small locks order the users of shared single-copy resources among themselves; both are taken BEFORE `mu`, and
    // up_mu before post_mu where a call needs both (ffl_sync, which releases them before it waits):
    //   up_mu    uploaders: the per-slot staging areas, the copy pool and the raw-frame ring
    //   post_mu  users of stream `post`, its single tables, scratch and result buffer (see d_ptab)
    mutable std::recursive_mutex mu;
    std::mutex up_mu, post_mu;
    int graph_bad_epoch = -1;  // option epoch in which a graph capture failed: batches launch eagerly until it changes
    bool graph_fail_reported = false;
};
typedef std::unique_lock<std::recursive_mutex> CtxLock;

static int set_err(ffl_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

// HIPCHK names the failing call by its text; a call made through a handle is reported AS the runtime call it makes
#define HIPCHK_AS(c, what, call)                                                                          \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return set_err(c, FFL_ERR_HIP, "%s failed: %s (%s:%d)", what, hipGetErrorString(e_), __FILE__, \
                           __LINE__);                                                                     \
    } while (0)
#define HIPCHK(c, call) HIPCHK_AS(c, #call, call)
#define HIPCHK_ALLOC(c, fn, buf, ...) HIPCHK_AS(c, #fn "(" #buf ", " #__VA_ARGS__ ")", (buf).alloc(__VA_ARGS__))

// ---- host-side constants (same published procedure as OpenCV's helpers) -------------------------
static inline int cv_round(double v) { return (int)lrint(v); }

static void gaussian_kernel(int n, double sigma, float *out) {  // getGaussianKernel(n, sigma, CV_32F)
    static const float tab1[] = {1.f};
    static const float tab3[] = {0.25f, 0.5f, 0.25f};
    static const float tab5[] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    static const float tab7[] = {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f};
    const float *fixed = nullptr;
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

// FarnebackPrepareGaussian(n, sigma): g, xg, xxg for x = 0..n and the four entries of the inverse moment matrix that
// PolyExp uses.  The one statement of the procedure: the tuned path calls it with (5, 1.2), the general path with the
// caller's values, and `fb_general = 1` promises the same bits through either.
static void farneback_prepare_gaussian(int n, double sigma, FbgPoly *out) {
    float gg[2 * 7 + 1];
    double s = 0;
    for (int x = -n; x <= n; x++) {
        gg[x + n] = (float)exp(-x * x / (2 * sigma * sigma));
        s += gg[x + n];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) gg[x + n] = (float)(gg[x + n] * s);
    for (int x = 0; x <= n; x++) {
        out->g[x] = gg[x + n];
        out->xg[x] = (float)(x * gg[x + n]);
        out->xxg[x] = (float)(x * x * gg[x + n]);
    }
    double G[6][6];
    memset(G, 0, sizeof(G));
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            float p = gg[y + n] * gg[x + n];
            G[0][0] += p;
            G[1][1] += p * x * x;
            G[3][3] += p * x * x * x * x;
            G[5][5] += p * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    double A[6][12];
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 12; j++) A[i][j] = j < 6 ? G[i][j] : (j - 6 == i ? 1.0 : 0.0);
    for (int c = 0; c < 6; c++) {
        int p = c;
        for (int r = c + 1; r < 6; r++)
            if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
        if (p != c)
            for (int j = 0; j < 12; j++) { double t = A[c][j]; A[c][j] = A[p][j]; A[p][j] = t; }
        double d = 1.0 / A[c][c];
        for (int j = 0; j < 12; j++) A[c][j] *= d;
        for (int r = 0; r < 6; r++)
            if (r != c) {
                double f = A[r][c];
                if (f != 0)
                    for (int j = 0; j < 12; j++) A[r][j] -= f * A[c][j];
            }
    }
    out->ig11 = A[1][7];
    out->ig03 = A[0][9];
    out->ig33 = A[3][9];
    out->ig55 = A[5][11];
}

static void polyexp_prepare(PolyConsts *pc) {  // FarnebackPrepareGaussian(n = 5, sigma = 1.2)
    FbgPoly q;
    farneback_prepare_gaussian(FFL_POLY_N, 1.2, &q);
    for (int x = 0; x <= FFL_POLY_N; x++) {
        pc->g[x] = q.g[x];
        pc->xg[x] = q.xg[x];
        pc->xxg[x] = q.xxg[x];
        pc->gd[x] = (double)pc->g[x];
        pc->xxgd[x] = (double)pc->xxg[x];
    }
    pc->ig11 = q.ig11;
    pc->ig03 = q.ig03;
    pc->ig33 = q.ig33;
    pc->ig55 = q.ig55;
}

// The level rule of FarnebackOpticalFlowImpl::calc for (pyr_scale, requested levels) on a w x h frame: how many coarser
// levels there are (A.1: none below min_size = 32) and, per level, its size and the Gaussian it is smoothed with.
struct LevelRule {
    int levels;
    int lw[FBG_MAX_SCALES], lh[FBG_MAX_SCALES], ksize[FBG_MAX_SCALES];
    double sigma[FBG_MAX_SCALES];
};
static void level_rule(int w, int h, double pyr_scale, int levels, LevelRule *r) {
    int k;
    double scale = 1.0;
    for (k = 0; k < levels; k++) {
        scale *= pyr_scale;
        if (w * scale < 32 || h * scale < 32) break;
    }
    r->levels = k;
    for (k = 0; k <= r->levels; k++) {
        double sc = 1.0;
        for (int i = 0; i < k; i++) sc *= pyr_scale;
        r->sigma[k] = (1.0 / sc - 1.0) * 0.5;
        const int sm = cv_round(r->sigma[k] * 5) | 1;
        r->ksize[k] = sm < 3 ? 3 : sm;
        r->lw[k] = cv_round(w * sc);
        r->lh[k] = cv_round(h * sc);
    }
}

static void level_geometry(int w, int h, Geometry *geo) {  // the reference's parameters: pyr_scale 0.5, levels 3
    LevelRule r;
    level_rule(w, h, 0.5, 3, &r);
    geo->levels = r.levels;
    for (int k = 0; k <= r.levels; k++) {
        LevelGeom &g = geo->lv[k];
        g.lw = r.lw[k];
        g.lh = r.lh[k];
        g.ksize = r.ksize[k];
        g.sigma = r.sigma[k];
        memset(&g.gk, 0, sizeof(g.gk));
        g.gk.ksize = g.ksize;
        gaussian_kernel(g.ksize, g.sigma, g.gk.k);
    }
}

// The sizes every sizing call and ffl_create accept.  Upper bound: the kernels index a pair's 5 M planes (20 bytes per
// pixel) and a batch's pixels with 32-bit offsets -> 20 * w * h must stay below 2^32 (about 214 Mpx; 5760x2880 is 16.6 Mpx)
#define FFL_FRAME_SIZE_RULE "unsupported frame size %dx%d (16x16 .. 20*w*h < 2^32)"
static bool frame_size_ok(int w, int h) { return !(w < 16 || h < 16 || (long)w * h * 20 >= (1L << 32)); }
static bool counts_ok(int n_frame_slots, int n_flow_slots, int max_batch) {
    return n_frame_slots >= 2 && n_flow_slots >= 1 && max_batch >= 1 && max_batch <= FFL_MAX_BATCH;
}

static Layout context_layout(int w, int h, int n_frame_slots, int n_flow_slots, int max_batch) {
    Geometry geo;
    level_geometry(w, h, &geo);
    const size_t N = (size_t)w * h, maxU = 2 * (size_t)max_batch;
    Layout l = {};
    for (int k = 0; k <= geo.levels; k++) {
        const size_t plane = (size_t)geo.lv[k].lw * geo.lv[k].lh;
        l.i_off[k] = l.I; l.t_off[k] = l.T; l.r_off[k] = l.R;
        l.I += plane * maxU;
        l.T += ffl_pyr_tmp_floats(w, h, geo.lv[k].lw) * maxU;
        l.R += 5 * plane * maxU;
    }
    l.M = 5 * N * max_batch; l.flow = 2 * N * max_batch;
    l.p1 = (size_t)ffl_pass1_blocks(w, h) * max_batch; l.tab = FFL_EV_RING;
    l.gray = (size_t)n_frame_slots * N; l.bgr = (size_t)n_frame_slots * N * 3;
    l.slots = 2 * N * n_flow_slots; l.res = n_flow_slots;
    return l;
}

// ---- profiling helpers ---------------------------------------------------------------------------
// Timing events come from a per-context pool (creating two events per launch cost more host time than the
// launch itself).  Where the caller knows that timed launches of a class are queued back to back (the three
// k_blur_solve iterations of a level) a launch starts at its predecessor's end event instead of recording one.
static hipEvent_t prof_event(ffl_ctx *c) {
    Event e;  // leaves the pool until prof_collect hands it back
    if (c->prof_pool.empty()) {
        hipEventCreate(e.put());
    } else {
        e = std::move(c->prof_pool.back());
        c->prof_pool.pop_back();
    }
    return e.release();
}

struct ProfScope {
    ffl_ctx *c;
    int cls;
    hipEvent_t a = nullptr, b = nullptr;
    bool on, shared = false;
    // chain: the caller guarantees that nothing was queued on `st` since the previous timed launch of this class
    ProfScope(ffl_ctx *c_, int cls_, hipStream_t st, bool chain = false)
        : c(c_), cls(cls_), on((c_->prof_mask >> cls_) & 1u) {
        if (on) {
            stream = st;
            if (chain && c->prof_last_end && c->prof_last_cls == cls && c->prof_last_stream == st) {
                a = c->prof_last_end;  // nothing was queued on `st` since that launch ended
                shared = true;
            } else {
                a = prof_event(c);
                hipEventRecord(a, st);
            }
        } else {
            c->prof_last_end = nullptr;  // an untimed launch breaks the chain
        }
    }
    ~ProfScope() {
        if (on) {
            b = prof_event(c);
            hipEventRecord(b, stream);
            c->prof_recs.push_back({cls, a, b, shared});
            c->prof_last_end = b;
            c->prof_last_cls = cls;
            c->prof_last_stream = stream;
        }
    }
    hipStream_t stream = nullptr;
};

static void prof_collect(ffl_ctx *c) {
    for (auto &r : c->prof_recs) {
        float ms = 0;
        hipEventSynchronize(r.b);
        hipEventElapsedTime(&ms, r.a, r.b);
        c->prof_launches[r.cls]++;
        c->prof_ms[r.cls] += ms;
    }
    for (auto &r : c->prof_recs) {
        if (!r.shared_start) c->prof_pool.emplace_back(r.a);
        c->prof_pool.emplace_back(r.b);
    }
    c->prof_recs.clear();
    c->prof_last_end = nullptr;
}

// hipStreamWaitEvent for every DISTINCT event of a list: the 257 frames of a 256-pair batch share one or two upload events and
// its 256 recycled flow slots one or two batch events, and a wait call costs ~0.5 us each (0.25 ms per 256-pair batch).
struct WaitOnce {
    hipStream_t st;
    hipEvent_t seen[8];
    int n = 0;
    explicit WaitOnce(hipStream_t s) : st(s) {}
    hipError_t operator()(hipEvent_t e) {
        if (!e) return hipSuccess;
        for (int k = 0; k < n; k++)
            if (seen[k] == e) return hipSuccess;
        if (n < 8) seen[n++] = e;
        return hipStreamWaitEvent(st, e, 0);
    }
};

// The host wait of every entry point (the lock rule at ffl_ctx::mu): every non-null event of evs[0..n) is waited for
// WITHOUT the context lock, which is held again on return.  A handle may be re-recorded meanwhile by another thread, but a
// ring entry is only ever re-recorded for LATER work of its stream, so the wait stays sufficient.
static int wait_unlocked(ffl_ctx *c, CtxLock &lk, const hipEvent_t *evs, int n) {
    HIPCHK(c, hipSetDevice(c->device));
    lk.unlock();
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; i++)
        if (evs[i]) e = hipEventSynchronize(evs[i]);
    lk.lock();
    if (e != hipSuccess) return set_err(c, FFL_ERR_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(e));
    return FFL_OK;
}

// Stream `copy` waits for the batches (of every lane) and the residual call (stream `post`) that may still read frame slot fs,
// before a transfer overwrites it.
static int wait_frame_free(ffl_ctx *c, WaitOnce &wait_copy, int fs) {
    const size_t nl = c->frame_readers();
    for (size_t l = 0; l < nl; l++) HIPCHK(c, wait_copy(c->ev_last_use[(size_t)fs * nl + l].get()));
    return FFL_OK;
}

// The end of an upload call: ONE event on stream `copy` for frame slots first..first+n-1.  A transfer into a slot may still
// be in flight out of the slot's staging area; the new event is later on the same stream, so waiting on it covers that too.
static int publish_frames(ffl_ctx *c, int first, int n) {
    EvRef ev;
    HIPCHK(c, c->up_ring.record(c->s_copy, &ev));  // the entry is 32 upload calls old: over long ago
    for (int i = first; i < first + n; i++) {
        c->ev_uploaded[i] = ev;
        c->frame_valid[i] = 1;
    }
    return FFL_OK;
}

// Flow slots written by the operation `done` (a batch or ffl_upload_flow): reuse of a slot waits for it, and `ready`
// says whether the slot holds a result once it has completed.
static void publish_slots(ffl_ctx *c, int n, const int *slots, EvRef done, bool ready) {
    for (int i = 0; i < n; i++) {
        c->ev_slot_done[slots[i]] = done;
        c->slot_state[slots[i]] = ready;
    }
}

// The frame slots first..first+n-1 of an upload call and its table of n frames; `frames` (host pointers) when every
// entry must be non-NULL too.  fn prefixes the message.
static int check_frame_run(ffl_ctx *c, const char *fn, int first, int n, const void *table, const uint8_t *const *frames = nullptr) {
    if (!table || n < 1 || first < 0 || first + n > c->n_fslots)
        return set_err(c, FFL_ERR_INVALID, "%s: bad frame slot range %d..%d", fn, first, first + n - 1);
    for (int i = 0; frames && i < n; i++)
        if (!frames[i]) return set_err(c, FFL_ERR_INVALID, "%s: frame %d is NULL", fn, i);
    return FFL_OK;
}

// The flow slots a call names: each in range, holding what the call reads (`holds`: "flow", "result", or nullptr when the
// call only writes them), and -- when `repeat_rule` words the refusal -- none named twice (O(n) through the context's
// scratch marks, which are cleared again on every path).  fn prefixes the message.
static bool flow_slot_ok(const ffl_ctx *c, int slot) { return slot >= 0 && slot < c->n_slots; }
static int check_flow_slots(ffl_ctx *c, const char *fn, int n, const int *slots, const char *holds, const char *repeat_rule) {
    for (int i = 0; i < n; i++) {
        if (!flow_slot_ok(c, slots[i])) return set_err(c, FFL_ERR_INVALID, "%s: flow slot %d out of range", fn, slots[i]);
        if (holds && !c->slot_state[slots[i]]) return set_err(c, FFL_ERR_STATE, "%s: flow slot %d holds no %s", fn, slots[i], holds);
    }
    if (!repeat_rule) return FFL_OK;
    int dup = -1;
    for (int i = 0; i < n; i++) {
        if (c->slot_mark[slots[i]] && dup < 0) dup = slots[i];
        c->slot_mark[slots[i]] = 1;
    }
    for (int i = 0; i < n; i++) c->slot_mark[slots[i]] = 0;
    if (dup >= 0) return set_err(c, FFL_ERR_INVALID, "%s: flow slot %d %s", fn, dup, repeat_rule);
    return FFL_OK;
}

// Flow slots read or written by an operation queued on stream `post`: ONE event of post_ring becomes their last use
// (*done), so that a batch recycling one of them runs behind it.  The slots hold a result once it has completed.
static int publish_post(ffl_ctx *c, int n, const int *slots, EvRef *done) {
    HIPCHK(c, c->post_ring.record(c->s_post, done));
    publish_slots(c, n, slots, *done, true);
    return FFL_OK;
}

// The opening of the calls that take a list of at most max_batch flow slots and hand it to a kernel as an ExportTab
// (ffl_import_flows, ffl_pass1_weighted, ffl_cell_stats): 1 <= n <= max_batch, the list given, every slot in range and holding
// `holds` (see check_flow_slots), none named twice; then *t is the list.  `what` names the items in the message.
static int open_slot_list(ffl_ctx *c, const char *fn, const char *what, int n, const int *slots, const char *holds,
                          ExportTab *t) {
    if (n < 1 || n > c->max_batch)
        return set_err(c, FFL_ERR_INVALID, "%s: n = %d %s outside 1..%d (the context's max_batch)", fn, n, what, c->max_batch);
    if (!slots) return set_err(c, FFL_ERR_INVALID, "%s: NULL flow_slots", fn);
    if (int rc = check_flow_slots(c, fn, n, slots, holds, "repeated in one call")) return rc;
    for (int i = 0; i < n; i++) t->slot[i] = slots[i];
    return FFL_OK;
}

// The geometry rules of every front-end path: the stream metadata (rules Y6 / Y7 of DESIGN.md appendix Y), source, resize
// and output sizes within 32768, the crop window inside the resized frame.  The only place that turns the stored size
// sw x sh into the upright one and that into the resize mode, the scales and the map of rule Y6: resize, crop, clamps and
// scales are all in upright terms.  cls: what the source is (full range is a property of 4:2:0; a gray frame is copied as
// it is, so its upright size is the output's).  Fills everything of *p but kind and rgb (the caller sets them) and the
// 16-bit reduction (front_depth()); fn prefixes the message.  si NULL: no metadata.
enum { FRONT_BGR = 0, FRONT_YUV = 1, FRONT_GRAY = 2 };
// The part of it that describes the source alone, which the map-driven calls (ffl_upload_frames_remap) share: the metadata
// rules, the upright size (p->sw x p->sh), the map of rule Y6 and rule Y7's flag.
static int front_source(ffl_ctx *c, const char *fn, int cls, int sw, int sh, const ffl_source_info *si, FrontParams *p) {
    static const ffl_source_info none = {0, 0, 0};
    if (!si) si = &none;
    if (si->rotate != 0 && si->rotate != 90 && si->rotate != 180 && si->rotate != 270)
        return set_err(c, FFL_ERR_INVALID, "%s: rotate %d is not one of 0, 90, 180, 270 (the clockwise rotation that makes the "
                                           "stored frame upright)", fn, si->rotate);
    if ((unsigned)si->mirror > 1u)
        return set_err(c, FFL_ERR_INVALID, "%s: mirror %d is neither 0 nor 1", fn, si->mirror);
    if ((unsigned)si->full_range > 1u)
        return set_err(c, FFL_ERR_INVALID, "%s: full_range %d is neither 0 nor 1", fn, si->full_range);
    if (si->full_range && cls != FRONT_YUV)
        return set_err(c, FFL_ERR_INVALID, "%s: full_range describes 4:2:0 sources (I420, NV12): BGR, RGB and gray frames carry "
                                           "no colour range", fn);
    const int rot = si->rotate / 90;
    const int uw = rot & 1 ? sh : sw, uh = rot & 1 ? sw : sh;  // the upright size
    p->sw = uw; p->sh = uh;
    p->shift16 = p->round16 = 0;  // front_depth() sets them for 16-bit sources
    // rule Y6: the mirror first (ux <- uw - 1 - ux = mx * ux + m0), then the row of the table for the rotation
    const int mx = si->mirror ? -1 : 1, m0 = si->mirror ? uw - 1 : 0;
    p->ax = p->bx = p->cx0 = p->ay = p->by = p->cy0 = 0;
    switch (rot) {
    case 0: p->ax = mx; p->cx0 = m0; p->by = 1; break;                                          // S[uy][ux]
    case 1: p->bx = 1; p->ay = -mx; p->cy0 = sh - 1 - m0; break;                                // S[sh - 1 - ux][uy]
    case 2: p->ax = -mx; p->cx0 = sw - 1 - m0; p->by = -1; p->cy0 = sh - 1; break;              // S[sh - 1 - uy][sw - 1 - ux]
    default: p->bx = -1; p->cx0 = sw - 1; p->ay = mx; p->cy0 = m0; break;                       // S[ux][sw - 1 - uy]
    }
    p->full = si->full_range;
    p->src = rot != 0 || si->mirror || si->full_range;
    return FFL_OK;
}

static int front_geometry(ffl_ctx *c, const char *fn, int cls, int sw, int sh, const ffl_source_info *si, int rw, int rh, int cx,
                          int cy, int ow, int oh, FrontParams *p) {
    if (int rc = front_source(c, fn, cls, sw, sh, si, p)) return rc;
    const int uw = p->sw, uh = p->sh;  // the upright size
    if (cls == FRONT_GRAY && (rw != uw || rh != uh))
        return set_err(c, FFL_ERR_INVALID, "%s: gray frames are copied as they are: a resize (%dx%d -> %dx%d) is refused", fn, uw, uh,
                       rw, rh);
    if (cls == FRONT_GRAY && (uw != ow || uh != oh))
        return set_err(c, FFL_ERR_INVALID, "%s: a gray frame must be the context size %dx%d, got %dx%d", fn, ow, oh, uw, uh);
    if (sw < 1 || sh < 1 || sw > 32768 || sh > 32768 || rw < 1 || rh < 1 || rw > 32768 || rh > 32768 || ow < 1 || oh < 1)
        return set_err(c, FFL_ERR_INVALID, "%s: unsupported source %dx%d / resize %dx%d / output %dx%d", fn, sw, sh, rw, rh, ow, oh);
    if (cx < 0 || cy < 0 || cx + ow > rw || cy + oh > rh)
        return set_err(c, FFL_ERR_INVALID, "%s: crop window (%d, %d) + %dx%d does not fit the %dx%d resized frame", fn, cx, cy, ow,
                       oh, rw, rh);
    p->cx = cx; p->cy = cy; p->ow = ow; p->oh = oh;
    p->scale_x = 1. / ((double)rw / uw);
    p->scale_y = 1. / ((double)rh / uh);
    p->mode = (rw == uw && rh == uh) ? FFL_FRONT_IDENTITY : (uw == 2 * rw && uh == 2 * rh) ? FFL_FRONT_AREA2 : FFL_FRONT_GENERIC;
    return FFL_OK;
}

// The frame-by-frame loop of ffl_upload_frames_raw and ffl_upload_frames_yuv, called with up_mu and the context lock held.
// Frame i takes the next buffer pair of the raw-frame ring; direct(i) says whether its fbytes go to the device straight
// out of caller memory (send_direct(i, d)) or are first staged into the pinned buffer (stage(i, h, copy_threads), run
// WITHOUT the context lock) and sent as one transfer; one k_frontend launch (rp: k_frontend_remap with that map) then reads
// desc(d) into frame slot first + i.
template <class Direct, class Stage, class SendDirect, class Desc>
static int upload_staged(ffl_ctx *c, CtxLock &lk, int first, int n, size_t fbytes, const FrontParams &fp, Direct direct,
                         Stage stage, SendDirect send_direct, Desc desc, const RemapParams *rp = nullptr) {
    for (int i = 0; i < n; i++) {
        const int fs = first + i;
        auto &rb = c->raw[c->raw_next++ % FFL_RAW_RING];
        if (rb.busy) {  // its previous frame has left both buffers
            if (int rc = wait_unlocked(c, lk, &rb.ev.h, 1)) return rc;
        }
        if (rb.cap < fbytes) {
            rb.cap = 0;  // the old pair goes first: the two sizes need not fit side by side
            rb.d.reset();
            rb.h.reset();
            DevBuf<uint8_t> d; PinBuf<uint8_t> h;  // into locals: a failed second allocation drops the first too, cap stays 0
            HIPCHK_ALLOC(c, hipMalloc, d, fbytes);
            HIPCHK_ALLOC(c, hipHostMalloc, h, fbytes, hipHostMallocDefault);
            rb.d = std::move(d);
            rb.h = std::move(h);
            rb.cap = fbytes;
        }
        const bool dir = direct(i);
        if (!dir) {
            const int copy_threads = c->opt.copy_threads;
            lk.unlock();  // the staging copy runs without the context lock (up_mu protects the ring and the pool)
            stage(i, rb.h, copy_threads);
            lk.lock();
        }
        // looked up under the lock, after the staging copy: a batch queued meanwhile is ordered ahead of the transfer
        WaitOnce wait_copy(c->s_copy);
        if (int rc = wait_frame_free(c, wait_copy, fs)) return rc;
        if (dir) {
            if (int rc = send_direct(i, rb.d)) return rc;
        } else {
            HIPCHK(c, hipMemcpyAsync(rb.d, rb.h, fbytes, hipMemcpyHostToDevice, c->s_copy));
        }
        {
            ProfScope ps(c, FFL_K_FRONTEND, c->s_copy);
            if (rp) ffl_launch_frontend_remap(desc(rb.d), c->d_gray + (size_t)fs * c->N, fp, *rp, c->s_copy);  // the map instead of
            else ffl_launch_frontend(desc(rb.d), c->d_gray + (size_t)fs * c->N, fp, c->s_copy);              // resize + crop
        }
        HIPCHK(c, hipEventRecord(rb.ev, c->s_copy));
        rb.busy = true;
    }
    return publish_frames(c, first, n);
}

// ---- API -----------------------------------------------------------------------------------------
extern "C" {

int ffl_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *ffl_last_error(const ffl_ctx *ctx) {
    if (!ctx) return g_create_error.c_str();
    // copied under the lock into a per-thread buffer: another thread's failing call may replace ctx->err while the caller
    // still reads the text (valid until this thread's next ffl_last_error call)
    static thread_local std::string copy;
    CtxLock lk(ctx->mu);
    copy = ctx->err;
    return copy.c_str();
}

const char *ffl_kernel_name(int k) {
    static const char *names[FFL_K_COUNT] = {"k_gray",  "k_pyr_level", "k_polyexp", "k_frontend",
                                             "k_update_matrices", "k_blur_solve", "k_pass1", "k_radial"};
    return (k >= 0 && k < FFL_K_COUNT) ? names[k] : "?";
}

void ffl_destroy(ffl_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    for (auto &L : c->lanes)
        if (L.st) hipStreamSynchronize(L.st);
    if (c->s_post) hipStreamSynchronize(c->s_post);
    if (c->s_copy) hipStreamSynchronize(c->s_copy);
    prof_collect(c);
    c->pool.shutdown();
    delete c;  // every stream has been drained: the handles release in no particular order
}

// The runtime resources of a context whose geometry, options and layout are set.  A failure is reported as the creation
// error (the null context of HIPCHK): the half-built context does not outlive the call.
static int create_resources(ffl_ctx *c) {
    const int width = c->w, height = c->h, n_frame_slots = c->n_fslots, n_flow_slots = c->n_slots;
    const int num_lanes = c->opt.lanes;  // fixed for the life of the context
    const Geometry &geo = c->geo;
    const Layout &lay = c->lay;
    HIPCHK(nullptr, hipSetDevice(c->device));
    // uploads and pass 2 are short and latency-critical (the host waits on pass 2): high priority, so
    // that they get their own hardware queues and are scheduled between a lane's queued kernels
    int prio_least = 0, prio_greatest = 0;
    HIPCHK(nullptr, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    HIPCHK(nullptr, hipStreamCreateWithPriority(c->s_copy.put(), hipStreamNonBlocking, prio_greatest));
    HIPCHK(nullptr, hipStreamCreateWithPriority(c->s_post.put(), hipStreamNonBlocking, prio_greatest));
    HIPCHK_ALLOC(nullptr, hipMalloc, c->d_gray, lay.gray + 16);  // +16: the pyramid kernels fetch taps as aligned words
    HIPCHK_ALLOC(nullptr, hipMalloc, c->d_bgr, lay.bgr);
    HIPCHK_ALLOC(nullptr, hipHostMalloc, c->h_stage_gray, lay.gray, hipHostMallocDefault);
    HIPCHK_ALLOC(nullptr, hipHostMalloc, c->h_stage_bgr, lay.bgr, hipHostMallocDefault);
    c->p1_blocks = ffl_pass1_blocks(width, height);
    if (!ffl_blur_slots(&c->blur_slots)) return set_err(nullptr, FFL_ERR_HIP, "ffl_create: the occupancy of k_blur_solve could not be queried");
    c->lanes.resize(num_lanes);
    for (auto &L : c->lanes) {
        HIPCHK(nullptr, hipStreamCreateWithFlags(L.st.put(), hipStreamNonBlocking));
        HIPCHK(nullptr, L.ring.create(FFL_EV_RING));
        HIPCHK_ALLOC(nullptr, hipMalloc, L.d_I, lay.I);
        HIPCHK_ALLOC(nullptr, hipMalloc, L.d_T, lay.T);
        HIPCHK_ALLOC(nullptr, hipMalloc, L.d_R, lay.R);
        for (auto &M : L.d_M) HIPCHK_ALLOC(nullptr, hipMalloc, M, lay.M);
        HIPCHK_ALLOC(nullptr, hipMalloc, L.d_flowA, lay.flow);
        HIPCHK_ALLOC(nullptr, hipMalloc, L.d_flowB, lay.flow);
        HIPCHK_ALLOC(nullptr, hipMalloc, L.d_pkey, lay.p1);
        HIPCHK_ALLOC(nullptr, hipMalloc, L.d_psum, lay.p1);
        HIPCHK_ALLOC(nullptr, hipMalloc, L.d_tab, 1);
        HIPCHK_ALLOC(nullptr, hipHostMalloc, L.h_tab, lay.tab, hipHostMallocDefault);
        for (int k = geo.levels; k >= 0; k--, L.n_jobs++) {
            const LevelGeom &g = geo.lv[k];
            const size_t plane = (size_t)g.lw * g.lh;
            PyrJob &P = L.pyr[L.n_jobs];
            P.w = width; P.h = height; P.lw = g.lw; P.lh = g.lh;
            P.sx = (double)width / g.lw; P.sy = (double)height / g.lh;
            P.gk = g.gk;
            P.tmp = L.d_T + lay.t_off[k]; P.tmp_stride = ffl_pyr_tmp_floats(width, height, g.lw);
            P.I = L.d_I + lay.i_off[k]; P.I_stride = plane;
            PolyJob &Q = L.poly[L.n_jobs];
            Q.I = P.I; Q.I_stride = plane;
            Q.R = L.d_R + lay.r_off[k]; Q.R_stride = 5 * plane; Q.plane = plane;
            Q.w = g.lw; Q.h = g.lh;
        }
    }
    HIPCHK_ALLOC(nullptr, hipMalloc, c->d_flow, lay.slots);
    HIPCHK_ALLOC(nullptr, hipHostMalloc, c->h_res, lay.res, hipHostMallocMapped);
    HIPCHK(nullptr, hipHostGetDevicePointer((void **)&c->d_res, c->h_res, 0));
    HIPCHK_ALLOC(nullptr, hipMalloc, c->d_rpsum, (size_t)c->p1_blocks * FFL_MAXB);
    {
        std::vector<double> wy(2 * (size_t)height);
        for (int y = 0; y < height; y++) {
            wy[y] = (double)(height - y) / (double)height;
            wy[height + y] = (double)y / (double)height;
        }
        HIPCHK_ALLOC(nullptr, hipMalloc, c->d_wytab, wy.size());
        HIPCHK(nullptr, hipMemcpy(c->d_wytab, wy.data(), sizeof(double) * wy.size(), hipMemcpyHostToDevice));
    }
    HIPCHK_ALLOC(nullptr, hipMalloc, c->d_wtab, FFL_MAXB);
    HIPCHK_ALLOC(nullptr, hipHostMalloc, c->h_wtab, FFL_MAXB, hipHostMallocDefault);
    HIPCHK_ALLOC(nullptr, hipMalloc, c->d_ptab, 1);
    HIPCHK_ALLOC(nullptr, hipHostMalloc, c->h_ptab, 1, hipHostMallocDefault);
    HIPCHK_ALLOC(nullptr, hipMalloc, c->d_pskey, lay.p1);
    HIPCHK_ALLOC(nullptr, hipHostMalloc, c->h_radial, FFL_MAXB, hipHostMallocMapped);
    HIPCHK(nullptr, hipHostGetDevicePointer((void **)&c->d_radial, c->h_radial, 0));
    c->ev_uploaded.assign(n_frame_slots, EvRef{});
    c->ev_last_use.assign((size_t)n_frame_slots * c->frame_readers(), EvRef{});  // references into the lanes' rings and post_ring
    c->frame_valid.assign(n_frame_slots, 0);
    c->u_of_fslot.assign(n_frame_slots, -1);
    c->slot_mark.assign(n_flow_slots, 0);
    HIPCHK(nullptr, c->up_ring.create(2 * FFL_EV_RING));
    HIPCHK(nullptr, c->post_ring.create(FFL_EV_RING));
    HIPCHK(nullptr, hipEventCreateWithFlags(c->ev_caller.put(), hipEventDisableTiming));
    for (auto &rb : c->raw) HIPCHK(nullptr, hipEventCreateWithFlags(rb.ev.put(), hipEventDisableTiming));
    c->ev_slot_done.assign(n_flow_slots, EvRef{});                        // set when a slot is queued
    c->slot_state.assign(n_flow_slots, 0);
    return FFL_OK;
}

int ffl_create(int device, int width, int height, int n_frame_slots, int n_flow_slots, int max_batch,
               ffl_ctx **out) {
    if (!out) return set_err(nullptr, FFL_ERR_INVALID, "ffl_create: out is NULL");
    *out = nullptr;
    if (!frame_size_ok(width, height)) return set_err(nullptr, FFL_ERR_INVALID, "ffl_create: " FFL_FRAME_SIZE_RULE, width, height);
    if (!counts_ok(n_frame_slots, n_flow_slots, max_batch))
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_create: bad slot/batch counts (%d, %d, %d)", n_frame_slots,
                       n_flow_slots, max_batch);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return set_err(nullptr, FFL_ERR_NO_DEVICE, "ffl_create: no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev)
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_create: device %d out of range (0..%d)", device, ndev - 1);
    // the level kernels serve what the reference's level rule yields for every accepted size; said here, where the
    // geometry is fixed, should that rule ever change
    Geometry geo;
    level_geometry(width, height, &geo);
    if (geo.levels + 1 > FFL_MAX_JOBS)
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_create: %d pyramid levels at %dx%d, the level tables hold %d", geo.levels + 1,
                       width, height, FFL_MAX_JOBS);
    for (int k = 0; k <= geo.levels; k++)
        if (!ffl_pyr_level_ok(width, height, geo.lv[k].lw, geo.lv[k].lh, geo.lv[k].ksize))
            return set_err(nullptr, FFL_ERR_INVALID, "ffl_create: no pyramid kernel for level %d of %dx%d (%d columns, %d-tap blur)",
                           k, width, height, geo.lv[k].lw, geo.lv[k].ksize);
    ffl_ctx *c = new ffl_ctx();
    c->device = device;
    c->w = width;
    c->h = height;
    c->N = (size_t)width * height;
    c->n_fslots = n_frame_slots;
    c->n_slots = n_flow_slots;
    c->max_batch = max_batch;
    {
        std::lock_guard<std::mutex> g(g_opt_mu);
        c->opt = g_opts;
    }
    c->geo = geo;
    c->lay = context_layout(width, height, n_frame_slots, n_flow_slots, max_batch);
    polyexp_prepare(&c->pc);
    if (const int rc = create_resources(c)) {
        ffl_destroy(c);           // works on a context that is built in part: null handles are no-ops
        (void)hipGetLastError();  // the failure is reported HERE: do not leave it to poison a later call's check
        return rc;
    }
    *out = c;
    return FFL_OK;
}

int ffl_device_mem_info(int device, size_t *free_bytes, size_t *total_bytes) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return set_err(nullptr, FFL_ERR_NO_DEVICE, "ffl_device_mem_info: no HIP device available");
    if (device < 0 || device >= ndev) return set_err(nullptr, FFL_ERR_INVALID, "ffl_device_mem_info: device %d out of range", device);
    size_t f = 0, t = 0;
    if (hipSetDevice(device) != hipSuccess || hipMemGetInfo(&f, &t) != hipSuccess)
        return set_err(nullptr, FFL_ERR_HIP, "ffl_device_mem_info: hipMemGetInfo failed");
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return FFL_OK;
}

static int default_lanes() {
    std::lock_guard<std::mutex> g(g_opt_mu);
    return g_opts.lanes;
}

// What ffl_create(width, height, n_frame_slots, n_flow_slots, max_batch) allocates with the current "lanes" option: the
// bytes of the layout ffl_create allocates from, plus 1 MiB each for the small tables it does not list.  No device needed.
int ffl_estimate_bytes(int width, int height, int n_frame_slots, int n_flow_slots, int max_batch, size_t *device_bytes,
                       size_t *pinned_bytes) {
    if (!frame_size_ok(width, height) || !counts_ok(n_frame_slots, n_flow_slots, max_batch))
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_estimate_bytes: bad geometry / slot counts");
    const Layout l = context_layout(width, height, n_frame_slots, n_flow_slots, max_batch);
    const size_t lanes = default_lanes(), small = (size_t)1 << 20;
    const size_t lane = sizeof(float) * (l.I + l.T + l.R + 2 * l.M + 2 * l.flow) + (sizeof(unsigned long long) + sizeof(double)) * l.p1;
    if (device_bytes) *device_bytes = lanes * lane + l.gray + l.bgr + sizeof(float) * l.slots + small;
    if (pinned_bytes) *pinned_bytes = l.gray + l.bgr + sizeof(Pass1Result) * l.res + lanes * sizeof(BatchTab) * l.tab + small;
    return FFL_OK;
}

int ffl_num_levels(const ffl_ctx *c) { return c ? c->geo.levels : -1; }

int ffl_level_size(const ffl_ctx *c, int level, int *out_wh) {
    if (!c || !out_wh || level < 0 || level > c->geo.levels) return FFL_ERR_INVALID;
    out_wh[0] = c->geo.lv[level].lw;
    out_wh[1] = c->geo.lv[level].lh;
    return FFL_OK;
}

static bool in_host_buf(const ffl_ctx *c, const uint8_t *p, size_t bytes) {
    for (auto &hb : c->host_bufs)
        if (p >= hb.first.h && p + bytes <= hb.first.h + hb.second) return true;
    return false;
}

int ffl_host_alloc(ffl_ctx *c, size_t bytes, void **out) {
    if (!c) return FFL_ERR_INVALID;
    CtxLock lk(c->mu);
    if (!out || bytes == 0) return set_err(c, FFL_ERR_INVALID, "ffl_host_alloc: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    PinBuf<uint8_t> p;
    HIPCHK_ALLOC(c, hipHostMalloc, p, bytes, hipHostMallocDefault);
    *out = p.h;
    c->host_bufs.emplace_back(std::move(p), bytes);
    return FFL_OK;
}

int ffl_host_free(ffl_ctx *c, void *ptr) {
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> ul(c->up_mu);  // no upload out of the buffer starts while it is being freed
    CtxLock lk(c->mu);
    bool mine = false;
    for (auto &hb : c->host_bufs) mine |= hb.first.h == ptr;
    if (!mine) return set_err(c, FFL_ERR_INVALID, "ffl_host_free: not a buffer of this context");
    HIPCHK(c, hipSetDevice(c->device));
    lk.unlock();
    hipError_t e = hipStreamSynchronize(c->s_copy);  // no transfer may still be reading it (waited for without the lock)
    lk.lock();
    HIPCHK(c, e);
    for (size_t i = 0; i < c->host_bufs.size(); i++)
        if (c->host_bufs[i].first.h == ptr) {
            const hipError_t fe = c->host_bufs[i].first.reset();
            c->host_bufs.erase(c->host_bufs.begin() + i);  // whatever the runtime answered: the handle is gone
            HIPCHK_AS(c, "hipHostFree", fe);
            return FFL_OK;
        }
    return set_err(c, FFL_ERR_INVALID, "ffl_host_free: not a buffer of this context");
}

// n frames into the consecutive frame slots first..first+n-1: host copies into pinned staging, then ONE
// H2D transfer (+ one BGR->gray launch) and ONE event for the whole run -- at 256x256 the per-frame
// runtime calls of a frame-at-a-time upload cost more than the copy itself.
int ffl_upload_frames(ffl_ctx *c, int first, int n, const uint8_t *const *frames, int width, int height, int channels,
                      ptrdiff_t stride_bytes) {
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> ul(c->up_mu);
    CtxLock lk(c->mu);
    if (int rc = check_frame_run(c, "ffl_upload_frames", first, n, frames, frames)) return rc;
    if (width != c->w || height != c->h)
        return set_err(c, FFL_ERR_INVALID, "ffl_upload_frames: frame is %dx%d, context is %dx%d", width, height, c->w, c->h);
    if (channels != 1 && channels != 3)
        return set_err(c, FFL_ERR_INVALID, "ffl_upload_frames: channels must be 1 (gray) or 3 (BGR), got %d", channels);
    if (stride_bytes < (ptrdiff_t)width * channels)
        return set_err(c, FFL_ERR_INVALID, "ffl_upload_frames: stride %td < row bytes %d", stride_bytes, width * channels);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = c->N, row = (size_t)width * channels, fbytes = N * channels;
    uint8_t *stage0 = (channels == 1 ? c->h_stage_gray : c->h_stage_bgr) + (size_t)first * fbytes;
    // frames that sit back to back in one ffl_host_alloc buffer go to the device straight out of it
    bool direct = (size_t)stride_bytes == row && in_host_buf(c, frames[0], fbytes * n);
    for (int i = 1; direct && i < n; i++) direct = frames[i] == frames[0] + (size_t)i * fbytes;
    // Staged frames go to the device in pieces of >= 8 MiB as soon as they are in pinned memory, so the transfer of
    // the first frames runs while the host still copies the later ones (one 200 MB transfer issued after a 33-frame
    // BGR run had been staged left the device waiting for it); small frames still travel as one run.
    auto send = [&](int i0, int i1) -> int {  // frames i0 .. i1-1 of the run; called with the context lock held
        // the device copies of these slots may still be read by batches queued on any lane -- looked up HERE, right before
        // the transfer is queued: the lock was dropped for the staging copies, and a batch another thread queued meanwhile
        // must be ordered ahead of the transfer that overwrites its frame
        WaitOnce wait_copy(c->s_copy);
        for (int i = i0; i < i1; i++)
            if (int rc = wait_frame_free(c, wait_copy, first + i)) return rc;
        uint8_t *gray = c->d_gray + (size_t)(first + i0) * N;
        const uint8_t *src = (direct ? frames[0] : stage0) + (size_t)i0 * fbytes;
        const int m = i1 - i0;
        if (channels == 1) {
            HIPCHK(c, hipMemcpyAsync(gray, src, N * m, hipMemcpyHostToDevice, c->s_copy));
        } else {
            uint8_t *bgr = c->d_bgr + (size_t)(first + i0) * N * 3;
            HIPCHK(c, hipMemcpyAsync(bgr, src, N * 3 * m, hipMemcpyHostToDevice, c->s_copy));
            ProfScope ps(c, FFL_K_GRAY, c->s_copy);
            // k_gray counts pixels in 32 bits: runs of frames of at most 2^30 pixels per launch
            const int per = (int)((size_t)(1u << 30) / N) > 0 ? (int)((size_t)(1u << 30) / N) : 1;
            for (int i = 0; i < m; i += per) {
                const int k = m - i < per ? m - i : per;
                ffl_launch_gray(bgr + (size_t)i * N * 3, gray + (size_t)i * N, (int)(N * k), c->s_copy);
            }
        }
        return FFL_OK;
    };
    if (direct) {
        int rc = send(0, n);
        if (rc) return rc;
    } else {
        const int copy_threads = c->opt.copy_threads;
        int i = 0;
        while (i < n) {
            // one piece: consecutive frames worth >= 8 MiB (or the rest of the run), staged together -- the piece's rows
            // are shared by the copy threads -- and sent as one transfer
            int j = i;
            for (size_t bytes = 0; j < n && bytes < ((size_t)8 << 20); j++) bytes += fbytes;
            // the previous transfers out of these slots' staging areas must have left the host buffer; the waits and the
            // staging copy run WITHOUT the context lock (up_mu keeps other uploaders out of the staging areas and the pool)
            std::vector<hipEvent_t> prev;
            for (int k = i; k < j; k++) {
                hipEvent_t e = c->ev_uploaded[first + k].get();
                if (e && (prev.empty() || prev.back() != e)) prev.push_back(e);
            }
            int rc = wait_unlocked(c, lk, prev.data(), (int)prev.size());
            if (rc) return rc;
            lk.unlock();
            c->pool.copy(stage0 + (size_t)i * fbytes, frames + i, j - i, stride_bytes, row, height, copy_threads);
            lk.lock();
            if ((rc = send(i, j))) return rc;
            i = j;
        }
    }
    return publish_frames(c, first, n);
}

// What ffl_upload_frames_raw and the 3-channel formats of ffl_upload_frames_remap share once the geometry is known: the stride
// rule and the whole stored frame's way through upload_staged.
static int send_raw(ffl_ctx *c, CtxLock &lk, const char *fn, int first, int n, const uint8_t *const *frames, int sw, int sh,
                    ptrdiff_t stride_bytes, int rgb_order, FrontParams &fp, const RemapParams *rp) {
    if (stride_bytes < (ptrdiff_t)sw * 3)
        return set_err(c, FFL_ERR_INVALID, "%s: stride %td < row bytes %d", fn, stride_bytes, sw * 3);
    HIPCHK(c, hipSetDevice(c->device));
    fp.kind = FFL_SRC_BGR;
    fp.rgb = rgb_order != 0;
    const size_t row = (size_t)sw * 3, fbytes = row * sh;
    // a tightly packed frame in ffl_host_alloc memory goes to the device straight out of it
    auto direct = [&](int i) { return (size_t)stride_bytes == row && in_host_buf(c, frames[i], fbytes); };
    auto stage = [&](int i, uint8_t *h, int threads) { c->pool.copy(h, frames + i, 1, stride_bytes, row, sh, threads); };
    auto send_direct = [&](int i, uint8_t *d) -> int {
        HIPCHK(c, hipMemcpyAsync(d, frames[i], fbytes, hipMemcpyHostToDevice, c->s_copy));
        return FFL_OK;
    };
    auto desc = [&](const uint8_t *d) {
        FrameDesc s = {};
        s.p0 = d;
        s.pitch0 = row;
        s.ps = 3;
        s.cs = 1;
        return s;
    };
    return upload_staged(c, lk, first, n, fbytes, fp, direct, stage, send_direct, desc, rp);
}

// Decoded frames -> gray frame slots through k_frontend (resize + crop + luma in one pass).  Frame by
// frame: tight copy into a pinned ring buffer, H2D, kernel -- the 3 * src_w * src_h byte transfer is the
// cost, so there is nothing to gain from batching the launches.
static int upload_raw(ffl_ctx *c, const char *fn, int first, int n, const uint8_t *const *frames, int sw, int sh,
                      ptrdiff_t stride_bytes, int rgb_order, int rw, int rh, int crop_x, int crop_y, const ffl_source_info *si) {
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> ul(c->up_mu);
    CtxLock lk(c->mu);
    if (int rc = check_frame_run(c, fn, first, n, frames, frames)) return rc;
    FrontParams fp;
    if (int rc = front_geometry(c, fn, FRONT_BGR, sw, sh, si, rw, rh, crop_x, crop_y, c->w, c->h, &fp)) return rc;
    return send_raw(c, lk, fn, first, n, frames, sw, sh, stride_bytes, rgb_order, fp, nullptr);
}

int ffl_upload_frames_raw(ffl_ctx *c, int first, int n, const uint8_t *const *frames, int sw, int sh,
                          ptrdiff_t stride_bytes, int rgb_order, int rw, int rh, int crop_x, int crop_y) {
    return upload_raw(c, "ffl_upload_frames_raw", first, n, frames, sw, sh, stride_bytes, rgb_order, rw, rh, crop_x, crop_y, nullptr);
}

int ffl_upload_frames_raw_src(ffl_ctx *c, int first, int n, const uint8_t *const *frames, int sw, int sh, ptrdiff_t stride_bytes,
                              int rgb_order, int rw, int rh, int crop_x, int crop_y, const ffl_source_info *si) {
    return upload_raw(c, "ffl_upload_frames_raw", first, n, frames, sw, sh, stride_bytes, rgb_order, rw, rh, crop_x, crop_y, si);
}

// ---- 4:2:0 YUV input ---------------------------------------------------------------
// Where the source rectangle of a YUV upload lies: the upright source rows / columns the crop window's first and last
// output row / column map to (k_frontend's arithmetic; it is monotone in the output coordinate), widened by one pixel per
// side and clamped to the upright frame (yuv_span); that span mapped through rule Y6 to the stored frame; and there
// rounded out (yuv_round) -- rows to even coordinates (chroma alignment), columns to multiples of 16 so that the rows of
// every plane start aligned in the frame (a 2-D copy out of host memory whose rows start unaligned ran at 0.3 GB/s) --
// and clamped to the frame.  The widening makes it a superset even if host and device round the coordinate arithmetic
// differently; it is not tight to the last pixel.
struct YuvWin {
    int x0, y0, w, h;  // window origin and size in the STORED frame (all even)
};

static void yuv_span(int d0, int d1, int s, double scale, int mode, int *lo, int *hi) {
    int a, b;  // first and last source coordinate the kernel loads (inclusive)
    if (mode == FFL_FRONT_IDENTITY) {
        a = d0; b = d1;
    } else if (mode == FFL_FRONT_AREA2) {
        a = 2 * d0; b = 2 * d1 + 1;
    } else {
        a = (int)floorf((float)((d0 + 0.5) * scale - 0.5));
        b = (int)floorf((float)((d1 + 0.5) * scale - 0.5)) + 1;
    }
    *lo = std::min(std::max(a - 1, 0), s - 1);
    *hi = std::min(std::max(b + 1, 0), s - 1);
}

static void yuv_round(int lo, int hi, int s, int align, int *origin, int *size) {  // [lo, hi] inclusive; s is even
    *origin = lo / align * align;
    *size = std::min((hi + 1 + align - 1) / align * align, s) - *origin;
}

// Rule Y5 (appendix Y) as the kernels apply it: s = msb ? raw >> (16 - depth) : raw; v8 = min(255, (s + (1 << (depth - 9)))
// >> (depth - 8)).  The alignment's shift folds into the rounding one exactly -- floor((floor(raw / A) + r) / B) =
// floor((raw + r * A) / (A * B)) -- so high-aligned samples of every depth are (raw + 128) >> 8.
static void front_depth(FrontParams *p, int depth, int msb) {
    p->shift16 = msb ? 8 : depth - 8;
    p->round16 = 1 << (p->shift16 - 1);
}

// the rules of a 4:2:0 single-array frame that need no geometry (es: bytes per sample; the stride is in bytes)
static int yuv_layout_rules(ffl_ctx *c, const char *fn, int sw, int sh, int layout, ptrdiff_t stride, int es, int depth) {
    const char *twice = es == 2 ? "2 * " : "";
    if (es == 2 && (depth < 9 || depth > 16))
        return set_err(c, FFL_ERR_INVALID, "%s: depth %d outside 9..16 (8-bit frames go through ffl_upload_frames_yuv)", fn, depth);
    if ((sw & 1) || (sh & 1))
        return set_err(c, FFL_ERR_INVALID, "%s: 4:2:0 needs an even width and height, source is %dx%d", fn, sw, sh);
    if (layout != FFL_YUV_I420 && layout != FFL_YUV_NV12)
        return set_err(c, FFL_ERR_INVALID, "%s: unknown layout %d (FFL_YUV_I420 0, FFL_YUV_NV12 1)", fn, layout);
    if (es == 2 && (stride & 1))
        return set_err(c, FFL_ERR_INVALID, "%s: odd stride %td: rows of 16-bit samples start 2-byte aligned", fn, stride);
    if (layout == FFL_YUV_I420 && stride != (ptrdiff_t)sw * es)
        return set_err(c, FFL_ERR_INVALID, "%s: I420 needs stride == %swidth (contiguous U and V planes), got %td for width %d",
                       fn, twice, stride, sw);
    if (layout == FFL_YUV_NV12 && stride < (ptrdiff_t)sw * es)
        return set_err(c, FFL_ERR_INVALID, "%s: NV12 needs stride >= %swidth, got %td for width %d", fn, twice, stride, sw);
    return FFL_OK;
}

// the upright span ux x uy (inclusive) of a stored sw x sh frame -> the stored rectangle that travels (rule R6 uses it too)
static void yuv_stored_window(const FrontParams &p, int sw, int sh, const int ux[2], const int uy[2], YuvWin *out) {
    // rule Y6 is affine with one unit coefficient per stored axis: two opposite corners of the span bound its image
    const int px[2] = {p.ax * ux[0] + p.bx * uy[0] + p.cx0, p.ax * ux[1] + p.bx * uy[1] + p.cx0};
    const int py[2] = {p.ay * ux[0] + p.by * uy[0] + p.cy0, p.ay * ux[1] + p.by * uy[1] + p.cy0};
    yuv_round(std::min(px[0], px[1]), std::max(px[0], px[1]), sw, 16, &out->x0, &out->w);
    yuv_round(std::min(py[0], py[1]), std::max(py[0], py[1]), sh, 2, &out->y0, &out->h);
}

// Every refusal of the YUV path (messages name the rule); fn prefixes the message.  Fills the geometry of *fp and the
// window.  es: bytes per sample (1; 2: the 16-bit frames of rule Y5, whose depth is checked here too); the stride is in
// bytes, the window in samples.
static int yuv_window(ffl_ctx *c, const char *fn, int sw, int sh, int layout, ptrdiff_t stride, int es, int depth,
                      const ffl_source_info *si, int rw, int rh, int crop_x, int crop_y, int ow, int oh, FrontParams *fp,
                      YuvWin *out) {
    if (int rc = yuv_layout_rules(c, fn, sw, sh, layout, stride, es, depth)) return rc;
    if (int rc = front_geometry(c, fn, FRONT_YUV, sw, sh, si, rw, rh, crop_x, crop_y, ow, oh, fp)) return rc;
    int ux[2], uy[2];  // the upright span, inclusive
    yuv_span(crop_x, crop_x + ow - 1, fp->sw, fp->scale_x, fp->mode, &ux[0], &ux[1]);
    yuv_span(crop_y, crop_y + oh - 1, fp->sh, fp->scale_y, fp->mode, &uy[0], &uy[1]);
    yuv_stored_window(*fp, sw, sh, ux, uy, out);
    return FFL_OK;
}

static int frontend_window(const char *fn, int src_w, int src_h, int layout, ptrdiff_t stride_bytes, int es, int depth,
                           const ffl_source_info *si, int resize_w, int resize_h, int crop_x, int crop_y, int out_w, int out_h,
                           int win[4], size_t *bytes) {
    FrontParams fp;
    YuvWin yw;
    if (int rc = yuv_window(nullptr, fn, src_w, src_h, layout, stride_bytes, es, depth, si, resize_w, resize_h, crop_x, crop_y,
                            out_w, out_h, &fp, &yw))
        return rc;
    if (win) {
        win[0] = yw.x0; win[1] = yw.y0; win[2] = yw.w; win[3] = yw.h;
    }
    if (bytes) *bytes = (size_t)yw.w * yw.h * 3 / 2 * es;
    return FFL_OK;
}

int ffl_frontend_yuv_window(int src_w, int src_h, int layout, ptrdiff_t stride_bytes, int resize_w, int resize_h, int crop_x,
                            int crop_y, int out_w, int out_h, int win[4], size_t *bytes) {
    return frontend_window("ffl_frontend_yuv_window", src_w, src_h, layout, stride_bytes, 1, 8, nullptr, resize_w, resize_h, crop_x,
                           crop_y, out_w, out_h, win, bytes);
}

int ffl_frontend_yuv_window_src(int src_w, int src_h, int layout, ptrdiff_t stride_bytes, int resize_w, int resize_h, int crop_x,
                                int crop_y, int out_w, int out_h, int win[4], size_t *bytes, const ffl_source_info *si) {
    return frontend_window("ffl_frontend_yuv_window", src_w, src_h, layout, stride_bytes, 1, 8, si, resize_w, resize_h, crop_x,
                           crop_y, out_w, out_h, win, bytes);
}

int ffl_frontend_yuv16_window(int src_w, int src_h, int layout, ptrdiff_t stride_bytes, int depth, int resize_w, int resize_h,
                              int crop_x, int crop_y, int out_w, int out_h, int win[4], size_t *bytes) {
    return frontend_window("ffl_frontend_yuv16_window", src_w, src_h, layout, stride_bytes, 2, depth, nullptr, resize_w, resize_h,
                           crop_x, crop_y, out_w, out_h, win, bytes);
}

int ffl_frontend_yuv16_window_src(int src_w, int src_h, int layout, ptrdiff_t stride_bytes, int depth, int resize_w, int resize_h,
                                  int crop_x, int crop_y, int out_w, int out_h, int win[4], size_t *bytes,
                                  const ffl_source_info *si) {
    return frontend_window("ffl_frontend_yuv16_window", src_w, src_h, layout, stride_bytes, 2, depth, si, resize_w, resize_h,
                           crop_x, crop_y, out_w, out_h, win, bytes);
}

// What ffl_upload_frames_yuv(16) and the 4:2:0 formats of ffl_upload_frames_remap share once the window is known: the
// alignment rule of 16-bit frames and the window's way through upload_staged.
static int send_yuv(ffl_ctx *c, CtxLock &lk, const char *fn, int first, int n, const uint8_t *const *frames, int sw, int sh,
                    ptrdiff_t stride_bytes, int layout, int es, int depth, int msb, FrontParams &fp, const YuvWin &yw,
                    const RemapParams *rp) {
    for (int i = 0; es == 2 && i < n; i++)
        if ((uintptr_t)frames[i] & 1) return set_err(c, FFL_ERR_INVALID, "%s: frame %d is not 2-byte aligned", fn, i);
    HIPCHK(c, hipSetDevice(c->device));
    fp.kind = es == 2 ? FFL_SRC_YUV16 : FFL_SRC_YUV;
    fp.rgb = 0;
    if (es == 2) front_depth(&fp, depth, msb);
    const bool nv12 = layout == FFL_YUV_NV12;
    const size_t ybytes = (size_t)yw.w * yw.h * es, fbytes = ybytes * 3 / 2;
    // the planes of the window: source offset and pitch inside the frame, row bytes, rows, offset in the packed window
    struct Plane {
        size_t src, dst;
        ptrdiff_t pitch;
        size_t row;
        int rows;
    } pl[3];
    const size_t cw = (size_t)sw / 2 * es, ch = (size_t)sh / 2;  // a chroma plane's row bytes (I420) and rows
    const size_t wrow = (size_t)yw.w * es, x0 = (size_t)yw.x0 * es;
    pl[0] = {(size_t)yw.y0 * stride_bytes + x0, 0, stride_bytes, wrow, yw.h};
    int np = 3;
    if (nv12) {
        pl[1] = {(size_t)(sh + yw.y0 / 2) * stride_bytes + x0, ybytes, stride_bytes, wrow, yw.h / 2};
        np = 2;
    } else {
        const size_t u0 = (size_t)sh * sw * es + (size_t)(yw.y0 / 2) * cw + x0 / 2;
        pl[1] = {u0, ybytes, (ptrdiff_t)cw, wrow / 2, yw.h / 2};
        pl[2] = {u0 + ch * cw, ybytes + ybytes / 4, (ptrdiff_t)cw, wrow / 2, yw.h / 2};
    }
    const size_t span = (size_t)stride_bytes * (sh + sh / 2 - 1) + (size_t)sw * es;  // bytes of one frame array
    auto direct = [&](int i) {
        bool ok = in_host_buf(c, frames[i], span);
        for (int k = 0; ok && k < np; k++) ok = ((uintptr_t)(frames[i] + pl[k].src) | (size_t)pl[k].pitch | pl[k].row) % 4 == 0;
        return ok;
    };
    auto stage = [&](int i, uint8_t *h, int threads) {
        const uint8_t *src[2] = {frames[i] + pl[0].src, nullptr};
        c->pool.copy(h, src, 1, pl[0].pitch, pl[0].row, pl[0].rows, threads);
        src[0] = frames[i] + pl[1].src;
        if (!nv12) src[1] = frames[i] + pl[2].src;  // U and V are shaped alike and packed back to back: one shared copy
        c->pool.copy(h + pl[1].dst, src, nv12 ? 1 : 2, pl[1].pitch, pl[1].row, pl[1].rows, threads);
    };
    auto send_direct = [&](int i, uint8_t *d) -> int {
        for (int k = 0; k < np; k++)
            HIPCHK(c, hipMemcpy2DAsync(d + pl[k].dst, pl[k].row, frames[i] + pl[k].src, (size_t)pl[k].pitch, pl[k].row,
                                       (size_t)pl[k].rows, hipMemcpyHostToDevice, c->s_copy));
        return FFL_OK;
    };
    auto desc = [&](const uint8_t *d) {  // the window's planes: their origin in the frame is (x0, y0)
        FrameDesc s = {};
        s.p0 = d;
        s.p1 = d + ybytes;
        s.p2 = nv12 ? s.p1 + es : s.p1 + ybytes / 4;
        s.pitch0 = wrow;
        s.pitch1 = s.pitch2 = nv12 ? wrow : wrow / 2;
        s.c_step = (nv12 ? 2 : 1) * es;
        s.wx = yw.x0;
        s.wy = yw.y0;
        return s;
    };
    return upload_staged(c, lk, first, n, fbytes, fp, direct, stage, send_direct, desc, rp);
}

// Decoded 4:2:0 frames -> gray frame slots through k_frontend: the body of ffl_upload_frames_yuv (es = 1) and
// ffl_upload_frames_yuv16 (es = 2 bytes per sample, reduced by rule Y5).  Frame by frame, as ffl_upload_frames_raw: only
// the window the crop samples travels -- out of ffl_host_alloc memory one 2-D copy per plane (when every plane's rows
// start 4-byte aligned and are a multiple of 4 bytes long: unaligned ones take a slow path in the runtime's copy),
// otherwise copied into the pinned ring buffer and sent as one transfer.  On the device the window is packed: Y (w x h),
// then U and V (w/2 x h/2 each, I420) or the interleaved UV rows (w x h/2, NV12), es bytes per sample.
static int upload_yuv(ffl_ctx *c, const char *fn, int first, int n, const uint8_t *const *frames, int sw, int sh,
                      ptrdiff_t stride_bytes, int layout, int es, int depth, int msb, int rw, int rh, int crop_x, int crop_y,
                      const ffl_source_info *si) {
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> ul(c->up_mu);
    CtxLock lk(c->mu);
    if (int rc = check_frame_run(c, fn, first, n, frames, frames)) return rc;
    FrontParams fp;
    YuvWin yw;
    if (int rc = yuv_window(c, fn, sw, sh, layout, stride_bytes, es, depth, si, rw, rh, crop_x, crop_y, c->w, c->h, &fp, &yw))
        return rc;
    return send_yuv(c, lk, fn, first, n, frames, sw, sh, stride_bytes, layout, es, depth, msb, fp, yw, nullptr);
}

int ffl_upload_frames_yuv(ffl_ctx *c, int first, int n, const uint8_t *const *frames, int sw, int sh, ptrdiff_t stride_bytes,
                          int layout, int rw, int rh, int crop_x, int crop_y) {
    return upload_yuv(c, "ffl_upload_frames_yuv", first, n, frames, sw, sh, stride_bytes, layout, 1, 8, 0, rw, rh, crop_x, crop_y,
                      nullptr);
}

int ffl_upload_frames_yuv_src(ffl_ctx *c, int first, int n, const uint8_t *const *frames, int sw, int sh, ptrdiff_t stride_bytes,
                              int layout, int rw, int rh, int crop_x, int crop_y, const ffl_source_info *si) {
    return upload_yuv(c, "ffl_upload_frames_yuv", first, n, frames, sw, sh, stride_bytes, layout, 1, 8, 0, rw, rh, crop_x, crop_y, si);
}

int ffl_upload_frames_yuv16(ffl_ctx *c, int first, int n, const uint16_t *const *frames, int sw, int sh, ptrdiff_t stride_bytes,
                            int layout, int depth, int msb_aligned, int rw, int rh, int crop_x, int crop_y) {
    return upload_yuv(c, "ffl_upload_frames_yuv16", first, n, (const uint8_t *const *)frames, sw, sh, stride_bytes, layout, 2,
                      depth, msb_aligned != 0, rw, rh, crop_x, crop_y, nullptr);
}

int ffl_upload_frames_yuv16_src(ffl_ctx *c, int first, int n, const uint16_t *const *frames, int sw, int sh, ptrdiff_t stride_bytes,
                                int layout, int depth, int msb_aligned, int rw, int rh, int crop_x, int crop_y,
                                const ffl_source_info *si) {
    return upload_yuv(c, "ffl_upload_frames_yuv16", first, n, (const uint8_t *const *)frames, sw, sh, stride_bytes, layout, 2,
                      depth, msb_aligned != 0, rw, rh, crop_x, crop_y, si);
}

int ffl_upload_frame(ffl_ctx *c, int fslot, const uint8_t *data, int width, int height, int channels,
                     ptrdiff_t stride_bytes) {
    return ffl_upload_frames(c, fslot, 1, &data, width, height, channels, stride_bytes);
}

int ffl_download_frame(ffl_ctx *c, int fslot, uint8_t *dst) {
    if (!c) return FFL_ERR_INVALID;
    CtxLock lk(c->mu);
    if (!dst || fslot < 0 || fslot >= c->n_fslots)
        return set_err(c, FFL_ERR_INVALID, "ffl_download_frame: bad frame slot %d", fslot);
    if (!c->frame_valid[fslot]) return set_err(c, FFL_ERR_STATE, "ffl_download_frame: frame slot %d was never uploaded", fslot);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(dst, c->d_gray + (size_t)fslot * c->N, c->N, hipMemcpyDeviceToHost, c->s_copy));
    HIPCHK(c, hipStreamSynchronize(c->s_copy));
    return FFL_OK;
}

struct DebugCapture {
    int level, iter;
    float *I0, *I1, *R0, *R1, *M, *flow;
};

// The launches of one batch (frame expansion, the level loop, pass 1) on the lane's stream.  Everything that
// differs between two batches of the same shape is read by the kernels from the lane's device table, so this
// sequence can be captured into a hipGraph (cap == nullptr, no timing events).
static int enqueue_batch(ffl_ctx *c, ffl_ctx::Lane &L, const BatchTab &T, int n, int nU, int pov_mode, const DebugCapture *cap) {
    hipStream_t st = L.st;
    const size_t N = c->N;
    const UTab *ut = &L.d_tab->ut;
    const PairTab *pt = &L.d_tab->pt;
    // The frame-only work (level images + PolyExp of the nU unique frames) of ALL levels up front in three launches
    // (pyramid phase A + B, PolyExp) instead of ten small ones whose ramps and tails leave the device idle.
    // fuse_l0_blur: PolyExp forms level 0's image (the last job) from the gray frame, so nothing reads that level's I
    // plane but the debug capture, and the pyramid leaves the level out unless one is running
    const PyrJob *l0 = &L.pyr[L.n_jobs - 1];
    const bool fuse_l0 = c->opt.fuse_l0_blur && ffl_polyexp_from_gray_ok(*l0);
    const int skip_l0 = fuse_l0 && !cap;
    {
        ProfScope ps(c, FFL_K_PYRAMID, st);
        if (!ffl_launch_pyr_multi(c->d_gray, N, ut, nU, L.pyr, L.n_jobs - skip_l0, c->opt, st))
            for (int k = c->geo.levels; k >= skip_l0; k--)  // a level outside the merged kinds: per-level kernels
                ffl_launch_pyr_level(c->d_gray, N, ut, nU, L.pyr[c->geo.levels - k], st);
    }
    {
        ProfScope ps(c, FFL_K_POLYEXP, st);
        ffl_launch_polyexp_multi(L.poly, L.n_jobs, nU, c->pc, c->d_gray, N, ut, fuse_l0 ? l0 : nullptr, st);
    }

    int pw = 0, ph = 0;
    for (int k = c->geo.levels; k >= 0; k--) {
        const LevelGeom &g = c->geo.lv[k];
        const int lw = g.lw, lh = g.lh;
        const size_t plane = (size_t)lw * lh;
        const size_t I_stride = plane, R_stride = 5 * plane, M_stride = 5 * plane;
        float *Rk = L.d_R + c->lay.r_off[k];
        // the coarsest level starts from zero flow; nothing reads that field but UpdateMatrices (which is told
        // so) and the debug capture, so it is only materialised for the latter
        if (pw == 0 && cap)
            for (int i = 0; i < n; i++) HIPCHK(c, hipMemsetAsync(T.pt.flow[k][i], 0, sizeof(float) * 2 * plane, st));
        int mi = 0;
        // fuse_first: the level's initial UpdateMatrices (and flow upsample) run inside the first blur+solve
        // launch; the debug capture wants the initial flow and M in memory, so it keeps the separate launch
        const bool fuse_first = c->opt.fuse_first > 0 && !cap && (long)((lw + 63) / 64) * ((lh + 15) / 16) * n >= c->opt.fuse_first;
        if (!fuse_first) {
            ProfScope ps(c, FFL_K_UPDATE_MATRICES, st);
            // the x2 upsample of the coarser level's flow (K3) is fused into this launch
            ffl_launch_update_matrices(Rk, R_stride, plane, pt, k, n, L.d_M[mi], M_stride, lw, lh, pw, ph, pw == 0, cap != nullptr, c->opt, st);
        }
        bool captured = false;
        auto capture = [&]() -> int {
            HIPCHK(c, hipStreamSynchronize(st));
            if (cap->I0) HIPCHK(c, hipMemcpy(cap->I0, L.d_I + c->lay.i_off[k] + (size_t)T.pt.u0[0] * I_stride, sizeof(float) * plane, hipMemcpyDeviceToHost));
            if (cap->I1) HIPCHK(c, hipMemcpy(cap->I1, L.d_I + c->lay.i_off[k] + (size_t)T.pt.u1[0] * I_stride, sizeof(float) * plane, hipMemcpyDeviceToHost));
            if (cap->R0) HIPCHK(c, hipMemcpy(cap->R0, Rk + (size_t)T.pt.u0[0] * R_stride, sizeof(float) * 5 * plane, hipMemcpyDeviceToHost));
            if (cap->R1) HIPCHK(c, hipMemcpy(cap->R1, Rk + (size_t)T.pt.u1[0] * R_stride, sizeof(float) * 5 * plane, hipMemcpyDeviceToHost));
            if (cap->M) HIPCHK(c, hipMemcpy(cap->M, L.d_M[mi], sizeof(float) * 5 * plane, hipMemcpyDeviceToHost));
            if (cap->flow) HIPCHK(c, hipMemcpy(cap->flow, T.pt.flow[k][0], sizeof(float) * 2 * plane, hipMemcpyDeviceToHost));
            captured = true;
            return FFL_OK;
        };
        for (int it = 0; it < 3; it++) {
            if (cap && cap->level == k && cap->iter == it) {
                int rc = capture();
                if (rc) return rc;
            }
            const int update = it < 2;
            {
                ProfScope ps(c, FFL_K_BLUR_SOLVE, st, it > 0 && !cap);  // the three iterations are queued back to back
                if (it == 0 && fuse_first)
                    ffl_launch_blur_solve_first(L.d_M[mi ^ 1], M_stride, Rk, R_stride, plane, pt, k, n, lw, lh, pw, ph, c->opt, c->blur_slots, st);
                else
                    ffl_launch_blur_solve(L.d_M[mi], L.d_M[mi ^ 1], M_stride, Rk, R_stride, plane, pt, k, n, lw, lh,
                                          update, cap != nullptr, c->opt, c->blur_slots, st);
            }
            if (update) mi ^= 1;
        }
        if (cap && cap->level == k && !captured) {
            int rc = capture();
            if (rc) return rc;
        }
        pw = lw;
        ph = lh;
    }
    // pass 1 on the finished level-0 flows; records are stored straight into mapped pinned memory
    {
        ProfScope ps(c, FFL_K_PASS1, st);
        ffl_launch_pass1(pt, n, c->w, c->h, pov_mode, L.d_pkey, L.d_psum, st);
    }
    return FFL_OK;
}

// The lane's captured graph of a batch shape under the current options (*ge), captured now if there is none yet; *ge stays
// nullptr when this option epoch launches eagerly after a failed capture.  The capture records the kernels only: the
// waits and the table copy are queued on the stream before it.
static int batch_graph(ffl_ctx *c, ffl_ctx::Lane &L, const BatchTab &T, int n, int nU, int pov_mode,
                       ffl_ctx::Lane::GraphEntry **ge) {
    *ge = nullptr;
    for (auto &g : L.graphs)
        if (g.n == n && g.nU == nU && g.pov == pov_mode && g.epoch == c->opt_epoch) *ge = &g;
    if (*ge || c->graph_bad_epoch == c->opt_epoch) return FFL_OK;
    hipStream_t st = L.st;
    ffl_ctx::Lane::GraphEntry g = {n, nU, pov_mode, c->opt_epoch, Graph(), GraphExec()};
    hipError_t fail = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (fail == hipSuccess) {
        const int rc = enqueue_batch(c, L, T, n, nU, pov_mode, nullptr);
        fail = hipStreamEndCapture(st, g.graph.put());  // always: the stream must leave capture mode
        if (fail == hipSuccess && (rc != FFL_OK || !g.graph)) fail = hipErrorStreamCaptureInvalidated;
        if (fail == hipSuccess) fail = hipGraphInstantiate(g.exec.put(), g.graph, nullptr, nullptr, 0);
    }
    if (fail != hipSuccess) {
        // nothing of the failed capture is kept (it would leak once per batch), the sticky error is cleared, and
        // this context launches eagerly until the option set changes -- the batch itself is not lost
        g.exec.reset();
        g.graph.reset();
        (void)hipGetLastError();
        c->graph_bad_epoch = c->opt_epoch;
        // never silent: counted (ffl_graph_stats, bench.py `config.graphs`) and said once per context on stderr
        c->graph_failed++;
        if (!c->graph_fail_reported) {
            c->graph_fail_reported = true;
            fprintf(stderr, "libffl_hip: hipGraph capture of a %d-pair batch failed (%s); this context launches its batches "
                            "one kernel at a time until its options change (results are unaffected)\n", n, hipGetErrorString(fail));
        }
        return FFL_OK;
    }
    if (L.graphs.size() >= 16) {  // bounded cache: callers that vary the batch shape a lot re-capture
        // a replay may still be queued: graph resources are released once the lane's stream has drained
        HIPCHK(c, hipStreamSynchronize(st));
        L.graphs.erase(L.graphs.begin());
    }
    L.graphs.push_back(std::move(g));
    *ge = &L.graphs.back();
    c->graph_captured++;
    return FFL_OK;
}

static int fbg_work(ffl_ctx *c, ffl_ctx::Lane &L, const FbgPlan &p, int nU, FbgWork *wk);

// Fills the batch's table T (*nU unique frames) and queues the batch on the lane's stream: the waits for its frames and
// recycled slots, the table copy, the launches.  Once the table is filled, a failure may leave part of the batch queued.
static int queue_batch(ffl_ctx *c, ffl_ctx::Lane &L, BatchTab &T, int *nU_out, int n, const int *f0, const int *f1,
                       const int *slots, int pov_mode, const DebugCapture *cap, const DisKParams *dis,
                       const FbgPlan *fbg) {
    hipStream_t st = L.st;
    const size_t N = c->N;
    int nU = 0;
    auto uidx = [&](int fs) {  // O(1) through the context's scratch map (a linear search cost 65 k compares per 256-pair batch)
        int &u = c->u_of_fslot[fs];
        if (u < 0) {
            T.ut.fslot[nU] = fs;
            u = nU++;
        }
        return u;
    };
    for (int i = 0; i < n; i++) {
        T.pt.u0[i] = uidx(f0[i]);
        T.pt.u1[i] = uidx(f1[i]);
        T.pt.res[i] = c->d_res + slots[i];
    }
    // per level: the pair's flow field -- the lane's two ping-pong buffers, coarsest level in A; level 0 is the slot
    for (int k = c->geo.levels; k >= 0; k--) {
        const size_t plane = (size_t)c->geo.lv[k].lw * c->geo.lv[k].lh;
        float *buf = ((c->geo.levels - k) & 1) ? L.d_flowB : L.d_flowA;
        for (int i = 0; i < n; i++)
            T.pt.flow[k][i] = (k == 0) ? c->d_flow + (size_t)slots[i] * 2 * N : buf + (size_t)i * 2 * plane;
    }
    for (int k = c->geo.levels + 1; k < FFL_MAX_LEVELS; k++)
        for (int i = 0; i < n; i++) T.pt.flow[k][i] = nullptr;
    for (int i = 0; i < nU; i++) c->u_of_fslot[T.ut.fslot[i]] = -1;  // the scratch map goes back to "empty"
    *nU_out = nU;
    WaitOnce wait(st);
    for (int i = 0; i < nU; i++) HIPCHK(c, wait(c->ev_uploaded[T.ut.fslot[i]].get()));
    // a flow slot being recycled may still be read by the batch (other lane) or pass 2 that used it last
    for (int i = 0; i < n; i++) HIPCHK(c, wait(c->ev_slot_done[slots[i]].get()));
    // stream order puts this copy behind the lane's previous batch, which reads the same device table
    HIPCHK(c, hipMemcpyAsync(L.d_tab, &T, sizeof(BatchTab), hipMemcpyHostToDevice, st));

    if (fbg || dis) {
        // general-parameter Farneback and DIS batches launch eagerly (graphs stay keyed on the tuned schedule's batch shapes)
        if (fbg) {
            FbgWork wk;
            if (int rc = fbg_work(c, L, *fbg, nU, &wk)) return rc;
            ffl_launch_fb_general(&L.d_tab->ut, &L.d_tab->pt, n, nU, c->d_gray, N, c->w, c->h, *fbg, wk, st);
        } else {
            ffl_launch_dis(&L.d_tab->ut, &L.d_tab->pt, n, c->d_gray, N, L.d_M[0], *dis, st);  // scratch: the lane's first M buffer
        }
        ProfScope ps(c, FFL_K_PASS1, st);
        ffl_launch_pass1(&L.d_tab->pt, n, c->w, c->h, pov_mode, L.d_pkey, L.d_psum, st);
    } else if (c->opt.use_graph && !cap && c->prof_mask == 0) {
        ffl_ctx::Lane::GraphEntry *ge;
        if (int rc = batch_graph(c, L, T, n, nU, pov_mode, &ge)) return rc;
        if (ge) {
            HIPCHK(c, hipGraphLaunch(ge->exec, st));
            c->graph_replayed++;
        } else if (int rc = enqueue_batch(c, L, T, n, nU, pov_mode, nullptr)) {
            return rc;
        }
    } else if (int rc = enqueue_batch(c, L, T, n, nU, pov_mode, cap)) {
        return rc;
    }
    HIPCHK(c, hipGetLastError());
    return FFL_OK;
}

// One batch of pairs through the 4-scale Farneback schedule (dis == nullptr) or the DIS path + pass-1 reductions, on
// compute lane `li`.
static int run_batch(ffl_ctx *c, int li, int n, const int *f0, const int *f1, const int *slots, int pov_mode,
                     const DebugCapture *cap, const DisKParams *dis = nullptr, const FbgPlan *fbg = nullptr) {
    ffl_ctx::Lane &L = c->lanes[li];
    // the batch's table is the pinned entry of the ring entry it will record; settling that entry frees the table (its
    // batch, FFL_EV_RING batches ago, has consumed it), and the record below does not wait again
    HIPCHK(c, L.ring.settle_next());
    BatchTab &T = L.h_tab[L.ring.next % FFL_EV_RING];
    int nU = 0;
    const int rc = queue_batch(c, L, T, &nU, n, f0, f1, slots, pov_mode, cap, dis, fbg);
    // ONE event per batch: it marks the slots' results as ready, the frames' last use and the lane's work buffers as free.
    // Recorded after a failure too: later uploads, slot reuse and ffl_sync stay ordered behind whatever was queued, and the
    // slots hold no result.
    EvRef ev;
    HIPCHK(c, L.ring.record(L.st, &ev));
    for (int i = 0; i < nU; i++) c->ev_last_use[(size_t)T.ut.fslot[i] * c->frame_readers() + li] = ev;
    publish_slots(c, n, slots, ev, rc == FFL_OK);
    return rc;
}

static int check_pairs(ffl_ctx *c, int n, const int *f0, const int *f1, const int *slots) {
    if (n < 1 || n > c->max_batch) return set_err(c, FFL_ERR_INVALID, "batch of %d pairs, context allows 1..%d", n, c->max_batch);
    if (!f0 || !f1 || !slots) return set_err(c, FFL_ERR_INVALID, "NULL slot table");
    for (int i = 0; i < n; i++) {
        if (f0[i] < 0 || f0[i] >= c->n_fslots || f1[i] < 0 || f1[i] >= c->n_fslots)
            return set_err(c, FFL_ERR_INVALID, "pair %d: frame slot out of range", i);
        if (!c->frame_valid[f0[i]] || !c->frame_valid[f1[i]])
            return set_err(c, FFL_ERR_STATE, "pair %d: frame slot was never uploaded", i);
    }
    return check_flow_slots(c, "ffl_flow_pairs", n, slots, nullptr, "used twice in one batch");
}

// ---- DIS (kernels_dis.hip) ------------------------------------------------------------------

int ffl_dis_default_params(ffl_dis_params *out) {
    if (!out) return FFL_ERR_INVALID;
    *out = ffl_dis_params{2, 8, 4, 16, 5, 20.0f, 10.0f, 5.0f, 1, 1, 0};
    return FFL_OK;
}

// floats of one pair's scratch region in kernels_dis.hip (DIS_PAIR_REGION); pyramid offsets into `off` when given
static size_t dis_pair_floats(int w, int h, int finest, int coarsest, size_t *off = nullptr, size_t *pyr = nullptr) {
    size_t o = 0;
    for (int s = finest; s <= coarsest; s++) {
        if (off) off[s - finest] = o;
        o += (size_t)(w >> s) * (h >> s);
    }
    if (pyr) *pyr = o;
    return 4 * o + 20 * (size_t)(w >> finest) * (h >> finest);
}

// D2: the scales of a frame size; nullptr when supported, else the reason
static const char *dis_geometry(int w, int h, const ffl_dis_params &p, int *coarsest) {
    if (w < 1 || h < 1) return "empty frame";
    if (p.patch_size != 8) return "only patch_size 8 is supported";
    if (p.patch_stride < 1 || p.patch_stride > 8) return "patch_stride must be 1..8";
    if (p.finest_scale < 0 || p.grad_descent_iters < 1 || p.var_refine_iters < 0 || p.stripes < 0)
        return "finest_scale, var_refine_iters and stripes must be >= 0, grad_descent_iters >= 1";
    const int mx = w > h ? w : h, mn = w < h ? w : h;
    const int a = (int)(log2((double)mx / (4.0 * 8)) + 0.5), b = (int)log2((double)mn / 8);
    const int cs = a < b ? a : b;
    if (cs < p.finest_scale) return "the frame is too small for finest_scale";
    if (cs - p.finest_scale + 1 > DIS_MAX_SCALES) return "too many scales";
    if ((w % (1 << cs)) || (h % (1 << cs)))
        return "width and height must be divisible by 2^coarsest (INTER_AREA reductions by exact integer factors only)";
    for (int s = p.finest_scale; s <= cs; s++) {
        const int lw = w >> s, lh = h >> s;
        if ((lw - 8) % p.patch_stride || (lh - 8) % p.patch_stride) return "a scale is not a whole number of patch strides";
        if ((1 + (lw - 8) / p.patch_stride) * (1 + (lh - 8) / p.patch_stride) > DIS_MAX_PATCHES) return "too many patches per scale";
    }
    // a pair's working set (4 pyramids of the scales + 20 planes of the finest scale, kernels_dis.hip) must fit the
    // 5 * W * H floats per pair of a lane's first work buffer, which ffl_create sizes for Farneback
    if (dis_pair_floats(w, h, p.finest_scale, cs) > (size_t)5 * w * h) return "the per-pair working set exceeds 5 * W * H floats";
    *coarsest = cs;
    return nullptr;
}

int ffl_dis_geometry(int width, int height, const ffl_dis_params *p, int *coarsest, int *finest) {
    ffl_dis_params d;
    ffl_dis_default_params(&d);
    int cs = 0;
    if (const char *why = dis_geometry(width, height, p ? *p : d, &cs))
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_dis_geometry: DIS at %dx%d: %s", width, height, why);
    if (coarsest) *coarsest = cs;
    if (finest) *finest = (p ? *p : d).finest_scale;
    return FFL_OK;
}

// kernel parameters of a DIS batch on this context, checked against the lane's scratch (ffl_create sizes nothing for DIS)
static int dis_kparams(ffl_ctx *c, const ffl_dis_params *pp, int n, DisKParams *k) {
    ffl_dis_params p;
    ffl_dis_default_params(&p);
    if (pp) p = *pp;
    int cs = 0;
    if (const char *why = dis_geometry(c->w, c->h, p, &cs))
        return set_err(c, FFL_ERR_INVALID, "DIS at %dx%d: %s", c->w, c->h, why);
    memset(k, 0, sizeof(*k));
    k->w = c->w;
    k->h = c->h;
    k->finest = p.finest_scale;
    k->coarsest = cs;
    k->stride = p.patch_stride;
    k->gd_iters = p.grad_descent_iters;
    k->vr_iters = p.var_refine_iters;
    k->mean_norm = p.use_mean_norm != 0;
    k->spatial_prop = p.use_spatial_prop != 0;
    k->stripes = p.stripes;
    k->alpha = p.vr_alpha;
    k->gamma = p.vr_gamma;
    k->delta = p.vr_delta;
    k->pair_floats = dis_pair_floats(c->w, c->h, p.finest_scale, cs, k->pyr_off, &k->pyr_floats);
    const size_t have = 5 * c->N * (size_t)c->max_batch;  // one lane's d_M[0]; dis_geometry keeps a pair within 5 * N
    if (k->pair_floats * (size_t)n > have)
        return set_err(c, FFL_ERR_INVALID, "DIS at %dx%d, finest_scale %d: %d pairs need %zu floats of scratch, the lane has %zu",
                       c->w, c->h, p.finest_scale, n, k->pair_floats * (size_t)n, have);
    return FFL_OK;
}

// ffl_flow_pairs (dis == false) and ffl_flow_pairs_dis: a checked batch on the next compute lane
static int submit_pairs(ffl_ctx *c, int n, const int *f0, const int *f1, const int *slots, int pov_mode, bool dis,
                        const ffl_dis_params *p, const FbgPlan *fbg = nullptr) {
    if (!c) return FFL_ERR_INVALID;
    CtxLock lk(c->mu);
    int rc = check_pairs(c, n, f0, f1, slots);
    if (rc) return rc;
    // F.8: a seeded batch reads its flow slots before it overwrites them.  The read runs behind each slot's last user like
    // any recycled slot's write: queue_batch makes the lane's stream wait for the slot's ev_slot_done reference.
    if (fbg && (fbg->mode & FFL_FB_USE_INITIAL_FLOW) &&
        (rc = check_flow_slots(c, "ffl_flow_pairs_farneback_ex", n, slots, "flow", nullptr)))
        return rc;
    DisKParams k;
    if (dis && (rc = dis_kparams(c, p, n, &k))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const int li = (int)(c->next_lane++ % c->lanes.size());
    return run_batch(c, li, n, f0, f1, slots, pov_mode, nullptr, dis ? &k : nullptr, fbg);
}

int ffl_flow_pairs(ffl_ctx *c, int n, const int *fslot0, const int *fslot1, const int *flow_slots, int pov_mode) {
    return submit_pairs(c, n, fslot0, fslot1, flow_slots, pov_mode, false, nullptr);
}

int ffl_flow_pairs_dis(ffl_ctx *c, int n, const int *fslot0, const int *fslot1, const int *flow_slots, int pov_mode,
                       const ffl_dis_params *p) {
    return submit_pairs(c, n, fslot0, fslot1, flow_slots, pov_mode, true, p);
}

int ffl_debug_dis_pair(ffl_ctx *c, int f0, int f1, const ffl_dis_params *p, int scale, int stage, float *out) {
    if (!c || !out) return FFL_ERR_INVALID;
    CtxLock lk(c->mu);
    int slot = 0;
    int rc = check_pairs(c, 1, &f0, &f1, &slot);
    if (rc) return rc;
    DisKParams k;
    if ((rc = dis_kparams(c, p, 1, &k))) return rc;
    if (scale < k.finest || scale > k.coarsest || stage < 0 || stage > 4)
        return set_err(c, FFL_ERR_INVALID, "DIS debug: scale %d (valid %d..%d) / stage %d (valid 0..4)", scale, k.finest, k.coarsest, stage);
    const size_t lw = c->w >> scale, lh = c->h >> scale;
    const size_t np = (size_t)(1 + (lw - 8) / k.stride) * (1 + (lh - 8) / k.stride);
    const size_t floats = stage <= 1 ? 2 * np : 2 * lw * lh;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<float> dbg;
    HIPCHK_ALLOC(c, hipMalloc, dbg, floats);
    k.dbg = dbg;
    k.dbg_scale = scale;
    k.dbg_stage = stage;
    rc = run_batch(c, 0, 1, &f0, &f1, &slot, 0, nullptr, &k);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->lanes[0].st));
    HIPCHK(c, hipMemcpy(out, k.dbg, sizeof(float) * floats, hipMemcpyDeviceToHost));
    return FFL_OK;
}

// ---- Farneback with caller-chosen parameters (kernels_farneback_general.hip) ----------------

int ffl_farneback_default_params(ffl_farneback_params *out) {
    if (!out) return FFL_ERR_INVALID;
    *out = ffl_farneback_params{0.5f, 3, 15, 3, 5, 1.2f, 0};
    return FFL_OK;
}

static bool fbg_is_default(const ffl_farneback_params &p) {
    return p.pyr_scale == 0.5f && p.levels == 3 && p.winsize == 15 && p.iterations == 3 && p.poly_n == 5 &&
           p.poly_sigma == 1.2f && p.flags == 0;
}

// F.0: the double a caller meant by a float parameter -- the shortest decimal that reads back as the same float (1.2f is
// computed with as 1.2, as the reference's literal is)
static double fbg_widen(float f) {
    char buf[32];
    for (int d = 1; d <= 9; d++) {
        snprintf(buf, sizeof buf, "%.*g", d, (double)f);
        const double v = strtod(buf, nullptr);
        if ((float)v == f) return v;
    }
    return (double)f;
}

// F.1: nullptr when the parameters are accepted, else the reason
static const char *fbg_check(const ffl_farneback_params &p) {
    if (!(p.pyr_scale > 0.f && p.pyr_scale < 1.f)) return "pyr_scale must be in (0, 1)";
    if (p.levels < 0 || p.levels > 12) return "levels must be 0..12";
    if (p.winsize < 3 || p.winsize > 2 * FBG_MAX_M + 1 || !(p.winsize & 1))
        return "winsize must be odd, 3..63 (even windows are not supported)";
    if (p.iterations < 1 || p.iterations > 10) return "iterations must be 1..10";
    if (p.poly_n != 5 && p.poly_n != 7) return "poly_n must be 5 or 7";
    if (!(p.poly_sigma > 0.f && p.poly_sigma <= 3.f)) return "poly_sigma must be in (0, 3]";
    if (p.flags & 4) return "OPTFLOW_USE_INITIAL_FLOW (4) is not supported";
    if (p.flags & 256) return "OPTFLOW_FARNEBACK_GAUSSIAN (256) is not supported";
    if (p.flags) return "flags must be 0";
    return nullptr;
}

// The plan of p on a w x h frame (levels, sizes, Gaussians, PolyExp constants, R layout) under the mode bits of
// ffl_flow_pairs_farneback_ex, which has checked them (0 everywhere else: sizes and memory do not depend on them); nullptr or
// the reason it is refused
static const char *fbg_plan(int w, int h, const ffl_farneback_params &p, unsigned mode, FbgPlan *pl, char *why, size_t why_len) {
    if (const char *e = fbg_check(p)) return e;
    if (!frame_size_ok(w, h)) {
        snprintf(why, why_len, FFL_FRAME_SIZE_RULE, w, h);
        return why;
    }
    memset(pl, 0, sizeof(*pl));
    const double ps = fbg_widen(p.pyr_scale);
    LevelRule r;
    level_rule(w, h, ps, p.levels, &r);
    pl->levels = r.levels;
    pl->iterations = p.iterations;
    pl->poly_n = p.poly_n;
    pl->m = p.winsize / 2;
    pl->mul = (float)(1.0 / ps);
    pl->mode = mode;
    // F.7: the Gaussian window's taps, sigma = 0.3 m
    pl->win.m = pl->m;
    const double wsig = pl->m * 0.3;
    double wsum = 1.0;
    pl->win.k[0] = 1.f;
    for (int i = 1; i <= pl->m; i++) {
        const float t = (float)exp(-(i * i) / (2 * wsig * wsig));
        pl->win.k[i] = t;
        wsum += t * 2;
    }
    wsum = 1. / wsum;
    for (int i = 0; i <= pl->m; i++) pl->win.k[i] = (float)(pl->win.k[i] * wsum);
    // F.8: the coarsest level's scale, by F.1's repeated multiplication
    double sc = 1.0;
    for (int i = 0; i < pl->levels; i++) sc *= ps;
    pl->seed_scale = (float)sc;
    size_t off = 0;
    for (int k = 0; k <= pl->levels; k++) {
        const int ks = r.ksize[k];
        if (ks > 2 * FBG_MAX_R + 1) {
            snprintf(why, why_len, "%dx%d: level %d needs a %d-tap Gaussian, at most %d are supported", w, h, k, ks,
                     2 * FBG_MAX_R + 1);
            return why;
        }
        float full[2 * FBG_MAX_R + 1];
        gaussian_kernel(ks, r.sigma[k], full);
        pl->gk[k].r = ks / 2;
        for (int j = 0; j <= ks / 2; j++) pl->gk[k].k[j] = full[ks / 2 + j];
        pl->lw[k] = r.lw[k];
        pl->lh[k] = r.lh[k];
        pl->r_off[k] = off;
        off += (size_t)5 * pl->lw[k] * pl->lh[k];
    }
    pl->r_frame = off;
    // F.3: FarnebackPrepareGaussian(poly_n, poly_sigma)
    farneback_prepare_gaussian(p.poly_n, fbg_widen(p.poly_sigma), &pl->poly);
    return nullptr;
}

// floats of one pair's working set: the R regions of its two frames, M (5 N) and the two level flows (2 N each)
static size_t fbg_pair_floats(const FbgPlan &pl, size_t N) { return 2 * pl.r_frame + 9 * N; }

int ffl_farneback_geometry(int width, int height, const ffl_farneback_params *p, int *n_scales, size_t *work_bytes_per_pair) {
    if (!p) return set_err(nullptr, FFL_ERR_INVALID, "ffl_farneback_geometry: params is NULL");
    FbgPlan pl;
    char why[160];
    if (const char *e = fbg_plan(width, height, *p, 0, &pl, why, sizeof why))
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_farneback_geometry: %s", e);
    if (n_scales) *n_scales = pl.levels + 1;
    if (work_bytes_per_pair) *work_bytes_per_pair = sizeof(float) * fbg_pair_floats(pl, (size_t)width * height);
    return FFL_OK;
}

// Device bytes that ffl_flow_pairs_farneback(p) may allocate on top of ffl_estimate_bytes for a context of these arguments
// (under the current "lanes" option): per lane, the R regions of 2 * max_batch frames beyond the lane's d_R.
int ffl_farneback_extra_bytes(int width, int height, int max_batch, const ffl_farneback_params *p, size_t *bytes) {
    if (!p || !bytes || max_batch < 1 || max_batch > FFL_MAX_BATCH)
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_farneback_extra_bytes: bad arguments");
    FbgPlan pl;
    char why[160];
    if (const char *e = fbg_plan(width, height, *p, 0, &pl, why, sizeof why))
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_farneback_extra_bytes: %s", e);
    const size_t r_cap = context_layout(width, height, 2, 1, max_batch).R;  // R does not depend on the slot counts
    const size_t need = pl.r_frame * 2 * (size_t)max_batch;
    *bytes = need > r_cap ? sizeof(float) * (need - r_cap) * (size_t)default_lanes() : 0;
    return FFL_OK;
}

// Where a general batch of nU unique frames works on lane L.  M and the level flows always fit the lane's d_M[0],
// d_flowA and d_flowB (sized for 5 N and 2 N per pair; the blur planes need 2 N and the level images N per unique frame, at
// most two per pair); the R regions of every level go to d_R when they fit, else to the lane's general-path work area, grown
// to the largest request seen once the lane's queued work is over.
static int fbg_work(ffl_ctx *c, ffl_ctx::Lane &L, const FbgPlan &p, int nU, FbgWork *wk) {
    wk->M = L.d_M[0];
    wk->fa = L.d_flowA;
    wk->fb = L.d_flowB;
    const size_t need = p.r_frame * (size_t)nU;
    if (need <= c->lay.R) {
        wk->R = L.d_R;
        return FFL_OK;
    }
    if (need > L.gen_cap) {
        if (L.d_gen) {
            hipEvent_t e = ev_latest(L.ring).get();  // the lane's last batch may still read the old area
            if (e) HIPCHK(c, hipEventSynchronize(e));
            L.gen_cap = 0;
            HIPCHK_AS(c, "hipFree", L.d_gen.reset());
        }
        const hipError_t e = L.d_gen.alloc(need);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            L.d_gen.release();  // nothing was allocated
            return set_err(c, FFL_ERR_HIP, "general Farneback work area: hipMalloc of %zu bytes (%d frames x %zu floats) failed: %s",
                           sizeof(float) * need, nU, p.r_frame, hipGetErrorString(e));
        }
        L.gen_cap = need;
    }
    wk->R = L.d_gen;
    return FFL_OK;
}

int ffl_flow_pairs_farneback(ffl_ctx *c, int n, const int *fslot0, const int *fslot1, const int *flow_slots, int pov_mode,
                             const ffl_farneback_params *p) {
    if (!c) return FFL_ERR_INVALID;
    ffl_farneback_params d;
    ffl_farneback_default_params(&d);
    const ffl_farneback_params &q = p ? *p : d;
    int force;
    {
        CtxLock lk(c->mu);
        force = c->opt.fb_general;
    }
    if (fbg_is_default(q) && !force) return ffl_flow_pairs(c, n, fslot0, fslot1, flow_slots, pov_mode);
    FbgPlan pl;
    char why[160];
    if (const char *e = fbg_plan(c->w, c->h, q, 0, &pl, why, sizeof why)) {
        CtxLock lk(c->mu);
        return set_err(c, FFL_ERR_INVALID, "ffl_flow_pairs_farneback: %s", e);
    }
    return submit_pairs(c, n, fslot0, fslot1, flow_slots, pov_mode, false, nullptr, &pl);
}

// mode == 0 is ffl_flow_pairs_farneback; any other mode runs the general kernels, at the default numbers too
int ffl_flow_pairs_farneback_ex(ffl_ctx *c, int n, const int *fslot0, const int *fslot1, const int *flow_slots, int pov_mode,
                                const ffl_farneback_params *p, unsigned mode) {
    if (mode == 0) return ffl_flow_pairs_farneback(c, n, fslot0, fslot1, flow_slots, pov_mode, p);
    if (const unsigned unknown = mode & ~(FFL_FB_USE_INITIAL_FLOW | FFL_FB_GAUSSIAN_WINDOW)) {
        CtxLock lk;
        if (c) lk = CtxLock(c->mu);
        return set_err(c, FFL_ERR_INVALID, "ffl_flow_pairs_farneback_ex: unknown mode bit(s) 0x%x (known: "
                       "FFL_FB_USE_INITIAL_FLOW 4, FFL_FB_GAUSSIAN_WINDOW 256)", unknown);
    }
    if (!c) return FFL_ERR_INVALID;
    ffl_farneback_params d;
    ffl_farneback_default_params(&d);
    FbgPlan pl;
    char why[160];
    if (const char *e = fbg_plan(c->w, c->h, p ? *p : d, mode, &pl, why, sizeof why)) {
        CtxLock lk(c->mu);
        return set_err(c, FFL_ERR_INVALID, "ffl_flow_pairs_farneback_ex: %s", e);
    }
    return submit_pairs(c, n, fslot0, fslot1, flow_slots, pov_mode, false, nullptr, &pl);
}

int ffl_debug_pair(ffl_ctx *c, int f0, int f1, int level, int iter, float *I0, float *I1, float *R0, float *R1,
                   float *M, float *flow) {
    if (!c) return FFL_ERR_INVALID;
    CtxLock lk(c->mu);
    int slot = 0;
    int rc = check_pairs(c, 1, &f0, &f1, &slot);
    if (rc) return rc;
    if (level < 0 || level > c->geo.levels || iter < 0 || iter > 3) return set_err(c, FFL_ERR_INVALID, "bad level/iter");
    HIPCHK(c, hipSetDevice(c->device));
    DebugCapture cap = {level, iter, I0, I1, R0, R1, M, flow};
    rc = run_batch(c, 0, 1, &f0, &f1, &slot, 0, &cap);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->lanes[0].st));
    return FFL_OK;
}

int ffl_pass1_result(ffl_ctx *c, int slot, float cut_threshold, int32_t *x, int32_t *y, float *div_val, float *mean_mag,
                     int *cut) {
    return ffl_pass1_results(c, 1, &slot, cut_threshold, x, y, div_val, mean_mag, cut);
}

int ffl_pass1_results(ffl_ctx *c, int n, const int *slots, float cut_threshold, int32_t *x, int32_t *y, float *div_val,
                      float *mean_mag, int *cut) {
    if (!c) return FFL_ERR_INVALID;
    CtxLock lk(c->mu);
    if (n < 0 || (n > 0 && !slots)) return set_err(c, FFL_ERR_INVALID, "ffl_pass1_results: bad arguments");
    // one lock, one wait per DISTINCT event (the slots of a batch share theirs), then the records: 256 one-slot calls
    // cost 0.3 ms of host time per batch at the 256x256 operating point.  At most lanes x FFL_EV_RING + FFL_EV_RING
    // events are live at a time (the lanes' rings and post_ring).
    if (int rc = check_flow_slots(c, "ffl_pass1_results", n, slots, "result", nullptr)) return rc;
    std::vector<hipEvent_t> evs;
    for (int i = 0; i < n; i++) {
        hipEvent_t e = c->ev_slot_done[slots[i]].get();
        if (e && std::find(evs.begin(), evs.end(), e) == evs.end()) evs.push_back(e);
    }
    if (int rc = wait_unlocked(c, lk, evs.data(), (int)evs.size())) return rc;
    const double npx = (double)c->w * (double)c->h;
    for (int i = 0; i < n; i++) {
        const Pass1Result &r = c->h_res[slots[i]];
        const float mm = (float)ffl_record_mean(r, npx);  // a record formed under a weight map holds its own quotient
        if (x) x[i] = r.x;
        if (y) y[i] = r.y;
        if (div_val) div_val[i] = r.div_val;
        if (mean_mag) mean_mag[i] = mm;
        if (cut) cut[i] = mm > cut_threshold ? 1 : 0;
    }
    return FFL_OK;
}

// The extra scratch of stream `post` (the DevBuf<double> members of ffl_ctx under "extra scratch"): what a context gains with
// the first four-component, weighted, ffl_cell_stats or ffl_motion_fit call, in doubles for FFL_MAXB items.  The ffl_*_extra_bytes entry points
// report a row, post_scratch allocates it.
enum { SCR_AXES = 0, SCR_WEIGHTS, SCR_CELLS, SCR_MOTION, SCR_REDETECT };
struct PostScratchRow {
    size_t (*doubles)(int w, int h, int max_batch);   // max_batch: read by the rows that are not sized for FFL_MAXB items
    const char *name;               // in the message of a failed allocation
    DevBuf<double> ffl_ctx::*buf;
};
static const PostScratchRow kPostScratch[] = {
    {[](int w, int h, int) { return (size_t)FFL_NAXES * (size_t)ffl_radial_blocks(w, h) * FFL_MAXB; }, "four-component",
     &ffl_ctx::d_apsum},
    // one buffer for whichever of the two runs: pass 2's FFL_NAXES + 1 partials per workgroup of the radial grid, or pass 1's SW
    // per workgroup of its grid
    {[](int w, int h, int) {
         const size_t p2 = (size_t)(FFL_NAXES + 1) * (size_t)ffl_radial_blocks(w, h), p1 = (size_t)ffl_pass1_blocks(w, h);
         return (p2 > p1 ? p2 : p1) * FFL_MAXB;
     }, "weighted", &ffl_ctx::d_wpsum},
    // the row sums of rule G5, whatever the size and the grid
    {[](int, int, int) { return (size_t)2 * FFL_MAX_CELLS * FFL_MAXB; }, "cell-row", &ffl_ctx::d_cellrow},
    // the twelve sums of rule C4 per workgroup of the radial grid
    {[](int w, int h, int) { return (size_t)FFL_MOTION_NSUMS * (size_t)ffl_radial_blocks(w, h) * FFL_MAXB; }, "motion-fit",
     &ffl_ctx::d_mpsum},
    // the tile keys, the pick and the re-walked keys of max_batch x FFL_MAX_TRACKS searches (64-bit words, held as doubles' bytes)
    {[](int w, int h, int mb) { return ffl_redetect_words(w, h) * (size_t)mb * FFL_TRACK_MAX_T; }, "re-detection",
     &ffl_ctx::d_rdscr},
};

static int cell_grid_check(ffl_ctx *c, const char *fn, int width, int height, int cells, int *cell_w, int *cell_h);

// cells: the grid of the SCR_CELLS row, whose size check is rule G1's
static int post_scratch_bytes(const char *fn, int row, int width, int height, int cells, size_t *bytes, int max_batch = FFL_MAXB) {
    if (!bytes) return set_err(nullptr, FFL_ERR_INVALID, "%s: bytes is NULL", fn);
    if (row == SCR_CELLS) {
        if (int rc = cell_grid_check(nullptr, fn, width, height, cells, nullptr, nullptr)) return rc;
    } else if (!frame_size_ok(width, height))
        return set_err(nullptr, FFL_ERR_INVALID, "%s: " FFL_FRAME_SIZE_RULE, fn, width, height);
    *bytes = sizeof(double) * kPostScratch[row].doubles(width, height, max_batch);
    return FFL_OK;
}

int ffl_axes_extra_bytes(int width, int height, size_t *bytes) {   // + sizeof(AxesRecord) * FFL_MAXB of page-locked host memory
    return post_scratch_bytes("ffl_axes_extra_bytes", SCR_AXES, width, height, 0, bytes);
}

int ffl_weights_extra_bytes(int width, int height, size_t *bytes) {
    return post_scratch_bytes("ffl_weights_extra_bytes", SCR_WEIGHTS, width, height, 0, bytes);
}

int ffl_cells_extra_bytes(int width, int height, int cells, size_t *bytes) {
    return post_scratch_bytes("ffl_cells_extra_bytes", SCR_CELLS, width, height, cells, bytes);
}

int ffl_motion_extra_bytes(int width, int height, size_t *bytes) {
    return post_scratch_bytes("ffl_motion_extra_bytes", SCR_MOTION, width, height, 0, bytes);
}

int ffl_redetect_extra_bytes(int width, int height, int max_batch, size_t *bytes) {
    if (max_batch < 1 || max_batch > FFL_MAX_BATCH)
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_redetect_extra_bytes: max_batch = %d outside 1..%d (FFL_MAX_BATCH)", max_batch,
                       (int)FFL_MAX_BATCH);
    return post_scratch_bytes("ffl_redetect_extra_bytes", SCR_REDETECT, width, height, 0, bytes, max_batch);
}

// The first call that needs a row allocates it (the caller holds post_mu and the context lock).  The axes row comes with
// ffl_radial_axes' mapped pinned records.
static int post_scratch(ffl_ctx *c, const char *fn, int row) {
    const PostScratchRow &r = kPostScratch[row];
    DevBuf<double> &buf = c->*r.buf;
    if (buf && (row != SCR_AXES || c->h_axes)) return FFL_OK;
    const size_t doubles = r.doubles(c->w, c->h, c->max_batch);
    hipError_t e = buf ? hipSuccess : buf.alloc(doubles);
    if (e != hipSuccess) buf.release();  // nothing was allocated
    if (e == hipSuccess && row == SCR_AXES && !c->h_axes) {
        e = c->h_axes.alloc(FFL_MAXB, hipHostMallocMapped);
        if (e != hipSuccess) c->h_axes.release();
        else if ((e = hipHostGetDevicePointer((void **)&c->d_axes, c->h_axes, 0)) != hipSuccess) (void)c->h_axes.reset();
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        char pinned[48] = "";
        if (row == SCR_AXES) snprintf(pinned, sizeof pinned, " + %zu page-locked", sizeof(AxesRecord) * FFL_MAXB);
        return set_err(c, FFL_ERR_HIP, "%s: allocating the %s scratch (%zu bytes%s) failed: %s", fn, r.name,
                       sizeof(double) * doubles, pinned, hipGetErrorString(e));
    }
    return FFL_OK;
}

// ffl_radial (axes = false: out[i]) and ffl_radial_axes (out[i * FFL_N_AXES + component]): one protocol.
static int radial_call(ffl_ctx *c, const char *fn, bool axes, int n, const int *slots, const double *cx, const double *cy,
                       const int *is_cut, int pov_mode, double *out) {
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // one pass-2 call at a time owns stream `post`, h_wtab and h_radial / h_axes
    CtxLock lk(c->mu);
    if (n < 1 || n > FFL_MAXB || !slots || !cx || !cy || !out) return set_err(c, FFL_ERR_INVALID, "%s: bad arguments", fn);
    if (int rc = check_flow_slots(c, fn, n, slots, "flow", nullptr)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const int nc = axes ? FFL_N_AXES : 1;
    WindowItem *tab = c->h_wtab;  // the previous call waited for s_post, so the pinned copy is free
    WaitOnce wait_post(c->s_post);
    int m = 0;
    int map[FFL_MAXB], used[FFL_MAXB];  // the slots pass 2 reads and their places in `out`
    for (int i = 0; i < n; i++) {
        if (is_cut && is_cut[i]) {  // FF:766-767: a cut returns 0.0 without looking at the flow
            for (int k = 0; k < nc; k++) out[(size_t)i * nc + k] = 0.0;
            continue;
        }
        HIPCHK(c, wait_post(c->ev_slot_done[slots[i]].get()));
        tab[m] = WindowItem{c->d_flow + (size_t)slots[i] * 2 * c->N, cx[i], cy[i], 0, 0};
        used[m] = slots[i];
        map[m++] = i;
    }
    if (m == 0) return FFL_OK;
    if (axes)
        if (int rc = post_scratch(c, fn, SCR_AXES)) return rc;
    hipStream_t st = c->s_post;
    {
        HIPCHK(c, hipMemcpyAsync(c->d_wtab, tab, sizeof(WindowItem) * m, hipMemcpyHostToDevice, st));
        ProfScope ps(c, FFL_K_RADIAL, st);
        ffl_launch_radial(c->d_wtab, m, c->w, c->h, pov_mode, c->d_wytab, RadialForm{nc, nullptr},
                          axes ? c->d_apsum : c->d_rpsum, axes ? (void *)c->d_axes : (void *)c->d_radial, st);
    }
    // the slots' "last use" now includes this pass 2: the wait below runs without the context lock, so another thread
    // may queue a batch that recycles one of these slots meanwhile -- it must run behind the kernel that reads them
    EvRef ev;
    if (int rc = publish_post(c, m, used, &ev)) return rc;
    lk.unlock();  // the wait (for the batches the slots come from, then pass 2) does not hold up uploads / submissions
    hipError_t se = hipStreamSynchronize(st);  // the final kernel stored into the mapped pinned buffer
    lk.lock();
    HIPCHK(c, se);
    HIPCHK(c, hipGetLastError());
    for (int j = 0; j < m; j++) {
        if (!axes) {
            out[map[j]] = c->h_radial[j].dot;
            continue;
        }
        const AxesRecord &r = c->h_axes[j];
        double *o = out + (size_t)map[j] * FFL_N_AXES;
        o[FFL_AXIS_RADIAL] = r.base.dot;
        o[FFL_AXIS_TANGENTIAL] = r.tangential;
        o[FFL_AXIS_SHIFT_X] = r.shift_x;
        o[FFL_AXIS_SHIFT_Y] = r.shift_y;
    }
    return FFL_OK;
}

int ffl_radial(ffl_ctx *c, int n, const int *slots, const double *cx, const double *cy, const int *is_cut, int pov_mode,
               double *out) {
    return radial_call(c, "ffl_radial", false, n, slots, cx, cy, is_cut, pov_mode, out);
}

int ffl_radial_axes(ffl_ctx *c, int n, const int *slots, const double *cx, const double *cy, const int *is_cut, int pov_mode,
                    double *out) {
    return radial_call(c, "ffl_radial_axes", true, n, slots, cx, cy, is_cut, pov_mode, out);
}

int ffl_download_flow(ffl_ctx *c, int slot, float *dst) {
    if (!c) return FFL_ERR_INVALID;
    CtxLock lk(c->mu);
    if (!dst) return set_err(c, FFL_ERR_INVALID, "ffl_download_flow: bad arguments");
    if (int rc = check_flow_slots(c, "ffl_download_flow", 1, &slot, "flow", nullptr)) return rc;
    hipEvent_t ev = c->ev_slot_done[slot].get();
    if (int rc = wait_unlocked(c, lk, &ev, 1)) return rc;
    HIPCHK(c, hipMemcpy(dst, c->d_flow + (size_t)slot * 2 * c->N, sizeof(float) * 2 * c->N, hipMemcpyDeviceToHost));
    return FFL_OK;
}

// ---- device-memory I/O -------------------------------------------------------------------------
// the rules of a device frame's format, sample size and depth (the map-driven call shares them and the plane rules)
static int dev_format_rules(ffl_ctx *c, const char *fn, int idx, int fmt, int es, int depth, int sw, int sh, const ffl_dev_frame *f) {
    if (!f) return set_err(c, FFL_ERR_INVALID, "%s: frame %d: NULL descriptor", fn, idx);
    if (fmt < FFL_DEV_GRAY || fmt > FFL_DEV_NV12)
        return set_err(c, FFL_ERR_INVALID, "%s: unknown format %d (FFL_DEV_GRAY 0, BGR 1, RGB 2, I420 3, NV12 4)", fn, fmt);
    const bool yuv = fmt == FFL_DEV_I420 || fmt == FFL_DEV_NV12;
    if (es == 2 && !yuv)
        return set_err(c, FFL_ERR_INVALID, "%s: 16-bit frames are 4:2:0 only: format %d is neither FFL_DEV_I420 3 nor FFL_DEV_NV12 4",
                       fn, fmt);
    if (es == 2 && (depth < 9 || depth > 16))
        return set_err(c, FFL_ERR_INVALID, "%s: depth %d outside 9..16 (8-bit frames go through ffl_upload_frames_device)", fn, depth);
    if (yuv && ((sw & 1) || (sh & 1)))
        return set_err(c, FFL_ERR_INVALID, "%s: 4:2:0 needs an even width and height, source is %dx%d", fn, sw, sh);
    return FFL_OK;
}

// the rules of the stored planes of a frame whose format passed dev_format_rules
static int dev_plane_rules(ffl_ctx *c, const char *fn, int idx, int fmt, int es, int sw, int sh, const ffl_dev_frame *f) {
    const bool yuv = fmt == FFL_DEV_I420 || fmt == FFL_DEV_NV12;
    const ptrdiff_t big = (ptrdiff_t)1 << 40;
    const ptrdiff_t p0 = f->pitch[0], ps = f->pixel_stride, cs = f->channel_stride;
    if (!f->plane[0] || (yuv && !f->plane[1]) || (fmt == FFL_DEV_I420 && !f->plane[2]))
        return set_err(c, FFL_ERR_INVALID, "%s: frame %d: a plane the format reads is NULL", fn, idx);
    if (yuv) {
        const ptrdiff_t p1 = f->pitch[1], p2 = fmt == FFL_DEV_I420 ? f->pitch[2] : p1;
        const ptrdiff_t cmin = (fmt == FFL_DEV_I420 ? sw / 2 : sw) * es;
        if (p0 < 0 || p1 < 0 || p2 < 0) return set_err(c, FFL_ERR_INVALID, "%s: frame %d: negative stride", fn, idx);
        if (es == 2 && ((p0 | p1 | p2) & 1))
            return set_err(c, FFL_ERR_INVALID, "%s: frame %d: odd pitch %td / %td / %td: rows of 16-bit samples start 2-byte aligned", fn,
                           idx, p0, p1, p2);
        if (es == 2 && (((uintptr_t)f->plane[0] | (uintptr_t)f->plane[1] | (fmt == FFL_DEV_I420 ? (uintptr_t)f->plane[2] : 0)) & 1))
            return set_err(c, FFL_ERR_INVALID, "%s: frame %d: a plane of 16-bit samples is not 2-byte aligned", fn, idx);
        if (p0 < (ptrdiff_t)sw * es || p0 > big)
            return set_err(c, FFL_ERR_INVALID, "%s: frame %d: Y pitch %td too small for a row of %d pixels", fn, idx, p0, sw);
        if (p1 < cmin || p2 < cmin || p1 > big || p2 > big)
            return set_err(c, FFL_ERR_INVALID, "%s: frame %d: chroma pitch %td / %td too small for a row of %td bytes", fn, idx, p1, p2, cmin);
        return FFL_OK;
    }
    if (p0 < 0 || ps < 0 || cs < 0) return set_err(c, FFL_ERR_INVALID, "%s: frame %d: negative stride", fn, idx);
    if (p0 > big || ps > big || cs > big) return set_err(c, FFL_ERR_INVALID, "%s: frame %d: stride beyond 2^40", fn, idx);
    if (ps < 1) return set_err(c, FFL_ERR_INVALID, "%s: frame %d: pixel stride %td too small (>= 1)", fn, idx, ps);
    if (fmt == FFL_DEV_GRAY) {
        if (p0 < (ptrdiff_t)(sw - 1) * ps + 1)
            return set_err(c, FFL_ERR_INVALID, "%s: frame %d: pitch %td too small for %d pixels %td bytes apart", fn, idx, p0, sw, ps);
        return FFL_OK;
    }
    if (cs < 1) return set_err(c, FFL_ERR_INVALID, "%s: frame %d: channel stride %td too small (>= 1)", fn, idx, cs);
    if (ps >= 3 * cs) {  // packed: the three channels of a pixel lie within its pixel stride
        if (p0 < (ptrdiff_t)(sw - 1) * ps + 2 * cs + 1)
            return set_err(c, FFL_ERR_INVALID, "%s: frame %d: pitch %td too small for %d pixels %td bytes apart (channel stride %td)",
                           fn, idx, p0, sw, ps, cs);
    } else {  // planar: every channel plane ends before the next begins
        if (p0 < (ptrdiff_t)(sw - 1) * ps + 1)
            return set_err(c, FFL_ERR_INVALID, "%s: frame %d: pitch %td too small for %d pixels %td bytes apart", fn, idx, p0, sw, ps);
        if (cs < p0 * sh)
            return set_err(c, FFL_ERR_INVALID,
                           "%s: frame %d: channel stride %td too small: neither packed (pixel stride %td >= 3 * channel stride) "
                           "nor planar (channel stride >= pitch * height = %td)", fn, idx, cs, ps, p0 * sh);
    }
    return FFL_OK;
}

static int dev_front_class(int fmt) {  // what front_source / front_geometry call the format
    return fmt == FFL_DEV_GRAY ? FRONT_GRAY : (fmt == FFL_DEV_I420 || fmt == FFL_DEV_NV12) ? FRONT_YUV : FRONT_BGR;
}

// Every geometry rule of a device frame (ffl.h, ffl_dev_frame_check / ffl_dev_frame_check16); fn and frame index prefix the
// message.  Fills the geometry of *p.  es: bytes per sample (2: the 16-bit 4:2:0 frames of rule Y5, whose depth is checked
// here too).
static int dev_frame_check(ffl_ctx *c, const char *fn, int idx, int fmt, int es, int depth, int sw, int sh, const ffl_dev_frame *f,
                           const ffl_source_info *si, int rw, int rh, int cx, int cy, int ow, int oh, FrontParams *p) {
    if (int rc = dev_format_rules(c, fn, idx, fmt, es, depth, sw, sh, f)) return rc;
    // the metadata, gray's two rules (in upright terms) and the crop; everything after it is about the stored planes
    if (int rc = front_geometry(c, fn, dev_front_class(fmt), sw, sh, si, rw, rh, cx, cy, ow, oh, p)) return rc;
    return dev_plane_rules(c, fn, idx, fmt, es, sw, sh, f);
}

// bytes of each plane a checked frame spans from plane[k] (0: unused)
static void dev_frame_extents(int fmt, int es, int sw, int sh, const ffl_dev_frame *f, size_t ext[3]) {
    ext[0] = ext[1] = ext[2] = 0;
    if (fmt == FFL_DEV_I420 || fmt == FFL_DEV_NV12) {
        const size_t row = (size_t)sw * es;  // es: bytes per sample
        ext[0] = (size_t)(sh - 1) * f->pitch[0] + row;
        if (fmt == FFL_DEV_NV12) {
            ext[1] = (size_t)(sh / 2 - 1) * f->pitch[1] + row;
        } else {
            ext[1] = (size_t)(sh / 2 - 1) * f->pitch[1] + row / 2;
            ext[2] = (size_t)(sh / 2 - 1) * f->pitch[2] + row / 2;
        }
    } else {
        ext[0] = (size_t)(sh - 1) * f->pitch[0] + (size_t)(sw - 1) * f->pixel_stride + 1 +
                 (fmt == FFL_DEV_GRAY ? 0 : 2 * (size_t)f->channel_stride);
    }
}

// [p, p + bytes) must be device memory of the context's device inside one allocation
static const char *kHostFrames = "host frames go through ffl_upload_frames, ffl_upload_frames_raw, ffl_upload_frames_yuv or "
                                 "ffl_upload_frames_yuv16";
static const char *kHostFramesRemap = "host frames go through ffl_upload_frames_remap";
static int dev_mem_check(ffl_ctx *c, const char *fn, const char *what, const void *p, size_t bytes,
                         const char *host_hint = kHostFrames) {
    hipPointerAttribute_t a;
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, FFL_ERR_INVALID, "%s: %s is not device memory (unknown to HIP); %s", fn, what, host_hint);
    }
    if (a.type == hipMemoryTypeHost)
        return set_err(c, FFL_ERR_INVALID, "%s: %s is page-locked host memory (ffl_host_alloc / hipHostMalloc); %s", fn, what,
                       host_hint);
    if (a.type != hipMemoryTypeDevice)
        return set_err(c, FFL_ERR_INVALID, "%s: %s is not device memory (memory type %d); %s", fn, what, (int)a.type, host_hint);
    if (a.device != c->device)
        return set_err(c, FFL_ERR_INVALID, "%s: %s is memory of device %d, the context is on device %d", fn, what, a.device, c->device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, FFL_ERR_INVALID, "%s: %s: hipMemGetAddressRange failed (%s)", fn, what, hipGetErrorString(e));
    }
    if ((const char *)p + bytes > (const char *)base + size)
        return set_err(c, FFL_ERR_INVALID, "%s: %s spans %zu bytes, %zu more than its allocation holds", fn, what, bytes,
                       (size_t)((const char *)p + bytes - ((const char *)base + size)));
    return FFL_OK;
}

// The stream contract of the device-memory calls (ffl.h): caller_stream() names the caller's stream and refuses it while it
// captures (the first HIP call made on it: device-memory I/O is never captured into anyone's graph); caller_join() orders the
// library's stream behind it; at its end a call makes the caller's stream wait for the library's event in turn.
static int caller_stream(ffl_ctx *c, const char *fn, uint64_t stream, hipStream_t *cst) {
    hipStream_t st = *cst = (hipStream_t)(uintptr_t)stream;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipError_t e = hipStreamIsCapturing(st, &cs);
    if (e == hipErrorStreamCaptureImplicit) cs = hipStreamCaptureStatusActive;  // the null stream while a global capture runs
    else if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_err(c, FFL_ERR_HIP, "%s: hipStreamIsCapturing failed: %s", fn, hipGetErrorString(e));
    }
    if (cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return set_err(c, FFL_ERR_STATE, "%s: the stream is capturing a graph; device-memory I/O is never captured (call it "
                                         "before or after the capture)", fn);
    }
    return FFL_OK;
}

// the stream `wait` is for (`copy` or `post`) waits for the work the caller has queued on cst
static int caller_join(ffl_ctx *c, hipStream_t cst, WaitOnce &wait) {
    HIPCHK(c, hipEventRecord(c->ev_caller, cst));
    HIPCHK(c, wait(c->ev_caller));
    return FFL_OK;
}

// The contract for a call that queues on stream `post` (the caller holds post_mu and the context lock, and has refused
// what it can refuse without the device).  post_begin(): the caller's stream (*cst), the check of the call's nreg regions of
// caller memory in order, then stream `post` behind the caller's queued work and behind the last users of the n slots the call reads
// or writes.  post_end(), after the launches: the call becomes those slots' last use, and the caller's later work runs
// behind it.
struct PostRegion {
    const char *what;
    const void *p;
    size_t bytes;
    const char *host_hint;
};
static int post_begin(ffl_ctx *c, const char *fn, uint64_t stream, hipStream_t *cst, const PostRegion *reg, int nreg, int n,
                      const int *slots) {
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = caller_stream(c, fn, stream, cst)) return rc;
    for (int k = 0; k < nreg; k++)
        if (int rc = dev_mem_check(c, fn, reg[k].what, reg[k].p, reg[k].bytes, reg[k].host_hint)) return rc;
    WaitOnce wait_post(c->s_post);
    if (int rc = caller_join(c, *cst, wait_post)) return rc;
    for (int i = 0; i < n; i++) HIPCHK(c, wait_post(c->ev_slot_done[slots[i]].get()));
    return FFL_OK;
}

static int post_end(ffl_ctx *c, hipStream_t cst, int n, const int *slots) {
    HIPCHK(c, hipGetLastError());
    EvRef done;
    if (int rc = publish_post(c, n, slots, &done)) return rc;  // a batch recycling one of the slots waits for this call
    HIPCHK(c, hipStreamWaitEvent(cst, done.get(), 0));
    return FFL_OK;
}

// post_end() for a call that also read frame slots on stream `post` (ffl_residual_weights, ffl_texture_weights): its event
// becomes the last reader on stream `post` of the nf slots of fs0 and (unless NULL) fs1 -- ev_last_use's last column, which
// every later upload into one of them waits for (wait_frame_free).  The reader is recorded whether or not post_end succeeds:
// an event of its own if post_end recorded none, so that a launch that was queued is never overtaken by an upload (if even that
// fails the stream is drained).
static int post_end_frames(ffl_ctx *c, hipStream_t cst, int n, const int *slots, int nf, const int *fs0, const int *fs1) {
    const unsigned long long before = c->post_ring.next;
    const int rc = post_end(c, cst, n, slots);
    EvRef done = ev_latest(c->post_ring);
    if (c->post_ring.next == before && c->post_ring.record(c->s_post, &done) != hipSuccess) {
        (void)hipStreamSynchronize(c->s_post);
        done = EvRef{};
    }
    const size_t nr = c->frame_readers();
    for (int i = 0; i < nf; i++) {
        c->ev_last_use[(size_t)fs0[i] * nr + (nr - 1)] = done;
        if (fs1) c->ev_last_use[(size_t)fs1[i] * nr + (nr - 1)] = done;
    }
    return rc;
}

int ffl_dev_frame_check(int format, int sw, int sh, const ffl_dev_frame *f, int rw, int rh, int cx, int cy, int out_w, int out_h) {
    FrontParams p;
    return dev_frame_check(nullptr, "ffl_dev_frame_check", 0, format, 1, 8, sw, sh, f, nullptr, rw, rh, cx, cy, out_w, out_h, &p);
}

int ffl_dev_frame_check_src(int format, int sw, int sh, const ffl_dev_frame *f, int rw, int rh, int cx, int cy, int out_w, int out_h,
                            const ffl_source_info *si) {
    FrontParams p;
    return dev_frame_check(nullptr, "ffl_dev_frame_check", 0, format, 1, 8, sw, sh, f, si, rw, rh, cx, cy, out_w, out_h, &p);
}

int ffl_dev_frame_check16(int format, int depth, int sw, int sh, const ffl_dev_frame *f, int rw, int rh, int cx, int cy, int out_w,
                          int out_h) {
    FrontParams p;
    return dev_frame_check(nullptr, "ffl_dev_frame_check16", 0, format, 2, depth, sw, sh, f, nullptr, rw, rh, cx, cy, out_w, out_h, &p);
}

int ffl_dev_frame_check16_src(int format, int depth, int sw, int sh, const ffl_dev_frame *f, int rw, int rh, int cx, int cy, int out_w,
                              int out_h, const ffl_source_info *si) {
    FrontParams p;
    return dev_frame_check(nullptr, "ffl_dev_frame_check16", 0, format, 2, depth, sw, sh, f, si, rw, rh, cx, cy, out_w, out_h, &p);
}

// What ffl_upload_frames_device(16) and ffl_upload_frames_device_remap share once every frame has passed its rules: the
// stream contract, the memory checks, the descriptor table, the one launch (rp: k_frontend_remap_dev with that map) and the
// publishing of the slots.
static int send_device(ffl_ctx *c, const char *fn, int first, int n, const ffl_dev_frame *frames, int fmt, int es, int depth,
                       int msb, int sw, int sh, uint64_t stream, FrontParams &p, const RemapParams *rp) {
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t cst;
    if (int rc = caller_stream(c, fn, stream, &cst)) return rc;
    static const char *names[3] = {"plane 0", "plane 1", "plane 2"};
    for (int i = 0; i < n; i++) {
        size_t ext[3];
        dev_frame_extents(fmt, es, sw, sh, &frames[i], ext);
        for (int k = 0; k < 3; k++)
            if (ext[k])
                if (int rc = dev_mem_check(c, fn, names[k], frames[i].plane[k], ext[k], rp ? kHostFramesRemap : kHostFrames)) return rc;
    }
    const size_t ring = c->up_ring.ev.size();
    if (!c->d_dtab) {
        DevBuf<FrameDesc> d; PinBuf<FrameDesc> h;  // all or nothing: the context takes them once both exist, else the next call retries
        HIPCHK_ALLOC(c, hipMalloc, d, c->n_fslots);
        HIPCHK_ALLOC(c, hipHostMalloc, h, c->n_fslots * ring, hipHostMallocDefault);
        c->d_dtab = std::move(d);
        c->h_dtab = std::move(h);
    }
    // the pinned table of the entry publish_frames records below: settled, so its copy of 32 calls ago has been consumed
    HIPCHK(c, c->up_ring.settle_next());
    FrameDesc *T = c->h_dtab + (size_t)(c->up_ring.next % ring) * c->n_fslots;
    const bool yuv = fmt == FFL_DEV_I420 || fmt == FFL_DEV_NV12;
    for (int i = 0; i < n; i++) {
        const ffl_dev_frame &f = frames[i];
        FrameDesc &d = T[i];
        d = FrameDesc();
        d.p0 = (const uint8_t *)f.plane[0];
        d.pitch0 = f.pitch[0];
        d.ps = f.pixel_stride;
        d.cs = f.channel_stride;
        d.c_step = es;
        if (fmt == FFL_DEV_I420) {
            d.p1 = (const uint8_t *)f.plane[1]; d.pitch1 = f.pitch[1];
            d.p2 = (const uint8_t *)f.plane[2]; d.pitch2 = f.pitch[2];
        } else if (fmt == FFL_DEV_NV12) {
            d.p1 = (const uint8_t *)f.plane[1]; d.pitch1 = f.pitch[1];
            d.p2 = d.p1 + es; d.pitch2 = f.pitch[1];
            d.c_step = 2 * es;
        }
        d.fslot = first + i;
    }
    p.kind = fmt == FFL_DEV_GRAY ? FFL_SRC_GRAY : !yuv ? FFL_SRC_BGR : es == 2 ? FFL_SRC_YUV16 : FFL_SRC_YUV;
    p.rgb = fmt == FFL_DEV_RGB;
    if (es == 2) front_depth(&p, depth, msb);
    // stream `copy` waits for the producer's queued work and for the batches that still read the slots
    WaitOnce wait_copy(c->s_copy);
    if (int rc = caller_join(c, cst, wait_copy)) return rc;
    for (int i = 0; i < n; i++)
        if (int rc = wait_frame_free(c, wait_copy, first + i)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_dtab, T, sizeof(FrameDesc) * n, hipMemcpyHostToDevice, c->s_copy));
    {
        ProfScope ps(c, FFL_K_FRONTEND, c->s_copy);
        if (rp) ffl_launch_frontend_remap_dev(c->d_dtab, n, c->d_gray, c->N, p, *rp, c->s_copy);
        else ffl_launch_frontend_dev(c->d_dtab, n, c->d_gray, c->N, p, c->s_copy);
    }
    HIPCHK(c, hipGetLastError());
    if (int rc = publish_frames(c, first, n)) return rc;
    // the caller's later work (overwriting the sources, the allocator reusing them) runs after the frames have been read
    HIPCHK(c, hipStreamWaitEvent(cst, ev_latest(c->up_ring).get(), 0));
    return FFL_OK;
}

// Device frames -> gray frame slots through ONE k_frontend_dev launch on stream `copy`, ordered after the caller's queued
// work and before the caller's later work (the stream contract of ffl.h): the body of ffl_upload_frames_device (es = 1)
// and ffl_upload_frames_device16 (es = 2 bytes per sample, reduced by rule Y5).  The descriptors travel in the pinned
// table of the up_ring entry the call records (publish_frames), copied to the device table on the same stream.
static int upload_device(ffl_ctx *c, const char *fn, int first, int n, const ffl_dev_frame *frames, int fmt, int es, int depth,
                         int msb, int sw, int sh, int rw, int rh, int cx, int cy, uint64_t stream, const ffl_source_info *si) {
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> ul(c->up_mu);
    CtxLock lk(c->mu);
    if (int rc = check_frame_run(c, fn, first, n, frames)) return rc;
    FrontParams p;
    for (int i = 0; i < n; i++)
        if (int rc = dev_frame_check(c, fn, i, fmt, es, depth, sw, sh, &frames[i], si, rw, rh, cx, cy, c->w, c->h, &p)) return rc;
    return send_device(c, fn, first, n, frames, fmt, es, depth, msb, sw, sh, stream, p, nullptr);
}

int ffl_upload_frames_device(ffl_ctx *c, int first, int n, const ffl_dev_frame *frames, int fmt, int sw, int sh, int rw, int rh,
                             int cx, int cy, uint64_t stream) {
    return upload_device(c, "ffl_upload_frames_device", first, n, frames, fmt, 1, 8, 0, sw, sh, rw, rh, cx, cy, stream, nullptr);
}

int ffl_upload_frames_device_src(ffl_ctx *c, int first, int n, const ffl_dev_frame *frames, int fmt, int sw, int sh, int rw, int rh,
                                 int cx, int cy, uint64_t stream, const ffl_source_info *si) {
    return upload_device(c, "ffl_upload_frames_device", first, n, frames, fmt, 1, 8, 0, sw, sh, rw, rh, cx, cy, stream, si);
}

int ffl_upload_frames_device16(ffl_ctx *c, int first, int n, const ffl_dev_frame *frames, int fmt, int depth, int msb_aligned,
                               int sw, int sh, int rw, int rh, int cx, int cy, uint64_t stream) {
    return upload_device(c, "ffl_upload_frames_device16", first, n, frames, fmt, 2, depth, msb_aligned != 0, sw, sh, rw, rh, cx, cy,
                         stream, nullptr);
}

int ffl_upload_frames_device16_src(ffl_ctx *c, int first, int n, const ffl_dev_frame *frames, int fmt, int depth, int msb_aligned,
                                   int sw, int sh, int rw, int rh, int cx, int cy, uint64_t stream, const ffl_source_info *si) {
    return upload_device(c, "ffl_upload_frames_device16", first, n, frames, fmt, 2, depth, msb_aligned != 0, sw, sh, rw, rh, cx, cy,
                         stream, si);
}

// ---- map-driven reprojection --------------------------------------------------------
static int remap_log2(int ss) { return ss == 1 ? 0 : ss == 2 ? 1 : ss == 4 ? 2 : -1; }

// Rule R1 for a map of an upright uw x uh source, and the upright bounding box of its taps (rule R6's first half).
static int remap_scan(ffl_ctx *c, const char *fn, const int32_t *map, int ow, int oh, int ss, int uw, int uh, int ux[2], int uy[2],
                      size_t *valid) {
    if (!map) return set_err(c, FFL_ERR_INVALID, "%s: NULL map", fn);
    if (remap_log2(ss) < 0) return set_err(c, FFL_ERR_INVALID, "%s: supersample %d is not one of 1, 2, 4", fn, ss);
    if (ow < 1 || oh < 1 || ow > 32768 || oh > 32768 || uw < 1 || uh < 1 || uw > 32768 || uh > 32768)
        return set_err(c, FFL_ERR_INVALID, "%s: unsupported output %dx%d / source %dx%d", fn, ow, oh, uw, uh);
    const size_t W = (size_t)ss * ow, H = (size_t)ss * oh;
    const int qxmax = 32 * (uw - 1), qymax = 32 * (uh - 1);
    int x0 = INT32_MAX, x1 = -1, y0 = INT32_MAX, y1 = -1;
    size_t nv = 0;
    for (size_t k = 0; k < W * H; k++) {
        const int qx = map[2 * k], qy = map[2 * k + 1];
        if (qx == FFL_REMAP_NO_SOURCE) continue;
        if (qx < 0 || qx > qxmax || qy < 0 || qy > qymax)
            return set_err(c, FFL_ERR_INVALID, "%s: map entry %zu (sample row %zu, column %zu) is (%d, %d), outside 0..%d x 0..%d "
                                               "(1/32 px of the upright %dx%d source; rule R1)", fn, k, k / W, k % W, qx, qy, qxmax,
                           qymax, uw, uh);
        x0 = std::min(x0, qx); x1 = std::max(x1, qx);
        y0 = std::min(y0, qy); y1 = std::max(y1, qy);
        nv++;
    }
    if (!nv) return set_err(c, FFL_ERR_INVALID, "%s: the map has no valid entry (every sample is FFL_REMAP_NO_SOURCE; rule R1)", fn);
    ux[0] = x0 >> 5; ux[1] = std::min((x1 >> 5) + 1, uw - 1);   // rule R2: the second tap is loaded whatever its weight
    uy[0] = y0 >> 5; uy[1] = std::min((y1 >> 5) + 1, uh - 1);
    if (valid) *valid = nv;
    return FFL_OK;
}

int ffl_remap_check(const int32_t *map, int ow, int oh, int ss, int sw, int sh, const ffl_source_info *si, int win_upright[4],
                    int win_stored[4], size_t *valid) {
    static const char *fn = "ffl_remap_check";
    FrontParams p;
    if (sw < 1 || sh < 1 || sw > 32768 || sh > 32768)
        return set_err(nullptr, FFL_ERR_INVALID, "%s: unsupported source %dx%d", fn, sw, sh);
    if (int rc = front_source(nullptr, fn, FRONT_YUV, sw, sh, si, &p)) return rc;  // full_range: the format is not known here
    int ux[2], uy[2];
    if (int rc = remap_scan(nullptr, fn, map, ow, oh, ss, p.sw, p.sh, ux, uy, valid)) return rc;
    if (win_upright) {
        win_upright[0] = ux[0]; win_upright[1] = uy[0]; win_upright[2] = ux[1] - ux[0] + 1; win_upright[3] = uy[1] - uy[0] + 1;
    }
    if (win_stored) {
        YuvWin yw;
        yuv_stored_window(p, sw, sh, ux, uy, &yw);
        win_stored[0] = yw.x0; win_stored[1] = yw.y0; win_stored[2] = yw.w; win_stored[3] = yw.h;
    }
    return FFL_OK;
}

int ffl_remap_bytes(int ow, int oh, int ss, size_t *bytes) {
    if (remap_log2(ss) < 0 || ow < 1 || oh < 1 || ow > 32768 || oh > 32768 || !bytes)
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_remap_bytes: bad arguments (supersample is one of 1, 2, 4)");
    *bytes = (size_t)8 * ss * ss * ow * oh;
    return FFL_OK;
}

// Nothing of a create but the table entry needs the context's locks: the scan (rule R1) and the copy to the device run
// without them, so that a large map does not hold up the other entry points.  A failure there is worded into the calling
// thread's buffer and becomes the context's message under the lock.
static int remap_fail(ffl_ctx *c, int rc) {
    const std::string msg = g_create_error;
    CtxLock lk(c->mu);
    return set_err(c, rc, "%s", msg.c_str());
}
static int remap_free_entry(const ffl_ctx *c) {
    int k = 0;
    while (k < FFL_MAX_REMAPS && c->remaps[k].d) k++;
    return k;
}

int ffl_remap_create(ffl_ctx *c, const int32_t *map, int ss, int sw, int sh, int *id) {
    static const char *fn = "ffl_remap_create";
    static const char *full = "%s: %d maps are alive already (FFL_MAX_REMAPS); destroy one first";
    if (!c) return FFL_ERR_INVALID;
    if (!id) return remap_fail(c, set_err(nullptr, FFL_ERR_INVALID, "%s: NULL id", fn));
    int ux[2], uy[2];
    if (int rc = remap_scan(nullptr, fn, map, c->w, c->h, ss, sw, sh, ux, uy, nullptr)) return remap_fail(c, rc);  // w, h never change
    {
        CtxLock lk(c->mu);  // a ninth map is refused before any device work
        if (remap_free_entry(c) == FFL_MAX_REMAPS) return set_err(c, FFL_ERR_INVALID, full, fn, FFL_MAX_REMAPS);
    }
    const size_t count = (size_t)ss * ss * c->N;
    DevBuf<int2> d;
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = d.alloc(count);
    if (e == hipSuccess) e = hipMemcpy(d, map, count * sizeof(int2), hipMemcpyHostToDevice);  // resident once this returns
    if (e != hipSuccess)
        return remap_fail(c, set_err(nullptr, FFL_ERR_HIP, "%s: copying the map to the device failed: %s", fn, hipGetErrorString(e)));
    std::unique_lock<std::mutex> ul(c->up_mu);
    CtxLock lk(c->mu);
    const int k = remap_free_entry(c);
    if (k == FFL_MAX_REMAPS) return set_err(c, FFL_ERR_INVALID, full, fn, FFL_MAX_REMAPS);  // another thread took the last entry
    ffl_ctx::Remap &m = c->remaps[k];
    m.d = std::move(d);
    m.ss = ss; m.sw = sw; m.sh = sh;
    m.ux[0] = ux[0]; m.ux[1] = ux[1]; m.uy[0] = uy[0]; m.uy[1] = uy[1];
    m.last = EvRef();
    *id = k;
    return FFL_OK;
}

// The end of an upload call that named map `id`: the event ffl_remap_destroy waits for.  A call that succeeded has just
// recorded it (publish_frames).  One that failed part-way may have queued launches that read the map and published
// nothing, so an event of its own is recorded behind them on stream `copy`; if even that fails the stream is drained.
static void remap_used(ffl_ctx *c, int id, int rc) {
    if (!c->remaps[id].d) return;
    if (rc == FFL_OK) {
        c->remaps[id].last = ev_latest(c->up_ring);
        return;
    }
    EvRef ev;
    if (c->up_ring.record(c->s_copy, &ev) == hipSuccess) c->remaps[id].last = ev;
    else (void)hipStreamSynchronize(c->s_copy);
}

// the map an upload call names, checked against the call's upright source size (fp->sw x fp->sh)
static int remap_open(ffl_ctx *c, const char *fn, int id, const FrontParams &fp, ffl_ctx::Remap **m, RemapParams *rp) {
    if (id < 0 || id >= FFL_MAX_REMAPS || !c->remaps[id].d)
        return set_err(c, FFL_ERR_INVALID, "%s: remap id %d names no map (never created, or destroyed)", fn, id);
    *m = &c->remaps[id];
    if ((*m)->sw != fp.sw || (*m)->sh != fp.sh)
        return set_err(c, FFL_ERR_INVALID, "%s: the upright source is %dx%d, map %d was created for %dx%d", fn, fp.sw, fp.sh, id,
                       (*m)->sw, (*m)->sh);
    rp->map = (*m)->d;
    rp->ss = (*m)->ss;
    rp->lg = remap_log2((*m)->ss);
    return FFL_OK;
}

int ffl_remap_destroy(ffl_ctx *c, int id) {
    static const char *fn = "ffl_remap_destroy";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> ul(c->up_mu);  // no upload call can start using the map meanwhile
    CtxLock lk(c->mu);
    if (id < 0 || id >= FFL_MAX_REMAPS || !c->remaps[id].d)
        return set_err(c, FFL_ERR_INVALID, "%s: remap id %d names no map (never created, or destroyed)", fn, id);
    hipEvent_t ev = c->remaps[id].last.get();  // the last launch that reads it; nullptr: long over
    if (int rc = wait_unlocked(c, lk, &ev, 1)) return rc;
    HIPCHK(c, c->remaps[id].d.reset());
    c->remaps[id] = ffl_ctx::Remap();
    return FFL_OK;
}

int ffl_upload_frames_remap(ffl_ctx *c, int first, int n, const uint8_t *const *frames, int fmt, int sw, int sh,
                            ptrdiff_t stride_bytes, int depth, int msb, int id, const ffl_source_info *si) {
    static const char *fn = "ffl_upload_frames_remap";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> ul(c->up_mu);
    CtxLock lk(c->mu);
    if (int rc = check_frame_run(c, fn, first, n, frames, frames)) return rc;
    if (fmt < FFL_DEV_BGR || fmt > FFL_DEV_NV12)
        return set_err(c, FFL_ERR_INVALID, "%s: format %d is not one of FFL_DEV_BGR 1, RGB 2, I420 3, NV12 4 (host gray frames have "
                                           "no map path)", fn, fmt);
    const bool yuv = fmt == FFL_DEV_I420 || fmt == FFL_DEV_NV12;
    if (depth != 8 && !yuv)
        return set_err(c, FFL_ERR_INVALID, "%s: depth %d: 3-channel frames are 8-bit (9..16 describe 4:2:0 frames)", fn, depth);
    // both depths are this call's own: refused here, so that the depth texts of the shared rules below, which send a caller
    // to the 8-bit entry points, are never reached from it
    if (yuv && depth != 8 && (depth < 9 || depth > 16))
        return set_err(c, FFL_ERR_INVALID, "%s: depth %d is neither 8 nor 9..16", fn, depth);
    if (sw < 1 || sh < 1 || sw > 32768 || sh > 32768) return set_err(c, FFL_ERR_INVALID, "%s: unsupported source %dx%d", fn, sw, sh);
    const int es = depth == 8 ? 1 : 2, layout = fmt == FFL_DEV_NV12 ? FFL_YUV_NV12 : FFL_YUV_I420;
    if (yuv)
        if (int rc = yuv_layout_rules(c, fn, sw, sh, layout, stride_bytes, es, depth)) return rc;
    FrontParams fp = {};
    if (int rc = front_source(c, fn, yuv ? FRONT_YUV : FRONT_BGR, sw, sh, si, &fp)) return rc;
    fp.ow = c->w; fp.oh = c->h;
    ffl_ctx::Remap *m;
    RemapParams rp;
    if (int rc = remap_open(c, fn, id, fp, &m, &rp)) return rc;
    int rc;
    if (yuv) {
        YuvWin yw;  // rule R6
        yuv_stored_window(fp, sw, sh, m->ux, m->uy, &yw);
        rc = send_yuv(c, lk, fn, first, n, frames, sw, sh, stride_bytes, layout, es, depth, msb != 0, fp, yw, &rp);
    } else {
        rc = send_raw(c, lk, fn, first, n, frames, sw, sh, stride_bytes, fmt == FFL_DEV_RGB, fp, &rp);
    }
    remap_used(c, id, rc);
    return rc;
}

int ffl_upload_frames_device_remap(ffl_ctx *c, int first, int n, const ffl_dev_frame *frames, int fmt, int depth, int msb, int sw,
                                   int sh, int id, uint64_t stream, const ffl_source_info *si) {
    static const char *fn = "ffl_upload_frames_device_remap";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> ul(c->up_mu);
    CtxLock lk(c->mu);
    if (int rc = check_frame_run(c, fn, first, n, frames)) return rc;
    // as in ffl_upload_frames_remap: the shared rules' depth texts name other entry points and are never reached from here
    if (depth != 8 && (depth < 9 || depth > 16)) return set_err(c, FFL_ERR_INVALID, "%s: depth %d is neither 8 nor 9..16", fn, depth);
    if (sw < 1 || sh < 1 || sw > 32768 || sh > 32768) return set_err(c, FFL_ERR_INVALID, "%s: unsupported source %dx%d", fn, sw, sh);
    const int es = depth == 8 ? 1 : 2;
    FrontParams p = {};
    for (int i = 0; i < n; i++) {
        if (int rc = dev_format_rules(c, fn, i, fmt, es, depth, sw, sh, &frames[i])) return rc;
        if (i == 0)
            if (int rc = front_source(c, fn, dev_front_class(fmt), sw, sh, si, &p)) return rc;
        if (int rc = dev_plane_rules(c, fn, i, fmt, es, sw, sh, &frames[i])) return rc;
    }
    p.ow = c->w; p.oh = c->h;
    ffl_ctx::Remap *m;
    RemapParams rp;
    if (int rc = remap_open(c, fn, id, p, &m, &rp)) return rc;
    const int rc = send_device(c, fn, first, n, frames, fmt, es, depth, msb != 0, sw, sh, stream, p, &rp);
    remap_used(c, id, rc);
    return rc;
}

// Flow slots -> caller device memory on stream `post`, ordered after the batches that produced them and the caller's
// queued work, and before the caller's later work; the export becomes the slots' last use.
int ffl_export_flows(ffl_ctx *c, int n, const int *slots, float *dst, int layout, ptrdiff_t item_stride, uint64_t stream) {
    static const char *fn = "ffl_export_flows";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post` and post_ring, as ffl_radial / ffl_upload_flow
    CtxLock lk(c->mu);
    if (n < 1 || !slots || !dst) return set_err(c, FFL_ERR_INVALID, "%s: bad arguments", fn);
    if (layout != FFL_FLOW_NHWC && layout != FFL_FLOW_NCHW)
        return set_err(c, FFL_ERR_INVALID, "%s: unknown layout %d (FFL_FLOW_NHWC 0, FFL_FLOW_NCHW 1)", fn, layout);
    const size_t item = sizeof(float) * 2 * c->N;
    if ((uintptr_t)dst % 4 || item_stride % 4)
        return set_err(c, FFL_ERR_INVALID, "%s: dst and the item stride (%td) must be multiples of 4 bytes", fn, item_stride);
    if (n > 1 && (size_t)(item_stride < 0 ? -item_stride : item_stride) < item)
        return set_err(c, FFL_ERR_INVALID, "%s: item stride %td is smaller than one flow field (%zu bytes)", fn, item_stride, item);
    if (int rc = check_flow_slots(c, fn, n, slots, "flow", nullptr)) return rc;
    hipStream_t cst;
    const ptrdiff_t span = (ptrdiff_t)(n - 1) * item_stride;
    const char *lo = (const char *)dst + (span < 0 ? span : 0);
    const PostRegion reg{"dst", lo, (size_t)(span < 0 ? -span : span) + item, kHostFrames};
    if (int rc = post_begin(c, fn, stream, &cst, &reg, 1, n, slots)) return rc;
    for (int i0 = 0; i0 < n; i0 += FFL_MAXB) {
        const int m = n - i0 < FFL_MAXB ? n - i0 : FFL_MAXB;
        ExportTab t;
        for (int i = 0; i < m; i++) t.slot[i] = slots[i0 + i];
        ffl_launch_export_flows(c->d_flow, t, m, c->N, (char *)dst + (ptrdiff_t)i0 * item_stride, item_stride, layout, c->s_post);
    }
    return post_end(c, cst, n, slots);
}

// The centre window, the cut test and pass 2 of items first .. first+n-1 of seq on stream `post`, ordered after the
// producers of every seq slot and the caller's queued work, and before the caller's later work (the stream contract of
// ffl.h).  The slot table travels as a kernel argument; the plan kernel's item table and the radial partials are single
// device copies, safe because every user of them runs on stream `post`.  Nothing waits on the host beyond post_ring's own
// settling.
static_assert(sizeof(ffl_pass2_record) == 48 && sizeof(Pass2Record) == 48 && offsetof(ffl_pass2_record, cx) == offsetof(Pass2Record, cx) &&
              offsetof(ffl_pass2_record, mean_mag) == offsetof(Pass2Record, mean_mag) && offsetof(ffl_pass2_record, x) == offsetof(Pass2Record, x) &&
              offsetof(ffl_pass2_record, cut) == offsetof(Pass2Record, cut), "Pass2Record mirrors ffl_pass2_record");
static_assert(FFL_MAX_RADIUS == FFL_WINDOW_MAX_RADIUS && FFL_MAX_BATCH == FFL_MAXB, "ffl.h and ffl_kernels.h agree");
static_assert(sizeof(ffl_axes_record) == 80 && sizeof(AxesRecord) == 80 && offsetof(ffl_axes_record, base) == 0 &&
              offsetof(AxesRecord, base) == 0 && offsetof(ffl_axes_record, tangential) == 48 &&
              offsetof(ffl_axes_record, tangential) == offsetof(AxesRecord, tangential) &&
              offsetof(ffl_axes_record, shift_x) == offsetof(AxesRecord, shift_x) &&
              offsetof(ffl_axes_record, shift_y) == offsetof(AxesRecord, shift_y) &&
              offsetof(ffl_axes_record, reserved) == offsetof(AxesRecord, reserved) && alignof(ffl_axes_record) == 8,
              "AxesRecord mirrors ffl_axes_record");
static_assert(FFL_N_AXES == FFL_NAXES && FFL_AXIS_RADIAL == 0 && FFL_AXIS_TANGENTIAL == 1 && FFL_AXIS_SHIFT_X == 2 &&
              FFL_AXIS_SHIFT_Y == 3, "ffl.h and ffl_kernels.h agree on the components");
// ---- weight maps --------------------------------------------------------------------
// Every geometry rule of a weight descriptor (ffl.h, ffl_dev_weights_check).  *bytes: the extent of all n maps from w->base.
static int dev_weights_check(ffl_ctx *c, const char *fn, int n, int width, int height, const ffl_dev_weights *w, size_t *bytes) {
    if (!w) return set_err(c, FFL_ERR_INVALID, "%s: NULL weight descriptor", fn);
    if (!w->base) return set_err(c, FFL_ERR_INVALID, "%s: NULL weight base", fn);
    if (n < 1) return set_err(c, FFL_ERR_INVALID, "%s: n = %d weight maps (>= 1)", fn, n);
    if (width < 2 || height < 2 || width > 32768 || height > 32768)
        return set_err(c, FFL_ERR_INVALID, "%s: weight map size %dx%d outside 2..32768", fn, width, height);
    const ptrdiff_t it = w->item_stride, pitch = w->row_pitch, big = (ptrdiff_t)1 << 40;
    if (it < 0 || pitch < 0) return set_err(c, FFL_ERR_INVALID, "%s: negative weight stride (item %td, row %td)", fn, it, pitch);
    if (it > big || pitch > big) return set_err(c, FFL_ERR_INVALID, "%s: weight stride beyond 2^40", fn);
    if (pitch < width) return set_err(c, FFL_ERR_INVALID, "%s: overlap: weight row pitch %td below the width %d", fn, pitch, width);
    const ptrdiff_t map = (ptrdiff_t)(height - 1) * pitch + width;
    if (it > 0 && it < map)
        return set_err(c, FFL_ERR_INVALID, "%s: overlap: weight item stride %td below one map's extent %td (0: one map for all items)",
                       fn, it, map);
    *bytes = (size_t)(n - 1) * (size_t)it + (size_t)map;
    return FFL_OK;
}

int ffl_dev_weights_check(int n, int width, int height, const ffl_dev_weights *w) {
    size_t bytes;
    return dev_weights_check(nullptr, "ffl_dev_weights_check", n, width, height, w, &bytes);
}

static const char *kHostWeights = "weight maps live in device memory (torch / hipMalloc)";

// The pass-1 records of n slots that hold a flow, recomputed under the maps by ONE k_pass1_weighted launch (plus its final
// kernel) on stream `post`: ffl_import_flows' protocol, with the flow only read.
int ffl_pass1_weighted(ffl_ctx *c, int n, const int *slots, const ffl_dev_weights *w, int pov_mode, uint64_t stream) {
    static const char *fn = "ffl_pass1_weighted";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post`, d_ptab and the partials, as ffl_import_flows
    CtxLock lk(c->mu);
    ExportTab t;
    if (int rc = open_slot_list(c, fn, "slots", n, slots, "flow", &t)) return rc;
    size_t bytes;
    if (int rc = dev_weights_check(c, fn, n, c->w, c->h, w, &bytes)) return rc;
    hipStream_t cst;
    const PostRegion reg{"the weight maps", w->base, bytes, kHostWeights};
    if (int rc = post_begin(c, fn, stream, &cst, &reg, 1, n, slots)) return rc;
    if (int rc = post_scratch(c, fn, SCR_WEIGHTS)) return rc;
    const WeightArgs wa{(const char *)w->base, (long long)w->item_stride, (long long)w->row_pitch};
    {
        ProfScope ps(c, FFL_K_PASS1, c->s_post);
        ffl_launch_pass1_weighted(wa, c->d_flow, c->d_res, t, n, c->w, c->h, pov_mode ? 1 : 0, c->d_ptab, c->d_pskey, c->d_rpsum,
                                  c->d_wpsum, c->s_post);
    }
    return post_end(c, cst, n, slots);  // the caller may overwrite or free the maps straight after the call
}

// ---- forward-backward consistency maps ----------------------------------------------
int ffl_consistency_default_params(ffl_consistency_params *out) {
    if (!out) return FFL_ERR_INVALID;
    *out = ffl_consistency_params{0.01f, 0.5f, 1};
    return FFL_OK;
}

// The accepted parameters of appendix K.  The comparisons are written so that a NaN fails them.
static int consistency_params_check(ffl_ctx *c, const char *fn, const ffl_consistency_params *p) {
    if (!p) return set_err(c, FFL_ERR_INVALID, "%s: NULL parameters", fn);
    if (!(p->alpha >= 0.0f && p->alpha <= 1.0f))
        return set_err(c, FFL_ERR_INVALID, "%s: alpha = %g outside 0..1 (finite)", fn, (double)p->alpha);
    if (!(p->beta > 0.0f && p->beta <= 1e6f))
        return set_err(c, FFL_ERR_INVALID, "%s: beta = %g outside 0 < beta <= 1e6 (finite)", fn, (double)p->beta);
    if (p->soft != 0 && p->soft != 1) return set_err(c, FFL_ERR_INVALID, "%s: soft = %d is neither 0 (hard) nor 1 (soft)", fn, p->soft);
    return FFL_OK;
}

int ffl_consistency_params_check(const ffl_consistency_params *p) {
    return consistency_params_check(nullptr, "ffl_consistency_params_check", p);
}

// n maps from n forward and n backward fields by ONE k_consistency launch on stream `post`: ffl_pass1_weighted's protocol
// over all 2n slots, with the flows and their records only read.
int ffl_consistency_weights(ffl_ctx *c, int n, const int *fwd_slots, const int *bwd_slots, const ffl_consistency_params *p,
                            const ffl_dev_weights *gate, const ffl_dev_weights *out, uint64_t stream) {
    static const char *fn = "ffl_consistency_weights";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post`, as ffl_pass1_weighted
    CtxLock lk(c->mu);
    if (n < 1 || n > c->max_batch)
        return set_err(c, FFL_ERR_INVALID, "%s: n = %d items outside 1..%d (the context's max_batch)", fn, n, c->max_batch);
    if (!fwd_slots || !bwd_slots) return set_err(c, FFL_ERR_INVALID, "%s: NULL %s", fn, !fwd_slots ? "fwd_slots" : "bwd_slots");
    int all[2 * FFL_MAXB];   // the forward slots, then the backward ones: what the call uses
    ExportTab tf, tb;
    for (int i = 0; i < n; i++) {
        all[i] = tf.slot[i] = fwd_slots[i];
        all[n + i] = tb.slot[i] = bwd_slots[i];
    }
    if (int rc = check_flow_slots(c, fn, 2 * n, all, "flow", "repeated among the forward and backward slots of one call")) return rc;
    ffl_consistency_params prm;
    ffl_consistency_default_params(&prm);
    if (p) prm = *p;
    if (int rc = consistency_params_check(c, fn, &prm)) return rc;
    size_t obytes, gbytes = 0;
    if (!out) return set_err(c, FFL_ERR_INVALID, "%s: NULL out descriptor", fn);
    if (int rc = dev_weights_check(c, fn, n, c->w, c->h, out, &obytes)) return rc;
    if (n > 1 && out->item_stride == 0)
        return set_err(c, FFL_ERR_INVALID, "%s: overlap: out item stride 0 with n = %d maps to write (one map per item)", fn, n);
    if (gate) {
        if (int rc = dev_weights_check(c, fn, n, c->w, c->h, gate, &gbytes)) return rc;
        const uintptr_t o0 = (uintptr_t)out->base, g0 = (uintptr_t)gate->base;
        if (o0 < g0 + gbytes && g0 < o0 + obytes)
            return set_err(c, FFL_ERR_INVALID, "%s: overlap: out (%zu bytes) and gate (%zu bytes) share memory", fn, obytes, gbytes);
    }
    hipStream_t cst;
    PostRegion reg[2] = {{"out", out->base, obytes, kHostWeights}, {"the gate maps", gate ? gate->base : nullptr, gbytes, kHostWeights}};
    if (int rc = post_begin(c, fn, stream, &cst, reg, gate ? 2 : 1, 2 * n, all)) return rc;
    WeightArgs ga;
    if (gate) ga = WeightArgs{(const char *)gate->base, (long long)gate->item_stride, (long long)gate->row_pitch};
    ffl_launch_consistency(c->d_flow, tf, tb, n, c->w, c->h, prm.alpha, prm.beta, prm.soft, gate ? &ga : nullptr, (char *)out->base,
                           (long long)out->item_stride, (long long)out->row_pitch, c->s_post);
    return post_end(c, cst, 2 * n, all);  // the caller may read the maps, or overwrite the gate, on `stream` straight after the call
}

// ---- photometric-residual maps -------------------------------------------------------
int ffl_residual_default_params(ffl_residual_params *out) {
    if (!out) return FFL_ERR_INVALID;
    *out = ffl_residual_params{0.5f, 4.0f, 1};   // the project's own choice, not tuned on footage
    return FFL_OK;
}

// The accepted parameters of appendix P.  The comparisons are written so that a NaN fails them.
static int residual_params_check(ffl_ctx *c, const char *fn, const ffl_residual_params *p) {
    if (!p) return set_err(c, FFL_ERR_INVALID, "%s: NULL parameters", fn);
    if (!(p->alpha >= 0.0f && p->alpha <= 16.0f))
        return set_err(c, FFL_ERR_INVALID, "%s: alpha = %g outside 0..16 (finite)", fn, (double)p->alpha);
    if (!(p->beta > 0.0f && p->beta <= 255.0f))
        return set_err(c, FFL_ERR_INVALID, "%s: beta = %g outside 0 < beta <= 255 (finite)", fn, (double)p->beta);
    if (p->soft != 0 && p->soft != 1) return set_err(c, FFL_ERR_INVALID, "%s: soft = %d is neither 0 (hard) nor 1 (soft)", fn, p->soft);
    return FFL_OK;
}

int ffl_residual_params_check(const ffl_residual_params *p) {
    return residual_params_check(nullptr, "ffl_residual_params_check", p);
}

// n maps from n pairs of frames and their forward fields by ONE k_residual launch on stream `post`: ffl_consistency_weights'
// protocol over the n flow slots, and a reader's protocol over the frame slots -- stream `post` waits for the uploads that
// filled them (ev_uploaded, as a batch does), and the call's event becomes their last reader on stream `post` (ev_last_use's
// last column), which every later upload into one of them waits for (wait_frame_free).  An upload looks that column up under
// the context lock right before it queues its transfer, and this call holds the lock from its waits to its event, so the two
// cannot interleave.
int ffl_residual_weights(ffl_ctx *c, int n, const int *fslot0, const int *fslot1, const int *flow_slots, const ffl_residual_params *p,
                         const ffl_dev_weights *gate, const ffl_dev_weights *out, uint64_t stream) {
    static const char *fn = "ffl_residual_weights";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post`, as ffl_consistency_weights
    CtxLock lk(c->mu);
    if (n < 1 || n > c->max_batch)
        return set_err(c, FFL_ERR_INVALID, "%s: n = %d items outside 1..%d (the context's max_batch)", fn, n, c->max_batch);
    if (!fslot0 || !fslot1 || !flow_slots)
        return set_err(c, FFL_ERR_INVALID, "%s: NULL %s", fn, !fslot0 ? "fslot0" : !fslot1 ? "fslot1" : "flow_slots");
    ExportTab t0, t1, tf;
    for (int i = 0; i < n; i++) {
        for (int fs : {fslot0[i], fslot1[i]}) {   // frame slots may repeat between items
            if (fs < 0 || fs >= c->n_fslots) return set_err(c, FFL_ERR_INVALID, "%s: item %d: frame slot %d out of range", fn, i, fs);
            if (!c->frame_valid[fs]) return set_err(c, FFL_ERR_STATE, "%s: item %d: frame slot %d was never uploaded", fn, i, fs);
        }
        t0.slot[i] = fslot0[i];
        t1.slot[i] = fslot1[i];
        tf.slot[i] = flow_slots[i];
    }
    if (int rc = check_flow_slots(c, fn, n, flow_slots, "flow", "repeated among the flow slots of one call")) return rc;
    ffl_residual_params prm;
    ffl_residual_default_params(&prm);
    if (p) prm = *p;
    if (int rc = residual_params_check(c, fn, &prm)) return rc;
    size_t obytes, gbytes = 0;
    if (!out) return set_err(c, FFL_ERR_INVALID, "%s: NULL out descriptor", fn);
    if (int rc = dev_weights_check(c, fn, n, c->w, c->h, out, &obytes)) return rc;
    if (n > 1 && out->item_stride == 0)
        return set_err(c, FFL_ERR_INVALID, "%s: overlap: out item stride 0 with n = %d maps to write (one map per item)", fn, n);
    if (gate) {
        if (int rc = dev_weights_check(c, fn, n, c->w, c->h, gate, &gbytes)) return rc;
        const uintptr_t o0 = (uintptr_t)out->base, g0 = (uintptr_t)gate->base;
        if (o0 < g0 + gbytes && g0 < o0 + obytes)
            return set_err(c, FFL_ERR_INVALID, "%s: overlap: out (%zu bytes) and gate (%zu bytes) share memory", fn, obytes, gbytes);
    }
    hipStream_t cst;
    PostRegion reg[2] = {{"out", out->base, obytes, kHostWeights}, {"the gate maps", gate ? gate->base : nullptr, gbytes, kHostWeights}};
    if (int rc = post_begin(c, fn, stream, &cst, reg, gate ? 2 : 1, n, flow_slots)) return rc;
    {
        WaitOnce wait_post(c->s_post);   // the frames: a run of slots shares one or two upload events
        for (int i = 0; i < n; i++) {
            HIPCHK(c, wait_post(c->ev_uploaded[fslot0[i]].get()));
            HIPCHK(c, wait_post(c->ev_uploaded[fslot1[i]].get()));
        }
    }
    WeightArgs ga;
    if (gate) ga = WeightArgs{(const char *)gate->base, (long long)gate->item_stride, (long long)gate->row_pitch};
    ffl_launch_residual(c->d_gray, c->d_flow, t0, t1, tf, n, c->w, c->h, prm.alpha, prm.beta, prm.soft, gate ? &ga : nullptr,
                        (char *)out->base, (long long)out->item_stride, (long long)out->row_pitch, c->s_post);
    // the caller may read the maps, or overwrite the gate, on `stream` straight after the call
    return post_end_frames(c, cst, n, flow_slots, n, fslot0, fslot1);
}

// ---- texture (structure-tensor) maps --------------------------------------------------
int ffl_texture_default_params(ffl_texture_params *out) {
    if (!out) return FFL_ERR_INVALID;
    *out = ffl_texture_params{7, 16.0f, 1};   // the project's own choice, not tuned on footage
    return FFL_OK;
}

// The accepted parameters of appendix T.  The comparisons are written so that a NaN fails them.
static int texture_params_check(ffl_ctx *c, const char *fn, const ffl_texture_params *p) {
    if (!p) return set_err(c, FFL_ERR_INVALID, "%s: NULL parameters", fn);
    if (p->radius < 1 || p->radius > 8) return set_err(c, FFL_ERR_INVALID, "%s: radius = %d outside 1..8", fn, p->radius);
    if (!(p->tau > 0.0f && p->tau <= 65025.0f))
        return set_err(c, FFL_ERR_INVALID, "%s: tau = %g outside 0 < tau <= 65025 (finite)", fn, (double)p->tau);
    if (p->soft != 0 && p->soft != 1) return set_err(c, FFL_ERR_INVALID, "%s: soft = %d is neither 0 (hard) nor 1 (soft)", fn, p->soft);
    return FFL_OK;
}

int ffl_texture_params_check(const ffl_texture_params *p) {
    return texture_params_check(nullptr, "ffl_texture_params_check", p);
}

// n maps from n frames by ONE k_texture launch on stream `post`: ffl_residual_weights' protocol without the flow slots -- stream
// `post` runs behind the caller's queued work and the uploads that filled the frame slots, and the call's event becomes their
// last reader on stream `post`.  gate may be exactly out (same base, item stride and row pitch): the in-place form, in which
// the lane that owns a pixel reads its gate byte and then writes it.
int ffl_texture_weights(ffl_ctx *c, int n, const int *fslots, const ffl_texture_params *p, const ffl_dev_weights *gate,
                        const ffl_dev_weights *out, uint64_t stream) {
    static const char *fn = "ffl_texture_weights";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post`, as ffl_residual_weights
    CtxLock lk(c->mu);
    if (n < 1 || n > c->max_batch)
        return set_err(c, FFL_ERR_INVALID, "%s: n = %d items outside 1..%d (the context's max_batch)", fn, n, c->max_batch);
    if (!fslots) return set_err(c, FFL_ERR_INVALID, "%s: NULL fslots", fn);
    ExportTab tf;
    for (int i = 0; i < n; i++) {   // frame slots may repeat between items
        const int fs = fslots[i];
        if (fs < 0 || fs >= c->n_fslots) return set_err(c, FFL_ERR_INVALID, "%s: item %d: frame slot %d out of range", fn, i, fs);
        if (!c->frame_valid[fs]) return set_err(c, FFL_ERR_STATE, "%s: item %d: frame slot %d was never uploaded", fn, i, fs);
        tf.slot[i] = fs;
    }
    ffl_texture_params prm;
    ffl_texture_default_params(&prm);
    if (p) prm = *p;
    if (int rc = texture_params_check(c, fn, &prm)) return rc;
    size_t obytes, gbytes = 0;
    if (!out) return set_err(c, FFL_ERR_INVALID, "%s: NULL out descriptor", fn);
    if (int rc = dev_weights_check(c, fn, n, c->w, c->h, out, &obytes)) return rc;
    if (n > 1 && out->item_stride == 0)
        return set_err(c, FFL_ERR_INVALID, "%s: overlap: out item stride 0 with n = %d maps to write (one map per item)", fn, n);
    bool in_place = false;
    if (gate) {
        if (int rc = dev_weights_check(c, fn, n, c->w, c->h, gate, &gbytes)) return rc;
        in_place = gate->base == out->base && gate->item_stride == out->item_stride && gate->row_pitch == out->row_pitch;
        const uintptr_t o0 = (uintptr_t)out->base, g0 = (uintptr_t)gate->base;
        if (!in_place && o0 < g0 + gbytes && g0 < o0 + obytes)
            return set_err(c, FFL_ERR_INVALID, "%s: overlap: out (%zu bytes) and gate (%zu bytes) share memory, and gate is not "
                                               "exactly out (same base, item stride and row pitch: the in-place form)",
                           fn, obytes, gbytes);
    }
    hipStream_t cst;
    PostRegion reg[2] = {{"out", out->base, obytes, kHostWeights}, {"the gate maps", gate ? gate->base : nullptr, gbytes, kHostWeights}};
    if (int rc = post_begin(c, fn, stream, &cst, reg, gate && !in_place ? 2 : 1, 0, nullptr)) return rc;
    {
        WaitOnce wait_post(c->s_post);   // the frames: a run of slots shares one upload event
        for (int i = 0; i < n; i++) HIPCHK(c, wait_post(c->ev_uploaded[fslots[i]].get()));
    }
    WeightArgs ga;
    if (gate) ga = WeightArgs{(const char *)gate->base, (long long)gate->item_stride, (long long)gate->row_pitch};
    ffl_launch_texture(c->d_gray, tf, n, c->w, c->h, prm.radius, prm.tau, prm.soft, gate ? &ga : nullptr, (char *)out->base,
                       (long long)out->item_stride, (long long)out->row_pitch, c->s_post);
    // the caller may read the maps, or overwrite the gate, on `stream` straight after the call
    return post_end_frames(c, cst, 0, nullptr, n, fslots, nullptr);
}

static const char *kHostCentres ="centres live in device memory (ffl_cell_stats' records, or a float64 (n_seq, 2) tensor)";

// What a window call computes: ffl_radial_window (axes = false: ffl_pass2_record) or one of the four ffl_radial_window_axes*
// (ffl_axes_record).  weighted / centred name the entry point, since a NULL descriptor or NULL centres_dev from the caller
// is refused, not taken for another form.  Either brings one more region of caller memory: the maps of the n computed
// items, or the n_seq centres; ffl_radial_window_axes_weighted_centres sets both.
struct WindowForm {
    bool axes, weighted, centred;
    const ffl_dev_weights *wts;
    const void *cen;
    ptrdiff_t cstride;
};

// One protocol for the five.
static int radial_window_call(ffl_ctx *c, const char *fn, const WindowForm &form, int n_seq, const int *seq, int first, int n,
                              int radius, float cut_threshold, int pov_mode, void *out, uint64_t stream) {
    if (!c) return FFL_ERR_INVALID;
    const size_t rec_bytes = form.axes ? sizeof(ffl_axes_record) : sizeof(ffl_pass2_record);
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post`, post_ring and d_rpsum, as ffl_radial / ffl_export_flows
    CtxLock lk(c->mu);
    if (n < 1 || n > FFL_MAX_BATCH) return set_err(c, FFL_ERR_INVALID, "%s: n = %d items outside 1..%d (FFL_MAX_BATCH)", fn, n, FFL_MAX_BATCH);
    const int max_seq = FFL_MAX_BATCH + 2 * FFL_MAX_RADIUS;
    if (n_seq < 1 || n_seq > max_seq)
        return set_err(c, FFL_ERR_INVALID, "%s: n_seq = %d slots outside 1..%d (FFL_MAX_BATCH + 2 * FFL_MAX_RADIUS)", fn, n_seq, max_seq);
    if (first < 0 || first > n_seq - n)   // n and n_seq are in range: no overflow
        return set_err(c, FFL_ERR_INVALID, "%s: first = %d, n = %d: the items lie outside seq 0..%d", fn, first, n, n_seq - 1);
    if (radius < 0 || radius > FFL_MAX_RADIUS)
        return set_err(c, FFL_ERR_INVALID, "%s: radius %d outside 0..%d (FFL_MAX_RADIUS)", fn, radius, FFL_MAX_RADIUS);
    if (!seq) return set_err(c, FFL_ERR_INVALID, "%s: NULL seq_slots", fn);
    if (!out) return set_err(c, FFL_ERR_INVALID, "%s: NULL out_dev", fn);
    // a slot's state stands for its record and its flow alike, so one check covers the neighbours and the computed items
    if (int rc = check_flow_slots(c, fn, n_seq, seq, "result", "repeated in one call")) return rc;
    if ((uintptr_t)out % 8) return set_err(c, FFL_ERR_INVALID, "%s: out_dev must be 8-byte aligned", fn);
    PostRegion reg[3] = {
        {"out_dev", out, rec_bytes * (size_t)n, "results in host memory come from ffl_pass1_results and ffl_radial"}};
    int nreg = 1;
    const ffl_dev_weights *wts = form.wts;
    if (form.weighted) {
        size_t wbytes;
        if (int rc = dev_weights_check(c, fn, n, c->w, c->h, wts, &wbytes)) return rc;
        reg[nreg++] = PostRegion{"the weight maps", wts->base, wbytes, kHostWeights};
    }
    const void *cen = form.cen;
    const ptrdiff_t cstride = form.cstride;
    if (form.centred) {   // rule G6: n_seq entries, two doubles at the head of each
        if (!cen) return set_err(c, FFL_ERR_INVALID, "%s: NULL centres_dev", fn);
        if ((uintptr_t)cen % 8) return set_err(c, FFL_ERR_INVALID, "%s: centres_dev must be 8-byte aligned", fn);
        if (cstride < 16 || cstride % 8 || cstride > ((ptrdiff_t)1 << 40))
            return set_err(c, FFL_ERR_INVALID, "%s: centre stride %td: a multiple of 8 bytes, at least 16 (two doubles)", fn, cstride);
        reg[nreg++] = PostRegion{"centres_dev", cen, (size_t)(n_seq - 1) * (size_t)cstride + 16, kHostCentres};
    }
    hipStream_t cst;
    if (int rc = post_begin(c, fn, stream, &cst, reg, nreg, n_seq, seq)) return rc;
    WindowSeq t;
    for (int i = 0; i < n_seq; i++) t.slot[i] = seq[i];
    if (form.axes)
        if (int rc = post_scratch(c, fn, form.weighted ? SCR_WEIGHTS : SCR_AXES)) return rc;
    // not timed under FFL_K_RADIAL: that class counts the radial pairs of ffl_radial / ffl_radial_axes, one per call
    ffl_launch_window_plan(t, n_seq, first, n, radius, cut_threshold, c->d_res, c->d_flow, c->w, c->h, cen, (long long)cstride,
                           c->d_wtab, out, (int)rec_bytes, c->s_post);
    WeightArgs wa{};
    if (form.weighted) wa = WeightArgs{(const char *)wts->base, (long long)wts->item_stride, (long long)wts->row_pitch};
    const RadialForm rf{form.axes ? FFL_NAXES : 1, form.weighted ? &wa : nullptr};
    double *psum = form.weighted ? c->d_wpsum : form.axes ? c->d_apsum : c->d_rpsum;
    ffl_launch_radial(c->d_wtab, n, c->w, c->h, pov_mode ? 1 : 0, c->d_wytab, rf, psum, out, c->s_post);
    return post_end(c, cst, n_seq, seq);
}

int ffl_radial_window(ffl_ctx *c, int n_seq, const int *seq, int first, int n, int radius, float cut_threshold, int pov_mode,
                      ffl_pass2_record *out, uint64_t stream) {
    return radial_window_call(c, "ffl_radial_window", {false, false, false, nullptr, nullptr, 0}, n_seq, seq, first, n, radius,
                              cut_threshold, pov_mode, out, stream);
}

int ffl_radial_window_axes(ffl_ctx *c, int n_seq, const int *seq, int first, int n, int radius, float cut_threshold, int pov_mode,
                           ffl_axes_record *out, uint64_t stream) {
    return radial_window_call(c, "ffl_radial_window_axes", {true, false, false, nullptr, nullptr, 0}, n_seq, seq, first, n, radius,
                              cut_threshold, pov_mode, out, stream);
}

int ffl_radial_window_axes_weighted(ffl_ctx *c, int n_seq, const int *seq, int first, int n, int radius, float cut_threshold,
                                    int pov_mode, const ffl_dev_weights *w, ffl_axes_record *out, uint64_t stream) {
    return radial_window_call(c, "ffl_radial_window_axes_weighted", {true, true, false, w, nullptr, 0}, n_seq, seq, first, n,
                              radius, cut_threshold, pov_mode, out, stream);
}

int ffl_radial_window_axes_centres(ffl_ctx *c, int n_seq, const int *seq, int first, int n, int radius, float cut_threshold,
                                   int pov_mode, const void *centres_dev, ptrdiff_t centre_stride_bytes, ffl_axes_record *out,
                                   uint64_t stream) {
    return radial_window_call(c, "ffl_radial_window_axes_centres", {true, false, true, nullptr, centres_dev, centre_stride_bytes},
                              n_seq, seq, first, n, radius, cut_threshold, pov_mode, out, stream);
}

int ffl_radial_window_axes_weighted_centres(ffl_ctx *c, int n_seq, const int *seq, int first, int n, int radius, float cut_threshold,
                                            int pov_mode, const ffl_dev_weights *w, const void *centres_dev,
                                            ptrdiff_t centre_stride_bytes, ffl_axes_record *out, uint64_t stream) {
    return radial_window_call(c, "ffl_radial_window_axes_weighted_centres", {true, true, true, w, centres_dev, centre_stride_bytes},
                              n_seq, seq, first, n, radius, cut_threshold, pov_mode, out, stream);
}

// ---- per-cell statistics and the variance centre -----------------------------------
static_assert(sizeof(ffl_cell_record) == 32 && sizeof(CellRecord) == 32 && offsetof(ffl_cell_record, mean_u) == offsetof(CellRecord, mean_u) &&
              offsetof(ffl_cell_record, mean_v) == offsetof(CellRecord, mean_v) && offsetof(ffl_cell_record, mean_mag) == offsetof(CellRecord, mean_mag) &&
              offsetof(ffl_cell_record, var_mag) == 24 && offsetof(CellRecord, var_mag) == 24 && alignof(ffl_cell_record) == 8,
              "CellRecord mirrors ffl_cell_record");
static_assert(sizeof(ffl_grid_centre) == 32 && sizeof(GridCentre) == 32 && offsetof(ffl_grid_centre, cx) == 0 && offsetof(GridCentre, cx) == 0 &&
              offsetof(ffl_grid_centre, cy) == 8 && offsetof(GridCentre, cy) == 8 && offsetof(ffl_grid_centre, total_var) == offsetof(GridCentre, total_var) &&
              offsetof(ffl_grid_centre, cells) == 24 && offsetof(GridCentre, cells) == 24 && offsetof(ffl_grid_centre, empty) == 28 &&
              offsetof(GridCentre, empty) == 28 && alignof(ffl_grid_centre) == 8,
              "GridCentre mirrors ffl_grid_centre");
static_assert(FFL_MAX_CELLS == FFL_CELLS_MAX, "ffl.h and ffl_kernels.h agree");

// rule G1 (FF:728-735): 1 <= cells <= FFL_MAX_CELLS and cells <= min(width, height)
static int cell_grid_check(ffl_ctx *c, const char *fn, int width, int height, int cells, int *cell_w, int *cell_h) {
    if (!frame_size_ok(width, height)) return set_err(c, FFL_ERR_INVALID, "%s: " FFL_FRAME_SIZE_RULE, fn, width, height);
    if (cells < 1 || cells > FFL_MAX_CELLS)
        return set_err(c, FFL_ERR_INVALID, "%s: rule G1: cells = %d outside 1..%d (FFL_MAX_CELLS)", fn, cells, FFL_MAX_CELLS);
    if (cells > width || cells > height)
        return set_err(c, FFL_ERR_INVALID, "%s: rule G1: cells = %d exceeds min(width, height) of %dx%d (a cell has at least one pixel)",
                       fn, cells, width, height);
    if (cell_w) *cell_w = width / cells;
    if (cell_h) *cell_h = height / cells;
    return FFL_OK;
}

int ffl_cell_grid_check(int width, int height, int cells, int *cell_w, int *cell_h) {
    return cell_grid_check(nullptr, "ffl_cell_grid_check", width, height, cells, cell_w, cell_h);
}

// The cells x cells statistics grid of n slots that hold a flow and / or its variance centre (FF:721-746), by one
// k_cell_stats launch plus k_grid_centre on stream `post`: ffl_pass1_weighted's protocol, with the flow only read and no
// pass-1 record touched.
int ffl_cell_stats(ffl_ctx *c, int n, const int *slots, int cells, ffl_cell_record *cells_dev, ffl_grid_centre *centres_dev,
                   uint64_t stream) {
    static const char *fn = "ffl_cell_stats";
    static const char *hint = "the grid's records are written to device memory (torch / hipMalloc)";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post` and d_cellrow
    CtxLock lk(c->mu);
    ExportTab t;
    if (int rc = open_slot_list(c, fn, "slots", n, slots, "flow", &t)) return rc;
    if (int rc = cell_grid_check(c, fn, c->w, c->h, cells, nullptr, nullptr)) return rc;
    if (!cells_dev && !centres_dev) return set_err(c, FFL_ERR_INVALID, "%s: cells_dev and centres_dev are both NULL (one output at least)", fn);
    if ((uintptr_t)cells_dev % 8 || (uintptr_t)centres_dev % 8)
        return set_err(c, FFL_ERR_INVALID, "%s: cells_dev and centres_dev must be 8-byte aligned", fn);
    PostRegion reg[2];
    int nreg = 0;
    if (cells_dev) reg[nreg++] = PostRegion{"cells_dev", cells_dev, sizeof(ffl_cell_record) * (size_t)n * cells * cells, hint};
    if (centres_dev) reg[nreg++] = PostRegion{"centres_dev", centres_dev, sizeof(ffl_grid_centre) * (size_t)n, hint};
    hipStream_t cst;
    if (int rc = post_begin(c, fn, stream, &cst, reg, nreg, n, slots)) return rc;
    if (int rc = post_scratch(c, fn, SCR_CELLS)) return rc;
    ffl_launch_cell_stats(c->d_flow, t, n, c->w, c->h, cells, (CellRecord *)cells_dev, (GridCentre *)centres_dev, c->d_cellrow,
                          c->s_post);
    return post_end(c, cst, n, slots);  // the caller may read, overwrite or free the outputs on `stream` straight after the call
}

// ---- region tracking and ROI maps (appendices Q and E) -------------------------------------------
static_assert(sizeof(ffl_track_state) == 48 && sizeof(TrackState) == 48 && offsetof(ffl_track_state, home_x) == offsetof(TrackState, home_x) &&
              offsetof(ffl_track_state, steps) == 32 && offsetof(TrackState, steps) == 32 && offsetof(ffl_track_state, lost_run) == 40 &&
              offsetof(TrackState, lost_run) == 40 && alignof(ffl_track_state) == 8, "TrackState mirrors ffl_track_state");
static_assert(sizeof(ffl_track_record) == 48 && sizeof(TrackRecord) == 48 && offsetof(ffl_track_record, x) == 0 && offsetof(TrackRecord, x) == 0 &&
              offsetof(ffl_track_record, y) == 8 && offsetof(TrackRecord, y) == 8 && offsetof(ffl_track_record, du) == offsetof(TrackRecord, du) &&
              offsetof(ffl_track_record, sw) == 32 && offsetof(TrackRecord, sw) == 32 && offsetof(ffl_track_record, count) == 40 &&
              offsetof(TrackRecord, count) == 40 && offsetof(ffl_track_record, status) == 44 && offsetof(TrackRecord, status) == 44 &&
              alignof(ffl_track_record) == 8, "TrackRecord mirrors ffl_track_record");
static_assert((int)FFL_MAX_TRACKS == FFL_TRACK_MAX_T && (int)FFL_MAX_TRACK_RADIUS == FFL_TRACK_MAX_R && (int)FFL_TRACK_HOLD == TRK_HOLD &&
              (int)FFL_TRACK_HOME == TRK_HOME && (int)FFL_TRACK_OK == TRK_OK && (int)FFL_TRACK_CUT == TRK_CUT && (int)FFL_TRACK_LOST == TRK_LOST &&
              (int)FFL_TRACK_CLAMPED == TRK_CLAMPED, "ffl.h and ffl_kernels.h agree");

int ffl_track_default_params(ffl_track_params *out) {
    if (!out) return FFL_ERR_INVALID;
    *out = ffl_track_params{12, FFL_TRACK_HOLD, 7.0f};   // the radius: the project's own choice, not tuned on footage; 7.0f: FF:876
    return FFL_OK;
}

// The accepted parameters of appendix Q.
static int track_params_check(ffl_ctx *c, const char *fn, const ffl_track_params *p) {
    if (!p) return set_err(c, FFL_ERR_INVALID, "%s: NULL parameters", fn);
    if (p->radius < 1 || p->radius > FFL_MAX_TRACK_RADIUS)
        return set_err(c, FFL_ERR_INVALID, "%s: radius = %d outside 1..%d (FFL_MAX_TRACK_RADIUS)", fn, p->radius, (int)FFL_MAX_TRACK_RADIUS);
    if (p->on_cut != FFL_TRACK_HOLD && p->on_cut != FFL_TRACK_HOME)
        return set_err(c, FFL_ERR_INVALID, "%s: on_cut = %d is neither 0 (FFL_TRACK_HOLD) nor 1 (FFL_TRACK_HOME)", fn, p->on_cut);
    if (p->cut_threshold != p->cut_threshold) return set_err(c, FFL_ERR_INVALID, "%s: cut_threshold is NaN", fn);
    return FFL_OK;
}

int ffl_track_params_check(const ffl_track_params *p) { return track_params_check(nullptr, "ffl_track_params_check", p); }

// n_tracks points through n slots that hold a flow, by ONE k_track launch of n_tracks workgroups on stream `post`:
// ffl_cell_stats' protocol, with the flow, its records and the maps only read.
int ffl_track_advance(ffl_ctx *c, int n, const int *slots, int n_tracks, const ffl_track_params *p, const ffl_dev_weights *w,
                      ffl_track_state *state_dev, ffl_track_record *out_dev, uint64_t stream) {
    static const char *fn = "ffl_track_advance";
    static const char *hint = "the track's state and records live in device memory (torch / hipMalloc)";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post`
    CtxLock lk(c->mu);
    ExportTab t;
    if (int rc = open_slot_list(c, fn, "items", n, slots, "flow", &t)) return rc;
    if (n_tracks < 1 || n_tracks > FFL_MAX_TRACKS)
        return set_err(c, FFL_ERR_INVALID, "%s: n_tracks = %d outside 1..%d (FFL_MAX_TRACKS)", fn, n_tracks, (int)FFL_MAX_TRACKS);
    ffl_track_params prm;
    ffl_track_default_params(&prm);
    if (p) prm = *p;
    if (int rc = track_params_check(c, fn, &prm)) return rc;
    size_t wbytes = 0;
    if (w)
        if (int rc = dev_weights_check(c, fn, n, c->w, c->h, w, &wbytes)) return rc;
    if (!state_dev || !out_dev) return set_err(c, FFL_ERR_INVALID, "%s: NULL %s", fn, !state_dev ? "state_dev" : "out_dev");
    if ((uintptr_t)state_dev % 8 || (uintptr_t)out_dev % 8)
        return set_err(c, FFL_ERR_INVALID, "%s: state_dev and out_dev must be 8-byte aligned", fn);
    const size_t sbytes = sizeof(ffl_track_state) * (size_t)n_tracks, obytes = sizeof(ffl_track_record) * (size_t)n * (size_t)n_tracks;
    const uintptr_t s0 = (uintptr_t)state_dev, o0 = (uintptr_t)out_dev;
    if (s0 < o0 + obytes && o0 < s0 + sbytes)
        return set_err(c, FFL_ERR_INVALID, "%s: overlap: state_dev (%zu bytes) and out_dev (%zu bytes) share memory", fn, sbytes, obytes);
    PostRegion reg[3] = {{"state_dev", state_dev, sbytes, hint}, {"out_dev", out_dev, obytes, hint}};
    int nreg = 2;
    if (w) reg[nreg++] = PostRegion{"the weight maps", w->base, wbytes, kHostWeights};
    hipStream_t cst;
    if (int rc = post_begin(c, fn, stream, &cst, reg, nreg, n, slots)) return rc;
    WeightArgs wa{};
    if (w) wa = WeightArgs{(const char *)w->base, (long long)w->item_stride, (long long)w->row_pitch};
    ffl_launch_track(c->d_flow, c->d_res, t, n, n_tracks, c->w, c->h, prm.radius, prm.on_cut, prm.cut_threshold, w ? &wa : nullptr,
                     (TrackState *)state_dev, (TrackRecord *)out_dev, c->s_post);
    return post_end(c, cst, n, slots);  // the caller may read the records, or re-seed the state, on `stream` straight after the call
}

int ffl_roi_default_params(ffl_roi_params *out) {
    if (!out) return FFL_ERR_INVALID;
    *out = ffl_roi_params{48.0f, 48.0f, 1};   // the project's own choice, not tuned on footage
    return FFL_OK;
}

// The accepted parameters of appendix E.  The comparisons are written so that a NaN fails them.
static int roi_params_check(ffl_ctx *c, const char *fn, const ffl_roi_params *p) {
    if (!p) return set_err(c, FFL_ERR_INVALID, "%s: NULL parameters", fn);
    if (!(p->ax >= 0.5f && p->ax <= 32768.0f) || !(p->ay >= 0.5f && p->ay <= 32768.0f))
        return set_err(c, FFL_ERR_INVALID, "%s: half-axes (%g, %g) outside 0.5..32768 (finite)", fn, (double)p->ax, (double)p->ay);
    if (p->soft != 0 && p->soft != 1) return set_err(c, FFL_ERR_INVALID, "%s: soft = %d is neither 0 (hard) nor 1 (soft)", fn, p->soft);
    return FFL_OK;
}

int ffl_roi_params_check(const ffl_roi_params *p) { return roi_params_check(nullptr, "ffl_roi_params_check", p); }

// n maps about n centres by ONE k_roi_weights launch on stream `post`: ffl_texture_weights' protocol without frame slots.  The
// call names no slot; post_end() records its event all the same (publish_post records before it publishes), and that event is
// what the caller's stream waits for.
int ffl_roi_weights(ffl_ctx *c, int n, const void *centres_dev, ptrdiff_t cstride, const ffl_roi_params *p, const ffl_dev_weights *gate,
                    const ffl_dev_weights *out, uint64_t stream) {
    static const char *fn = "ffl_roi_weights";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post`, as ffl_texture_weights
    CtxLock lk(c->mu);
    if (n < 1 || n > c->max_batch)
        return set_err(c, FFL_ERR_INVALID, "%s: n = %d items outside 1..%d (the context's max_batch)", fn, n, c->max_batch);
    ffl_roi_params prm;
    ffl_roi_default_params(&prm);
    if (p) prm = *p;
    if (int rc = roi_params_check(c, fn, &prm)) return rc;
    size_t obytes, gbytes = 0;
    if (!out) return set_err(c, FFL_ERR_INVALID, "%s: NULL out descriptor", fn);
    if (int rc = dev_weights_check(c, fn, n, c->w, c->h, out, &obytes)) return rc;
    if (n > 1 && out->item_stride == 0)
        return set_err(c, FFL_ERR_INVALID, "%s: overlap: out item stride 0 with n = %d maps to write (one map per item)", fn, n);
    bool in_place = false;
    const uintptr_t o0 = (uintptr_t)out->base;
    if (gate) {
        if (int rc = dev_weights_check(c, fn, n, c->w, c->h, gate, &gbytes)) return rc;
        in_place = gate->base == out->base && gate->item_stride == out->item_stride && gate->row_pitch == out->row_pitch;
        const uintptr_t g0 = (uintptr_t)gate->base;
        if (!in_place && o0 < g0 + gbytes && g0 < o0 + obytes)
            return set_err(c, FFL_ERR_INVALID, "%s: overlap: out (%zu bytes) and gate (%zu bytes) share memory, and gate is not "
                                               "exactly out (same base, item stride and row pitch: the in-place form)",
                           fn, obytes, gbytes);
    }
    if (!centres_dev) return set_err(c, FFL_ERR_INVALID, "%s: NULL centres_dev", fn);   // rule E1
    if ((uintptr_t)centres_dev % 8) return set_err(c, FFL_ERR_INVALID, "%s: centres_dev must be 8-byte aligned", fn);
    if (cstride < 16 || cstride % 8 || cstride > ((ptrdiff_t)1 << 40))
        return set_err(c, FFL_ERR_INVALID, "%s: centre stride %td: a multiple of 8 bytes, at least 16 (two doubles)", fn, cstride);
    const size_t cbytes = (size_t)(n - 1) * (size_t)cstride + 16;
    const uintptr_t c0 = (uintptr_t)centres_dev;
    if (o0 < c0 + cbytes && c0 < o0 + obytes)
        return set_err(c, FFL_ERR_INVALID, "%s: overlap: out (%zu bytes) and the centres (%zu bytes) share memory", fn, obytes, cbytes);
    hipStream_t cst;
    PostRegion reg[3] = {{"out", out->base, obytes, kHostWeights}, {"centres_dev", centres_dev, cbytes, kHostCentres}};
    int nreg = 2;
    if (gate && !in_place) reg[nreg++] = PostRegion{"the gate maps", gate->base, gbytes, kHostWeights};
    if (int rc = post_begin(c, fn, stream, &cst, reg, nreg, 0, nullptr)) return rc;
    WeightArgs ga;
    if (gate) ga = WeightArgs{(const char *)gate->base, (long long)gate->item_stride, (long long)gate->row_pitch};
    ffl_launch_roi_weights((const char *)centres_dev, (long long)cstride, n, c->w, c->h, prm.ax, prm.ay, prm.soft, gate ? &ga : nullptr,
                           (char *)out->base, (long long)out->item_stride, (long long)out->row_pitch, c->s_post);
    return post_end(c, cst, 0, nullptr);  // the caller may read the maps, or overwrite the gate or the centres, on `stream` straight after
}

// ---- template matching about tracked centres -----------------------------------------
static_assert(sizeof(ffl_match_record) == 48 && sizeof(MatchRecord) == 48 && offsetof(ffl_match_record, x) == 0 && offsetof(MatchRecord, x) == 0 &&
              offsetof(ffl_match_record, y) == 8 && offsetof(MatchRecord, y) == 8 && offsetof(ffl_match_record, dx) == 16 &&
              offsetof(MatchRecord, dx) == 16 && offsetof(ffl_match_record, dy) == 20 && offsetof(MatchRecord, dy) == 20 &&
              offsetof(ffl_match_record, cost) == 24 && offsetof(MatchRecord, cost) == 24 && offsetof(ffl_match_record, second) == 32 &&
              offsetof(MatchRecord, second) == 32 && offsetof(ffl_match_record, status) == 40 && offsetof(MatchRecord, status) == 40 &&
              alignof(ffl_match_record) == 8, "MatchRecord mirrors ffl_match_record");
static_assert((int)FFL_MAX_MATCH_P == FFL_MATCH_MAX_P && (int)FFL_MAX_MATCH_S == FFL_MATCH_MAX_S && (int)FFL_MATCH_SSD == MCH_SSD &&
              (int)FFL_MATCH_ZSSD == MCH_ZSSD && (int)FFL_MATCH_FLAT == MCH_FLAT && (int)FFL_MATCH_POOR == MCH_POOR &&
              (int)FFL_MATCH_AMBIGUOUS == MCH_AMBIGUOUS && sizeof(ffl_track_state) == sizeof(ffl_match_record),
              "ffl.h and ffl_kernels.h agree; a state and a record are 48 bytes, the track pitch of rule N1");

int ffl_match_default_params(ffl_match_params *out) {
    if (!out) return FFL_ERR_INVALID;
    *out = ffl_match_params{8, 8, FFL_MATCH_ZSSD, 0, 25.0, 400.0, 0.8};   // the project's own choice, not tuned on footage
    return FFL_OK;
}

// The accepted parameters of appendix N.  The comparisons are written so that a NaN fails them.
static int match_params_check(ffl_ctx *c, const char *fn, const ffl_match_params *p) {
    if (!p) return set_err(c, FFL_ERR_INVALID, "%s: NULL parameters", fn);
    if (p->p < 1 || p->p > FFL_MAX_MATCH_P)
        return set_err(c, FFL_ERR_INVALID, "%s: p = %d outside 1..%d (FFL_MAX_MATCH_P; the template is (2p+1)^2)", fn, p->p, (int)FFL_MAX_MATCH_P);
    if (p->s < 1 || p->s > FFL_MAX_MATCH_S)
        return set_err(c, FFL_ERR_INVALID, "%s: s = %d outside 1..%d (FFL_MAX_MATCH_S; the search is |dx|, |dy| <= s)", fn, p->s, (int)FFL_MAX_MATCH_S);
    if (p->mode != FFL_MATCH_SSD && p->mode != FFL_MATCH_ZSSD)
        return set_err(c, FFL_ERR_INVALID, "%s: mode = %d is neither 0 (FFL_MATCH_SSD) nor 1 (FFL_MATCH_ZSSD)", fn, p->mode);
    if (!(p->min_var >= 0.0 && p->min_var < HUGE_VAL)) return set_err(c, FFL_ERR_INVALID, "%s: min_var = %g outside 0 <= min_var (finite)", fn, p->min_var);
    if (!(p->max_mse >= 0.0 && p->max_mse <= 65025.0))
        return set_err(c, FFL_ERR_INVALID, "%s: max_mse = %g outside 0..65025 (finite)", fn, p->max_mse);
    if (!(p->ratio > 0.0 && p->ratio <= 1.0)) return set_err(c, FFL_ERR_INVALID, "%s: ratio = %g outside 0 < ratio <= 1 (finite)", fn, p->ratio);
    return FFL_OK;
}

int ffl_match_params_check(const ffl_match_params *p) { return match_params_check(nullptr, "ffl_match_params_check", p); }

static const char *kHostMatch = "templates, centres and match records live in device memory (torch / hipMalloc)";

// what both calls refuse of their track count, their pointers and the three regions (templates, centres, records; obytes 0: no
// records): NULL, alignment, the centre stride of rule N1 and any overlap
static int match_regions_check(ffl_ctx *c, const char *fn, int n, int n_tracks, int p, const void *tmpl, const void *cen, ptrdiff_t cstride,
                               const void *out, bool has_out, size_t *tbytes, size_t *cbytes, size_t *obytes) {
    if (n_tracks < 1 || n_tracks > FFL_MAX_TRACKS)
        return set_err(c, FFL_ERR_INVALID, "%s: n_tracks = %d outside 1..%d (FFL_MAX_TRACKS)", fn, n_tracks, (int)FFL_MAX_TRACKS);
    if (!tmpl || !cen || (has_out && !out))
        return set_err(c, FFL_ERR_INVALID, "%s: NULL %s", fn, !tmpl ? "templates_dev" : !cen ? "centres_dev" : "out_dev");
    if ((uintptr_t)cen % 8 || (has_out && (uintptr_t)out % 8))
        return set_err(c, FFL_ERR_INVALID, "%s: centres_dev and out_dev must be 8-byte aligned", fn);
    const ptrdiff_t span = 48 * (ptrdiff_t)(n_tracks - 1) + 16;   // rule N1: track t's centre at + 48 t
    if (cstride % 8 || cstride < span || cstride > ((ptrdiff_t)1 << 40))
        return set_err(c, FFL_ERR_INVALID, "%s: centre stride %td: a multiple of 8 bytes, at least 48 * (n_tracks - 1) + 16 = %td (rule N1)",
                       fn, cstride, span);
    const size_t side = 2 * (size_t)p + 1;
    *tbytes = side * side * (size_t)n_tracks;
    *cbytes = (size_t)(n - 1) * (size_t)cstride + (size_t)span;
    *obytes = has_out ? sizeof(ffl_match_record) * (size_t)n * (size_t)n_tracks : 0;
    const struct { const char *what; uintptr_t a; size_t b; } r[3] = {
        {"templates_dev", (uintptr_t)tmpl, *tbytes}, {"centres_dev", (uintptr_t)cen, *cbytes}, {"out_dev", (uintptr_t)out, *obytes}};
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (r[i].b && r[j].b && r[i].a < r[j].a + r[j].b && r[j].a < r[i].a + r[i].b)
                return set_err(c, FFL_ERR_INVALID, "%s: overlap: %s (%zu bytes) and %s (%zu bytes) share memory", fn, r[i].what, r[i].b,
                               r[j].what, r[j].b);
    return FFL_OK;
}

// n_tracks templates out of one frame slot by ONE k_track_template launch on stream `post`: ffl_texture_weights' protocol.
int ffl_track_template(ffl_ctx *c, int fslot, int n_tracks, const void *centres_dev, int p, void *templates_dev, uint64_t stream) {
    static const char *fn = "ffl_track_template";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post`, as ffl_texture_weights
    CtxLock lk(c->mu);
    if (fslot < 0 || fslot >= c->n_fslots) return set_err(c, FFL_ERR_INVALID, "%s: frame slot %d out of range", fn, fslot);
    if (!c->frame_valid[fslot]) return set_err(c, FFL_ERR_STATE, "%s: frame slot %d was never uploaded", fn, fslot);
    if (p < 1 || p > FFL_MAX_MATCH_P)
        return set_err(c, FFL_ERR_INVALID, "%s: p = %d outside 1..%d (FFL_MAX_MATCH_P; the template is (2p+1)^2)", fn, p, (int)FFL_MAX_MATCH_P);
    size_t tbytes, cbytes, obytes;
    if (int rc = match_regions_check(c, fn, 1, n_tracks, p, templates_dev, centres_dev, 48 * (ptrdiff_t)n_tracks, nullptr, false, &tbytes,
                                     &cbytes, &obytes))
        return rc;
    hipStream_t cst;
    PostRegion reg[2] = {{"templates_dev", templates_dev, tbytes, kHostMatch}, {"centres_dev", centres_dev, cbytes, kHostMatch}};
    if (int rc = post_begin(c, fn, stream, &cst, reg, 2, 0, nullptr)) return rc;
    {
        WaitOnce wait_post(c->s_post);   // the upload that filled the frame slot
        HIPCHK(c, wait_post(c->ev_uploaded[fslot].get()));
    }
    ffl_launch_track_template(c->d_gray + (size_t)fslot * c->N, n_tracks, c->w, c->h, p, (const char *)centres_dev,
                              (unsigned char *)templates_dev, c->s_post);
    return post_end_frames(c, cst, 0, nullptr, 1, &fslot, nullptr);  // the caller may read the templates on `stream` straight after
}

// n x n_tracks searches by ONE k_track_match launch of (n_tracks, n) workgroups on stream `post`: ffl_texture_weights' protocol,
// with the frames and the templates only read and the centres read and, with write_back, written.
int ffl_track_match(ffl_ctx *c, int n, const int *fslots, int n_tracks, const ffl_match_params *p, const void *templates_dev,
                    void *centres_dev, ptrdiff_t cstride, int write_back, ffl_match_record *out_dev, uint64_t stream) {
    static const char *fn = "ffl_track_match";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post`, as ffl_texture_weights
    CtxLock lk(c->mu);
    if (n < 1 || n > c->max_batch)
        return set_err(c, FFL_ERR_INVALID, "%s: n = %d items outside 1..%d (the context's max_batch)", fn, n, c->max_batch);
    if (!fslots) return set_err(c, FFL_ERR_INVALID, "%s: NULL fslots", fn);
    ExportTab tf;
    for (int i = 0; i < n; i++) {   // frame slots may repeat between items
        const int fs = fslots[i];
        if (fs < 0 || fs >= c->n_fslots) return set_err(c, FFL_ERR_INVALID, "%s: item %d: frame slot %d out of range", fn, i, fs);
        if (!c->frame_valid[fs]) return set_err(c, FFL_ERR_STATE, "%s: item %d: frame slot %d was never uploaded", fn, i, fs);
        tf.slot[i] = fs;
    }
    ffl_match_params prm;
    ffl_match_default_params(&prm);
    if (p) prm = *p;
    if (int rc = match_params_check(c, fn, &prm)) return rc;
    if (write_back != 0 && write_back != 1)
        return set_err(c, FFL_ERR_INVALID, "%s: write_back = %d is neither 0 nor 1 (rule N8)", fn, write_back);
    size_t tbytes, cbytes, obytes;
    if (int rc = match_regions_check(c, fn, n, n_tracks, prm.p, templates_dev, centres_dev, cstride, out_dev, true, &tbytes, &cbytes, &obytes))
        return rc;
    hipStream_t cst;
    PostRegion reg[3] = {{"out_dev", out_dev, obytes, kHostMatch}, {"templates_dev", templates_dev, tbytes, kHostMatch},
                         {"centres_dev", centres_dev, cbytes, kHostMatch}};
    if (int rc = post_begin(c, fn, stream, &cst, reg, 3, 0, nullptr)) return rc;
    {
        WaitOnce wait_post(c->s_post);   // the frames: a run of slots shares one upload event
        for (int i = 0; i < n; i++) HIPCHK(c, wait_post(c->ev_uploaded[fslots[i]].get()));
    }
    ffl_launch_track_match(c->d_gray, c->N, tf, n, n_tracks, c->w, c->h, prm.p, prm.s, prm.mode, prm.min_var, prm.max_mse, prm.ratio,
                           (const unsigned char *)templates_dev, (char *)centres_dev, (long long)cstride, write_back,
                           (MatchRecord *)out_dev, c->s_post);
    // the caller may read the records and the corrected centres on `stream` straight after the call
    return post_end_frames(c, cst, 0, nullptr, n, fslots, nullptr);
}

// ---- whole-frame template re-detection -------------------------------------------------
static_assert((int)FFL_MAX_REDETECT_EXCLUDE == FFL_REDETECT_MAX_EXCLUDE && (int)FFL_REDETECT_SKIPPED == RDT_SKIPPED &&
              (FFL_REDETECT_SKIPPED & (FFL_MATCH_FLAT | FFL_MATCH_POOR | FFL_MATCH_AMBIGUOUS)) == 0 &&
              2 * FFL_REDETECT_MAX_EXCLUDE + 1 <= 64 * (RDT_EXCL_NX - 1) + 1 && 2 * FFL_REDETECT_MAX_EXCLUDE + 1 <= 16 * (RDT_EXCL_NY - 1) + 1,
              "ffl.h and ffl_kernels.h agree; the exclusion square fits the re-walked tiles");

int ffl_redetect_default_params(ffl_redetect_params *out) {
    if (!out) return FFL_ERR_INVALID;
    ffl_match_params m;
    ffl_match_default_params(&m);   // the match defaults with exclude = p, the whole frame, triggered by POOR: not tuned on footage
    *out = ffl_redetect_params{m.p, m.mode, m.p, 0, FFL_MATCH_POOR, 0, m.min_var, m.max_mse, m.ratio};
    return FFL_OK;
}

// The accepted parameters of appendix L.  The comparisons are written so that a NaN fails them.
static int redetect_params_check(ffl_ctx *c, const char *fn, const ffl_redetect_params *p) {
    if (!p) return set_err(c, FFL_ERR_INVALID, "%s: NULL parameters", fn);
    if (p->p < 1 || p->p > FFL_MAX_MATCH_P)
        return set_err(c, FFL_ERR_INVALID, "%s: p = %d outside 1..%d (FFL_MAX_MATCH_P; the template is (2p+1)^2)", fn, p->p, (int)FFL_MAX_MATCH_P);
    if (p->mode != FFL_MATCH_SSD && p->mode != FFL_MATCH_ZSSD)
        return set_err(c, FFL_ERR_INVALID, "%s: mode = %d is neither 0 (FFL_MATCH_SSD) nor 1 (FFL_MATCH_ZSSD)", fn, p->mode);
    if (p->exclude < 1 || p->exclude > FFL_MAX_REDETECT_EXCLUDE)
        return set_err(c, FFL_ERR_INVALID, "%s: exclude = %d outside 1..%d (FFL_MAX_REDETECT_EXCLUDE; rule L5's square)", fn, p->exclude,
                       (int)FFL_MAX_REDETECT_EXCLUDE);
    if (p->reach < 0 || p->reach > 32768)
        return set_err(c, FFL_ERR_INVALID, "%s: reach = %d outside 0 (the whole frame) or 1..32768 (rule L2)", fn, p->reach);
    if (!(p->min_var >= 0.0 && p->min_var < HUGE_VAL)) return set_err(c, FFL_ERR_INVALID, "%s: min_var = %g outside 0 <= min_var (finite)", fn, p->min_var);
    if (!(p->max_mse >= 0.0 && p->max_mse <= 65025.0))
        return set_err(c, FFL_ERR_INVALID, "%s: max_mse = %g outside 0..65025 (finite)", fn, p->max_mse);
    if (!(p->ratio > 0.0 && p->ratio <= 1.0)) return set_err(c, FFL_ERR_INVALID, "%s: ratio = %g outside 0 < ratio <= 1 (finite)", fn, p->ratio);
    return FFL_OK;
}

int ffl_redetect_params_check(const ffl_redetect_params *p) { return redetect_params_check(nullptr, "ffl_redetect_params_check", p); }

// n x n_tracks searches by four launches on stream `post`: ffl_track_match's protocol, with the trigger words as a fourth
// caller region and the tile keys in the SCR_REDETECT scratch.
int ffl_track_redetect(ffl_ctx *c, int n, const int *fslots, int n_tracks, const ffl_redetect_params *p, const void *templates_dev,
                       void *centres_dev, ptrdiff_t cstride, const void *trigger_dev, ptrdiff_t tstride, int write_back,
                       ffl_match_record *out_dev, uint64_t stream) {
    static const char *fn = "ffl_track_redetect";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post` and d_rdscr
    CtxLock lk(c->mu);
    if (n < 1 || n > c->max_batch)
        return set_err(c, FFL_ERR_INVALID, "%s: n = %d items outside 1..%d (the context's max_batch)", fn, n, c->max_batch);
    if (!fslots) return set_err(c, FFL_ERR_INVALID, "%s: NULL fslots", fn);
    RedetectArgs a;
    for (int i = 0; i < n; i++) {   // frame slots may repeat between items
        const int fs = fslots[i];
        if (fs < 0 || fs >= c->n_fslots) return set_err(c, FFL_ERR_INVALID, "%s: item %d: frame slot %d out of range", fn, i, fs);
        if (!c->frame_valid[fs]) return set_err(c, FFL_ERR_STATE, "%s: item %d: frame slot %d was never uploaded", fn, i, fs);
        a.fr.slot[i] = fs;
    }
    ffl_redetect_params prm;
    ffl_redetect_default_params(&prm);
    if (p) prm = *p;
    if (int rc = redetect_params_check(c, fn, &prm)) return rc;
    if (write_back != 0 && write_back != 1)
        return set_err(c, FFL_ERR_INVALID, "%s: write_back = %d is neither 0 nor 1 (rule L8)", fn, write_back);
    size_t tbytes, cbytes, obytes, gbytes = 0;
    if (int rc = match_regions_check(c, fn, n, n_tracks, prm.p, templates_dev, centres_dev, cstride, out_dev, true, &tbytes, &cbytes, &obytes))
        return rc;
    if (trigger_dev) {
        if ((uintptr_t)trigger_dev % 4) return set_err(c, FFL_ERR_INVALID, "%s: trigger_dev must be 4-byte aligned (rule L1)", fn);
        const ptrdiff_t span = 48 * (ptrdiff_t)(n_tracks - 1) + 4;   // rule L1: track t's word at + 48 t
        if (tstride % 4 || tstride < span || tstride > ((ptrdiff_t)1 << 40))
            return set_err(c, FFL_ERR_INVALID, "%s: trigger stride %td: a multiple of 4 bytes, at least 48 * (n_tracks - 1) + 4 = %td (rule L1)",
                           fn, tstride, span);
        gbytes = (size_t)(n - 1) * (size_t)tstride + (size_t)span;
        const struct { const char *what; uintptr_t a; size_t b; } r[3] = {
            {"centres_dev", (uintptr_t)centres_dev, cbytes}, {"templates_dev", (uintptr_t)templates_dev, tbytes}, {"out_dev", (uintptr_t)out_dev, obytes}};
        const uintptr_t g = (uintptr_t)trigger_dev;
        for (int i = 0; i < 3; i++)
            if (g < r[i].a + r[i].b && r[i].a < g + gbytes)
                return set_err(c, FFL_ERR_INVALID, "%s: overlap: trigger_dev (%zu bytes) and %s (%zu bytes) share memory", fn, gbytes, r[i].what,
                               r[i].b);
    }
    hipStream_t cst;
    PostRegion reg[4] = {{"out_dev", out_dev, obytes, kHostMatch}, {"templates_dev", templates_dev, tbytes, kHostMatch},
                         {"centres_dev", centres_dev, cbytes, kHostMatch}, {"trigger_dev", trigger_dev, gbytes, kHostMatch}};
    if (int rc = post_begin(c, fn, stream, &cst, reg, trigger_dev ? 4 : 3, 0, nullptr)) return rc;
    if (int rc = post_scratch(c, fn, SCR_REDETECT)) return rc;
    {
        WaitOnce wait_post(c->s_post);   // the frames: a run of slots shares one upload event
        for (int i = 0; i < n; i++) HIPCHK(c, wait_post(c->ev_uploaded[fslots[i]].get()));
    }
    a.gray = c->d_gray;
    a.N = c->N;
    a.n_tracks = n_tracks;
    a.w = c->w;
    a.h = c->h;
    a.p = prm.p;
    a.mode = prm.mode;
    a.exclude = prm.exclude;
    a.reach = prm.reach;
    a.mask = prm.trigger_mask;
    a.write_back = write_back;
    a.min_var = prm.min_var;
    a.max_mse = prm.max_mse;
    a.ratio = prm.ratio;
    a.tmpl = (const unsigned char *)templates_dev;
    a.cen = (char *)centres_dev;
    a.cstride = (long long)cstride;
    a.trig = (const char *)trigger_dev;
    a.tstride = (long long)tstride;
    a.scr = reinterpret_cast<unsigned long long *>((double *)c->d_rdscr);
    a.sstride = (long long)ffl_redetect_words(c->w, c->h);
    a.TX = ffl_redetect_tiles_x(c->w);
    a.TY = ffl_redetect_tiles_y(c->h);
    // L columns touch at most ceil(L / 64) + 1 tile columns wherever they start; rows alike with 16
    const int side = 2 * prm.reach + 1, eside = 2 * prm.exclude + 1;
    a.gx = prm.reach ? std::min(a.TX, (side + 63) / 64 + 1) : a.TX;
    a.gy = prm.reach ? std::min(a.TY, (side + 15) / 16 + 1) : a.TY;
    a.ex = std::min(RDT_EXCL_NX, (eside + 63) / 64 + 1);
    a.ey = std::min(RDT_EXCL_NY, (eside + 15) / 16 + 1);
    a.out = (MatchRecord *)out_dev;
    ffl_launch_track_redetect(a, n, c->s_post);
    // the caller may read the records and the re-detected centres on `stream` straight after the call
    return post_end_frames(c, cst, 0, nullptr, n, fslots, nullptr);
}

// ---- global-motion fit and compensation ---------------------------------------------
static_assert(sizeof(ffl_motion_record) == 64 && sizeof(MotionRecord) == 64 && offsetof(ffl_motion_record, a0) == 0 &&
              offsetof(MotionRecord, a0) == 0 && offsetof(ffl_motion_record, b0) == 24 && offsetof(MotionRecord, b0) == 24 &&
              offsetof(ffl_motion_record, sw) == 48 && offsetof(MotionRecord, sw) == 48 && offsetof(ffl_motion_record, model) == 56 &&
              offsetof(MotionRecord, model) == 56 && offsetof(ffl_motion_record, status) == 60 && offsetof(MotionRecord, status) == 60 &&
              alignof(ffl_motion_record) == 8, "MotionRecord mirrors ffl_motion_record");
static_assert(FFL_MOTION_N_SUMS == FFL_MOTION_NSUMS && FFL_MOTION_TRANSLATION == MOT_TRANSLATION && FFL_MOTION_RIGID == MOT_RIGID &&
              FFL_MOTION_SIMILARITY == MOT_SIMILARITY && FFL_MOTION_AFFINE == MOT_AFFINE && FFL_MOTION_OK == MOT_OK &&
              FFL_MOTION_EMPTY == MOT_EMPTY && FFL_MOTION_DEGENERATE == MOT_DEGENERATE, "ffl.h and ffl_kernels.h agree");

int ffl_motion_default_params(ffl_motion_params *out) {   // rule C9
    if (!out) return FFL_ERR_INVALID;
    *out = ffl_motion_params{FFL_MOTION_TRANSLATION, 3, 1.0f};
    return FFL_OK;
}

// The accepted parameters of appendix C.  The comparisons are written so that a NaN fails them.
static int motion_params_check(ffl_ctx *c, const char *fn, const ffl_motion_params *p) {
    if (!p) return set_err(c, FFL_ERR_INVALID, "%s: NULL parameters", fn);
    if (p->model < FFL_MOTION_TRANSLATION || p->model > FFL_MOTION_AFFINE)
        return set_err(c, FFL_ERR_INVALID, "%s: rule C2: model = %d is none of FFL_MOTION_TRANSLATION 0, RIGID 1, SIMILARITY 2, AFFINE 3",
                       fn, p->model);
    if (p->iterations < 1 || p->iterations > 8)
        return set_err(c, FFL_ERR_INVALID, "%s: rule C7: iterations = %d outside 1..8", fn, p->iterations);
    if (!(p->tau > 0.0f && p->tau <= 1e6f))
        return set_err(c, FFL_ERR_INVALID, "%s: rule C3: tau = %g outside 0 < tau <= 1e6 (finite)", fn, (double)p->tau);
    return FFL_OK;
}

int ffl_motion_params_check(const ffl_motion_params *p) { return motion_params_check(nullptr, "ffl_motion_params_check", p); }

int ffl_motion_solve(const double *sums, int model, ffl_motion_record *out) {
    static const char *fn = "ffl_motion_solve";
    if (!sums || !out) return set_err(nullptr, FFL_ERR_INVALID, "%s: NULL %s", fn, !sums ? "sums" : "out");
    if (model < FFL_MOTION_TRANSLATION || model > FFL_MOTION_AFFINE)
        return set_err(nullptr, FFL_ERR_INVALID, "%s: rule C2: model = %d is none of FFL_MOTION_TRANSLATION 0, RIGID 1, SIMILARITY 2, "
                                                 "AFFINE 3", fn, model);
    MotionRecord r;
    ffl_motion_solve_body(sums, model, &r);
    memcpy(out, &r, sizeof r);
    return FFL_OK;
}

static const char *kHostModels = "models, sums and priors live in device memory (torch / hipMalloc)";

// six doubles per item at `stride` bytes: rule C2's model as ffl_motion_fit's prior and ffl_motion_subtract's models read it
static int model_array_check(ffl_ctx *c, const char *fn, const char *what, const void *p, ptrdiff_t stride) {
    if ((uintptr_t)p % 8) return set_err(c, FFL_ERR_INVALID, "%s: %s must be 8-byte aligned", fn, what);
    if (stride < 48 || stride % 8 || stride > ((ptrdiff_t)1 << 40))
        return set_err(c, FFL_ERR_INVALID, "%s: %s stride %td: a multiple of 8 bytes, at least 48 (six doubles)", fn, what, stride);
    return FFL_OK;
}

// `iterations` times the fit's k_strip_sums + k_motion_solve over n slots that hold a flow, on stream `post`: ffl_pass1_weighted's protocol
// with the flow and its records only read.  Pass k + 1 reads the records pass k wrote (rule C7), on the one stream.
int ffl_motion_fit(ffl_ctx *c, int n, const int *slots, const ffl_motion_params *p, const ffl_dev_weights *w, const void *prior_dev,
                   ptrdiff_t prior_stride, ffl_motion_record *models_dev, double *sums_dev, uint64_t stream) {
    static const char *fn = "ffl_motion_fit";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post` and d_mpsum
    CtxLock lk(c->mu);
    ExportTab t;
    if (int rc = open_slot_list(c, fn, "slots", n, slots, "flow", &t)) return rc;
    ffl_motion_params prm;
    ffl_motion_default_params(&prm);
    if (p) prm = *p;
    if (int rc = motion_params_check(c, fn, &prm)) return rc;
    size_t wbytes = 0;
    if (w)
        if (int rc = dev_weights_check(c, fn, n, c->w, c->h, w, &wbytes)) return rc;
    if (!models_dev) return set_err(c, FFL_ERR_INVALID, "%s: NULL models_dev", fn);
    if ((uintptr_t)models_dev % 8 || (uintptr_t)sums_dev % 8) return set_err(c, FFL_ERR_INVALID, "%s: models_dev and sums_dev must be 8-byte aligned", fn);
    const size_t mbytes = sizeof(ffl_motion_record) * (size_t)n;
    size_t pbytes = 0;
    if (prior_dev) {
        if (int rc = model_array_check(c, fn, "prior_dev", prior_dev, prior_stride)) return rc;
        pbytes = (size_t)(n - 1) * (size_t)prior_stride + 48;
        const uintptr_t m0 = (uintptr_t)models_dev, p0 = (uintptr_t)prior_dev;
        if (prm.iterations > 1 && m0 < p0 + pbytes && p0 < m0 + mbytes)
            return set_err(c, FFL_ERR_INVALID, "%s: rule C7: overlap: models_dev (%zu bytes) and prior_dev (%zu bytes) share memory "
                                               "with iterations = %d (pass 2 reads models_dev as its prior)", fn, mbytes, pbytes, prm.iterations);
    }
    PostRegion reg[4];
    int nreg = 0;
    reg[nreg++] = PostRegion{"models_dev", models_dev, mbytes, kHostModels};
    if (sums_dev) reg[nreg++] = PostRegion{"sums_dev", sums_dev, sizeof(double) * FFL_MOTION_N_SUMS * (size_t)n, kHostModels};
    if (prior_dev) reg[nreg++] = PostRegion{"prior_dev", prior_dev, pbytes, kHostModels};
    if (w) reg[nreg++] = PostRegion{"the weight maps", w->base, wbytes, kHostWeights};
    hipStream_t cst;
    if (int rc = post_begin(c, fn, stream, &cst, reg, nreg, n, slots)) return rc;
    if (int rc = post_scratch(c, fn, SCR_MOTION)) return rc;
    WeightArgs wa{};
    if (w) wa = WeightArgs{(const char *)w->base, (long long)w->item_stride, (long long)w->row_pitch};
    for (int k = 0; k < prm.iterations; k++) {
        const MotionPrior pr = k == 0 ? MotionPrior{(const char *)prior_dev, (long long)prior_stride}
                                      : MotionPrior{(const char *)models_dev, (long long)sizeof(ffl_motion_record)};
        ffl_launch_motion_fit(c->d_flow, t, n, c->w, c->h, w ? &wa : nullptr, pr, prm.tau, prm.model, c->d_mpsum,
                              (MotionRecord *)models_dev, k == prm.iterations - 1 ? sums_dev : nullptr, c->s_post);
    }
    return post_end(c, cst, n, slots);  // the caller may read the records, or overwrite the maps, on `stream` straight after the call
}

// k_motion_subtract into the dst slots, then the k_pass1 / k_pass1_final pair over them, on stream `post`: ffl_pass1_weighted's
// protocol over the src and the dst slots.  The dst slots hold a flow and an ordinary record afterwards.
int ffl_motion_subtract(ffl_ctx *c, int n, const int *src_slots, const int *dst_slots, const void *models_dev, ptrdiff_t model_stride,
                        int pov_mode, uint64_t stream) {
    static const char *fn = "ffl_motion_subtract";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post`, d_ptab and the pass-1 partials, as ffl_import_flows
    CtxLock lk(c->mu);
    if (n < 1 || n > c->max_batch)
        return set_err(c, FFL_ERR_INVALID, "%s: n = %d items outside 1..%d (the context's max_batch)", fn, n, c->max_batch);
    if (!src_slots || !dst_slots) return set_err(c, FFL_ERR_INVALID, "%s: NULL %s", fn, !src_slots ? "src_slots" : "dst_slots");
    if (int rc = check_flow_slots(c, fn, n, src_slots, "flow", "repeated among the src slots of one call")) return rc;
    if (int rc = check_flow_slots(c, fn, n, dst_slots, nullptr, "repeated among the dst slots of one call")) return rc;
    // the src slots are distinct: a dst slot that is a src slot and not its own item's is another item's
    int clash = -1;
    for (int i = 0; i < n; i++) c->slot_mark[src_slots[i]] = 1;
    for (int i = 0; i < n; i++)
        if (c->slot_mark[dst_slots[i]] && dst_slots[i] != src_slots[i] && clash < 0) clash = dst_slots[i];
    for (int i = 0; i < n; i++) c->slot_mark[src_slots[i]] = 0;
    if (clash >= 0) return set_err(c, FFL_ERR_INVALID, "%s: dst flow slot %d is another item's src slot", fn, clash);
    if (!models_dev) return set_err(c, FFL_ERR_INVALID, "%s: NULL models_dev", fn);
    if (int rc = model_array_check(c, fn, "models_dev", models_dev, model_stride)) return rc;
    int all[2 * FFL_MAXB], m = 0;   // every slot the call reads or writes, once
    ExportTab ts, td;
    for (int i = 0; i < n; i++) all[m++] = ts.slot[i] = src_slots[i];
    for (int i = 0; i < n; i++) {
        td.slot[i] = dst_slots[i];
        if (dst_slots[i] != src_slots[i]) all[m++] = dst_slots[i];
    }
    hipStream_t cst;
    const PostRegion reg{"models_dev", models_dev, (size_t)(n - 1) * (size_t)model_stride + 48, kHostModels};
    if (int rc = post_begin(c, fn, stream, &cst, &reg, 1, m, all)) return rc;
    ffl_launch_motion_subtract(c->d_flow, c->d_res, ts, td, n, c->w, c->h, (const char *)models_dev, (long long)model_stride, c->d_ptab,
                               c->s_post);
    {
        ProfScope ps(c, FFL_K_PASS1, c->s_post);
        ffl_launch_pass1(c->d_ptab, n, c->w, c->h, pov_mode ? 1 : 0, c->d_pskey, c->d_rpsum, c->s_post);
    }
    return post_end(c, cst, m, all);
}

// ---- flow import -------------------------------------------------------------------------------
// Every geometry rule of a device flow descriptor (ffl.h, ffl_dev_flow_check).  *mode: the load path of k_import_pass1
// (FFL_IMP_*); *bytes: the extent of all n items from f->base.
static int dev_flow_check(ffl_ctx *c, const char *fn, int dtype, int n, int w, int h, const ffl_dev_flow *f, int *mode,
                          size_t *bytes) {
    if (!f) return set_err(c, FFL_ERR_INVALID, "%s: NULL descriptor", fn);
    if (dtype != FFL_F32 && dtype != FFL_F16 && dtype != FFL_BF16)
        return set_err(c, FFL_ERR_INVALID, "%s: unknown dtype %d (FFL_F32 0, FFL_F16 1, FFL_BF16 2)", fn, dtype);
    if (n < 1) return set_err(c, FFL_ERR_INVALID, "%s: n = %d fields (>= 1)", fn, n);
    if (w < 2 || h < 2 || w > 32768 || h > 32768) return set_err(c, FFL_ERR_INVALID, "%s: size %dx%d outside 2..32768", fn, w, h);
    if (!f->base) return set_err(c, FFL_ERR_INVALID, "%s: NULL base", fn);
    const ptrdiff_t e = dtype == FFL_F32 ? 4 : 2, big = (ptrdiff_t)1 << 40;
    const ptrdiff_t it = f->item_stride, pitch = f->row_pitch, ps = f->pixel_stride, cs = f->channel_stride;
    if (it < 0 || pitch < 0 || ps < 0 || cs < 0)
        return set_err(c, FFL_ERR_INVALID, "%s: negative stride (item %td, row %td, pixel %td, channel %td)", fn, it, pitch, ps, cs);
    if (it > big || pitch > big || ps > big || cs > big) return set_err(c, FFL_ERR_INVALID, "%s: stride beyond 2^40", fn);
    if ((uintptr_t)f->base % e || it % e || pitch % e || ps % e || cs % e)
        return set_err(c, FFL_ERR_INVALID, "%s: misaligned: base and strides (item %td, row %td, pixel %td, channel %td) must be "
                                           "multiples of the element size %td", fn, it, pitch, ps, cs, e);
    // one component: pixels of a row apart, rows one after the other (a transposed view is refused)
    if (ps < e) return set_err(c, FFL_ERR_INVALID, "%s: overlap: pixel stride %td below the element size %td", fn, ps, e);
    const ptrdiff_t row = (ptrdiff_t)(w - 1) * ps + e, plane = (ptrdiff_t)(h - 1) * pitch + row;
    if (pitch < row) return set_err(c, FFL_ERR_INVALID, "%s: overlap: row pitch %td too small for %d pixels %td bytes apart", fn, pitch, w, ps);
    // u and v: interleaved inside a pixel, planar (v plane after the u plane), or row-planar (v row after the u row)
    const bool pixel = cs >= e && cs + e <= ps, planar = cs >= plane, rows = cs >= row && cs + row <= pitch;
    if (!pixel && !planar && !rows)
        return set_err(c, FFL_ERR_INVALID, "%s: overlap: channel stride %td makes u and v overlap (interleaved: %td <= channel "
                                           "stride <= pixel stride - %td; planar: >= %td; row-planar: %td .. row pitch - %td)",
                       fn, cs, e, e, plane, row, row);
    *bytes = (size_t)(n - 1) * (size_t)it + (size_t)(plane + cs);
    const bool al4 = (uintptr_t)f->base % 4 == 0 && pitch % 4 == 0 && it % 4 == 0;
    *mode = (ps == 2 * e && cs == e && (e == 4 || al4)) ? FFL_IMP_NHWC : (e == 4 && ps == 4) ? FFL_IMP_NCHW : FFL_IMP_ANY;
    return FFL_OK;
}

int ffl_dev_flow_check(int dtype, int n, int width, int height, const ffl_dev_flow *f) {
    int mode;
    size_t bytes;
    return dev_flow_check(nullptr, "ffl_dev_flow_check", dtype, n, width, height, f, &mode, &bytes);
}

// Caller device fields -> flow slots + their pass-1 records through ONE k_import_pass1 launch on stream `post`, ordered
// after the caller's queued work and the slots' last users, and before the caller's later work (the stream contract of
// ffl.h).  Slot indices travel as a kernel argument; nothing waits on the host beyond post_ring's own settling.
int ffl_import_flows(ffl_ctx *c, int n, const int *slots, const ffl_dev_flow *f, int dtype, int pov_mode, uint64_t stream) {
    static const char *fn = "ffl_import_flows";
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);  // stream `post` and post_ring, as ffl_radial / ffl_export_flows
    CtxLock lk(c->mu);
    ExportTab t;
    if (int rc = open_slot_list(c, fn, "fields", n, slots, nullptr, &t)) return rc;
    int mode;
    size_t bytes;
    if (int rc = dev_flow_check(c, fn, dtype, n, c->w, c->h, f, &mode, &bytes)) return rc;
    // stream `post` waits for the producer's queued work and for the last users of the slots (a batch, a pass 2, an export)
    hipStream_t cst;
    const PostRegion reg{"the flow fields", f->base, bytes, "host flow fields go through ffl_upload_flow"};
    if (int rc = post_begin(c, fn, stream, &cst, &reg, 1, n, slots)) return rc;
    const ImportArgs a{(const char *)f->base, (long long)f->item_stride, (long long)f->row_pitch, (long long)f->pixel_stride,
                       (long long)f->channel_stride, c->d_flow, c->d_res};
    {
        ProfScope ps(c, FFL_K_PASS1, c->s_post);
        ffl_launch_import_pass1(a, t, n, dtype, mode, c->w, c->h, pov_mode ? 1 : 0, c->d_ptab, c->d_pskey, c->d_rpsum,
                                c->s_post);
    }
    return post_end(c, cst, n, slots);  // the caller's later work (overwriting or freeing the sources) runs after the fields have been read
}

int ffl_upload_flow(ffl_ctx *c, int slot, const float *src, int pov_mode) {
    if (!c) return FFL_ERR_INVALID;
    std::unique_lock<std::mutex> pl(c->post_mu);
    CtxLock lk(c->mu);
    if (!flow_slot_ok(c, slot) || !src) return set_err(c, FFL_ERR_INVALID, "ffl_upload_flow: bad arguments");
    hipStream_t st = c->s_post;
    hipEvent_t ev = c->ev_slot_done[slot].get();  // the slot's last batch or pass 2 still reads or writes it
    if (int rc = wait_unlocked(c, lk, &ev, 1)) return rc;
    lk.unlock();
    hipError_t se = hipStreamSynchronize(st);  // the previous call's pass 1 has consumed the pinned table
    lk.lock();
    HIPCHK(c, se);
    HIPCHK(c, hipMemcpy(c->d_flow + (size_t)slot * 2 * c->N, src, sizeof(float) * 2 * c->N, hipMemcpyHostToDevice));
    c->h_ptab->flow[0][0] = c->d_flow + (size_t)slot * 2 * c->N;  // the stream was drained above: the pinned copy is free
    c->h_ptab->res[0] = c->d_res + slot;
    HIPCHK(c, hipMemcpyAsync(c->d_ptab, c->h_ptab, sizeof(PairTab), hipMemcpyHostToDevice, st));
    {
        ProfScope ps(c, FFL_K_PASS1, st);
        ffl_launch_pass1(c->d_ptab, 1, c->w, c->h, pov_mode, c->d_pskey, c->d_rpsum, st);
    }
    EvRef done;
    if (int rc = publish_post(c, 1, &slot, &done)) return rc;
    HIPCHK(c, hipGetLastError());
    return FFL_OK;
}

int ffl_submit_pair(ffl_ctx *c, int slot, const uint8_t *prev, const uint8_t *next, int width, int height, int channels,
                    ptrdiff_t stride_bytes, int pov_mode) {
    if (!c) return FFL_ERR_INVALID;
    // no lock around the three calls (each takes its own; holding `mu` here would invert the up_mu -> mu order): calls on
    // distinct slots from several threads interleave safely, n_fslots / n_slots are fixed at creation
    if (!flow_slot_ok(c, slot) || 2 * slot + 1 >= c->n_fslots) {
        CtxLock lk(c->mu);
        return set_err(c, FFL_ERR_INVALID, "ffl_submit_pair: slot %d needs frame slots %d,%d and a flow slot", slot, 2 * slot, 2 * slot + 1);
    }
    int rc = ffl_upload_frame(c, 2 * slot, prev, width, height, channels, stride_bytes);
    if (rc) return rc;
    rc = ffl_upload_frame(c, 2 * slot + 1, next, width, height, channels, stride_bytes);
    if (rc) return rc;
    int f0 = 2 * slot, f1 = 2 * slot + 1;
    return ffl_flow_pairs(c, 1, &f0, &f1, &slot, pov_mode);
}

int ffl_sync(ffl_ctx *c) {
    if (!c) return FFL_ERR_INVALID;
    // up_mu / post_mu: an upload or pass-2 call of another thread that is under way finishes queueing first, so the latest
    // events of streams `copy` and `post` stand for everything those calls put there.  All three locks are released for
    // the wait: it holds up no other thread.
    std::unique_lock<std::mutex> ul(c->up_mu);
    std::unique_lock<std::mutex> pl(c->post_mu);
    CtxLock lk(c->mu);
    std::vector<hipEvent_t> evs;
    evs.push_back(ev_latest(c->up_ring).get());
    for (auto &rb : c->raw)
        if (rb.busy) evs.push_back(rb.ev);
    for (auto &L : c->lanes) evs.push_back(ev_latest(L.ring).get());
    evs.push_back(ev_latest(c->post_ring).get());
    pl.unlock();
    ul.unlock();
    return wait_unlocked(c, lk, evs.data(), (int)evs.size());
}

// one knob of an option set, described by its row of kFflOptionRows; `live`: the set belongs to an existing context (its
// lane count is fixed).  What is more than a row: the fixed knobs, names that accept and read back one value and are no
// member of the set ("blur_tile_h": the box-sum order is anchored to blocks of 16 rows; "run_ahead" and "merge_expand":
// the frame-only kernels have one schedule, serial in the merged launches); "lanes" is a property of a live context's
// buffers.
static constexpr struct { const char *name; int value; } kFixedKnobs[] = {
    {"blur_tile_h", 16}, {"run_ahead", 0}, {"merge_expand", 1}};
static const int *fixed_knob(const char *name) {
    for (const auto &k : kFixedKnobs)
        if (!strcmp(name, k.name)) return &k.value;
    return nullptr;
}
static const FflOptionRow *option_row(const char *name) {
    for (const FflOptionRow &r : kFflOptionRows)
        if (!strcmp(name, r.name)) return &r;
    return nullptr;
}

static int set_option_impl(FflOptions &o, const char *name, int value, bool live) {
    if (const int *fixed = fixed_knob(name)) return value == *fixed ? FFL_OK : FFL_ERR_INVALID;
    const FflOptionRow *r = option_row(name);
    if (!r || value < r->lo || value > r->hi) return FFL_ERR_INVALID;
    if (live && r->member == &FflOptions::lanes) return value == o.lanes ? FFL_OK : FFL_ERR_STATE;
    o.*r->member = r->flag ? value != 0 : value;
    return FFL_OK;
}

static int get_option_impl(const FflOptions &o, const char *name, int *value) {
    const int *fixed = fixed_knob(name);
    const FflOptionRow *r = option_row(name);
    if (!fixed && !r) return FFL_ERR_INVALID;
    *value = fixed ? *fixed : o.*r->member;
    return FFL_OK;
}

int ffl_debug_blur_plan(int tiles_x, int tiles_y, int n_pairs, int slots, int blur_rows, int blur_min_wgs, int blur_taper,
                        int blur_taper_pairs, int tile_order, int *segments, int *n_segments, int *grid, int *blocks,
                        int max_blocks) {
    FflOptions o;
    if (tiles_x < 1 || tiles_y < 1 || n_pairs < 1 || n_pairs > FFL_MAXB || slots < 0 || !segments || !n_segments || !grid ||
        set_option_impl(o, "blur_rows", blur_rows, false) || set_option_impl(o, "blur_min_wgs", blur_min_wgs, false) ||
        set_option_impl(o, "blur_taper", blur_taper, false) || set_option_impl(o, "blur_taper_pairs", blur_taper_pairs, false) ||
        set_option_impl(o, "tile_order", tile_order, false))
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_debug_blur_plan: bad size, pair count, slot count, option value or NULL output");
    BlurPlan plan;
    const unsigned g = ffl_blur_plan(tiles_x, tiles_y, n_pairs, slots, o, &plan);
    *n_segments = plan.n;
    *grid = (int)g;
    for (int i = 0; i < FFL_BLUR_SEGS; i++) {
        const BlurSeg &s = plan.s[i];
        const int row[5] = {s.first_block, s.first_pair, s.pairs, s.nrb, s.strips};
        memcpy(segments + 5 * i, row, sizeof(row));
    }
    if (!blocks) return FFL_OK;
    if ((unsigned)max_blocks < g)
        return set_err(nullptr, FFL_ERR_INVALID, "ffl_debug_blur_plan: %u workgroups, room for %d", g, max_blocks);
    for (unsigned blk = 0; blk < g; blk++) {
        int b, tile_x, row0, nrb;
        int *out = blocks + 4 * (size_t)blk;
        if (ffl_blur_block(plan, blk, tiles_x, tile_order, b, tile_x, row0, nrb)) {
            out[0] = b; out[1] = tile_x; out[2] = row0; out[3] = std::max(0, std::min(nrb, tiles_y - row0));
        } else {
            out[0] = -1; out[1] = out[2] = out[3] = 0;
        }
    }
    return FFL_OK;
}

int ffl_set_option(const char *name, int value) {
    if (!name) return FFL_ERR_INVALID;
    std::lock_guard<std::mutex> g(g_opt_mu);
    return set_option_impl(g_opts, name, value, false);
}

int ffl_ctx_set_option(ffl_ctx *c, const char *name, int value) {
    if (!c || !name) return FFL_ERR_INVALID;
    CtxLock lk(c->mu);
    const int rc = set_option_impl(c->opt, name, value, true);
    if (rc == FFL_OK) c->opt_epoch++;  // only an option that was actually applied invalidates this context's captured graphs
    else if (rc == FFL_ERR_STATE) set_err(c, rc, "ffl_ctx_set_option: \"lanes\" is fixed once the context exists (%d)", c->opt.lanes);
    else set_err(c, rc, "ffl_ctx_set_option: unknown option or value out of range: %s = %d", name, value);
    return rc;
}

int ffl_ctx_get_option(ffl_ctx *c, const char *name, int *value) {
    if (!name || !value) return FFL_ERR_INVALID;
    if (!c) {
        std::lock_guard<std::mutex> g(g_opt_mu);
        return get_option_impl(g_opts, name, value);
    }
    CtxLock lk(c->mu);
    return get_option_impl(c->opt, name, value);
}

int ffl_graph_stats(ffl_ctx *c, int *captured, int *replayed, int *capture_failures) {
    if (!c) return FFL_ERR_INVALID;
    CtxLock lk(c->mu);
    if (captured) *captured = c->graph_captured;
    if (replayed) *replayed = c->graph_replayed;
    if (capture_failures) *capture_failures = c->graph_failed;
    return FFL_OK;
}

int ffl_profile_enable(ffl_ctx *c, unsigned class_mask) {
    if (!c) return FFL_ERR_INVALID;
    int rc = ffl_sync(c);  // before the context lock: ffl_sync takes up_mu / post_mu first (lock order)
    if (rc) return rc;
    CtxLock lk(c->mu);
    prof_collect(c);
    c->prof_mask = class_mask;
    return FFL_OK;
}

int ffl_profile_read(ffl_ctx *c, int k, int *launches, double *total_ms) {
    if (!c || k < 0 || k >= FFL_K_COUNT) return FFL_ERR_INVALID;
    int rc = ffl_sync(c);  // before the context lock (lock order up_mu -> post_mu -> mu)
    if (rc) return rc;
    CtxLock lk(c->mu);
    prof_collect(c);  // launches another thread queued since the sync are waited for here, under the lock (measurement hook)
    if (launches) *launches = c->prof_launches[k];
    if (total_ms) *total_ms = c->prof_ms[k];
    c->prof_launches[k] = 0;
    c->prof_ms[k] = 0;
    return FFL_OK;
}

}  // extern "C"
