// Input front-end (DESIGN.md sections 8, 11, 12): a decoded frame -> the gray operand of the pair
// kernel, in one pass.  Replaces, for the HIP backend, the reference's per-frame host work
//   cv2.cvtColor(BGR2RGB) FF:182, cv2.resize(frame, (256, 256)) FF:185-186 / cv2.resize(f, (512, 512)) +
//   crop f[256:, :256] FF:1076-1079, cv2.cvtColor(RGB2GRAY) FF:1079/1082.
// Every output pixel of the crop window is computed directly from its (up to) 4 source pixels with
// OpenCV's 8-bit fixed-point rules (11-bit lerp weights, 15-bit luma weights) -- integer work, so the
// result is bit-identical to the two-pass CPU restatements in oracle/frontend_oracle.c and tests/yuv_ref.py.
// The source is described by a FrameDesc: packed or planar BGR / RGB with any row pitch, pixel stride and channel stride,
// 4:2:0 YUV (I420, NV12) in 8-bit or 9- to 16-bit samples, or gray copied as it is.  A stream's display rotation and
// mirroring (rule Y6) are an index permutation applied where a source pixel is fetched, its colour range (rule Y7) a choice
// of integers there: what cv2.VideoCapture.read applies before the reference sees a pixel (FF:178).  Both entry points run
// the one per-pixel body; they differ only in where the descriptor comes from:
//   k_frontend      ffl_upload_frames_raw / ffl_upload_frames_yuv / _yuv16: one frame in a staging buffer, descriptor by value
//   k_frontend_dev  ffl_upload_frames_device / _device16: one launch for n frames in caller memory, descriptor tab[blockIdx.z]
// k_frontend_remap / k_frontend_remap_dev are the same pair for ffl_upload_frames_remap / _device_remap: the operand is
// gathered through a per-pixel source map instead of the resize + crop (a pinhole view, an undistortion; section 20).
// Roofline: HBM / PCIe -- the kernel touches at most 12 source bytes per output pixel; on the host paths the frame's
// H2D transfer is what bounds the path.
#include "ffl_kernels.h"

__device__ __forceinline__ int ffl_sat_short_round(float v) {
    int r = (int)rintf(v);  // round half to even (cvRound)
    return min(max(r, -32768), 32767);
}

__device__ __forceinline__ int ffl_sat_u8(int v) { return min(max(v, 0), 255); }

// Rule Y6 (appendix Y): upright pixel (x, y) -> the stored pixel that holds it, through the integer affine map
// front_geometry() forms (coefficients in {-1, 0, 1}).  S: the launch carries stream metadata (p.src); without it the
// map is the identity and costs nothing.
template <bool S>
__device__ __forceinline__ void ffl_front_map(const FrontParams &p, int &x, int &y) {
    if (S) {
        const int ux = x, uy = y;
        x = p.ax * ux + p.bx * uy + p.cx0;
        y = p.ay * ux + p.by * uy + p.cy0;
    }
}

// The three colour channels of upright source pixel (sx, sy) in the order the frame stores them (BGR, RGB, or B, G, R out
// of YUV).  (sx, sy) is in full-frame upright terms; rule Y6 turns it into the stored pixel, and the origin of the window
// the planes hold (stored terms) is only subtracted at the load.  K is the source kind, or FFL_SRC_ANY: p.kind, tested
// here.  YUV: BT.601 limited range, OpenCV's 20-bit fixed point, nearest chroma (appendix Y) -- with S and p.full rule
// Y7 instead: one wave-uniform choice of the luma offset, the luma gain and the four chroma integers.  YUV16: the same
// from 16-bit samples, each reduced to 8 bits at its load by rule Y5 -- round half up with saturation; the alignment's
// own shift is folded into p.shift16 on the host, so one add and one shift do it.
template <int K, bool S>
__device__ __forceinline__ void ffl_front_fetch(const FrameDesc &d, const FrontParams &p, int sx, int sy, int c3[3]) {
    const int kind = K == FFL_SRC_ANY ? p.kind : K;
    ffl_front_map<S>(p, sx, sy);
    if (kind == FFL_SRC_YUV || kind == FFL_SRC_YUV16) {
        const long long cy = (sy >> 1) - (d.wy >> 1), cx = (long long)((sx >> 1) - (d.wx >> 1)) * d.c_step;
        int Y, u, v;
        if (kind == FFL_SRC_YUV16) {  // pitches and c_step stay in bytes; every address is even
            const int y16 = *(const uint16_t *)(d.p0 + (long long)(sy - d.wy) * d.pitch0 + 2LL * (sx - d.wx));
            const int u16 = *(const uint16_t *)(d.p1 + cy * d.pitch1 + cx), v16 = *(const uint16_t *)(d.p2 + cy * d.pitch2 + cx);
            Y = min((y16 + p.round16) >> p.shift16, 255);
            u = min((u16 + p.round16) >> p.shift16, 255) - 128;
            v = min((v16 + p.round16) >> p.shift16, 255) - 128;
        } else {
            Y = d.p0[(long long)(sy - d.wy) * d.pitch0 + (sx - d.wx)];
            u = d.p1[cy * d.pitch1 + cx] - 128;
            v = d.p2[cy * d.pitch2 + cx] - 128;
        }
        const bool full = S && p.full;  // rule Y7: no offset, no 255/219 gain, the JFIF integers
        const int yh = max(Y - (full ? 0 : 16), 0) * (full ? 1 << 20 : 1220542) + (1 << 19);
        c3[0] = ffl_sat_u8((yh + (full ? 1858077 : 2116026) * u) >> 20);
        c3[1] = ffl_sat_u8((yh - (full ? 748826 : 852492) * v - (full ? 360853 : 409993) * u) >> 20);
        c3[2] = ffl_sat_u8((yh + (full ? 1470104 : 1673527) * v) >> 20);
    } else {
        const uint8_t *s = d.p0 + (long long)(sy - d.wy) * d.pitch0 + (long long)(sx - d.wx) * d.ps;
        c3[0] = s[0];
        c3[1] = s[d.cs];
        c3[2] = s[2 * d.cs];
    }
}

// Output pixel (x, y) of the crop window from a BGR / RGB or YUV source of kind K (FFL_SRC_ANY: p.kind).  Everything here
// is in upright terms (p.sw x p.sh is the upright size); only the fetch knows about rule Y6.  Where the kind is tested
// decides when the compiler waits for the taps' loads, and each launch keeps the form it was measured fastest in:
// k_frontend instantiates the body per kind, so every tap's loads are issued before the first wait (testing the kind in
// each fetch made it wait tap by tap: +0.8 us per 4:2:0 launch); k_frontend_dev tests it in each fetch (per-kind bodies
// made its 64-frame launch from 4K BGR frames 6 % slower).  S (the launch carries stream metadata: rotation, mirroring,
// full range) is a template parameter of both kernels too: launches without metadata run the S = false instantiations,
// whose code is what it was before rules Y6 / Y7 existed; those with metadata take the map and the Y7 integers as
// uniform operands of one S = true body per kernel, with the kind tested in each fetch.  Measured against giving every
// launch the uniform operands (S = true for all): that form cost the unoriented 4:2:0 k_frontend launch 1.0 us (6.4 ->
// 7.4 us, 1080p NV12 into 256x256) and left the others within 1 %.
template <int K, bool S>
__device__ __forceinline__ void ffl_front_resample(const FrameDesc &d, const FrontParams &p, uint8_t *gray, int x, int y) {
    const int dx = x + p.cx, dy = y + p.cy;  // position in the (virtual) resized image
    int v[3];
    if (p.mode == FFL_FRONT_IDENTITY) {
        ffl_front_fetch<K, S>(d, p, dx, dy, v);
    } else if (p.mode == FFL_FRONT_AREA2) {  // exact 2x2 down-scale: INTER_LINEAR is routed to INTER_AREA
        int s00[3], s01[3], s10[3], s11[3];
        ffl_front_fetch<K, S>(d, p, 2 * dx, 2 * dy, s00);
        ffl_front_fetch<K, S>(d, p, 2 * dx + 1, 2 * dy, s01);
        ffl_front_fetch<K, S>(d, p, 2 * dx, 2 * dy + 1, s10);
        ffl_front_fetch<K, S>(d, p, 2 * dx + 1, 2 * dy + 1, s11);
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = (s00[c] + s01[c] + s10[c] + s11[c] + 2) >> 2;
    } else {
        float fx = (float)((dx + 0.5) * p.scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= sx;
        if (sx < 0) { sx = 0; fx = 0.f; }
        if (sx >= p.sw - 1) { sx = p.sw - 1; fx = 0.f; }
        const int sx1 = min(sx + 1, p.sw - 1);
        const int a0 = ffl_sat_short_round((1.f - fx) * 2048.f), a1 = ffl_sat_short_round(fx * 2048.f);
        float fy = (float)((dy + 0.5) * p.scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= sy;
        const int b0 = ffl_sat_short_round((1.f - fy) * 2048.f), b1 = ffl_sat_short_round(fy * 2048.f);
        const int y0 = min(max(sy, 0), p.sh - 1), y1 = min(max(sy + 1, 0), p.sh - 1);
        int s00[3], s01[3], s10[3], s11[3];
        ffl_front_fetch<K, S>(d, p, sx, y0, s00);
        ffl_front_fetch<K, S>(d, p, sx1, y0, s01);
        ffl_front_fetch<K, S>(d, p, sx, y1, s10);
        ffl_front_fetch<K, S>(d, p, sx1, y1, s11);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int h0 = s00[c] * a0 + s01[c] * a1;
            const int h1 = s10[c] * a0 + s11[c] * a1;
            v[c] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        }
    }
    const int r = p.rgb ? v[0] : v[2], b = p.rgb ? v[2] : v[0];
    gray[(size_t)y * p.ow + x] = (uint8_t)((r * 9798 + v[1] * 19235 + b * 3735 + 16384) >> 15);
}

// One output pixel per lane in 64x4 workgroups.  S = false is the kernel every launch without metadata runs: its code is
// what it was before S existed.
template <bool S>
__global__ __launch_bounds__(256) void k_frontend(FrameDesc d, uint8_t *__restrict__ gray, FrontParams p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= p.ow || y >= p.oh) return;
    if (S) ffl_front_resample<FFL_SRC_ANY, true>(d, p, gray, x, y);
    else if (p.kind == FFL_SRC_YUV) ffl_front_resample<FFL_SRC_YUV, false>(d, p, gray, x, y);
    else if (p.kind == FFL_SRC_YUV16) ffl_front_resample<FFL_SRC_YUV16, false>(d, p, gray, x, y);
    else ffl_front_resample<FFL_SRC_BGR, false>(d, p, gray, x, y);
}

// grid = output tiles x frames; the frame's descriptor is read with a wave-uniform index.
template <bool S>
__global__ __launch_bounds__(256) void k_frontend_dev(const FrameDesc *__restrict__ tab, uint8_t *__restrict__ gray_base,
                                                      size_t N, FrontParams p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= p.ow || y >= p.oh) return;
    const FrameDesc d = tab[blockIdx.z];
    uint8_t *gray = gray_base + (size_t)d.fslot * N;
    if (p.kind == FFL_SRC_GRAY) {  // the context's size (upright), copied as it is
        int sx = x, sy = y;
        ffl_front_map<S>(p, sx, sy);
        gray[(size_t)y * p.ow + x] = d.p0[(long long)sy * d.pitch0 + (long long)sx * d.ps];
    } else {
        ffl_front_resample<FFL_SRC_ANY, S>(d, p, gray, x, y);
    }
}

// Map-driven reprojection (rules R2 to R5 are stated in include/ffl.h): output pixel
// (x, y) is the rounded mean of its ss x ss samples, each a bilinear blend (5 fractional bits, 10-bit weight products) of the
// four taps a map entry names in upright 1/32 px -- the taps are ffl_front_fetch's, so rules Y5, Y6 and Y7 apply where a tap
// is loaded and the map never sees how a frame is stored.  The map was checked on the host (rule R1): no tap is
// range-checked here.  An entry is one 8-byte load; the lanes of a wave read consecutive entries of a sample row (ss = 1)
// or entries ss apart.  Nothing the resize kernels read was added for this: the map and ss travel in RemapParams, and of
// FrontParams only the source description (kind, rgb, sw, sh, ow, oh, rules Y5 to Y7) is used.  Gray sources have one channel,
// stored as it is.
template <int K, bool S>
__device__ __forceinline__ void ffl_front_remap(const FrameDesc &d, const FrontParams &p, const RemapParams &r, uint8_t *gray,
                                                int x, int y) {
    const int kind = K == FFL_SRC_ANY ? p.kind : K;
    const int NC = 3;
    int acc[NC] = {0, 0, 0};
    const size_t W = (size_t)r.ss * p.ow;
    const int2 *row = r.map + (size_t)y * r.ss * W + (size_t)x * r.ss;
    for (int j = 0; j < r.ss; j++, row += W) {
        for (int i = 0; i < r.ss; i++) {
            const int2 q = row[i];
            if (q.x == FFL_REMAP_NONE) continue;  // rule R4: no source, 0 in every channel
            const int x0 = q.x >> 5, fx = q.x & 31, x1 = min(x0 + 1, p.sw - 1);
            const int y0 = q.y >> 5, fy = q.y & 31, y1 = min(y0 + 1, p.sh - 1);
            const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
            if (kind == FFL_SRC_GRAY) {
                int tx[4] = {x0, x1, x0, x1}, ty[4] = {y0, y0, y1, y1}, s[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    ffl_front_map<S>(p, tx[k], ty[k]);
                    s[k] = d.p0[(long long)ty[k] * d.pitch0 + (long long)tx[k] * d.ps];
                }
                acc[0] += (s[0] * w00 + s[1] * w01 + s[2] * w10 + s[3] * w11 + 512) >> 10;
            } else {
                int s00[3], s01[3], s10[3], s11[3];
                ffl_front_fetch<K, S>(d, p, x0, y0, s00);
                ffl_front_fetch<K, S>(d, p, x1, y0, s01);
                ffl_front_fetch<K, S>(d, p, x0, y1, s10);
                ffl_front_fetch<K, S>(d, p, x1, y1, s11);
#pragma unroll
                for (int c = 0; c < NC; c++) acc[c] += (s00[c] * w00 + s01[c] * w01 + s10[c] * w10 + s11[c] * w11 + 512) >> 10;
            }
        }
    }
    const int half = (r.ss * r.ss) >> 1, sh = 2 * r.lg;  // rule R5
    int v[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) v[c] = (acc[c] + half) >> sh;
    if (kind == FFL_SRC_GRAY) {
        gray[(size_t)y * p.ow + x] = (uint8_t)v[0];
        return;
    }
    const int rr = p.rgb ? v[0] : v[2], b = p.rgb ? v[2] : v[0];
    gray[(size_t)y * p.ow + x] = (uint8_t)((rr * 9798 + v[1] * 19235 + b * 3735 + 16384) >> 15);
}

// The two entry points mirror k_frontend / k_frontend_dev: the same 64x4 workgroups, one output pixel per lane, the
// descriptor by value (host frames, a body per kind without metadata) or tab[blockIdx.z] (device frames, the kind tested in
// each fetch).
template <bool S>
__global__ __launch_bounds__(256) void k_frontend_remap(FrameDesc d, uint8_t *__restrict__ gray, FrontParams p, RemapParams r) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= p.ow || y >= p.oh) return;
    if (S) ffl_front_remap<FFL_SRC_ANY, true>(d, p, r, gray, x, y);
    else if (p.kind == FFL_SRC_YUV) ffl_front_remap<FFL_SRC_YUV, false>(d, p, r, gray, x, y);
    else if (p.kind == FFL_SRC_YUV16) ffl_front_remap<FFL_SRC_YUV16, false>(d, p, r, gray, x, y);
    else ffl_front_remap<FFL_SRC_BGR, false>(d, p, r, gray, x, y);
}

template <bool S>
__global__ __launch_bounds__(256) void k_frontend_remap_dev(const FrameDesc *__restrict__ tab, uint8_t *__restrict__ gray_base,
                                                            size_t N, FrontParams p, RemapParams r) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= p.ow || y >= p.oh) return;
    const FrameDesc d = tab[blockIdx.z];
    ffl_front_remap<FFL_SRC_ANY, S>(d, p, r, gray_base + (size_t)d.fslot * N, x, y);
}

void ffl_launch_frontend(const FrameDesc &d, uint8_t *gray, const FrontParams &p, hipStream_t st) {
    dim3 grid((p.ow + 63) / 64, (p.oh + 3) / 4);
    if (p.src) hipLaunchKernelGGL(k_frontend<true>, grid, dim3(256), 0, st, d, gray, p);
    else hipLaunchKernelGGL(k_frontend<false>, grid, dim3(256), 0, st, d, gray, p);
}

void ffl_launch_frontend_dev(const FrameDesc *tab, int n, uint8_t *gray_base, size_t N, const FrontParams &p, hipStream_t st) {
    dim3 grid((p.ow + 63) / 64, (p.oh + 3) / 4, n);
    if (p.src) hipLaunchKernelGGL(k_frontend_dev<true>, grid, dim3(256), 0, st, tab, gray_base, N, p);
    else hipLaunchKernelGGL(k_frontend_dev<false>, grid, dim3(256), 0, st, tab, gray_base, N, p);
}

void ffl_launch_frontend_remap(const FrameDesc &d, uint8_t *gray, const FrontParams &p, const RemapParams &r, hipStream_t st) {
    dim3 grid((p.ow + 63) / 64, (p.oh + 3) / 4);
    if (p.src) hipLaunchKernelGGL(k_frontend_remap<true>, grid, dim3(256), 0, st, d, gray, p, r);
    else hipLaunchKernelGGL(k_frontend_remap<false>, grid, dim3(256), 0, st, d, gray, p, r);
}

void ffl_launch_frontend_remap_dev(const FrameDesc *tab, int n, uint8_t *gray_base, size_t N, const FrontParams &p,
                                   const RemapParams &r, hipStream_t st) {
    dim3 grid((p.ow + 63) / 64, (p.oh + 3) / 4, n);
    if (p.src) hipLaunchKernelGGL(k_frontend_remap_dev<true>, grid, dim3(256), 0, st, tab, gray_base, N, p, r);
    else hipLaunchKernelGGL(k_frontend_remap_dev<false>, grid, dim3(256), 0, st, tab, gray_base, N, p, r);
}
