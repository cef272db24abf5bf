// Input front-end: decoded 3-channel u8 frame -> the gray operand of the pair
// kernel, in one pass.  Replaces, for the HIP backend, the reference's per-frame host work
//   cv2.cvtColor(BGR2RGB) FF:182, cv2.resize(frame, (256, 256)) FF:185-186 / cv2.resize(f, (512, 512)) +
//   crop f[256:, :256] FF:1076-1079, cv2.cvtColor(RGB2GRAY) FF:1079/1082.
// Every output pixel of the crop window is computed directly from its (up to) 4 source pixels with
// OpenCV's 8-bit fixed-point rules (11-bit lerp weights, 15-bit luma weights) -- integer work, so the
// result is bit-identical to the two-pass CPU restatement in oracle/frontend_oracle.c.
// Roofline: HBM / PCIe -- the kernel touches at most 12 source bytes per output pixel; the frame's
// H2D transfer (3 * src_w * src_h bytes) is what bounds the path.
#include "ffl_kernels.h"

__device__ __forceinline__ int ffl_sat_short_round(float v) {
    int r = (int)rintf(v);  // round half to even (cvRound)
    return min(max(r, -32768), 32767);
}

__global__ __launch_bounds__(256) void k_frontend(const uint8_t *__restrict__ src, uint8_t *__restrict__ gray,
                                                  FrontParams p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= p.ow || y >= p.oh) return;
    const int dx = x + p.cx, dy = y + p.cy;  // position in the (virtual) resized image
    int v[3];
    if (p.mode == FFL_FRONT_IDENTITY) {
        const uint8_t *s = src + (size_t)dy * p.stride + 3 * dx;
        v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
    } else if (p.mode == FFL_FRONT_AREA2) {  // exact 2x2 down-scale: INTER_LINEAR is routed to INTER_AREA
        const uint8_t *s0 = src + (size_t)(2 * dy) * p.stride + 6 * dx, *s1 = s0 + p.stride;
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = (s0[c] + s0[3 + c] + s1[c] + s1[3 + c] + 2) >> 2;
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
        const uint8_t *S0 = src + (size_t)y0 * p.stride, *S1 = src + (size_t)y1 * p.stride;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int h0 = S0[3 * sx + c] * a0 + S0[3 * sx1 + c] * a1;
            const int h1 = S1[3 * sx + c] * a0 + S1[3 * sx1 + c] * a1;
            v[c] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        }
    }
    const int r = p.rgb ? v[0] : v[2], b = p.rgb ? v[2] : v[0];
    gray[(size_t)y * p.ow + x] = (uint8_t)((r * 9798 + v[1] * 19235 + b * 3735 + 16384) >> 15);
}

void ffl_launch_frontend(const uint8_t *src, uint8_t *gray, FrontParams p, hipStream_t st) {
    dim3 grid((p.ow + 63) / 64, (p.oh + 3) / 4);
    hipLaunchKernelGGL(k_frontend, grid, dim3(256), 0, st, src, gray, p);
}

// ---- 4:2:0 YUV input --------------------------------------------------------------
// k_frontend_yuv is k_frontend with a YUV->BGR conversion in front of every source pixel it reads: BT.601 limited range
// in OpenCV's 20-bit fixed point, chroma nearest (the U, V samples at (x >> 1, y >> 1)).  The resize and luma integer
// arithmetic are k_frontend's.  The source is the window [wx, wx + window) x [wy, ...) of the frame that went to the
// device: coordinates and clamps are computed in full-frame terms and the window origin is only subtracted at the load.
__device__ __forceinline__ int ffl_sat_u8(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ void ffl_yuv_bgr(const uint8_t *__restrict__ py, const uint8_t *__restrict__ pu,
                                            const uint8_t *__restrict__ pv, const FrontYuvParams &p, int sx, int sy,
                                            int bgr[3]) {
    const int Y = py[(size_t)(sy - p.wy) * p.y_pitch + (sx - p.wx)];
    const size_t co = (size_t)((sy >> 1) - (p.wy >> 1)) * p.c_pitch + (size_t)((sx >> 1) - (p.wx >> 1)) * p.c_step;
    const int u = pu[co] - 128, v = pv[co] - 128;
    const int yh = max(Y - 16, 0) * 1220542 + (1 << 19);
    bgr[0] = ffl_sat_u8((yh + 2116026 * u) >> 20);
    bgr[1] = ffl_sat_u8((yh - 852492 * v - 409993 * u) >> 20);
    bgr[2] = ffl_sat_u8((yh + 1673527 * v) >> 20);
}

__global__ __launch_bounds__(256) void k_frontend_yuv(const uint8_t *__restrict__ py, const uint8_t *__restrict__ pu,
                                                      const uint8_t *__restrict__ pv, uint8_t *__restrict__ gray,
                                                      FrontYuvParams p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= p.ow || y >= p.oh) return;
    const int dx = x + p.cx, dy = y + p.cy;  // position in the (virtual) resized image
    int v[3];
    if (p.mode == FFL_FRONT_IDENTITY) {
        ffl_yuv_bgr(py, pu, pv, p, dx, dy, v);
    } else if (p.mode == FFL_FRONT_AREA2) {  // exact 2x2 down-scale: INTER_LINEAR is routed to INTER_AREA
        int s00[3], s01[3], s10[3], s11[3];
        ffl_yuv_bgr(py, pu, pv, p, 2 * dx, 2 * dy, s00);
        ffl_yuv_bgr(py, pu, pv, p, 2 * dx + 1, 2 * dy, s01);
        ffl_yuv_bgr(py, pu, pv, p, 2 * dx, 2 * dy + 1, s10);
        ffl_yuv_bgr(py, pu, pv, p, 2 * dx + 1, 2 * dy + 1, s11);
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
        ffl_yuv_bgr(py, pu, pv, p, sx, y0, s00);
        ffl_yuv_bgr(py, pu, pv, p, sx1, y0, s01);
        ffl_yuv_bgr(py, pu, pv, p, sx, y1, s10);
        ffl_yuv_bgr(py, pu, pv, p, sx1, y1, s11);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int h0 = s00[c] * a0 + s01[c] * a1;
            const int h1 = s10[c] * a0 + s11[c] * a1;
            v[c] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        }
    }
    gray[(size_t)y * p.ow + x] = (uint8_t)((v[2] * 9798 + v[1] * 19235 + v[0] * 3735 + 16384) >> 15);
}

void ffl_launch_frontend_yuv(const uint8_t *y, const uint8_t *u, const uint8_t *v, uint8_t *gray, FrontYuvParams p,
                             hipStream_t st) {
    dim3 grid((p.ow + 63) / 64, (p.oh + 3) / 4);
    hipLaunchKernelGGL(k_frontend_yuv, grid, dim3(256), 0, st, y, u, v, gray, p);
}
