// Device-memory I/O: frames read in place from caller device memory, flow fields written to it.
//
// k_frontend_dev is the per-pixel arithmetic of k_frontend (BGR / RGB) and k_frontend_yuv (I420 / NV12) with the source
// addressed through a per-frame descriptor -- any row pitch, pixel stride and channel stride -- instead of a packed
// staging copy, plus a gray copy.  One launch covers every frame of a call: grid = output tiles x frames, one output
// pixel per lane, the frame's descriptor read with a wave-uniform index.  The rules are the host paths' to the bit:
// 11-bit lerp weights, the 2x2 mean of an exact 2x down-scale, identity, 15-bit luma; 4:2:0 as appendix Y with the
// window being the whole frame.  Roofline: at most 12 source bytes and 1 byte written per output pixel -- a 256x256
// operand from any source is a few us; the frame is never copied.
//
// k_export_flows gathers flow slots into caller memory: (H, W, 2) with 16-byte copies, or (2, H, W) de-interleaved with
// 16-byte loads and stores on both sides.  Pure bandwidth.
#include "ffl_kernels.h"

__device__ __forceinline__ int ffl_dev_sat_short_round(float v) {
    int r = (int)rintf(v);  // round half to even (cvRound)
    return min(max(r, -32768), 32767);
}

__device__ __forceinline__ int ffl_dev_sat_u8(int v) { return min(max(v, 0), 255); }

// the three colour channels of source pixel (sx, sy) in the order the frame stores them (BGR, RGB, or B,G,R from YUV)
__device__ __forceinline__ void ffl_dev_fetch(const DevFrameDesc &d, int kind, int sx, int sy, int c3[3]) {
    if (kind == FFL_DEVK_YUV) {  // BT.601 limited range, OpenCV's 20-bit fixed point, nearest chroma (appendix Y)
        const int Y = d.p0[(long long)sy * d.pitch0 + sx];
        const long long cx = (long long)(sx >> 1) * d.c_step;
        const int u = d.p1[(long long)(sy >> 1) * d.pitch1 + cx] - 128, v = d.p2[(long long)(sy >> 1) * d.pitch2 + cx] - 128;
        const int yh = max(Y - 16, 0) * 1220542 + (1 << 19);
        c3[0] = ffl_dev_sat_u8((yh + 2116026 * u) >> 20);
        c3[1] = ffl_dev_sat_u8((yh - 852492 * v - 409993 * u) >> 20);
        c3[2] = ffl_dev_sat_u8((yh + 1673527 * v) >> 20);
    } else {
        const uint8_t *s = d.p0 + (long long)sy * d.pitch0 + (long long)sx * d.ps;
        c3[0] = s[0];
        c3[1] = s[d.cs];
        c3[2] = s[2 * d.cs];
    }
}

__global__ __launch_bounds__(256) void k_frontend_dev(const DevFrameDesc *__restrict__ tab, uint8_t *__restrict__ gray_base,
                                                      size_t N, DevFrontParams p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= p.ow || y >= p.oh) return;
    const DevFrameDesc d = tab[blockIdx.z];
    uint8_t *gray = gray_base + (size_t)d.fslot * N;
    if (p.kind == FFL_DEVK_GRAY) {  // the context's size, copied as it is
        gray[(size_t)y * p.ow + x] = d.p0[(long long)y * d.pitch0 + (long long)x * d.ps];
        return;
    }
    const int dx = x + p.cx, dy = y + p.cy;  // position in the (virtual) resized image
    int v[3];
    if (p.mode == FFL_FRONT_IDENTITY) {
        ffl_dev_fetch(d, p.kind, dx, dy, v);
    } else if (p.mode == FFL_FRONT_AREA2) {  // exact 2x2 down-scale: INTER_LINEAR is routed to INTER_AREA
        int s00[3], s01[3], s10[3], s11[3];
        ffl_dev_fetch(d, p.kind, 2 * dx, 2 * dy, s00);
        ffl_dev_fetch(d, p.kind, 2 * dx + 1, 2 * dy, s01);
        ffl_dev_fetch(d, p.kind, 2 * dx, 2 * dy + 1, s10);
        ffl_dev_fetch(d, p.kind, 2 * dx + 1, 2 * dy + 1, s11);
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] = (s00[c] + s01[c] + s10[c] + s11[c] + 2) >> 2;
    } else {
        float fx = (float)((dx + 0.5) * p.scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= sx;
        if (sx < 0) { sx = 0; fx = 0.f; }
        if (sx >= p.sw - 1) { sx = p.sw - 1; fx = 0.f; }
        const int sx1 = min(sx + 1, p.sw - 1);
        const int a0 = ffl_dev_sat_short_round((1.f - fx) * 2048.f), a1 = ffl_dev_sat_short_round(fx * 2048.f);
        float fy = (float)((dy + 0.5) * p.scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= sy;
        const int b0 = ffl_dev_sat_short_round((1.f - fy) * 2048.f), b1 = ffl_dev_sat_short_round(fy * 2048.f);
        const int y0 = min(max(sy, 0), p.sh - 1), y1 = min(max(sy + 1, 0), p.sh - 1);
        int s00[3], s01[3], s10[3], s11[3];
        ffl_dev_fetch(d, p.kind, sx, y0, s00);
        ffl_dev_fetch(d, p.kind, sx1, y0, s01);
        ffl_dev_fetch(d, p.kind, sx, y1, s10);
        ffl_dev_fetch(d, p.kind, sx1, y1, s11);
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

void ffl_launch_frontend_dev(const DevFrameDesc *tab, int n, uint8_t *gray_base, size_t N, DevFrontParams p, hipStream_t st) {
    dim3 grid((p.ow + 63) / 64, (p.oh + 3) / 4, n);
    hipLaunchKernelGGL(k_frontend_dev, grid, dim3(256), 0, st, tab, gray_base, N, p);
}

// ---- flow export ----------------------------------------------------------------------------------------------------
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
