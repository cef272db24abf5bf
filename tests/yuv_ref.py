"""numpy restatement of DESIGN.md appendix Y: 4:2:0 (I420 / NV12) -> BGR as the YUV front-end converts it, composed with
the oracle's resize and luma (oracle/frontend_oracle.c) into the gray operand ffl_upload_frames_yuv must produce.

    operand = gray( resize( cvtColor(frame, COLOR_YUV2BGR_I420 | COLOR_YUV2BGR_NV12), (rw, rh) ) [crop window] )

The conversion is BT.601 limited range in OpenCV's 20-bit fixed point as recalled (no OpenCV source or cv2 to check it
against): chroma nearest, y = max(0, Y - 16) * 1220542, R = sat((y + 2^19 + 1673527 v) >> 20),
G = sat((y + 2^19 - 852492 v - 409993 u) >> 20), B = sat((y + 2^19 + 2116026 u) >> 20), u = U - 128, v = V - 128."""
import numpy as np

import oracle as orc

LAYOUTS = ("i420", "nv12")


def planes(frame, layout):
    """(Y, U, V) views of a (3h/2, w) uint8 4:2:0 frame (an NV12 frame's rows may be strided)"""
    if layout not in LAYOUTS:
        raise ValueError(layout)
    h, w = frame.shape[0] * 2 // 3, frame.shape[1]
    if frame.shape[0] != h * 3 // 2 or h % 2 or w % 2:
        raise ValueError(f"not a 4:2:0 frame with even sides: {frame.shape}")
    y = frame[:h]
    if layout == "nv12":
        uv = frame[h:]
        return y, uv[:, 0::2], uv[:, 1::2]
    flat = np.ascontiguousarray(frame).reshape(-1)
    q = (h // 2) * (w // 2)
    return y, flat[h * w:h * w + q].reshape(h // 2, w // 2), flat[h * w + q:h * w + 2 * q].reshape(h // 2, w // 2)


def yuv_to_bgr_pixels(Y, U, V):
    """appendix Y on integer arrays of equal shape -> (..., 3) uint8 BGR"""
    y = np.maximum(np.asarray(Y, np.int32) - 16, 0) * 1220542 + (1 << 19)
    u, v = np.asarray(U, np.int32) - 128, np.asarray(V, np.int32) - 128
    b = (y + 2116026 * u) >> 20
    g = (y - 852492 * v - 409993 * u) >> 20
    r = (y + 1673527 * v) >> 20
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def yuv_to_bgr(frame, layout):
    """cvtColor(frame, COLOR_YUV2BGR_I420 | COLOR_YUV2BGR_NV12) as appendix Y states it: (h, w, 3) uint8"""
    Y, U, V = planes(frame, layout)
    up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1)   # noqa: E731 -- chroma nearest: (x >> 1, y >> 1)
    return yuv_to_bgr_pixels(Y, up(U), up(V))


def operand(frame, layout, resize, crop=(0, 0), out_size=(256, 256)):
    """the gray operand of ffl_upload_frames_yuv(frame, layout, resize, crop) on an out_size context"""
    rgb = orc.swap_rb(yuv_to_bgr(frame, layout))
    if (rgb.shape[1], rgb.shape[0]) != tuple(resize):
        rgb = orc.resize_linear_u8c3(rgb, int(resize[0]), int(resize[1]))
    (cx, cy), (ow, oh) = crop, out_size
    return orc.rgb2gray(rgb[cy:cy + oh, cx:cx + ow])


def source_span(d0, d1, s, r):
    """sorted source coordinates (one axis, length s) the resize to r reads for output coordinates d0..d1, zero-weight
    taps included: what k_frontend / k_frontend_yuv load (identity; exact 2x -> 2x2 mean; else the two lerp taps)"""
    d = np.arange(d0, d1 + 1)
    if r == s:
        return d
    if s == 2 * r:
        return np.unique(np.concatenate([2 * d, 2 * d + 1]))
    scale = 1. / (float(r) / s)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(f).astype(np.int64)
    sx = np.clip(sx, 0, s - 1)
    return np.unique(np.concatenate([sx, np.minimum(sx + 1, s - 1)]))


def random_frame(w, h, layout, seed, pitch=None):
    """a random (3h/2, w) 4:2:0 frame; pitch > w (NV12 only): a view of a wider buffer"""
    rng = np.random.default_rng(seed)
    if pitch is None or pitch == w:
        return rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8)
    return rng.integers(0, 256, (h * 3 // 2, pitch), dtype=np.uint8)[:, :w]
