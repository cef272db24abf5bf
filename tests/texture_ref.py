"""A numpy restatement of the texture (structure-tensor) rules T1 to T6 (include/ffl.h): int64
arrays for the integer steps, float64 arrays for the rest, element-wise operations in exactly the written order.  Every numpy
float64 operation rounds once and numpy never contracts, which is the arithmetic the rules ask of the kernel.  The window sums
are formed the slow, literal way -- one shifted gather of the gradient AT THE CLAMPED POSITION per window offset -- and not
separably, so that they share nothing with the kernel but the rule."""
import functools

import numpy as np

import residual_ref

RADIUS, TAU, SOFT = 7, np.float32(16.0), 1   # the library's defaults (the project's own choice, not tuned on footage)
RADII = (1, 3, 7, 8)


def gradients(I):
    """rule T1: (gx, gy) int64 (h, w), clamped central differences"""
    I = np.asarray(I)
    assert I.dtype == np.uint8
    I = I.astype(np.int64)
    h, w = I.shape
    xs, ys = np.arange(w), np.arange(h)
    gx = I[:, np.minimum(xs + 1, w - 1)] - I[:, np.maximum(xs - 1, 0)]
    gy = I[np.minimum(ys + 1, h - 1), :] - I[np.maximum(ys - 1, 0), :]
    return gx, gy


def window_sums(I, radius):
    """rule T2: (Sxx, Sxy, Syy) int64 (h, w) over the (2r+1)^2 offsets, the gradient taken at the clamped position"""
    gx, gy = gradients(I)
    h, w = gx.shape
    xs, ys = np.arange(w), np.arange(h)
    Sxx, Sxy, Syy = (np.zeros((h, w), np.int64) for _ in range(3))
    for j in range(-radius, radius + 1):
        yy = np.clip(ys + j, 0, h - 1)[:, None]
        for i in range(-radius, radius + 1):
            xx = np.clip(xs + i, 0, w - 1)[None, :]
            a, b = gx[yy, xx], gy[yy, xx]
            Sxx += a * a
            Sxy += a * b
            Syy += b * b
    assert Sxx.max() < 2 ** 31 and Syy.max() < 2 ** 31 and np.abs(Sxy).max() < 2 ** 31   # they fit int32
    return Sxx, Sxy, Syy


def cornerness(I, radius):
    """rule T3: (c float64, det int64, tr int64), each (h, w)"""
    Sxx, Sxy, Syy = window_sums(I, radius)
    tr = Sxx + Syy
    det = Sxx * Syy - Sxy * Sxy            # int64: exact
    assert det.min() >= 0 and det.max() < 2 ** 53
    c = np.zeros(tr.shape, np.float64)
    nz = tr != 0
    c[nz] = det[nz].astype(np.float64) / tr[nz].astype(np.float64)   # one IEEE division; none where tr == 0
    return c, det, tr


def texture_map(I, radius=RADIUS, tau=TAU, soft=SOFT, gate=None):
    """the (h, w) uint8 map of the gray frame I ((h, w) uint8); gate: (h, w) uint8 or None"""
    c, det, tr = cornerness(I, radius)
    tn = np.float64(np.float32(tau)) * np.float64((2 * radius + 1) ** 2)                          # T4
    if soft:
        q = c / tn
        q = np.where(q < 1.0, q, 1.0)
        W = (q * 255.0 + 0.5).astype(np.int64)
    else:                                                                                        # T5: no division
        W = np.where((tr != 0) & (det.astype(np.float64) >= tn * tr.astype(np.float64)), 255, 0).astype(np.int64)
    if gate is not None:                                                                         # T6
        W = np.minimum(W, np.asarray(gate).astype(np.int64))
    assert W.min() >= 0 and W.max() <= 255
    return W.astype(np.uint8)


# ---- the synthetic inputs of the GPU tests (their conditions are asserted in test_texture_ref_host.py) -----------------------
# widths = 0, 2, 1, 0 mod 4; 16x16 is smaller than k_texture's 64 x 16 tile; 130, 257 and 96 straddle tile seams in x, heights
# 17, 40 and 70 in y, and 40 = 2 * 16 + 8 and 70 = 4 * 16 + 6 have at least two whole tile rows and a ragged last one
SIZES = [(16, 16), (130, 17), (257, 40), (96, 70)]
SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def thirds(w, h, seed):
    """(h, w) uint8 of three vertical bands: the left third 128 plus Gaussian noise of sigma 1 (a flat wall), the middle third
    horizontal stripes 128 + 40 sin(2 pi y / 9) (the aperture problem), the right third residual_ref.texture"""
    rng = np.random.default_rng(12000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b = w // 3, (2 * w) // 3
    out = residual_ref.texture(w, h, seed)
    out[:, :a] = 128.0 + rng.standard_normal((h, a))
    out[:, a:b] = 128.0 + 40.0 * np.sin(2 * np.pi * y[:, a:b] / 9.0)
    out = residual_ref.to_u8(out)
    out.setflags(write=False)
    return out


def checkerboard(w, h):
    """2 x 2 blocks of 0 and 255: |gx| = |gy| = 255 at every interior pixel, so Sxx = Syy = N * 65025 in the interior and at
    radius 8 Sxx * Syy = 3.5e14 -- the trap for a 32-bit product"""
    y, x = np.mgrid[0:h, 0:w]
    return ((((x // 2) + (y // 2)) & 1) * 255).astype(np.uint8)


def constant(w, h, v=77):
    return np.full((h, w), v, np.uint8)


def single_pixel(w, h):
    out = np.zeros((h, w), np.uint8)
    out[h // 2, w // 2] = 255
    return out


def edge_steps(w, h):
    """0 / 255 steps on all four edges and corners: the clamped gradient neighbours of every border"""
    out = np.full((h, w), 128, np.uint8)
    out[0, :], out[1, :] = 255, 0
    out[h - 1, :], out[h - 2, :] = 0, 255
    out[:, 0], out[:, 1] = 0, 255
    out[:, w - 1], out[:, w - 2] = 255, 0
    out[0, 0], out[0, w - 1], out[h - 1, 0], out[h - 1, w - 1] = 255, 0, 255, 0
    out[1, 1], out[1, w - 2], out[h - 2, 1], out[h - 2, w - 2] = 0, 255, 0, 255
    return out


HOSTILE = {"checkerboard": checkerboard, "constant": constant, "single_pixel": single_pixel, "edge_steps": edge_steps}


# ---- the fit scene: a wall that reports zero flow next to texture that moves -------------------------------------------------
MOVE = (3.0, -2.0)


def wall_scene(w, h, seed):
    """(I, F): the left 3/5 of the frame a flat wall (128 plus noise of sigma 1) whose flow is zero, the rest
    residual_ref.texture moving by MOVE"""
    rng = np.random.default_rng(13000 + seed)
    a = (3 * w) // 5
    I = residual_ref.texture(w, h, seed)
    I[:, :a] = 128.0 + rng.standard_normal((h, a))
    F = np.zeros((h, w, 2), np.float32)
    F[:, a:] = MOVE
    return residual_ref.to_u8(I), F
