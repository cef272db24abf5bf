"""A numpy restatement of the photometric-residual rules P1 to P6 (include/ffl.h): float32
arrays, element-wise operations in exactly the written order, np.floor; the integer steps in int32.  Every numpy float32
operation rounds once and numpy never contracts, which is the arithmetic the rules ask of the kernel."""
import functools

import numpy as np

F32 = np.float32
ALPHA, BETA, SOFT = F32(0.5), F32(4.0), 1   # the library's defaults (the project's own choice, not tuned on footage)


def threshold(I0, alpha=ALPHA, beta=BETA):
    """thr of rule P3, (h, w) float32: alpha * (|gx| + |gy|) + beta with clamped central differences of I0"""
    I = np.asarray(I0).astype(np.int32)
    h, w = I.shape
    xs, ys = np.arange(w), np.arange(h)
    gx = I[:, np.minimum(xs + 1, w - 1)] - I[:, np.maximum(xs - 1, 0)]
    gy = I[np.minimum(ys + 1, h - 1), :] - I[np.maximum(ys - 1, 0), :]
    g = np.abs(gx.astype(F32)) + np.abs(gy.astype(F32))
    thr = F32(alpha) * g + F32(beta)
    assert thr.dtype == F32
    return thr


def residual(I0, I1, F, alpha=ALPHA, beta=BETA, soft=SOFT, gate=None, with_outside=False):
    """the (h, w) uint8 map of gray frames I0, I1 ((h, w) uint8) under the forward field F ((h, w, 2) float32); gate: (h, w)
    uint8 or None.  with_outside: also the (h, w) bool array of pixels that land outside (rule P1)."""
    I0, I1, F = np.asarray(I0), np.asarray(I1), np.asarray(F, F32)
    assert I0.dtype == np.uint8 and I1.dtype == np.uint8
    h, w = F.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    u, v = F[..., 0], F[..., 1]
    with np.errstate(all="ignore"):
        px, py = x.astype(F32) + u, y.astype(F32) + v                                           # P1
        inside = (px >= F32(0)) & (px <= F32(w - 1)) & (py >= F32(0)) & (py <= F32(h - 1))
        pxs, pys = np.where(inside, px, F32(0)), np.where(inside, py, F32(0))   # nothing of I1 is read for the others
        fx, fy = np.floor(pxs), np.floor(pys)                                                   # P2
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        ax, ay = pxs - fx, pys - fy
        P = I1.astype(F32)
        i00, i01, i10, i11 = P[y0, x0], P[y0, x1], P[y1, x0], P[y1, x1]
        t = i00 + ax * (i01 - i00)
        s = i10 + ax * (i11 - i10)
        ic = t + ay * (s - t)
        a = np.abs(ic - I0.astype(F32))                                                         # P3
        thr = threshold(I0, alpha, beta)
        assert a.dtype == F32
        if soft:                                                                                # P4
            q = F32(1) - a / thr
            q = np.where(q > F32(0), q, F32(0))
            W = (q * F32(255) + F32(0.5)).astype(np.int32)
        else:                                                                                   # P5
            W = np.where(a < thr, 255, 0).astype(np.int32)
    W = np.where(inside, W, 0)
    if gate is not None:                                                                        # P6
        W = np.minimum(W, np.asarray(gate).astype(np.int32))
    assert W.min() >= 0 and W.max() <= 255
    W = W.astype(np.uint8)
    return (W, ~inside) if with_outside else W


# ---- the synthetic inputs of the GPU tests (their conditions are asserted in test_residual_ref_host.py) ----------------------
SIZES = [(16, 16), (130, 17), (257, 40)]   # widths = 0, 2, 1 mod 4; 16x16 is the smallest size the contexts of the tests accept
SEEDS = (1, 2, 3, 4, 5)                    # the seeds in use: each meets test_residual_ref_host.py's conditions at every size
SHIFT = (2.5, -1.25)                       # the displacement of synthetic()'s texture, (dx, dy)


def texture(w, h, seed, dx=0.0, dy=0.0):
    """(h, w) float64: six sinusoids about 128 (amplitude 18 each, wavelengths of 7 to 40 px), sampled at (x - dx, y - dy) --
    the texture displaced by (dx, dy)"""
    rng = np.random.default_rng(9000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - dx, y - dy
    out = np.full((h, w), 128.0)
    for _ in range(6):
        lam, th, ph = rng.uniform(7, 40), rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
        k = 2 * np.pi / lam
        out += 18.0 * np.sin(k * (np.cos(th) * x + np.sin(th) * y) + ph)
    return out


def to_u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def synthetic(w, h, seed):
    """(I0, I1, F): I0 a texture of six sinusoids; I1 the same texture displaced by SHIFT plus rounded Gaussian noise of sigma
    3; F that displacement plus a smooth perturbation of amplitude 1.5 px plus noise of sigma 0.3; and one central block of
    about 2/5 x 2/5 of the frame where F = 0 and I1 = I0 (it supplies the 255s)"""
    rng = np.random.default_rng(9500 + seed)
    I0 = to_u8(texture(w, h, seed))
    I1 = to_u8(texture(w, h, seed, *SHIFT) + np.rint(rng.standard_normal((h, w)) * 3.0))
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    ph = rng.uniform(0, 6.28, 4).astype(F32)
    F = (rng.standard_normal((h, w, 2)) * 0.3).astype(F32)
    F[..., 0] += F32(SHIFT[0]) + F32(1.5) * np.sin(x * F32(0.045) + ph[0]) * np.cos(y * F32(0.06) + ph[1])
    F[..., 1] += F32(SHIFT[1]) + F32(1.5) * np.cos(x * F32(0.05) + ph[2]) * np.sin(y * F32(0.07) + ph[3])
    bw, bh = max(4, (w * 2) // 5), max(4, (h * 2) // 5)
    bx, by = (w - bw) // 2, (h - bh) // 2
    F[by:by + bh, bx:bx + bw] = 0
    I1[by:by + bh, bx:bx + bw] = I0[by:by + bh, bx:bx + bw]
    for a in (I0, I1, F):
        a.setflags(write=False)
    return I0, I1, F


def displaced(I, dx, dy):
    """I displaced by the integers (dx, dy) with wrap-around: out[(y + dy) % h][(x + dx) % w] = I[y][x]"""
    return np.roll(I, (dy, dx), axis=(0, 1))


# Hostile content placed into a synthetic triple: non-finite, enormous and denormal flow values in either component, landings
# exactly on the last column and row and on column 0, fractional landings in the last column and row, and grey values 0 and
# 255 at sampled corners and at the clamped gradient neighbours of all four edges.
DENORMAL = 1e-40


def hostile(w, h, seed):
    I0, I1, F = (a.copy() for a in synthetic(w, h, seed))
    cx, cy = w // 2, h // 2   # inside the zero block: these pixels land on themselves
    F[1, 1] = (np.nan, 0)
    F[1, 2] = (0, np.nan)
    F[2, 1] = (np.inf, 0)
    F[2, 2] = (0, -np.inf)
    F[2, 3] = (-np.inf, 0)
    F[2, 4] = (0, np.inf)
    F[3, 1] = (1e30, 0)
    F[3, 2] = (-1e30, 1e30)
    F[3, 3] = (0, -1e30)
    F[cy - 2, cx - 1] = (DENORMAL, -DENORMAL)   # absorbed by the coordinate: lands on itself
    F[cy, 0] = (DENORMAL, 0)                    # px = a denormal: x0 = 0 and ax = that denormal
    F[h - 1, w - 1] = (0, 0)                    # px = w - 1, py = h - 1 exactly: x1 = x0, y1 = y0
    F[h - 3, w - 2] = (1, 2)                    # the same landing from another pixel
    F[5, w - 1] = (0, 0.5)                      # the last column, a fractional row: x1 = x0
    F[6, w - 2] = (0.75, -0.25)                 # between the last two columns
    F[h - 1, 5] = (0.5, 0)                      # the last row, a fractional column: y1 = y0
    F[h - 2, 6] = (-0.25, 0.75)                 # between the last two rows
    F[h - 1, 0] = (0, 0)
    F[0, w - 1] = (0, 0)
    F[0, 0] = (0, 0)
    # 0 and 255 at the corners those landings sample ...
    I1[h - 1, w - 1], I1[h - 1, w - 2], I1[h - 2, w - 1], I1[h - 2, w - 2] = 255, 0, 0, 255
    I1[5, w - 1], I1[6, w - 1], I1[6, w - 2], I1[5, w - 2] = 0, 255, 0, 255
    I1[h - 1, 5], I1[h - 1, 6], I1[h - 2, 5], I1[h - 2, 6] = 255, 0, 0, 255
    I1[cy, 0], I1[cy, 1], I1[cy + 1, 0] = 255, 0, 0
    I1[0, 0], I1[0, w - 1], I1[h - 1, 0] = 0, 255, 0
    # ... and at the pixels and clamped gradient neighbours of the four edges and corners
    I0[cy, 0], I0[cy, 1] = 0, 255
    I0[cy + 1, w - 1], I0[cy + 1, w - 2] = 255, 0
    I0[0, cx], I0[1, cx] = 255, 0
    I0[h - 1, cx], I0[h - 2, cx] = 0, 255
    I0[0, 0], I0[0, 1], I0[1, 0] = 255, 0, 0
    I0[h - 1, w - 1], I0[h - 1, w - 2], I0[h - 2, w - 1] = 0, 255, 255
    I0[0, w - 1], I0[h - 1, 0] = 0, 255
    return I0, I1, F
