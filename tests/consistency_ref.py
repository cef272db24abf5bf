"""A numpy restatement of the forward-backward consistency rules K1 to K6 (include/ffl.h):
float32 arrays, element-wise operations in exactly the written order, np.floor.  Every numpy float32 operation rounds once
and numpy never contracts, which is the arithmetic the rules ask of the kernel."""
import functools

import numpy as np

F32 = np.float32
ALPHA, BETA, SOFT = F32(0.01), F32(0.5), 1   # the library's defaults


def consistency(F, B, alpha=ALPHA, beta=BETA, soft=SOFT, gate=None, with_outside=False):
    """the (h, w) uint8 map of forward field F and backward field B, both (h, w, 2) float32; gate: (h, w) uint8 or None.
    with_outside: also the (h, w) bool array of pixels that land outside (rule K1)."""
    F, B = np.asarray(F, F32), np.asarray(B, F32)
    h, w = F.shape[:2]
    alpha, beta = F32(alpha), F32(beta)
    y, x = np.mgrid[0:h, 0:w]
    u, v = F[..., 0], F[..., 1]
    with np.errstate(all="ignore"):
        px, py = x.astype(F32) + u, y.astype(F32) + v                                           # K1
        inside = (px >= F32(0)) & (px <= F32(w - 1)) & (py >= F32(0)) & (py <= F32(h - 1))
        pxs, pys = np.where(inside, px, F32(0)), np.where(inside, py, F32(0))   # nothing of B is read for the others
        fx, fy = np.floor(pxs), np.floor(pys)                                                   # K2
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        ax, ay = pxs - fx, pys - fy
        b = []
        for c in range(2):
            P = B[..., c]
            b00, b01, b10, b11 = P[y0, x0], P[y0, x1], P[y1, x0], P[y1, x1]
            t = b00 + ax * (b01 - b00)
            s = b10 + ax * (b11 - b10)
            b.append(t + ay * (s - t))
        bu, bv = b
        ex, ey = u + bu, v + bv                                                                 # K3
        e2 = ex * ex + ey * ey
        thr = alpha * ((u * u + v * v) + (bu * bu + bv * bv)) + beta
        assert e2.dtype == F32 and thr.dtype == F32
        if soft:                                                                                # K4
            q = F32(1) - e2 / thr
            q = np.where(q > F32(0), q, F32(0))
            W = (q * F32(255) + F32(0.5)).astype(np.int32)
        else:                                                                                   # K5
            W = np.where(e2 < thr, 255, 0).astype(np.int32)
    W = np.where(inside, W, 0)
    if gate is not None:                                                                        # K6
        W = np.minimum(W, np.asarray(gate).astype(np.int32))
    assert W.min() >= 0 and W.max() <= 255
    W = W.astype(np.uint8)
    return (W, ~inside) if with_outside else W


# ---- the synthetic inputs of the GPU tests (their conditions are asserted in test_consistency_ref_host.py) -------------------
SIZES = [(16, 16), (130, 17), (257, 40)]


@functools.lru_cache(maxsize=None)
def synthetic_pair(w, h, seed):
    """(F, B): a smooth field of amplitude about 4 px plus noise, B = -F plus noise of sigma 0.45, and one block of about a
    sixth of the frame where F = B = 0 (it supplies the 255s)"""
    rng = np.random.default_rng(7000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    ph = rng.uniform(0, 6.28, 4).astype(F32)
    F = (rng.standard_normal((h, w, 2)) * 0.3).astype(F32)
    F[..., 0] += F32(4.0) * np.sin(x * F32(0.045) + ph[0]) * np.cos(y * F32(0.06) + ph[1])
    F[..., 1] += F32(4.0) * np.cos(x * F32(0.05) + ph[2]) * np.sin(y * F32(0.07) + ph[3])
    B = (-F + (rng.standard_normal((h, w, 2)) * 0.45).astype(F32)).astype(F32)
    bw, bh = max(4, (w * 2) // 5), max(4, (h * 2) // 5)
    bx, by = (w - bw) // 2, (h - bh) // 2
    F[by:by + bh, bx:bx + bw] = 0
    B[by:by + bh, bx:bx + bw] = 0
    F.setflags(write=False)
    B.setflags(write=False)
    return F, B


# Hostile content: (pixel (x, y), forward value (u, v)) and (pixel, backward value) placed into a synthetic pair.  Denormal
# 1e-40, 1e30 (its square overflows float32), inf of either sign, NaN; the backward ones sit at corners that zero-flow and
# small-flow neighbours sample.
DENORMAL = 1e-40


def hostile_pair(w, h, seed):
    F, B = (a.copy() for a in synthetic_pair(w, h, seed))
    cx, cy = w // 2, h // 2   # inside the zero block: these pixels and their neighbours land on themselves
    F[1, 1] = (np.nan, 0)
    F[1, 2] = (0, np.nan)
    F[2, 1] = (np.inf, 0)
    F[2, 2] = (0, -np.inf)
    F[3, 1] = (1e30, 0)
    F[3, 2] = (-1e30, 1e30)
    F[cy - 3, cx - 1] = (DENORMAL, -DENORMAL)       # absorbed by the coordinate: lands on itself; u * u underflows to 0
    F[cy, 0] = (DENORMAL, 0)                    # px = a denormal: x0 = 0 and ax = that denormal
    F[cy + 1, cx - 1] = (0.5, 0.5)              # samples the four corners below
    B[cy + 1, cx - 1] = (1e30, 0)
    B[cy + 1, cx] = (np.nan, 1)
    B[cy + 2, cx - 1] = (0, np.inf)
    B[cy + 2, cx] = (DENORMAL, DENORMAL)
    F[cy - 1, cx + 1] = (0, 0)
    B[cy - 1, cx + 1] = (1e30, -1e30)           # a zero forward flow reads an enormous backward one: e2 = inf
    F[cy - 1, cx] = (0, 0)
    B[cy - 1, cx] = (np.inf, 0)                 # ax = 0 times (b01 - inf): a NaN through the interpolation
    F[cy - 2, cx] = (0, 0)
    B[cy - 2, cx] = (DENORMAL, 0)
    F[h - 1, w - 1] = (0, 0)                    # px = w - 1, py = h - 1 exactly: x1 = x0, y1 = y0
    B[h - 1, w - 1] = (0.25, -0.25)
    return F, B
