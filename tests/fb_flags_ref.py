"""ctypes loader of the restatement of general Farneback's two modes (tests/fb_flags_ref/fb_flags_ref.c, DESIGN.md
appendix F.7 and F.8) and the level driver that composes them with the stages of tests/fb_general_ref.

Test-only: the product and bench.py never import it.  The shared object is built on first use next to its source, written
under a temporary name and moved into place with os.replace, as fb_general_ref.py builds its own."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import fb_general_ref as fbr

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fb_flags_ref")
_SRC = os.path.join(_DIR, "fb_flags_ref.c")
_LIB = os.path.join(_DIR, "libfb_flags_ref.so")
_lib = None

AREA_PATHS = {0: "a", 1: "b", 2: "c"}


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB) or os.path.getmtime(_LIB) < os.path.getmtime(_SRC):
        fd, tmp = tempfile.mkstemp(suffix=".so", dir=_DIR)
        os.close(fd)
        try:
            subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", tmp,
                                   _SRC, "-lm"])
            os.replace(tmp, _LIB)
        finally:
            if os.path.exists(tmp):
                os.unlink(tmp)
    L = C.CDLL(_LIB)
    vp = C.c_void_p
    L.ffr_taps.argtypes = [C.c_int, vp]
    L.ffr_taps.restype = None
    L.ffr_gauss_solve.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.ffr_area_table.argtypes = [C.c_int, C.c_int, vp, vp, vp]
    L.ffr_area_init.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp]
    _lib = L
    return L


def taps(winsize):
    """F.7: the winsize // 2 + 1 float32 taps k[0..m]"""
    k = np.empty(winsize // 2 + 1, np.float32)
    lib().ffr_taps(int(winsize), k.ctypes.data)
    return k


def gauss_solve(M, winsize):
    """F.7: (5, h, w) -> (h, w, 2)"""
    M = np.ascontiguousarray(M, np.float32)
    _, h, w = M.shape
    out = np.empty((h, w, 2), np.float32)
    assert lib().ffr_gauss_solve(M.ctypes.data, w, h, int(winsize), out.ctypes.data) == 0
    return out


def area_table(S, D):
    """F.8 (c): (dst, src, alpha) arrays of one axis"""
    n = S + 2 * D
    di, si, al = np.empty(n, np.intc), np.empty(n, np.intc), np.empty(n, np.float32)
    k = lib().ffr_area_table(int(S), int(D), di.ctypes.data, si.ctypes.data, al.ctypes.data)
    return di[:k].copy(), si[:k].copy(), al[:k].copy()


def area_init(seed, lw, lh, scale):
    """F.8: ((lh, lw, 2) float32, path) with path "a", "b" or "c\""""
    seed = np.ascontiguousarray(seed, np.float32)
    H, W = seed.shape[:2]
    out = np.empty((lh, lw, 2), np.float32)
    path = lib().ffr_area_init(seed.ctypes.data, W, H, int(lw), int(lh), float(scale), out.ctypes.data)
    assert path >= 0
    return out, AREA_PATHS[path]


def level_scale(p, k):
    """F.1's double: pyr_scale^k by repeated multiplication"""
    ps, sc = fbr.widen(fbr._p(p).pyr_scale), 1.0
    for _ in range(k):
        sc *= ps
    return sc


TEXTURE_FLOW = (2.0, 1.0)


def textured_frames(w, h, n=3):
    """n frames of one broadband texture (uniform noise under a 3 x 3 box), each the one before moved by TEXTURE_FLOW
    pixels.  Unlike a smooth pattern, which is locally the exact quadratic whose Farneback update does not depend on the
    starting flow (tests/test_oracle_farneback.py), its estimate keeps a trace of where the iteration started."""
    rng = np.random.default_rng(w * 31 + h)
    dx, dy = int(TEXTURE_FLOW[0]), int(TEXTURE_FLOW[1])
    big = rng.integers(0, 256, (h + dy * n + 2, w + dx * n + 2)).astype(np.float64)
    sm = sum(big[j:j + h + dy * n, i:i + w + dx * n] for j in range(3) for i in range(3)) / 9
    return [np.ascontiguousarray(np.rint(sm[dy * (n - k):dy * (n - k) + h, dx * (n - k):dx * (n - k) + w]).astype(np.uint8))
            for k in range(n)]


def _expansion(f, p, k, sig, rcache):
    if rcache is None:
        return fbr.polyexp(fbr.pyr_level(f, p, k), p.poly_n, sig)
    key = (f.shape, f.tobytes(), bytes(p), k)
    if key not in rcache:
        rcache[key] = fbr.polyexp(fbr.pyr_level(f, p, k), p.poly_n, sig)
    return rcache[key]


def flow(f0, f1, p=None, window="box", seed=None, info=None, rcache=None):
    """The (h, w, 2) float32 flow of the pair under p (a Params or a dict of overrides), the level chain of fbr.flow composed
    in Python: window "box" (F.5) or "gaussian" (F.7); seed: None (zero start) or the (h, w, 2) initial flow (F.8).  info, a
    dict, receives the F.8 path taken; rcache, a dict, keeps the frames' expansions for later calls (they depend on neither
    mode)."""
    assert window in ("box", "gaussian")
    p = fbr._p(p)
    f0, f1 = np.ascontiguousarray(f0, np.uint8), np.ascontiguousarray(f1, np.uint8)
    h, w = f0.shape
    ns = fbr.geometry(w, h, p)
    if ns is None:
        raise ValueError(f"restatement refused {w}x{h} with {p.as_dict()}")
    sig, mul = fbr.widen(p.poly_sigma), np.float32(1.0 / fbr.widen(p.pyr_scale))
    solve = fbr.blur_solve if window == "box" else gauss_solve
    prev = None
    for k in range(ns - 1, -1, -1):
        lw, lh, _, _ = fbr.level_params(w, h, p, k)
        if prev is not None:
            cur = np.empty((lh, lw, 2), np.float32)
            ph, pw = prev.shape[:2]
            assert fbr.lib().fbr_flow_upsample(prev.ctypes.data, pw, ph, cur.ctypes.data, lw, lh, C.c_float(mul)) == 0
        elif seed is not None:
            cur, path = area_init(seed, lw, lh, level_scale(p, k))
            if info is not None:
                info["path"] = path
        else:
            cur = np.zeros((lh, lw, 2), np.float32)
        R0, R1 = _expansion(f0, p, k, sig, rcache), _expansion(f1, p, k, sig, rcache)
        M = fbr.update_matrices(R0, R1, cur)
        for it in range(p.iterations):
            cur = solve(M, p.winsize)
            if it < p.iterations - 1:
                M = fbr.update_matrices(R0, R1, cur)
        prev = cur
    return prev
