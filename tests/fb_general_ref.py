"""ctypes loader of the general-parameter Farneback restatement (tests/fb_general_ref/fb_general_ref.c, DESIGN.md
appendix F).

Test-only: the product and bench.py never import it.  The shared object is built on first use next to its source, written
under a temporary name and moved into place with os.replace, so two processes that build at once never load a
half-written file."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fb_general_ref")
_SRC = os.path.join(_DIR, "fb_general_ref.c")
_LIB = os.path.join(_DIR, "libfb_general_ref.so")
_lib = None

FIELDS = ["pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags"]
DEFAULTS = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0)


class Params(C.Structure):
    _fields_ = [("pyr_scale", C.c_float), ("levels", C.c_int), ("winsize", C.c_int), ("iterations", C.c_int),
                ("poly_n", C.c_int), ("poly_sigma", C.c_float), ("flags", C.c_int)]

    def as_dict(self):
        return {n: getattr(self, n) for n in FIELDS}


def params(**over):
    """cv2's defaults of the reference's call with single fields overridden (cv2 keyword names)."""
    d = dict(DEFAULTS)
    for k, v in over.items():
        if k not in d:
            raise ValueError(f"unknown Farneback parameter {k!r}")
        d[k] = v
    return Params(**d)


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
    vp, ip, P = C.c_void_p, C.POINTER(C.c_int), C.POINTER(Params)
    L.fbr_widen.argtypes = [C.c_float]
    L.fbr_widen.restype = C.c_double
    L.fbr_check.argtypes = [P]
    L.fbr_check.restype = C.c_char_p
    L.fbr_geometry.argtypes = [C.c_int, C.c_int, P, ip]
    L.fbr_level_params.argtypes = [C.c_int, C.c_int, P, C.c_int, ip, ip, C.POINTER(C.c_double), ip]
    L.fbr_level_params.restype = None
    L.fbr_pyr_level.argtypes = [vp, C.c_int, C.c_int, P, C.c_int, vp]
    L.fbr_polyexp.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, vp]
    L.fbr_flow_upsample.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_float]
    L.fbr_update_matrices.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
    L.fbr_update_matrices.restype = None
    L.fbr_blur_solve.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.fbr_flow.argtypes = [vp, vp, C.c_int, C.c_int, P, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    _lib = L
    return L


def _p(p):
    return p if isinstance(p, Params) else params(**(p or {}))


def widen(x):
    """F.0: the double the restatement computes with for a float parameter"""
    return lib().fbr_widen(float(x))


def check(p):
    """None when the parameters are valid, else the refusal message"""
    m = lib().fbr_check(C.byref(_p(p)))
    return None if m is None else m.decode()


def geometry(w, h, p=None):
    """number of scales, or None when the size / parameters are refused"""
    n = C.c_int()
    if lib().fbr_geometry(int(w), int(h), C.byref(_p(p)), C.byref(n)):
        return None
    return n.value


def level_params(w, h, p, k):
    lw, lh, ks, s = C.c_int(), C.c_int(), C.c_int(), C.c_double()
    lib().fbr_level_params(int(w), int(h), C.byref(_p(p)), int(k), C.byref(lw), C.byref(lh), C.byref(s), C.byref(ks))
    return lw.value, lh.value, s.value, ks.value


def pyr_level(img, p, k):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    lw, lh, _, _ = level_params(w, h, p, k)
    out = np.empty((lh, lw), np.float32)
    assert lib().fbr_pyr_level(img.ctypes.data, w, h, C.byref(_p(p)), int(k), out.ctypes.data) == 0
    return out


def polyexp(I, n=5, sigma=1.2):
    """(5, h, w) planes; sigma is used as given (a double)"""
    I = np.ascontiguousarray(I, np.float32)
    h, w = I.shape
    out = np.empty((5, h, w), np.float32)
    assert lib().fbr_polyexp(I.ctypes.data, w, h, int(n), float(sigma), out.ctypes.data) == 0
    return out


def update_matrices(R0, R1, flow):
    R0, R1 = np.ascontiguousarray(R0, np.float32), np.ascontiguousarray(R1, np.float32)
    flow = np.ascontiguousarray(flow, np.float32)
    h, w = flow.shape[:2]
    out = np.empty((5, h, w), np.float32)
    lib().fbr_update_matrices(R0.ctypes.data, R1.ctypes.data, flow.ctypes.data, w, h, out.ctypes.data)
    return out


def blur_solve(M, winsize):
    M = np.ascontiguousarray(M, np.float32)
    _, h, w = M.shape
    out = np.empty((h, w, 2), np.float32)
    assert lib().fbr_blur_solve(M.ctypes.data, w, h, int(winsize), out.ctypes.data) == 0
    return out


def flow(f0, f1, p=None, dump=None):
    """The (h, w, 2) float32 flow of the pair under p (a Params or a dict of overrides).  dump = (level, iter) also returns
    that level's dict of I0, I1, R0, R1 (5 planes), M (5 planes) and the flow as they stand before blur iteration iter."""
    p = _p(p)
    f0, f1 = np.ascontiguousarray(f0, np.uint8), np.ascontiguousarray(f1, np.uint8)
    h, w = f0.shape
    out = np.empty((h, w, 2), np.float32)
    if dump is None:
        rc = lib().fbr_flow(f0.ctypes.data, f1.ctypes.data, w, h, C.byref(p), out.ctypes.data, -1, 0, *([None] * 6))
        if rc:
            raise ValueError(f"restatement refused {w}x{h} with {p.as_dict()} ({rc})")
        return out
    k, it = dump
    lw, lh, _, _ = level_params(w, h, p, k)
    d = dict(I0=np.empty((lh, lw), np.float32), I1=np.empty((lh, lw), np.float32), R0=np.empty((5, lh, lw), np.float32),
             R1=np.empty((5, lh, lw), np.float32), M=np.empty((5, lh, lw), np.float32), flow=np.empty((lh, lw, 2), np.float32))
    rc = lib().fbr_flow(f0.ctypes.data, f1.ctypes.data, w, h, C.byref(p), out.ctypes.data, int(k), int(it),
                        *[d[n].ctypes.data for n in ("I0", "I1", "R0", "R1", "M", "flow")])
    if rc:
        raise ValueError(f"restatement refused {w}x{h} with {p.as_dict()} ({rc})")
    return out, d
