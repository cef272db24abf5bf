"""ctypes loader of the DIS restatement (tests/dis_ref/dis_ref.c).

Test-only: the product never imports it.  The shared object is built on first use next to its source, written under a
temporary name and moved into place with os.replace, so two processes that build at once never load a half-written
file."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dis_ref")
_SRC = os.path.join(_DIR, "dis_ref.c")
_LIB = os.path.join(_DIR, "libdis_ref.so")
_lib = None

FIELDS = ["finest_scale", "patch_size", "patch_stride", "grad_descent_iters", "var_refine_iters", "vr_alpha",
          "vr_gamma", "vr_delta", "use_mean_norm", "use_spatial_prop", "stripes"]
STAGE_PASS1, STAGE_PASS2, STAGE_DENSE, STAGE_VR, STAGE_IMAGES = 0, 1, 2, 3, 4


class Params(C.Structure):
    _fields_ = [(n, C.c_int) for n in FIELDS[:5]] + [(n, C.c_float) for n in FIELDS[5:8]] + \
               [(n, C.c_int) for n in FIELDS[8:]]


def fast_params(**over):
    """PRESET_FAST (DESIGN appendix D1) with single fields overridden."""
    d = dict(finest_scale=2, patch_size=8, patch_stride=4, grad_descent_iters=16, var_refine_iters=5, vr_alpha=20.0,
             vr_gamma=10.0, vr_delta=5.0, use_mean_norm=1, use_spatial_prop=1, stripes=0)
    for k, v in over.items():
        if k not in d:
            raise ValueError(f"unknown DIS parameter {k!r}")
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
    L.dis_geometry.argtypes = [C.c_int, C.c_int, P, ip, ip]
    L.dis_flow.argtypes = [vp, vp, C.c_int, C.c_int, P, vp, C.c_int, C.c_int, vp]
    L.dis_area_down.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.dis_area_down.restype = None
    L.dis_densify.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]
    L.dis_densify.restype = None
    L.dis_upsample.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_float, vp]
    L.dis_upsample.restype = None
    _lib = L
    return L


def geometry(w, h, p=None):
    """(coarsest, finest) scale, or None when the size / parameters are refused."""
    p = p or fast_params()
    c, f = C.c_int(), C.c_int()
    if lib().dis_geometry(int(w), int(h), C.byref(p), C.byref(c), C.byref(f)):
        return None
    return c.value, f.value


def flow(f0, f1, p=None, dbg=None):
    """The (h, w, 2) float32 DIS flow of the pair; dbg = (scale, stage) also returns that stage's field."""
    p = p or fast_params()
    f0, f1 = np.ascontiguousarray(f0, np.uint8), np.ascontiguousarray(f1, np.uint8)
    h, w = f0.shape
    out = np.empty((h, w, 2), np.float32)
    g = geometry(w, h, p)
    if g is None:
        raise ValueError(f"DIS: {w}x{h} is not a supported size for these parameters")
    buf, sc, st = None, -1, -1
    if dbg is not None:
        sc, st = dbg
        buf = np.zeros(2 * (h >> sc) * (w >> sc) + 16, np.float32)
    rc = lib().dis_flow(f0.ctypes.data, f1.ctypes.data, w, h, C.byref(p), out.ctypes.data, sc, st,
                        None if buf is None else buf.ctypes.data)
    assert rc == 0
    if dbg is None:
        return out
    return out, stage_view(buf, w, h, p, sc, st)


def stage_view(buf, w, h, p, scale, stage):
    lw, lh = w >> scale, h >> scale
    if stage in (STAGE_PASS1, STAGE_PASS2):
        ws, hs = 1 + (lw - p.patch_size) // p.patch_stride, 1 + (lh - p.patch_size) // p.patch_stride
        return buf[:2 * ws * hs].reshape(hs, ws, 2).copy()
    if stage == STAGE_IMAGES:
        return buf[:2 * lw * lh].reshape(2, lh, lw).copy()
    return buf[:2 * lw * lh].reshape(lh, lw, 2).copy()


def area_down(img, f):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.empty((h // f, w // f), np.uint8)
    lib().dis_area_down(img.ctypes.data, w, h, f, out.ctypes.data)
    return out


def densify(I0, I1, S, stride=4):
    I0, I1 = np.ascontiguousarray(I0, np.float32), np.ascontiguousarray(I1, np.float32)
    S = np.ascontiguousarray(S, np.float32)
    h, w = I0.shape
    out = np.empty((h, w, 2), np.float32)
    lib().dis_densify(I0.ctypes.data, I1.ctypes.data, w, h, S.ctypes.data, stride, out.ctypes.data)
    return out
