"""numpy restatement of DESIGN.md appendix Y, rules Y6 (display rotation and mirroring) and Y7 (full-range 4:2:0), for the
front-end's stream metadata (ffl_source_info):

    orient / inverse_orient            stored image <-> upright image, on (h, w[, 3]) arrays
    orient420 / inverse_orient420      the same on cv2's single (3h/2, w) 4:2:0 arrays of uint8 or uint16, plane by plane
    stored_xy                          rule Y6's table per pixel: where in the stored frame an upright pixel lies
    yuv_to_bgr_full(_pixels)           rule Y7
    stored_window                      the rectangle of the STORED frame ffl_upload_frames_yuv_src transfers

Index and integer work throughout: every comparison built on this module is bit for bit."""
import numpy as np

import front_sweep as fs
import yuv_ref

ORIENTATIONS = tuple((r, m) for r in (0, 90, 180, 270) for m in (False, True))
ORI_IDS = [f"r{r}{'m' if m else ''}" for r, m in ORIENTATIONS]
# rule Y7: round(c * 2^20) of the JFIF / BT.601 constants 1.772, 0.714136, 0.344136, 1.402
CB, CG_V, CG_U, CR = 1858077, 748826, 360853, 1470104


def orient(img, rotate, mirror):
    """stored -> upright: np.rot90(S, -rotate // 90), then a left-right flip if mirror"""
    u = np.rot90(img, -(rotate // 90))
    return u[:, ::-1] if mirror else u


def inverse_orient(img, rotate, mirror):
    """upright -> the stored frame that orient() turns back into it"""
    u = img[:, ::-1] if mirror else img
    return np.rot90(u, rotate // 90)


def pack420(Y, U, V, layout):
    """front_sweep.pack420 for any sample type"""
    h, w = Y.shape
    if layout == "nv12":
        uv = np.empty((h // 2, w), Y.dtype)
        uv[:, 0::2], uv[:, 1::2] = U, V
        return np.ascontiguousarray(np.concatenate([Y, uv]))
    return np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).astype(Y.dtype).reshape(h * 3 // 2, w)


def _each_plane(frame, layout, f):
    return pack420(*[np.ascontiguousarray(f(p)) for p in yuv_ref.planes(frame, layout)], layout)


def orient420(frame, layout, rotate, mirror):
    """orient() of a 4:2:0 frame: both sides are even, so a quarter turn or flip maps 2x2 blocks to 2x2 blocks and every
    plane turns by itself"""
    return _each_plane(frame, layout, lambda p: orient(p, rotate, mirror))


def inverse_orient420(frame, layout, rotate, mirror):
    return _each_plane(frame, layout, lambda p: inverse_orient(p, rotate, mirror))


def stored_xy(ux, uy, stored_size, rotate, mirror):
    """rule Y6's table: the stored (x, y) of upright pixel (ux, uy) of a stored_size = (sw, sh) frame"""
    sw, sh = stored_size
    uw = sh if rotate in (90, 270) else sw
    ux, uy = np.asarray(ux), np.asarray(uy)
    if mirror:
        ux = uw - 1 - ux
    return {0: (ux, uy), 90: (uy, sh - 1 - ux), 180: (sw - 1 - ux, sh - 1 - uy), 270: (sw - 1 - uy, ux)}[rotate]


def yuv_to_bgr_full_pixels(Y, U, V):
    """rule Y7 on integer arrays of equal shape -> (..., 3) uint8 BGR"""
    yh = (np.asarray(Y, np.int64) << 20) + (1 << 19)
    u, v = np.asarray(U, np.int64) - 128, np.asarray(V, np.int64) - 128
    b = (yh + CB * u) >> 20
    g = (yh - CG_V * v - CG_U * u) >> 20
    r = (yh + CR * v) >> 20
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def yuv_to_bgr_full(frame, layout):
    """a (3h/2, w) uint8 full-range 4:2:0 frame -> (h, w, 3) uint8 BGR, chroma nearest"""
    Y, U, V = yuv_ref.planes(frame, layout)
    up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1)   # noqa: E731
    return yuv_to_bgr_full_pixels(Y, up(U), up(V))


def full_operand(frame, layout, resize, crop, out):
    """the operand of a full-range frame: rule Y7, then the per-pixel restatement of resize, crop and luma"""
    return fs.direct_operand(yuv_to_bgr_full(frame, layout), resize, crop, out, False)


def upright_taps(d0, d1, s, r, generic):
    """yuv_ref.source_span, plus the zero-weight second tap the generic resize loads on an axis that happens not to scale
    (the resize mode is chosen by both axes together, source_span looks at one)"""
    t = yuv_ref.source_span(d0, d1, s, r)
    if generic and r == s:
        t = np.unique(np.concatenate([t, np.minimum(t + 1, s - 1)]))
    return t


def stored_window(stored_size, resize, crop, out, rotate, mirror):
    """((x, y, w, h) of the stored frame, mapped taps (xs, ys)): the upright tap set of each axis, widened by one pixel per
    side and clamped to the upright frame, its corners mapped through rule Y6, bounded, and rounded out on the STORED axes
    -- x to multiples of 16, y to even, clamped to the stored frame"""
    sw, sh = stored_size
    uw, uh = (sh, sw) if rotate in (90, 270) else (sw, sh)
    generic = fs.mode((uw, uh), resize) == "generic"
    tx = upright_taps(crop[0], crop[0] + out[0] - 1, uw, resize[0], generic)
    ty = upright_taps(crop[1], crop[1] + out[1] - 1, uh, resize[1], generic)
    ux = np.array([max(tx.min() - 1, 0), min(tx.max() + 1, uw - 1)])
    uy = np.array([max(ty.min() - 1, 0), min(ty.max() + 1, uh - 1)])
    px, py = stored_xy(ux, uy, stored_size, rotate, mirror)
    x0, y0 = px.min() // 16 * 16, py.min() // 2 * 2
    x1, y1 = min((px.max() + 16) // 16 * 16, sw), min((py.max() + 2) // 2 * 2, sh)
    gx, gy = np.meshgrid(tx, ty)
    return (int(x0), int(y0), int(x1 - x0), int(y1 - y0)), stored_xy(gx, gy, stored_size, rotate, mirror)
