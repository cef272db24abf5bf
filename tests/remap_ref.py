"""numpy restatement of DESIGN.md appendix R, rules R1 to R6: the operand a source map gathers from an UPRIGHT image, and the
rectangle of the stored frame it touches.

    check(map, S, src)                  rule R1: the valid mask, or ValueError naming the first offender's index
    operand(upright, map, S, rgb)       rules R2 to R5 on an (h, w, 3) image in the order the frame keeps its channels, or on
                                        an (h, w) gray image; int64 throughout
    windows(map, S, stored, rot, mir)   rule R6: the upright bounding box of all taps and the stored rectangle that travels
    hostile_map(out, S, src, seed)      a seeded map uniform over the whole source (or `rect`), with entries at exactly 0
                                        and 32 * (s - 1), fractions 0 and 31, and one sentinel in eight

The image handed to operand() is what the taps yield: a BGR / RGB frame as stored, yuv_ref.yuv_to_bgr (or
front_orient.yuv_to_bgr_full) of a 4:2:0 frame, after yuv16_ref.reduce8 for 16-bit samples.  Integer work: every comparison
built on this module is bit for bit."""
import numpy as np

import front_orient as fo

NONE = -2 ** 31


def _split(map, S):
    m = np.asarray(map)
    assert m.dtype == np.int32 and m.ndim == 3 and m.shape[2] == 2 and m.shape[0] % S == 0 and m.shape[1] % S == 0, m.shape
    return m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)


def check(map, S, src):
    """rule R1 for an upright src = (w, h) source: the (S*oh, S*ow) bool mask of valid entries"""
    if S not in (1, 2, 4):
        raise ValueError(f"supersample {S}")
    qx, qy = _split(map, S)
    valid = qx != NONE
    bad = valid & ((qx < 0) | (qx > 32 * (src[0] - 1)) | (qy < 0) | (qy > 32 * (src[1] - 1)))
    if bad.any():
        raise ValueError(f"entry {int(np.flatnonzero(bad.reshape(-1))[0])}")
    if not valid.any():
        raise ValueError("no valid entry")
    return valid


def taps(map, S, src):
    """rule R2: (valid, x0, x1, y0, y1, fx, fy), the coordinates 0 where the entry is invalid"""
    qx, qy = _split(map, S)
    valid = check(map, S, src)
    qx, qy = np.where(valid, qx, 0), np.where(valid, qy, 0)
    x0, y0 = qx >> 5, qy >> 5
    return valid, x0, np.minimum(x0 + 1, src[0] - 1), y0, np.minimum(y0 + 1, src[1] - 1), qx & 31, qy & 31


def operand(upright, map, S, rgb=False):
    """the (oh, ow) uint8 operand of rules R2 to R5"""
    img = np.asarray(upright).astype(np.int64)
    gray = img.ndim == 2
    if gray:
        img = img[..., None]
    h, w = img.shape[:2]
    valid, x0, x1, y0, y1, fx, fy = taps(map, S, (w, h))
    fx, fy, ok = fx[..., None], fy[..., None], valid[..., None]
    r = (img[y0, x0] * (32 - fx) * (32 - fy) + img[y0, x1] * fx * (32 - fy) + img[y1, x0] * (32 - fx) * fy
         + img[y1, x1] * fx * fy + 512) >> 10                                                            # R3
    r = np.where(ok, r, 0)                                                                               # R4
    H, W = r.shape[:2]
    v = (r.reshape(H // S, S, W // S, S, -1).sum(axis=(1, 3)) + S * S // 2) >> (2 * {1: 0, 2: 1, 4: 2}[S])  # R5
    if gray:
        return v[..., 0].astype(np.uint8)
    red, blue = (v[..., 0], v[..., 2]) if rgb else (v[..., 2], v[..., 0])
    return ((red * 9798 + v[..., 1] * 19235 + blue * 3735 + 16384) >> 15).astype(np.uint8)


def windows(map, S, stored, rotate=0, mirror=False):
    """rule R6 for a stored = (sw, sh) frame: ((x, y, w, h) of all taps in the upright frame, (x, y, w, h) of the stored
    frame: the box's corners through rule Y6, columns rounded out to 16, rows to 2, clamped)"""
    sw, sh = stored
    src = (sh, sw) if rotate in (90, 270) else (sw, sh)
    valid, x0, x1, y0, y1, _, _ = taps(map, S, src)
    ux = np.array([x0[valid].min(), x1[valid].max()])
    uy = np.array([y0[valid].min(), y1[valid].max()])
    px, py = fo.stored_xy(ux, uy, stored, rotate, mirror)
    a, b = int(px.min()) // 16 * 16, int(py.min()) // 2 * 2
    c, d = min((int(px.max()) + 16) // 16 * 16, sw), min((int(py.max()) + 2) // 2 * 2, sh)
    return (int(ux[0]), int(uy[0]), int(ux[1] - ux[0] + 1), int(uy[1] - uy[0] + 1)), (a, b, c - a, d - b)


def hostile_map(out, S, src, seed, rect=None, sentinels=True):
    """an (S*oh, S*ow, 2) int32 map over rect = (x, y, w, h) of the upright src = (w, h) source (None: all of it): uniform
    coordinates in 1/32 px, the first entries forced to the rectangle's extremes (exactly its first and last pixel, so 0 and
    32 * (s - 1) for the whole source) and to the fractions 0 and 31, and every eighth entry on average a sentinel whose qy
    is junk"""
    rng = np.random.default_rng(seed)
    x, y, w, h = (0, 0, src[0], src[1]) if rect is None else rect
    H, W = S * out[1], S * out[0]
    lo = np.array([32 * x, 32 * y])
    hi = np.array([32 * (x + w - 1), 32 * (y + h - 1)])
    m = rng.integers(lo, hi + 1, (H, W, 2)).astype(np.int64)
    forced = [(lo[0], lo[1]), (hi[0], hi[1]), (lo[0], hi[1]), (hi[0], lo[1])]
    if w > 1 and h > 1:
        forced += [(lo[0] + 31, lo[1] + 31), (hi[0] - 1, hi[1] - 32), (hi[0] - 32, hi[1] - 1), (lo[0] + 32, lo[1] + 31)]
    flat = m.reshape(-1, 2)
    spots = rng.permutation(H * W)[:len(forced)]
    if sentinels:
        gone = rng.random(H * W) < 0.125
        gone[spots] = False
        flat[gone, 0] = NONE
        flat[gone, 1] = rng.integers(-2 ** 31, 2 ** 31, int(gone.sum()))
    for k, q in zip(spots, forced):
        flat[k] = q
    return flat.reshape(H, W, 2).astype(np.int32)
