"""The small-shape sweep of the 8-bit front-end (k_frontend, k_frontend_dev; DESIGN.md sections 8, 11, 12): the table of
geometries, seeded content, and a second, independent restatement of the operand.

    OUTS, geoms(ow, oh)     output (context) sizes and, for each, the families of source / resize / crop
    direct_operand(...)     one output pixel straight from its at most four source pixels -- the rules of the header comment
                            of oracle/frontend_oracle.c organised per pixel, where that file (and so tests/yuv_ref.operand)
                            makes two whole-image passes.  The two must agree bit for bit; a kernel must equal both.
    bgr_frame / yuv_frame   uniform noise, a 1-px checkerboard, constant 255, a ramp that tells x, y and the channel apart,
                            and for 4:2:0 the eight corners of (Y, U, V) in {0, 255}^3 (both saturations of appendix Y)
    yuv_planes, yuv_direct  the transfer rule of ffl_upload_frames_yuv, stated once: which bytes travel and whether they go
                            straight out of page-locked memory or through the staging copy

Integer and copy work throughout: every comparison built on this module is bit for bit."""
import functools

import numpy as np

import oracle as orc
import yuv_ref

OUTS = ((16, 16), (17, 19), (65, 21), (130, 16))   # smallest; odd N; two x-tiles + a 1-row y-tile; three x-tiles
MODES = ("identity", "area2", "generic")
BGR_KINDS = ("noise", "checker", "white", "ramp")
YUV_KINDS = BGR_KINDS + ("corners",)


def e(v):
    """v rounded up to even: every source side is even, so one table serves BGR and 4:2:0"""
    return v + (v & 1)


def mode(src, resize):
    """the resize mode front_geometry must choose: both axes decide together"""
    (sw, sh), (rw, rh) = src, resize
    if (rw, rh) == (sw, sh):
        return "identity"
    if (sw, sh) == (2 * rw, 2 * rh):
        return "area2"
    return "generic"


def families(ow, oh):
    """name -> (source (sw, sh), resize (rw, rh)) for an ow x oh context"""
    ident, wide, y_only = (e(ow + 14), e(oh + 10)), (e(ow + 54), e(oh + 10)), (e(3 * ow), e(oh + 6))
    return {
        "identity": (ident, ident),
        "identity_wide": (wide, wide),                                        # a window well inside the rows, x0 > 0
        "area2": ((2 * (ow + 7), 2 * (oh + 5)), (ow + 7, oh + 5)),
        "down_1p5": ((e(int(1.5 * ow) + 9), e(int(1.5 * oh) + 7)), (ow + 5, oh + 3)),
        "down_5p3": ((e(int(5.3 * ow) + 1), e(int(5.3 * oh) + 1)), (ow + 2, oh + 1)),   # non-adjacent taps
        "up_3p7": ((e(ow // 3 + 2), e(oh // 3 + 2)), (ow + 9, oh + 11)),
        "up_from_2x2": ((2, 2), (ow + 3, oh + 2)),
        "x2_only_in_x": ((2 * (ow + 4), e(oh + 9)), (ow + 4, oh + 2)),          # must stay generic
        "identity_only_in_y": (y_only, (ow + 6, y_only[1])),                   # must stay generic
        "exact_fit": ((e(2 * ow + 6), e(2 * oh + 2)), (ow, oh)),
    }


def crops(resize, out):
    """(0, 0), the far corner, and an odd interior point where the free space allows it; no duplicates"""
    fx, fy = resize[0] - out[0], resize[1] - out[1]
    c = [(0, 0), (fx, fy)]
    ix, iy = fx // 2 | 1, fy // 2 | 1
    if ix <= fx and iy <= fy:
        c.append((ix, iy))
    return list(dict.fromkeys(c))


def geoms(ow, oh):
    """[(family, source, resize, crop)] of an ow x oh context"""
    return [(name, src, rs, c) for name, (src, rs) in families(ow, oh).items() for c in crops(rs, (ow, oh))]


# ---- the per-pixel restatement ------------------------------------------------------------------------------------------
def _weights(frac):
    """the two 11-bit weights of a float32 fraction: cvRound (half to even), saturated to short"""
    frac = frac.astype(np.float32)
    w0 = np.rint((np.float32(1) - frac) * np.float32(2048))
    w1 = np.rint(frac * np.float32(2048))
    return np.clip(w0, -32768, 32767).astype(np.int32), np.clip(w1, -32768, 32767).astype(np.int32)


def _coord(d, s, r):
    """output coordinates d of an axis resized from s to r -> (floor of the float32 source coordinate, its fraction)"""
    scale = 1. / (float(r) / s)
    f = ((d.astype(np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    i = np.floor(f)
    return i.astype(np.int64), (f - i).astype(np.float32)


def direct_operand(stored, resize, crop, out, rgb):
    """gray(resize(stored, resize)[crop window of size out]): `stored` an (h, w, 3) uint8 image in the order the frame
    keeps its channels -- B, G, R, or with rgb R, G, B."""
    S = np.asarray(stored).astype(np.int32)
    sh, sw = S.shape[:2]
    (rw, rh), (cx, cy), (ow, oh) = resize, crop, out
    dx, dy = np.arange(cx, cx + ow), np.arange(cy, cy + oh)
    m = mode((sw, sh), (rw, rh))
    if m == "identity":                                   # the reference skips a same-size resize: a plain fetch
        v = S[dy[:, None], dx[None, :]]
    elif m == "area2":                                    # INTER_LINEAR re-routed to INTER_AREA: the 2x2 mean
        y, x = 2 * dy[:, None], 2 * dx[None, :]
        v = (S[y, x] + S[y, x + 1] + S[y + 1, x] + S[y + 1, x + 1] + 2) >> 2
    else:
        sx, fx = _coord(dx, sw, rw)
        lo, hi = sx < 0, sx >= sw - 1                     # x only: a clamped column loses its fraction
        sx = np.where(lo, 0, np.where(hi, sw - 1, sx))
        fx = np.where(lo | hi, np.float32(0), fx)
        sx1 = np.minimum(sx + 1, sw - 1)
        sy, fy = _coord(dy, sh, rh)                       # y: the rows are clamped, the fraction is kept
        y0, y1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
        (a0, a1), (b0, b1) = _weights(fx), _weights(fy)
        a0, a1, b0, b1 = a0[None, :, None], a1[None, :, None], b0[:, None, None], b1[:, None, None]
        h0 = S[y0[:, None], sx[None, :]] * a0 + S[y0[:, None], sx1[None, :]] * a1
        h1 = S[y1[:, None], sx[None, :]] * a0 + S[y1[:, None], sx1[None, :]] * a1
        v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
    v = v & 255                                           # the resize stores uchar
    r, b = (v[..., 0], v[..., 2]) if rgb else (v[..., 2], v[..., 0])
    return ((r * 9798 + v[..., 1] * 19235 + b * 3735 + 16384) >> 15).astype(np.uint8)


def oracle_operand(stored, resize, crop, out, rgb):
    """the same through oracle/frontend_oracle.c: whole-image resize, then crop, then luma"""
    img = np.ascontiguousarray(stored) if rgb else orc.swap_rb(np.ascontiguousarray(stored))
    if (img.shape[1], img.shape[0]) != tuple(resize):
        img = orc.resize_linear_u8c3(img, int(resize[0]), int(resize[1]))
    (cx, cy), (ow, oh) = crop, out
    return orc.rgb2gray(img[cy:cy + oh, cx:cx + ow])


def yuv_direct_operand(frame, layout, resize, crop, out):
    """direct_operand of a (3h/2, w) 4:2:0 frame: appendix Y's B, G, R per source pixel, then the per-pixel form"""
    return direct_operand(yuv_ref.yuv_to_bgr(frame, layout), resize, crop, out, False)


# ---- content ------------------------------------------------------------------------------------------------------------
def bgr_frame(kind, w, h, seed):
    """an (h, w, 3) uint8 frame of one of BGR_KINDS"""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "checker":
        return (((x + y + seed) & 1) * 255).astype(np.uint8)
    if kind == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if kind == "ramp":                                    # x, y and the channel enter differently: a swap of any two shows
        return ((7 * x + 29 * y + 83 * c + 3 * x * (c + 1) + seed) % 256).astype(np.uint8)
    raise ValueError(kind)


def pack420(Y, U, V, layout):
    """(h, w), (h/2, w/2), (h/2, w/2) uint8 planes -> cv2's single (3h/2, w) array"""
    h, w = Y.shape
    if layout == "nv12":
        uv = np.empty((h // 2, w), np.uint8)
        uv[:, 0::2], uv[:, 1::2] = U, V
        return np.ascontiguousarray(np.concatenate([Y, uv]))
    return np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).astype(np.uint8).reshape(h * 3 // 2, w)


def yuv_frame(kind, w, h, layout, seed):
    """a (3h/2, w) uint8 4:2:0 frame of one of YUV_KINDS (w, h even)"""
    ch, cw = h // 2, w // 2
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    v, u = np.meshgrid(np.arange(ch), np.arange(cw), indexing="ij")
    if kind == "noise":
        r = np.random.default_rng(seed)
        Y, U, V = r.integers(0, 256, (h, w)), r.integers(0, 256, (ch, cw)), r.integers(0, 256, (ch, cw))
    elif kind == "checker":
        Y, U, V = ((x + y + seed) & 1) * 255, ((u + v + seed) & 1) * 255, ((u + v + seed + 1) & 1) * 255
    elif kind == "white":
        Y, U, V = np.full((h, w), 255), np.full((ch, cw), 255), np.full((ch, cw), 255)
    elif kind == "ramp":
        Y, U, V = (7 * x + 29 * y + seed) % 256, (11 * u + 53 * v + 90 + seed) % 256, (37 * u + 5 * v + 170 + seed) % 256
    elif kind == "corners":                               # block (bx, by) holds corner (bx + 3 by + seed) % 8 of {0, 255}^3
        k = (u + 3 * v + seed) % 8
        U, V = (k >> 1 & 1) * 255, (k >> 2 & 1) * 255
        Y = np.repeat(np.repeat((k & 1) * 255, 2, 0), 2, 1)
    else:
        raise ValueError(kind)
    return pack420(Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8), layout)


# ---- the transfer rule of ffl_upload_frames_yuv (8-bit) -----------------------------------------------------------------------
def yuv_planes(src, layout, stride, window):
    """[(byte offset in the frame array, row pitch, row bytes, rows)] of the planes ffl_upload_frames_yuv transfers for
    `window` = (x0, y0, w, h) of a src = (sw, sh) frame whose rows are `stride` bytes apart: Y, then U and V (I420, planes
    of sw/2 x sh/2 behind the luma) or the interleaved UV rows (NV12)"""
    (sw, sh), (x0, y0, w, h) = src, window
    luma = (y0 * stride + x0, stride, w, h)
    if layout == "nv12":
        return [luma, ((sh + y0 // 2) * stride + x0, stride, w, h // 2)]
    cw = sw // 2
    u0 = sh * sw + (y0 // 2) * cw + x0 // 2
    return [luma, (u0, cw, w // 2, h // 2), (u0 + (sh // 2) * cw, cw, w // 2, h // 2)]


def yuv_direct(address, src, layout, stride, window):
    """The rule that chooses between one 2-D copy per plane straight out of page-locked memory (True) and the staging
    copy (False) for a frame array at `address` inside ffl_host_alloc memory: every plane's rows must start 4-byte aligned
    and be a multiple of 4 bytes long -- first row address, pitch and row bytes all multiples of 4.  Frames outside
    ffl_host_alloc memory are always staged."""
    return all((address + off) % 4 == 0 and pitch % 4 == 0 and row % 4 == 0
               for off, pitch, row, _ in yuv_planes(src, layout, stride, window))


def zero_copy_addresses(src, n=2):
    """byte offsets of the n frames of the zero-copy placement the GPU sweep uses -- one ctx.pinned_frames(n, size=src,
    yuv=True) array per table row, frame i at i * 3/2 * sw * sh -- relative to the allocation, which is page aligned (the
    GPU test asserts it is 4-byte aligned; the rule needs no more)"""
    return [i * src[0] * src[1] * 3 // 2 for i in range(n)]


# ---- cases with their references, computed once per output size ---------------------------------------------------------
def kinds_for(k, kinds, n=2):
    """the content kinds of the n frames of table row k: consecutive rows and frames cycle through `kinds`; frames beyond
    one cycle are noise, so that no two frames of a row are alike (every frame has a seed of its own)"""
    return [kinds[(k + i) % len(kinds)] if i < len(kinds) else "noise" for i in range(n)]


def both(stored, resize, crop, out, rgb):
    """the operand, after checking that the two restatements agree on it"""
    a, b = oracle_operand(stored, resize, crop, out, rgb), direct_operand(stored, resize, crop, out, rgb)
    assert np.array_equal(a, b), "the two restatements disagree: the bug is in the test infrastructure"
    return a


@functools.lru_cache(maxsize=None)
def bgr_cases(out, n=2):
    """[(family, src, resize, crop, frames, operands read as BGR, operands read as RGB)] for an output size"""
    rows = []
    for k, (name, src, rs, crop) in enumerate(geoms(*out)):
        fr = [bgr_frame(kind, src[0], src[1], 100 * k + i) for i, kind in enumerate(kinds_for(k, BGR_KINDS, n))]
        rows.append((name, src, rs, crop, fr, [both(f, rs, crop, out, False) for f in fr], [both(f, rs, crop, out, True) for f in fr]))
    return rows


@functools.lru_cache(maxsize=None)
def yuv_cases(out, layout, n=2):
    """[(family, src, resize, crop, frames, operands)] for an output size and a 4:2:0 layout"""
    rows = []
    for k, (name, src, rs, crop) in enumerate(geoms(*out)):
        fr = [yuv_frame(kind, src[0], src[1], layout, 100 * k + i) for i, kind in enumerate(kinds_for(k, YUV_KINDS, n))]
        ops = []
        for f in fr:
            op = yuv_ref.operand(f, layout, rs, crop, out)
            assert np.array_equal(op, yuv_direct_operand(f, layout, rs, crop, out)), "the two restatements disagree"
            ops.append(op)
        rows.append((name, src, rs, crop, fr, ops))
    return rows


def slot_pattern(slot, out):
    """what a frame slot holds before the sweep writes it: distinct per slot, never constant along a row or a column"""
    ow, oh = out
    i = np.arange(ow * oh, dtype=np.int64)
    return ((i * 7 + (i // ow) * 13 + slot * 31 + 5) % 251).astype(np.uint8).reshape(oh, ow)
