"""Restatement of the template-matching rules N1-N10 (include/ffl.h), importable without a
GPU.  The costs are integers (numpy int64, whose range the rules' bounds stay far inside), so there is no order of summation
and these ARE the kernel's values; the verdict's three compares are numpy float64 scalars, one operation per written
operation, left to right."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SSD, ZSSD = 0, 1
FLAT, POOR, AMBIGUOUS = 1, 2, 4
MAX_P, MAX_S, MAX_TRACKS = 16, 16, 8
DEFAULTS = {"p": 8, "s": 8, "mode": ZSSD, "min_var": 25.0, "max_mse": 400.0, "ratio": 0.8}   # not tuned on footage

RECORD_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("dx", "<i4"), ("dy", "<i4"), ("cost", "<i8"), ("second", "<i8"),
                         ("status", "<i4"), ("pad", "<i4")])


def params_ok(p, s, mode, min_var, max_mse, ratio):
    """the accepted parameters; a NaN fails every compare"""
    return bool(isinstance(p, (int, np.integer)) and isinstance(s, (int, np.integer)) and 1 <= p <= MAX_P and 1 <= s <= MAX_S and
                mode in (SSD, ZSSD) and 0.0 <= min_var < math.inf and 0.0 <= max_mse <= 65025.0 and 0.0 < ratio <= 1.0)


def clamp(c, hi):
    """rule Q1: two selects; a NaN fails c >= 0 and becomes 0"""
    c, hi = np.float64(c), np.float64(hi)
    return (c if c <= hi else hi) if c >= 0.0 else np.float64(0.0)


def anchor(cx, cy, w, h):
    """rule N1: the sanitised centre and rule Q2's rounding"""
    x, y = clamp(cx, w - 1), clamp(cy, h - 1)
    return x, y, int(math.floor(x + np.float64(0.5))), int(math.floor(y + np.float64(0.5)))


def patch(I, ix, iy, half):
    """the (2 half + 1)^2 samples about (ix, iy), coordinates clamped (rules N2 and N10), as int64"""
    h, w = I.shape
    ys = np.clip(np.arange(iy - half, iy + half + 1), 0, h - 1)
    xs = np.clip(np.arange(ix - half, ix + half + 1), 0, w - 1)
    return I[np.ix_(ys, xs)].astype(np.int64)


def template(I, centres, p):
    """rule N10: (T, 2p+1, 2p+1) uint8 about the centres (T, 2) (any bit patterns)"""
    I = np.asarray(I, np.uint8)
    h, w = I.shape
    c = np.asarray(centres, np.float64).reshape(-1, 2)
    out = np.zeros((len(c), 2 * p + 1, 2 * p + 1), np.uint8)
    for t in range(len(c)):
        _, _, ix, iy = anchor(c[t, 0], c[t, 1], w, h)
        out[t] = patch(I, ix, iy, p).astype(np.uint8)
    return out


def surface(I, Tm, ix, iy, p, s, mode):
    """rules N2 and N3: the (2s+1, 2s+1) int64 costs, [dy + s][dx + s]"""
    win = patch(I, ix, iy, p + s)                                       # row dy + s + j, column dx + s + i
    d = sliding_window_view(win, (2 * p + 1, 2 * p + 1)) - Tm.astype(np.int64)[None, None]
    S1, S2 = d.sum(axis=(2, 3)), (d * d).sum(axis=(2, 3))
    assert np.abs(S1).max() < 2 ** 31 and S2.max() < 2 ** 31            # N3: they fit int32
    N = (2 * p + 1) ** 2
    return N * S2 if mode == SSD else N * S2 - S1 * S1


def match_one(I, Tm, cx, cy, p, s, mode, min_var, max_mse, ratio):
    """rules N1-N7 for one (item, track): (record as a tuple, accepted)"""
    h, w = I.shape
    x, y, ix, iy = anchor(cx, cy, w, h)
    cost = surface(I, Tm, ix, iy, p, s, mode)
    off = np.arange(-s, s + 1)
    dx, dy = np.meshgrid(off, off)                                      # [dy + s][dx + s]
    k = np.lexsort((dx.ravel(), dy.ravel(), (dx * dx + dy * dy).ravel(), cost.ravel()))[0]   # N4: (cost, dist^2, dy, dx)
    bdx, bdy, best = int(dx.ravel()[k]), int(dy.ravel()[k]), int(cost.ravel()[k])
    far = np.maximum(np.abs(dx - bdx), np.abs(dy - bdy)) > 1            # N5
    second = int(cost[far].min()) if far.any() else -1
    N = (2 * p + 1) ** 2
    t = Tm.astype(np.int64)
    tvar = N * int((t * t).sum()) - int(t.sum()) ** 2
    dN = np.float64(N)
    status = 0                                                          # N6
    if np.float64(tvar) < np.float64(min_var) * dN * dN:
        status |= FLAT
    if np.float64(best) > np.float64(max_mse) * dN * dN:
        status |= POOR
    if second >= 0 and np.float64(best) > np.float64(ratio) * np.float64(second):
        status |= AMBIGUOUS
    if status == 0:                                                     # N7
        x, y = clamp(np.float64(ix + bdx), w - 1), clamp(np.float64(iy + bdy), h - 1)
    return (x, y, bdx, bdy, best, second, status, 0), status == 0


def match(frames, templates, centres, p=8, s=8, mode=ZSSD, min_var=25.0, max_mse=400.0, ratio=0.8, write_back=True):
    """Rules N1-N9.  frames: n (h, w) uint8 arrays, item i's frame; templates: (T, 2p+1, 2p+1) uint8; centres: (n, T, 2)
    float64, any bit patterns.  Returns (records (n, T) RECORD_DTYPE, the centres after the call: a copy, and with write_back
    the accepted ones overwritten, every other left bit for bit)."""
    assert params_ok(p, s, mode, min_var, max_mse, ratio)
    cen = np.array(centres, np.float64).copy()
    n, T = cen.shape[:2]
    assert len(frames) == n and 1 <= T <= MAX_TRACKS and np.asarray(templates).shape == (T, 2 * p + 1, 2 * p + 1)
    rec = np.zeros((n, T), RECORD_DTYPE)
    with np.errstate(all="ignore"):
        for i in range(n):
            I = np.asarray(frames[i], np.uint8)
            for t in range(T):
                r, ok = match_one(I, np.asarray(templates[t], np.uint8), cen[i, t, 0], cen[i, t, 1], p, s, mode, min_var, max_mse,
                                  ratio)
                rec[i, t] = r
                if ok and write_back:                                   # N8
                    cen[i, t] = (r[0], r[1])
    return rec, cen


# ---- the drift scene and the corrected run --------------------------------------------------------------------------------
DRIFT = {"size": 256, "side": 64, "n": 33, "step": (2, -1), "flow": (2.3, -1.0), "start": (40, 150), "radius": 7, "p": 8, "s": 12,
         "split": 17, "seed": 5}


def drift_scene(seed=DRIFT["seed"]):
    """A 64-px random square that moves (2, -1) per frame over static noise, and fields that read (2.3, -1) inside the square
    (0 outside): the flow's bias of 0.3 px per frame is what a tracker integrates.  Returns (frames (n + 1, 256, 256) uint8,
    flows (n, 256, 256, 2) float32, the true centres (n + 1, 2) of the square -- integers)."""
    d, rng = DRIFT, np.random.default_rng(seed)
    size, side, n = d["size"], d["side"], d["n"]
    back = rng.integers(0, 256, (size, size), dtype=np.uint8)
    square = rng.integers(0, 256, (side, side), dtype=np.uint8)
    frames = np.repeat(back[None], n + 1, axis=0)
    flows = np.zeros((n, size, size, 2), np.float32)
    true = np.zeros((n + 1, 2), np.float64)
    for k in range(n + 1):
        x0, y0 = d["start"][0] + d["step"][0] * k, d["start"][1] + d["step"][1] * k
        frames[k, y0:y0 + side, x0:x0 + side] = square
        true[k] = (x0 + side // 2, y0 + side // 2)
        if k < n:
            flows[k, y0:y0 + side, x0:x0 + side] = d["flow"]
    return frames, flows, true


def corrected_batch(track_ref, frames, flows, st, templates, radius, prm, cuts=None):
    """One batch of the corrected schedule on the restatements (track_ref: the tracking restatement's module): advance through
    `flows` (nb fields; frames holds their nb + 1 frames), match the records on frames[:nb] with write-back, match the state
    on frames[nb] with write-back.  Returns (track records with corrected heads, match records, the state's match records,
    the new state)."""
    nb = len(flows)
    rec, st = track_ref.advance(flows, [False] * nb if cuts is None else cuts, st, radius)
    cen = np.stack([rec["x"], rec["y"]], axis=-1)
    mrec, cen = match(list(frames[:nb]), templates, cen, write_back=True, **prm)
    rec["x"], rec["y"] = cen[..., 0], cen[..., 1]
    scen = np.stack([st["x"], st["y"]], axis=-1)[None]
    srec, scen = match([frames[nb]], templates, scen, write_back=True, **prm)
    st = st.copy()
    st["x"], st["y"] = scen[0, :, 0], scen[0, :, 1]
    return rec, mrec, srec, st
