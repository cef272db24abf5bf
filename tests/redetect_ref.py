"""Restatement of the re-detection rules L1-L9 (include/ffl.h), importable without a GPU.
The costs are integers (numpy int64, whose range the rules' bounds stay far inside), so there is no order of summation and
these ARE the kernels' values; the verdict's three compares are numpy float64 scalars, one operation per written operation,
left to right.  The cost surface is accumulated over the (2p+1)^2 template pixels as shifted whole-frame differences of the
frame edge-padded by p: a materialised sliding view of a 1080p frame would need gigabytes."""
import math

import numpy as np

import match_ref
from match_ref import AMBIGUOUS, FLAT, POOR, RECORD_DTYPE, SSD, ZSSD, anchor, clamp, template  # noqa: F401

SKIPPED = 8
MAX_EXCLUDE, MAX_REACH = 32, 32768
DEFAULTS = {"p": 8, "mode": ZSSD, "exclude": 8, "reach": 0, "trigger_mask": POOR, "min_var": 25.0, "max_mse": 400.0,
            "ratio": 0.8}   # the match defaults with exclude = p; not tuned on footage


def params_ok(p, mode, exclude, reach, min_var, max_mse, ratio):
    """the accepted parameters; a NaN fails every compare"""
    ints = all(isinstance(v, (int, np.integer)) for v in (p, exclude, reach))
    return bool(ints and 1 <= p <= match_ref.MAX_P and mode in (SSD, ZSSD) and 1 <= exclude <= MAX_EXCLUDE and
                0 <= reach <= MAX_REACH and 0.0 <= min_var < math.inf and 0.0 <= max_mse <= 65025.0 and 0.0 < ratio <= 1.0)


def window(w, h, ix, iy, reach):
    """rule L2: the candidates' rectangle (x0, x1, y0, y1), inclusive"""
    if reach == 0:
        return 0, w - 1, 0, h - 1
    return max(ix - reach, 0), min(ix + reach, w - 1), max(iy - reach, 0), min(iy + reach, h - 1)


def sums(I, Tm, p, win=None):
    """rule L3: (S1, S2) of the candidates of `win` (None: the whole frame), [cy - y0][cx - x0], as int32: N3 says
    they fit, and the assertion below holds it for any bytes"""
    I = np.asarray(I, np.uint8)
    h, w = I.shape
    x0, x1, y0, y1 = (0, w - 1, 0, h - 1) if win is None else win
    pad = np.pad(I, p, mode="edge").astype(np.int32)       # pad[y + p][x + p] = I[clamp(y)][clamp(x)]
    t = np.asarray(Tm, np.uint8).astype(np.int32)
    nh, nw = y1 - y0 + 1, x1 - x0 + 1
    assert (2 * p + 1) ** 2 * 255 * 255 < 2 ** 31                       # N3: |S1| and S2 fit int32 whatever the bytes are
    S1, S2 = np.zeros((nh, nw), np.int32), np.zeros((nh, nw), np.int32)
    for j in range(2 * p + 1):
        for i in range(2 * p + 1):
            d = pad[y0 + j:y0 + j + nh, x0 + i:x0 + i + nw] - t[j, i]   # row cy + j - p of the frame is row cy + j of pad
            S1 += d
            S2 += d * d
    return S1, S2


def cost_of(S1, S2, p, mode):
    """rule N3 in int64"""
    N, S1, S2 = (2 * p + 1) ** 2, S1.astype(np.int64), S2.astype(np.int64)
    return N * S2 if mode == SSD else N * S2 - S1 * S1


def surface(I, Tm, p, mode, win=None):
    """rule L3: the int64 costs of the candidates of `win` (None: the whole frame), [cy - y0][cx - x0]"""
    return cost_of(*sums(I, Tm, p, win), p, mode)


def verdict(best, second, Tm, p, min_var, max_mse, ratio, strict=False):
    """rule L6 (strict: N6's `>` in the ambiguity test, which the rules do NOT use)"""
    N = (2 * p + 1) ** 2
    t = np.asarray(Tm, np.uint8).astype(np.int64)
    tvar = N * int((t * t).sum()) - int(t.sum()) ** 2
    dN = np.float64(N)
    status = 0
    if np.float64(tvar) < np.float64(min_var) * dN * dN:
        status |= FLAT
    if np.float64(best) > np.float64(max_mse) * dN * dN:
        status |= POOR
    if second >= 0:
        lhs, rhs = np.float64(best), np.float64(ratio) * np.float64(second)
        if (lhs > rhs) if strict else (lhs >= rhs):
            status |= AMBIGUOUS
    return status


def redetect_one(I, Tm, cx, cy, p, mode, exclude, reach, min_var, max_mse, ratio, word=None, mask=POOR, strict=False,
                 full=None):
    """rules L1-L7 for one (item, track): (record as a tuple, accepted).  word None: no trigger words.  full: sums(I, Tm, p) of
    the whole frame where the caller has them already (they do not depend on the centre)."""
    I = np.asarray(I, np.uint8)
    h, w = I.shape
    x, y, ix, iy = anchor(cx, cy, w, h)
    if word is not None and (int(word) & int(mask)) == 0:               # L1
        return (x, y, 0, 0, -1, -1, SKIPPED, 0), False
    x0, x1, y0, y1 = win = window(w, h, ix, iy, reach)
    if full is None:
        cost = surface(I, Tm, p, mode, win)
    else:
        cost = cost_of(full[0][y0:y1 + 1, x0:x1 + 1], full[1][y0:y1 + 1, x0:x1 + 1], p, mode)
    k = int(np.argmin(cost))                                            # L4: the first minimum in row-major order
    by, bx = k // cost.shape[1] + y0, k % cost.shape[1] + x0
    best = int(cost.ravel()[k])
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    far = np.maximum(np.abs(xx - bx), np.abs(yy - by)) > exclude        # L5
    second = int(cost[far].min()) if far.any() else -1
    status = verdict(best, second, Tm, p, min_var, max_mse, ratio, strict)
    if status == 0:                                                     # L7
        x, y = clamp(np.float64(bx), w - 1), clamp(np.float64(by), h - 1)
    return (x, y, bx - ix, by - iy, best, second, status, 0), status == 0


def redetect(frames, templates, centres, p=8, mode=ZSSD, exclude=8, reach=0, trigger_mask=POOR, min_var=25.0, max_mse=400.0,
             ratio=0.8, trigger=None, write_back=True, full=None):
    """Rules L1-L9.  frames: n (h, w) uint8 arrays; templates: (T, 2p+1, 2p+1) uint8; centres: (n, T, 2) float64, any bit
    patterns; trigger: None or (n, T) int32 words; full: None or a function (i, t) -> sums(frames[i], templates[t], p).
    Returns (records (n, T) RECORD_DTYPE, the centres after the call: a copy, and with write_back the accepted ones
    overwritten, every other left bit for bit)."""
    assert params_ok(p, mode, exclude, reach, min_var, max_mse, ratio)
    cen = np.array(centres, np.float64).copy()
    n, T = cen.shape[:2]
    assert len(frames) == n and 1 <= T <= match_ref.MAX_TRACKS and np.asarray(templates).shape == (T, 2 * p + 1, 2 * p + 1)
    rec = np.zeros((n, T), RECORD_DTYPE)
    with np.errstate(all="ignore"):
        for i in range(n):
            for t in range(T):
                r, ok = redetect_one(frames[i], templates[t], cen[i, t, 0], cen[i, t, 1], p, mode, exclude, reach, min_var,
                                     max_mse, ratio, None if trigger is None else trigger[i][t], trigger_mask,
                                     full=None if full is None else full(i, t))
                rec[i, t] = r
                if ok and write_back:                                   # L8
                    cen[i, t] = (r[0], r[1])
    return rec, cen


# ---- the lost-and-found scene ---------------------------------------------------------------------------------------------
JUMP = {"pair": 16, "move": (0, -90), "batch": 11}   # the square is 90 px higher from frame 17 on: in the middle of the second batch of 11


def lost_scene():
    """match_ref.drift_scene with the square moved by JUMP["move"] from frame JUMP["pair"] + 1 on; the flow fields do not show
    the jump (a move the flow under-reads).  Returns (frames, flows, the true integer centres)."""
    d = match_ref.DRIFT
    frames, flows, true = match_ref.drift_scene()
    rng = np.random.default_rng(d["seed"])
    back = rng.integers(0, 256, (d["size"], d["size"]), dtype=np.uint8)
    square = rng.integers(0, 256, (d["side"], d["side"]), dtype=np.uint8)
    frames, flows, true = frames.copy(), flows.copy(), true.copy()
    mx, my = JUMP["move"]
    for k in range(JUMP["pair"] + 1, d["n"] + 1):
        x0, y0 = d["start"][0] + d["step"][0] * k + mx, d["start"][1] + d["step"][1] * k + my
        frames[k] = back
        frames[k, y0:y0 + d["side"], x0:x0 + d["side"]] = square
        true[k] = (x0 + d["side"] // 2, y0 + d["side"] // 2)
        if k < d["n"]:
            flows[k] = 0
            flows[k, y0:y0 + d["side"], x0:x0 + d["side"]] = d["flow"]
    return frames, flows, true


def found_batch(track_ref, frames, flows, st, templates, radius, prm, rprm=None, cuts=None):
    """match_ref.corrected_batch (cuts: rule Q5's outcome per field, None: no cut), then (rprm not None) the re-detection of the
    state on frames[nb] triggered by the state's match records, with write-back.  Returns (track records, match records, the
    state's match records, the state's re-detection records or None, the new state)."""
    rec, mrec, srec, st = match_ref.corrected_batch(track_ref, frames, flows, st, templates, radius, prm, cuts)
    rrec = None
    if rprm is not None:
        scen = np.stack([st["x"], st["y"]], axis=-1)[None]
        rrec, scen = redetect([frames[len(flows)]], templates, scen, trigger=srec["status"], write_back=True, **rprm)
        st = st.copy()
        st["x"], st["y"] = scen[0, :, 0], scen[0, :, 1]
    return rec, mrec, srec, rrec, st
