"""Restatement of the tracking rules Q1-Q9, the ROI rules E1-E5 and the fifth window form (appendices Q
and E; include/ffl.h), importable without a GPU.  Plain numpy float64 scalars, one operation per line where the rules say
"one rounding per written operation", loops in the rules' order: a column top to bottom, the columns left to right.  numpy's
float64 +, *, / are single IEEE operations, so on the rules' inputs these ARE the kernel's bits, not an approximation.

The fifth form composes two restatements that exist: the centre of item j is grid_ref.window (rule G6) over the caller's
centres, and the four components are weights_ref's rule W4 about it; check_window holds a record to weights_ref.check_axes'
bound, which comes from the kernels' code."""
import math

import numpy as np

import grid_ref
import weights_ref

HOLD, HOME = 0, 1
OK, CUT, LOST, CLAMPED = 0, 1, 2, 4
MAX_TRACKS, MAX_RADIUS = 8, 32
FLT_MAX = np.float32(np.finfo(np.float32).max)

STATE_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("home_x", "<f8"), ("home_y", "<f8"), ("steps", "<i8"), ("lost_run", "<i4"),
                        ("pad", "<i4")])
RECORD_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("du", "<f8"), ("dv", "<f8"), ("sw", "<f8"), ("count", "<i4"),
                         ("status", "<i4")])


def state(points, home=None):
    """(T,) STATE_DTYPE out of (x, y) or (T, 2) points; home defaults to the points"""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    hm = p if home is None else np.asarray(home, np.float64).reshape(-1, 2)
    st = np.zeros(len(p), STATE_DTYPE)
    st["x"], st["y"], st["home_x"], st["home_y"] = p[:, 0], p[:, 1], hm[:, 0], hm[:, 1]
    return st


def clamp(c, hi):
    """rule Q1: two selects; a NaN fails c >= 0 and becomes 0"""
    c, hi = np.float64(c), np.float64(hi)
    return (c if c <= hi else hi) if c >= 0.0 else np.float64(0.0)


def window_of(x, y, r, w, h):
    """rule Q2: (x0, x1, y0, y1), inclusive, of the clipped window about a sanitised position"""
    ix, iy = int(math.floor(np.float64(x) + 0.5)), int(math.floor(np.float64(y) + 0.5))
    return max(ix - r, 0), min(ix + r, w - 1), max(iy - r, 0), min(iy + r, h - 1)


def window_sums(flow, W, x0, x1, y0, y1):
    """rules Q3 and Q4: (S, U, V, count)"""
    cols = x1 - x0 + 1
    cS, cU, cV = np.zeros(cols), np.zeros(cols), np.zeros(cols)       # one sum per window column, all starting at +0.0
    count = 0
    for y in range(y0, y1 + 1):                                        # rows top to bottom; the columns side by side
        u, v = flow[y, x0:x1 + 1, 0], flow[y, x0:x1 + 1, 1]
        wb = np.ones(cols, np.int64) if W is None else W[y, x0:x1 + 1].astype(np.int64)
        keep = (wb != 0) & (np.abs(u) <= FLT_MAX) & (np.abs(v) <= FLT_MAX)
        wt = wb.astype(np.float64)
        cS = np.where(keep, cS + wt, cS)                               # a select: nothing of a dropped member reaches a sum
        cU = np.where(keep, cU + wt * u.astype(np.float64), cU)
        cV = np.where(keep, cV + wt * v.astype(np.float64), cV)
        count += int(keep.sum())
    S = U = V = np.float64(0.0)
    for c in range(cols):                                              # the column sums left to right
        S, U, V = S + cS[c], U + cU[c], V + cV[c]
    return S, U, V, count


def advance(flows, cuts, st, radius=12, on_cut=HOLD, maps=None):
    """Rules Q1-Q8 for every track of `st` ((T,) STATE_DTYPE; a copy is advanced) through the n fields `flows` ((n, h, w, 2)
    float32) in order.  cuts: n bools, rule Q5's outcome per item (see mean_mag_cut).  maps: None, one (h, w) uint8 map or
    (n, h, w).  Returns (records (n, T) RECORD_DTYPE, the new state)."""
    flows = np.asarray(flows, np.float32)
    n, h, w, _ = flows.shape
    st = np.array(st, STATE_DTYPE).reshape(-1).copy()
    T = len(st)
    assert 1 <= T <= MAX_TRACKS and 1 <= radius <= MAX_RADIUS and on_cut in (HOLD, HOME)
    maps = None if maps is None else np.asarray(maps)
    rec = np.zeros((n, T), RECORD_DTYPE)
    xmax, ymax = np.float64(w - 1), np.float64(h - 1)
    with np.errstate(all="ignore"):
        for t in range(T):
            x, y = clamp(st["x"][t], xmax), clamp(st["y"][t], ymax)                      # Q1
            hx, hy = clamp(st["home_x"][t], xmax), clamp(st["home_y"][t], ymax)
            steps, lost = int(st["steps"][t]), int(st["lost_run"][t])
            for i in range(n):
                status, du, dv, S, count = OK, np.float64(0.0), np.float64(0.0), np.float64(0.0), 0
                if cuts[i]:                                                              # Q6
                    status |= CUT
                else:
                    W = None if maps is None else maps if maps.ndim == 2 else maps[i]
                    S, U, V, count = window_sums(flows[i], W, *window_of(x, y, radius, w, h))
                    if S == 0.0:
                        status |= LOST
                        lost = (lost + 1 + 2 ** 31) % 2 ** 32 - 2 ** 31                  # wraps as int32
                    else:
                        du, dv = U / S, V / S
                        lost = 0
                if cuts[i] and on_cut == HOME:                                           # Q8
                    nx, ny = hx, hy
                else:
                    rx, ry = x + du, y + dv
                    nx, ny = clamp(rx, xmax), clamp(ry, ymax)
                    if not (nx == rx) or not (ny == ry):
                        status |= CLAMPED
                rec[i, t] = (x, y, du, dv, S, count, status)                             # Q7: the position before the step
                x, y = nx, ny
                steps = (steps + 1 + 2 ** 63) % 2 ** 64 - 2 ** 63
            st[t] = (x, y, hx, hy, steps, lost, st["pad"][t])
    return rec, st


def mean_mag_cut(mean_mag, cut_threshold):
    """rule Q5 on the float32 mean magnitudes ffl_pass1_results reports: NaN is no cut"""
    return [bool(np.float32(m) > np.float32(cut_threshold)) for m in mean_mag]


# ---- ROI maps (appendix E) ------------------------------------------------------------------------------------------------
def roi_map(w, h, centre, ax, ay, soft=True, gate=None):
    """rules E2-E5: the (h, w) uint8 map about `centre` with float32 half-axes ax, ay"""
    cx, cy = np.float64(centre[0]), np.float64(centre[1])
    fax, fay = np.float64(np.float32(ax)), np.float64(np.float32(ay))
    with np.errstate(all="ignore"):
        dx = (np.arange(w, dtype=np.float64) - cx) / fax
        dy = (np.arange(h, dtype=np.float64) - cy) / fay
        e = (dx * dx)[None, :] + (dy * dy)[:, None]
        if soft:
            q = 1.0 - e
            q = np.where(q > 0.0, q, 0.0)          # a select: NaN gives 0
            out = (q * 255.0 + 0.5).astype(np.int64)   # truncation of a value in 0.5 .. 255.5
        else:
            out = np.where(e <= 1.0, 255, 0)
    out = out.astype(np.uint8)
    return out if gate is None else np.minimum(out, np.asarray(gate, np.uint8))


def roi_maps(w, h, centres, ax, ay, soft=True, gate=None):
    """(n, h, w): one map per centre; gate None, (h, w) or (n, h, w)"""
    c = np.asarray(centres, np.float64).reshape(-1, 2)
    g = None if gate is None else np.asarray(gate)
    return np.stack([roi_map(w, h, c[i], ax, ay, soft, None if g is None else g if g.ndim == 2 else g[i]) for i in range(len(c))])


# ---- the fifth window form ------------------------------------------------------------------------------------------------
def window_centres(centres, radius=6):
    """rule G6 over the caller's centres"""
    return grid_ref.window(centres, radius)


def check_window(rec, flow, centres, j, W, pov, radius=6):
    """one record of radial_window_axes_weighted_centres: its centre is rule G6's, bit for bit, and its four components are rule
    W4's about that centre within weights_ref's bound"""
    c = window_centres(centres, radius)[j]
    assert rec["cx"].tobytes() == c[0].tobytes() and rec["cy"].tobytes() == c[1].tobytes(), (rec["cx"], rec["cy"], c)
    got = [rec["dot"], rec["tangential"], rec["shift_x"], rec["shift_y"]]
    if rec["cut"]:
        assert [float(g) for g in got] == [0.0] * 4
        return 0.0
    return weights_ref.check_axes(got, flow, (float(c[0]), float(c[1])), W, pov)
