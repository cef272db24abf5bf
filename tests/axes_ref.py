"""Exact reference for the four motion components about the centre (the four-component pass 2), importable
without a GPU: plain numpy and post_ref's exact sum, no ctypes.

The rule, per pixel (x, y) of an h x w field with float32 flow (u, v) widened to float64 and centre (cx, cy):

    dx = x - cx                     dy = y - cy
    wx = 1 if pov else ((w - x) / w if x > cx else x / w)
    wy = 1 if pov else ((h - y) / h if y > cy else y / h)
    radial     = ((u * dx + v * dy) * wx) * wy          component 0
    tangential = ((v * dx - u * dy) * wx) * wy          component 1, > 0 = clockwise on screen
    shift_x    = (u * wx) * wy                          component 2
    shift_y    = (v * wx) * wy                          component 3

and each component is the sum of its terms divided once by w * h.  axes_terms() performs exactly these float64 operations
in this order; numpy's elementwise float64 arithmetic is the IEEE sequence the kernel executes (the library is built with
-ffp-contract=off, the quotients are single IEEE divisions on both sides), so the restatement's terms ARE the kernel's
terms and only the order of the additions differs.  Hence, with post_ref's count of the longest chain of additions
(radial_depth, which includes the two divisions by w * h):

    components 1..3   |kernel - exact| <= sum_bound(0, radial_depth(w, h)) * S,   S = mean |term|
    component 0       post_ref.check_radial: held against the REFERENCE's term order (8 roundings per term), as ffl_radial is

Nothing here is measured on a device.
"""
import math

import numpy as np

from post_ref import U, check_radial, fsum, radial_depth, sum_bound

AXES = ("radial", "tangential", "shift_x", "shift_y")


def axes_terms(flow, centre, pov=False):
    """the four (h, w) float64 term arrays, in the kernel's operation order"""
    flow = np.asarray(flow, np.float32)
    h, w, _ = flow.shape
    cx, cy = float(centre[0]), float(centre[1])
    u, v = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
    xi, yi = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    x, y = xi.astype(np.float64), yi.astype(np.float64)
    dx, dy = x - cx, y - cy
    if pov:
        wx, wy = np.ones((1, w)), np.ones((h, 1))
    else:
        wx = np.where(x > cx, (w - xi).astype(np.float64) / float(w), x / float(w))
        wy = np.where(y > cy, (h - yi).astype(np.float64) / float(h), y / float(h))
    with np.errstate(all="ignore"):
        return (((u * dx + v * dy) * wx) * wy, ((v * dx - u * dy) * wx) * wy, (u * wx) * wy, (v * wx) * wy)


def axes_exact(flow, centre, pov=False, components=(0, 1, 2, 3)):
    """[(exactly summed mean of the component's terms, S = mean |term|)] for the four components (None for one that was not
    asked for: an exact sum over a large field takes a second).  S only scales the bound: numpy's pairwise sum of the
    non-negative |term| (post_ref.radial_exact's choice)."""
    out = []
    with np.errstate(all="ignore"):
        for c, t in enumerate(axes_terms(flow, centre, pov)):
            out.append((fsum(t) / t.size, float(np.sum(np.abs(t))) / t.size) if c in components else None)
    return out


def axes_bound(w, h, S):
    """components 1..3: the terms are the kernel's own, so the additions on the longest chain are all that differs"""
    return sum_bound(0, radial_depth(w, h)) * S


def check_axes(got, flow, centre, pov, components=(0, 1, 2, 3)):
    """assert the kernel's four values for one item; returns the worst error of components 1..3 in units of u * S"""
    h, w, _ = np.asarray(flow).shape
    exact = axes_exact(flow, centre, pov, [c for c in components if c])
    worst = 0.0
    for c in components:
        g = float(got[c])
        if c == 0:
            check_radial(g, np.asarray(flow, np.float32), (float(centre[0]), float(centre[1])), pov)
            continue
        want, S = exact[c]
        if not math.isfinite(want):
            assert math.isnan(g) == math.isnan(want) and (math.isnan(want) or g == want), (AXES[c], g, want)
            continue
        bound = axes_bound(w, h, S)
        err = abs(g - want)
        assert err <= bound, f"{AXES[c]} {g!r} vs exact {want!r}: off by {err / (U * S) if S else err:.1f} u*S, " \
                             f"bound {bound / (U * S) if S else 0:.0f} (centre {centre}, pov {pov}, {w}x{h})"
        if S:
            worst = max(worst, err / (U * S))
    return worst


def integer_mean(total, w, h):
    """the kernel's value for a component whose terms are integers that sum (exactly) to `total`"""
    return float(total) / (float(w) * float(h))


# ---- fields with known answers: integer-valued, integer centre -------------------------------------------------------------
# In POV mode every term of every component is then an integer far below 2^53, so every order of additions is exact and
# the kernel's value is the exact integer sum divided once by w * h: equality, not a bound.
def _grid(w, h, centre):
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    return x - int(centre[0]) + 0 * y, y - int(centre[1]) + 0 * x


def known_fields(w, h, centre, k=3, a=5, b=-2):
    """{name: (float32 field, [expected component or None] * 4)} for POV mode"""
    dx, dy = _grid(w, h, centre)
    r2 = int((dx * dx + dy * dy).sum())

    def field(u, v):
        f = np.empty((h, w, 2), np.float32)
        f[..., 0], f[..., 1] = u, v
        assert np.array_equal(f[..., 0], u) and np.array_equal(f[..., 1], v)      # integer values a float32 holds exactly
        return f

    m = lambda total: integer_mean(total, w, h)
    return {"rotation": (field(-k * dy, k * dx), [0.0, m(k * r2), m(-k * int(dy.sum())), m(k * int(dx.sum()))]),
            "expansion": (field(k * dx, k * dy), [m(k * r2), 0.0, m(k * int(dx.sum())), m(k * int(dy.sum()))]),
            "uniform": (field(a + 0 * dx, b + 0 * dy), [m(a * int(dx.sum()) + b * int(dy.sum())),
                                                        m(b * int(dx.sum()) - a * int(dy.sum())), float(a), float(b)])}


def weighted_uniform_16(centre, a=5, b=-2):
    """16x16 with the quadrant weights on: w = h = 16 makes every weight a multiple of 1/16, every shift term a multiple of
    1/256 and every sum exact.  (field, expected shift_x, expected shift_y)"""
    w = h = 16
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    wx = np.where(x > centre[0], (w - x) / w, x / w)
    wy = np.where(y > centre[1], (h - y) / h, y / h)
    ww = fsum(wx * wy)            # exact: multiples of 1/256
    f = np.empty((h, w, 2), np.float32)
    f[..., 0], f[..., 1] = a, b
    return f, a * ww / 256.0, b * ww / 256.0
