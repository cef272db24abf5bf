"""Restatement of the weight-map rules W1-W6 (include/ffl.h), importable without a GPU:
plain numpy on top of post_ref's exact sum and divergence and axes_ref's terms.

The rules, for an (h, w) uint8 map W over a float32 field:

  W1  wt = float64(W[y, x]); W == 0 excludes the pixel (np.where, never a product); SW = sum of wt, an exact integer.
  W2  the divergence is post_ref.divergence of the whole field; the candidates of the argmax are the pixels with W > 0;
      among them the first NaN of |div| in row-major order, else the first maximum.
  W3  mean_mag = float32(sum(float64(mag) * wt) / SW), mag = post_ref.mag_terms.
  W4  component c = sum(axes_ref.axes_terms(...)[c] * wt) / SW.
  W5  SW == 0: (x, y, div_val, mean_mag, cut) = (w // 2, h // 2, +0.0, +0.0, False) and four +0.0.
  W6  a cut item is four +0.0.

Error bounds, from the kernels' code (kernels_post.hip), not from device output:

  components  ffl_radial_body forms ((...) * wx) * wy exactly as axes_terms does (float64, -ffp-contract=off, the quotients
              single IEEE divisions on both sides) and multiplies once more by the float64 weight: numpy's elementwise
              product is that operation, so the restatement's weighted terms ARE the kernel's for all four components
              (component 0 included: it is held against the kernel's own term order here, not the reference's).  What
              differs is the order of the additions and nothing else.  The longest chain of additions a term passes
              through is post_ref's: 2 * 16 in a lane, 6 shuffle steps, 3 waves, ceil(nblk / 256) trips of the final
              kernel's loop, its 6 + 3, then the kernel's one division by SW and the restatement's one division of the
              correctly rounded sum -- post_ref.radial_depth(w, h), which already counts the two divisions.  Excluded
              pixels add +0.0 and cost nothing.  SW itself is exact in any order (integers below 2^53).  Hence
                  |kernel - exact| <= sum_bound(0, radial_depth(w, h)) * S,    S = sum |term * wt| / SW.
  mean_mag    mag * wt is exact in float64 (24 x 8 bits), so the terms are again the kernel's; the chain is k_pass1's
              (post_ref.pass1_depth, which counts the division by SW done in k_pass1_weighted_final and the
              restatement's).  Accepted as post_ref.mean_mag_accepted accepts the unweighted mean: float32 of the exact
              weighted mean, or both neighbours when it lies within sum_bound(0, pass1_depth) * mean of a rounding boundary.
"""
import math

import numpy as np

from axes_ref import AXES, axes_terms
from post_ref import U, divergence, fsum, mag_terms, pass1_depth, radial_depth, sum_bound


def weights_of(W):
    W = np.asarray(W)
    assert W.dtype in (np.uint8, np.bool_) and W.ndim == 2, (W.dtype, W.shape)
    return W.astype(np.float64)


def total_weight(W):
    """SW: an exact integer"""
    return int(np.asarray(W).astype(np.int64).sum())


def argmax_weighted(flow, W):
    """(x, y, div[y, x]) under rule W2; None when no pixel is a candidate"""
    div = divergence(flow)
    a = np.abs(div).ravel()
    cand = np.asarray(W).ravel() > 0
    if not cand.any():
        return None
    nan = np.isnan(a) & cand
    if nan.any():
        idx = int(np.flatnonzero(nan)[0])
    else:
        idx = int(np.flatnonzero(cand & (a == a[cand].max()))[0])
    y, x = divmod(idx, div.shape[1])
    return x, y, div[y, x]


def mag_exact_weighted(flow, W):
    """the exact weighted mean of rule W3 as a float (NaN / inf where a candidate's magnitude is); +0.0 when SW == 0"""
    wt, sw = weights_of(W), total_weight(W)
    if sw == 0:
        return 0.0
    with np.errstate(all="ignore"):
        t = np.where(wt > 0, mag_terms(flow).astype(np.float64) * wt, 0.0)
    return fsum(t) / float(sw)


def mean_mag_accepted(flow, W):
    """(exact weighted mean, the float32 values the kernel's mean_mag may take)"""
    h, w, _ = np.asarray(flow).shape
    mean = mag_exact_weighted(flow, W)
    if not math.isfinite(mean):
        return mean, (np.float32(mean),)
    b = sum_bound(0, pass1_depth(w, h)) * mean
    return mean, tuple({np.float32(mean - b), np.float32(mean + b)})


def check_mean_mag(got, flow, W):
    mean, ok = mean_mag_accepted(flow, W)
    if math.isnan(mean):
        assert math.isnan(float(got)), (got, mean)
    else:
        assert np.float32(got) in ok, f"mean_mag {float(got)!r} not in {[float(v) for v in ok]} (exact {mean!r})"
    return mean


def pass1_record(flow, W, pov=False, cut_threshold=7.0):
    """(x, y, div_val, exact mean, cut) of rules W2, W3, W5; cut is judged on float32(exact mean)"""
    h, w, _ = np.asarray(flow).shape
    if total_weight(W) == 0:
        return w // 2, h // 2, np.float32(0.0), 0.0, False
    mean = mag_exact_weighted(flow, W)
    if pov:
        x, y, d = w // 2, h - 1, np.float32(0.0)
    else:
        x, y, d = argmax_weighted(flow, W)
    return x, y, d, mean, bool(np.float32(mean) > np.float32(cut_threshold))


def weighted_terms(flow, centre, W, pov=False):
    """the four (h, w) float64 arrays term * wt, +0.0 where W == 0"""
    wt = weights_of(W)
    with np.errstate(all="ignore"):
        return tuple(np.where(wt > 0, t * wt, 0.0) for t in axes_terms(flow, centre, pov))


def axes_exact_weighted(flow, centre, W, pov=False):
    """[(exact component, S = sum |term * wt| / SW)] * 4; four (+0.0, 0.0) when SW == 0 (rule W5)"""
    sw = total_weight(W)
    if sw == 0:
        return [(0.0, 0.0)] * 4
    with np.errstate(all="ignore"):
        return [(fsum(t) / float(sw), float(np.sum(np.abs(t))) / float(sw)) for t in weighted_terms(flow, centre, W, pov)]


def axes_bound(w, h, S):
    return sum_bound(0, radial_depth(w, h)) * S


def check_axes(got, flow, centre, W, pov):
    """assert the kernel's four values for one item under the map; returns the worst error in units of u * S"""
    h, w, _ = np.asarray(flow).shape
    worst = 0.0
    for c, (want, S) in enumerate(axes_exact_weighted(flow, centre, W, pov)):
        g = float(got[c])
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


def known_weighted(field, centre, W):
    """The kernel's four values for an integer-valued field, an integer centre, POV mode and integer weights: every term and
    every product by a weight is an integer far below 2^53, every order of additions is exact, and the value is
    float(total) / float(SW) -- equality, not a bound.  Integer arithmetic throughout (np.int64), independent of axes_terms."""
    f = np.asarray(field, np.float32)
    h, w, _ = f.shape
    u, v = f[..., 0].astype(np.int64), f[..., 1].astype(np.int64)
    assert np.array_equal(u, f[..., 0]) and np.array_equal(v, f[..., 1])
    dx = np.arange(w, dtype=np.int64)[None, :] - int(centre[0])
    dy = np.arange(h, dtype=np.int64)[:, None] - int(centre[1])
    q = np.asarray(W).astype(np.int64)
    sw = int(q.sum())
    if sw == 0:
        return [0.0] * 4
    totals = [int(((u * dx + v * dy) * q).sum()), int(((v * dx - u * dy) * q).sum()), int((u * q).sum()), int((v * q).sum())]
    return [float(t) / float(sw) for t in totals]
