"""Exact references for the post kernels (kernels_post.hip), importable without a GPU: plain numpy and math.fsum, no
ctypes, no oracle library.

The reference's radial_motion_weighted (FF:761-785) is float64 throughout and so is pass 2's k_strip_sums, so the two differ only in how
each term is rounded and in the order the terms are added.  Both are bounded here from the code, not from device output:

  per term   reference  ((dot * (w - x)) / w * (h - y)) / h           4 roundings after `dot`
             kernel     dot * ((w - x) / w) * wytab[y]                2 quotients + 2 products = 4 roundings
             `dot` = u * dx + v * dy is formed the same way by both (the library is built with -ffp-contract=off), so it
             cancels; each rounding moves a term by at most u * |term| (u = 2^-53, first order): 8 * u * |term| in all.
  summation  every addition a term passes through multiplies it by (1 + d), |d| <= u.  The longest chain of additions
             in k_strip_sums / k_radial_final (and equally k_pass1 / k_pass1_final for the magnitude sum) is
               2 * 16   a lane adds its two pixels of each of the 16 rows of its row group, in sequence
               6        __shfl_down steps of the wave sum
               3        thread 0 adds the other three waves' sums
               trips    ceil(nblk / 256) sequential adds per thread of the final kernel's loop
               6 + 3    its wave sum and its four waves
             plus one rounding for the kernel's division by w * h (radial) or the host's division by w * h (mean
             magnitude) and one for the reference's own division of the exactly rounded fsum:
               depth = 32 + 6 + 3 + trips + 6 + 3 + 2
             which is 56 for pass 2 at 3840x2160 (nblk = 1013, 4 trips) and 61 for k_pass1 at 5760x2880 (nblk = 2070,
             9 trips).
  so         |kernel - radial_exact| <= sum_bound(8, depth) * S,   S = sum |term| / (w * h),
             about 7e-15 * S.  The bound is relative to S, not to the result: a field whose terms cancel is held to the
             same absolute error as one whose terms do not.

Non-finite rule of pass 1 (np.argmax(np.abs(div)), FF:756): the first NaN of |div| in row-major order wins whatever its
payload; without a NaN the first maximum (+inf included) wins.
"""
import itertools
import math

import numpy as np

U = 2.0 ** -53
P1_STRIP, P2_STRIP, ROW_GROUP, THREADS = 126, 128, 16, 256   # kernels_post.hip


def fsum(a, chunk=1 << 20):
    """math.fsum of a numpy array: the correctly rounded sum, fed in chunks to bound memory.  A sum with a NaN, or with
    infinities of both signs, is NaN (math.fsum raises on the latter); one with infinities of one sign is that infinity."""
    a = np.ascontiguousarray(a, np.float64).ravel()
    if not np.isfinite(a).all():
        with np.errstate(invalid="ignore"):
            return float(np.sum(a[~np.isfinite(a)]))
    return math.fsum(itertools.chain.from_iterable(a[i:i + chunk].tolist() for i in range(0, a.size, chunk)))


def radial_terms(flow, centre, pov=False):
    """weighted_dot of FF:761-785 before its np.mean: the reference's operations in the reference's order, float64."""
    h, w, _ = flow.shape
    y, x = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]   # np.indices, broadcast
    dx = x - centre[0]
    dy = y - centre[1]
    dot = flow[..., 0] * dx + flow[..., 1] * dy
    if pov:
        return dot
    wd = np.where(x > centre[0], dot * (w - x) / w, dot * x / w)
    return np.where(y > centre[1], wd * (h - y) / h, wd * y / h)


def radial_exact(flow, centre, pov=False):
    """(exactly summed mean of the reference's terms, S = mean |term|).  S only scales the bound, so it is numpy's pairwise
    sum of the non-negative |term| (relative error below 1e-13) rather than a second exact sum."""
    with np.errstate(all="ignore"):
        t = radial_terms(np.asarray(flow, np.float32), (float(centre[0]), float(centre[1])), pov)
        n = t.shape[0] * t.shape[1]
        return fsum(t) / n, float(np.sum(np.abs(t))) / n


def mag_terms(flow):
    """sqrtf(u * u + v * v) in float32 as k_pass1 forms it: two products, one sum, one correctly rounded square root, no
    contraction.  numpy float32 arithmetic is the same IEEE operation sequence."""
    flow = np.asarray(flow, np.float32)
    u, v = flow[..., 0], flow[..., 1]
    with np.errstate(all="ignore"):
        return np.sqrt(u * u + v * v)


def mag_exact(flow):
    """(mean of the kernel's float32 terms from their exact sum, that sum): the mean is the correctly rounded sum divided
    once, i.e. within 2 u of the true mean (counted in pass1_depth)."""
    t = mag_terms(flow)
    s = fsum(t)
    return s / t.size, s


def divergence(flow):
    """div of FF:754, float32: np.gradient(u, axis=0) + np.gradient(v, axis=1), restated as oracle.max_divergence_np does."""
    flow = np.asarray(flow, np.float32)
    u, v = flow[..., 0], flow[..., 1]
    with np.errstate(all="ignore"):
        du = np.empty_like(u)
        du[1:-1] = (u[2:] - u[:-2]) / np.float32(2.0)
        du[0] = u[1] - u[0]
        du[-1] = u[-1] - u[-2]
        dv = np.empty_like(v)
        dv[:, 1:-1] = (v[:, 2:] - v[:, :-2]) / np.float32(2.0)
        dv[:, 0] = v[:, 1] - v[:, 0]
        dv[:, -1] = v[:, -1] - v[:, -2]
        return du + dv


def argmax_ref(flow):
    """(x, y, div[y, x]) of the reference's max_divergence with np.argmax's rule spelled out: the first NaN of |div| in C
    order if there is one, else the first maximum."""
    div = divergence(flow)
    a = np.abs(div).ravel()
    nan = np.isnan(a)
    if nan.any():
        idx = int(np.flatnonzero(nan)[0])
    else:
        idx = int(np.flatnonzero(a == a.max())[0])
    y, x = divmod(idx, div.shape[1])
    return x, y, div[y, x]


def sum_bound(n_roundings_per_term, depth):
    """relative to S: n roundings per term plus `depth` additions on the longest chain, each at most u = 2^-53"""
    return (n_roundings_per_term + depth) * U


def _depth(w, h, strip):
    waves = -(-w // strip) * -(-h // ROW_GROUP)
    nblk = -(-waves // 4)
    return 2 * ROW_GROUP + 6 + 3 + -(-nblk // THREADS) + 6 + 3 + 2, nblk


def radial_depth(w, h):
    return _depth(w, h, P2_STRIP)[0]


def pass1_depth(w, h):
    return _depth(w, h, P1_STRIP)[0]


def pass1_blocks(w, h):
    """partials per field that k_pass1_final reduces (ffl_pass1_blocks)"""
    return _depth(w, h, P1_STRIP)[1]


def pass1_block_of(w, x, y):
    """index of the k_pass1 workgroup (= slot of k_pass1_final's loop) that owns pixel (x, y)"""
    nstrips = -(-w // P1_STRIP)
    return ((y // ROW_GROUP) * nstrips + x // P1_STRIP) // 4


def check_radial(got, flow, centre, pov):
    """assert the kernel's radial value against radial_exact; returns (error, bound) in units of u * S for printing"""
    h, w, _ = flow.shape
    want, S = radial_exact(flow, centre, pov)
    if not math.isfinite(want):
        assert math.isnan(got) == math.isnan(want) and (math.isnan(want) or got == want), (got, want)
        return 0.0, 0.0
    bound = sum_bound(8, radial_depth(w, h)) * S
    err = abs(got - want)
    assert err <= bound, f"radial {got!r} vs exact {want!r}: off by {err / (U * S) if S else err:.1f} u*S, " \
                         f"bound {bound / (U * S) if S else 0:.0f} (centre {centre}, pov {pov}, {w}x{h})"
    return (err / (U * S), bound / (U * S)) if S else (0.0, 0.0)


def mean_mag_accepted(flow):
    """the float32 values the kernel's mean magnitude may take: float32 of the exact mean, or both neighbours when the
    exact mean lies within sum_bound * mean of a float32 rounding boundary"""
    h, w, _ = flow.shape
    mean, _ = mag_exact(flow)
    if not math.isfinite(mean):
        return mean, (np.float32(mean),)
    b = sum_bound(0, pass1_depth(w, h)) * mean
    return mean, tuple({np.float32(mean - b), np.float32(mean + b)})


def check_mean_mag(got, flow):
    mean, ok = mean_mag_accepted(flow)
    if math.isnan(mean):
        assert math.isnan(float(got)), (got, mean)
    else:
        assert np.float32(got) in ok, f"mean_mag {float(got)!r} not in {[float(v) for v in ok]} (exact {mean!r})"
    return mean
