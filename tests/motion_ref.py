"""Restatement of the global-motion rules C1-C9 (include/ffl.h), importable without a GPU:
plain numpy for the per-pixel terms, post_ref.fsum for their exact sums, Python floats for the solve.

  C1  xc = x - (w - 1) / 2.0, yc = y - (h - 1) / 2.0.
  C2  mu = (a0 + a1 * xc) + a2 * yc, mv = (b0 + b1 * xc) + b2 * yc.
  C3  wt = float64(W) or 1; excluded (np.where, never a product): W == 0, or u or v not finite.  With a prior p:
      rho = t2 / (t2 + (ru * ru + rv * rv)), ru = u - mu_p, rv = v - mv_p, t2 = float64(float32(tau)) ** 2; omega = wt * rho.
  C4  the twelve terms of MOTION_SUMS' order, each formed as written: omega, omega*xc, omega*yc, (omega*xc)*xc, (omega*xc)*yc,
      (omega*yc)*yc, omega*u, (omega*u)*xc, (omega*u)*yc and the three of v.
  C5, C6  solve(): the lines of appendix C in Python floats.  A Python float is an IEEE double and every line below is one
      operation per written operator, as the C body is under -ffp-contract=off; the one difference of the languages, a
      division by zero, goes through _div, which returns what IEEE does.
  C7  fit(): pass k + 1 takes pass k's six numbers as its prior.
  C8  subtract(): float32(float64(u) - mu).

Error bounds, from the code (kernels_post.hip), not from device output:

  sums   the fit's k_strip_sums forms every term with the operations written above, in float64 without contraction, and numpy's
         elementwise float64 operations are those operations (the division of C3 is one correctly rounded IEEE division on
         both sides): the restated terms ARE the kernel's, bit for bit -- 0 roundings per term.  What differs is the order of
         the additions.  The walk is pass 2's (P2_STRIP = 128 columns per wave, two pixels per lane, a row group of 16 rows,
         wave shuffle, four waves through LDS, then k_motion_solve adds the workgroup partials in k_radial_final's tree), so
         the longest chain of additions a term passes through is post_ref.radial_depth(w, h): 2 * 16 + 6 + 3 + trips + 6 + 3,
         and the 2 that function adds for radial's two divisions, which the fit does not have, only loosen the bound by 2 u.
         Excluded pixels add +0.0 here and +0.0 or -0.0 in the kernel (it selects their omega, u and v to +0.0 before it
         forms the terms): the same bits of a sum that started at +0.0.  Hence for each of the twelve sums
             |kernel - fsum(terms)| <= sum_bound(0, radial_depth(w, h)) * sum |term|.
  solve  an exactly affine field whose samples and weights are short dyadic numbers has twelve sums that are exact in any
         order (every term is an integer multiple of 2^-k far below 2^53 * 2^-k), so the only error of the six numbers is
         the LDL^T elimination's.  For a symmetric positive definite n x n system without pivoting the computed solution
         solves (M + dM) x = r with |dM| <= gamma(3n + 1) |L||D||L^T| (Higham, Accuracy and Stability of Numerical Algorithms,
         2nd ed., Theorem 10.4 and section 10.1 for the LDL^T form), and || |L||D||L^T| || <= n ||M||, so
         ||dM|| / ||M|| <= n * (3n + 1) u = 30 u for n = 3 (first order), the right-hand sides being exact.  The forward
         error is then at most cond(M) * 30 u * max|x|; affine_tolerance() returns cond_inf(M) * 64 u * max|x|, the factor
         of two above 30 covering the first-order terms dropped and the change of norm.  M is formed from the exact sums.
"""
import numpy as np

from post_ref import U, fsum, radial_depth, sum_bound
import weights_ref  # noqa: F401  (rule W1's map form is shared: weights_ref.weights_of)

MODELS = ("translation", "rigid", "similarity", "affine")
OK, EMPTY, DEGENERATE = 0, 1, 2
SUMS = ("S", "Sx", "Sy", "Sxx", "Sxy", "Syy", "Su", "Sux", "Suy", "Sv", "Svx", "Svy")
RECORD = np.dtype([(k, "<f8") for k in ("a0", "a1", "a2", "b0", "b1", "b2", "sw")] + [("model", "<i4"), ("status", "<i4")])
EPS = 1e-12


def coords(w, h):
    """rule C1: (xc[1, w], yc[h, 1]) float64, exact"""
    xc = np.arange(w, dtype=np.float64)[None, :] - (w - 1) / 2.0
    yc = np.arange(h, dtype=np.float64)[:, None] - (h - 1) / 2.0
    return xc, yc


def model_flow(m, w, h):
    """rule C2: (mu, mv) float64 (h, w) of the six numbers m"""
    xc, yc = coords(w, h)
    a0, a1, a2, b0, b1, b2 = (np.float64(v) for v in m)
    with np.errstate(all="ignore"):
        return (a0 + a1 * xc) + a2 * yc, (b0 + b1 * xc) + b2 * yc


def omega(flow, W=None, prior=None, tau=1.0):
    """rule C3: (omega float64 (h, w), included bool (h, w)); omega of an excluded pixel is whatever IEEE gives and is never used"""
    flow = np.asarray(flow, np.float32)
    h, w, _ = flow.shape
    u, v = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
    inc = np.isfinite(flow[..., 0]) & np.isfinite(flow[..., 1])
    wt = np.ones((h, w))
    if W is not None:
        wt = weights_ref.weights_of(W)
        inc &= wt > 0
    if prior is None:
        return wt, inc
    mu, mv = model_flow(prior, w, h)
    t2 = np.float64(np.float32(tau)) * np.float64(np.float32(tau))
    with np.errstate(all="ignore"):
        ru, rv = u - mu, v - mv
        r2 = ru * ru + rv * rv
        rho = t2 / (t2 + r2)
        return wt * rho, inc


def terms(flow, W=None, prior=None, tau=1.0):
    """rule C4: the twelve (h, w) float64 term arrays, +0.0 where the pixel is excluded"""
    flow = np.asarray(flow, np.float32)
    h, w, _ = flow.shape
    xc, yc = coords(w, h)
    u, v = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
    om, inc = omega(flow, W, prior, tau)
    with np.errstate(all="ignore"):
        ox, oy, ou, ov = om * xc, om * yc, om * u, om * v
        t = [om, ox, oy, ox * xc, ox * yc, oy * yc, ou, ou * xc, ou * yc, ov, ov * xc, ov * yc]
    return [np.where(inc, a, 0.0) for a in t]


def sums_exact(flow, W=None, prior=None, tau=1.0):
    """[(exactly rounded sum, sum |term|)] * 12"""
    return [(fsum(t), float(np.sum(np.abs(t)))) for t in terms(flow, W, prior, tau)]


def _div(a, b):
    """a / b as IEEE has it (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def solve(s, model):
    """rules C5 and C6 on twelve sums: a RECORD (numpy, shape ()); the lines of DESIGN.md appendix C in their order"""
    model = MODELS.index(model) if isinstance(model, str) else int(model)
    S, Sx, Sy, Sxx, Sxy, Syy, Su, Sux, Suy, Sv, Svx, Svy = (float(v) for v in s)
    a0 = a1 = a2 = b0 = b1 = b2 = 0.0
    status = EMPTY
    if not S == 0.0:
        ta, tb = _div(Su, S), _div(Sv, S)
        a0, b0, status = ta, tb, OK
        if model in (1, 2):
            Q = Sxx + Syy
            q, p = _div(Sx, S), _div(Sy, S)
            D = (Q - q * Sx) - p * Sy
            if not (S > EPS * S) or not (D > EPS * Q):
                status = DEGENERATE
            else:
                g3 = Svx - Suy
                z3 = (g3 + p * Su) - q * Sv
                rot = _div(z3, D)
                sc = 0.0
                if model == 2:
                    g2 = Sux + Svy
                    z2 = (g2 - q * Su) - p * Sv
                    sc = _div(z2, D)
                a0 = (ta - q * sc) + p * rot
                b0 = (tb - p * sc) - q * rot
                a1, a2, b1, b2 = sc, -rot, rot, sc
        elif model == 3:
            ok = S > EPS * S
            l10 = l20 = l21 = d1 = d2 = 0.0
            if ok:
                l10 = _div(Sx, S)
                l20 = _div(Sy, S)
                d1 = Sxx - l10 * Sx
                ok = d1 > EPS * Sxx
            if ok:
                m21 = Sxy - l20 * Sx
                l21 = _div(m21, d1)
                d2 = (Syy - l20 * Sy) - l21 * m21
                ok = d2 > EPS * Syy
            if not ok:
                status = DEGENERATE
            else:
                za1 = Sux - l10 * Su
                za2 = (Suy - l20 * Su) - l21 * za1
                zb1 = Svx - l10 * Sv
                zb2 = (Svy - l20 * Sv) - l21 * zb1
                a2 = _div(za2, d2)
                a1 = _div(za1, d1) - l21 * a2
                a0 = (ta - l10 * a1) - l20 * a2
                b2 = _div(zb2, d2)
                b1 = _div(zb1, d1) - l21 * b2
                b0 = (tb - l10 * b1) - l20 * b2
    r = np.zeros((), RECORD)
    r["a0"], r["a1"], r["a2"], r["b0"], r["b1"], r["b2"], r["sw"], r["model"], r["status"] = a0, a1, a2, b0, b1, b2, S, model, status
    return r


def six(rec):
    return [float(rec[k]) for k in ("a0", "a1", "a2", "b0", "b1", "b2")]


def fit(flow, model="translation", iterations=3, tau=1.0, W=None, prior=None):
    """rule C7 over the exact sums: the RECORD of every pass, in order"""
    out = []
    for _ in range(iterations):
        rec = solve([s for s, _ in sums_exact(flow, W, prior, tau)], model)
        out.append(rec)
        prior = six(rec)
    return out


def subtract(flow, m):
    """rule C8: float32 (h, w, 2)"""
    flow = np.asarray(flow, np.float32)
    h, w, _ = flow.shape
    mu, mv = model_flow(m, w, h)
    with np.errstate(all="ignore"):
        return np.stack([(flow[..., 0].astype(np.float64) - mu).astype(np.float32),
                         (flow[..., 1].astype(np.float64) - mv).astype(np.float32)], axis=-1)


def sums_bound(w, h, abs_sum):
    return sum_bound(0, radial_depth(w, h)) * abs_sum


def check_sums(got, flow, W=None, prior=None, tau=1.0):
    """assert twelve kernel sums against the exact sums of the restated terms; returns the worst error in units of u * sum|term|"""
    h, w, _ = np.asarray(flow).shape
    worst = 0.0
    for name, g, (want, A) in zip(SUMS, got, sums_exact(flow, W, prior, tau)):
        g = float(g)
        assert np.isfinite(want), (name, want)   # excluded pixels reach no sum
        bound = sums_bound(w, h, A)
        err = abs(g - want)
        assert err <= bound, f"{name} {g!r} vs exact {want!r}: off by {err / (U * A) if A else err:.1f} u*A, " \
                             f"bound {bound / (U * A) if A else 0:.0f} ({w}x{h})"
        if A:
            worst = max(worst, err / (U * A))
    return worst


def affine_tolerance(s, x):
    """the forward-error bound of the module docstring for the AFFINE system over sums s and solution numbers x"""
    S, Sx, Sy, Sxx, Sxy, Syy = (float(v) for v in s[:6])
    M = np.array([[S, Sx, Sy], [Sx, Sxx, Sxy], [Sy, Sxy, Syy]])
    return float(np.linalg.cond(M, np.inf)) * 64 * U * max(abs(float(v)) for v in x)
