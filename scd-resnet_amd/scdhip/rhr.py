"""The end of the reference pipeline (test.py:148-183): the relative-halo-radius (Rhr) histogram of a cohort, its
two-Gaussian fit and the share of the first component.  numpy float64 on the host; no scipy.

The histogram itself is built on the device (ops.slide_samples): bin b = floor((Rhr - LO) * SCALE), 0 <= b < BINS.
"""
from collections import namedtuple

import numpy as np

BINS = 150
LO = -0.25
SCALE = 100.0
# test.py:177: [a1, m1, s1, a2, m2, s2]
LOWER = np.array([0.0, -0.25, 0.0, 0.0, 0.0, 0.0])
UPPER = np.array([1.0, 0.33, 0.2, 1.0, 1.25, 1.0])

Fit = namedtuple("Fit", "params sse iterations converged")


def xs():
    """test.py:174: the abscissae (i - 25) / 100, i.e. the left edges of the bins."""
    return np.array([(i - 25) / 100 for i in range(BINS)], np.float64)


def bin_index(r, lo=LO, scale=SCALE, nbins=BINS):
    """Bin of each Rhr value, the device's expression restated: floor((r - lo) * scale) in float64, or -1 where the
    value is not counted (not finite, or outside 0 <= b < nbins)."""
    r = np.asarray(r, np.float64)
    with np.errstate(all="ignore"):
        b = np.floor((r - lo) * scale)
        ok = np.isfinite(r) & (b >= 0) & (b < nbins)
    return np.where(ok, b, -1).astype(np.int64)


def frequencies(hist):
    """hist / hist.sum(): the `ys` of test.py:175-181."""
    h = np.asarray(hist, np.float64)
    total = h.sum()
    if h.size == 0 or not total > 0:
        raise ValueError("empty Rhr histogram: nothing to fit")
    return h / total


def gauss2(x, p):
    """test.py:14."""
    a1, m1, s1, a2, m2, s2 = p
    return a1 * np.exp(-((x - m1) / s1) ** 2) + a2 * np.exp(-((x - m2) / s2) ** 2)


def _residual_jac(x, y, p):
    a1, m1, s1, a2, m2, s2 = p
    z1, z2 = (x - m1) / s1, (x - m2) / s2
    e1, e2 = np.exp(-z1 * z1), np.exp(-z2 * z2)
    J = np.stack([e1, a1 * e1 * 2 * z1 / s1, a1 * e1 * 2 * z1 * z1 / s1,
                  e2, a2 * e2 * 2 * z2 / s2, a2 * e2 * 2 * z2 * z2 / s2], 1)
    return a1 * e1 + a2 * e2 - y, J


def _lm_interior(x, y, p, max_iter):
    """Levenberg-Marquardt on strictly interior iterates with the Coleman-Li scaling: with g the gradient, v_i is
    the distance to the bound that -g_i points at, the step solves (D J^T J D + diag(|g|) + mu I) q = -D g with
    D = diag(sqrt(v)) and is cut to stay 0.5 % (or less, near a stationary point) short of the bounds.  A clipped
    Gauss-Newton step cannot leave a1 = 0 or s1 = 0, where component 1's Jacobian columns vanish; this one never
    gets there."""
    r, J = _residual_jac(x, y, p)
    f = float(r @ r)
    mu = 1e-3
    for it in range(1, max_iter + 1):
        g = J.T @ r
        v = np.where(g < 0, UPPER - p, p - LOWER)
        gs = np.sqrt(v) * g
        gnorm = float(np.max(np.abs(v * g)))
        if gnorm <= 1e-17:
            return p, f, it, True
        d = np.sqrt(v)
        A = (J * d).T @ (J * d) + np.diag(np.abs(g))
        theta = max(0.995, 1.0 - gnorm)
        improved = False
        for _ in range(40):
            try:
                q = np.linalg.solve(A + mu * np.eye(6), -gs)
            except np.linalg.LinAlgError:
                mu *= 10.0
                continue
            step = d * q
            with np.errstate(all="ignore"):
                room = np.where(step > 0, (UPPER - p) / step, np.where(step < 0, (LOWER - p) / step, np.inf))
            hit = float(np.min(room))
            if hit <= 1.0:
                step = step * (theta * hit)
            pn = p + step
            rn, Jn = _residual_jac(x, y, pn)
            fn = float(rn @ rn)
            if np.isfinite(fn) and fn < f:
                improved = True
                break
            mu *= 4.0
            if mu > 1e20:
                break
        if not improved:
            return p, f, it, True         # no descent at any damping: a stationary point to rounding
        small = (f - fn) <= 1e-16 * f and float(np.max(np.abs(step))) <= 1e-12
        p, r, J, f = pn, rn, Jn, fn
        mu = max(mu / 8.0, 1e-15)
        if small:
            return p, f, it, True
    return p, f, max_iter, False


def _starts():
    """The reference start first (curve_fit without p0 starts at the midpoint of the bounds), then a fixed list:
    component 1 narrow and low, component 2 at a few places and widths."""
    mid = 0.5 * (LOWER + UPPER)
    out = [mid]
    for m1, s1 in ((0.0, 0.05), (0.12, 0.08), (0.25, 0.12)):
        for m2, s2 in ((0.35, 0.12), (0.6, 0.15), (0.9, 0.2)):
            out.append(np.array([0.05, m1, s1, 0.05, m2, s2]))
    return out


def fit_gauss2(ys, xs=None, max_iter=2000):
    """Bounded least squares of a1 exp(-((x-m1)/s1)^2) + a2 exp(-((x-m2)/s2)^2) to the frequencies `ys` over the
    reference's bounds (test.py:177).  Deterministic: the reference start, then a fixed list of further starts;
    the smallest residual sum of squares wins (an earlier start on ties).  Returns Fit(params (6,), sse,
    iterations (all starts), converged (the winning start))."""
    x = globals()["xs"]() if xs is None else np.asarray(xs, np.float64)
    y = np.asarray(ys, np.float64)
    if x.shape != y.shape or y.ndim != 1 or not np.all(np.isfinite(y)):
        raise ValueError("fit_gauss2: finite 1-d frequencies on matching abscissae expected")
    best, total = None, 0
    for p0 in _starts():
        p, f, it, ok = _lm_interior(x, y, p0.copy(), max_iter)
        total += it
        if best is None or f < best[1]:
            best = (p, f, ok)
    return Fit(best[0], float(np.sum((gauss2(x, best[0]) - y) ** 2)), total, best[2])


def dfi(params):
    """Share of component 1 by area, a1 s1 / (a1 s1 + a2 s2): the area of a exp(-((x-m)/s)^2) is a s sqrt(pi).
    This is the project's own definition of the DNA-fragmentation share: no definition from the paper was
    available when it was written, and whether the two agree has not been checked.  Reports print the six raw
    parameters beside it for that reason."""
    a1, _, s1, a2, _, s2 = [float(v) for v in params]
    den = a1 * s1 + a2 * s2
    if not den > 0:
        raise ValueError("dfi: both components have zero area")
    return a1 * s1 / den
