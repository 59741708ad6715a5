"""Checker for sts_factor_ols / sts_factor_remove / sts_factor_add (helper module, not collected):
commons-math3 3.4.1 OLSMultipleLinearRegression with intercept restated in float64 numpy from the
pieces of tests/stattests_ref.py (ols_householder, _upper_inverse, _seq) -- coefficients, standard
errors, residuals, RSS, TSS, R^2 and the error variance -- the same quantities in 60-digit mpmath
(for tools/gen_factor_ols_golden.py and the CPU tests only), the bit-exact restatement of the
effects pair, and the test inputs.

Factors are (T, k) or (S, T, k) throughout, the reference's DenseMatrix orientation.
"""
import functools
import math

import numpy as np

import bgbp_ref as br
import stattests_ref as ref

MAX_FACTORS = br.MAX_FACTORS
SINGULAR, BAD_ARG, NOT_ENOUGH_DATA = 8, 1, 7
BAR = 1e-10                         # the project's bar
KAPPA_BAR = 16 * 1e6 * 2.0 ** -53   # coefficients / standard errors of the collinear rows (kappa = 1e6)
COEF = np.array([0.7, -1.3, 0.4, 1.1, -0.6, 0.25, -0.9, 0.5])
INTERCEPT = 2.5


class Fit:
    """beta (k + 1,), se (k + 1,), resid (T,), rss, tss, r2, sigma2; beta_lo: what beta's rounding to
    float64 left (exact fits only)"""

    def __init__(self, beta, se, resid, rss, tss, r2, sigma2, beta_lo=None):
        self.beta, self.se, self.resid, self.beta_lo = beta, se, resid, beta_lo
        self.rss, self.tss, self.r2, self.sigma2 = rss, tss, r2, sigma2

    @property
    def stats(self):
        return np.array([self.rss, self.tss, self.r2, self.sigma2])


def ols(y, F):
    """newSampleData(y, F) with intercept: estimateRegressionParameters, ...StandardErrors,
    estimateResiduals, calculateResidualSumOfSquares, calculateTotalSumOfSquares, calculateRSquared,
    estimateErrorVariance."""
    y = np.asarray(y, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    n, k = F.shape
    Xi = np.column_stack([np.ones(n), F])
    beta, R, res = ref.ols_householder(y, Xi)
    rss = ref._seq(res * res)
    tss = br.second_moment(y)
    sigma2 = rss / (n - k - 1)
    rinv = ref._upper_inverse(R)
    se = np.array([math.sqrt(sigma2 * ref._seq(rinv[i] * rinv[i])) for i in range(k + 1)])
    with np.errstate(invalid="ignore", divide="ignore"):
        r2 = np.float64(1.0) - np.float64(rss) / np.float64(tss)
    return Fit(beta, se, res, rss, tss, float(r2), sigma2)


def exact(y, F, dps=60):
    """The same quantities from the normal equations in `dps`-digit arithmetic, rounded to float64."""
    import mpmath as mp
    y = np.asarray(y, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    n, k = F.shape
    with mp.workdps(dps):
        yy = [mp.mpf(float(v)) for v in y]
        cols = [[mp.mpf(1)] * n] + [[mp.mpf(float(v)) for v in F[:, j]] for j in range(k)]
        G, beta = ref._mp_solve_ols(mp, yy, cols)
        res = [yy[r] - mp.fsum(c[r] * beta[i] for i, c in enumerate(cols)) for r in range(n)]
        rss = mp.fsum(v * v for v in res)
        mean = mp.fsum(yy) / n
        tss = mp.fsum((v - mean) ** 2 for v in yy)
        sigma2 = rss / (n - k - 1)
        Gi = G ** -1
        se = [mp.sqrt(sigma2 * Gi[i, i]) for i in range(k + 1)]
        hi = np.array([float(b) for b in beta])
        lo = np.array([float(b - mp.mpf(float(b))) for b in beta])
        return Fit(hi, np.array([float(v) for v in se]), np.array([float(v) for v in res]), float(rss), float(tss),
                   float(1 - rss / tss), float(sigma2), beta_lo=lo)


def exact_resid(y, F, beta_hi, beta_lo):
    """The exact fit's residuals from its coefficients kept to 106 bits (hi + lo), in rational
    arithmetic, rounded to float64 once: what the fixture stores instead of T residuals per row.  The
    coefficients' own error, 2^-106 of a value at the series' level, is below 1e-20 of any residual here."""
    from fractions import Fraction
    b = [Fraction(float(h)) + Fraction(float(l)) for h, l in zip(beta_hi, beta_lo)]
    F = np.asarray(F, dtype=np.float64)
    out = np.empty(len(y))
    for t in range(len(y)):
        r = Fraction(float(y[t])) - b[0]
        for j in range(F.shape[1]):
            r -= Fraction(float(F[t, j])) * b[1 + j]
        out[t] = float(r)
    return out


def ols_panel(Y, F):
    """Fits of every row of Y (S, T) on F (T, k) or (S, T, k) -> (beta, se, stats, resid) arrays"""
    Y = np.asarray(Y, dtype=np.float64)
    fits = [ols(Y[s], F if np.ndim(F) == 2 else F[s]) for s in range(Y.shape[0])]
    return (np.stack([f.beta for f in fits]), np.stack([f.se for f in fits]), np.stack([f.stats for f in fits]),
            np.stack([f.resid for f in fits]))


# ---- the effects pair, bit for bit ----

def fit_values(beta, F):
    """((b0 + b1 f0[t]) + b2 f1[t]) + ..., left to right, every product and sum rounded (no FMA).
    beta (k + 1,) or (S, k + 1); F (T, k) or (S, T, k) -> (T,) or (S, T)"""
    beta = np.asarray(beta, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    k = F.shape[-1]
    b = beta[..., None, :] if beta.ndim == 2 else beta
    fit = b[..., 0] + np.zeros(F.shape[:-1])
    for j in range(k):
        fit = fit + b[..., 1 + j] * F[..., j]
    return fit


def remove(x, beta, F):
    return np.asarray(x, dtype=np.float64) - fit_values(beta, F)


def add(x, beta, F):
    return np.asarray(x, dtype=np.float64) + fit_values(beta, F)


# ---- inputs ----

def panel(seed, S, T, k, per_series=False):
    """-> (Y (S, T), F (T, k) or (S, T, k)): y = 2.5 + F . COEF[:k] + standard normal noise, factors of
    bgbp_ref.factors (factor 0 alternates +-1)."""
    F = br.factors(seed, T, k, S if per_series else None)
    e = np.random.RandomState(seed + 7919).standard_normal((S, T))
    return INTERCEPT + F @ COEF[:k] + e, F


# hard rows: bgbp_ref's ten (k = 3) with y = 2.5 + F . (0.7, -1.3, 0.4) + e, and a near-exact fit at
# level 1e4 (R^2 about 1 - 1e-8)
HARD_ROWS = list(br.HARD_ROWS) + [("near_exact_level_1e4", 390)]
HARD_K = br.HARD_K


@functools.lru_cache(maxsize=None)
def _hard_row(i):
    if i < len(br.HARD_ROWS):
        e, F = br.hard_row(i)
        return INTERCEPT + F @ COEF[:HARD_K] + e, F
    rng = np.random.RandomState(br.HARD_SEED + 300)
    F = rng.standard_normal((390, HARD_K))
    return 1e4 + F @ COEF[:HARD_K] + 1e-4 * rng.standard_normal(390), F


def hard_row(i):
    """-> (y (T,), F (T, 3))"""
    y, F = _hard_row(i)
    return y.copy(), F.copy()


def collinear(i):
    return HARD_ROWS[i][0].startswith("collinear")


# ---- comparisons: the largest relative error of a group, residuals over the rms of the reference's ----

def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    m = ~np.isnan(want)
    if not m.any():
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(got[m] - want[m]) / np.abs(want[m])
    e[(got[m] == want[m])] = 0.0
    return float(e.max())


def resid_err(got, want):
    """max |got - want| over the rms of want, per series; the largest"""
    got, want = np.atleast_2d(got), np.atleast_2d(want)
    assert got.shape == want.shape
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    rms = np.sqrt(np.mean(want * want, axis=1))
    d = np.max(np.abs(got - want), axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(d == 0.0, 0.0, d / rms)
    e = e[~np.isnan(e)]
    return float(e.max()) if e.size else 0.0
