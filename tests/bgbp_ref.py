"""Checker for bgtest / bptest (helper module, not collected): the two functions of
S/stats/TimeSeriesStatisticalTests.scala (:266-278, :311-319) restated in float64 numpy the way
commons-math3 3.4.1 OLSMultipleLinearRegression (with intercept) computes them -- Householder QR
with a leading column of ones (stattests_ref.ols_householder), RSS as a sequential dot product, TSS
by SecondMoment's update loop, R^2 = 1 - RSS / TSS -- the same formulas in 60-digit mpmath (for
tools/gen_bgbp_golden.py and the CPU tests only), and the test inputs.

Factors are (T, k) throughout, the reference's DenseMatrix orientation.
"""
import math

import numpy as np

import stattests_ref as ref

MAX_FACTORS = 8           # STS_MAX_FACTORS
MAX_LAG = 31


def second_moment(y):
    """commons-math3 SecondMoment.evaluate: FirstMoment / SecondMoment.increment per value."""
    m1 = m2 = 0.0
    for i, v in enumerate(np.asarray(y, dtype=np.float64).tolist()):
        d = v - m1
        nd = d / (i + 1.0)
        m1 += nd
        m2 += float(i) * d * nd
    return m2


def r_squared(y, X):
    """calculateRSquared() of newSampleData(y, X) with intercept."""
    y = np.asarray(y, dtype=np.float64)
    Xi = np.column_stack([np.ones(y.size), np.asarray(X, dtype=np.float64)])
    _, _, res = ref.ols_householder(y, Xi)
    return 1.0 - ref._seq(res * res) / second_moment(y)


def bg_design(e, F, max_lag):
    """response e[maxLag..T), columns: the factors' rows maxLag..T, then e[t-1] .. e[t-maxLag]"""
    e = np.asarray(e, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    n = e.size - max_lag
    lags = [e[max_lag - j:max_lag - j + n] for j in range(1, max_lag + 1)]
    return e[max_lag:], np.column_stack([F[max_lag:]] + lags)


def bp_stat(e, F):
    e = np.asarray(e, dtype=np.float64)
    return e.size * r_squared(e * e, F)


def bg_stat(e, F, max_lag):
    y, X = bg_design(e, F, max_lag)
    return y.size * r_squared(y, X)


def bp_min_T(k):
    return k + 2                     # T > 1 + k


def bg_min_T(k, max_lag):
    return 2 * max_lag + k + 2       # nObs = T - maxLag > 1 + k + maxLag


# ---- the same formulas in mpmath ----

def _exact_r2(mp, y, cols):
    n = len(y)
    cols = [[mp.mpf(1)] * n] + cols
    _, beta = ref._mp_solve_ols(mp, y, cols)
    rss = mp.mpf(0)
    for r in range(n):
        rss += (y[r] - mp.fsum(c[r] * beta[i] for i, c in enumerate(cols))) ** 2
    mean = mp.fsum(y) / n
    tss = mp.fsum((v - mean) ** 2 for v in y)
    return 1 - rss / tss


def exact_bp(e, F, dps=60):
    import mpmath as mp
    with mp.workdps(dps):
        ee = [mp.mpf(float(v)) for v in e]
        F = np.asarray(F, dtype=np.float64)
        cols = [[mp.mpf(float(v)) for v in F[:, j]] for j in range(F.shape[1])]
        return float(len(ee) * _exact_r2(mp, [v * v for v in ee], cols))


def exact_bg(e, F, max_lag, dps=60):
    import mpmath as mp
    with mp.workdps(dps):
        ee = [mp.mpf(float(v)) for v in e]
        F = np.asarray(F, dtype=np.float64)
        n = len(ee) - max_lag
        cols = [[mp.mpf(float(v)) for v in F[max_lag:, j]] for j in range(F.shape[1])]
        cols += [ee[max_lag - j:max_lag - j + n] for j in range(1, max_lag + 1)]
        return float(n * _exact_r2(mp, ee[max_lag:], cols))


# ---- inputs ----

def factors(seed, T, k, S=None):
    """Standard normal factors with factor 0 the alternating +-1 of the reference's suite; (T, k), or
    (S, T, k) with every series its own draw."""
    rng = np.random.RandomState(seed)
    F = rng.standard_normal((T, k) if S is None else (S, T, k))
    F[..., 0] = (-1.0) ** np.arange(T)
    return F


def bg_resid(seed, S, T):
    """AR(1) residuals, coefficient 0.5: R^2 of the auxiliary regression around 0.25"""
    rng = np.random.RandomState(seed)
    u = rng.standard_normal((S, T))
    e = np.empty((S, T))
    prev = np.zeros(S)
    for t in range(T):
        prev = 0.5 * prev + u[:, t]
        e[:, t] = prev
    return e


def bp_resid(seed, S, T, F):
    """Residuals whose scale follows factor 0 (F: (T, k) or (S, T, k))"""
    rng = np.random.RandomState(seed)
    u = rng.standard_normal((S, T))
    return u * (1.0 + 1.5 * (np.asarray(F)[..., 0] > 0))


def white(seed, S, T):
    return np.random.RandomState(seed).standard_normal((S, T))


# hard rows: (name, T); k = 3, maxLag = 5.  "white_noise" is hard in another way: R^2 is of the order
# of maxLag / T, where every form of R^2 loses relative accuracy.
HARD_K, HARD_LAG, HARD_SEED = 3, 5, 20161
HARD_ROWS = [(name, T) for T in (390, 2520)
             for name in ("resid_level_1e4", "factor_level_1e6", "collinear_1e-6", "trend_factor", "white_noise")]


def hard_row(i):
    """-> (e (T,), F (T, 3))"""
    name, T = HARD_ROWS[i]
    rng = np.random.RandomState(HARD_SEED + i)
    F = rng.standard_normal((T, HARD_K))
    e = bg_resid(HARD_SEED + 100 + i, 1, T)[0]
    t = np.arange(T, dtype=np.float64)
    if name == "resid_level_1e4":
        e = e + 1e4
    elif name == "factor_level_1e6":
        F = F + 1e6
    elif name == "collinear_1e-6":
        F[:, 2] = F[:, 0] + 1e-6 * F[:, 2]
    elif name == "white_noise":
        e = white(HARD_SEED + 200 + i, 1, T)[0]
    else:
        F[:, 2] = t + 1e-2 * F[:, 2]
        e = e + 1e-3 * t
    return e, F


# ---- the reference suite's two scenarios (TimeSeriesStatisticalTestsSuite.scala:26-85) ----

def _first_stage_residuals(y, X):
    Xi = np.column_stack([np.ones(y.size), X])
    return ref.ols_householder(y, Xi)[2]


def suite_bg():
    """-> (factors (100, 1), residuals of the stationary series, residuals of the AR(1) series)"""
    from mt19937 import MersenneTwister
    rand = MersenneTwister(5)
    n, coef = 100, 0.5
    x = np.array([1.0, -1.0] * (n // 2))
    y1 = np.array([v + 1 + rand.next_gaussian() for v in x])
    y2 = np.empty(n)                      # scanLeft(0.0)(prior * coef + curr).tail
    prior = 0.0
    for i in range(n):
        prior = prior * coef + y1[i]
        y2[i] = prior
    F = x.reshape(n, 1)
    return F, _first_stage_residuals(y1, F), _first_stage_residuals(y2, F)


def suite_bp():
    """-> (factors (100, 1), homoskedastic residuals, alternating-variance residuals)"""
    from mt19937 import MersenneTwister
    rand = MersenneTwister(5)
    n, var_factor = 100, 2
    x = np.array([-1.0, 1.0] * (n // 2))
    err1 = np.array([rand.next_gaussian() for _ in range(n)])
    err2 = np.array([v * var_factor if i % 2 == 0 else v for i, v in enumerate(err1)])
    y1 = np.array([xi + ei + 1 for xi, ei in zip(x, err1)])
    y2 = np.array([xi + ei + 1 for xi, ei in zip(x, err2)])
    F = x.reshape(n, 1)
    return F, _first_stage_residuals(y1, F), _first_stage_residuals(y2, F)


def chi2_sf(stat, dof):
    return ref.chi2_sf(stat, dof) if not math.isnan(stat) else float("nan")
