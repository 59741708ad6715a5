"""Checker for the statistical tests (helper module, not collected): the four functions of
S/stats/TimeSeriesStatisticalTests.scala restated in float64 numpy in the reference's loop order,
their p-value functions in pure Python, the test inputs, and (for tools/gen_stattests_golden.py
and the CPU tests only) the same formulas in 60-digit mpmath.

Sequential sums: the reference accumulates left to right; np.cumsum is strictly sequential, so
_seq(v) = cumsum(v)[-1] is that loop, vectorised.
"""
import math

import numpy as np

REGRESSIONS = ("nc", "c", "ct", "ctt")
TREND_COLS = {"nc": 0, "c": 1, "ct": 2, "ctt": 3}
ONE_WAVE = 2560           # sts::kStatOneWave: longer series take the workgroup kernels


def _seq(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.cumsum(v)[-1]) if v.size else 0.0


# ---- commons-math3 3.4.1 OLSMultipleLinearRegression, noIntercept (operation order as in
# oracle/sts_oracle.c:318-390 for beta; plus calculateBetaVariance / calculateErrorVariance) ----

class Singular(Exception):
    pass


def ols_householder(y, X):
    """-> (beta, R, residuals).  X: (n, k) float64."""
    y = np.asarray(y, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    n, k = X.shape
    if k > n:
        raise ValueError("NOT_ENOUGH_DATA_FOR_NUMBER_OF_PREDICTORS")
    qrt = np.ascontiguousarray(X.T).copy()          # qrt[col][row]
    rdiag = np.zeros(k)
    for minor in range(min(n, k)):
        qm = qrt[minor]
        x2 = _seq(qm[minor:] * qm[minor:])
        a = -math.sqrt(x2) if qm[minor] > 0 else math.sqrt(x2)
        rdiag[minor] = a
        if a != 0.0:
            qm[minor] -= a
            for col in range(minor + 1, k):
                qc = qrt[col]
                alpha = -_seq(qc[minor:] * qm[minor:])
                alpha /= a * qm[minor]
                qc[minor:] -= alpha * qm[minor:]
    if np.any(np.abs(rdiag) <= 0.0):
        raise Singular()
    yy = y.copy()
    for minor in range(min(n, k)):
        qm = qrt[minor]
        dot = _seq(yy[minor:] * qm[minor:])
        dot /= rdiag[minor] * qm[minor]
        yy[minor:] += dot * qm[minor:]
    beta = np.zeros(k)
    for row in range(k - 1, -1, -1):
        yy[row] /= rdiag[row]
        beta[row] = yy[row]
        yy[:row] -= yy[row] * qrt[row][:row]
    R = np.zeros((k, k))
    for i in range(k):
        R[i, i] = rdiag[i]
        for j in range(i + 1, k):
            R[i, j] = qrt[j][i]
    fit = np.zeros(n)
    for c in range(k):                               # X.operate(beta): per row, columns in order
        fit += X[:, c] * beta[c]
    return beta, R, y - fit


def _upper_inverse(R):
    """LUDecomposition(R).getSolver().getInverse() of an upper-triangular R (no pivoting happens:
    everything below the diagonal is zero): back substitution per unit column."""
    k = R.shape[0]
    inv = np.zeros((k, k))
    for c in range(k):
        for r in range(c, -1, -1):
            v = 1.0 if r == c else 0.0
            for j in range(r + 1, c + 1):
                v -= R[r, j] * inv[j, c]
            inv[r, c] = v / R[r, r]
    return inv


def adf_design(ts, max_lag, regression):
    ts = np.asarray(ts, dtype=np.float64)
    T = ts.size
    diff = ts[1:] - ts[:-1]
    n_obs = diff.size - max_lag
    cols = [ts[T - n_obs - 1:T - 1]]
    for c in range(1, max_lag + 1):                  # lagMatTrimBoth(diff, maxLag, true), columns 1..
        cols.append(diff[max_lag - c:max_lag - c + n_obs])
    r = np.arange(1, n_obs + 1, dtype=np.float64)
    q = TREND_COLS[regression]
    trend = [np.ones(n_obs)]
    for _ in range(1, 3):
        trend.append(r * trend[-1])                  # vanderflipped
    cols += trend[:q]
    return diff[diff.size - n_obs:], np.stack(cols, axis=1)


def adf_stat(ts, max_lag, regression="c"):
    y, X = adf_design(ts, max_lag, regression)
    n, k = X.shape
    beta, R, res = ols_householder(y, X)
    rinv = _upper_inverse(R)
    var00 = _seq(rinv[0] * rinv[0])                  # (Rinv Rinv^T)[0][0]
    sigma = _seq(res * res) / (n - k)
    return beta[0] / math.sqrt(sigma * var00)


def kpss_lag(n):
    return int(3 * math.sqrt(n) / 13)


def kpss_stat(ts, method):
    ts = np.asarray(ts, dtype=np.float64)
    n = ts.size
    cols = [np.ones(n)]
    if method == "ct":
        cols.append(1.0 + np.arange(n, dtype=np.float64))
    _, _, res = ols_householder(ts, np.stack(cols, axis=1))
    cs = np.cumsum(res)
    s2 = _seq(cs * cs)
    lag = kpss_lag(n)
    terms = 0.0
    for i in range(1, lag + 1):
        terms += _seq(res[i:] * res[:n - i]) * (1 - (float(i) / (lag + 1)))
    lrv = (terms * 2) / n + _seq(res * res) / n
    return (s2 / lrv) / (float(n) * float(n))


def dw_stat(res):
    res = np.asarray(res, dtype=np.float64)
    d = res[1:] - res[:-1]
    return _seq(d * d) / _seq(res * res)


def lb_stat(res, max_lag):
    import oracle
    res = np.asarray(res, dtype=np.float64)
    n = res.size
    ac = np.asarray(oracle.autocorr(res, max_lag), dtype=np.float64)
    adj = (ac * ac) / (n - np.arange(max_lag, dtype=np.float64) - 1)
    return float(n) * float(n + 2) * _seq(adj)


# ---- p-values, pure Python ----

# MacKinnon (1994), N = 1: tau*, tau_min, tau_max, small-p (c0, c1, c2), large-p (c0..c3)
MACKINNON = {
    "nc": (-1.04, -19.04, math.inf, (0.6344, 1.2378, 3.2496e-2), (0.4797, 9.3557e-1, -0.6999e-1, 3.3066e-2)),
    "c": (-1.61, -18.83, 2.74, (2.1659, 1.4412, 3.8269e-2), (1.7339, 9.3202e-1, -1.2745e-1, -1.0368e-2)),
    "ct": (-2.89, -16.18, 0.7, (3.2512, 1.6047, 4.9588e-2), (2.5261, 6.1654e-1, -3.7956e-1, -6.0285e-2)),
    "ctt": (-3.21, -17.17, 0.54, (4.0003, 1.658, 4.8288e-2), (3.0778, 4.9529e-1, -4.1477e-1, -5.9359e-2)),
}


def norm_cdf(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


def mackinnon_p(tau, regression):
    star, lo, hi, small, large = MACKINNON[regression]
    if tau != tau:
        return tau
    if tau > hi:
        return 1.0
    if tau < lo:
        return 0.0
    if tau <= star:
        z = (small[2] * tau + small[1]) * tau + small[0]
    else:
        z = ((large[3] * tau + large[2]) * tau + large[1]) * tau + large[0]
    return norm_cdf(z)


def gamma_p(a, x):
    """Regularised lower incomplete gamma: series below a + 1, continued fraction above."""
    if x != x:
        return x
    if x <= 0.0:
        return 0.0
    if math.isinf(x):
        return 1.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1.0:
        ap, term = a, 1.0 / a
        total = term
        for _ in range(100000):
            ap += 1.0
            term *= x / ap
            total += term
            if abs(term) < abs(total) * 1e-15:
                break
        return total * lead
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        if abs(d) < tiny:
            d = tiny
        c = b + an / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < 1e-15:
            break
    return 1.0 - lead * h


def chi2_sf(stat, dof):
    """1 - ChiSquaredDistribution(dof).cumulativeProbability(stat), formed as the reference does."""
    return 1.0 - gamma_p(0.5 * dof, 0.5 * stat)


# ---- inputs ----

def ordinary_panel(seed, S, T):
    """Even rows: stationary AR(1), phi in [0.3, 0.9]; odd rows: random walks.  Level of the order
    of the spread."""
    rng = np.random.RandomState(seed)
    e = rng.standard_normal((S, T))
    x = np.empty((S, T))
    for s in range(S):
        if s % 2 == 0:
            phi = 0.3 + 0.6 * ((s // 2) % 7) / 6.0
            v = np.empty(T)
            prev = 0.0
            for t in range(T):
                prev = phi * prev + e[s, t]
                v[t] = prev
            x[s] = 1.0 + v
        else:
            x[s] = 2.0 + np.cumsum(e[s])
    return x


def ar1_panel(seed, S, T):
    """Stationary AR(1) rows only, phi cycling over 0.3 .. 0.9 (the Ljung-Box rows)."""
    rng = np.random.RandomState(seed)
    e = rng.standard_normal((S, T))
    x = np.empty((S, T))
    for s in range(S):
        phi = 0.3 + 0.6 * (s % 7) / 6.0
        prev = 0.0
        for t in range(T):
            prev = phi * prev + e[s, t]
            x[s, t] = prev
    return x


HARD_ROWS = [(level, drift, noise, kind, T)
             for T in (390, 2520)
             for level in (1e4, 1e6)
             for drift in (0.0, 1.0, 10.0)
             for noise in (1e-2, 1e-1)
             for kind in ("walk", "stationary")]
HARD_SEED = 20151
# the statistics stored per hard row
HARD_STATS = [("adf", 1, "c"), ("adf", 5, "ct"), ("adf", 2, "ctt"), ("kpss", 0, "c"), ("kpss", 0, "ct")]


def hard_row(i):
    level, drift, noise, kind, T = HARD_ROWS[i]
    rng = np.random.RandomState(HARD_SEED + i)
    e = noise * rng.standard_normal(T)
    v = np.cumsum(e) if kind == "walk" else e
    return level + drift * np.arange(T, dtype=np.float64) + v


def ref_stat(kind, lag, reg, x):
    return adf_stat(x, lag, reg) if kind == "adf" else kpss_stat(x, reg)


# ---- the same formulas in mpmath (tools/gen_stattests_golden.py, tests/test_stattests_cpu.py) ----

def _mp_solve_ols(mp, y, cols):
    k = len(cols)
    G = mp.matrix(k, k)
    b = mp.matrix(k, 1)
    for i in range(k):
        for j in range(i, k):
            G[i, j] = G[j, i] = mp.fdot(cols[i], cols[j])
        b[i] = mp.fdot(cols[i], y)
    return G, mp.lu_solve(G, b)


def exact_adf(ts, max_lag, regression, dps=60):
    import mpmath as mp
    with mp.workdps(dps):
        y = [mp.mpf(float(v)) for v in ts]
        T = len(y)
        diff = [y[t + 1] - y[t] for t in range(T - 1)]
        n = len(diff) - max_lag
        cols = [y[T - n - 1:T - 1]]
        for c in range(1, max_lag + 1):
            cols.append(diff[max_lag - c:max_lag - c + n])
        for d in range(TREND_COLS[regression]):
            cols.append([mp.mpf(r) ** d for r in range(1, n + 1)])
        resp = diff[len(diff) - n:]
        G, beta = _mp_solve_ols(mp, resp, cols)
        k = len(cols)
        rss = mp.mpf(0)
        for r in range(n):
            rss += (resp[r] - mp.fsum(cols[c][r] * beta[c] for c in range(k))) ** 2
        e0 = mp.matrix(k, 1)
        e0[0] = 1
        inv00 = mp.lu_solve(G, e0)[0]
        return float(beta[0] / mp.sqrt(rss / (n - k) * inv00))


def exact_kpss(ts, method, dps=60):
    import mpmath as mp
    with mp.workdps(dps):
        y = [mp.mpf(float(v)) for v in ts]
        n = len(y)
        cols = [[mp.mpf(1)] * n]
        if method == "ct":
            cols.append([mp.mpf(t) for t in range(1, n + 1)])
        _, beta = _mp_solve_ols(mp, y, cols)
        res = [y[t] - mp.fsum(c[t] * beta[i] for i, c in enumerate(cols)) for t in range(n)]
        run, s2 = mp.mpf(0), mp.mpf(0)
        for v in res:
            run += v
            s2 += run * run
        lag = kpss_lag(n)
        terms = mp.mpf(0)
        for i in range(1, lag + 1):
            terms += mp.fdot(res[i:], res[:n - i]) * (1 - mp.mpf(i) / (lag + 1))
        lrv = terms * 2 / n + mp.fdot(res, res) / n
        return float(s2 / lrv / (mp.mpf(n) * n))


def exact_stat(kind, lag, reg, x):
    return exact_adf(x, lag, reg) if kind == "adf" else exact_kpss(x, reg)
