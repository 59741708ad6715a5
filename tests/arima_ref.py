"""Checker for ARIMA (helper module, not collected): S/models/ARIMA.scala restated in float64
Python in the reference's statement order -- iterateARMA, the CSS likelihood (math.log as
oracle.fdlibm_log) and its gradient, the Hannan-Rissanen start (commons-math3's OLS as
stattests_ref.ols_householder), remove / add / forecast, inverseDifferencesOfOrderD, and a
straight-line restatement of commons-math3 3.4.1's NonLinearConjugateGradientOptimizer as
fitWithCSSCGD configures it.  Python floats are IEEE binary64 and nothing here contracts, so
these are the reference's bits wherever its operation order is pinned (see the parity notes
in include/sts.h for the two places where it is not).
"""
import math

import numpy as np

import oracle
from stattests_ref import Singular, ols_householder

OK, BAD_ARG, TOO_MANY_EVALUATIONS, TOO_MANY_ITERATIONS = 0, 1, 10, 11
NOT_ENOUGH_DATA, SINGULAR = 7, 8


def n_coef(p, q, icpt):
    return int(bool(icpt)) + p + q


def update_ma_errors(errs, new_error):
    """:390-400 -- the copy runs over ASCENDING i."""
    n = len(errs)
    for i in range(n - 1):
        errs[i + 1] = errs[i]
    if n > 0:
        errs[0] = new_error


def iterate_arma(p, q, coef, icpt, ts, dest, sign, gold=None, errors=None, init_ma=None):
    """:426-463; op is `+` (sign = 1) or `-` (sign = -1).  dest is modified and returned."""
    ma = [0.0] * q if init_ma is None else init_ma
    intercept = 1 if icpt else 0
    n = len(ts)
    i = max(p, q)
    while i < n:
        v = dest[i]
        t = intercept * coef[0]
        v = v + t if sign > 0 else v - t
        j = 0
        while j < p and i - j - 1 >= 0:
            t = ts[i - j - 1] * coef[intercept + j]
            v = v + t if sign > 0 else v - t
            j += 1
        for j in range(q):
            t = ma[j] * coef[intercept + p + j]
            v = v + t if sign > 0 else v - t
        dest[i] = v
        error = errors[i] if gold is None else gold[i] - dest[i]
        update_ma_errors(ma, error)
        i += 1
    return dest


def loglik_css_arma(p, q, coef, icpt, y):
    """:278-293 on an already differenced series."""
    y = [float(v) for v in y]
    coef = [float(v) for v in coef]
    n = len(y)
    yhat = iterate_arma(p, q, coef, icpt, y, [0.0] * n, 1, gold=y)
    css = 0.0
    for i in range(max(p, q), n):
        e = y[i] - yhat[i]
        css += e * e
    sigma2 = css / n if n else float("nan")
    half = -(n // 2)                                    # (-n / 2): Int division truncates
    arg = 2 * math.pi * sigma2
    try:
        tail = css / (2 * sigma2)
    except ZeroDivisionError:
        tail = float("nan") if css == 0.0 or css != css else math.copysign(float("inf"), css)
    return half * oracle.fdlibm_log(arg) - tail


def gradient_css_arma(p, q, coef, icpt, y):
    """:312-381."""
    y = [float(v) for v in y]
    coef = [float(v) for v in coef]
    n = len(y)
    nc = len(coef)
    intercept = 1 if icpt else 0
    max_lag = max(p, q)
    ma = [0.0] * q
    d = [[0.0] * nc for _ in range(q + 1)]
    grad = [0.0] * nc
    sigma2 = 0.0
    for i in range(max_lag, n):
        for j in range(nc):
            for k in range(q):
                d[0][j] -= coef[intercept + p + k] * d[k + 1][j]
        yhat = 0.0
        yhat += intercept * coef[0]
        d[0][0] -= intercept
        j = 0
        while j < p and i - j - 1 >= 0:
            yhat += y[i - j - 1] * coef[intercept + j]
            d[0][intercept + j] -= y[i - j - 1]
            j += 1
        for j in range(q):
            yhat += ma[j] * coef[intercept + p + j]
            d[0][intercept + p + j] -= ma[j]
        error = y[i] - yhat
        sigma2 += error * error / n
        update_ma_errors(ma, error)
        for j in range(nc):
            grad[j] += d[0][j] * error
        d = [[0.0] * nc] + d[:-1]                       # rows move back by one, row 0 reset
    out = []
    for gj in grad:
        try:
            out.append(gj / -sigma2)
        except ZeroDivisionError:
            out.append(float("nan") if gj == 0.0 or gj != gj else math.copysign(float("inf"), -gj))
    return np.array(out)


def diffed(ts, d):
    """differencesOfOrderD(ts, d).drop(d)"""
    ts = np.asarray(ts, dtype=np.float64)
    return oracle.differences_of_order_d(ts, d)[d:] if d > 0 else ts.copy()


def loglik_css(p, d, q, coef, icpt, ts):
    return loglik_css_arma(p, q, coef, icpt, diffed(ts, d))


def gradient_css(p, d, q, coef, icpt, ts):
    return gradient_css_arma(p, q, coef, icpt, diffed(ts, d))


def lag_mat_trim_both(x, max_lag):
    """Lag.lagMatTrimBoth(x, maxLag, includeOriginal = false): row r = x[maxLag + r - 1 - j], j < maxLag"""
    x = np.asarray(x, dtype=np.float64)
    rows = max(len(x) - max_lag, 0)
    out = np.zeros((rows, max_lag))
    for j in range(max_lag):
        out[:, j] = x[max_lag - 1 - j: max_lag - 1 - j + rows]
    return out


def hr_design(p, q, y, icpt):
    """:212-230 -> (response, design with the intercept column first when icpt)."""
    y = np.asarray(y, dtype=np.float64)
    m = max(p, q) + 1
    c, phi = oracle.ar_fit(y, m)
    y_trunc = y[m:]
    est = np.zeros(len(y_trunc))
    for r in range(len(y_trunc)):
        s = 0.0                                          # .sum of the products, then + c
        for j in range(m):
            s += y[m + r - 1 - j] * phi[j]
        est[r] = s + c
    errors = y_trunc - est
    ar_terms = lag_mat_trim_both(y_trunc, p)[max(q - p, 0):]
    err_terms = lag_mat_trim_both(errors, q)[max(p - q, 0):]
    rows = min(len(ar_terms), len(err_terms))
    X = np.hstack([ar_terms[:rows], err_terms[:rows]])
    resp = y_trunc[m - 1:]
    if icpt:
        X = np.hstack([np.ones((rows, 1)), X])
    return resp, X


def hannan_rissanen(p, q, y, icpt):
    resp, X = hr_design(p, q, y, icpt)
    if len(resp) != X.shape[0]:
        raise ValueError("dimension mismatch %d != %d" % (len(resp), X.shape[0]))
    beta, _, _ = ols_householder(resp, X)
    return beta


def scaled_condition(X):
    """condition number of the design with every column scaled to unit length"""
    Xs = X / np.sqrt((X * X).sum(axis=0))
    s = np.linalg.svd(Xs, compute_uv=False)
    return s[0] / s[-1]


def inverse_differences_of_order_d(v, d):
    a = [float(x) for x in v]
    for i in range(d, 0, -1):
        for t in range(i, len(a)):
            a[t] = a[t] + a[t - 1]
    return np.array(a)


def remove_effects(p, d, q, coef, icpt, ts):
    """:474-487"""
    coef = [float(v) for v in coef]
    diff = oracle.differences_of_order_d(np.asarray(ts, dtype=np.float64), d) if d > 0 else np.asarray(ts, float)
    max_lag = max(p, q)
    amt = coef[0] if icpt else 0.0
    ext = [amt] * max_lag + [float(v) for v in diff]
    changes = list(ext)
    iterate_arma(p, q, coef, icpt, ext, changes, -1, errors=changes)
    return np.array(changes[max_lag:])


def add_effects(p, d, q, coef, icpt, ts):
    """:498-510"""
    coef = [float(v) for v in coef]
    max_lag = max(p, q)
    amt = coef[0] if icpt else 0.0
    changes = [amt] * max_lag + [float(v) for v in ts]
    provided = list(changes)
    iterate_arma(p, q, coef, icpt, changes, changes, 1, errors=provided)
    return inverse_differences_of_order_d(changes[max_lag:], d)


def forecast(p, d, q, coef, icpt, ts, n_future):
    """:537-605; sum(diffMatrix(0 until d, i - 1)) is taken in increasing difference order."""
    coef = [float(v) for v in coef]
    ts = [float(v) for v in ts]
    T = len(ts)
    max_lag = max(p, q)
    dts = [float(v) for v in diffed(ts, d)]
    amt = coef[0] if icpt else 0.0
    ext = [amt] * max_lag + dts
    hist_len = len(ext)
    hist = iterate_arma(p, q, coef, icpt, ext, [0.0] * hist_len, 1, gold=ext)
    ma = [ext[i] - hist[i] for i in range(hist_len - max_lag, hist_len)]
    forward = [0.0] * (n_future + max_lag)
    if max_lag:
        forward[:max_lag] = hist[-max_lag:]
    iterate_arma(p, q, coef, icpt, forward, forward, 1, gold=forward, init_ma=ma)
    res = [0.0] * (T + n_future)
    res[:d] = ts[:d]
    res[d:d + hist_len - max_lag] = hist[max_lag:]
    res[T:] = forward[max_lag:]
    if d != 0:
        dm = [[0.0] * T for _ in range(d + 1)]
        dm[0] = list(ts)
        for i in range(1, d + 1):
            prev = dm[i - 1]
            dm[i][i] = prev[i]
            for t in range(i + 1, T):
                dm[i][t] = prev[t] - prev[t - 1]
        for i in range(d, hist_len - max_lag):
            s = 0.0
            for k in range(d):
                s += dm[k][i - 1]
            res[i] = s + hist[max_lag + i]
        prev_terms = [dm[k][T - d + k] for k in range(d)]
        integ = inverse_differences_of_order_d(prev_terms + forward[max_lag:], d)
        res[T - d:] = list(integ)
    return np.array(res)


# ---- commons-math3 3.4.1: NonLinearConjugateGradientOptimizer(FLETCHER_REEVES,
# SimpleValueChecker(1e-7, 1e-7)), GoalType.MAXIMIZE, MaxIter / MaxEval 10000; LineSearch(1e-8,
# 1e-8, 1e-8) = BracketFinder(100, 500) + BrentOptimizer(1e-15, MIN_VALUE,
# SimpleUnivariateValueChecker(1e-8, 1e-8)) ----

class _Stop(Exception):
    def __init__(self, status):
        self.status = status


def _converged(p, c, rel, abs_):
    diff = abs(p - c)
    size = max(abs(p), abs(c)) if not (p != p or c != c) else float("nan")
    return diff <= size * rel or diff <= abs_


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _precision_equals(x, y):
    """Precision.equals(x, y, 1)"""
    if x != x or y != y:
        return False
    xi, yi = _bits(x), _bits(y)
    if (xi ^ yi) >= 0:
        return abs(xi - yi) <= 1
    sgn = -(1 << 63)
    if xi < yi:
        dp, dm = yi - 0, xi - sgn
    else:
        dp, dm = xi - 0, yi - sgn
    return False if dp > 1 else dm <= 1 - dp


def _best_max(a, b):
    return a if a[1] >= b[1] else b


class CEval:
    """loglik / gradient of one series through tests/native/arima_ref_eval.cpp (a ctypes handle
    of its shared library): the same straight-line restatement at C speed."""

    def __init__(self, lib, p, q, icpt, y):
        import ctypes
        self.lib, self.p, self.q, self.icpt = lib, p, q, int(bool(icpt))
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        self.n = self.p + self.q + self.icpt
        self._dp = ctypes.POINTER(ctypes.c_double)
        lib.aref_loglik.restype = ctypes.c_double
        lib.aref_loglik.argtypes = [ctypes.c_int] * 3 + [self._dp, self._dp, ctypes.c_int]
        lib.aref_gradient.restype = None
        lib.aref_gradient.argtypes = [ctypes.c_int] * 3 + [self._dp, self._dp, ctypes.c_int, self._dp]

    def loglik(self, x):
        c = np.ascontiguousarray(x, dtype=np.float64)
        return self.lib.aref_loglik(self.p, self.q, self.icpt, c.ctypes.data_as(self._dp),
                                    self.y.ctypes.data_as(self._dp), self.y.size)

    def gradient(self, x):
        c = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros(self.n)
        self.lib.aref_gradient(self.p, self.q, self.icpt, c.ctypes.data_as(self._dp),
                               self.y.ctypes.data_as(self._dp), self.y.size, out.ctypes.data_as(self._dp))
        return out


def fit_css_cgd(p, q, icpt, y, init, ev=None):
    """fitWithCSSCGD (:166-192) -> (status, point, evaluations).  ev: a CEval of the same series
    (the evaluations then run in C; the optimizer is this function either way)."""
    y = [float(v) for v in y]
    n = len(init)
    point = [float(v) for v in init]
    evals = [0]

    def objective(x):
        evals[0] += 1
        if evals[0] > 10000:
            raise _Stop(TOO_MANY_EVALUATIONS)
        return ev.loglik(x) if ev is not None else loglik_css_arma(p, q, x, icpt, y)

    def gradient(x):
        return [float(v) for v in (ev.gradient(x) if ev is not None else gradient_css_arma(p, q, x, icpt, y))]

    GOLD, EPS_MIN = 1.618034, 1e-21

    def line_search(start, direction):
        def f(t):
            return objective([start[i] + t * direction[i] for i in range(n)])
        bev = [0]

        def fb(t):
            bev[0] += 1
            if bev[0] > 500:
                raise _Stop(TOO_MANY_EVALUATIONS)
            return f(t)
        # BracketFinder.search(f, MAXIMIZE, 0, 1e-8)
        xA, xB = 0.0, 1e-8
        fA = fb(xA)
        fB = fb(xB)
        if fA > fB:
            xA, xB = xB, xA
            fA, fB = fB, fA
        xC = xB + GOLD * (xB - xA)
        fC = fb(xC)
        while fC > fB:
            tmp1 = (xB - xA) * (fB - fC)
            tmp2 = (xB - xC) * (fB - fA)
            val = tmp2 - tmp1
            denom = 2 * EPS_MIN if abs(val) < EPS_MIN else val     # as csrc/sts_garch_opt.hpp restates it
            w = xB - ((xB - xC) * tmp2 - (xB - xA) * tmp1) / (2 * denom)
            wLim = xB + 100 * (xC - xB)
            if (w - xC) * (xB - w) > 0:
                fW = fb(w)
                if fW > fC:
                    xA, xB, fA, fB = xB, w, fB, fW
                    break
                elif fW < fB:
                    xC, fC = w, fW
                    break
                w = xC + GOLD * (xC - xB)
                fW = fb(w)
            elif (w - wLim) * (wLim - xC) >= 0:
                w = wLim
                fW = fb(w)
            elif (w - wLim) * (xC - w) > 0:
                fW = fb(w)
                if fW > fC:
                    xB, xC = xC, w
                    w = xC + GOLD * (xC - xB)
                    fB, fC = fC, fW
                    fW = fb(w)
            else:
                w = xC + GOLD * (xC - xB)
                fW = fb(w)
            xA, fA = xB, fB
            xB, fB = xC, fC
            xC, fC = w, fW
        if xA > xC:
            xA, xC = xC, xA
        if not (xA < xC) or not (xA <= xB <= xC):
            raise _Stop(BAD_ARG)
        # BrentOptimizer.doOptimize, isMinim = false
        REL, ABS = 1e-15, 4.9406564584124654e-324
        GOLDEN = 0.5 * (3 - math.sqrt(5.0))
        a, b, x = xA, xC, xB
        v = w = x
        d = e = 0.0
        fx = -f(x)
        fv = fw = fx
        previous = None
        current = (x, -fx)
        best = current
        while True:
            m = 0.5 * (a + b)
            tol1 = REL * abs(x) + ABS
            tol2 = 2 * tol1
            if abs(x - m) <= tol2 - 0.5 * (b - a):
                prev = current if previous is None else _best_max(previous, current)
                return _best_max(best, prev)[0]
            if abs(e) > tol1:
                r = (x - w) * (fv - fx)
                qq = (x - v) * (fw - fx)
                pp = (x - v) * qq - (x - w) * r
                qq = 2 * (qq - r)
                if qq > 0:
                    pp = -pp
                else:
                    qq = -qq
                r = e
                e = d
                if pp > qq * (a - x) and pp < qq * (b - x) and abs(pp) < abs(0.5 * qq * r):
                    d = pp / qq
                    u = x + d
                    if u - a < tol2 or b - u < tol2:
                        d = tol1 if x <= m else -tol1
                else:
                    e = b - x if x < m else a - x
                    d = GOLDEN * e
            else:
                e = b - x if x < m else a - x
                d = GOLDEN * e
            if abs(d) < tol1:
                u = x + tol1 if d >= 0 else x - tol1
            else:
                u = x + d
            fu = -f(u)
            previous = current
            current = (u, -fu)
            best = _best_max(best, _best_max(previous, current))
            if _converged(previous[1], current[1], 1e-8, 1e-8):
                return best[0]
            if fu <= fx:
                if u < x:
                    b = x
                else:
                    a = x
                v, fv = w, fw
                w, fw = x, fx
                x, fx = u, fu
            else:
                if u < x:
                    a = u
                else:
                    b = u
                if fu <= fw or _precision_equals(w, x):
                    v, fv = w, fw
                    w, fw = u, fu
                elif fu <= fv or _precision_equals(v, x) or _precision_equals(v, w):
                    v, fv = u, fu

    try:
        r = gradient(point)
        direction = list(r)
        delta = 0.0
        for i in range(n):
            delta += r[i] * direction[i]
        current = None
        iters = 0
        while True:
            iters += 1
            if iters > 10000:
                raise _Stop(TOO_MANY_ITERATIONS)
            obj = objective(point)
            previous, current = current, obj
            if previous is not None and _converged(previous, current, 1e-7, 1e-7):
                return OK, np.array(point), evals[0]
            step = line_search(list(point), direction)
            for i in range(n):
                point[i] += step * direction[i]
            r = gradient(point)
            delta_old = delta
            delta = 0.0
            for i in range(n):
                delta += r[i] * r[i]
            try:
                beta = delta / delta_old
            except ZeroDivisionError:
                beta = float("nan") if delta == 0.0 or delta != delta else math.copysign(float("inf"), delta)
            if iters % n == 0 or beta < 0:
                direction = list(r)
            else:
                direction = [r[i] + beta * direction[i] for i in range(n)]
    except _Stop as s:
        return s.status, np.array(point), evals[0]
