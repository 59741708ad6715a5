"""ols: the regression whose residuals bgtest / bptest take (include/sts_regress.h g1).

The reference has no operator of its own for it: its suite regresses with commons-math3
OLSMultipleLinearRegression (TimeSeriesStatisticalTestsSuite.scala:39-45, 72-78), and OLSResult
carries what that class hands back, under its names.  y is one series (T,) or a panel (S, T), and the
call makes ONE batched C-ABI call: torch GPU tensors take the device path on torch's current stream,
numpy arrays the host-staging (`_host`) path.  factors are (T, k), one matrix shared by every
series, or (S, T, k), one per series, of y's kind, exactly as factor_tests takes them.  Wrong shapes
and kinds raise IllegalArgumentException before any native call.
"""
from __future__ import annotations

from .. import _native
from .._panel import Panel, check, ptr
from ..errors import IllegalArgumentException, MathIllegalArgumentException
from .factor_tests import _Factors

__all__ = ["ols", "OLSResult", "MAX_FACTORS"]

MAX_FACTORS = 8   # STS_MAX_FACTORS


class OLSResult:
    """OLS with intercept of y on 1, F_0 .. F_{k-1}.  A panel gives (S, k + 1) / (S,) / (S, T) arrays
    of the input's kind, a single series (k + 1,) arrays and floats.

    coefficients, standardErrors: the intercept first (estimateRegressionParameters,
    estimateRegressionParametersStandardErrors); tStatistics = coefficients / standardErrors.
    residualSumOfSquares, totalSumOfSquares (centred), rSquared, errorVariance (rss / (T - k - 1)):
    the calculate* / estimateErrorVariance values; adjustedRSquared = 1 - rss (T - 1) / (tss (T - k - 1))
    and regressionStandardError = sqrt(errorVariance) are derived as commons-math3 derives them.
    residuals: estimateResiduals(), or None when not asked for.  errors: int32 statuses per series.
    """

    def __init__(self, p, k, beta, se, stats, resid, err):
        self.numFactors = k
        self.numObservations = p.T
        self.coefficients = p.out(beta)
        self.standardErrors = p.out(se)
        self.tStatistics = self.coefficients / self.standardErrors

        def col(v):
            return float(v[0]) if p.squeeze else v

        rss, tss = stats[:, 0], stats[:, 1]
        self.residualSumOfSquares = col(rss)
        self.totalSumOfSquares = col(tss)
        self.rSquared = col(stats[:, 2])
        self.errorVariance = col(stats[:, 3])
        self.adjustedRSquared = col(1.0 - (rss * (p.T - 1.0)) / (tss * (p.T - k - 1.0)))
        self.regressionStandardError = col(stats[:, 3] ** 0.5)
        self.residuals = None if resid is None else p.out(resid)
        self.errors = err


def ols(y, factors, residuals: bool = True) -> OLSResult:
    """OLS with intercept of every series of y on the factors -> OLSResult.  Per-series outcomes of a
    panel are in OLSResult.errors (a rank-deficient design: STS_ERR_SINGULAR and NaN results) and do
    not raise; a single series raises its status.  A series with a NaN gets NaN results, status 0."""
    p = Panel(y, "y")
    f = _Factors(factors, p, "ols")
    if f.k > MAX_FACTORS:
        raise IllegalArgumentException("ols: %d factors, at most %d" % (f.k, MAX_FACTORS))
    if p.T <= f.k + 1:
        raise MathIllegalArgumentException("ols: not enough data (%d rows) for the number of predictors (%d)"
                                           % (p.T, f.k + 1))
    w = f.k + 1
    beta, se, stats = p.empty(T=w), p.empty(T=w), p.empty(T=4)
    resid = p.empty() if residuals else None
    err = p.empty_i32(p.S)
    lib = _native.lib()
    if p.device:
        st = lib.sts_factor_ols(ptr(p.t), p.S, p.T, p.ld, ptr(f.t), f.k, f.ld_f, f.fs, ptr(beta), w, ptr(se),
                                ptr(stats), ptr(resid), p.T, ptr(err), p.stream)
    else:
        st = lib.sts_factor_ols_host(ptr(p.t), p.S, p.T, p.ld, ptr(f.t), f.k, f.ld_f, f.fs, ptr(beta), ptr(se),
                                     ptr(stats), ptr(resid), ptr(err))
    check(st, "ols")
    if p.squeeze:
        check(int(err[0]), "ols")   # one series: its status is the call's, as the reference's exception
    return OLSResult(p, f.k, beta, se, stats, resid, err)
