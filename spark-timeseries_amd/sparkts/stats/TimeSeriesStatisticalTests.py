"""Host mirror of com.cloudera.sparkts.stats.TimeSeriesStatisticalTests
(S/stats/TimeSeriesStatisticalTests.scala): adftest, dwtest, lbtest, kpsstest.

Same names, arguments and exceptions as the Scala object.  Every function accepts one series
(T,) or a panel (S, T) and makes ONE batched C-ABI call (include/sts.h, t1-t4): torch GPU
tensors take the device path on torch's current stream, numpy arrays the host-staging
(`_host`) path, exactly as UnivariateTimeSeries.autocorr does.  A series gives scalars, a panel
gives (S,) arrays of the input's kind.

The object's other two functions, bgtest and bptest, take a factor matrix next to the residuals:
they are in sparkts.stats.factor_tests (t5 / t6) and exported from sparkts.stats like these four.
"""
from __future__ import annotations

from .. import _native
from .._panel import Panel, check, ptr
from ..errors import IllegalArgumentException

__all__ = ["adftest", "dwtest", "lbtest", "kpsstest", "regression_code",
           "KPSS_CONSTANT_CRITICAL_VALUES", "KPSS_CONSTANT_AND_TREND_CRITICAL_VALUES"]

# Kwiatkowski, Phillips, Schmidt & Shin (1992), table 1 (:328-341)
KPSS_CONSTANT_CRITICAL_VALUES = {0.10: 0.347, 0.05: 0.463, 0.025: 0.574, 0.01: 0.739}
KPSS_CONSTANT_AND_TREND_CRITICAL_VALUES = {0.10: 0.119, 0.05: 0.146, 0.025: 0.176, 0.01: 0.216}


def regression_code(regression: str) -> int:
    """"nc" | "c" | "ct" | "ctt" -> sts_regression (addTrend's IllegalArgumentException, :177)."""
    code = _native.lib().sts_regression_from_name(regression.encode() if isinstance(regression, str) else regression)
    if code == -2:
        raise IllegalArgumentException("Trend %s is not c, ct, or ctt" % (regression,))
    return code


def _scalar(p, v):
    """(S,) results -> a float for a single series, else the array"""
    return float(v[0]) if p.squeeze else v


def _vec(p):
    return p.empty(S=1, T=p.S).reshape(-1)


def adftest(ts, maxLag: int, regression: str = "c"):
    """:204-232 -> (statistic, MacKinnon p-value)."""
    code = regression_code(regression)
    p = Panel(ts)
    stat, pv = _vec(p), _vec(p)
    lib = _native.lib()
    if p.device:
        check(lib.sts_adf_test(ptr(p.t), p.S, p.T, p.ld, maxLag, code, ptr(stat), ptr(pv), None, p.stream), "adftest")
    else:
        check(lib.sts_adf_test_host(ptr(p.t), p.S, p.T, p.ld, maxLag, code, ptr(stat), ptr(pv), None), "adftest")
    return _scalar(p, stat), _scalar(p, pv)


def dwtest(residuals):
    """:241-252 -> the Durbin-Watson statistic."""
    p = Panel(residuals, "residuals")
    stat = _vec(p)
    lib = _native.lib()
    if p.device:
        check(lib.sts_dw_test(ptr(p.t), p.S, p.T, p.ld, ptr(stat), p.stream), "dwtest")
    else:
        check(lib.sts_dw_test_host(ptr(p.t), p.S, p.T, p.ld, ptr(stat)), "dwtest")
    return _scalar(p, stat)


def lbtest(residuals, maxLag: int):
    """:289-298 -> (statistic, chi-squared(maxLag) upper-tail p-value)."""
    p = Panel(residuals, "residuals")
    stat, pv = _vec(p), _vec(p)
    lib = _native.lib()
    if p.device:
        check(lib.sts_lb_test(ptr(p.t), p.S, p.T, p.ld, maxLag, ptr(stat), ptr(pv), p.stream), "lbtest")
    else:
        check(lib.sts_lb_test_host(ptr(p.t), p.S, p.T, p.ld, maxLag, ptr(stat), ptr(pv)), "lbtest")
    return _scalar(p, stat), _scalar(p, pv)


def kpsstest(ts, method: str):
    """:359-421 -> (statistic, {0.10: .., 0.05: .., 0.025: .., 0.01: ..} critical values)."""
    if method not in ("c", "ct"):
        raise IllegalArgumentException("requirement failed: trend must be c or ct")
    code = regression_code(method)
    crit = KPSS_CONSTANT_CRITICAL_VALUES if method == "c" else KPSS_CONSTANT_AND_TREND_CRITICAL_VALUES
    p = Panel(ts)
    stat = _vec(p)
    lib = _native.lib()
    if p.device:
        check(lib.sts_kpss_test(ptr(p.t), p.S, p.T, p.ld, code, ptr(stat), p.stream), "kpsstest")
    else:
        check(lib.sts_kpss_test_host(ptr(p.t), p.S, p.T, p.ld, code, ptr(stat)), "kpsstest")
    return _scalar(p, stat), dict(crit)
