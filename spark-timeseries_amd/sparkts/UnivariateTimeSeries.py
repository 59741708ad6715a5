"""Host mirror of com.cloudera.sparkts.UnivariateTimeSeries (S/UnivariateTimeSeries.scala).

Same function names, argument meaning and exceptions as the Scala object; every
function accepts one series (T,) or a whole panel (S, T) and dispatches ONE batched
C-ABI call (include/sts.h, include/sts_transforms.h, include/sts_roll.h) -- torch GPU tensors take the device path on torch's
current stream, numpy arrays take the host-staging (`_host`) path.  Results are
always fresh arrays, as in the reference.
"""
from __future__ import annotations

import numpy as np

from . import _native
from ._panel import Panel, check, ptr
from .errors import UnsupportedOperationException

__all__ = ["fillts", "fillLinear", "fillNearest", "fillNext", "fillPrevious", "fillSpline", "autocorr", "lag",
           "differencesAtLag", "ar", "fill_method_code", "quotients", "price2ret", "fillWithDefault", "downsample",
           "upsample", "firstNotNaN", "lastNotNaN", "trimLeading", "trimTrailing", "inverseDifferencesAtLag",
           "differencesOfOrderD", "inverseDifferencesOfOrderD", "rollSum", "rollMean", "rollVar", "rollStd", "rollMin",
           "rollMax", "rollZScore"]


def fill_method_code(method: str) -> int:
    """fillts's string dispatch (S/UnivariateTimeSeries.scala:141-150)."""
    code = _native.lib().sts_fill_method_from_name(method.encode() if isinstance(method, str) else method)
    if code == -2:
        raise UnsupportedOperationException("unsupported fill method %r" % (method,))
    return code


def _fill(ts, code: int):
    p = Panel(ts)
    out = p.empty()
    lib = _native.lib()
    if p.device:
        check(lib.sts_fill(ptr(p.t), ptr(out), p.S, p.T, p.ld, p.T, code, None, p.stream), "fill")
    else:
        check(lib.sts_fill_host(ptr(p.t), ptr(out), p.S, p.T, p.ld, code, None), "fill")
    return p.out(out)


def fillts(ts, fillMethod: str):
    """S/UnivariateTimeSeries.scala:141-150: "linear" | "nearest" | "next" | "previous" |
    "spline"; anything else raises UnsupportedOperationException."""
    return _fill(ts, fill_method_code(fillMethod))


def fillLinear(values):
    """S/UnivariateTimeSeries.scala:247-266 (bit-exact, sequential accumulation)."""
    return _fill(values, 0)


def fillNearest(values):
    """S/UnivariateTimeSeries.scala:156-184; raises IllegalArgumentException("Input is all NaNs!")."""
    return _fill(values, 1)


def fillNext(values):
    """S/UnivariateTimeSeries.scala:214-224."""
    return _fill(values, 2)


def fillPrevious(values):
    """S/UnivariateTimeSeries.scala:194-204."""
    return _fill(values, 3)


def fillSpline(values):
    """S/UnivariateTimeSeries.scala:268-297: natural cubic spline through the non-NaN steps
    (commons-math3 3.4.1 SplineInterpolator), evaluated at every step from the first valid one
    up to the last; bit-exact.  Fewer than 3 non-NaN values raises NumberIsTooSmallException."""
    return _fill(values, 4)


def autocorr(ts, numLags: int):
    """S/UnivariateTimeSeries.scala:68-93; (K,) for a series, (S, K) for a panel."""
    p = Panel(ts)
    out = p.empty(T=numLags)
    lib = _native.lib()
    if p.device:
        check(lib.sts_autocorr(ptr(p.t), p.S, p.T, p.ld, numLags, ptr(out), p.stream), "autocorr")
    else:
        check(lib.sts_autocorr_host(ptr(p.t), p.S, p.T, p.ld, numLags, ptr(out)), "autocorr")
    return p.out(out)


def lag(ts, maxLag: int, includeOriginal: bool):
    """S/UnivariateTimeSeries.scala:37-39 -> Lag.lagMatTrimBoth (S/Lag.scala:62-77).

    Returns the Breeze DenseMatrix as a (rows, cols) array -- (S, rows, cols) for a
    panel -- whose storage is column-major per series, exactly like Breeze's."""
    p = Panel(ts)
    ncols = maxLag + (1 if includeOriginal else 0)
    rows = p.T - maxLag
    lib = _native.lib()
    if rows < 0 or maxLag < 0:
        from .errors import IllegalArgumentException
        raise IllegalArgumentException("lag: maxLag %d outside [0, %d]" % (maxLag, p.T))
    if p.device:
        import torch
        buf = torch.empty((p.S, ncols, rows), dtype=torch.float64, device=p.t.device)
        check(lib.sts_lag_matrix(ptr(p.t), ptr(buf), p.S, p.T, p.ld, maxLag, int(includeOriginal), p.stream), "lag")
        mat = buf.transpose(1, 2)
    else:
        buf = np.empty((p.S, ncols, rows), dtype=np.float64)
        check(lib.sts_lag_matrix_host(ptr(p.t), ptr(buf), p.S, p.T, p.ld, maxLag, int(includeOriginal)), "lag")
        mat = buf.transpose(0, 2, 1)
    return mat[0] if p.squeeze else mat


def differencesAtLag(ts, lag: int, destTs=None, startIndex=None):
    """S/UnivariateTimeSeries.scala:356-386.

    differencesAtLag(ts, lag) returns a differenced copy (startIndex = lag).  With
    destTs given the result is written there and returned; destTs may be ts itself,
    which reproduces the reference's in-place semantics (later elements see already
    differenced values)."""
    return _at_lag("differencesAtLag", "sts_diff_at_lag", ts, lag, destTs, startIndex)


def inverseDifferencesAtLag(diffedTs, lag: int, destTs=None, startIndex=None):
    """S/UnivariateTimeSeries.scala:397-427: destTs(i) = diffedTs(i) + destTs(i - lag) from
    startIndex (default lag) on, a copy before it.  destTs as in differencesAtLag; in place
    (destTs is diffedTs) gives the same values."""
    return _at_lag("inverseDifferencesAtLag", "sts_inverse_diff_at_lag", diffedTs, lag, destTs, startIndex)


def _at_lag(what, fn, ts, lag, destTs, startIndex):
    start = lag if startIndex is None else startIndex
    p = Panel(ts)
    lib = _native.lib()
    if destTs is None:
        dest = p.t.clone() if p.device else p.t.copy()   # ts.copy (:363)
        dview = dest
        in_place_ptr = False
        dld = (int(dview.stride(0)) if p.S > 1 else p.T) if p.device else p.T
    else:
        dp = Panel(destTs, "destTs")
        if dp.device != p.device or (dp.S, dp.T) != (p.S, p.T):
            raise ValueError("%s: destTs must be the same kind and shape as ts: (%d, %d) %s vs "
                             "(%d, %d) %s" % (what, dp.S, dp.T, "device" if dp.device else "host", p.S, p.T,
                                              "device" if p.device else "host"))
        dview = p.t if destTs is ts else dp.t     # ts may have been made unit-stride: stay in place
        in_place_ptr = dview.data_ptr() == p.t.data_ptr() if p.device else dview.ctypes.data == p.t.ctypes.data
        dld = dp.ld
        dest = dview
    if p.device:
        check(getattr(lib, fn)(ptr(p.t), ptr(dview), p.S, p.T, p.ld, p.ld if in_place_ptr else dld, lag, start,
                               p.stream), what)
    else:
        check(getattr(lib, fn + "_host")(ptr(p.t), ptr(dview), p.S, p.T, p.ld, lag, start), what)
    if destTs is not None and p.device and dview.data_ptr() != destTs.data_ptr():
        # Panel made a unit-stride copy of a strided destTs: write the result back
        destTs.copy_(dview[0] if dp.squeeze else dview)
        return destTs
    if destTs is not None and not p.device and dview is not destTs:
        np.copyto(np.asarray(destTs).reshape(dview.shape), dview)
        return destTs
    if destTs is not None:
        return destTs
    return p.out(dest)


def ar(values, maxLag: int):
    """S/UnivariateTimeSeries.scala:299 -> Autoregression.fitModel(values, maxLag)."""
    from .models.Autoregression import Autoregression
    return Autoregression.fitModel(values, maxLag)


def _resized(what, fn, ts, width, *args):
    """one call of a transform whose output has `width` columns (packed): fn(in, out, S, T, ld_in,
    ld_out, *args, stream) on the device, fn_host(in, out, S, T, ld, *args) on the host"""
    p = Panel(ts)
    w = width(p.T)
    out = p.empty(T=max(w, 0))
    lib = _native.lib()
    if p.device:
        check(getattr(lib, fn)(ptr(p.t), ptr(out), p.S, p.T, p.ld, max(w, 0), *args, p.stream), what)
    else:
        check(getattr(lib, fn + "_host")(ptr(p.t), ptr(out), p.S, p.T, p.ld, *args), what)
    return p.out(out)


def _same_shape(what, fn, ts, *args):
    p = Panel(ts)
    out = p.empty()
    lib = _native.lib()
    if p.device:
        check(getattr(lib, fn)(ptr(p.t), ptr(out), p.S, p.T, p.ld, p.T, *args, p.stream), what)
    else:
        check(getattr(lib, fn + "_host")(ptr(p.t), ptr(out), p.S, p.T, p.ld, *args), what)
    return p.out(out)


def quotients(ts, lag: int):
    """S/UnivariateTimeSeries.scala:45-53: ret(i) = ts(i + lag) / ts(i), T - lag values."""
    return _resized("quotients", "sts_quotients", ts, lambda T: T - lag, lag, 0)


def price2ret(ts, lag: int):
    """S/UnivariateTimeSeries.scala:55-63: ret(i) = ts(i + lag) / ts(i) - 1.0, T - lag values."""
    return _resized("price2ret", "sts_quotients", ts, lambda T: T - lag, lag, 1)


def fillWithDefault(values, filler: float):
    """S/UnivariateTimeSeries.scala:233-241: NaN -> filler."""
    return _same_shape("fillWithDefault", "sts_fill_with_default", values, float(filler))


def downsample(values, n: int, phase: int = 0):
    """S/UnivariateTimeSeries.scala:308-321: every n-th value from `phase` on,
    ceil((T - phase) / n) values."""
    return _resized("downsample", "sts_downsample", values,
                    lambda T: -(-(T - phase) // n) if n >= 1 and 0 <= phase < T else 0, n, phase)


def upsample(values, n: int, phase: int = 0, useZero: bool = False):
    """S/UnivariateTimeSeries.scala:331-345: T * n values, values(j) at phase + j * n and NaN
    (or 0.0 with useZero) elsewhere.  phase outside [0, n) raises IllegalArgumentException (the
    reference runs off its array there)."""
    return _resized("upsample", "sts_upsample", values, lambda T: T * n if n >= 1 else 0, n, phase, int(bool(useZero)))


def _first_last(ts, want_first: bool):
    p = Panel(ts)
    lib = _native.lib()
    if p.device:
        import torch
        res = torch.empty((p.S,), dtype=torch.int64, device=p.t.device)
        f, l = (ptr(res), None) if want_first else (None, ptr(res))
        check(lib.sts_first_last_not_nan(ptr(p.t), p.S, p.T, p.ld, f, l, p.stream), "firstNotNaN / lastNotNaN")
    else:
        res = np.empty((p.S,), dtype=np.int64)
        f, l = (ptr(res), None) if want_first else (None, ptr(res))
        check(lib.sts_first_last_not_nan_host(ptr(p.t), p.S, p.T, p.ld, f, l), "firstNotNaN / lastNotNaN")
    return int(res[0]) if p.squeeze else res


def firstNotNaN(ts):
    """S/UnivariateTimeSeries.scala:119-128: the first non-NaN position, T when there is none;
    an int for a series, an (S,) int64 array for a panel."""
    return _first_last(ts, True)


def lastNotNaN(ts):
    """S/UnivariateTimeSeries.scala:130-139: the last non-NaN position, -1 when there is none."""
    return _first_last(ts, False)


def _rows(ts, bounds):
    """ts[a:b] for a series, [ts[s, a_s:b_s]] for a panel"""
    if isinstance(bounds, tuple):
        return ts[bounds[0]:bounds[1]]
    return [ts[s][a:b] for s, (a, b) in enumerate(bounds)]


def trimLeading(ts):
    """S/UnivariateTimeSeries.scala:98-105: ts(firstNotNaN until length), empty when all NaN.  A
    slice for a series, a list of per-series slices for a panel."""
    first = firstNotNaN(ts)
    T = int(ts.shape[-1])
    if isinstance(first, int):
        return _rows(ts, (first, T))
    return _rows(ts, [(int(f), T) for f in first.tolist()])


def trimTrailing(ts):
    """S/UnivariateTimeSeries.scala:110-117, the reference's own bounds: ts(0 until lastNotNaN),
    which drops the last valid value, and an empty series when lastNotNaN <= 0."""
    last = lastNotNaN(ts)
    if isinstance(last, int):
        return _rows(ts, (0, max(last, 0)))
    return _rows(ts, [(0, max(int(l), 0)) for l in last.tolist()])


def differencesOfOrderD(ts, d: int):
    """S/UnivariateTimeSeries.scala:438-450: d sweeps of differencesAtLag(_, _, 1, i), full length."""
    return _same_shape("differencesOfOrderD", "sts_diff_order_d", ts, d)


def inverseDifferencesOfOrderD(diffedTs, d: int):
    """S/UnivariateTimeSeries.scala:459-465: the sweeps i = d..1 of inverseDifferencesAtLag(_, _, 1, i)."""
    return _same_shape("inverseDifferencesOfOrderD", "sts_inverse_diff_order_d", diffedTs, d)


# ---- rolling-window statistics (include/sts_roll.h; later releases of the reference grew rollSum /
# rollMean).  out[t] belongs to the trailing window of n steps ending at t; fewer than minPeriods
# (default n) non-NaN steps in it give NaN.  The result has ts's shape. ----

def _roll(op, ts, n, minPeriods):
    from .rolling import roll
    return roll(ts, op, n, minPeriods)


def rollSum(ts, n: int, minPeriods=None):
    """The sum of the window's non-NaN values, in ascending order."""
    return _roll("sum", ts, n, minPeriods)


def rollMean(ts, n: int, minPeriods=None):
    """rollSum over the count of non-NaN values."""
    return _roll("mean", ts, n, minPeriods)


def rollVar(ts, n: int, minPeriods=None):
    """The sample variance (divisor count - 1) in the corrected two-pass form; exactly +0.0 on a
    bit-constant window."""
    return _roll("var", ts, n, minPeriods)


def rollStd(ts, n: int, minPeriods=None):
    """sqrt(rollVar): rolling volatility."""
    return _roll("std", ts, n, minPeriods)


def rollMin(ts, n: int, minPeriods=None):
    return _roll("min", ts, n, minPeriods)


def rollMax(ts, n: int, minPeriods=None):
    return _roll("max", ts, n, minPeriods)


def rollZScore(ts, n: int, minPeriods=None):
    """(ts[t] - rollMean) / rollStd; NaN where ts[t] is NaN and on a constant window."""
    return _roll("zscore", ts, n, minPeriods)
