"""bgtest and bptest of com.cloudera.sparkts.stats.TimeSeriesStatisticalTests
(S/stats/TimeSeriesStatisticalTests.scala:266-278, :311-319): the two tests that take the factors of
the regression the residuals came from.

Same names, arguments and exceptions as the Scala object; residuals are one series (T,) or a panel
(S, T) as in TimeSeriesStatisticalTests.py, and each function makes ONE batched C-ABI call
(include/sts.h, t5 / t6): torch GPU tensors take the device path on torch's current stream, numpy
arrays the host-staging (`_host`) path.  A series gives floats, a panel (S,) arrays of the input's
kind.

factors has the reference's orientation: (T, k), one matrix shared by every series, or (S, T, k),
one per series, of the residuals' kind (and device).  The C ABI wants each factor as a series (time
stride 1): a view whose time axis already has stride 1 (a transposed (k, T) array, a Breeze-style
column-major matrix) is passed as it is, anything else is copied once into a contiguous (.., k, T)
array.  Wrong shapes and kinds raise IllegalArgumentException before any native call.
"""
from __future__ import annotations

from .. import _native
from .._panel import Panel, check, is_torch, ptr
from ..errors import IllegalArgumentException
from .TimeSeriesStatisticalTests import _scalar, _vec

__all__ = ["bgtest", "bptest"]


class _Factors:
    """factors (T, k) or (S, T, k) of the residuals' kind -> (array kept alive, k, ld_f, fs)."""

    def __init__(self, factors, p, name):
        if is_torch(factors) != p.device:
            raise IllegalArgumentException("%s: factors must be of the residuals' kind (numpy with numpy, torch "
                                           "with torch)" % name)
        if p.device:
            import torch
            f = factors
            if f.dtype != torch.float64:
                raise IllegalArgumentException("%s: factors must be float64, got %s" % (name, f.dtype))
            if f.device != p.t.device:
                raise IllegalArgumentException("%s: factors on %s, residuals on %s" % (name, f.device, p.t.device))
            strides = lambda a: tuple(int(v) for v in a.stride())
        else:
            import numpy as np
            f = np.asarray(factors, dtype=np.float64)
            strides = lambda a: tuple(v // 8 for v in a.strides)
        nd = f.dim() if p.device else f.ndim
        if nd == 2:
            want = (p.T,)
        elif nd == 3:
            if p.squeeze:
                raise IllegalArgumentException("%s: per-series factors (S, T, k) need a panel of residuals" % name)
            want = (p.S, p.T)
        else:
            raise IllegalArgumentException("%s: factors must be (T, k) or (S, T, k)" % name)
        shape = tuple(int(v) for v in f.shape)
        if shape[:-1] != want or shape[-1] < 1:
            raise IllegalArgumentException("%s: factors of shape %s do not match residuals (S=%d, T=%d)"
                                           % (name, shape, p.S, p.T))
        self.k = k = shape[-1]
        T = p.T
        # (.., T, k) -> (.., k, T): factor j is a row with time stride 1
        ft = f.transpose(-1, -2) if p.device else f.swapaxes(-1, -2)
        st = strides(ft)
        ok = T == 1 or st[-1] == 1
        ld_f = st[-2] if k > 1 else T
        ok = ok and ld_f >= T
        if nd == 3:
            fs = st[0] if p.S > 1 else (k - 1) * ld_f + T
            ok = ok and fs >= (k - 1) * ld_f + T
        if not ok:
            ft = ft.contiguous() if p.device else np.ascontiguousarray(ft)
            ld_f = T
            fs = k * T
        self.t = ft
        self.ld_f = ld_f
        self.fs = fs if nd == 3 else 0


def bptest(residuals, factors):
    """:311-319 -> (Breusch-Pagan statistic, chi-squared(k) upper-tail p-value)."""
    p = Panel(residuals, "residuals")
    f = _Factors(factors, p, "bptest")
    stat, pv = _vec(p), _vec(p)
    lib = _native.lib()
    if p.device:
        check(lib.sts_bp_test(ptr(p.t), p.S, p.T, p.ld, ptr(f.t), f.k, f.ld_f, f.fs, ptr(stat), ptr(pv), None,
                              p.stream), "bptest")
    else:
        check(lib.sts_bp_test_host(ptr(p.t), p.S, p.T, p.ld, ptr(f.t), f.k, f.ld_f, f.fs, ptr(stat), ptr(pv), None),
              "bptest")
    return _scalar(p, stat), _scalar(p, pv)


def bgtest(residuals, factors, maxLag: int):
    """:266-278 -> (Breusch-Godfrey statistic, chi-squared(maxLag) upper-tail p-value)."""
    p = Panel(residuals, "residuals")
    f = _Factors(factors, p, "bgtest")
    stat, pv = _vec(p), _vec(p)
    lib = _native.lib()
    if p.device:
        check(lib.sts_bg_test(ptr(p.t), p.S, p.T, p.ld, ptr(f.t), f.k, f.ld_f, f.fs, maxLag, ptr(stat), ptr(pv), None,
                              p.stream), "bgtest")
    else:
        check(lib.sts_bg_test_host(ptr(p.t), p.S, p.T, p.ld, ptr(f.t), f.k, f.ld_f, f.fs, maxLag, ptr(stat), ptr(pv),
                                   None), "bgtest")
    return _scalar(p, stat), _scalar(p, pv)
