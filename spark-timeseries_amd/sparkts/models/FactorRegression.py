"""FactorRegressionModel: a TimeSeriesModel whose time-dependent effect is a fitted linear
combination of factors (include/sts_regress.h g2).

The reference has no such model; it is the effects pair of the regression that sparkts.stats.ols
fits, so that coefficients fitted on one window can be taken out of (or put back into) other data --
out-of-sample hedged returns.  removeTimeDependentEffects(ts) = ts - (b0 + b1 f0 + b2 f1 + ...),
addTimeDependentEffects its inverse, both bit-exact in the stated order of operations.
"""
from __future__ import annotations

import numpy as np

from .. import _native
from .._panel import Panel, check, is_torch, ptr
from ..errors import IllegalArgumentException
from ..stats.factor_tests import _Factors
from ..stats.regression import ols
from .TimeSeriesModel import TimeSeriesModel


class FactorRegressionModel(TimeSeriesModel):
    """FactorRegressionModel(coefficients, factors): coefficients (k + 1,), the intercept first, for
    every series, or (S, k + 1) per series; factors (T, k) shared or (S, T, k) per series, of the
    kind (numpy / torch) of the series the effects are applied to."""

    def __init__(self, coefficients, factors):
        self.coefficients = coefficients
        self.factors = factors

    def _coefficients(self, p: Panel, k: int):
        coef = self.coefficients
        if is_torch(coef):
            coef = coef.detach()
        else:
            coef = np.asarray(coef, dtype=np.float64)
        shape = tuple(int(v) for v in coef.shape)
        if len(shape) not in (1, 2) or shape[-1] != k + 1 or (len(shape) == 2 and shape[0] not in (1, p.S)):
            raise IllegalArgumentException("FactorRegressionModel: coefficients of shape %s, expected (%d,) or (%d, %d)"
                                           % (shape, k + 1, p.S, k + 1))
        if p.device and is_torch(coef) and coef.device == p.t.device:
            import torch
            return coef.to(torch.float64).reshape(-1, k + 1).expand(p.S, k + 1).contiguous()   # no round trip
        arr = coef.cpu().numpy() if is_torch(coef) else coef
        arr = np.array(np.broadcast_to(arr.reshape(-1, k + 1), (p.S, k + 1)), dtype=np.float64, order="C")
        if p.device:
            import torch
            return torch.as_tensor(arr, device=p.t.device)
        return arr

    def _run(self, add: bool, ts, destTs):
        name = "addTimeDependentEffects" if add else "removeTimeDependentEffects"
        p = Panel(ts)
        f = _Factors(self.factors, p, name)
        coef = self._coefficients(p, f.k)
        lib = _native.lib()
        if destTs is None:
            out = p.empty()
            dptr, dld, inplace = out, p.T, False
        else:
            if is_torch(destTs) != p.device:
                raise IllegalArgumentException("%s: destTs must be of ts's kind (numpy with numpy, torch with torch)"
                                               % name)
            d = Panel(destTs, "destTs")
            if (d.S, d.T) != (p.S, p.T):
                raise IllegalArgumentException("%s: destTs of shape (%d, %d), ts (%d, %d)" % (name, d.S, d.T, p.S, p.T))
            # the call writes d.t: it must be destTs's own memory, not a copy Panel had to make
            own = (d.t.data_ptr() == destTs.data_ptr() and d.t.device == p.t.device) if p.device else (
                isinstance(destTs, np.ndarray) and np.shares_memory(d.t, destTs))
            if not own:
                raise IllegalArgumentException("%s: destTs must be a contiguous float64 panel%s"
                                               % (name, " on ts's device" if p.device else ""))
            out = destTs
            dptr, dld = d.t, d.ld
            inplace = (d.t.data_ptr() == p.t.data_ptr()) if p.device else (d.t.ctypes.data == p.t.ctypes.data)
        if p.device:
            fn = lib.sts_factor_add if add else lib.sts_factor_remove
            check(fn(ptr(p.t), ptr(dptr), p.S, p.T, p.ld, dld, ptr(f.t), f.k, f.ld_f, f.fs, ptr(coef), f.k + 1,
                     p.stream), name)
        else:
            fn = lib.sts_factor_add_host if add else lib.sts_factor_remove_host
            check(fn(ptr(p.t), ptr(p.t) if inplace else ptr(dptr), p.S, p.T, p.ld, ptr(f.t), f.k, f.ld_f, f.fs,
                     ptr(coef)), name)
        if destTs is None:
            return p.out(out)
        return destTs

    def removeTimeDependentEffects(self, ts, destTs=None):
        """ts - ((b0 + b1 f0) + b2 f1 + ...), bit-exact."""
        return self._run(False, ts, destTs)

    def addTimeDependentEffects(self, ts, destTs=None):
        """ts + ((b0 + b1 f0) + b2 f1 + ...), bit-exact."""
        return self._run(True, ts, destTs)

    @staticmethod
    def fitModel(ts, factors) -> "FactorRegressionModel":
        """The model of sparkts.stats.ols(ts, factors): one batched call, no residual panel."""
        return FactorRegressionModel(ols(ts, factors, residuals=False).coefficients, factors)


class FactorRegression:
    @staticmethod
    def fitModel(ts, factors) -> FactorRegressionModel:
        return FactorRegressionModel.fitModel(ts, factors)
