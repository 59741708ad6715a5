"""Host mirror of com.cloudera.sparkts.models.{ARIMA, ARIMAModel} (S/models/ARIMA.scala).

ARIMA.fitModel(p, d, 0, ts) -- the AR-only path (:80-90) -- is differencesOfOrderD(ts, d).drop(d)
followed by Autoregression.fitModel(diffed, p, !includeIntercept); both run batched on the
device (sts_arima_fit_ar).

ARIMA.fitModelCSS(p, d, q, ts) is the reference's default method, "css-cgd" (:166-192), for
every order 0 <= p, q <= 4: the Hannan-Rissanen start (:207-233, sts_arima_hr_init) unless the
caller gives one, then commons-math3's conjugate-gradient optimizer over the CSS likelihood,
run per series on the device with every evaluation in the reference's operation order
(sts_arima_fit_css): bit-exact given the start.  ARIMA.fitModel itself still refuses q > 0 and
p == 0 and names fitModelCSS.

ARIMAModel carries the whole TimeSeriesModel interface on device panels: remove / add
(:474-510), forecast (:537-605), logLikelihoodCSS and its gradient (:266-381), and the host-side
isStationary / isInvertible (:617-656).  `coefficients` is one vector (intercept, AR, MA) for
one series or for every series of a panel, or (S, n) with one row per series.

sample(n, rand, paths=None) (:517-520) is addTimeDependentEffects(vec, vec) of n draws made on
the device from a sparkts.random.PhiloxGenerator (sts_arima_sample).

Not supported: method="css-bobyqa" (commons-math3's BOBYQAOptimizer is not restated).
"""
from __future__ import annotations

import ctypes

import numpy as np

from .. import _native
from .. import random as _random
from .._panel import Panel, check, is_torch, ptr
from ..errors import IllegalArgumentException, NullPointerException, UnsupportedOperationException
from .TimeSeriesModel import TimeSeriesModel

MAX_ORDER = 4   # STS_ARIMA_MAX_ORDER


def _check_orders(p, d, q, hasIntercept, what):
    if not (0 <= p <= MAX_ORDER and 0 <= q <= MAX_ORDER):
        raise IllegalArgumentException("%s: orders p=%d, q=%d outside [0, %d]" % (what, p, q, MAX_ORDER))
    if d < 0:
        raise IllegalArgumentException("%s: negative differencing order %d" % (what, d))
    n = int(bool(hasIntercept)) + p + q
    if n < 1:
        raise IllegalArgumentException("%s: a model without intercept, AR and MA terms has no coefficients" % what)
    return n


def _device_panel(ts, what, name="ts"):
    pn = Panel(ts, name)
    if not pn.device:
        raise TypeError("%s runs on device-resident series (torch GPU tensors)" % what)
    return pn


def _coef_matrix(coefficients, pn, n, what):
    """(S, n) contiguous device tensor from a vector (every series) or one row per series"""
    import torch
    if is_torch(coefficients):
        c = coefficients.to(device=pn.t.device, dtype=torch.float64)
    else:
        c = torch.as_tensor(np.asarray(coefficients, dtype=np.float64), device=pn.t.device)
    if c.dim() == 1:
        c = c.unsqueeze(0).expand(pn.S, -1)
    if c.dim() != 2 or tuple(c.shape) != (pn.S, n):
        raise ValueError("%s: expected %d coefficients per series (%d series), got shape %s"
                         % (what, n, pn.S, tuple(c.shape)))
    return c.contiguous()


class ARIMAModel(TimeSeriesModel):
    """ARIMAModel(p, d, q, coefficients, hasIntercept) (S/models/ARIMA.scala:251-256):
    coefficients = [intercept] ++ AR ++ MA, per series ((S, n) for a panel)."""

    def __init__(self, p, d, q, coefficients, hasIntercept=True):
        self.p, self.d, self.q = p, d, q
        self.coefficients = coefficients
        self.hasIntercept = hasIntercept

    def _n(self, what):
        return _check_orders(self.p, self.d, self.q, self.hasIntercept, what)

    def _effects(self, add, ts, dest):
        what = "ARIMAModel.%sTimeDependentEffects" % ("add" if add else "remove")
        n = self._n(what)
        if dest is None:   # the reference writes into destTs (:485, :508): NPE
            raise NullPointerException("%s: dest is null" % what)
        pn = _device_panel(ts, what)
        dn = _device_panel(dest, what, "dest")
        coef = _coef_matrix(self.coefficients, pn, n, what)
        fn = _native.lib().sts_arima_add if add else _native.lib().sts_arima_remove
        check(fn(ptr(pn.t), ptr(dn.t), pn.S, pn.T, pn.ld, dn.ld, self.p, self.d, self.q, int(bool(self.hasIntercept)),
                 ptr(coef), pn.stream), what)
        return dest

    def removeTimeDependentEffects(self, ts, dest=None):
        """S/models/ARIMA.scala:474-487 (bit-exact); dest may be ts (the reference works on copies)."""
        return self._effects(False, ts, dest)

    def addTimeDependentEffects(self, ts, dest=None):
        """S/models/ARIMA.scala:498-510 (bit-exact); dest may be ts."""
        return self._effects(True, ts, dest)

    def sample(self, n: int, rand, paths=None, device=None):
        """S/models/ARIMA.scala:517-520 (bit-exact given the draws): (n,) for one coefficient
        vector, (paths, n) for `paths` paths of it, (S, n) for (S, ncoef) coefficients."""
        what = "ARIMAModel.sample"
        _random.require_generator(rand, what)
        ncoef = self._n(what)
        lib = _native.lib()
        return _random.run_sample(
            what, n, rand, paths, [(self.coefficients, "coefficients", 1, ncoef)], device,
            lambda out, S, v, t0, st: lib.sts_arima_sample(ptr(out), rand.first_series, S, n, n, self.p, self.d, self.q,
                                                           int(bool(self.hasIntercept)), ptr(v[0]), t0,
                                                           ctypes.c_uint64(rand.seed), st))

    def forecast(self, ts, nFuture: int):
        """S/models/ARIMA.scala:537-605: the fitted one-step values of ts followed by nFuture
        forecasts, (T + nFuture,) or (S, T + nFuture)."""
        what = "ARIMAModel.forecast"
        n = self._n(what)
        if nFuture < 0:
            raise IllegalArgumentException("%s: negative nFuture" % what)
        pn = _device_panel(ts, what)
        coef = _coef_matrix(self.coefficients, pn, n, what)
        out = pn.empty(pn.S, pn.T + nFuture)
        check(_native.lib().sts_arima_forecast(ptr(pn.t), ptr(out), pn.S, pn.T, pn.ld, pn.T + nFuture, self.p, self.d,
                                               self.q, int(bool(self.hasIntercept)), ptr(coef), nFuture, pn.stream),
              what)
        return pn.out(out)

    def _loglik_grad(self, y, want_ll, want_grad):
        import torch
        what = "ARIMAModel.logLikelihoodCSS"
        n = self._n(what)
        pn = _device_panel(y, what, "y")
        coef = _coef_matrix(self.coefficients, pn, n, what)
        ll = torch.empty((pn.S,), dtype=torch.float64, device=pn.t.device) if want_ll else None
        g = torch.empty((pn.S, n), dtype=torch.float64, device=pn.t.device) if want_grad else None
        check(_native.lib().sts_arima_css_loglik_gradient(ptr(pn.t), pn.S, pn.T, pn.ld, self.p, self.d, self.q,
                                                          int(bool(self.hasIntercept)), ptr(coef), ptr(ll), ptr(g),
                                                          pn.stream), what)
        return (pn.out(ll) if want_ll else None, (g[0] if pn.squeeze else g) if want_grad else None)

    def logLikelihoodCSS(self, y):
        """S/models/ARIMA.scala:266-293, per series (y is differenced by d first)."""
        return self._loglik_grad(y, True, False)[0]

    def gradientlogLikelihoodCSS(self, y):
        """gradientlogLikelihoodCSSARMA (S/models/ARIMA.scala:312-381) of y differenced by d."""
        return self._loglik_grad(y, False, True)[1]

    def _host_coefficients(self):
        c = self.coefficients
        c = c.detach().cpu().numpy() if is_torch(c) else np.asarray(c, dtype=np.float64)
        return c

    def _roots_outside(self, lo, hi, sign):
        """allRootsOutsideUnitCircle (:650-656) of 1 + sign * (c[lo] x + c[lo + 1] x^2 + ...)"""
        c = self._host_coefficients()
        rows = c.reshape(1, -1) if c.ndim == 1 else c
        res = np.empty(rows.shape[0], dtype=bool)
        for s, row in enumerate(rows):
            poly = np.concatenate([[1.0], sign * row[lo:hi]])
            roots = np.roots(poly[::-1])
            res[s] = not bool((np.abs(roots) <= 1.0).any())
        return bool(res[0]) if c.ndim == 1 else res

    def isStationary(self):
        """S/models/ARIMA.scala:617-625 (host): the AR polynomial's roots lie outside the unit
        circle; True without AR terms.  A bool, or one per series."""
        if self.p == 0:
            return True
        off = int(bool(self.hasIntercept))
        return self._roots_outside(off, off + self.p, -1.0)

    def isInvertible(self):
        """S/models/ARIMA.scala:634-642 (host): the same for the MA polynomial."""
        if self.q == 0:
            return True
        off = int(bool(self.hasIntercept)) + self.p
        return self._roots_outside(off, off + self.q, 1.0)


class ARIMA:
    @staticmethod
    def fitModel(p: int, d: int, q: int, ts, includeIntercept: bool = True, method: str = "css-cgd",
                 userInitParams=None) -> ARIMAModel:
        if not (p > 0 and q == 0):
            raise UnsupportedOperationException(
                "ARIMA.fitModel(p=%d, d=%d, q=%d): only the AR path (p > 0, q = 0) runs here; "
                "use ARIMA.fitModelCSS for models with MA terms or without AR terms" % (p, d, q))
        pn = Panel(ts)
        if not pn.device:
            raise TypeError("ARIMA.fitModel runs on device-resident series (torch GPU tensors)")
        import torch
        c = torch.empty((pn.S,), dtype=torch.float64, device=pn.t.device)
        coef = torch.empty((pn.S, p), dtype=torch.float64, device=pn.t.device)
        check(_native.lib().sts_arima_fit_ar(ptr(pn.t), pn.S, pn.T, pn.ld, p, d, int(includeIntercept), ptr(c),
                                             ptr(coef), None, pn.stream), "ARIMA.fitModel")
        params = torch.cat([c[:, None], coef], dim=1) if includeIntercept else coef
        if pn.squeeze:
            params = params[0]
        return ARIMAModel(p, d, q, params, includeIntercept)

    @staticmethod
    def fitModelCSS(p: int, d: int, q: int, ts, includeIntercept: bool = True, userInitParams=None, errors=None,
                    method: str = "css-cgd") -> ARIMAModel:
        """ARIMA.fitModel's "css-cgd" method (S/models/ARIMA.scala:73-110, :166-192) for a series
        or a panel.  The start is HannanRissanenInit (:207-233) unless userInitParams (a vector,
        or (S, n)) is given; the model keeps it as `initParams` and the objective evaluations
        commons-math3 counted as `evaluations`.  A series the optimizer cannot fit raises the
        reference's exception (TooManyEvaluationsException ...), unless `errors` (S int32, on
        the device) is given: then it receives the per-series status and that series'
        coefficients are NaN.  With p > 0 and q == 0 this is fitModel (:84-90)."""
        what = "ARIMA.fitModelCSS"
        n = _check_orders(p, d, q, includeIntercept, what)
        if method != "css-cgd":
            raise UnsupportedOperationException("%s: method %r is not supported (only \"css-cgd\")" % (what, method))
        if p > 0 and q == 0:
            return ARIMA.fitModel(p, d, q, ts, includeIntercept)
        import torch
        pn = _device_panel(ts, what)
        lib = _native.lib()
        icpt = int(bool(includeIntercept))
        hr_err = None
        if userInitParams is None:
            init = torch.empty((pn.S, n), dtype=torch.float64, device=pn.t.device)
            hr_err = pn.empty_i32(pn.S) if errors is not None else None
            check(lib.sts_arima_hr_init(ptr(pn.t), pn.S, pn.T, pn.ld, p, d, q, icpt, ptr(init), ptr(hr_err), pn.stream),
                  what + " (Hannan-Rissanen start)")
        else:
            init = _coef_matrix(userInitParams, pn, n, what)
        coef = torch.empty((pn.S, n), dtype=torch.float64, device=pn.t.device)
        evals = pn.empty_i32(pn.S)
        check(lib.sts_arima_fit_css(ptr(pn.t), pn.S, pn.T, pn.ld, p, d, q, icpt, ptr(init), ptr(coef), ptr(errors),
                                    ptr(evals), pn.stream), what)
        if hr_err is not None:   # a failed start keeps its own status
            errors.copy_(torch.where(hr_err != 0, hr_err, errors))
        model = ARIMAModel(p, d, q, coef[0] if pn.squeeze else coef, includeIntercept)
        model.initParams = init[0] if pn.squeeze else init
        model.evaluations = int(evals[0]) if pn.squeeze else evals
        return model
