"""The stream contract of include/sts.h ("Stream contract": every device entry point is
stream-ordered on `stream`, NULL meaning hipStreamPerThread) on every entry point whose last parameter is
`void* stream`, through the C ABI and through the Python mirror.  Needs an MI355X.

Every row of TABLE is one entry point at one small packed shape (S between 5 and 70) chosen to
take its multi-launch path.  A row is run through the gate of tests/stream_gate.py on a fresh
non-blocking torch stream and must

  * give snapshots bit-identical to the same call made plainly (NULL stream, device synchronised
    before and after), whose result in turn meets the operator's existing bar against the oracle
    (the assertion helpers of test_layout_gpu.py and of the operator's own test module),
  * leave every output buffer holding the sentinel after the final synchronise (nothing ran late),
  * return the plain call's status and host values,
  * when the row is not in SYNC: return while the event after the delay is still pending.

test_two_streams runs two gated calls of one row, on different panels, on two streams in flight
together: each must match its own plain result (shared scratch, device globals).

ASYNC / SYNC (read from sts_api.cpp).  An entry point returns before its work ran unless
  - err_per_series == NULL: ErrSink::finish() synchronises the stream and reports the first
    failing series ("wait and turn the first failing series into a status"); sts_autocorr always
    passes NULL ("return sts_fill_autocorr(in, nullptr, ..., nullptr, stream)"),
  - sts_ar_rule_count: "HIP_TRY(hipStreamSynchronize(st), name);" before "*count = (int64_t)h;"
    (sts.h: "synchronous"),
  - sts_fill_autocorr with T == 0 and K > 0: the NaN ACF comes from a host vector,
    "HIP_TRY(hipStreamSynchronize(st), "acf");",
  - sts_stream_synchronize.
Every other row, with a non-NULL error array where the entry point takes one, is in ASYNC.

The mirror level (TimeSeriesRDD, the models, the tests, io.toWire) runs the same gate once on a
side stream and once on torch's default stream.  The default-stream case pins what the mirror
relies on there: Panel.stream hands the library handle 0, i.e. hipStreamPerThread, while torch's
producers and consumers run on the legacy null stream, and nothing in the project orders the two.
Observed: the results are the plain call's bits ("Stream contract").  MIRROR says for
each pipeline whether its call returns with the gate still shut; io.toWire opens the gate itself
before its library call and is not evidence either way.

No graph capture, at most two streams in flight, one finite delay per gated call.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
import stream_gate as sg
from stream_gate import GIn, Case, vp
from test_layout_gpu import assert_bits, assert_rel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sts.h")
NaN = np.nan
ALL_NAN = 2
_MEMO = {}


def memo(key, fn):
    """references are computed once and shared (plain, gated and two-stream runs of a row)"""
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


@pytest.fixture(scope="module")
def delay(torch):
    """cycles of the calibrated ~20 ms delay (fails, does not skip, outside 10-200 ms)"""
    return sg.calibrate(torch)[0]


def L():
    from sparkts import _native
    return _native.lib()


def stream_entry_points():
    """every function of sts.h whose last parameter is `void* stream` (parsed as test_abi.py does)"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(m.group(2) for m in re.finditer(r"\b(int|const char\*)\s+(sts_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
                  if re.search(r"void\s*\*\s*stream\s*$", m.group(3).strip()))


def gins(torch, gen, v, dtypes=None):
    """gen(k) -> list of numpy inputs; real = gen(v), the decoys gen(50 + v) and gen(90 + v)"""
    real, d1, d2 = (memo((gen, k), lambda k=k: gen(k)) for k in (v, 50 + v, 90 + v))
    dtypes = dtypes or [np.float64] * len(real)
    return [GIn(torch, a, b, c, dt) for a, b, c, dt in zip(real, d1, d2, dtypes)], real


def out(torch, shape, dtype=None):
    return torch.empty(shape, dtype=dtype or torch.float64, device="cuda:0")


def i32(torch, n):
    return out(torch, (n,), torch.int32)


SYNC_NULL_ERR = "err_per_series == NULL: ErrSink::finish() synchronises (sts_api.cpp, 'wait and turn the first failing series into a status')"

TABLE = []      # (id, entry points covered, build(torch, v) -> Case, sync)


def row(ident, *covers, sync=None):
    """sync: None for a row on the ASYNC list, else why the entry point synchronises by design"""
    def deco(build):
        TABLE.append((ident, covers, build, sync))
        return build
    return deco


# ---------------- fills ----------------

def _fill_gen(method):
    def gen(k):
        x = oracle.gen_panel(100 + k, 5, 390, 0.05)
        x[1, 0] = NaN
        x[2, -1] = NaN
        if method == "nearest":
            x[4, :] = NaN
        return [x]
    return memo(("fill_gen", method), lambda: gen)


for _m in ("linear", "nearest", "next", "previous", "spline"):
    @row("fill-" + _m, "sts_fill")
    def _b(torch, v, method=_m):
        S, T = 5, 390
        ins, (x,) = gins(torch, _fill_gen(method), v)
        o, e = out(torch, (S, T)), i32(torch, S)
        ref, rerr = memo(("fill", method, v), lambda: oracle.panel_fill(x, method))

        def check(outs, host):
            assert np.array_equal(outs[1], rerr), (outs[1], rerr)
            ok = rerr == 0
            assert_bits(outs[0][ok], ref[ok], "fill " + method)
        return Case(ins, [o, e], lambda st: L().sts_fill(vp(ins[0].buf), vp(o), S, T, T, T, oracle.FILL_METHODS[method],
                                                        vp(e), st), check)


# ---------------- ACF: fused partials + finalize, wide blocks, the exact loop; rule 3 ----------------

def _acf_gen(T, nans):
    def gen(k):
        from test_acf_robust import hard_rows, with_nans
        x = hard_rows(T, 7 + k)                    # series far from their level: rule 3's recompute runs
        return [with_nans(x, np.random.default_rng(k)) if nans else x]
    return memo(("acf_gen", T, nans), lambda: gen)


def _check_acf(got, ref, src, K, what):
    from test_acf_robust import noise_floor, rel_err, within
    e = within(got, ref, np.array([noise_floor(r, K) for r in src]))
    assert e <= 1.0, "%s: error %.3g x (1e-10 rel + noise floor)" % (what, e)
    assert rel_err(got[:-1], ref[:-1]) <= 1e-10, what     # every row but the outlier-dominated last one


for _T, _K in ((390, 20), (390, 64), (100, 60)):
    @row("fill_autocorr-T%d-K%d" % (_T, _K), "sts_fill_autocorr")
    def _b(torch, v, T=_T, K=_K):
        S = 9
        ins, (x,) = gins(torch, _acf_gen(T, True), v)
        f, acf, e = out(torch, (S, T)), out(torch, (S, K)), i32(torch, S)
        rf, racf, rerr = memo(("fill_acf", T, K, v), lambda: oracle.panel_fill_autocorr(x, "linear", K))

        def check(outs, host):
            assert np.array_equal(outs[2], rerr)
            assert_bits(outs[0], rf, "filled")
            _check_acf(outs[1], racf, rf, K, "fill_autocorr T=%d K=%d" % (T, K))
        return Case(ins, [f, acf, e], lambda st: L().sts_fill_autocorr(vp(ins[0].buf), vp(f), S, T, T, T, 0, K, vp(acf),
                                                                       vp(e), st), check)


@row("fill_autocorr-T0", "sts_fill_autocorr",
     sync="T == 0: the NaN ACF is copied from a host vector, 'HIP_TRY(hipStreamSynchronize(st), \"acf\");'")
def _b(torch, v):
    S, K = 5, 3
    acf, e = out(torch, (S, K)), i32(torch, S)

    def check(outs, host):
        assert np.isnan(outs[0]).all() and (outs[1] == 0).all()
    return Case([], [acf, e], lambda st: L().sts_fill_autocorr(None, None, S, 0, 0, 0, -1, K, vp(acf), vp(e), st), check)


@row("autocorr-T390-K64", "sts_autocorr", sync=SYNC_NULL_ERR)
def _b(torch, v):
    S, T, K = 9, 390, 64
    ins, (x,) = gins(torch, _acf_gen(T, False), v)
    acf = out(torch, (S, K))
    racf = memo(("acf", v), lambda: np.array([oracle.autocorr(r, K) for r in x]))
    return Case(ins, [acf], lambda st: L().sts_autocorr(vp(ins[0].buf), S, T, T, K, vp(acf), st),
                lambda outs, host: _check_acf(outs[0], racf, x, K, "autocorr"))


# ---------------- index-driven work and recurrences: bit-exact ----------------

def _rec_gen(k):
    rng = np.random.default_rng(1000 + k)
    S, T = 7, 390
    return [rng.standard_normal((S, T)) + 10, rng.uniform(0.05, 0.95, S), rng.standard_normal(S),
            rng.uniform(-0.3, 0.3, (S, 8))]


def _rec_row(ident, name, ref_fn, args):
    @row(ident, name)
    def _b(torch, v):
        S, T = 7, 390
        ins, (x, sm, c, coef) = gins(torch, _rec_gen, v)
        o = out(torch, (S, T))
        ref = memo((ident, v), lambda: np.array([ref_fn(x, sm, c, coef, s) for s in range(S)]))
        bx, bsm, bc, bcoef = (g.buf for g in ins)
        return Case(ins, [o], lambda st: getattr(L(), name)(vp(bx), vp(o), S, T, T, T, *args(bsm, bc, bcoef), st),
                    lambda outs, host: assert_bits(outs[0], ref, ident))


_rec_row("diff_at_lag", "sts_diff_at_lag", lambda x, sm, c, f, s: oracle.differences_at_lag(x[s], 3, start=7),
         lambda sm, c, f: (3, 7))
_rec_row("ewma_add", "sts_ewma_add", lambda x, sm, c, f, s: oracle.ewma_add(x[s], sm[s]), lambda sm, c, f: (vp(sm),))
_rec_row("ewma_remove", "sts_ewma_remove", lambda x, sm, c, f, s: oracle.ewma_remove(x[s], sm[s]), lambda sm, c, f: (vp(sm),))
_rec_row("ar_remove", "sts_ar_remove", lambda x, sm, c, f, s: oracle.ar_remove(x[s], c[s], f[s]),
         lambda sm, c, f: (vp(c), vp(f), 8))
_rec_row("ar_add", "sts_ar_add", lambda x, sm, c, f, s: oracle.ar_add(x[s], c[s], f[s]), lambda sm, c, f: (vp(c), vp(f), 8))


def _lag_gen(k):
    x = oracle.gen_panel(5 + k, 5, 65, 0.3)
    x[:, 1] = 1.0
    return [x]


def _lag_filled_gen(k):
    return [oracle.panel_fill(_lag_gen(k)[0], "next")[0]]      # real and decoys alike: no NaN paths


@row("lag_matrix", "sts_lag_matrix")
def _b(torch, v):
    S, T, p = 5, 65, 10
    ins, (f,) = gins(torch, _lag_filled_gen, v)
    ref = np.concatenate([oracle.lag(r, p, True).T.ravel() for r in f])
    lm = out(torch, (ref.size,))
    return Case(ins, [lm], lambda st: L().sts_lag_matrix(vp(ins[0].buf), vp(lm), S, T, T, p, 1, st),
                lambda outs, host: assert_bits(outs[0], ref, "lag_matrix"))


@row("fill_lag_matrix", "sts_fill_lag_matrix")
def _b(torch, v):
    S, T, p = 5, 65, 10
    ins, (x,) = gins(torch, _lag_gen, v)
    f = oracle.panel_fill(x, "linear")[0]
    ref = np.concatenate([oracle.lag(r, p, True).T.ravel() for r in f])
    fo, lm, e = out(torch, (S, T)), out(torch, (ref.size,)), i32(torch, S)

    def check(outs, host):
        assert (outs[2] == 0).all()
        assert_bits(outs[0], f, "filled")
        assert_bits(outs[1], ref, "fill_lag_matrix")
    return Case(ins, [fo, lm, e], lambda st: L().sts_fill_lag_matrix(vp(ins[0].buf), vp(fo), vp(lm), S, T, T, T, 0, p, 1,
                                                                    vp(e), st), check)


def _c2_gen(k):
    rng = np.random.default_rng(7 + k)
    S, T = 7, 390
    x = 100 + rng.standard_normal((S, T)).cumsum(axis=1)
    x[rng.random((S, T)) < 0.2] = NaN
    x[0, :5] = NaN
    x[2, :] = NaN
    return [x, rng.uniform(0.05, 0.95, S)]


for _m, _lag in (("previous", 1), ("linear", 3)):     # the fused recurrence | fill -> scratch -> diff -> EWMA add
    @row("fill_diff_ewma-" + _m, "sts_fill_diff_ewma")
    def _b(torch, v, method=_m, lag=_lag):
        S, T = 7, 390
        ins, (x, sm) = gins(torch, _c2_gen, v)
        fill = {"previous": oracle.fill_previous, "linear": oracle.fill_linear}[method]
        ref = memo(("c2", method, v), lambda: np.array([oracle.ewma_add(oracle.differences_at_lag(fill(r), lag), q)
                                                        for r, q in zip(x, sm)]))
        o, e = out(torch, (S, T)), i32(torch, S)

        def check(outs, host):
            assert (outs[1] == 0).all()
            assert_bits(outs[0], ref, "fill_diff_ewma " + method)
        return Case(ins, [o, e], lambda st: L().sts_fill_diff_ewma(vp(ins[0].buf), vp(o), S, T, T, T,
                                                                   oracle.FILL_METHODS[method], lag, vp(ins[1].buf), vp(e), st),
                    check)


# ---------------- EWMA fit, seriesStats ----------------

def _ewma_gen(k):
    rng = np.random.default_rng(1000 + k)
    S, T = 7, 65
    return [np.cumsum(rng.standard_normal((S, T)), axis=1) + 50 + rng.uniform(-5, 5, (S, 1)), rng.uniform(0.05, 1.5, S)]


@row("ewma_fit", "sts_ewma_fit")
def _b(torch, v):
    S, T = 7, 65
    ins, (x, _) = gins(torch, _ewma_gen, v)
    fit, e = out(torch, (S,)), i32(torch, S)
    rfit, rerr = memo(("ewma_fit", v), lambda: oracle.panel_ewma_fit(x))

    def check(outs, host):
        assert np.array_equal(outs[1], rerr)
        assert_bits(outs[0], rfit, "ewma_fit")
    return Case(ins[:1], [fit, e], lambda st: L().sts_ewma_fit(vp(ins[0].buf), S, T, T, vp(fit), vp(e), st), check)


@row("ewma_sse_gradient", "sts_ewma_sse_gradient")
def _b(torch, v):
    S, T = 7, 65
    ins, (x, sm) = gins(torch, _ewma_gen, v)
    sse, grad = out(torch, (S,)), out(torch, (S,))

    def check(outs, host):
        assert_bits(outs[0], np.array([oracle.ewma_sse(r, q) for r, q in zip(x, sm)]), "sse")
        assert_bits(outs[1], np.array([oracle.ewma_gradient(r, q) for r, q in zip(x, sm)]), "gradient")
    return Case(ins, [sse, grad], lambda st: L().sts_ewma_sse_gradient(vp(ins[0].buf), S, T, T, vp(ins[1].buf), vp(sse),
                                                                      vp(grad), st), check)


@row("series_stats", "sts_series_stats")
def _b(torch, v):
    S, T = 7, 65
    ins, (x, _) = gins(torch, _ewma_gen, v)
    stats = out(torch, (S, 4))
    return Case(ins[:1], [stats], lambda st: L().sts_series_stats(vp(ins[0].buf), S, T, T, vp(stats), st),
                lambda outs, host: assert_bits(outs[0], np.array([oracle.stat_counter(r)[1:] for r in x]), "series_stats"))


# ---------------- GARCH / ARGARCH, T = 200 ----------------
G_S, G_T = 5, 200


def _garch_gen(k):
    from mt19937 import MersenneTwister
    from test_garch import argarch_sample, garch_panel
    rng = np.random.default_rng(9 + k)
    S = G_S
    y = np.vstack([argarch_sample(1.0 + 0.1 * s, 0.3 - 0.05 * s, 0.2, 0.3, 0.4, G_T, MersenneTwister(40 + 7 * k + s))
                   for s in range(S)])
    om, al, be = rng.uniform(0.05, 0.4, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.1, 0.5, S)
    return [garch_panel(S, G_T, 21 + 11 * k), y, rng.uniform(-1, 1, S), rng.uniform(-0.5, 0.5, S), om, al, be,
            np.stack([om, al, be], axis=1)]


@row("garch_fit", "sts_garch_fit")
def _b(torch, v):
    ins, real = gins(torch, _garch_gen, v)
    par, e = out(torch, (G_S, 3)), i32(torch, G_S)
    rpar, rerr = memo(("garch_fit", v), lambda: oracle.panel_garch_fit(real[0]))

    def check(outs, host):
        assert np.array_equal(outs[1], rerr)
        assert_bits(outs[0], rpar, "garch_fit")
    return Case(ins[:1], [par, e], lambda st: L().sts_garch_fit(vp(ins[0].buf), G_S, G_T, G_T, vp(par), vp(e), st), check)


@row("argarch_fit", "sts_argarch_fit")
def _b(torch, v):
    ins, real = gins(torch, _garch_gen, v)
    y = real[1]
    c, phi, par, e = out(torch, (G_S,)), out(torch, (G_S,)), out(torch, (G_S, 3)), i32(torch, G_S)

    def check(outs, host):
        gc, gphi, gpar, gerr = outs
        fits = [oracle.ar_fit(r, 1, False) for r in y]
        assert np.allclose(gc, [f[0] for f in fits], rtol=1e-10, atol=0)
        assert np.allclose(gphi, [f[1][0] for f in fits], rtol=1e-10, atol=0)
        # the GARCH stage: bit-exact given the device's own (c, phi) residuals
        rpar, rerr = oracle.panel_garch_fit(np.array([oracle.ar_remove(y[s], gc[s], [gphi[s]]) for s in range(G_S)]))
        assert np.array_equal(gerr, rerr)
        assert_bits(gpar, rpar, "argarch_fit")
    return Case(ins[1:2], [c, phi, par, e], lambda st: L().sts_argarch_fit(vp(ins[1].buf), G_S, G_T, G_T, vp(c), vp(phi),
                                                                          vp(par), vp(e), st), check)


@row("garch_loglik_gradient", "sts_garch_loglik_gradient")
def _b(torch, v):
    ins, (x, _, _, _, om, al, be, _) = gins(torch, _garch_gen, v)
    ll, g = out(torch, (G_S,)), out(torch, (G_S, 3))

    def check(outs, host):
        R = range(G_S)
        assert_bits(outs[0], np.array([oracle.garch_loglik(x[s], om[s], al[s], be[s]) for s in R]), "loglik")
        assert_bits(outs[1], np.array([oracle.garch_gradient(x[s], om[s], al[s], be[s]) for s in R]), "gradient")
    return Case([ins[0], ins[7]], [ll, g], lambda st: L().sts_garch_loglik_gradient(vp(ins[0].buf), G_S, G_T, G_T,
                                                                                   vp(ins[7].buf), vp(ll), vp(g), st), check)


def _garch_effect(name, orc, ar):
    @row(name[4:], name)
    def _b(torch, v):
        ins, (x, _, c, phi, om, al, be, _) = gins(torch, _garch_gen, v)
        o = out(torch, (G_S, G_T))
        par = ((c, phi) if ar else ()) + (om, al, be)
        used = [ins[0]] + ins[(2 if ar else 4):7]
        ref = np.array([orc(x[s], *[a[s] for a in par]) for s in range(G_S)])
        return Case(used, [o], lambda st: getattr(L(), name)(vp(ins[0].buf), vp(o), G_S, G_T, G_T, G_T,
                                                             *[vp(g.buf) for g in used[1:]], st),
                    lambda outs, host: assert_bits(outs[0], ref, name))


_garch_effect("sts_garch_remove", oracle.garch_remove, False)
_garch_effect("sts_garch_add", oracle.garch_add, False)
_garch_effect("sts_argarch_remove", oracle.argarch_remove, True)
_garch_effect("sts_argarch_add", oracle.argarch_add, True)


# ---------------- AR fits: p = 5 on a panel whose price-level rows go to the QR refit ----------------
AR_S, AR_T, AR_P = 12, 400, 5


def _ar_gen(k):
    from test_ar_price_levels import walk
    x = oracle.gen_ar_panel(33 + k, AR_S, AR_T, AR_P)
    step = 3 if k < 50 else 2               # the decoys hold six price-level rows, the real panels four:
    x[::step] = walk(1e6, 1e-2, x[::step].shape[0], AR_T, 5 + k)    # a wrong order gives another rule count
    return [x]


def _check_ar(x, gc, gcoef):
    from test_ar_price_levels import ELEM_TOL, elementwise
    for s in range(AR_S):
        rc, rcoef = oracle.ar_fit(x[s], AR_P)
        assert elementwise(np.r_[gc[s], gcoef[s]], np.r_[rc, rcoef]) <= ELEM_TOL, s


@row("ar_fit", "sts_ar_fit")
def _b(torch, v):
    ins, (x,) = gins(torch, _ar_gen, v)
    c, coef, e = out(torch, (AR_S,)), out(torch, (AR_S, AR_P)), i32(torch, AR_S)

    def check(outs, host):
        assert (outs[2] == 0).all()
        _check_ar(x, outs[0], outs[1])
    return Case(ins, [c, coef, e], lambda st: L().sts_ar_fit(vp(ins[0].buf), AR_S, AR_T, AR_T, AR_P, 0, vp(c), vp(coef),
                                                             vp(e), st), check)


@row("ar_fit_remove", "sts_ar_fit_remove")
def _b(torch, v):
    ins, (x,) = gins(torch, _ar_gen, v)
    o, c, coef, e = out(torch, (AR_S, AR_T)), out(torch, (AR_S,)), out(torch, (AR_S, AR_P)), i32(torch, AR_S)

    def check(outs, host):
        assert (outs[3] == 0).all()
        _check_ar(x, outs[1], outs[2])
        assert_bits(outs[0], np.array([oracle.ar_remove(x[s], outs[1][s], outs[2][s]) for s in range(AR_S)]), "residuals")
    return Case(ins, [o, c, coef, e], lambda st: L().sts_ar_fit_remove(vp(ins[0].buf), vp(o), AR_S, AR_T, AR_T, AR_T, AR_P,
                                                                      0, vp(c), vp(coef), vp(e), st), check)


@row("ar_rule_count", "sts_ar_rule_count",
     sync="'HIP_TRY(hipStreamSynchronize(st), name);' before '*count = (int64_t)h;' (sts.h: synchronous)")
def _b(torch, v):
    ins, (x,) = gins(torch, _ar_gen, v)

    def call(st):
        n = ctypes.c_int64(-1)
        r = L().sts_ar_rule_count(vp(ins[0].buf), AR_S, AR_T, AR_T, AR_P, 0, ctypes.addressof(n), st)
        case.host.append(n.value)
        return r

    def check(outs, host):
        # the four price-level rows are flagged (test_gpu_ar_rule_flagged_series_are_the_reference_bits),
        # the AR(5) rows are not (test_gpu_ar_rule_is_quiet_on_c4_panels): the decoys would give six
        print("ar_rule_count:", host[0])
        assert host[0] == 4, host
    case = Case(ins, [], call, check)
    return case


# ---------------- ARIMA (1,1,1) and (2,2,1); the AR-only path ----------------
AM_S, AM_T = 6, 120


def _arima_gen(p, d, q):
    def gen(k):
        from test_arima import arma_panel, random_coef, starts
        x = arma_panel(300 + 13 * k + p, AM_S, AM_T, p, q, level=2.0, d=d)
        return [x, starts(p, d, q, x), random_coef(91 + k, AM_S, p, q) * 0.8]
    return memo(("arima_gen", p, d, q), lambda: gen)


def _arima_rows(p, d, q):
    import arima_ref as ar
    tag = "%d%d%d" % (p, d, q)
    n = 1 + p + q
    gen = _arima_gen(p, d, q)
    R = range(AM_S)

    @row("arima_hr_init-" + tag, "sts_arima_hr_init")
    def _b(torch, v):
        ins, (x, _, _) = gins(torch, gen, v)
        init, e = out(torch, (AM_S, n)), i32(torch, AM_S)

        def check(outs, host):
            assert (outs[1] == 0).all()
            for s in R:
                y = ar.diffed(x[s], d)
                assert ar.scaled_condition(ar.hr_design(p, q, y, True)[1]) <= 1e4, s
                ref = ar.hannan_rissanen(p, q, y, True)
                assert np.abs(outs[0][s] - ref).max() / np.abs(ref).max() <= 1e-10, s
        return Case(ins[:1], [init, e], lambda st: L().sts_arima_hr_init(vp(ins[0].buf), AM_S, AM_T, AM_T, p, d, q, 1,
                                                                        vp(init), vp(e), st), check)

    @row("arima_fit_css-" + tag, "sts_arima_fit_css")
    def _b(torch, v):
        ins, (x, init, _) = gins(torch, gen, v)
        coef, e, ev = out(torch, (AM_S, n)), i32(torch, AM_S), i32(torch, AM_S)
        ref = memo(("fit_css", tag, v), lambda: [ar.fit_css_cgd(p, q, True, ar.diffed(x[s], d), init[s]) for s in R])

        def check(outs, host):
            for s in R:
                rst, rcoef, rev = ref[s]
                assert (int(outs[1][s]), int(outs[2][s])) == (rst, rev), s
                if rst == ar.OK:
                    assert_bits(outs[0][s], np.asarray(rcoef), "fit_css row %d" % s)
                else:
                    assert np.isnan(outs[0][s]).all(), s
        return Case(ins[:2], [coef, e, ev], lambda st: L().sts_arima_fit_css(vp(ins[0].buf), AM_S, AM_T, AM_T, p, d, q, 1,
                                                                            vp(ins[1].buf), vp(coef), vp(e), vp(ev), st), check)

    @row("arima_css_loglik_gradient-" + tag, "sts_arima_css_loglik_gradient")
    def _b(torch, v):
        ins, (x, _, coef) = gins(torch, gen, v)
        ll, g = out(torch, (AM_S,)), out(torch, (AM_S, n))

        def check(outs, host):
            assert_bits(outs[0], np.array([ar.loglik_css(p, d, q, coef[s], True, x[s]) for s in R]), "loglik")
            assert_bits(outs[1], np.array([ar.gradient_css(p, d, q, coef[s], True, x[s]) for s in R]), "gradient")
        return Case([ins[0], ins[2]], [ll, g], lambda st: L().sts_arima_css_loglik_gradient(
            vp(ins[0].buf), AM_S, AM_T, AM_T, p, d, q, 1, vp(ins[2].buf), vp(ll), vp(g), st), check)

    for name, orc in (("sts_arima_remove", ar.remove_effects), ("sts_arima_add", ar.add_effects)):
        @row(name[4:] + "-" + tag, name)
        def _b(torch, v, name=name, orc=orc):
            ins, (x, _, coef) = gins(torch, gen, v)
            o = out(torch, (AM_S, AM_T))
            return Case([ins[0], ins[2]], [o], lambda st: getattr(L(), name)(vp(ins[0].buf), vp(o), AM_S, AM_T, AM_T, AM_T, p,
                                                                            d, q, 1, vp(ins[2].buf), st),
                        lambda outs, host: assert_bits(outs[0], np.array([orc(p, d, q, coef[s], True, x[s]) for s in R]), name))

    @row("arima_forecast-" + tag, "sts_arima_forecast")
    def _b(torch, v):
        nf = 7
        ins, (x, _, coef) = gins(torch, gen, v)
        o = out(torch, (AM_S, AM_T + nf))
        return Case([ins[0], ins[2]], [o], lambda st: L().sts_arima_forecast(vp(ins[0].buf), vp(o), AM_S, AM_T, AM_T, AM_T + nf,
                                                                            p, d, q, 1, vp(ins[2].buf), nf, st),
                    lambda outs, host: assert_bits(outs[0], np.array([ar.forecast(p, d, q, coef[s], True, x[s], nf) for s in R]),
                                                   "forecast"))


_arima_rows(1, 1, 1)
_arima_rows(2, 2, 1)


def _fit_ar_gen(k):
    from test_arima import arma_panel
    return [arma_panel(400 + k, AM_S, AM_T, 2, 0, level=1.0, d=1)]


@row("arima_fit_ar", "sts_arima_fit_ar")
def _b(torch, v):
    p, d = 2, 1
    ins, (x,) = gins(torch, _fit_ar_gen, v)
    c, coef, e = out(torch, (AM_S,)), out(torch, (AM_S, p)), i32(torch, AM_S)

    def check(outs, host):
        assert (outs[2] == 0).all()
        ref = [oracle.ar_fit(oracle.differences_of_order_d(r, d)[d:], p, no_intercept=False) for r in x]
        assert_rel(np.column_stack([outs[0], outs[1]]), np.array([[rc] + list(rf) for rc, rf in ref]), what="arima_fit_ar")
    return Case(ins[:1], [c, coef, e], lambda st: L().sts_arima_fit_ar(vp(ins[0].buf), AM_S, AM_T, AM_T, p, d, 1, vp(c),
                                                                      vp(coef), vp(e), st), check)


# ---------------- the six statistical tests ----------------
ST_S = 9


def _stat_gen(T):
    def gen(k):
        import bgbp_ref as br
        import stattests_ref as sref
        Fs, Fp = br.factors(5000 + k, T, 3, None), br.factors(5100 + k, T, 3, ST_S)
        from test_bgbp_gpu import factor_panel
        return [sref.ordinary_panel(1000 + k, ST_S, T), sref.ar1_panel(2000 + k, ST_S, T),
                br.bp_resid(6000 + k, ST_S, T, Fs), br.bp_resid(6100 + k, ST_S, T, Fp), br.bg_resid(7000 + k, ST_S, T),
                factor_panel(Fs)[0], factor_panel(Fp)[0]]
    return memo(("stat_gen", T), lambda: gen)


def _close(got, want, rtol, what):
    from test_stattests_gpu import assert_close
    assert_close(got, want, rtol, what)


@row("adf_test", "sts_adf_test")
def _b(torch, v):
    import stattests_ref as sref
    from test_stattests_gpu import check_adf_p
    T, lag = 129, 5
    ins, real = gins(torch, _stat_gen(T), v)
    stat, pv, e = out(torch, (ST_S,)), out(torch, (ST_S,)), i32(torch, ST_S)

    def check(outs, host):
        assert (outs[2] == 0).all()
        _close(outs[0], [sref.adf_stat(r, lag, "ct") for r in real[0]], 1e-10, "adf")
        check_adf_p(outs[0], outs[1], "ct")
    return Case(ins[:1], [stat, pv, e], lambda st: L().sts_adf_test(vp(ins[0].buf), ST_S, T, T, lag, 2, vp(stat), vp(pv),
                                                                   vp(e), st), check)


@row("kpss_test", "sts_kpss_test")
def _b(torch, v):
    import stattests_ref as sref
    T = 129
    ins, real = gins(torch, _stat_gen(T), v)
    stat = out(torch, (ST_S,))
    return Case(ins[:1], [stat], lambda st: L().sts_kpss_test(vp(ins[0].buf), ST_S, T, T, 2, vp(stat), st),
                lambda outs, host: _close(outs[0], [sref.kpss_stat(r, "ct") for r in real[0]], 1e-10, "kpss"))


@row("dw_test", "sts_dw_test")
def _b(torch, v):
    import stattests_ref as sref
    T = 129
    ins, real = gins(torch, _stat_gen(T), v)
    stat = out(torch, (ST_S,))
    return Case(ins[:1], [stat], lambda st: L().sts_dw_test(vp(ins[0].buf), ST_S, T, T, vp(stat), st),
                lambda outs, host: _close(outs[0], [sref.dw_stat(r) for r in real[0]], 1e-10, "dw"))


for _K in (20, 70):       # the fused ACF partials + finalize | the wide lag blocks, each into scratch
    @row("lb_test-K%d" % _K, "sts_lb_test")
    def _b(torch, v, K=_K):
        import stattests_ref as sref
        from test_stattests_gpu import check_lb_p
        T = 390
        ins, real = gins(torch, _stat_gen(T), v)
        stat, pv = out(torch, (ST_S,)), out(torch, (ST_S,))

        def check(outs, host):
            _close(outs[0], [sref.lb_stat(r, K) for r in real[1]], 2e-10, "lb")
            check_lb_p(outs[0], outs[1], K)
        return Case(ins[1:2], [stat, pv], lambda st: L().sts_lb_test(vp(ins[1].buf), ST_S, T, T, K, vp(stat), vp(pv), st), check)


for _kind in ("bp", "bg"):
    for _mode in ("shared", "per_series"):
        @row("%s_test-%s" % (_kind, _mode), "sts_%s_test" % _kind)
        def _b(torch, v, kind=_kind, per=(_mode == "per_series")):
            import bgbp_ref as br
            from test_bgbp_gpu import check_p
            T, k, lag = 129, 3, 4
            ins, real = gins(torch, _stat_gen(T), v)
            ie = 4 if kind == "bg" else (3 if per else 2)
            fi = 6 if per else 5
            fs = k * T if per else 0
            stat, pv, e = out(torch, (ST_S,)), out(torch, (ST_S,)), i32(torch, ST_S)

            def call(st):
                a = (vp(ins[ie].buf), ST_S, T, T, vp(ins[fi].buf), k, T, fs)
                if kind == "bg":
                    return L().sts_bg_test(*a, lag, vp(stat), vp(pv), vp(e), st)
                return L().sts_bp_test(*a, vp(stat), vp(pv), vp(e), st)

            def check(outs, host):
                assert (outs[2] == 0).all()
                F = real[fi]                       # (k, T) or (S, k, T)
                want = []
                for s, r in enumerate(real[ie]):
                    Fs = (F[s] if per else F).T
                    want.append(br.bg_stat(r, Fs, lag) if kind == "bg" else br.bp_stat(r, Fs))
                _close(outs[0], want, 1e-10, kind)
                check_p(outs[0], outs[1], lag if kind == "bg" else k)
            return Case([ins[ie], ins[fi]], [stat, pv, e], call, check)


# ---------------- instants: the NaN chain as one sequence, the transpose ----------------

def _inst_gen(S, T):
    def gen(k):
        rng = np.random.default_rng(S * 7 + T + 31 * k)
        x = rng.standard_normal((S, T))
        x[rng.random((S, T)) < 0.03] = NaN
        x[S - 1, T - 1] = NaN
        x[k % S, 2 + k % 3] = NaN                   # the decoys' flags differ from the real panel's
        x[:, 0] = 1.0
        return [x]
    return memo(("inst_gen", S, T), lambda: gen)


for _S, _T in ((6, 16), (5, 17)):                   # even: the 16-byte kernels; odd: the 8-byte ones
    @row("nan_instants_chain-%dx%d" % (_S, _T), "sts_nan_instants", "sts_active_instants", "sts_gather_instants")
    def _b(torch, v, S=_S, T=_T):
        ins, (x,) = gins(torch, _inst_gen(S, T), v)
        rg, ract = oracle.remove_instants_with_nans(x)
        n = ract.size
        # the flags are read-modify-write: zero (real) or all set (the decoys) before the call
        flags = GIn(torch, np.zeros(T), np.ones(T), np.ones(T), np.uint8)
        active, n_dev, o = out(torch, (T,), torch.int64), out(torch, (1,), torch.int64), out(torch, (S, max(n, 1)))

        def call(st):
            r = L().sts_nan_instants(vp(ins[0].buf), S, T, T, vp(flags.buf), st)
            r = r or L().sts_active_instants(vp(flags.buf), T, vp(active), vp(n_dev), st)
            return r or L().sts_gather_instants(vp(ins[0].buf), vp(o), S, T, max(n, 1), vp(active), n, st)

        def check(outs, host):
            assert np.array_equal(outs[0], np.isnan(x).any(axis=0).astype(np.uint8))
            assert int(outs[2][0]) == n and np.array_equal(outs[1][:n], ract)
            assert_bits(outs[3][:, :n], rg, "gather_instants")
        return Case(ins + [flags], [flags.buf, active, n_dev, o], call, check)

    @row("to_instants-%dx%d" % (_S, _T), "sts_to_instants")
    def _b(torch, v, S=_S, T=_T):
        ins, (x,) = gins(torch, _inst_gen(S, T), v)
        o = out(torch, (T, S))
        return Case(ins, [o], lambda st: L().sts_to_instants(vp(ins[0].buf), vp(o), S, T, T, S, st),
                    lambda outs, host: assert_bits(outs[0], oracle.to_instants(x), "to_instants"))


# ---------------- ingest / egress, generators ----------------
W_S = 5


def _wire(T, aligned, k):
    def make():
        from sparkts import io as sio
        rng = np.random.default_rng(31 + T + 17 * k)
        keys = ["k%07d" % i for i in range(W_S)] if aligned else ["k%d" % i + "x" * (i % 3 + 1) for i in range(W_S)]
        x = rng.standard_normal((W_S, T)) * 1e3
        x.ravel()[rng.random(W_S * T) < 0.05] = NaN
        x[0, 0] = -0.0
        data = oracle.wire_records(keys, x)
        _, T2, val_off = sio.wire_scan(data)
        assert T2 == T and np.all((np.asarray(val_off) % 8 == 0) == aligned)
        return x, np.frombuffer(data, dtype=np.uint8).copy(), np.asarray(val_off, dtype=np.int64)
    return memo(("wire", T, aligned, k), make)


for _T, _al in ((390, True), (4097, False)):        # one wave per record | the per-series grid, byte loads
    @row("wire_decode-T%d" % _T, "sts_wire_decode")
    def _b(torch, v, T=_T, al=_al):
        (x, data, off), (_, d1, _), (_, d2, _) = (_wire(T, al, k) for k in (v, 50 + v, 90 + v))
        raw = GIn(torch, data, d1, d2, np.uint8)    # 16-byte aligned allocation: val_off decides the load form
        offd, o = sg.dev(torch, off, np.int64), out(torch, (W_S, T))
        return Case([raw], [o], lambda st: L().sts_wire_decode(vp(raw.buf), vp(offd), W_S, T, vp(o), T, st),
                    lambda outs, host: assert_bits(outs[0], x, "wire_decode"))

    @row("wire_encode-T%d" % _T, "sts_wire_encode")
    def _b(torch, v, T=_T, al=_al):
        (x, data, off), (x1, _, _), (x2, _, _) = (_wire(T, al, k) for k in (v, 50 + v, 90 + v))
        panel = GIn(torch, x, x1, x2)
        offd, raw = sg.dev(torch, off, np.int64), out(torch, (data.size,), torch.uint8)

        def check(outs, host):
            want = np.full(data.size, 0xA5, np.uint8)          # headers are the caller's: untouched
            for o in off:
                want[o:o + 8 * T] = data[o:o + 8 * T]
            assert np.array_equal(outs[0], want), "wire_encode"
        return Case([panel], [raw], lambda st: L().sts_wire_encode(vp(panel.buf), W_S, T, T, vp(offd), vp(raw), st), check)


def _obs_gen(k):
    S, T, n = 5, 37, 600
    rng = np.random.default_rng(8 + k)
    loc = rng.integers(-3, T, n).astype(np.int64)
    loc[loc < 0] = -1
    return [rng.integers(0, S, n).astype(np.int32), loc, rng.standard_normal(n)]


@row("observations_to_panel", "sts_observations_to_panel")
def _b(torch, v):
    S, T, n = 5, 37, 600
    ins, (sid, loc, val) = gins(torch, _obs_gen, v, [np.int32, np.int64, np.float64])
    ref = np.full((S, T), NaN)
    for i in range(n):
        if loc[i] >= 0:
            ref[sid[i], loc[i]] = val[i]
    o = out(torch, (S, T))
    return Case(ins, [o], lambda st: L().sts_observations_to_panel(vp(ins[0].buf), vp(ins[1].buf), vp(ins[2].buf), n, vp(o),
                                                                  S, T, T, st),
                lambda outs, host: assert_bits(outs[0], ref, "observations"))


@row("gen_panel", "sts_gen_panel")
def _b(torch, v):
    S, T, s0 = 5, 1001, 3
    o = out(torch, (S, T))
    return Case([], [o], lambda st: L().sts_gen_panel(vp(o), s0, S, T, T, 123 + v, 0.3, st),
                lambda outs, host: assert_bits(outs[0], oracle.gen_panel(123 + v, S, T, 0.3, s0=s0), "gen_panel"))


@row("gen_ar_panel", "sts_gen_ar_panel")
def _b(torch, v):
    S, T, s0, p = 5, 1001, 3, 5
    o, c, phi = out(torch, (S, T)), out(torch, (S,)), out(torch, (S, p))
    return Case([], [o, c, phi], lambda st: L().sts_gen_ar_panel(vp(o), vp(c), vp(phi), s0, S, T, T, 77 + v, p, st),
                lambda outs, host: assert_bits(outs[0], oracle.gen_ar_panel(77 + v, S, T, p, s0=s0), "gen_ar_panel"))


IDS = [t[0] for t in TABLE]
SYNC = {t[0]: t[3] for t in TABLE if t[3] is not None}      # id -> why it synchronises by design
ASYNC = sorted({name for t in TABLE if t[3] is None for name in t[1]})


def build(ident, torch, v):
    case = next(t[2] for t in TABLE if t[0] == ident)(torch, v)
    case.sync = SYNC.get(ident)
    return case


COVERED = {name for t in TABLE for name in t[1]} | {"sts_stream_synchronize"}   # its own test below


# ---------------- the tests ----------------

def to_np(ts):
    return [t.cpu().numpy() for t in ts]


def run_plain(torch, case, what):
    st, res, host = sg.plain(torch, case)
    assert st == case.status, (what, st, L().sts_last_error())
    case.check(to_np(res), host)
    return res, host


def assert_ticket(torch, t, res, host, what):
    late = sg.finish(torch, t)
    assert t.status == t.case.status, (what, t.status, L().sts_last_error())
    assert t.host == host, (what, t.host, host)
    for i, (s, r) in enumerate(zip(t.snaps, res)):
        assert sg.same_bits(s, r), "%s: output %d of the gated call differs from the plain call" % (what, i)
    assert not late, "%s: outputs %s were written after the snapshot" % (what, late)


@pytest.mark.parametrize("ident", IDS)
def test_gated_call_is_stream_ordered(torch, delay, ident):
    case = build(ident, torch, 0)
    res, host = run_plain(torch, case, ident)
    t = sg.enqueue(torch, case, torch.cuda.Stream(), delay)
    pending = t.pending_at_return
    assert_ticket(torch, t, res, host, ident)
    print("%s: returned %s the gate opened" % (ident, "before" if pending else "after"))
    if case.sync is None:
        assert pending, "%s is expected to be asynchronous but returned after the delay had run out" % ident


@pytest.mark.parametrize("ident", IDS)
def test_two_streams(torch, delay, ident):
    a, b = build(ident, torch, 0), build(ident, torch, 1)
    ra, ha = run_plain(torch, a, ident + " [a]")
    rb, hb = run_plain(torch, b, ident + " [b]")
    ta = sg.enqueue(torch, a, torch.cuda.Stream(), delay)
    tb = sg.enqueue(torch, b, torch.cuda.Stream(), delay)
    assert_ticket(torch, ta, ra, ha, ident + " [a]")
    assert_ticket(torch, tb, rb, hb, ident + " [b]")


def test_stream_synchronize(torch, delay):
    """after sts_stream_synchronize(st) returns, a gated call's work on st is complete"""
    case = build("series_stats", torch, 0)
    res, host = run_plain(torch, case, "series_stats")
    case.preset("decoy")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ev, done = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(st):
        torch.cuda._sleep(delay)
        ev.record(st)
        case.ins[0].buf.copy_(case.ins[0].real, non_blocking=True)
        assert case.call(ctypes.c_void_p(st.cuda_stream)) == 0
        done.record(st)
        assert not ev.query(), "the call was expected to return before the gate opened"
        assert L().sts_stream_synchronize(ctypes.c_void_p(st.cuda_stream)) == 0
        assert ev.query() and done.query(), "sts_stream_synchronize returned before the stream's work was complete"
    assert sg.same_bits(case.outs[0], res[0])
    torch.cuda.synchronize()


def test_error_status_through_the_gate(torch, delay):
    """fill nearest, err_per_series == NULL: the all-NaN series arrives only through the gate (the
    decoys have none), and the call must return STS_ERR_ALL_NAN -- the synchronise-then-report
    path with the mapped error sink."""
    S, T = 5, 390
    real = oracle.gen_panel(100, S, T, 0.05)
    real[3, :] = NaN
    g = GIn(torch, real, oracle.gen_panel(150, S, T, 0.05), oracle.gen_panel(190, S, T, 0.05))
    o = out(torch, (S, T))
    ref, rerr = oracle.panel_fill(real, "nearest")
    assert rerr[3] == ALL_NAN and (np.delete(rerr, 3) == 0).all()

    def check(outs, host):
        assert_bits(np.delete(outs[0], 3, axis=0), np.delete(ref, 3, axis=0), "fill nearest")
    case = Case([g], [o], lambda st: L().sts_fill(vp(g.buf), vp(o), S, T, T, T, 1, None, st), check, sync=SYNC_NULL_ERR,
                status=ALL_NAN)
    res, host = run_plain(torch, case, "fill nearest, NULL err")
    assert b"all NaNs" in L().sts_last_error()
    t = sg.enqueue(torch, case, torch.cuda.Stream(), delay)
    assert not t.pending_at_return, "a call that reports a per-series status must have waited for its work"
    assert_ticket(torch, t, res, host, "fill nearest, NULL err")


# ---------------- the Python mirror ----------------

def _mirror_panel(k):
    x = oracle.gen_panel(500 + k, 12, 390, 0.05)
    x[:, :2] = oracle.gen_panel(600 + k, 12, 2, 0.0)          # a valid start for every fill
    return x


def _mirror_clean(k):
    return oracle.gen_ar_panel(700 + k, 12, 390, 3) + 0.01 * np.sin(np.arange(390))[None, :]


def _m_fill_acf(torch, x, aux):
    from sparkts.timeseriesrdd import TimeSeriesRDD
    f, acf = TimeSeriesRDD(None, None, x).fillAndAutocorr("linear", 20)
    return [f.data, acf]


def _m_stats(torch, x, aux):
    from sparkts.timeseriesrdd import TimeSeriesRDD
    return [TimeSeriesRDD(None, None, x).seriesStats().stats]


def _m_remove_instants(torch, x, aux):
    from sparkts.timeseriesrdd import TimeSeriesRDD
    r = TimeSeriesRDD(None, None, x).removeInstantsWithNaNs()
    return [r.data, torch.as_tensor(np.asarray(r.index))]


def _m_ar(torch, x, aux):
    from sparkts.models import Autoregression
    m, resid = Autoregression.fitModelAndRemove(x, 3)
    return [m.c, m.coefficients, resid]


def _m_ewma(torch, x, aux):
    from sparkts.models import EWMA
    return [EWMA.fitModel(x, errors=torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)).smoothing]


def _m_arima(torch, x, aux):
    from sparkts.models.ARIMA import ARIMA
    m = ARIMA.fitModelCSS(1, 1, 1, x, errors=torch.zeros(x.shape[0], dtype=torch.int32, device=x.device))
    return [m.coefficients, m.evaluations]


def _m_lb(torch, x, aux):
    from sparkts.timeseriesrdd import TimeSeriesRDD
    return list(TimeSeriesRDD(None, None, x).lbtest(20))


def _m_bg(torch, x, aux):
    from sparkts.timeseriesrdd import TimeSeriesRDD
    return list(TimeSeriesRDD(None, None, x).bgtest(aux, 4))      # aux: the factors, on the device before the gate


def _bg_factors(torch):
    import bgbp_ref as br
    return sg.dev(torch, br.factors(5000, 390, 3, None))


def _m_wire(torch, x, aux):
    from sparkts import io as sio
    from sparkts.timeseriesrdd import TimeSeriesRDD
    return [torch.frombuffer(bytearray(sio.toWire(TimeSeriesRDD(None, ["k%d" % i for i in range(x.shape[0])], x))),
                             dtype=torch.uint8)]


def _sparse_nans(k):
    x = _mirror_clean(k)
    x[k % 12, 5 + k % 7] = NaN
    x[3, 200] = NaN
    return x


# name -> (fn, panel generator, what is put on the device before the gate, host behaviour):
#   "async"   the mirror call returns without waiting: the event after the delay must still be
#             pending when it has returned (the case was not vacuous);
#   "waits"   the mirror waits for the device by design, in the library (err_per_series NULL) or for a
#             host value (n_active), after its first library call was queued behind the shut gate;
#   "chain"   two library calls with stream-ordered scratch, one after the other on one stream
#             (ARIMA.fitModelCSS: sts_arima_hr_init, then sts_arima_fit_css).  Each is asynchronous
#             alone (its ABI row says so), and the first returns with the gate shut; in the second,
#             the runtime's hipMallocAsync waits on the host for the first call's still pending
#             hipFreeAsync (measured: 0.05 ms for the first call, 20 ms -- the delay -- for the
#             second).  The work was queued behind the shut gate all the same;
#   "opens"   the mirror itself waits for the stream BEFORE its library call (io.toWire uploads
#             val_off from pageable memory, which torch synchronises): the gate is open by the time
#             sts_wire_encode is queued, so the case holds toWire to the plain call's bytes but cannot
#             see the order against the producer.  It is not counted as evidence for the
#             default-stream property.
MIRROR = {
    "fillAndAutocorr": (_m_fill_acf, _mirror_panel, None, "waits"),
    "seriesStats": (_m_stats, _mirror_panel, None, "async"),
    "removeInstantsWithNaNs": (_m_remove_instants, _sparse_nans, None, "waits"),
    "fitModelAndRemove": (_m_ar, _mirror_clean, None, "waits"),
    "EWMA.fitModel": (_m_ewma, _mirror_clean, None, "async"),
    "ARIMA.fitModelCSS": (_m_arima, lambda k: _mirror_clean(k)[:, :120].cumsum(axis=1), None, "chain"),
    "lbtest": (_m_lb, _mirror_clean, None, "async"),
    "bgtest": (_m_bg, _mirror_clean, _bg_factors, "waits"),
    "toWire": (_m_wire, _mirror_panel, None, "opens"),
}


def _host(ts):
    return [t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t) for t in ts]


def _mirror_oracle(name, x, got):
    """the cheap oracle bars of the plain mirror result (the ABI rows above hold the others)"""
    if name == "fillAndAutocorr":
        rf, racf, _ = oracle.panel_fill_autocorr(x, "linear", 20)
        assert_bits(got[0], rf, "filled")
        assert_rel(got[1], racf, what="acf")
    elif name == "seriesStats":
        assert_bits(got[0], np.array([oracle.stat_counter(r)[1:] for r in x]), "seriesStats")
    elif name == "removeInstantsWithNaNs":
        rg, ract = oracle.remove_instants_with_nans(x)
        assert_bits(got[0], rg, "removeInstantsWithNaNs")
        assert np.array_equal(got[1], ract)
    elif name == "toWire":
        assert bytes(got[0]) == oracle.wire_records(["k%d" % i for i in range(x.shape[0])], x)


@pytest.mark.parametrize("where", ["side_stream", "default_stream"])
@pytest.mark.parametrize("name", sorted(MIRROR))
def test_mirror(torch, delay, name, where):
    """The gate around a mirror call, results read with .cpu() on the same torch stream.
    default_stream: delay, copy, call and reads all on torch's default stream -- the mirror then
    passes handle 0 (hipStreamPerThread) while torch works on the legacy null stream, and the
    result shows whether HIP ordered the two (include/sts.h "Stream contract", sparkts/_panel.py).
    The event after the delay is still pending when the mirror call starts and, for the "async"
    pipelines, when it has returned: the library's work was queued behind a shut gate (MIRROR says
    why each of the others waits)."""
    fn, gen, prep, host = MIRROR[name]
    g = GIn(torch, gen(0), gen(50), gen(90))
    aux = prep(torch) if prep else None
    g.buf.copy_(g.real)
    torch.cuda.synchronize()
    want = _host(fn(torch, g.buf, aux))
    torch.cuda.synchronize()
    _mirror_oracle(name, g.real.cpu().numpy(), want)
    g.buf.copy_(g.decoy)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if where == "side_stream" else torch.cuda.default_stream()
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(delay)
        ev.record(stream)
        g.buf.copy_(g.real, non_blocking=True)
        shut_before = not ev.query()
        res = fn(torch, g.buf, aux)
        shut_after = not ev.query()
        g.buf.copy_(g.decoy2, non_blocking=True)
        got = _host(res)
    stream.synchronize()
    torch.cuda.synchronize()
    print("%s on the %s: gate shut before the call %s, after it returned %s" % (name, where, shut_before, shut_after))
    assert shut_before, "the host reached the mirror call only after the delay had run out"
    if host == "async":
        assert shut_after, "%s is expected to return without waiting for the device" % name
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s on the %s: result %d differs from the plain call" % (
            name, where, i)
