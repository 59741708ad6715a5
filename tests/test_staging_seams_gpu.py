"""Every chunked `_host` entry point across the staging pipeline's chunk seams
(spark-timeseries_amd/csrc/sts_host.cpp).  Needs an MI355X.

tests/staging_plan.py restates what staged() decides and holds one row per wrapper; the shapes it
gives (proved in tests/test_staging_plan_cpu.py) have at least three chunks with a partial last one
and an odd number of series per chunk, so every per-series offset (s0 * hstride, factor blocks at fs,
roll_pair's y at its own ld_y), every shared upload, the stride-0 zero row, packed outputs, NULL
outputs and in-place sharing run for a second and a third chunk, and the chunk's kernels see series
paired differently from a whole-panel launch.

One case = one row x one variant x {pageable, pinned (sts_host_alloc)} (+ inputs pinned / outputs
pageable on three rows).  Host panels have ld = T + 3 inside poisoned arenas (tests/layout_arena.py),
per-series factors ld_f = T + 3 and fs = span + 5, roll_pair's y has ld_y = T + 5.  Each case asserts

  1. status 0 and sts_staging_stats() chunks == the plan's nchunks (the seam was really crossed);
  2. H2D / D2H bytes == the plan's, direct == the pinned share (0 pageable, > 0.99 pinned);
  3. every output, err included, equals BIT FOR BIT the same device entry point called once on the
     whole panel in HBM (packed ld = T, NULL stream, the same vectors and factors uploaded whole);
  4. the series on both sides of every seam (staging_plan.seam_series) meet the CPU reference of the
     operation at the bar and with the helper of the operation's own GPU test file;
  5. inputs unchanged, nothing outside an output's own elements written.

Statuses across chunks, one series larger than a chunk, and the Python mirror follow the table.
"""
import functools
import re
import types

import numpy as np
import pytest

import bgbp_ref as br
import factor_ols_ref as fr
import index_ref as ir
import layout_arena as la
import oracle
import roll_ref as rr
import staging_plan as sp
import stattests_ref as sr
import transforms_ref as tr
from test_acf_robust import noise_floor, within
from test_bgbp_gpu import assert_close, check_p
from test_layout_gpu import RTOL, HostArenas, _ar_remove_in_place, _dest_is_ts, assert_bits, assert_rel
from test_stattests_gpu import check_adf_p, check_lb_p

pytestmark = pytest.mark.gpu

METHODS = {"none": -1, "linear": 0, "nearest": 1, "next": 2, "previous": 3, "spline": 4}
REG = {"nc": 0, "c": 1, "ct": 2, "ctt": 3}
ROLL_OPS = ("sum", "mean", "var", "std", "min", "max", "zscore")
ROLL_PAIR_OPS = ("cov", "corr", "beta")
NP_DTYPE = {"f8": np.float64, "i8": np.int64, "i4": np.int32}
STAT_KEYS = ["wall_ms", "h2d_ms", "kernel_ms", "d2h_ms", "h2d_bytes", "d2h_bytes", "chunks", "direct"]


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    # a library built with another STS_STAGE_MB / STS_STAGE_SLOTS would no longer cross the seams the plan proves
    assert pool_info()[7] == sp.SLOTS * (sp.CHUNK + 16 * 256) == sp.POOL_KEEP
    return _t


def lib():
    from sparkts import _native
    return _native.lib()


def P(a):
    return a.ctypes.data


def stats():
    s = np.zeros(8)
    assert lib().sts_staging_stats(P(s)) == 0
    return dict(zip(STAT_KEYS, s))


def pool_info():
    v = np.zeros(8, dtype=np.int64)
    assert lib().sts_staging_pool_info(P(v)) == 0
    return v


def last_error():
    m = lib().sts_last_error()
    return m.decode() if m else ""


def same_bits(a, b):
    """uint64 views equal, NaN equal to NaN (integers: equal)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a, b))
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def first_diff(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        bad = ~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))
    else:
        bad = a != b
    i = np.argwhere(bad)
    return "%d differ, first at %s: %r != %r" % (len(i), i[0].tolist(), a[tuple(i[0])], b[tuple(i[0])])


# ---------------- inputs: one cached base panel, every series distinct ----------------

S_MAX = max(r.plan(v).S for r, v in sp.CASES + sp.STATUS_CASES)
T_MAX = 396


@functools.lru_cache(maxsize=None)
def base():
    rng = np.random.default_rng(20150410)
    z = rng.standard_normal((S_MAX, T_MAX))
    nan = rng.integers(0, 256, (S_MAX, T_MAX), dtype=np.uint8) < 13        # about 5 %
    nan[:, :2] = False          # x[0], x[1] valid: every fill method leaves a series it can fill
    z.setflags(write=False)
    nan.setflags(write=False)
    return z, nan


def level(S):
    s = np.arange(S, dtype=np.float64)
    return (s % 977.0) * 0.001 + (s % 13.0) * 0.1          # a per-row level


def frac(S, w, mult, lo, hi):
    """(S, w) distinct values in [lo, hi): a Weyl sequence over the series"""
    i = np.arange(S * w, dtype=np.float64).reshape(S, w) + 1.0
    return lo + (hi - lo) * ((i * mult) % 1.0)


@functools.lru_cache(maxsize=2)
def panel(kind, S, T):
    z, nan = base()
    z, nan = z[:S, :T], nan[:S, :T]
    if kind in ("noise", "nan"):
        x = z + level(S)[:, None]
    elif kind in ("price", "price-nan"):
        x = 100.0 + z + level(S)[:, None]
    elif kind == "ar":
        x = oracle.gen_ar_panel(7, S, T, 3) + 0.01 * np.sin(np.arange(T))[None, :]
    elif kind == "garch":
        om = 0.1 + 0.02 * (np.arange(S) % 5)
        al = 0.1 + 0.05 * (np.arange(S) % 4)
        be = 0.3 + 0.05 * (np.arange(S) % 3)
        x = np.empty((S, T))
        h = om / (1.0 - al - be)
        e = np.zeros(S)
        for t in range(T):
            h = om + al * e * e + be * h
            e = np.sqrt(h) * z[:, t]
            x[:, t] = e
    elif kind == "edges":
        x = z + level(S)[:, None]
        s = np.arange(S)
        t = np.arange(T)[None, :]
        x[t < (s % 7)[:, None]] = np.nan
        x[t >= T - (s % 5)[:, None]] = np.nan
        x[s % 101 == 50] = np.nan
        x[nan] = np.nan
    else:
        raise KeyError(kind)
    if kind in ("nan", "price-nan"):
        x = np.where(nan, np.nan, x)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def factors(S, T, k, shared):
    """(T, k) shared or (S, T, k) per series, every value distinct"""
    rng = np.random.default_rng(77 + k + (0 if shared else S))
    return rng.standard_normal((T, k)) if shared else rng.standard_normal((S, T, k))


def rebase_map(T_in, T_out):
    m = (np.arange(T_out, dtype=np.int64) * 7 + 3) % (T_in + 9) - 4       # absent entries on both sides
    m[5:9] = m[4]                                                          # repeats
    m[-1] = -1
    return m


# ---------------- the calls: host form and device twin of every row ----------------

def _pair(host, dev):
    return lambda L, a, p, h: host(L, a, p) if h else dev(L, a, p)


def _panels(name, tail=lambda a, p: ()):
    """in, out panels then a tail of scalars / vectors; the device twin takes ld_in, ld_out and a stream"""
    return lambda L, a, p, h: (getattr(L, name + "_host")(a["in"], a["out"], p.S, p.T, p.ld, *tail(a, p)) if h else
                               getattr(L, name)(a["in"], a["out"], p.S, p.T, p.ld, p.ld, *(tuple(tail(a, p)) + (None,))))


def _fit(name, outs, head=lambda p: (), err=True):
    """input panel, scalars, outputs (err last)"""
    def call(L, a, p, h):
        args = (a["in"], p.S, p.T, p.ld) + tuple(head(p)) + tuple(a[o] for o in outs) + ((a["err"],) if err else ())
        return getattr(L, name + "_host")(*args) if h else getattr(L, name)(*(args + (None,)))
    return call


def _fac(p):
    return (p.k, p.ld_f, p.fs)


CALLS = {
    "sts_fill_host": _pair(lambda L, a, p: L.sts_fill_host(a["in"], a["out"], p.S, p.T, p.ld, p.method, a["err"]),
                           lambda L, a, p: L.sts_fill(a["in"], a["out"], p.S, p.T, p.ld, p.ld, p.method, a["err"], None)),
    "sts_autocorr_host": _pair(lambda L, a, p: L.sts_autocorr_host(a["in"], p.S, p.T, p.ld, p.K, a["acf"]),
                               lambda L, a, p: L.sts_fill_autocorr(a["in"], None, p.S, p.T, p.ld, p.ld, -1, p.K, a["acf"],
                                                                   a["err"], None)),
    "sts_fill_autocorr_host": _pair(
        lambda L, a, p: L.sts_fill_autocorr_host(a["in"], a["filled"], p.S, p.T, p.ld, p.method, p.K, a["acf"], a["err"]),
        lambda L, a, p: L.sts_fill_autocorr(a["in"], a["filled"], p.S, p.T, p.ld, p.ld, p.method, p.K, a["acf"], a["err"], None)),
    "sts_diff_at_lag_host": _panels("sts_diff_at_lag", lambda a, p: (p.lag, p.start)),
    "sts_lag_matrix_host": _pair(lambda L, a, p: L.sts_lag_matrix_host(a["in"], a["out"], p.S, p.T, p.ld, p.max_lag, p.inc),
                                 lambda L, a, p: L.sts_lag_matrix(a["in"], a["out"], p.S, p.T, p.ld, p.max_lag, p.inc, None)),
    "sts_ewma_add_host": _panels("sts_ewma_add", lambda a, p: (a["smoothing"],)),
    "sts_ewma_remove_host": _panels("sts_ewma_remove", lambda a, p: (a["smoothing"],)),
    "sts_fill_diff_ewma_host": _panels("sts_fill_diff_ewma", lambda a, p: (p.method, p.lag, a["smoothing"], a["err"])),
    "sts_ewma_fit_host": _fit("sts_ewma_fit", ("smoothing",)),
    "sts_ar_fit_host": _fit("sts_ar_fit", ("c", "coef"), lambda p: (p.p, p.no_intercept)),
    "sts_ar_fit_remove_host": _panels("sts_ar_fit_remove", lambda a, p: (p.p, p.no_intercept, a["c"], a["coef"], a["err"])),
    "sts_garch_fit_host": _fit("sts_garch_fit", ("params",)),
    "sts_argarch_fit_host": _fit("sts_argarch_fit", ("c", "phi", "params")),
    "sts_ar_remove_host": _panels("sts_ar_remove", lambda a, p: (a["c"], a["coef"], p.p)),
    "sts_ar_add_host": _panels("sts_ar_add", lambda a, p: (a["c"], a["coef"], p.p)),
    "sts_dw_test_host": _fit("sts_dw_test", ("stat",), err=False),
    "sts_kpss_test_host": _fit("sts_kpss_test", ("stat",), lambda p: (p.regression,), err=False),
    "sts_adf_test_host": _fit("sts_adf_test", ("stat", "pvalue"), lambda p: (p.max_lag, p.regression)),
    "sts_lb_test_host": _fit("sts_lb_test", ("stat", "pvalue"), lambda p: (p.max_lag,), err=False),
    "sts_bp_test_host": _pair(
        lambda L, a, p: L.sts_bp_test_host(a["resid"], p.S, p.T, p.ld, a["factors"], *_fac(p), a["stat"], a["pvalue"], a["err"]),
        lambda L, a, p: L.sts_bp_test(a["resid"], p.S, p.T, p.ld, a["factors"], *_fac(p), a["stat"], a["pvalue"], a["err"], None)),
    "sts_bg_test_host": _pair(
        lambda L, a, p: L.sts_bg_test_host(a["resid"], p.S, p.T, p.ld, a["factors"], *_fac(p), p.max_lag, a["stat"],
                                           a["pvalue"], a["err"]),
        lambda L, a, p: L.sts_bg_test(a["resid"], p.S, p.T, p.ld, a["factors"], *_fac(p), p.max_lag, a["stat"], a["pvalue"],
                                      a["err"], None)),
    "sts_factor_ols_host": _pair(
        lambda L, a, p: L.sts_factor_ols_host(a["y"], p.S, p.T, p.ld, a["factors"], *_fac(p), a["beta"], a["stderr"],
                                              a["stats"], a["resid"], a["err"]),
        lambda L, a, p: L.sts_factor_ols(a["y"], p.S, p.T, p.ld, a["factors"], *_fac(p), a["beta"], p.k + 1, a["stderr"],
                                         a["stats"], a["resid"], p.ld, a["err"], None)),
    "sts_factor_remove_host": _pair(
        lambda L, a, p: L.sts_factor_remove_host(a["in"], a["out"], p.S, p.T, p.ld, a["factors"], *_fac(p), a["beta"]),
        lambda L, a, p: L.sts_factor_remove(a["in"], a["out"], p.S, p.T, p.ld, p.ld, a["factors"], *_fac(p), a["beta"],
                                            p.k + 1, None)),
    "sts_factor_add_host": _pair(
        lambda L, a, p: L.sts_factor_add_host(a["in"], a["out"], p.S, p.T, p.ld, a["factors"], *_fac(p), a["beta"]),
        lambda L, a, p: L.sts_factor_add(a["in"], a["out"], p.S, p.T, p.ld, p.ld, a["factors"], *_fac(p), a["beta"],
                                         p.k + 1, None)),
    "sts_roll_stat_host": _panels("sts_roll_stat", lambda a, p: (p.window, p.min_periods, p.op)),
    "sts_roll_pair_host": _pair(
        lambda L, a, p: L.sts_roll_pair_host(a["in"], a["y"], p.Sy, p.ld_y, a["out"], p.S, p.T, p.ld, p.window,
                                             p.min_periods, p.op),
        lambda L, a, p: L.sts_roll_pair(a["in"], a["y"], p.Sy, p.ld_y, a["out"], p.S, p.T, p.ld, p.ld, p.window,
                                        p.min_periods, p.op, None)),
    "sts_quotients_host": _pair(
        lambda L, a, p: L.sts_quotients_host(a["in"], a["out"], p.S, p.T, p.ld, p.lag, p.minus_one),
        lambda L, a, p: L.sts_quotients(a["in"], a["out"], p.S, p.T, p.ld, p.T - p.lag, p.lag, p.minus_one, None)),
    "sts_fill_quotients_host": _pair(
        lambda L, a, p: L.sts_fill_quotients_host(a["in"], a["out"], p.S, p.T, p.ld, p.method, p.lag, p.minus_one, a["err"]),
        lambda L, a, p: L.sts_fill_quotients(a["in"], a["out"], p.S, p.T, p.ld, p.T - p.lag, p.method, p.lag, p.minus_one,
                                             a["err"], None)),
    "sts_fill_with_default_host": _panels("sts_fill_with_default", lambda a, p: (p.filler,)),
    "sts_downsample_host": _pair(
        lambda L, a, p: L.sts_downsample_host(a["in"], a["out"], p.S, p.T, p.ld, p.n, p.phase),
        lambda L, a, p: L.sts_downsample(a["in"], a["out"], p.S, p.T, p.ld, (p.T - p.phase + p.n - 1) // p.n, p.n, p.phase,
                                         None)),
    "sts_upsample_host": _pair(
        lambda L, a, p: L.sts_upsample_host(a["in"], a["out"], p.S, p.T, p.ld, p.n, p.phase, p.use_zero),
        lambda L, a, p: L.sts_upsample(a["in"], a["out"], p.S, p.T, p.ld, p.T * p.n, p.n, p.phase, p.use_zero, None)),
    "sts_first_last_not_nan_host": _fit("sts_first_last_not_nan", ("first", "last"), err=False),
    "sts_inverse_diff_at_lag_host": _panels("sts_inverse_diff_at_lag", lambda a, p: (p.lag, p.start)),
    "sts_diff_order_d_host": _panels("sts_diff_order_d", lambda a, p: (p.d,)),
    "sts_inverse_diff_order_d_host": _panels("sts_inverse_diff_order_d", lambda a, p: (p.d,)),
    "sts_rebase_shift_host": _pair(
        lambda L, a, p: L.sts_rebase_shift_host(a["in"], a["out"], p.S, p.T, p.T_out, p.ld, p.start_loc, p.default),
        lambda L, a, p: L.sts_rebase_shift(a["in"], a["out"], p.S, p.T, p.T_out, p.ld, p.T_out, p.start_loc, p.default, None)),
    "sts_rebase_map_host": _pair(
        lambda L, a, p: L.sts_rebase_map_host(a["in"], a["out"], p.S, p.T, p.T_out, p.ld, a["map"], p.default),
        lambda L, a, p: L.sts_rebase_map(a["in"], a["out"], p.S, p.T, p.T_out, p.ld, p.T_out, a["map"], p.default, None)),
}


# ---------------- the CPU references at the seam series ----------------
# ref(i, o, p): i = the inputs' seam rows (name -> array; shared inputs whole), o = the outputs' seam rows
# (None where the variant passes NULL), p = the parameters (names, not codes).  Index-driven and recurrence
# outputs bit for bit; reductions and fits at the bar of the operation's own GPU test file.

def rows_of(f, x, *vecs):
    return np.array([f(r, *[v[s] for v in vecs]) for s, r in enumerate(x)])


def r_fill(i, o, p):
    ref, err = oracle.panel_fill(i["in"], p["method"])
    assert_bits(o["out"], ref, "fill")
    assert np.array_equal(o["err"].ravel(), err)


def r_autocorr(i, o, p):
    for s, r in enumerate(i["in"]):
        assert within(o["acf"][s], oracle.autocorr(r, p["K"]), noise_floor(r, p["K"])) <= 1.0, s


def r_fill_autocorr(i, o, p):
    rf, racf, rerr = oracle.panel_fill_autocorr(i["in"], p["method"], p["K"])
    assert_bits(o["filled"], rf, "fill_autocorr filled")
    assert np.array_equal(o["err"].ravel(), rerr)
    for s in range(len(rf)):
        floor = noise_floor(rf[s], p["K"]) if not np.isnan(rf[s]).any() else np.zeros(p["K"])
        assert within(o["acf"][s], racf[s], floor) <= 1.0, s


def r_diff(i, o, p):
    if p["inplace"]:
        ref = rows_of(lambda r: oracle.differences_at_lag(r.copy(), p["lag"], start=p["start"], inplace=True), i["in"])
    else:
        ref = rows_of(lambda r: oracle.differences_at_lag(r, p["lag"], start=p["start"]), i["in"])
    assert_bits(o["out"], ref, "diff_at_lag")


def r_lag_matrix(i, o, p):
    ref = np.array([oracle.lag(r, p["max_lag"], bool(p["inc"])).T.ravel() for r in i["in"]])
    assert_bits(o["out"], ref, "lag_matrix")


def r_ewma(orc):
    def ref(i, o, p):
        sm = i["smoothing"].ravel()
        f = (lambda r, v: _dest_is_ts(orc, r, v)) if p["inplace"] else (lambda r, v: orc(r, v))
        assert_bits(o["out"], rows_of(f, i["in"], sm), orc.__name__)
    return ref


def r_fill_diff_ewma(i, o, p):
    def f(r, v):
        return oracle.ewma_add(oracle.differences_at_lag(oracle.fillts(r, p["method"]), p["lag"]), v)
    assert_bits(o["out"], rows_of(f, i["in"], i["smoothing"].ravel()), "fill_diff_ewma")
    assert (o["err"] == 0).all()


def r_ewma_fit(i, o, p):
    sm, err = oracle.panel_ewma_fit(i["in"])
    assert np.array_equal(o["err"].ravel(), err)
    assert_bits(o["smoothing"].ravel(), sm, "ewma_fit")


def r_ar_fit(i, o, p):
    x = i["in"]
    fits = [oracle.ar_fit(r, p["p"], bool(p["no_intercept"])) for r in x]
    assert (o["err"] == 0).all()
    assert_rel(o["coef"], np.array([f[1] for f in fits]), what="ar_fit coef")
    assert_rel(o["c"].ravel(), np.array([f[0] for f in fits]), what="ar_fit c")
    if "out" in o:
        assert_bits(o["out"], rows_of(oracle.ar_remove, x, o["c"].ravel(), o["coef"]), "ar_fit_remove residuals")


def r_garch_fit(i, o, p):
    par, err = oracle.panel_garch_fit(i["in"])
    assert np.array_equal(o["err"].ravel(), err)
    assert_bits(o["params"], par, "garch_fit")


def r_argarch_fit(i, o, p):
    x = i["in"]
    gc, gphi = o["c"].ravel(), o["phi"].ravel()
    fits = [oracle.ar_fit(r, 1, False) for r in x]
    assert np.allclose(gc, [f[0] for f in fits], rtol=RTOL, atol=0)
    assert np.allclose(gphi, [f[1][0] for f in fits], rtol=RTOL, atol=0)
    par, err = oracle.panel_garch_fit(np.array([oracle.ar_remove(x[s], gc[s], [gphi[s]]) for s in range(len(x))]))
    assert np.array_equal(o["err"].ravel(), err)
    assert_bits(o["params"], par, "argarch_fit")


def r_ar(add):
    def ref(i, o, p):
        c = i["c"].ravel()
        coef = i["coef"] if p["p"] > 0 else np.zeros((len(c), 0))
        if p["inplace"]:
            f = (lambda r, a, b: oracle.ar_add(r.copy(), a, b, inplace=True)) if add else _ar_remove_in_place
        else:
            f = oracle.ar_add if add else oracle.ar_remove
        assert_bits(o["out"], rows_of(f, i["in"], c, coef), "ar_add" if add else "ar_remove")
    return ref


def r_dw(i, o, p):
    assert_close(o["stat"].ravel(), [sr.dw_stat(r) for r in i["in"]], 1e-10, "dw")


def r_kpss(i, o, p):
    assert_close(o["stat"].ravel(), [sr.kpss_stat(r, p["regression"]) for r in i["in"]], 1e-10, "kpss")


def r_adf(i, o, p):
    stat = o["stat"].ravel()
    assert_close(stat, [sr.adf_stat(r, p["max_lag"], p["regression"]) for r in i["in"]], 1e-10, "adf")
    assert (o["err"] == 0).all()
    if o["pvalue"] is not None:
        check_adf_p(stat, o["pvalue"].ravel(), p["regression"])


def r_lb(i, o, p):
    stat = o["stat"].ravel()
    assert_close(stat, [sr.lb_stat(r, p["max_lag"]) for r in i["in"]], 2e-10, "lb")
    if o["pvalue"] is not None:
        check_lb_p(stat, o["pvalue"].ravel(), p["max_lag"])


def r_bgbp(bp):
    def ref(i, o, p):
        F = i["F"]
        want = [br.bp_stat(r, F if F.ndim == 2 else F[s]) if bp else br.bg_stat(r, F if F.ndim == 2 else F[s], p["max_lag"])
                for s, r in enumerate(i["resid"])]
        stat = o["stat"].ravel()
        assert_close(stat, want, 1e-10, "bp" if bp else "bg")
        assert (o["err"] == 0).all()
        if o["pvalue"] is not None:
            check_p(stat, o["pvalue"].ravel(), p["k"] if bp else p["max_lag"])
    return ref


def r_factor_ols(i, o, p):
    beta, se, st, resid = fr.ols_panel(i["y"], i["F"])
    assert fr.rel(o["beta"], beta) <= fr.BAR and fr.rel(o["stats"], st) <= fr.BAR
    if o["stderr"] is not None:
        assert fr.rel(o["stderr"], se) <= fr.BAR
    if o["resid"] is not None:
        assert fr.resid_err(o["resid"], resid) <= fr.BAR
    if o["err"] is not None:
        assert (o["err"] == 0).all()


def r_factor_effect(f):
    def ref(i, o, p):
        assert_bits(o["out"], f(i["in"], i["beta"], i["F"]), f.__name__)
    return ref


def r_roll_stat(i, o, p):
    assert rr.same_bits(o["out"], rr.stat(i["in"], p["op"], p["window"], p["min_periods"]))


def r_roll_pair(i, o, p):
    assert rr.same_bits(o["out"], rr.pair(i["in"], i["y"], p["op"], p["window"], p["min_periods"]))


def r_fill_quotients(i, o, p):
    filled, err = oracle.panel_fill(i["in"], p["method"])
    tr.assert_bits(o["out"], tr.quotients(filled, p["lag"], bool(p["minus_one"])), "fill_quotients")
    assert np.array_equal(o["err"].ravel(), err)


def r_first_last(i, o, p):
    assert np.array_equal(o["first"].ravel(), tr.first_not_nan(i["in"]))
    if o["last"] is not None:
        assert np.array_equal(o["last"].ravel(), tr.last_not_nan(i["in"]))


def r_inverse_diff(i, o, p):
    # in place gives the same bits (a history of outputs)
    tr.assert_bits(o["out"], tr.inverse_differences_at_lag(i["in"], p["lag"], p["start"]), "inverse_diff_at_lag")


REFS = {
    "sts_fill_host": r_fill,
    "sts_autocorr_host": r_autocorr,
    "sts_fill_autocorr_host": r_fill_autocorr,
    "sts_diff_at_lag_host": r_diff,
    "sts_lag_matrix_host": r_lag_matrix,
    "sts_ewma_add_host": r_ewma(oracle.ewma_add),
    "sts_ewma_remove_host": r_ewma(oracle.ewma_remove),
    "sts_fill_diff_ewma_host": r_fill_diff_ewma,
    "sts_ewma_fit_host": r_ewma_fit,
    "sts_ar_fit_host": r_ar_fit,
    "sts_ar_fit_remove_host": r_ar_fit,
    "sts_garch_fit_host": r_garch_fit,
    "sts_argarch_fit_host": r_argarch_fit,
    "sts_ar_remove_host": r_ar(False),
    "sts_ar_add_host": r_ar(True),
    "sts_dw_test_host": r_dw,
    "sts_kpss_test_host": r_kpss,
    "sts_adf_test_host": r_adf,
    "sts_lb_test_host": r_lb,
    "sts_bp_test_host": r_bgbp(True),
    "sts_bg_test_host": r_bgbp(False),
    "sts_factor_ols_host": r_factor_ols,
    "sts_factor_remove_host": r_factor_effect(fr.remove),
    "sts_factor_add_host": r_factor_effect(fr.add),
    "sts_roll_stat_host": r_roll_stat,
    "sts_roll_pair_host": r_roll_pair,
    "sts_quotients_host": lambda i, o, p: tr.assert_bits(o["out"], tr.quotients(i["in"], p["lag"], bool(p["minus_one"])), "quotients"),
    "sts_fill_quotients_host": r_fill_quotients,
    "sts_fill_with_default_host": lambda i, o, p: tr.assert_bits(o["out"], tr.fill_with_default(i["in"], p["filler"]), "fill_with_default"),
    "sts_downsample_host": lambda i, o, p: tr.assert_bits(o["out"], tr.downsample(i["in"], p["n"], p["phase"]), "downsample"),
    "sts_upsample_host": lambda i, o, p: tr.assert_bits(o["out"], tr.upsample(i["in"], p["n"], p["phase"], bool(p["use_zero"])), "upsample"),
    "sts_first_last_not_nan_host": r_first_last,
    "sts_inverse_diff_at_lag_host": r_inverse_diff,
    "sts_diff_order_d_host": lambda i, o, p: tr.assert_bits(o["out"], tr.differences_of_order_d(i["in"], p["d"]), "diff_order_d"),
    "sts_inverse_diff_order_d_host": lambda i, o, p: tr.assert_bits(o["out"], tr.inverse_differences_of_order_d(i["in"], p["d"]), "inverse_diff_order_d"),
    "sts_rebase_shift_host": lambda i, o, p: ir.assert_bits(o["out"], ir.gather_panel(i["in"], ir.shift_map(p["T"], p["T_out"], p["start_loc"]), p["default"]), "rebase_shift"),
    "sts_rebase_map_host": lambda i, o, p: ir.assert_bits(o["out"], ir.gather_panel(i["in"], i["map"], p["default"]), "rebase_map"),
}


def test_every_row_has_its_calls_and_reference():
    assert set(CALLS) == set(sp.NAMES) == set(REFS)


# ---------------- one case ----------------

def prefill(dtype, n):
    """what an output holds before the call, on the host and on the device alike"""
    if dtype == "f8":
        return np.full(n, la.OUT_FILL)
    if dtype == "i8":
        return np.full(n, -7777, dtype=np.int64)
    return np.full(n, -1, dtype=np.int32)


class HostArr(object):
    """one per-series array on the host: an arena (poisoned padding and red zones) seen as dtype"""

    def __init__(self, H, arr, S, w, stride, values, poison):
        self.arr, self.S, self.w, self.dtype = arr, S, w, NP_DTYPE[arr.dtype]
        self.panel = arr.kind != "vec"
        if self.panel:
            self.arena = H.carve(S, w, stride, poison, data=values)
        else:
            flat = np.ascontiguousarray(values).reshape(-1)
            pad = (-flat.nbytes) % 8
            raw = np.concatenate([flat.view(np.uint8), np.zeros(pad, np.uint8)]).view(np.float64)
            self.arena = H.carve(1, raw.size, raw.size, poison, data=raw.reshape(1, -1), red=64)
        self.ptr = self.arena.ptr

    def get(self):
        if self.panel:
            return self.arena.data()
        flat = self.arena.data().reshape(-1).view(self.dtype)[:self.S * self.w]
        return flat.reshape(self.S, self.w).copy()


class Case(object):
    """the inputs of one (row, variant), its host call and its device twin"""

    def __init__(self, torch, row, v, pin_in, pin_out, H_in, H_out, plant=None, override=None):
        """override: S, x (the input panel), F (per-series factors) and y (per-series y) given by the caller,
        for the per-series form fed copies of a shared form's inputs at the shared form's shape"""
        self.torch, self.row, self.v = torch, row, v
        override = override or {}
        self.pl = pl = row.plan(v)
        if "S" in override:
            self.pl = pl = pl._replace(S=override["S"], nchunks=sp.chunking(override["S"], pl.per_series)[1], h2d=None, d2h=None)
        self.pp = pp = row.p(v)                    # the parameters by name
        S, T = pl.S, pl.T
        self.arrays = row.arrays(v)
        self.poison = la.POISONS["sentinel" if pin_in else "nan"]
        # ---- input values, packed ----
        x = override["x"] if "x" in override else panel(row.data, S, T)
        ins, shared, F = {}, {}, None
        if "k" in pp:
            F = override["F"] if "F" in override else factors(S, T, pp["k"], pp["fs"] == "shared")
        if row.name == "sts_factor_ols_host" and "x" not in override:
            x = x + fr.INTERCEPT + (F @ fr.COEF[:pp["k"]] if F.ndim == 2 else np.einsum("stk,k->st", F, fr.COEF[:pp["k"]]))
        if plant is not None:
            x, F = plant(self, x.copy() if not x.flags.writeable else x, F)
        for a in self.arrays:
            if a.dir != "in":
                continue
            if a.kind == "panel":
                ins[a.name] = x
            elif a.kind == "ypanel":
                ins[a.name] = np.ascontiguousarray(override["y"] if "y" in override else x[::-1] * 0.5 + 1.0)
            elif a.kind == "fblock":
                ins[a.name] = np.ascontiguousarray(F.transpose(0, 2, 1))          # (S, k, T)
            elif a.kind == "zero":
                ins[a.name] = None
            elif a.name == "smoothing":
                ins[a.name] = frac(S, 1, 0.6180339887, 0.05, 0.95)
            elif a.name == "c":
                ins[a.name] = frac(S, 1, 0.7548776662, -1.0, 1.0)
            elif a.name == "coef":
                ins[a.name] = frac(S, a.width(pp), 0.5698402910, -0.3, 0.3)
            elif a.name == "beta":
                ins[a.name] = frac(S, a.width(pp), 0.4142135623, -1.5, 1.5)
            else:
                raise KeyError(a.name)
        if F is not None and F.ndim == 2:
            shared["factors"] = np.ascontiguousarray(F.T)                          # (k, T)
        if pp.get("Sy") == "shared":
            shared["y"] = np.ascontiguousarray(x[S // 2] * 0.5 + 1.0)
        if "T_out" in pp and row.name == "sts_rebase_map_host":
            shared["map"] = rebase_map(T, pp["T_out"])
        self.ins, self.shared, self.F = ins, shared, F
        self.null = set(v.null)
        self.outs = [a for a in self.arrays if a.dir == "out"]
        # ---- the host side ----
        self.H_in, self.H_out = H_in, H_out
        self.h = {}
        for a in self.arrays:
            w = a.width(pp)
            if a.dir == "in":
                if a.kind == "zero":
                    continue
                if a.kind == "fblock":
                    ld_f, k = pp["ld_f"], pp["k"]
                    blk = np.full((S, w), self.poison)
                    for j in range(k):
                        blk[:, j * ld_f:j * ld_f + T] = ins[a.name][:, j, :]
                    self.h[a.name] = HostArr(H_in, a, S, w, w + 5, blk, self.poison)
                else:
                    stride = {"panel": T + 3, "ypanel": T + 5, "vec": w}[a.kind]
                    self.h[a.name] = HostArr(H_in, a, S, w, stride, ins[a.name], self.poison)
            elif a.name in self.null:
                continue
            elif v.inplace and a.name == "out":
                self.h["out"] = self.h["in"]
            else:
                vals = prefill(a.dtype, S * w).reshape(S, w)
                self.h[a.name] = HostArr(H_out, a, S, w, T + 3 if a.kind == "panel" else w, vals, self.poison)
        if row.status and "err" not in self.null and row.name != "sts_autocorr_host":
            self.h["err"] = HostArr(H_out, sp.Arr("err", "out", "i4", None, "vec"), S, 1, 1, prefill("i4", S), self.poison)
        # shared uploads, each in a poisoned arena of its own: the factor matrix with ld_f = T + 3, the shared
        # y and the map (int64 behind a float64 view) as one row
        self.hs = {}
        for name, val in shared.items():
            if name == "factors":
                self.hs[name] = la.carve_np(pp["k"], T, T + 3, 3, self.poison, data=val)
            else:
                self.hs[name] = la.carve_np(1, val.size, val.size, 3, self.poison, data=val.view(np.float64).reshape(1, -1))

    # ---- parameters as the C calls take them ----
    def cparams(self, host):
        pp, T = self.pp, self.pl.T
        q = dict(pp)
        q["S"] = self.pl.S
        q["ld"] = T + 3 if host else T
        if "method" in q:
            q["method"] = METHODS[q["method"]]
        if "regression" in q:
            q["regression"] = REG[q["regression"]]
        if "op" in q:
            q["op"] = (ROLL_PAIR_OPS if "Sy" in q else ROLL_OPS).index(q["op"])
        if "k" in q:
            k = q["k"]
            q["ld_f"] = T + 3 if host else T
            q["fs"] = 0 if pp["fs"] == "shared" else ((k - 1) * (T + 3) + T + 5 if host else k * T)
        if "Sy" in q:
            q["Sy"] = 1 if pp["Sy"] == "shared" else self.pl.S
            q["ld_y"] = T + 5 if host else T
        return types.SimpleNamespace(**q)

    def host_ptrs(self):
        a = {n: h.ptr for n, h in self.h.items()}
        for n, hs in self.hs.items():
            a[n] = hs.ptr
        for n in list(self.null) + [x.name for x in self.arrays if x.kind == "zero"] + ["err"]:
            a.setdefault(n, None)
        return a

    def run_host(self, want_status=0):
        """the host call, with the arenas checked -> (status, message)"""
        ins = [h for n, h in self.h.items() if self.arr_dir(n) == "in" and not (self.v.inplace and n == "in")]
        outs = [h for n, h in self.h.items() if self.arr_dir(n) == "out"]
        snaps_in = [h.arena.snapshot() for h in ins] + [hs.snapshot() for hs in self.hs.values()]
        snaps_out = [h.arena.snapshot() for h in outs]
        st = CALLS[self.row.name](lib(), self.host_ptrs(), self.cparams(True), True)
        msg = last_error() if st else ""
        assert want_status is None or st == want_status, (self.row.name, st, msg)
        arenas_in = [h.arena for h in ins] + list(self.hs.values())
        for a, snap in zip(arenas_in, snaps_in):
            a.verify_all(snap, self.row.name + ": host input")
        for h, snap in zip(outs, snaps_out):
            if h.panel:
                h.arena.verify_outside(snap, self.row.name + ": host output " + h.arr.name)
            else:
                bad = (h.arena.snapshot() != snap) & ~h.arena.inside_mask()
                assert not bad.any(), (self.row.name, h.arr.name, "written outside the vector")
        return st, msg

    def arr_dir(self, name):
        if name == "err":
            return "out"
        return next(a.dir for a in self.arrays if a.name == name)

    def host_outputs(self):
        return {n: h.get() for n, h in self.h.items() if self.arr_dir(n) == "out"}

    def run_device(self, want_status=0):
        """the device twin: packed ld = T, NULL stream, everything uploaded whole -> (outputs, status, message)"""
        t, S, pp = self.torch, self.pl.S, self.pp
        up = lambda a: t.as_tensor(np.ascontiguousarray(a), device="cuda:0")
        d, a = {}, {}
        for arr in self.arrays:
            if arr.dir == "in":
                if arr.kind == "zero":
                    a[arr.name] = None
                    continue
                d[arr.name] = up(self.ins[arr.name])
            elif arr.name in self.null:
                a[arr.name] = None
                continue
            elif self.v.inplace and arr.name == "out":
                d["out"] = d["in"]
            else:
                d[arr.name] = up(prefill(arr.dtype, S * arr.width(pp)))
        if "err" in self.h or self.row.name == "sts_autocorr_host":
            d["err"] = up(prefill("i4", S))
        for n, val in self.shared.items():
            d[n] = up(val)
        for n, x in d.items():
            a[n] = x.data_ptr()
        a.setdefault("err", None)
        st = CALLS[self.row.name](lib(), a, self.cparams(False), False)
        t.cuda.synchronize()
        msg = last_error() if st else ""
        assert want_status is None or st == want_status, (self.row.name, "device twin", st, msg)
        out = {}
        for arr in self.outs + ([sp.Arr("err", "out", "i4", lambda q: 1, "vec")] if "err" in self.h else []):
            if arr.name in self.null:
                continue
            w = arr.width(pp)
            out[arr.name] = d[arr.name].cpu().numpy().reshape(S, w)
        return out, st, msg

    def reference(self, got):
        """the CPU reference of the operation on the seam series"""
        idx = sp.seam_series(self.pl)
        i = {n: (x[idx] if x is not None else None) for n, x in self.ins.items()}
        for n, val in self.shared.items():
            i[n] = val
        if self.F is not None:
            i["F"] = self.F if self.F.ndim == 2 else self.F[idx]
        o = {n: x[idx] for n, x in got.items()}
        for n in self.null:
            o[n] = None
        p = dict(self.pp)
        p["inplace"] = self.v.inplace
        REFS[self.row.name](i, o, p)


def check_stats(pl, pinned_bytes):
    st = stats()
    assert st["chunks"] == pl.nchunks, (st, pl)
    assert st["h2d_bytes"] == pl.h2d and st["d2h_bytes"] == pl.d2h, (st, pl)
    assert abs(st["direct"] - pinned_bytes / float(pl.h2d + pl.d2h)) < 1e-9, (st, pinned_bytes)
    return st


MODES = {"pageable": (False, False), "pinned": (True, True), "in_pinned_out_pageable": (True, False)}
RUNS = [(r, v, m) for r, v in sp.CASES for m in ("pageable", "pinned") + (("in_pinned_out_pageable",) if v.mixed else ())]


@pytest.mark.parametrize("row,v,mode", RUNS, ids=["%s-%s" % (sp.case_id(r, v), m) for r, v, m in RUNS])
def test_host_call_across_chunk_seams(torch, row, v, mode):
    pin_in, pin_out = MODES[mode]
    with HostArenas(pin_in) as H_in, HostArenas(pin_out) as H_out:
        c = Case(torch, row, v, pin_in, pin_out, H_in, H_out)
        pl = c.pl
        c.run_host()
        # 1, 2: the seams were crossed and the pipeline moved exactly the plan's bytes
        zero = sum(8 * pl.S for a in c.arrays if a.kind == "zero")          # the wrapper's own (pageable) zero
        st = check_stats(pl, (pl.h2d - zero if pin_in else 0) + (pl.d2h - (4 * pl.S if "err" not in c.h and row.status else 0)
                                                                 if pin_out else 0))
        if mode == "pageable":
            assert st["direct"] == 0.0
        elif mode == "pinned":
            assert st["direct"] > 0.99
        print("%s %s: T=%d S=%d ns=%d chunks=%d wall %.1f ms" % (sp.case_id(row, v), mode, pl.T, pl.S, pl.ns, pl.nchunks,
                                                                  st["wall_ms"]))
        got = c.host_outputs()
        # 3: bit for bit the device entry point on the whole panel
        twin = c.run_device()[0]
        assert set(twin) == set(got), (sorted(twin), sorted(got))
        for n in sorted(got):
            assert same_bits(got[n], twin[n]), "%s: %s differs from the device twin: %s" % (row.name, n, first_diff(got[n], twin[n]))
        # 4: the reference at the seams
        c.reference(got)


# ---------------- statuses across chunks ----------------

def plant_rows(pl):
    return [3, pl.ns, pl.S - 5]         # the first chunk, the first series of chunk 1, the last chunk


def planter(kind, rows_of_case):
    def plant(c, x, F):
        x = np.array(x)
        if kind == "duplicate_factor":
            F = np.array(F)
        for s in rows_of_case(c):
            if kind == "all_nan_but_first":       # nearest: "Input is all NaNs!" (the index-0 quirk)
                x[s, 1:] = np.nan
            elif kind == "nan":                   # the fits: every sse / likelihood is NaN
                x[s, :] = np.nan
            elif kind == "constant":              # a dyadic constant: an exactly singular AR / ADF design
                x[s, :] = 2.0
            elif kind == "duplicate_factor":      # a rank-deficient design
                F[s, :, 1] = F[s, :, 0]
        return x, F
    return plant


@pytest.mark.parametrize("row,v,kind", sp.STATUS_CASES_KIND, ids=[sp.case_id(r, v) for r, v, _ in sp.STATUS_CASES_KIND])
def test_statuses_across_chunks(torch, row, v, kind):
    # with an err array: status 0, err and every output equal to the device twin's
    with HostArenas(False) as H:
        c = Case(torch, row, v, False, False, H, H, plant=planter(kind, lambda c: plant_rows(c.pl)))
        pl = c.pl
        bad = plant_rows(pl)
        c.run_host()
        assert stats()["chunks"] == pl.nchunks
        got = c.host_outputs()
        twin = c.run_device()[0]
        failed = list(np.flatnonzero(got["err"].ravel()))
        assert failed == bad, (failed[:10], bad)          # the planted series and no other
        for n in sorted(got):
            assert same_bits(got[n], twin[n]), "%s: %s differs from the device twin: %s" % (row.name, n, first_diff(got[n], twin[n]))
    # err = NULL: the status of the lowest failing series, named by its index in the WHOLE panel (the lowest
    # planted one is the first series of chunk 1); the device twin, one launch, says the same
    with HostArenas(False) as H:
        v0 = sp.Variant(v.id, T=v.T, chunks=v.chunks, inplace=v.inplace, null=tuple(v.null) + ("err",), **v.params)
        c = Case(torch, row, v0, False, False, H, H, plant=planter(kind, lambda c: plant_rows(c.pl)[1:]))
        _, dst, dmsg = c.run_device(want_status=None)
        st, msg = c.run_host(want_status=None)
        assert stats()["chunks"] == pl.nchunks
        assert st == dst != 0 and msg == dmsg, (st, msg, dst, dmsg)
        named = int(re.search(r"series (\d+)", msg).group(1))
        assert named == pl.ns, (msg, pl.ns)
        assert st == got["err"].ravel()[pl.ns]


# ---------------- the shared form against the per-series form fed copies ----------------

@pytest.mark.parametrize("name", sorted(sp.SHARED_AGAINST_COPIES))
def test_shared_form_equals_per_series_copies(torch, name):
    """The same T and S through both host forms, each over three chunks or more: fs == 0 against fs > 0 with
    every block a copy of the shared matrix, Sy == 1 against a y panel whose every row is the shared y.  The
    whole panel is compared, so every chunk of both calls is.  staging_plan.SHARED_AGAINST_COPIES says which
    rows are held to bits and which, by the design of their kernels, to the operation's own bar."""
    row = next(r for r in sp.TABLE if r.name == name)
    vs = next(v for v in row.variants if v.id == "shared")
    vo = next(v for v in row.variants if v.id == "per_series")
    vo = sp.Variant("copies", T=vs.T, **vo.params)
    with HostArenas(False) as H:
        a = Case(torch, row, vs, False, False, H, H)
        a.run_host()
        assert stats()["chunks"] == a.pl.nchunks >= 3
        ga = a.host_outputs()
        S, T = a.pl.S, a.pl.T
        x = next(a.ins[arr.name] for arr in a.arrays if arr.dir == "in" and arr.kind == "panel")
        over = {"S": S, "x": x}
        if a.F is not None:
            over["F"] = np.broadcast_to(a.F, (S,) + a.F.shape)
        if "y" in a.shared:
            over["y"] = np.broadcast_to(a.shared["y"], (S, T))
        a.h = a.hs = None
    with HostArenas(False) as H:
        b = Case(torch, row, vo, False, False, H, H, override=over)
        b.run_host()
        assert stats()["chunks"] == b.pl.nchunks >= 3
        gb = b.host_outputs()
    assert set(ga) == set(gb)
    if sp.SHARED_AGAINST_COPIES[name] == "bits":
        for n in sorted(ga):
            assert same_bits(ga[n], gb[n]), "%s: %s, shared against copies: %s" % (name, n, first_diff(ga[n], gb[n]))
        return
    assert np.array_equal(ga["err"], gb["err"]) and (ga["err"] == 0).all()
    if name == "sts_factor_ols_host":
        # the bar and the measures of tests/test_factor_ols_gpu.py's shared-against-copies test
        e = {"beta": fr.rel(gb["beta"], ga["beta"]), "se": fr.rel(gb["stderr"], ga["stderr"]),
             "stats": fr.rel(gb["stats"], ga["stats"]), "resid": fr.resid_err(gb["resid"], ga["resid"])}
        print("%s copies against shared: %s" % (name, e))
        assert max(e.values()) <= fr.BAR, e
        return
    assert_close(gb["stat"].ravel(), ga["stat"].ravel(), 1e-10, name + " copies against shared")
    # p = 1 - chi2cdf(stat): |dp| <= max pdf * |dstat|; the chi-squared density with 3 (bp) or 5 (bg) degrees
    # of freedom stays below 0.25, |dstat| <= 1e-10 |stat| by the line above, and forming 1 - cdf rounds by 2^-53
    dp = np.abs(gb["pvalue"].ravel() - ga["pvalue"].ravel())
    assert (dp <= 0.25e-10 * np.abs(ga["stat"].ravel()) + 4e-16).all(), dp.max()


# ---------------- one series larger than a chunk ----------------

def test_one_series_larger_than_a_chunk(torch):
    S, T = 7, 4500000                      # in + out = 72 MB per series: ns = 1, seven chunks, slots 0 and 1 reused
    assert sp.chunking(S, 2 * T * 8 + 4) == (1, 7)
    L = lib()
    rng = np.random.default_rng(5)
    x = rng.standard_normal((S, T)) + np.arange(S)[:, None]
    x[rng.random((S, T)) < 0.05] = np.nan
    x[:, 0] = np.arange(S)
    assert L.sts_staging_release() == 0
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    out, err = np.full((S, T), la.OUT_FILL), np.full(S, -1, np.int32)
    assert L.sts_fill_host(P(x), P(out), S, T, T, METHODS["previous"], P(err)) == 0, last_error()
    st = stats()
    assert st["chunks"] == 7 and st["h2d_bytes"] == S * T * 8 and st["d2h_bytes"] == S * (T * 8 + 4)
    assert (err == 0).all()
    # the slots grew for this call and Borrow trimmed them again: an untrimmed set would hold 5 x 72 MB
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 <= 64 << 20, (free0, free1)
    assert pool_info()[2] == 0             # borrowed
    xd = torch.as_tensor(x, device="cuda:0")
    od = torch.full((S, T), la.OUT_FILL, dtype=torch.float64, device="cuda:0")
    assert L.sts_fill(xd.data_ptr(), od.data_ptr(), S, T, T, T, METHODS["previous"], None, None) == 0
    torch.cuda.synchronize()
    assert same_bits(out, od.cpu().numpy())
    del xd, od
    ref, _ = oracle.panel_fill(x[[0, 6]], "previous")
    assert_bits(out[[0, 6]], ref, "fill previous, series 0 and 6")
    # a small call afterwards still has the right bits
    y = oracle.gen_panel(1, 10, 100, 0.1)
    o2 = np.empty_like(y)
    assert L.sts_fill_host(P(y), P(o2), 10, 100, 100, METHODS["previous"], None) == 0
    assert stats()["chunks"] == 1
    assert_bits(o2, oracle.panel_fill(y, "previous")[0], "small call after the large one")


# ---------------- the mirror ----------------

def test_mirror_fill_return_rates_across_chunks(torch):
    from sparkts.timeseriesrdd import TimeSeriesRDD
    row = next(r for r in sp.TABLE if r.name == "sts_fill_host")
    pl = row.plan(next(v for v in row.variants if v.id == "linear"))
    x = np.array(panel("price-nan", pl.S, pl.T))
    host = TimeSeriesRDD(None, None, x).fill("linear")
    assert stats()["chunks"] == 3
    host = host.returnRates().data
    assert stats()["chunks"] == sp.chunking(pl.S, 8 * (2 * pl.T - 1))[1] >= 2
    dev = TimeSeriesRDD(None, None, torch.as_tensor(x, device="cuda:0")).fill("linear").returnRates().data
    assert isinstance(host, np.ndarray) and same_bits(host, dev.cpu().numpy())


def test_mirror_bgtest_across_chunks(torch):
    from sparkts import stats as sts_stats
    from sparkts.errors import SingularMatrixException
    # the mirror passes packed factors (ld_f = T, fs = k T): the plan of that call, three chunks of it
    # (T = 392 gives an odd series count per chunk)
    T, k = 392, 3
    per = T * 8 + 8 + 8 + 4 + k * T * 8
    S = 2 * (sp.CHUNK // per) + 37
    ns, nchunks = sp.chunking(S, per)
    assert nchunks == 3 and ns % 2 == 1
    e = np.array(panel("ar", S, T))
    F = factors(S, T, k, False)
    hs, hp = sts_stats.bgtest(e, F, 5)
    assert stats()["chunks"] == nchunks
    ds, dp = sts_stats.bgtest(torch.as_tensor(e, device="cuda:0"), torch.as_tensor(F, device="cuda:0"), 5)
    assert same_bits(hs, ds.cpu().numpy()) and same_bits(hp, dp.cpu().numpy())
    F[S - 3, :, 1] = F[S - 3, :, 0]            # a duplicated factor in the last chunk
    with pytest.raises(SingularMatrixException, match=r"series %d\b" % (S - 3)):
        sts_stats.bgtest(e, F, 5)
