"""The preconditions of tests/test_scale_gpu.py and tests/test_isolation_gpu.py, on the CPU.

Those files compare the device with the oracle on inputs multiplied by 2^k and on panels that
hold non-finite or degenerate series.  A multiplication by a power of two is exact, so every
reference here (autocorr, the AR fit, the statistical tests) must return the SAME BITS at every
scale: then the tolerance contracts of the unscaled tests -- and their noise floors, computed on
the unscaled series -- apply unchanged at every scale.  This file asserts exactly that for the
scale lists and inputs the GPU files import from here, and the oracle's definite answers outside
the invariant range (overflow, total underflow, infinities), which the GPU files compare with.

The optimiser fits (EWMA, GARCH, ARIMA: commons-math3 state machines with absolute tolerances)
are NOT scale invariant; for them the file pins what the oracle does at the chosen scales (the
exits the unit-scale fuzz sweeps never visit), and the device is compared bit for bit with the
oracle at the same scaled input.

Pairs dropped because the ORACLE is not bit-invariant there (none of them a device matter):
  * none so far -- see DROPPED below, which both GPU files honour.
"""
import functools

import numpy as np
import pytest

import bgbp_ref as br
import oracle
import stattests_ref as ref
from test_acf_robust import hard_rows, with_nans

cache = functools.lru_cache(maxsize=None)

# ---------------- the scale lists (one place; the GPU files import them) ----------------

SCALES = [-400, -300, -120, -40, 40, 120, 300, 400]
ACF_SCALES = list(SCALES)                                  # autocorr is bit-invariant over [-400, 480]
AR_SCALES = list(SCALES)                                   # ar_fit over [-480, 480]
STAT_SCALES = [k for k in SCALES if abs(k) <= 300]         # ADF, KPSS, DW, LB, BG over [-300, 300]
BP_SCALES = [k for k in SCALES if abs(k) <= 240]           # bp_stat squares the residuals: [-240, 240]
EWMA_SCALES = [-300, -30, -10, 10, 30, 300, 400]
GARCH_SCALES = [-200, -20, -5, 5, 20, 60, 200]
ARGARCH_SCALES = [-5, 5]
ARIMA_SCALES = [-40, 40]
# (operation, input id, k) triples the oracle itself is not bit-invariant at: skipped by both files
DROPPED = set()

FILLS = ["linear", "previous", "next", "nearest", None]    # None: STS_FILL_NONE on the NaN-free rows
# (T, K): one shape per dispatch path of the fused fill + ACF
ACF_SHAPES = [(256, 8),      # short kernel, pair form
              (2560, 24),    # short kernel's upper edge
              (3000, 40),    # segment kernel, fused finalize
              (100, 60),     # segment kernel, unfused: T <= 2K
              (4097, 60),    # odd row stride: the tile kernel, two tiles
              (1000, 200),   # wide path, K > 60
              (30, 20)]      # exact-lag path
# (p, T): the register kernel, its edge, the MFMA kernel reached by p and by T
AR_SHAPES = [(5, 300), (8, 2560), (12, 300), (3, 2600)]
AR_FAMILIES = ["ar1", "walk", "walk_tight"]
STAT_T = [64, 200]
STAT_S = 6
OUT_OF_RANGE = ["x2^520", "x2^600", "centred x2^-600", "x2^-1060", "+inf", "+inf -inf"]
SINGULAR, TOO_MANY_EVALUATIONS = 8, 10


def scaled(x, k):
    """x * 2^k, exactly (np.ldexp); NaN stays NaN."""
    return np.ldexp(np.asarray(x, dtype=np.float64), k)


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------- inputs ----------------

@cache
def acf_rows(T):
    """hard_rows(T) (nine far-level rows), one walk, one white noise, a non-dyadic constant and a
    constant-but-one-end row: 13 series."""
    rng = np.random.default_rng(9000 + T)
    rows = list(hard_rows(T, T + 1))
    rows.append(100.0 + np.cumsum(0.1 * rng.standard_normal(T)))
    rows.append(rng.standard_normal(T))
    rows.append(np.full(T, 100.1))
    r = np.full(T, 100.1)
    r[-1] = 100.2
    rows.append(r)
    return frozen(np.array(rows))


@cache
def acf_panel(T, method):
    """The unscaled panel of one (T, fill): NaNs for the fills, none for STS_FILL_NONE."""
    x = acf_rows(T)
    return x if method is None else frozen(with_nans(x, np.random.default_rng(7 * T + len(method))))


@cache
def acf_ref(T, K, method):
    """-> (filled, acf) of the unscaled panel (filled is the panel itself without a fill)."""
    f, a, err = oracle.panel_fill_autocorr(acf_panel(T, method), method, K)
    assert (err == 0).all()
    return frozen(f, a)


@cache
def ar_panel(p, T):
    """Four series of each family: stationary AR(1) around 0 (unflagged by the AR rule), a walk at
    level 1e4 and a walk at level 1e4 with spread 1e-2 (flagged: the QR lane kernel)."""
    rng = np.random.default_rng(100 * p + T)
    rows = [oracle.ar_add(rng.standard_normal(T), 0.0, [phi]) for phi in (0.3, 0.5, 0.7, 0.9)]
    rows += [1e4 + np.cumsum(rng.standard_normal(T)) for _ in range(4)]
    rows += [1e4 + np.cumsum(1e-2 * rng.standard_normal(T)) for _ in range(4)]
    return frozen(np.array(rows))


def ar_ref(x, p, no_intercept):
    """oracle.ar_fit per series -> (c, coef, status); NaN where the fit fails."""
    S = len(x)
    c, coef, st = np.full(S, np.nan), np.full((S, p), np.nan), np.zeros(S, np.int32)
    for s in range(S):
        try:
            c[s], coef[s] = oracle.ar_fit(x[s], p, no_intercept)
        except oracle.OracleError as e:
            st[s] = e.code
    return c, coef, st


@cache
def ar_ref0(p, T, no_intercept):
    c, coef, st = ar_ref(ar_panel(p, T), p, no_intercept)
    assert (st == 0).all()
    return frozen(c, coef)


@cache
def stat_panel(T):
    return frozen(ref.ordinary_panel(300 + T, STAT_S, T))


@cache
def lb_panel(T):
    return frozen(ref.ar1_panel(400 + T, STAT_S, T))


@cache
def bg_inputs(T):
    """-> (residuals (S, T), factors (T, 3))"""
    return frozen(br.bg_resid(500 + T, STAT_S, T), br.factors(600 + T, T, 3))


@cache
def bp_inputs(T):
    F = br.factors(700 + T, T, 3)
    return frozen(br.bp_resid(800 + T, STAT_S, T, F), F)


def factor_exps(k):
    """The per-column powers of two of the factor-scaling cases."""
    return (k // 2, -k // 3, 7)


def scaled_factors(F, k):
    F = np.array(F, dtype=np.float64)
    for j, e in enumerate(factor_exps(k)):
        F[..., j] = np.ldexp(F[..., j], e)
    return F


# the statistical tests of one series: name -> callable(row)
STAT_FUNCS = {"adf0_nc": lambda r: ref.adf_stat(r, 0, "nc"), "adf0_c": lambda r: ref.adf_stat(r, 0, "c"),
              "adf0_ct": lambda r: ref.adf_stat(r, 0, "ct"), "adf3_nc": lambda r: ref.adf_stat(r, 3, "nc"),
              "adf3_c": lambda r: ref.adf_stat(r, 3, "c"), "adf3_ct": lambda r: ref.adf_stat(r, 3, "ct"),
              "kpss_c": lambda r: ref.kpss_stat(r, "c"), "kpss_ct": lambda r: ref.kpss_stat(r, "ct"),
              "dw": ref.dw_stat, "lb5": lambda r: ref.lb_stat(r, 5)}


def stat_input(name, T):
    return lb_panel(T) if name == "lb5" else stat_panel(T)


@cache
def stat_ref0(name, T):
    return frozen(np.array([STAT_FUNCS[name](r) for r in stat_input(name, T)]))


@cache
def bg_ref0(T):
    e, F = bg_inputs(T)
    return frozen(np.array([br.bg_stat(r, F, 2) for r in e]))


@cache
def bp_ref0(T):
    e, F = bp_inputs(T)
    return frozen(np.array([br.bp_stat(r, F) for r in e]))


@cache
def ewma_panel(T):
    rng = np.random.default_rng(50 + T)
    return frozen(np.cumsum(rng.standard_normal((8, T)), axis=1) + 100.0 + rng.uniform(-5, 5, (8, 1)))


@cache
def garch_panel():
    from mt19937 import MersenneTwister
    from test_garch import garch_sample
    rows = [garch_sample(0.1 + 0.05 * s, 0.1 + 0.04 * s, 0.3 + 0.05 * (s % 3), 200, MersenneTwister(70 + s))
            for s in range(6)]
    return frozen(np.array(rows))


@cache
def argarch_panel():
    from mt19937 import MersenneTwister
    from test_garch import argarch_sample
    rows = [argarch_sample(1.0 + 0.1 * s, 0.3 - 0.05 * s, 0.2, 0.3, 0.4, 400, MersenneTwister(90 + s))
            for s in range(4)]
    return frozen(np.array(rows))


@cache
def out_of_range_rows(T):
    """The six rows whose scale leaves the invariant range, from one walk at level 100: overflow
    of the squares (x 2^520, x 2^600), total underflow of the squares ((x - mean) 2^-600,
    x 2^-1060: subnormal values), one +inf, and +inf with -inf."""
    rng = np.random.default_rng(4000 + T)
    x = 100.0 + np.cumsum(0.1 * rng.standard_normal(T))
    rows = [scaled(x, 520), scaled(x, 600), scaled(x - x.mean(), -600), scaled(x, -1060)]
    r = x.copy()
    r[T // 2] = np.inf
    rows.append(r)
    r = x.copy()
    r[T // 3] = np.inf
    r[2 * T // 3] = -np.inf
    rows.append(r)
    return frozen(np.array(rows))


# ---------------- the tests ----------------

@pytest.mark.parametrize("T,K", ACF_SHAPES)
def test_fill_and_autocorr_are_bit_invariant(T, K):
    for method in FILLS:
        f0, a0 = acf_ref(T, K, method)
        for k in ACF_SCALES:
            if ("acf", (T, K, method), k) in DROPPED:
                continue
            f, a, err = oracle.panel_fill_autocorr(scaled(acf_panel(T, method), k), method, K)
            assert (err == 0).all()
            assert same_bits(f, scaled(f0, k)), (T, K, method, k, "fill")
            assert same_bits(a, a0), (T, K, method, k, "acf")
            assert np.array_equal(np.isfinite(a), np.isfinite(a0))


@pytest.mark.parametrize("no_intercept", [False, True])
@pytest.mark.parametrize("p,T", AR_SHAPES)
def test_ar_fit_is_bit_invariant(p, T, no_intercept):
    c0, coef0 = ar_ref0(p, T, no_intercept)
    assert np.isfinite(coef0).all() and np.isfinite(c0).all()
    for k in AR_SCALES:
        if ("ar", (p, T, no_intercept), k) in DROPPED:
            continue
        c, coef, st = ar_ref(scaled(ar_panel(p, T), k), p, no_intercept)
        assert (st == 0).all(), k
        assert same_bits(coef, coef0), (p, T, no_intercept, k)
        assert same_bits(c, scaled(c0, k)), (p, T, no_intercept, k, "c rescaled")


@pytest.mark.parametrize("T", STAT_T)
@pytest.mark.parametrize("name", sorted(STAT_FUNCS))
def test_statistical_tests_are_bit_invariant(name, T):
    want = stat_ref0(name, T)
    assert np.isfinite(want).all()
    for k in STAT_SCALES:
        if (name, T, k) in DROPPED:
            continue
        got = np.array([STAT_FUNCS[name](r) for r in scaled(stat_input(name, T), k)])
        assert same_bits(got, want), (name, T, k)


@pytest.mark.parametrize("T", STAT_T)
def test_bg_and_bp_are_bit_invariant(T):
    e, F = bg_inputs(T)
    want = bg_ref0(T)
    assert np.isfinite(want).all()
    for k in STAT_SCALES:
        if ("bg", T, k) not in DROPPED:
            assert same_bits([br.bg_stat(r, F, 2) for r in scaled(e, k)], want), ("bg", T, k)
        if ("bg_factors", T, k) not in DROPPED:
            assert same_bits([br.bg_stat(r, scaled_factors(F, k), 2) for r in e], want), ("bg factors", T, k)
    e, F = bp_inputs(T)
    want = bp_ref0(T)
    assert np.isfinite(want).all()
    for k in BP_SCALES:
        if ("bp", T, k) not in DROPPED:
            assert same_bits([br.bp_stat(r, F) for r in scaled(e, k)], want), ("bp", T, k)
    for k in STAT_SCALES:
        if ("bp_factors", T, k) not in DROPPED:
            assert same_bits([br.bp_stat(r, scaled_factors(F, k)) for r in e], want), ("bp factors", T, k)


@pytest.mark.parametrize("T", [64, 390])
def test_ewma_fit_exits_change_with_the_scale(T):
    """Not invariant: the optimiser's absolute tolerances see the data's units.  At x 2^400 every
    series ends in TooManyEvaluations; at the moderate scales every series converges."""
    x = ewma_panel(T)
    for k in EWMA_SCALES:
        sm, err = oracle.panel_ewma_fit(scaled(x, k))
        if k == 400:
            assert (err == TOO_MANY_EVALUATIONS).all() and np.isnan(sm).all(), (k, err)
        else:
            assert np.isin(err, [0, TOO_MANY_EVALUATIONS]).all(), (k, err)
            assert np.array_equal(np.isnan(sm), err != 0)
        if abs(k) <= 30:
            assert (err == 0).all(), (k, err)


def test_garch_fit_exits_change_with_the_scale():
    """The oracle mixes status 0 and TooManyEvaluations over these scales, by series."""
    x = garch_panel()
    seen = set()
    for k in GARCH_SCALES:
        par, err = oracle.panel_garch_fit(scaled(x, k))
        assert np.array_equal(np.isnan(par).any(axis=1), err != 0), k
        seen |= set(int(v) for v in err)
    assert {0, TOO_MANY_EVALUATIONS} <= seen, seen
    for k in ARGARCH_SCALES:
        par, err = oracle.panel_argarch_fit(scaled(argarch_panel(), k))
        assert np.array_equal(np.isnan(par).any(axis=1), err != 0), k


@pytest.mark.parametrize("T,K", [(256, 8), (3000, 40)])
def test_out_of_range_autocorr(T, K):
    """Overflow, total underflow and infinities: every autocorrelation is NaN, status 0."""
    x = out_of_range_rows(T)
    assert np.isfinite(x[:4]).all() and (x[3] != 0).any()
    for method in ("linear", None):
        xs = with_nans(x, np.random.default_rng(T)) if method else x
        f, a, err = oracle.panel_fill_autocorr(xs, method, K)
        assert (err == 0).all()
        assert np.isnan(a).all(), np.argwhere(~np.isnan(a))[:4]


@pytest.mark.parametrize("p", [2, 12])
def test_out_of_range_ar_fit(p):
    """Overflow and infinities: NaN coefficients with status 0; total underflow: a singular
    design (SingularMatrixException)."""
    x = out_of_range_rows(300)
    for no_intercept in (False, True):
        c, coef, st = ar_ref(x, p, no_intercept)
        assert st.tolist() == [0, 0, SINGULAR, SINGULAR, 0, 0], st
        assert np.isnan(coef).all()
        if not no_intercept:
            assert np.isnan(c).all()
