"""Every float-reduction kernel across magnitudes: the device against the oracle on inputs
multiplied by 2^k, under the bar the project already uses for each operation.  Needs an MI355X.

tests/test_scale_cpu.py proves on the CPU that the references return the same bits at every
scale used here, so the unscaled contracts hold unchanged: the ACF's 1e-10 relative plus the
reference's own noise floor (computed on the UNSCALED filled series; tests/test_acf_robust.py),
the AR fit's 1e-10 elementwise over coefficients above 1e-6 of the vector (tests/test_fuzz_gpu.py;
the intercept is brought back to the unscaled units by an exact power of two first, so the mask
is the unscaled test's at every k), 1e-10 / 2e-10 relative and 1e-12 absolute p-values for the
statistical tests, bits and per-series status for the optimiser fits.  What differs from one
scale to the next is only the device's own arithmetic: products of moments in the rule-3 and
AR-rule heuristics, reciprocals, absolute tolerances of the commons-math3 state machines.

The scale lists, shapes and inputs live in tests/test_scale_cpu.py.
"""
import ctypes

import numpy as np
import pytest

import oracle
import test_scale_cpu as sc
from test_acf_robust import noise_floor, with_nans, within
from test_arima import arma_panel, check_fit, ref_lib, starts  # noqa: F401  (ref_lib: a fixture)
from test_parity_gpu import KNOB_VARIANTS, assert_bits, dev, host, torch  # noqa: F401  (torch: a fixture)

pytestmark = pytest.mark.gpu
cache = sc.cache


def lib():
    from sparkts import _native
    return _native.lib()


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ids(v):
    return "none" if v is None else str(v)


# ---------------- 1. fill + ACF ----------------

def fill_acf(torch, x, method, K):
    """-> (filled or None, acf, err_per_series) of sts_fill_autocorr"""
    from sparkts import UnivariateTimeSeries as uts
    S, T = x.shape
    xd = dev(torch, x)
    acf = torch.full((S, K), -7.0, dtype=torch.float64, device="cuda:0")
    err = torch.full((S,), -1, dtype=torch.int32, device="cuda:0")
    filled = None if method is None else torch.empty_like(xd)
    code = -1 if method is None else uts.fill_method_code(method)
    st = lib().sts_fill_autocorr(vp(xd), vp(filled), S, T, T, T, code, K, vp(acf), vp(err), None)
    assert st == 0, lib().sts_last_error()
    torch.cuda.synchronize()
    return (None if filled is None else host(filled)), host(acf), host(err)


@cache
def acf_floor(T, K, method):
    """the reference's noise floor per row and lag, on the UNSCALED filled series"""
    f0, _ = sc.acf_ref(T, K, method)
    return sc.frozen(np.array([noise_floor(r, K) for r in f0]))


def check_fill_acf(torch, T, K, method, k):
    x = sc.scaled(sc.acf_panel(T, method), k)
    filled, got, err = fill_acf(torch, x, method, K)
    rf, ref, rerr = oracle.panel_fill_autocorr(x, method, K)
    assert np.array_equal(err, rerr) and (rerr == 0).all()
    if method is not None:
        assert_bits(filled, rf, "fill %s T=%d k=%d" % (method, T, k))
    floor = acf_floor(T, K, method)
    for s in range(len(x)):
        w = within(got[s], ref[s], floor[s])
        print("T=%d K=%d %s k=%d row %d: %.3g x (1e-10 rel + noise floor)" % (T, K, method, k, s, w))
        assert w <= 1.0, (T, K, method, k, s, w)


@pytest.mark.parametrize("k", sc.ACF_SCALES)
@pytest.mark.parametrize("method", sc.FILLS, ids=ids)
@pytest.mark.parametrize("T,K", sc.ACF_SHAPES)
def test_fill_autocorr_scaled(torch, T, K, method, k):
    if ("acf", (T, K, method), k) in sc.DROPPED:
        return
    check_fill_acf(torch, T, K, method, k)


@pytest.mark.parametrize("k", [-300, 300])
@pytest.mark.parametrize("T,K", [(256, 8), (3000, 40)])
@pytest.mark.parametrize("method", ["linear", "previous"])
@pytest.mark.parametrize("kernel", ["tile", "seg", "short1", "short2"])
def test_fill_autocorr_scaled_kernel_variants(torch, ab_lib, kernel, method, T, K, k):
    ab_lib(**KNOB_VARIANTS[kernel])
    check_fill_acf(torch, T, K, method, k)


# ---------------- 2. AR fit ----------------

def ar_fit(torch, x, p, no_intercept, remove=False):
    """-> (c, coef, err_per_series[, residuals]) of sts_ar_fit / sts_ar_fit_remove"""
    S, T = x.shape
    xd = dev(torch, x)
    c = torch.full((S,), -7.0, dtype=torch.float64, device="cuda:0")
    coef = torch.full((S, p), -7.0, dtype=torch.float64, device="cuda:0")
    err = torch.full((S,), -1, dtype=torch.int32, device="cuda:0")
    if remove:
        out = torch.full_like(xd, -7.0)
        st = lib().sts_ar_fit_remove(vp(xd), vp(out), S, T, T, T, p, int(no_intercept), vp(c), vp(coef), vp(err), None)
    else:
        st = lib().sts_ar_fit(vp(xd), S, T, T, p, int(no_intercept), vp(c), vp(coef), vp(err), None)
    assert st == 0, lib().sts_last_error()
    torch.cuda.synchronize()
    res = (host(c), host(coef), host(err))
    return res + (host(out),) if remove else res


def ar_rule_count(torch, x, p, no_intercept):
    S, T = x.shape
    xd = dev(torch, x)
    n = ctypes.c_int64(-1)
    assert lib().sts_ar_rule_count(vp(xd), S, T, T, p, int(no_intercept), ctypes.byref(n), None) == 0
    return n.value


def ar_worst(c, coef, rc, rcoef, k, no_intercept):
    """tests/test_fuzz_gpu.py's bar per series, in the unscaled units (c * 2^-k: exact)"""
    worst = 0.0
    for s in range(len(c)):
        ref = np.r_[np.ldexp(rc[s], -k), rcoef[s]]
        got = np.r_[np.ldexp(c[s], -k), coef[s]]
        if no_intercept:
            ref, got = ref[1:], got[1:]
        assert np.isfinite(ref).all() and np.isfinite(got).all(), (s, got, ref)
        big = np.abs(ref) > 1e-6 * np.linalg.norm(ref)
        worst = max(worst, float(np.max(np.abs(got[big] - ref[big]) / np.abs(ref[big]))))
    return worst


@pytest.mark.parametrize("k", sc.AR_SCALES)
@pytest.mark.parametrize("no_intercept", [False, True], ids=["intercept", "no_intercept"])
@pytest.mark.parametrize("p,T", sc.AR_SHAPES)
def test_ar_fit_scaled(torch, p, T, no_intercept, k):
    if ("ar", (p, T, no_intercept), k) in sc.DROPPED:
        return
    x0 = sc.ar_panel(p, T)
    x = sc.scaled(x0, k)
    rc, rcoef, rst = sc.ar_ref(x, p, no_intercept)
    assert (rst == 0).all()
    for remove in (False, True):
        res = ar_fit(torch, x, p, no_intercept, remove)
        c, coef, err = res[:3]
        assert np.array_equal(err, rst), (remove, err)
        w = ar_worst(c, coef, rc, rcoef, k, no_intercept)
        print("p=%d T=%d no_int=%s k=%d remove=%s: worst elementwise %.3g" % (p, T, no_intercept, k, remove, w))
        assert w <= 1e-10, (p, T, no_intercept, k, remove, w)
        if remove:   # bit-exact given the device's own model
            assert_bits(res[3], np.array([oracle.ar_remove(x[s], c[s], coef[s]) for s in range(len(x))]),
                        "residuals p=%d T=%d k=%d" % (p, T, k))
    n0, n = ar_rule_count(torch, x0, p, no_intercept), ar_rule_count(torch, x, p, no_intercept)
    assert n == n0, "AR rule flags %d series at 2^%d, %d unscaled" % (n, k, n0)
    if no_intercept:
        assert n0 == len(x0)
    else:
        assert 4 <= n0 < len(x0), n0   # the tight walks are flagged, not every AR(1) row: both fits run


# ---------------- 3. statistical tests ----------------

def stat_call(torch, name, x):
    """-> (stat, check of the p-value or None)"""
    import test_stattests_gpu as tg
    if name.startswith("adf"):
        lag, reg = int(name[3]), name.split("_")[1]
        st, stat, pv = tg.call_adf(torch, x, lag, reg)
        assert st == 0
        return stat, lambda: tg.check_adf_p(stat, pv, reg)
    if name.startswith("kpss"):
        st, stat = tg.call_kpss(torch, x, name.split("_")[1])
        assert st == 0
        return stat, None
    if name == "dw":
        st, stat = tg.call_dw(torch, x)
        assert st == 0
        return stat, None
    st, stat, pv = tg.call_lb(torch, x, 5)
    assert st == 0
    return stat, lambda: tg.check_lb_p(stat, pv, 5)


@pytest.mark.parametrize("k", sc.STAT_SCALES)
@pytest.mark.parametrize("T", sc.STAT_T)
@pytest.mark.parametrize("name", sorted(sc.STAT_FUNCS))
def test_statistical_tests_scaled(torch, name, T, k):
    from test_stattests_gpu import assert_close
    if (name, T, k) in sc.DROPPED:
        return
    x = sc.scaled(sc.stat_input(name, T), k)
    want = np.array([sc.STAT_FUNCS[name](r) for r in x])
    stat, check_p = stat_call(torch, name, x)
    assert_close(stat, want, 2e-10 if name == "lb5" else 1e-10, "%s T=%d k=%d" % (name, T, k))
    if check_p is not None:
        check_p()


@pytest.mark.parametrize("k", sc.STAT_SCALES)
@pytest.mark.parametrize("T", sc.STAT_T)
@pytest.mark.parametrize("scale_what", ["residuals", "factors"])
@pytest.mark.parametrize("kind", ["bg", "bp"])
def test_bg_bp_scaled(torch, kind, scale_what, T, k):
    import bgbp_ref as br
    import test_bgbp_gpu as bt
    key = kind if scale_what == "residuals" else kind + "_factors"
    if (key, T, k) in sc.DROPPED or (key == "bp" and k not in sc.BP_SCALES):
        return   # bp_stat squares the residuals: the oracle's own range ends at 2^240
    e, F = sc.bg_inputs(T) if kind == "bg" else sc.bp_inputs(T)
    if scale_what == "residuals":
        e = sc.scaled(e, k)
    else:
        F = sc.scaled_factors(F, k)
    lag = 2 if kind == "bg" else None
    want = bt.ref_stats(e, F, lag)
    err = torch.full((len(e),), -1, dtype=torch.int32, device="cuda:0")
    st, stat, pv = bt.call(torch, e, F, lag, err=err)
    assert st == 0 and (host(err) == 0).all()
    bt.assert_close(stat, want, 1e-10, "%s %s T=%d k=%d" % (kind, scale_what, T, k))
    bt.check_p(stat, pv, 2 if kind == "bg" else 3)
    assert br.MAX_FACTORS >= 3


# ---------------- 4. optimiser fits: bits and per-series status ----------------

@pytest.mark.parametrize("k", sc.EWMA_SCALES)
@pytest.mark.parametrize("T", [64, 390])
def test_ewma_fit_scaled(torch, T, k):
    from sparkts.models import EWMA
    x = sc.scaled(sc.ewma_panel(T), k)
    err = torch.full((len(x),), -1, dtype=torch.int32, device="cuda:0")
    m = EWMA.fitModel(dev(torch, x), errors=err)
    ref_s, ref_err = oracle.panel_ewma_fit(x)
    print("EWMA T=%d k=%d: status %s" % (T, k, ref_err.tolist()))
    assert np.array_equal(host(err), ref_err), (host(err), ref_err)
    assert_bits(host(m.smoothing), ref_s, "EWMA.fitModel T=%d k=%d" % (T, k))
    if k == 400:
        assert (ref_err == sc.TOO_MANY_EVALUATIONS).all()


@pytest.mark.parametrize("k", sc.GARCH_SCALES)
def test_garch_fit_scaled(torch, k):
    from sparkts.models import GARCH
    x = sc.scaled(sc.garch_panel(), k)
    err = torch.full((len(x),), -1, dtype=torch.int32, device="cuda:0")
    m = GARCH.fitModel(dev(torch, x), errors=err)
    got = np.stack([host(m.omega), host(m.alpha), host(m.beta)], axis=1)
    rpar, rerr = oracle.panel_garch_fit(x)
    print("GARCH k=%d: status %s" % (k, rerr.tolist()))
    assert np.array_equal(host(err), rerr), (host(err), rerr)
    assert_bits(got, rpar, "GARCH.fitModel k=%d" % k)


@pytest.mark.parametrize("k", sc.ARGARCH_SCALES)
def test_argarch_fit_scaled(torch, k):
    """The AR stage within 1e-10, the GARCH stage bit-exact given the device's own residuals
    (tests/test_garch.py's contract), the per-series status the oracle's on those residuals."""
    from sparkts.models import ARGARCH
    x = sc.scaled(sc.argarch_panel(), k)
    S = len(x)
    err = torch.full((S,), -1, dtype=torch.int32, device="cuda:0")
    m = ARGARCH.fitModel(dev(torch, x), errors=err)
    c, phi = host(m.c), host(m.phi)
    rc, rcoef, rst = sc.ar_ref(x, 1, False)
    assert (rst == 0).all()
    assert np.allclose(c, rc, rtol=1e-10, atol=0) and np.allclose(phi, rcoef[:, 0], rtol=1e-10, atol=0)
    resid = np.array([oracle.ar_remove(x[s], c[s], [phi[s]]) for s in range(S)])
    rpar, rerr = oracle.panel_garch_fit(resid)
    assert np.array_equal(host(err), rerr), (host(err), rerr)
    assert_bits(np.stack([host(m.omega), host(m.alpha), host(m.beta)], axis=1), rpar, "ARGARCH k=%d" % k)


@pytest.mark.parametrize("k", sc.ARIMA_SCALES)
@pytest.mark.parametrize("p,d,q", [(1, 1, 1), (2, 0, 2)])
def test_arima_css_fit_scaled(torch, ref_lib, p, d, q, k):
    x = sc.scaled(arma_panel(60 + p + q, 4, 120, p, q, level=1.0, d=d), k)
    statuses = check_fit(ref_lib, p, d, q, x, starts(p, d, q, x))
    print("ARIMA(%d,%d,%d) k=%d: status %s" % (p, d, q, k, statuses))


# ---------------- 5. out-of-range rows ----------------

@pytest.mark.parametrize("method", ["linear", None], ids=ids)
@pytest.mark.parametrize("T,K", [(256, 8), (3000, 40)])
def test_out_of_range_fill_autocorr(torch, T, K, method):
    """Overflowing squares, total underflow, infinities: the oracle's NaN pattern and status
    (tests/test_scale_cpu.py pins them: all NaN, status 0), the fill bit for bit."""
    x = sc.out_of_range_rows(T)
    if method is not None:
        x = with_nans(x, np.random.default_rng(T))
    filled, got, err = fill_acf(torch, x, method, K)
    rf, ref, rerr = oracle.panel_fill_autocorr(x, method, K)
    assert np.array_equal(err, rerr), (err, rerr)
    if method is not None:
        assert_bits(filled, rf, "fill T=%d" % T)
    for s, name in enumerate(sc.OUT_OF_RANGE):
        assert np.array_equal(np.isnan(got[s]), np.isnan(ref[s])), (name, got[s], ref[s])
        assert_bits(got[s], ref[s], name)   # (a finite value, should the oracle ever give one)


@pytest.mark.parametrize("remove", [False, True], ids=["fit", "fit_remove"])
@pytest.mark.parametrize("no_intercept", [False, True], ids=["intercept", "no_intercept"])
@pytest.mark.parametrize("p", [2, 12])
def test_out_of_range_ar_fit(torch, p, no_intercept, remove):
    x = sc.out_of_range_rows(300)
    rc, rcoef, rst = sc.ar_ref(x, p, no_intercept)
    res = ar_fit(torch, x, p, no_intercept, remove)
    c, coef, err = res[:3]
    assert np.array_equal(err, rst), (err, rst)
    for s, name in enumerate(sc.OUT_OF_RANGE):
        assert np.array_equal(np.isnan(coef[s]), np.isnan(rcoef[s])), (name, coef[s], rcoef[s])
        if not no_intercept:
            assert np.isnan(c[s]) == np.isnan(rc[s]), (name, c[s], rc[s])
