"""One poisoned series between clean ones changes nothing for its neighbours.  Needs an MI355X.

Several kernels put more than one series in a wave or workgroup: the short fill + ACF kernel two
per LDS block, the AR register and QR lane kernels and the EWMA / GARCH fits one per lane with
wave-uniform branches, the statistical tests one factor basis per panel.  Every test here runs
one call on a clean panel and the same call on a copy in which chosen series are replaced by
poisons, and asserts

  * every clean series meets its oracle bar;
  * every clean series is BIT-IDENTICAL to the same call on the clean panel;
  * every poisoned series has the oracle's NaN pattern (and, where the oracle gives a finite
    answer -- a constant series, a leading NaN that fillNext fills -- meets the bar too);
  * err_per_series equals the oracle's for the whole panel.

Poisons: the six out-of-range rows of tests/test_scale_cpu.py (overflow, total underflow,
infinities), an all-NaN series, a constant series, a leading NaN run (left unfilled by "linear"
and "previous") and a trailing one (left unfilled by "next").  Placements: even and odd indices
(the short kernel's pair: clean + poison, poison + clean, poison + poison), the first and the
last series and, for the one-series-per-lane kernels, lanes 0, 31, 32, 63, 64 of S = 130.

The numpy restatements of the statistical tests have no per-series status: where they raise
their Singular exception the device may report STS_ERR_SINGULAR or a NaN with status 0 (an
underflowed design is singular to the one and rank-deficient noise to the other); everywhere
else the status must be 0.
"""
import numpy as np
import pytest

import bgbp_ref as br
import oracle
import stattests_ref as ref
import test_scale_cpu as sc
from test_acf_robust import noise_floor, with_nans, within
from test_parity_gpu import assert_bits, dev, host, torch  # noqa: F401  (torch: a fixture)
from test_scale_gpu import ar_fit, ar_worst, fill_acf, ids, lib, vp

pytestmark = pytest.mark.gpu
cache = sc.cache

POISONS = sc.OUT_OF_RANGE + ["all NaN", "constant", "leading NaN", "trailing NaN"]
PAIR_SLOTS = [0, 3, 6, 9, 10, 13, 16, 19, 22, 23]          # S = 24: the short kernel's pairs
LANE_SLOTS = [0, 1, 6, 31, 32, 63, 64, 65, 100, 129]       # S = 130: lanes 0, 63, 64, first, last
SINGULAR = 8


@cache
def poison_rows(T, constant=100.1):
    rng = np.random.default_rng(5000 + T)
    base = 100.0 + np.cumsum(0.1 * rng.standard_normal(T))
    rows = list(sc.out_of_range_rows(T))
    rows.append(np.full(T, np.nan))
    rows.append(np.full(T, constant))
    r = base.copy()
    r[:3] = np.nan
    rows.append(r)
    r = base.copy()
    r[-2:] = np.nan
    rows.append(r)
    assert len(rows) == len(POISONS)
    return sc.frozen(np.array(rows))


def poisoned(clean, slots, constant=100.1):
    x = np.array(clean)
    x[slots] = poison_rows(clean.shape[1], constant)
    return x


def clean_mask(S, slots):
    m = np.ones(S, bool)
    m[slots] = False
    return m


# ---------------- fill + ACF ----------------

@cache
def acf_clean(T, method):
    rows = sc.acf_rows(T)
    x = np.array([rows[i % len(rows)] for i in range(24)])
    return x if method is None else with_nans(x, np.random.default_rng(T + len(method)))


def safe_floor(r, K):
    with np.errstate(all="ignore"):
        return noise_floor(r, K) if np.isfinite(r).all() else np.zeros(K)


@pytest.mark.parametrize("method", sc.FILLS, ids=ids)
@pytest.mark.parametrize("T,K", [(256, 8), (3000, 40), (4097, 60)])
def test_fill_autocorr_neighbours(torch, T, K, method):
    clean = acf_clean(T, method)
    x = poisoned(clean, PAIR_SLOTS)
    ok = clean_mask(len(x), PAIR_SLOTS)
    f0, a0, e0 = fill_acf(torch, clean, method, K)
    f1, a1, e1 = fill_acf(torch, x, method, K)
    rf, ref_acf, rerr = oracle.panel_fill_autocorr(x, method, K)
    assert np.array_equal(e1, rerr), (e1, rerr)
    assert (e0 == 0).all() and (rerr[ok] == 0).all()
    if method is not None:
        assert_bits(f1, rf, "fill %s T=%d" % (method, T))
        assert_bits(f1[ok], f0[ok], "clean rows' fill next to poisons")
    assert_bits(a1[ok], a0[ok], "clean rows' ACF next to poisons (%s T=%d)" % (method, T))
    assert np.isfinite(ref_acf[ok]).any(axis=1).all()
    for s in range(len(x)):
        w = within(a1[s], ref_acf[s], safe_floor(rf[s], K))   # asserts the NaN pattern too
        assert w <= 1.0, (T, K, method, s, "poison" if not ok[s] else "clean", w)


# ---------------- AR fit ----------------

@cache
def ar_clean(kind, p, T):
    S = 130
    if kind == "ar":
        return oracle.gen_ar_panel(31, S, T, min(p, 5)) + 0.01 * np.sin(np.arange(T))[None, :]
    rng = np.random.default_rng(77 + p)
    return 1e4 + np.cumsum(1e-2 * rng.standard_normal((S, T)), axis=1)   # price levels: the QR lane kernel


@pytest.mark.parametrize("remove", [False, True], ids=["fit", "fit_remove"])
@pytest.mark.parametrize("kind,p,T,no_intercept", [("ar", 5, 300, False), ("ar", 12, 300, False), ("ar", 5, 300, True),
                                                   ("levels", 5, 300, False), ("levels", 12, 300, False)])
def test_ar_fit_neighbours(torch, kind, p, T, no_intercept, remove):
    clean = ar_clean(kind, p, T)
    x = poisoned(clean, LANE_SLOTS)
    ok = clean_mask(len(x), LANE_SLOTS)
    r0 = ar_fit(torch, clean, p, no_intercept, remove)
    r1 = ar_fit(torch, x, p, no_intercept, remove)
    rc, rcoef, rst = sc.ar_ref(x, p, no_intercept)
    assert np.array_equal(r1[2], rst), (r1[2][~ok], rst[~ok])
    assert (r0[2] == 0).all() and (rst[ok] == 0).all()
    w = ar_worst(r1[0][ok], r1[1][ok], rc[ok], rcoef[ok], 0, no_intercept)
    assert w <= 1e-10, w
    assert_bits(r1[1][ok], r0[1][ok], "clean rows' coefficients next to poisons")
    assert_bits(r1[0][ok], r0[0][ok], "clean rows' intercepts next to poisons")
    for s in np.flatnonzero(~ok):
        assert np.array_equal(np.isnan(r1[1][s]), np.isnan(rcoef[s])), (s, r1[1][s], rcoef[s])
        if not no_intercept:
            assert np.isnan(r1[0][s]) == np.isnan(rc[s]), (s, r1[0][s], rc[s])
    if remove:
        assert_bits(r1[3][ok], r0[3][ok], "clean rows' residuals next to poisons")
        good = np.flatnonzero(ok)
        assert_bits(r1[3][good], np.array([oracle.ar_remove(x[s], r1[0][s], r1[1][s]) for s in good]), "residuals")


# ---------------- statistical tests ----------------

def ref_or_nan(f, row):
    """-> (value, raised Singular?) of a numpy restatement; its exceptions (Singular,
    ZeroDivisionError: Python's float division where the JVM gives NaN / inf) as NaN."""
    try:
        with np.errstate(all="ignore"):
            return float(f(row)), False
    except ZeroDivisionError:
        return np.nan, False
    except Exception as e:   # stattests_ref.Singular
        assert type(e).__name__ == "Singular", e
        return np.nan, True


STAT_T = 100
# The statistical tests' constant poison is dyadic: its exact statistics are 0 / 0 (KPSS, BP, BG)
# or a singular design (ADF), and on a dyadic constant the float64 restatements say the same.  On
# a non-dyadic one (100.1) the restatement's KPSS residuals are cancellation noise of its QR and
# the ratio a noise value (11.38 at T = 100) that no relative bar can be held to; the device gives
# the exact answer's NaN there, as its contract for bit-constant responses says (include/sts.h).
STAT_CONSTANT = 3.5


@cache
def stat_clean(name):
    return sc.frozen(ref.ar1_panel(12, 130, STAT_T) if name == "lb" else ref.ordinary_panel(11, 130, STAT_T))


def check_stat(stat0, stat1, err1, want, singular, ok, rtol, what):
    from test_stattests_gpu import assert_close
    assert_close(stat1[ok], want[ok], rtol, what)
    assert_bits(stat1[ok], stat0[ok], "%s: clean rows next to poisons" % what)
    bad = ~ok
    assert np.array_equal(np.isnan(stat1[bad]), np.isnan(want[bad])), (what, stat1[bad], want[bad])
    fin = bad & ~np.isnan(want)
    assert np.allclose(stat1[fin], want[fin], rtol=rtol, atol=0)
    if err1 is not None:
        assert (err1[~singular] == 0).all(), (what, err1)
        assert np.isin(err1[singular], [0, SINGULAR]).all(), (what, err1)


@pytest.mark.parametrize("name", ["adf", "kpss", "dw", "lb"])
def test_statistical_tests_neighbours(torch, name):
    import test_stattests_gpu as tg
    clean = stat_clean(name)
    x = poisoned(clean, LANE_SLOTS, STAT_CONSTANT)
    ok = clean_mask(len(x), LANE_SLOTS)
    f = {"adf": lambda r: ref.adf_stat(r, 1, "c"), "kpss": lambda r: ref.kpss_stat(r, "c"), "dw": ref.dw_stat,
         "lb": lambda r: ref.lb_stat(r, 5)}[name]
    res = [ref_or_nan(f, r) for r in x]
    want, singular = np.array([v for v, _ in res]), np.array([s for _, s in res])
    out = []
    for panel in (clean, x):
        err = torch.full((len(x),), -1, dtype=torch.int32, device="cuda:0") if name == "adf" else None
        if name == "adf":
            st, stat, pv = tg.call_adf(torch, panel, 1, "c", err=err)
            tg.check_adf_p(stat, pv, "c")
        elif name == "kpss":
            st, stat = tg.call_kpss(torch, panel, "c")
        elif name == "dw":
            st, stat = tg.call_dw(torch, panel)
        else:
            st, stat, pv = tg.call_lb(torch, panel, 5)
            tg.check_lb_p(stat, pv, 5)
        assert st == 0
        out.append((stat, None if err is None else host(err)))
    check_stat(out[0][0], out[1][0], out[1][1], want, singular, ok, 2e-10 if name == "lb" else 1e-10, name)


@pytest.mark.parametrize("mode", ["shared", "per_series"])
@pytest.mark.parametrize("kind", ["bg", "bp"])
def test_bg_bp_neighbours(torch, kind, mode):
    import test_bgbp_gpu as bt
    S, T, lag = 130, STAT_T, (2 if kind == "bg" else None)
    F = br.factors(21, T, 3, None if mode == "shared" else S)
    clean = br.bg_resid(22, S, T) if kind == "bg" else br.bp_resid(23, S, T, F)
    x = poisoned(clean, LANE_SLOTS, STAT_CONSTANT)
    ok = clean_mask(S, LANE_SLOTS)
    res = []
    for s, row in enumerate(x):
        Fs = F if F.ndim == 2 else F[s]
        res.append(ref_or_nan((lambda r: br.bp_stat(r, Fs)) if lag is None else (lambda r: br.bg_stat(r, Fs, lag)), row))
    want, singular = np.array([v for v, _ in res]), np.array([s for _, s in res])
    out = []
    for panel in (clean, x):
        err = torch.full((S,), -1, dtype=torch.int32, device="cuda:0")
        st, stat, pv = bt.call(torch, panel, F, lag, err=err)
        assert st == 0
        bt.check_p(stat, pv, 2 if kind == "bg" else 3)
        out.append((stat, host(err)))
    assert (out[0][1] == 0).all()
    check_stat(out[0][0], out[1][0], out[1][1], want, singular, ok, 1e-10, "%s %s" % (kind, mode))


# ---------------- fits and the fused recurrence ----------------

def test_ewma_fit_neighbours(torch):
    from sparkts.models import EWMA
    rng = np.random.default_rng(61)
    clean = np.cumsum(rng.standard_normal((130, 64)), axis=1) + 100.0 + rng.uniform(-5, 5, (130, 1))
    x = poisoned(clean, LANE_SLOTS)
    ok = clean_mask(len(x), LANE_SLOTS)
    out = []
    for panel in (clean, x):
        err = torch.full((len(x),), -1, dtype=torch.int32, device="cuda:0")
        m = EWMA.fitModel(dev(torch, panel), errors=err)
        out.append((host(m.smoothing), host(err)))
    ref_s, ref_err = oracle.panel_ewma_fit(x)
    assert np.array_equal(out[1][1], ref_err), (out[1][1], ref_err)
    assert_bits(out[1][0], ref_s, "EWMA.fitModel next to poisons")
    assert (ref_err[ok] == 0).all() and (ref_err[~ok] != 0).any()
    assert_bits(out[1][0][ok], out[0][0][ok], "clean rows' smoothing next to poisons")
    assert np.array_equal(out[1][1][ok], out[0][1][ok])


def test_garch_fit_neighbours(torch):
    from mt19937 import MersenneTwister
    from sparkts.models import GARCH
    from test_garch import garch_sample
    clean = np.array([garch_sample(0.1 + 0.02 * (s % 5), 0.1 + 0.05 * (s % 4), 0.3 + 0.05 * (s % 3), 200,
                                   MersenneTwister(300 + s)) for s in range(130)])
    x = poisoned(clean, LANE_SLOTS)
    ok = clean_mask(len(x), LANE_SLOTS)
    out = []
    for panel in (clean, x):
        err = torch.full((len(x),), -1, dtype=torch.int32, device="cuda:0")
        m = GARCH.fitModel(dev(torch, panel), errors=err)
        out.append((np.stack([host(m.omega), host(m.alpha), host(m.beta)], axis=1), host(err)))
    rpar, rerr = oracle.panel_garch_fit(x, threads=8)
    assert np.array_equal(out[1][1], rerr), (out[1][1], rerr)
    assert_bits(out[1][0], rpar, "GARCH.fitModel next to poisons")
    assert (rerr[ok] == 0).sum() > ok.sum() // 2
    assert_bits(out[1][0][ok], out[0][0][ok], "clean rows' parameters next to poisons")
    assert np.array_equal(out[1][1][ok], out[0][1][ok])


@pytest.mark.parametrize("lag", [1, 3])
def test_fill_diff_ewma_neighbours(torch, lag):
    S, T = 130, 390
    clean = oracle.gen_panel(5, S, T, 0.05)
    x = poisoned(clean, LANE_SLOTS)
    ok = clean_mask(S, LANE_SLOTS)
    sm = np.random.default_rng(lag).uniform(0.05, 0.95, S)
    out = []
    for panel in (clean, x):
        xd = dev(torch, panel)
        o = torch.full_like(xd, -7.0)
        smd = dev(torch, sm)
        assert lib().sts_fill_diff_ewma(vp(xd), vp(o), S, T, T, T, 3, lag, vp(smd), None, None) == 0
        torch.cuda.synchronize()
        out.append(host(o))
    with np.errstate(all="ignore"):
        want = np.array([oracle.ewma_add(oracle.differences_at_lag(oracle.fill_previous(r), lag), float(s))
                         for r, s in zip(x, sm)])
    assert_bits(out[1], want, "fill -> diff -> EWMA next to poisons")
    assert_bits(out[1][ok], out[0][ok], "clean rows next to poisons")
    assert np.isfinite(want[ok][:, -1]).sum() > ok.sum() // 2   # (a NaN x[0] stays NaN through the recurrence)
