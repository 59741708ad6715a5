"""Batched statistical tests on the device (sts_adf_test, sts_kpss_test, sts_dw_test, sts_lb_test
and their `_host` variants) against tests/stattests_ref.py, the float64 restatement of
S/stats/TimeSeriesStatisticalTests.scala.

Shapes.  T in {minimum legal, 19, 20, 63, 64, 65, 129, 390, 2520, one past the one-wave limit,
5000}: 19 / 20 straddle the KPSS lag 0 -> 1, 63 / 64 / 65 the wave width, 129 a third tile,
2520 / 2561 the one-wave / workgroup kernels, 5000 several workgroup tiles.  S in {1, 3, 65, 257}
is paired with T so that every S and every T occurs and the checker (Householder QR in numpy, per
series) stays within a second or two per id: the kernels give one workgroup to a series, so S
only sets the grid size and the large S ride on the short series.

Bars.  Ordinary rows (stationary AR(1) and random walks, level of the order of the spread):
|got - ref| <= 1e-10 |ref|; Ljung-Box 2e-10 (a squared correlation doubles the ACF bar's relative
error).  Hard rows (ADF, KPSS; level 1e4 / 1e6, drift, noise 1e-2 .. 1e-1):
|got - exact| <= 1e-10 |exact| + 4 |ref64 - exact| with `exact` from 60-digit arithmetic
(tests/golden/stattests_exact.json).  p-values: 1e-12 absolute against the restated p-value
function fed the device's own statistic.
"""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest

import layout_arena as la
import stattests_ref as ref

pytestmark = pytest.mark.gpu
cache = functools.lru_cache(maxsize=None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, BAD_ARG, REQUIREMENT, NOT_ENOUGH_DATA, SINGULAR = 0, 1, 5, 7, 8
REG = {"nc": 0, "c": 1, "ct": 2, "ctt": 3}
T_LIST = [19, 20, 63, 64, 65, 129, 390, 2520, ref.ONE_WAVE + 1, 5000]
S_FOR_T = {19: 257, 20: 65, 63: 3, 64: 1, 65: 65, 129: 65, 390: 65, 2520: 3, ref.ONE_WAVE + 1: 3, 5000: 3}
S_MIN = 3          # at each method's minimum legal T
ADF_LAGS = [0, 1, 5, 31]
LB_LAGS = [1, 20, 60, 70]


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


def lib():
    from sparkts import _native
    return _native.lib()


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dev(torch, a, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda:0")


def outvec(torch, S, fill=-3.0e55):
    return torch.full((S,), fill, dtype=torch.float64, device="cuda:0")


@cache
def panel(T, S):
    return ref.ordinary_panel(1000 + T, S, T)


@cache
def ar_panel(T, S):
    return ref.ar1_panel(2000 + T, S, T)


def assert_close(got, want, rtol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN pattern differs" % what
    fin = ~np.isnan(want)
    if fin.any():
        err = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
        print("%s: max rel err %.3g over %d" % (what, err.max(), int(fin.sum())))
        assert err.max() <= rtol, "%s: max rel err %g > %g (series %d)" % (what, err.max(), rtol, int(np.argmax(err)))


# ---- the device calls ----

def call_adf(torch, x, lag, reg, want_p=True, err=None, ld=None):
    S, T = x.shape
    d = dev(torch, x)
    stat, pv = outvec(torch, S), outvec(torch, S) if want_p else None
    st = lib().sts_adf_test(vp(d), S, T, T if ld is None else ld, lag, REG.get(reg, reg), vp(stat), vp(pv), vp(err), None)
    torch.cuda.synchronize()
    return st, stat.cpu().numpy(), (pv.cpu().numpy() if want_p else None)


def call_kpss(torch, x, reg):
    S, T = x.shape
    d, stat = dev(torch, x), outvec(torch, S)
    st = lib().sts_kpss_test(vp(d), S, T, T, REG.get(reg, reg), vp(stat), None)
    torch.cuda.synchronize()
    return st, stat.cpu().numpy()


def call_dw(torch, x):
    S, T = x.shape
    d, stat = dev(torch, x), outvec(torch, S)
    st = lib().sts_dw_test(vp(d), S, T, T, vp(stat), None)
    torch.cuda.synchronize()
    return st, stat.cpu().numpy()


def call_lb(torch, x, K, want_p=True):
    S, T = x.shape
    d, stat, pv = dev(torch, x), outvec(torch, S), outvec(torch, S) if want_p else None
    st = lib().sts_lb_test(vp(d), S, T, T, K, vp(stat), vp(pv), None)
    torch.cuda.synchronize()
    return st, stat.cpu().numpy(), (pv.cpu().numpy() if want_p else None)


def adf_min_T(lag, reg):
    return 2 * lag + REG[reg] + 3          # nObs = T - 1 - lag > k = 1 + lag + q


def check_adf_p(stat, pv, reg):
    want = np.array([ref.mackinnon_p(float(v), reg) for v in stat])
    assert np.array_equal(np.isnan(pv), np.isnan(want))
    fin = ~np.isnan(want)
    assert np.all(np.abs(pv[fin] - want[fin]) <= 1e-12), np.abs(pv[fin] - want[fin]).max()


def check_lb_p(stat, pv, K):
    want = np.array([ref.chi2_sf(float(v), K) for v in stat])
    assert np.array_equal(np.isnan(pv), np.isnan(want))
    fin = ~np.isnan(want)
    assert np.all(np.abs(pv[fin] - want[fin]) <= 1e-12), np.abs(pv[fin] - want[fin]).max()


# ---- ordinary rows ----

ADF_CASES = [(T, lag, reg) for T in T_LIST for lag in ADF_LAGS for reg in ref.REGRESSIONS if T >= adf_min_T(lag, reg)]
ADF_MIN_CASES = [(lag, reg) for lag in ADF_LAGS for reg in ref.REGRESSIONS]


@pytest.mark.parametrize("T,lag,reg", ADF_CASES)
def test_adf_ordinary(torch, T, lag, reg):
    x = panel(T, S_FOR_T[T])
    st, stat, pv = call_adf(torch, x, lag, reg)
    assert st == OK
    assert_close(stat, [ref.adf_stat(r, lag, reg) for r in x], 1e-10, "adf(%d, %s) T=%d" % (lag, reg, T))
    check_adf_p(stat, pv, reg)


@pytest.mark.parametrize("lag,reg", ADF_MIN_CASES)
def test_adf_minimum_legal_length(torch, lag, reg):
    T = adf_min_T(lag, reg)
    x = panel(T, S_MIN)
    st, stat, pv = call_adf(torch, x, lag, reg)
    assert st == OK
    assert_close(stat, [ref.adf_stat(r, lag, reg) for r in x], 1e-10, "adf(%d, %s) T=%d" % (lag, reg, T))
    check_adf_p(stat, pv, reg)


@pytest.mark.parametrize("reg", ["c", "ct"])
@pytest.mark.parametrize("T", ["min"] + T_LIST)
def test_kpss_ordinary(torch, T, reg):
    if T == "min":
        T, S = REG[reg] + 1, S_MIN
    else:
        S = S_FOR_T[T]
    x = panel(T, S)
    st, stat = call_kpss(torch, x, reg)
    assert st == OK
    assert_close(stat, [ref.kpss_stat(r, reg) for r in x], 1e-10, "kpss(%s) T=%d" % (reg, T))


@pytest.mark.parametrize("T", [1, 2] + T_LIST)
def test_dw_ordinary(torch, T):
    x = panel(T, S_FOR_T.get(T, S_MIN))
    st, stat = call_dw(torch, x)
    assert st == OK
    assert_close(stat, [ref.dw_stat(r) for r in x], 1e-10, "dw T=%d" % T)


@pytest.mark.parametrize("K", LB_LAGS)
@pytest.mark.parametrize("T", ["min"] + T_LIST)
def test_lb_ordinary(torch, T, K):
    if T == "min":
        T, S = K + 2, S_MIN     # the shortest series whose K autocorrelations are all defined
    else:
        S = S_FOR_T[T]
    x = ar_panel(T, S)
    st, stat, pv = call_lb(torch, x, K)
    assert st == OK
    assert_close(stat, [ref.lb_stat(r, K) for r in x], 2e-10, "lb(%d) T=%d" % (K, T))   # NaN where K >= T, as the reference
    check_lb_p(stat, pv, K)


# ---- hard rows ----

@cache
def exact_doc():
    with open(os.path.join(ROOT, "tests", "golden", "stattests_exact.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("T", [390, 2520])
@pytest.mark.parametrize("kind,lag,reg", ref.HARD_STATS)
def test_hard_rows(torch, kind, lag, reg, T):
    idx = [i for i, r in enumerate(ref.HARD_ROWS) if r[4] == T]
    x = np.stack([ref.hard_row(i) for i in idx])
    exact = np.array([float.fromhex(exact_doc()["rows"][i]["exact"]["%s_%d_%s" % (kind, lag, reg)]) for i in idx])
    ref64 = np.array([ref.ref_stat(kind, lag, reg, r) for r in x])
    st, got = call_adf(torch, x, lag, reg)[:2] if kind == "adf" else call_kpss(torch, x, reg)
    assert st == OK
    bar = 1e-10 * np.abs(exact) + 4 * np.abs(ref64 - exact)
    err = np.abs(got - exact)
    for i, j in enumerate(idx):
        print("%s(%d, %s) row %s: |got-exact|/|exact| %.3g, |ref64-exact|/|exact| %.3g" % (
            kind, lag, reg, ref.HARD_ROWS[j], err[i] / abs(exact[i]), abs(ref64[i] - exact[i]) / abs(exact[i])))
    assert np.all(err <= bar), [ref.HARD_ROWS[idx[i]] for i in np.flatnonzero(~(err <= bar))]


# ---- p-values ----

@pytest.mark.parametrize("reg", ref.REGRESSIONS)
def test_adf_pvalue_branches_and_clamps(torch, reg):
    """The device p-value kernel over a grid of statistics that crosses tau_min, tau* and tau_max:
    reached through a panel whose ADF statistics are whatever they are, then the kernel is checked
    on its own statistic -- and directly on the clamps via very stationary / explosive series."""
    T = 64
    t = np.arange(T, dtype=np.float64)
    rng = np.random.RandomState(5)
    rows = [(-1.0) ** t + 1e-3 * rng.standard_normal(T),          # tau far below tau_min: p = 0
            np.exp(0.2 * t) + 1e-3 * rng.standard_normal(T),      # explosive: tau above tau_max: p = 1
            np.cumsum(rng.standard_normal(T)),                    # a walk: the large-p cubic
            rng.standard_normal(T)]                               # noise: the small-p quadratic
    x = np.stack(rows + [r for r in panel(T, 65)[:28]])
    st, stat, pv = call_adf(torch, x, 0, reg)
    assert st == OK
    check_adf_p(stat, pv, reg)
    star, lo, hi, _, _ = ref.MACKINNON[reg]
    assert stat[0] < lo and pv[0] == 0.0
    if math.isfinite(hi):
        assert stat[1] > hi and pv[1] == 1.0
    assert (stat[2:] > star).any() and ((stat[2:] <= star) & (stat[2:] >= lo)).any()
    # pvalue = NULL: the statistic alone, bit-identical
    st2, stat2, _ = call_adf(torch, x, 0, reg, want_p=False)
    assert st2 == OK and np.array_equal(stat2.view(np.uint64), stat.view(np.uint64))


def test_lb_without_pvalue(torch):
    x = ar_panel(129, 257)[:9]
    st, stat, pv = call_lb(torch, x, 5)
    st2, stat2, _ = call_lb(torch, x, 5, want_p=False)
    assert st == OK and st2 == OK and np.array_equal(stat.view(np.uint64), stat2.view(np.uint64))


# ---- errors ----

def test_adf_singular_series(torch):
    x = panel(64, 1).repeat(5, axis=0) + np.arange(5)[:, None]
    x[1] = 5.0
    x[3] = -2.5
    err = torch.full((5,), -1, dtype=torch.int32, device="cuda:0")
    st, stat, pv = call_adf(torch, x, 2, "c", err=err)
    assert st == OK
    assert err.cpu().numpy().tolist() == [0, SINGULAR, 0, SINGULAR, 0]
    assert np.isnan(stat[[1, 3]]).all() and np.isnan(pv[[1, 3]]).all()
    assert_close(stat[[0, 2, 4]], [ref.adf_stat(x[i], 2, "c") for i in (0, 2, 4)], 1e-10, "neighbours of singular series")
    st, _, _ = call_adf(torch, x, 2, "c")                  # no err array: the first failure is the return
    assert st == SINGULAR
    assert b"series 1" in lib().sts_last_error()


def test_nan_series_give_nan_and_status_zero(torch):
    x = panel(129, 257)[:6].copy()
    x[1, 40] = np.nan
    x[4, 0] = np.nan
    good = [0, 2, 3, 5]
    err = torch.full((6,), -1, dtype=torch.int32, device="cuda:0")
    st, stat, pv = call_adf(torch, x, 1, "ct", err=err)
    assert st == OK and err.cpu().numpy().tolist() == [0] * 6
    assert np.isnan(stat[[1, 4]]).all() and np.isnan(pv[[1, 4]]).all()
    assert_close(stat[good], [ref.adf_stat(x[i], 1, "ct") for i in good], 1e-10, "adf next to NaN series")
    st, stat = call_kpss(torch, x, "ct")
    assert st == OK and np.isnan(stat[[1, 4]]).all()
    assert_close(stat[good], [ref.kpss_stat(x[i], "ct") for i in good], 1e-10, "kpss next to NaN series")
    st, stat = call_dw(torch, x)
    assert st == OK and np.isnan(stat[[1, 4]]).all()
    assert_close(stat[good], [ref.dw_stat(x[i]) for i in good], 1e-10, "dw next to NaN series")
    st, stat, pv = call_lb(torch, x, 5)
    assert st == OK and np.isnan(stat[[1, 4]]).all() and np.isnan(pv[[1, 4]]).all()
    assert_close(stat[good], [ref.lb_stat(x[i], 5) for i in good], 2e-10, "lb next to NaN series")


def test_call_level_errors_leave_outputs_alone(torch):
    x = panel(20, 65)[:4]
    S, T = x.shape
    d = dev(torch, x)
    stat, pv = outvec(torch, S), outvec(torch, S)
    untouched = lambda: bool((stat == -3.0e55).all()) and bool((pv == -3.0e55).all())
    L = lib()
    # nObs <= k: T = 20, maxLag = 8, ct -> nObs = 11 = k
    assert L.sts_adf_test(vp(d), S, T, T, 8, REG["ct"], vp(stat), vp(pv), None, None) == NOT_ENOUGH_DATA
    assert L.sts_adf_test(vp(d), S, T, T, 1, 4, vp(stat), vp(pv), None, None) == BAD_ARG
    assert L.sts_adf_test(vp(d), S, T, T, 1, -1, vp(stat), vp(pv), None, None) == BAD_ARG
    assert L.sts_adf_test(vp(d), S, T, T, 32, REG["c"], vp(stat), vp(pv), None, None) == BAD_ARG
    assert L.sts_adf_test(vp(d), S, T, T, -1, REG["c"], vp(stat), vp(pv), None, None) == BAD_ARG
    assert L.sts_lb_test(vp(d), S, T, T, 0, vp(stat), vp(pv), None) == BAD_ARG
    assert L.sts_kpss_test(vp(d), S, T, T, REG["ctt"], vp(stat), None) == REQUIREMENT
    assert L.sts_kpss_test(vp(d), S, 2, T, REG["ct"], vp(stat), None) == NOT_ENOUGH_DATA
    assert L.sts_dw_test(vp(d), S, T, T - 1, vp(stat), None) == BAD_ARG
    torch.cuda.synchronize()
    assert untouched()
    # the _host variants report the same statuses before staging anything
    hs, hp = np.full(S, -3.0e55), np.full(S, -3.0e55)
    hv = lambda a: ctypes.c_void_p(a.ctypes.data)
    xc = np.ascontiguousarray(x)
    assert L.sts_adf_test_host(hv(xc), S, T, T, 8, REG["ct"], hv(hs), hv(hp), None) == NOT_ENOUGH_DATA
    assert L.sts_adf_test_host(hv(xc), S, T, T, 1, 7, hv(hs), hv(hp), None) == BAD_ARG
    assert L.sts_lb_test_host(hv(xc), S, T, T, 0, hv(hs), hv(hp)) == BAD_ARG
    assert L.sts_kpss_test_host(hv(xc), S, T, T, REG["nc"], hv(hs)) == REQUIREMENT
    assert (hs == -3.0e55).all() and (hp == -3.0e55).all()


# ---- layout contract (tests/layout_arena.py): padded-odd-ld and skewed panels, both poisons ----

LAY_S, LAY_T = 5, 131
ENTRY = ["adf", "kpss", "dw", "lb"]


def layout_ref(name, x):
    if name == "adf":
        return [ref.adf_stat(r, 3, "ct") for r in x], 1e-10
    if name == "kpss":
        return [ref.kpss_stat(r, "ct") for r in x], 1e-10
    if name == "dw":
        return [ref.dw_stat(r) for r in x], 1e-10
    return [ref.lb_stat(r, 7) for r in x], 2e-10


def layout_call(name, host, ptr, S, T, ld, stat, pv, stream_args):
    L = lib()
    sfx = "_host" if host else ""
    if name == "adf":
        return getattr(L, "sts_adf_test" + sfx)(ptr, S, T, ld, 3, REG["ct"], stat, pv, None, *stream_args)
    if name == "kpss":
        return getattr(L, "sts_kpss_test" + sfx)(ptr, S, T, ld, REG["ct"], stat, *stream_args)
    if name == "dw":
        return getattr(L, "sts_dw_test" + sfx)(ptr, S, T, ld, stat, *stream_args)
    return getattr(L, "sts_lb_test" + sfx)(ptr, S, T, ld, 7, stat, pv, *stream_args)


@pytest.mark.parametrize("poison", list(la.POISONS))
@pytest.mark.parametrize("lay", ["odd", "skew"])
@pytest.mark.parametrize("name", ENTRY)
def test_layout_device(torch, name, lay, poison):
    x = ar_panel(LAY_T, LAY_S)
    ld, _, base, _ = la.layout(lay, LAY_T)
    a = la.carve(LAY_S, LAY_T, ld, base, la.POISONS[poison], data=x)
    so, po = la.carve(1, LAY_S, LAY_S, 0, la.OUT_FILL, red=64), la.carve(1, LAY_S, LAY_S, 0, la.OUT_FILL, red=64)
    snap, ssnap, psnap = a.snapshot(), so.snapshot(), po.snapshot()
    st = layout_call(name, False, ctypes.c_void_p(a.ptr), LAY_S, LAY_T, ld, ctypes.c_void_p(so.ptr),
                     ctypes.c_void_p(po.ptr), (None,))
    torch.cuda.synchronize()
    assert st == OK
    a.verify_all(snap)
    so.verify_outside(ssnap)
    po.verify_outside(psnap)
    want, rtol = layout_ref(name, x)
    assert_close(so.data()[0], want, rtol, "%s %s %s" % (name, lay, poison))


@pytest.mark.parametrize("poison", list(la.POISONS))
@pytest.mark.parametrize("lay", ["odd", "skew"])
@pytest.mark.parametrize("name", ENTRY)
def test_layout_host(torch, name, lay, poison):
    x = ar_panel(LAY_T, LAY_S)
    ld, _, base, _ = la.layout(lay, LAY_T)
    a = la.carve_np(LAY_S, LAY_T, ld, base, la.POISONS[poison], data=x)
    so = la.carve_np(1, LAY_S, LAY_S, 0, la.OUT_FILL, red=64)
    po = la.carve_np(1, LAY_S, LAY_S, 0, la.OUT_FILL, red=64)
    snap, ssnap, psnap = a.snapshot(), so.snapshot(), po.snapshot()
    st = layout_call(name, True, ctypes.c_void_p(a.ptr), LAY_S, LAY_T, ld, ctypes.c_void_p(so.ptr),
                     ctypes.c_void_p(po.ptr), ())
    assert st == OK
    a.verify_all(snap)
    so.verify_outside(ssnap)
    po.verify_outside(psnap)
    want, rtol = layout_ref(name, x)
    assert_close(so.data()[0], want, rtol, "%s_host %s %s" % (name, lay, poison))


# ---- Python mirror ----

def test_python_mirror(torch):
    from sparkts.stats import TimeSeriesStatisticalTests as tst
    from sparkts.timeseriesrdd import TimeSeriesRDD
    x = ar_panel(129, 257)[:7]
    want_adf = np.array([ref.adf_stat(r, 2, "c") for r in x])
    want_kpss = np.array([ref.kpss_stat(r, "ct") for r in x])
    want_dw = np.array([ref.dw_stat(r) for r in x])
    want_lb = np.array([ref.lb_stat(r, 6) for r in x])
    xd = dev(torch, x)
    for data, back in ((x, np.asarray), (xd, lambda v: v.cpu().numpy())):
        s, p = tst.adftest(data, 2)
        assert_close(back(s), want_adf, 1e-10, "adftest panel")
        check_adf_p(back(s), back(p), "c")
        s, crit = tst.kpsstest(data, "ct")
        assert_close(back(s), want_kpss, 1e-10, "kpsstest panel")
        assert crit == {0.10: 0.119, 0.05: 0.146, 0.025: 0.176, 0.01: 0.216}
        assert tst.kpsstest(data, "c")[1] == {0.10: 0.347, 0.05: 0.463, 0.025: 0.574, 0.01: 0.739}
        assert_close(back(tst.dwtest(data)), want_dw, 1e-10, "dwtest panel")
        s, p = tst.lbtest(data, 6)
        assert_close(back(s), want_lb, 2e-10, "lbtest panel")
        check_lb_p(back(s), back(p), 6)
        # one series: scalars
        s, p = tst.adftest(data[0], 2, "c")
        assert isinstance(s, float) and isinstance(p, float)
        assert_close([s], want_adf[:1], 1e-10, "adftest series")
        assert_close([tst.kpsstest(data[0], "ct")[0]], want_kpss[:1], 1e-10, "kpsstest series")
        assert_close([tst.dwtest(data[0])], want_dw[:1], 1e-10, "dwtest series")
        assert_close([tst.lbtest(data[0], 6)[0]], want_lb[:1], 2e-10, "lbtest series")
    rdd = TimeSeriesRDD(None, ["s%d" % i for i in range(7)], xd)
    assert_close(rdd.adftest(2)[0].cpu().numpy(), want_adf, 1e-10, "rdd.adftest")
    assert_close(rdd.kpsstest("ct")[0].cpu().numpy(), want_kpss, 1e-10, "rdd.kpsstest")
    assert_close(rdd.dwtest().cpu().numpy(), want_dw, 1e-10, "rdd.dwtest")
    assert_close(rdd.lbtest(6)[0].cpu().numpy(), want_lb, 2e-10, "rdd.lbtest")
