"""Batched Breusch-Godfrey and Breusch-Pagan tests on the device (sts_bg_test, sts_bp_test and
their `_host` variants) against tests/bgbp_ref.py, the float64 restatement of
S/stats/TimeSeriesStatisticalTests.scala:266-278 and :311-319.

Shapes.  T in {minimum legal, 19, 64, 65, 129, 390, 2520, one past the one-wave limit, 5000},
paired with S exactly as tests/test_stattests_gpu.py pairs them (the kernels give one workgroup to
a series, so S only sets the grid size and the large S ride on the short series); k in {1, 3, 8};
Breusch-Godfrey maxLag in {1, 4, 31} where legal; shared (fs = 0) and per-series factors.

Bars.  Ordinary rows (R^2 of 0.1 .. 0.5): |got - ref| <= 1e-10 |ref|.  Hard rows (residuals at
level 1e4, factors at level 1e6, two factors collinear to 1e-6, a trending factor, and white-noise
residuals whose R^2 is of the order of maxLag / T): |got - exact| <= 1e-10 |exact| + 4 |ref64 - exact|
with `exact` from 60-digit arithmetic (tests/golden/bgbp_exact.json).  p-values: 1e-12 absolute
against the restated chi-squared tail fed the device's own statistic.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import bgbp_ref as br
import layout_arena as la
import stattests_ref as ref
from test_stattests_gpu import S_FOR_T, S_MIN

pytestmark = pytest.mark.gpu
cache = functools.lru_cache(maxsize=None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, BAD_ARG, NOT_ENOUGH_DATA, SINGULAR = 0, 1, 7, 8
T_LIST = ["min", 19, 64, 65, 129, 390, 2520, ref.ONE_WAVE + 1, 5000]
K_LIST = [1, 3, 8]
BG_LAGS = [1, 4, 31]
MODES = ["shared", "per_series"]
POISON_OUT = -3.0e55


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


def hv(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def dev(torch, a, dtype=np.float64):
    return torch.as_tensor(np.array(a, dtype=dtype, order="C"), device="cuda:0")


def factor_panel(F):
    """(T, k) -> (k, T), ld_f = T, fs = 0; (S, T, k) -> (S, k, T), ld_f = T, fs = k T"""
    F = np.asarray(F, dtype=np.float64)
    if F.ndim == 2:
        return np.ascontiguousarray(F.T), F.shape[1], F.shape[0], 0
    return np.ascontiguousarray(F.transpose(0, 2, 1)), F.shape[2], F.shape[1], F.shape[1] * F.shape[2]


def call(torch, e, F, lag=None, want_p=True, err=None, host=False):
    """lag None: Breusch-Pagan.  -> (status, stat, pvalue or None)"""
    e = np.ascontiguousarray(e, dtype=np.float64)
    S, T = e.shape
    fp, k, ld_f, fs = factor_panel(F)
    L = lib()
    if host:
        stat = np.full(S, POISON_OUT)
        pv = np.full(S, POISON_OUT) if want_p else None
        if lag is None:
            st = L.sts_bp_test_host(hv(e), S, T, T, hv(fp), k, ld_f, fs, hv(stat), hv(pv), hv(err))
        else:
            st = L.sts_bg_test_host(hv(e), S, T, T, hv(fp), k, ld_f, fs, lag, hv(stat), hv(pv), hv(err))
        return st, stat, pv
    de, df = dev(torch, e), dev(torch, fp)
    stat = torch.full((S,), POISON_OUT, dtype=torch.float64, device="cuda:0")
    pv = torch.full((S,), POISON_OUT, dtype=torch.float64, device="cuda:0") if want_p else None
    if lag is None:
        st = L.sts_bp_test(vp(de), S, T, T, vp(df), k, ld_f, fs, vp(stat), vp(pv), vp(err), None)
    else:
        st = L.sts_bg_test(vp(de), S, T, T, vp(df), k, ld_f, fs, lag, vp(stat), vp(pv), vp(err), None)
    torch.cuda.synchronize()
    return st, stat.cpu().numpy(), (pv.cpu().numpy() if want_p else None)


def ref_stats(e, F, lag):
    """the per-series numpy checker; F (T, k) or (S, T, k)"""
    F = np.asarray(F)
    out = []
    for s, row in enumerate(e):
        Fs = F if F.ndim == 2 else F[s]
        out.append(br.bp_stat(row, Fs) if lag is None else br.bg_stat(row, Fs, lag))
    return np.array(out)


def assert_close(got, want, rtol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN pattern differs" % what
    fin = ~np.isnan(want)
    if fin.any():
        err = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
        print("%s: max rel err %.3g over %d" % (what, err.max(), int(fin.sum())))
        assert err.max() <= rtol, "%s: max rel err %g > %g (series %d)" % (what, err.max(), rtol, int(np.argmax(err)))


def check_p(stat, pv, dof):
    want = np.array([br.chi2_sf(float(v), dof) for v in stat])
    assert np.array_equal(np.isnan(pv), np.isnan(want))
    fin = ~np.isnan(want)
    assert np.all(np.abs(pv[fin] - want[fin]) <= 1e-12), np.abs(pv[fin] - want[fin]).max()


# ---- inputs and their references, computed once per shape ----

def shape_of(T, k, lag):
    if T == "min":
        return (br.bp_min_T(k) if lag is None else br.bg_min_T(k, lag)), S_MIN
    return T, S_FOR_T[T]


def legal(T, k, lag):
    return T == "min" or T >= (br.bp_min_T(k) if lag is None else br.bg_min_T(k, lag))


@cache
def inputs(T, S, k, lag, mode):
    F = br.factors(5000 + 7 * T + k, T, k, None if mode == "shared" else S)
    e = br.bp_resid(6000 + T, S, T, F) if lag is None else br.bg_resid(7000 + T, S, T)
    want = ref_stats(e, F, lag)
    for a in (F, e, want):
        a.setflags(write=False)
    return e, F, want


# ---- ordinary rows ----

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", K_LIST)
@pytest.mark.parametrize("T", T_LIST)
def test_bp_ordinary(torch, T, k, mode):
    T, S = shape_of(T, k, None)
    e, F, want = inputs(T, S, k, None, mode)
    st, stat, pv = call(torch, e, F)
    assert st == OK
    assert_close(stat, want, 1e-10, "bp k=%d T=%d %s" % (k, T, mode))
    check_p(stat, pv, k)


BG_CASES = [(T, k, lag) for T in T_LIST for k in K_LIST for lag in BG_LAGS if legal(T, k, lag)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,k,lag", BG_CASES)
def test_bg_ordinary(torch, T, k, lag, mode):
    T, S = shape_of(T, k, lag)
    e, F, want = inputs(T, S, k, lag, mode)
    st, stat, pv = call(torch, e, F, lag)
    assert st == OK
    assert_close(stat, want, 1e-10, "bg(%d) k=%d T=%d %s" % (lag, k, T, mode))
    check_p(stat, pv, lag)


# ---- hard rows ----

@cache
def exact_doc():
    with open(os.path.join(ROOT, "tests", "golden", "bgbp_exact.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [390, 2520])
@pytest.mark.parametrize("kind", ["bp", "bg"])
def test_hard_rows(torch, kind, T, mode):
    lag = None if kind == "bp" else br.HARD_LAG
    key = "bp" if kind == "bp" else "bg_%d" % br.HARD_LAG
    idx = [i for i, r in enumerate(br.HARD_ROWS) if r[1] == T]
    rows = [br.hard_row(i) for i in idx]
    exact = np.array([float.fromhex(exact_doc()["rows"][i]["exact"][key]) for i in idx])
    ref64 = np.array([br.bp_stat(e, F) if lag is None else br.bg_stat(e, F, lag) for e, F in rows])
    got = np.empty(len(idx))
    if mode == "shared":       # one call per row: each row has its own factor matrix
        for j, (e, F) in enumerate(rows):
            st, stat, _ = call(torch, e[None, :], F, lag)
            assert st == OK
            got[j] = stat[0]
    else:
        st, got, _ = call(torch, np.stack([e for e, _ in rows]), np.stack([F for _, F in rows]), lag)
        assert st == OK
    bar = 1e-10 * np.abs(exact) + 4 * np.abs(ref64 - exact)
    err = np.abs(got - exact)
    for i, j in enumerate(idx):
        print("%s %s row %s: |got-exact|/|exact| %.3g, |ref64-exact|/|exact| %.3g" % (
            kind, mode, br.HARD_ROWS[j], err[i] / abs(exact[i]), abs(ref64[i] - exact[i]) / abs(exact[i])))
    assert np.all(err <= bar), [br.HARD_ROWS[idx[i]] for i in np.flatnonzero(~(err <= bar))]


# ---- p-values ----

@pytest.mark.parametrize("lag", [None, 4])
def test_statistic_is_bit_identical_without_pvalue(torch, lag):
    e, F, _ = inputs(129, 65, 3, lag, "shared")
    st, stat, pv = call(torch, e[:9], F, lag)
    st2, stat2, pv2 = call(torch, e[:9], F, lag, want_p=False)
    assert st == OK and st2 == OK and pv2 is None
    assert np.array_equal(stat.view(np.uint64), stat2.view(np.uint64))
    check_p(stat, pv, 3 if lag is None else lag)


# ---- the reference suite's two scenarios (TimeSeriesStatisticalTestsSuite.scala:26-85) ----

def test_breusch_godfrey_suite_on_the_device(torch):
    F, r1, r2 = br.suite_bg()
    for lag in (1, 4):
        st, stat, pv = call(torch, np.stack([r1, r2]), F, lag)
        assert st == OK
        assert pv[0] > 0.05 and pv[1] < 0.05
        assert_close(stat, [br.bg_stat(r1, F, lag), br.bg_stat(r2, F, lag)], 1e-10, "suite bg(%d)" % lag)


def test_breusch_pagan_suite_on_the_device(torch):
    F, r1, r2 = br.suite_bp()
    st, stat, pv = call(torch, np.stack([r1, r2]), F)
    assert st == OK
    assert pv[0] > 0.05 and pv[1] < 0.05
    assert_close(stat, [br.bp_stat(r1, F), br.bp_stat(r2, F)], 1e-10, "suite bp")


# ---- shared against per-series ----

@pytest.mark.parametrize("T", [129, ref.ONE_WAVE + 1])
@pytest.mark.parametrize("lag", [None, 4])
def test_shared_and_replicated_factors_agree(torch, T, lag):
    S = S_FOR_T[T]
    e, F, want = inputs(T, S, 3, lag, "shared")
    st1, shared, _ = call(torch, e, F, lag)
    st2, repl, _ = call(torch, e, np.broadcast_to(F, (S,) + F.shape), lag)
    assert st1 == OK and st2 == OK
    assert_close(shared, want, 1e-10, "shared")
    assert_close(repl, want, 1e-10, "replicated")


# ---- the scratch's chunk seam ----

@pytest.mark.parametrize("lag", [None, 4])
def test_basis_chunk_seam(torch, lag):
    """Per-series factors one chunk of scratch bases and more: k = 8, T = 8192 is 524 288 bytes per basis
    (BP; 524 032 at lag 4), 512 bases to the 256 MiB bound, so S = 600 takes two chunks (512 + 88).  The
    series around the seam and at the ends against the restatement and, bit for bit, against a call of
    their own (S = 1)."""
    S, T, k = 600, 8192, 8
    F = br.factors(99, T, k, S)
    e = br.bp_resid(98, S, T, F) if lag is None else br.bg_resid(97, S, T)
    err = torch.full((S,), -1, dtype=torch.int32, device="cuda:0")
    st, stat, _ = call(torch, e, F, lag, want_p=False, err=err)
    assert st == OK and not err.cpu().numpy().any()
    assert np.isfinite(stat).all()
    rows = [0, 511, 512, 513, 599]
    assert_close(stat[rows], ref_stats(e[rows], F[rows], lag), 1e-10, "chunk seam, lag %s" % lag)
    for s in rows:
        st, one, _ = call(torch, e[s:s + 1], F[s:s + 1], lag, want_p=False)
        assert st == OK and one.view(np.uint64)[0] == stat.view(np.uint64)[s], s


# ---- per-series outcomes ----

NB_T, NB_S, NB_K, NB_LAG = 129, 6, 3, 4


def neighbours(lag, mode):
    e, F, want = inputs(NB_T, S_FOR_T[NB_T], NB_K, lag, mode)
    return e[:NB_S].copy(), (F.copy() if mode == "shared" else F[:NB_S].copy()), want[:NB_S]


@pytest.mark.parametrize("lag", [None, NB_LAG])
def test_nan_gives_nan_with_status_zero(torch, lag):
    dof = NB_K if lag is None else lag
    # a NaN in one series' residuals (for BG: once among the first maxLag values, read by the lags only)
    e, F, want = neighbours(lag, "shared")
    e[1, 40] = np.nan
    e[4, 0] = np.nan
    err = torch.full((NB_S,), -1, dtype=torch.int32, device="cuda:0")
    st, stat, pv = call(torch, e, F, lag, err=err)
    assert st == OK and err.cpu().numpy().tolist() == [0] * NB_S
    want = want.copy()
    want[[1, 4]] = np.nan
    assert_close(stat, want, 1e-10, "next to NaN residuals")
    assert np.isnan(pv[[1, 4]]).all()
    check_p(stat, pv, dof)
    # a NaN in one series' own factors
    e, F, want = neighbours(lag, "per_series")
    F[2, 77, 1] = np.nan
    err.fill_(-1)
    st, stat, pv = call(torch, e, F, lag, err=err)
    assert st == OK and err.cpu().numpy().tolist() == [0] * NB_S
    want = want.copy()
    want[2] = np.nan
    assert_close(stat, want, 1e-10, "next to NaN factors")
    assert np.isnan(pv[2])
    # a NaN in the shared matrix: every series
    e, F, want = neighbours(lag, "shared")
    F[50, 2] = np.nan
    err.fill_(-1)
    st, stat, pv = call(torch, e, F, lag, err=err)
    assert st == OK and err.cpu().numpy().tolist() == [0] * NB_S
    assert np.isnan(stat).all() and np.isnan(pv).all()


def test_bg_ignores_factor_rows_it_does_not_read(torch):
    """Rows 0 .. maxLag - 1 of the factors are dropped with the residuals' (lagMatTrimBoth)."""
    e, F, want = neighbours(NB_LAG, "shared")
    F[:NB_LAG] = np.nan
    st, stat, _ = call(torch, e, F, NB_LAG)
    assert st == OK
    assert_close(stat, want, 1e-10, "NaN in the dropped factor rows")


@pytest.mark.parametrize("lag", [None, NB_LAG])
def test_bit_constant_response_gives_nan_with_status_zero(torch, lag):
    e, F, want = neighbours(lag, "shared")
    if lag is None:
        e[2] = 1.5 * (-1.0) ** (np.arange(NB_T) // 3)      # e^2 all equal
    else:
        e[2, lag:] = -0.75                                  # the response window; the lags still vary
    err = torch.full((NB_S,), -1, dtype=torch.int32, device="cuda:0")
    st, stat, pv = call(torch, e, F, lag, err=err)
    assert st == OK and err.cpu().numpy().tolist() == [0] * NB_S
    want = want.copy()
    want[2] = np.nan
    assert_close(stat, want, 1e-10, "next to a constant response")
    assert np.isnan(pv[2])


@pytest.mark.parametrize("lag", [None, NB_LAG])
def test_singular_designs(torch, lag):
    e, F, want = neighbours(lag, "per_series")
    lo = 0 if lag is None else lag
    F[1, lo:, 2] = 3.25            # bit-constant over the rows used (for BG the dropped rows still vary)
    F[3, :, 1] = F[3, :, 0]        # two bit-identical factor rows
    F[4, :, 2] = F[4, :, 1]
    err = torch.full((NB_S,), -1, dtype=torch.int32, device="cuda:0")
    st, stat, pv = call(torch, e, F, lag, err=err)
    assert st == OK
    assert err.cpu().numpy().tolist() == [0, SINGULAR, 0, SINGULAR, SINGULAR, 0]
    assert np.isnan(stat[[1, 3, 4]]).all() and np.isnan(pv[[1, 3, 4]]).all()
    assert_close(stat[[0, 2, 5]], want[[0, 2, 5]], 1e-10, "neighbours of singular designs")
    st, _, _ = call(torch, e, F, lag)                      # no err array: the first failure is the return
    assert st == SINGULAR
    assert b"series 1" in lib().sts_last_error()
    herr = np.full(NB_S, -1, dtype=np.int32)                # the _host path: the same statuses
    st, hstat, _ = call(torch, e, F, lag, err=herr, host=True)
    assert st == OK and herr.tolist() == [0, SINGULAR, 0, SINGULAR, SINGULAR, 0]
    assert_close(hstat[[0, 2, 5]], want[[0, 2, 5]], 1e-10, "_host neighbours of singular designs")
    st, _, _ = call(torch, e, F, lag, host=True)
    assert st == SINGULAR and b"series 1" in lib().sts_last_error()
    # a shared matrix with a duplicated factor: every series
    e, F, _ = neighbours(lag, "shared")
    F[:, 2] = F[:, 0]
    err.fill_(-1)
    st, stat, pv = call(torch, e, F, lag, err=err)
    assert st == OK and err.cpu().numpy().tolist() == [SINGULAR] * NB_S
    assert np.isnan(stat).all() and np.isnan(pv).all()


def test_bg_constant_residuals_are_a_constant_response_not_a_singular_design(torch):
    e, F, _ = neighbours(NB_LAG, "shared")
    e[3] = 2.0
    err = torch.full((NB_S,), -1, dtype=torch.int32, device="cuda:0")
    st, stat, _ = call(torch, e, F, NB_LAG, err=err)
    assert st == OK and err.cpu().numpy().tolist() == [0] * NB_S and np.isnan(stat[3])


# ---- call-level errors ----

def test_call_level_errors_leave_outputs_alone(torch):
    """Every call-level error, from the device and the `_host` entry points, with poisoned outputs."""
    S, T, k = 4, 40, 3
    e = br.bg_resid(1, S, T)
    fp = np.ascontiguousarray(br.factors(2, T, 8, S).transpose(0, 2, 1))     # (S, 8, T)
    L = lib()
    de, df = dev(torch, e), dev(torch, fp)
    dstat = torch.full((S,), POISON_OUT, dtype=torch.float64, device="cuda:0")
    dpv = dstat.clone()
    hstat, hpv = np.full(S, POISON_OUT), np.full(S, POISON_OUT)
    fs = 8 * T
    base = dict(T=T, ld=T, k=k, ld_f=T, fs=fs, lag=2)
    cases = [  # (which tests, overrides, status)
        ("both", dict(k=0), BAD_ARG), ("both", dict(k=9), BAD_ARG),
        ("bg", dict(lag=0), BAD_ARG), ("bg", dict(lag=32), BAD_ARG),
        ("both", dict(ld=T - 1), BAD_ARG), ("both", dict(ld_f=T - 1), BAD_ARG),
        ("both", dict(fs=(k - 1) * T + T - 1), BAD_ARG),          # the next series starts inside the last factor row
        ("both", dict(fs=-fs), BAD_ARG),
        ("bp", dict(T=1 + k), NOT_ENOUGH_DATA),                   # observations == columns
        ("bg", dict(T=2 + 1 + k + 2), NOT_ENOUGH_DATA),           # nObs == 1 + k + maxLag
    ]
    for which, over, status in cases:
        c = dict(base, **over)
        if which in ("both", "bp"):
            assert L.sts_bp_test(vp(de), S, c["T"], c["ld"], vp(df), c["k"], c["ld_f"], c["fs"], vp(dstat), vp(dpv), None,
                                 None) == status, over
            assert L.sts_bp_test_host(hv(e), S, c["T"], c["ld"], hv(fp), c["k"], c["ld_f"], c["fs"], hv(hstat), hv(hpv),
                                      None) == status, over
        if which in ("both", "bg"):
            assert L.sts_bg_test(vp(de), S, c["T"], c["ld"], vp(df), c["k"], c["ld_f"], c["fs"], c["lag"], vp(dstat),
                                 vp(dpv), None, None) == status, over
            assert L.sts_bg_test_host(hv(e), S, c["T"], c["ld"], hv(fp), c["k"], c["ld_f"], c["fs"], c["lag"], hv(hstat),
                                      hv(hpv), None) == status, over
    torch.cuda.synchronize()
    assert bool((dstat == POISON_OUT).all()) and bool((dpv == POISON_OUT).all())
    assert (hstat == POISON_OUT).all() and (hpv == POISON_OUT).all()
    # one more observation than columns is legal
    assert L.sts_bp_test(vp(de), S, 2 + k, T, vp(df), k, T, fs, vp(dstat), vp(dpv), None, None) == OK
    assert L.sts_bg_test(vp(de), S, 2 + 2 + k + 2, T, vp(df), k, T, fs, 2, vp(dstat), vp(dpv), None, None) == OK
    torch.cuda.synchronize()
    assert not bool((dstat == POISON_OUT).any())


# ---- layout contract (tests/layout_arena.py) ----

LAY_S, LAY_T, LAY_K, LAY_LAG = 5, 131, 3, 3


def factor_arena(carve, lay, poison, F, mode):
    """The factor panel as an arena of rows of T: shared -> k rows; per series -> S groups of k + 1
    rows whose last row is all poison, i.e. fs = (k + 1) ld_f > k ld_f."""
    ld_f, _, base, _ = la.layout(lay, LAY_T)
    ld_f += 2                                   # another odd padding than the residuals'
    if mode == "shared":
        return carve(LAY_K, LAY_T, ld_f, base, poison, data=np.ascontiguousarray(F.T)), ld_f, 0
    rows = np.full((LAY_S, LAY_K + 1, LAY_T), poison)
    rows[:, :LAY_K] = F.transpose(0, 2, 1)
    a = carve(LAY_S * (LAY_K + 1), LAY_T, ld_f, base, poison, data=rows.reshape(-1, LAY_T))
    return a, ld_f, (LAY_K + 1) * ld_f


@pytest.mark.parametrize("poison", list(la.POISONS))
@pytest.mark.parametrize("lay", ["odd", "skew"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", ["bp", "bg"])
def test_layout(torch, name, host, mode, lay, poison):
    lag = None if name == "bp" else LAY_LAG
    F = br.factors(81, LAY_T, LAY_K, None if mode == "shared" else LAY_S)
    e = br.bp_resid(82, LAY_S, LAY_T, F) if lag is None else br.bg_resid(83, LAY_S, LAY_T)
    carve = la.carve_np if host else la.carve
    ld, _, base, _ = la.layout(lay, LAY_T)
    a = carve(LAY_S, LAY_T, ld, base, la.POISONS[poison], data=e)
    fa, ld_f, fs = factor_arena(carve, lay, la.POISONS[poison], F, mode)
    so, po = carve(1, LAY_S, LAY_S, 0, la.OUT_FILL, red=64), carve(1, LAY_S, LAY_S, 0, la.OUT_FILL, red=64)
    snap, fsnap, ssnap, psnap = a.snapshot(), fa.snapshot(), so.snapshot(), po.snapshot()
    cp = ctypes.c_void_p
    L = lib()
    tail = () if host else (None,)
    if lag is None:
        fn = L.sts_bp_test_host if host else L.sts_bp_test
        st = fn(cp(a.ptr), LAY_S, LAY_T, ld, cp(fa.ptr), LAY_K, ld_f, fs, cp(so.ptr), cp(po.ptr), None, *tail)
    else:
        fn = L.sts_bg_test_host if host else L.sts_bg_test
        st = fn(cp(a.ptr), LAY_S, LAY_T, ld, cp(fa.ptr), LAY_K, ld_f, fs, lag, cp(so.ptr), cp(po.ptr), None, *tail)
    torch.cuda.synchronize()
    assert st == OK
    a.verify_all(snap, "residual arena")
    fa.verify_all(fsnap, "factor arena")
    so.verify_outside(ssnap)
    po.verify_outside(psnap)
    stat = so.data()[0]
    assert_close(stat, ref_stats(e, F, lag), 1e-10, "%s %s %s %s" % (name, mode, lay, poison))
    check_p(stat, po.data()[0], LAY_K if lag is None else lag)


# ---- Python mirror ----

def test_python_mirror(torch):
    from sparkts.stats import factor_tests as tst
    from sparkts.timeseriesrdd import TimeSeriesRDD
    S, T, k, lag = 7, 129, 3, 4
    F = br.factors(91, T, k)
    Fs = br.factors(92, T, k, S)
    e_bg, e_bp = br.bg_resid(93, S, T), br.bp_resid(94, S, T, F)
    want = {("bg", "shared"): ref_stats(e_bg, F, lag), ("bg", "per"): ref_stats(e_bg, Fs, lag),
            ("bp", "shared"): ref_stats(e_bp, F, None), ("bp", "per"): ref_stats(e_bp, Fs, None)}
    kt = np.ascontiguousarray(F.T)                      # (k, T): its transpose is a stride-1 view
    skt = np.ascontiguousarray(Fs.transpose(0, 2, 1))   # (S, k, T)
    for to, back, swap in ((lambda a: a, np.asarray, lambda a: a.transpose(0, 2, 1)),
                           (lambda a: dev(torch, a), lambda v: v.cpu().numpy(), lambda a: a.transpose(1, 2))):
        ebg, ebp = to(e_bg), to(e_bp)
        # (T, k) row-major forces the one copy; the transposed (k, T) is passed as a view
        for fac in (to(F), to(kt).T):
            s, p = tst.bgtest(ebg, fac, lag)
            assert_close(back(s), want["bg", "shared"], 1e-10, "bgtest panel")
            check_p(back(s), back(p), lag)
            s, p = tst.bptest(ebp, fac)
            assert_close(back(s), want["bp", "shared"], 1e-10, "bptest panel")
            check_p(back(s), back(p), k)
        for fac in (to(Fs), swap(to(skt))):
            s, p = tst.bgtest(ebg, fac, lag)
            assert_close(back(s), want["bg", "per"], 1e-10, "bgtest panel, per-series factors")
            s, p = tst.bptest(ebp, fac)
            assert_close(back(s), want["bp", "per"], 1e-10, "bptest panel, per-series factors")
            check_p(back(s), back(p), k)
        # one series: floats
        s, p = tst.bgtest(ebg[0], to(F), lag)
        assert isinstance(s, float) and isinstance(p, float)
        assert_close([s], want["bg", "shared"][:1], 1e-10, "bgtest series")
        s, p = tst.bptest(ebp[0], to(F))
        assert isinstance(s, float) and isinstance(p, float)
        assert_close([s], want["bp", "shared"][:1], 1e-10, "bptest series")
    from sparkts.errors import IllegalArgumentException
    with pytest.raises(IllegalArgumentException):        # torch residuals, numpy factors
        tst.bptest(dev(torch, e_bp), F)
    with pytest.raises(IllegalArgumentException):        # factors on another device than the residuals
        tst.bgtest(dev(torch, e_bg), torch.as_tensor(F), lag)
    rdd = TimeSeriesRDD(None, ["s%d" % i for i in range(S)], dev(torch, e_bg))
    assert_close(rdd.bgtest(dev(torch, F), lag)[0].cpu().numpy(), want["bg", "shared"], 1e-10, "rdd.bgtest")
    rdd = TimeSeriesRDD(None, ["s%d" % i for i in range(S)], dev(torch, e_bp))
    assert_close(rdd.bptest(dev(torch, Fs))[0].cpu().numpy(), want["bp", "per"], 1e-10, "rdd.bptest")
