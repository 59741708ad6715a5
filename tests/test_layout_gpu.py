"""The panel-layout contract of include/sts.h ("Panel layout") on every device entry point that
takes a panel, through the C ABI, so that `ld` and the pointers are exactly what the test chose.
Needs an MI355X.

Every case runs in every named layout of tests/layout_arena.py (packed, even, odd,
in_fast_out_slow, in_slow_out_fast, skew) with both poisons (NaN and a finite sentinel) around
the panel, and asserts

  * the result equals the oracle at the bar of the operator's packed test (index-driven work and
    reference-order recurrences bit-exact; ACF and AR coefficients 1e-10 relative with identical
    NaN patterns; noIntercept AR fits bit-identical to oracle.ar_fit),
  * err_per_series equals the oracle's,
  * the output arena is unchanged outside (s, t < T): row padding, skew and both red zones,
  * the input arena is unchanged everywhere.

One test id is one operator x one layout; shapes and poisons loop inside.  References are
computed once per shape (lru_cache) and shared by the layouts.  Two layouts are never compared
with each other: different layouts legitimately run different kernels.

Entry points that take a panel and are not in this matrix, with the test that sweeps their
layouts:
  sts_ar_rule_count                              diagnostic; it launches the kernels of sts_ar_fit, swept here
  sts_fill_autocorr_host, sts_fill_host, sts_fill_diff_ewma_host   test_staging.py, test_fuzz_gpu.py
sts_series_stats and the EWMA fit are swept for row offsets by
test_parity_gpu.py::test_stats_and_ewma_row_alignments; here they get the red-zone and
unchanged-input assertions.
"""
import ctypes
import functools

import numpy as np
import pytest

import layout_arena as la
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-10
NaN = np.nan
LAYOUT = pytest.mark.parametrize("lay", la.LAYOUT_NAMES)
cache = functools.lru_cache(maxsize=None)


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


# ---------------- assertions (the bars of test_parity_gpu.py) ----------------

def assert_bits(got, ref, what=""):
    got = np.ascontiguousarray(got, dtype=np.float64)
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = (got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))
    if not same.all():
        idx = np.argwhere(~same)[:5]
        raise AssertionError("%s: %d mismatches, first %s got %s ref %s" % (
            what, (~same).sum(), idx.tolist(), [got[tuple(i)] for i in idx], [ref[tuple(i)] for i in idx]))


def assert_rel(got, ref, rtol=RTOL, what=""):
    got = np.asarray(got)
    ref = np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN pattern differs" % what
    fin = ~np.isnan(ref)
    if fin.any():
        err = np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-300)
        assert err.max() <= rtol, "%s: max rel err %g > %g" % (what, err.max(), rtol)


# ---------------- arenas and the checked call ----------------

def arena_in(x, ld, base, poison):
    S, T = x.shape
    return la.carve(S, T, ld, base, la.POISONS[poison], data=x)


def arena_out(S, T, ld, base):
    return la.carve(S, T, ld, base, la.OUT_FILL)


def vec_out(n):
    """A flat output array (acf, coefficients, a lag matrix ...) with red zones of its own."""
    return la.carve(1, n, n, 0, la.OUT_FILL, red=64)


def dvec(torch, v, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(v, dtype=dtype), device="cuda:0")


def err_dev(torch, S):
    return torch.full((S,), -1, dtype=torch.int32, device="cuda:0")


def run(torch, what, fn, args, ins=(), outs=()):
    """fn(*args) == STS_OK, then: inputs bit-identical everywhere, outputs bit-identical outside
    their (s, t < T) elements."""
    before_in = [a.snapshot() for a in ins]
    before_out = [a.snapshot() for a in outs]
    st = fn(*args)
    assert st == 0, (what, st, lib().sts_last_error())
    torch.cuda.synchronize()
    for a, snap in zip(ins, before_in):
        a.verify_all(snap, what + ": input arena")
    for a, snap in zip(outs, before_out):
        a.verify_outside(snap, what + ": output arena")


def cases(*lists):
    """Cartesian product with both poisons last."""
    import itertools
    return itertools.product(*lists, sorted(la.POISONS))


# ---------------- fills (a1-a5): bit-exact ----------------
# T = 1, 3, 64, 65, 390, 2520, 4097: the segment kernel (sts_seg.hip, T <= 16384) on 16-B aligned
# panels with even ld, the workgroup tile kernel (sts_tile.hip) in every other layout -- the only
# way the product dispatch sends small T there (run_tile); T = 16386 > 16384: the tile kernel in
# every layout, its 16-B forms when aligned.  Spline: spline_lds_kernel needs an even ld
# (sts_spline.hip), the odd layouts take its global-memory form.
FILL_T = [1, 3, 64, 65, 390, 2520, 4097, 16386]
FILL_S = 5


@cache
def fill_case(method, T):
    x = oracle.gen_panel(100 + T, FILL_S, T, 0.05)
    if T >= 3:
        x[1, 0] = NaN            # a series that starts missing: nothing before it but the skew / padding
        x[2, T - 1] = NaN        # ends missing: the next value in memory is row padding
        x[3, T // 2] = NaN
    if method == "nearest":
        x[4, :] = NaN            # Input is all NaNs!: the error array
    ref, err = oracle.panel_fill(x, method)
    return x, ref, err


@LAYOUT
@pytest.mark.parametrize("method", ["linear", "previous", "next", "nearest", "spline"])
def test_fill(torch, method, lay):
    code = oracle.FILL_METHODS[method]
    for T, poison in cases(FILL_T):
        x, ref, rerr = fill_case(method, T)
        ld_in, ld_out, b_in, b_out = la.layout(lay, T)
        what = "fill %s T=%d %s %s" % (method, T, lay, poison)
        a, o, e = arena_in(x, ld_in, b_in, poison), arena_out(FILL_S, T, ld_out, b_out), err_dev(torch, FILL_S)
        run(torch, what, lib().sts_fill, (a.ptr, o.ptr, FILL_S, T, ld_in, ld_out, code, e.data_ptr(), None), [a], [o])
        assert np.array_equal(e.cpu().numpy(), rerr), (what, e.cpu().numpy(), rerr)
        ok = rerr == 0
        assert_bits(o.data()[ok], ref[ok], what)


# ---------------- fused fill + ACF (C1 / C3, a8): fill bit-exact, ACF 1e-10 ----------------
# K = 24 | 25: either side of short_ok's bound (sts_short.hip: linear / previous, even T <= 2560,
# aligned); K = 63 | 64: either side of kFusedMaxLags (fused partials | sts_acf_wide.hip);
# K = 130: three 61-lag wide blocks.  T = 130, 390, 2520: short kernel (K <= 24) or one-segment
# seg kernel with the fused finalize; T = 2562: past the short kernel's 2560; T = 4097: nine
# 512-step seg tiles, the last one of a single step (no fused finalize: last_len < 64);
# T = 16386: tile kernel.  Misaligned layouts: tile kernel + partials + finalize at every T.
# (100, 60): T <= 2K, the exact-loop path.  STS_FILL_NONE: filled == NULL, the sts_autocorr path.
ACF_S = 5
ACF_TK = ([(T, K) for T in (130, 390, 2520, 2562, 4097) for K in (1, 20, 24, 25, 60, 63, 64, 130)]
          + [(16386, 20), (16386, 64), (100, 60)])


@cache
def acf_case(method, T, K):
    if method is None:
        rng = np.random.default_rng(K * 100003 + T)          # test_autocorr_panels's walk
        x = 50.0 + rng.standard_normal((ACF_S, T)).cumsum(axis=1) * 0.5 + rng.standard_normal((ACF_S, T))
        return x, None, np.array([oracle.autocorr(r, K) for r in x]), np.zeros(ACF_S, np.int32)
    x = oracle.gen_panel(3 + T + K, ACF_S, T, 0.05)          # test_fill_autocorr_fused's panels
    rf, racf, err = oracle.panel_fill_autocorr(x, method, K)
    return x, rf, racf, err


@LAYOUT
@pytest.mark.parametrize("method", ["linear", "previous", None])
def test_fill_autocorr(torch, method, lay):
    for (T, K), poison in cases(ACF_TK):
        x, rf, racf, rerr = acf_case(method, T, K)
        ld_in, ld_out, b_in, b_out = la.layout(lay, T)
        what = "fill_autocorr %s T=%d K=%d %s %s" % (method, T, K, lay, poison)
        a, acf = arena_in(x, ld_in, b_in, poison), vec_out(ACF_S * K)
        if method is None:
            run(torch, what, lib().sts_autocorr, (a.ptr, ACF_S, T, ld_in, K, acf.ptr, None), [a], [acf])
        else:
            o, e = arena_out(ACF_S, T, ld_out, b_out), err_dev(torch, ACF_S)
            run(torch, what, lib().sts_fill_autocorr,
                (a.ptr, o.ptr, ACF_S, T, ld_in, ld_out, oracle.FILL_METHODS[method], K, acf.ptr, e.data_ptr(), None),
                [a], [o, acf])
            assert np.array_equal(e.cpu().numpy(), rerr), (what, e.cpu().numpy(), rerr)
            assert_bits(o.data(), rf, what + " filled")
        assert_rel(acf.data().reshape(ACF_S, K), racf, what=what)


# ---------------- lag matrices (a7, C5): bit-exact ----------------
# sts_lag_matrix: lagmat_kernel; sts_fill_lag_matrix: the tile kernel's lag-matrix store
# (sts_tile.hip), whose 16-B form depends on the parity of each column's first element: the lag
# matrix sits at an even and at an odd double offset.  T = 11 = max_lag + 1: one-row blocks.
LAG_S = 5
LAG_T = [11, 64, 65, 4097]


@cache
def lag_case(method, T):
    x = oracle.gen_panel(5 + T, LAG_S, T, 0.3)
    x[:, 1] = 1.0
    f = x if method is None else oracle.panel_fill(x, method)[0]
    mats = {(p, inc): np.concatenate([oracle.lag(r, p, bool(inc)).T.ravel() for r in f])
            for p in (1, 2, 10) for inc in (0, 1)}
    return x, f, mats


@LAYOUT
@pytest.mark.parametrize("method", [None, "next", "linear"])
def test_lag_matrix(torch, method, lay):
    for T, p, inc, lm_base, with_filled, poison in cases(LAG_T, (1, 2, 10), (0, 1), (0, 1), (True, False)):
        if method is None and not with_filled:
            continue                                      # sts_lag_matrix has no filled panel
        x, f, mats = lag_case(method, T)
        ref = mats[(p, inc)]
        ld_in, ld_out, b_in, b_out = la.layout(lay, T)
        what = "lag %s T=%d p=%d inc=%d lm_base=%d filled=%s %s %s" % (method, T, p, inc, lm_base, with_filled, lay, poison)
        a = arena_in(x, ld_in, b_in, poison)
        lm = la.carve(1, ref.size, ref.size, lm_base, la.OUT_FILL, red=64)
        if method is None:
            run(torch, what, lib().sts_lag_matrix, (a.ptr, lm.ptr, LAG_S, T, ld_in, p, inc, None), [a], [lm])
        else:
            o = arena_out(LAG_S, T, ld_out, b_out) if with_filled else None
            e = err_dev(torch, LAG_S)
            run(torch, what, lib().sts_fill_lag_matrix,
                (a.ptr, o.ptr if o else None, lm.ptr, LAG_S, T, ld_in, ld_out, oracle.FILL_METHODS[method], p, inc,
                 e.data_ptr(), None), [a], [lm] + ([o] if o else []))
            assert (e.cpu().numpy() == 0).all(), what
            if o:
                assert_bits(o.data(), f, what + " filled")
        assert_bits(lm.data().ravel(), ref, what)


# ---------------- AR fits (a11, C4) ----------------
# register kernel ar_fit_blk_kernel (p <= 8, T <= 2560): per row LDS-DMA loads | 16-B register
# loads | clamped 8-B loads, and independently for the fused-remove output DMA | double2 | scalar
# stores; T = 2p + 1: the smallest design; 64 | 65: one lane block edge; 2559 | 2560: its limit.
# staged / MFMA kernel ar_fit_kernel: p = 5 at T = 2561 (first T past the register kernel), p = 9
# at T = 200 and 2561.  The residual panel of sts_ar_fit_remove is an output arena with
# ld_out != ld_in.  Row 2 holds a NaN: a NaN model, the other rows unaffected.
AR_S = 5


@cache
def ar_case(p, T, no_intercept):
    x = oracle.gen_ar_panel(7, AR_S, T, min(p, 5)) + 0.01 * np.sin(np.arange(T))[None, :]
    x[2, max(T - 3, 0)] = NaN
    rc = np.empty(AR_S)
    rcoef = np.empty((AR_S, p))
    for s in range(AR_S):
        rc[s], rcoef[s] = oracle.ar_fit(x[s], p, bool(no_intercept))     # row 2: NaN, no exception
    return x, rc, rcoef


def check_ar(torch, p, T, no_intercept, lay, poison):
    x, rc, rcoef = ar_case(p, T, no_intercept)
    ld_in, ld_out, b_in, b_out = la.layout(lay, T)
    ok = [0, 1, 3, 4]
    for fused in (False, True):
        what = "ar_fit%s p=%d T=%d noint=%d %s %s" % ("_remove" if fused else "", p, T, no_intercept, lay, poison)
        a, c, coef, e = arena_in(x, ld_in, b_in, poison), vec_out(AR_S), vec_out(AR_S * p), err_dev(torch, AR_S)
        if fused:
            o = arena_out(AR_S, T, ld_out, b_out)
            run(torch, what, lib().sts_ar_fit_remove,
                (a.ptr, o.ptr, AR_S, T, ld_in, ld_out, p, no_intercept, c.ptr, coef.ptr, e.data_ptr(), None),
                [a], [o, c, coef])
        else:
            run(torch, what, lib().sts_ar_fit,
                (a.ptr, AR_S, T, ld_in, p, no_intercept, c.ptr, coef.ptr, e.data_ptr(), None), [a], [c, coef])
        assert (e.cpu().numpy() == 0).all(), (what, e.cpu().numpy())      # the oracle raises for no row
        gc, gcoef = c.data().ravel(), coef.data().reshape(AR_S, p)
        if not no_intercept:
            assert np.isnan(gc[2]) and np.isnan(gcoef[2]).all(), what + ": the NaN row must give a NaN model"
        if no_intercept:
            assert_bits(gcoef, rcoef, what + " coef (reference-order QR)")
        else:
            assert_rel(gcoef, rcoef, what=what + " coef")
            assert_rel(gc, rc, what=what + " c")
        if fused:   # bit-exact given the fitted model
            ref = np.array([oracle.ar_remove(x[s], gc[s], gcoef[s]) for s in ok])
            assert_bits(o.data()[ok], ref, what + " residuals")


@LAYOUT
@pytest.mark.parametrize("p", [1, 5, 8])
def test_ar_fit_register_kernel(torch, p, lay):
    for T, poison in cases((2 * p + 1, 64, 65, 1000, 2520, 2559, 2560)):
        check_ar(torch, p, T, 0, lay, poison)


@LAYOUT
def test_ar_fit_staged_kernel(torch, lay):
    for (p, T), poison in cases(((5, 2561), (9, 200), (9, 2561))):
        check_ar(torch, p, T, 0, lay, poison)


@LAYOUT
@pytest.mark.parametrize("p", [8, 9])
def test_ar_fit_no_intercept_qr(torch, p, lay):
    # either side of ar_qr_lane_ok (p <= 8): ar_qr_lane_kernel (one lane per series) | the
    # one-wave-per-series QR on a scratch design matrix
    for T, poison in cases((2 * p + 1, 64, 65, 1000)):
        check_ar(torch, p, T, 1, lay, poison)


# ARIMA(p, d, 0): differencesOfOrderD into packed scratch panels, then the AR fit on a view
# that starts d doubles into each row (sts_arima_fit_ar); only the input panel is the caller's.
@cache
def arima_case(p, d, inc):
    rng = np.random.default_rng(p * 10 + d)                  # test_arima_ar_path's first rows
    S, T = 5, 800
    x = np.empty((S, T))
    ref = []
    for s in range(S):
        y = oracle.ar_add(rng.standard_normal(T), 0.3, [0.5 / p] * p, inplace=True)
        for _ in range(d):
            y = np.cumsum(y)
        x[s] = y + 50.0
        c, coef = oracle.ar_fit(oracle.differences_of_order_d(x[s], d)[d:], p, no_intercept=not inc)
        ref.append(([c] if inc else []) + list(coef))
    return x, np.array(ref)


@LAYOUT
def test_arima_fit_ar(torch, lay):
    S, T = 5, 800
    for (p, d, inc), poison in cases(((1, 1, True), (2, 1, False), (3, 2, True))):
        x, ref = arima_case(p, d, inc)
        ld, _, base, _ = la.layout(lay, T)
        what = "arima p=%d d=%d inc=%s %s %s" % (p, d, inc, lay, poison)
        a, c, coef, e = arena_in(x, ld, base, poison), vec_out(S), vec_out(S * p), err_dev(torch, S)
        run(torch, what, lib().sts_arima_fit_ar,
            (a.ptr, S, T, ld, p, d, int(inc), c.ptr, coef.ptr, e.data_ptr(), None), [a], [c, coef])
        assert (e.cpu().numpy() == 0).all(), what
        got = coef.data().reshape(S, p)
        if inc:
            got = np.concatenate([c.data().reshape(S, 1), got], axis=1)
        assert_rel(got, ref, what=what)


# ---------------- out-of-place recurrences (a6, a10, a12): bit-exact ----------------
# test_recur_shapes.py runs these padded but in place; out of place they are diff_kernel,
# ewma_remove_kernel and ar_remove_kernel (index-driven, 16-B forms on aligned even rows).
REC_S = 7
REC_T = [2, 129, 390]


@cache
def rec_case(T):
    rng = np.random.default_rng(1000 + T)
    x = rng.standard_normal((REC_S, T)) + 10
    sm = rng.uniform(0.05, 0.95, REC_S)
    c = rng.standard_normal(REC_S)
    coef = {p: rng.uniform(-0.3, 0.3, (REC_S, p)) for p in (1, 8, 16)}
    return x, sm, c, coef


@LAYOUT
@pytest.mark.parametrize("lag,start", [(1, 1), (3, 7), (40, 40)])
def test_diff_out_of_place(torch, lag, start, lay):
    for T, poison in cases(REC_T):
        x = rec_case(T)[0]
        ld_in, ld_out, b_in, b_out = la.layout(lay, T)
        what = "diff lag=%d start=%d T=%d %s %s" % (lag, start, T, lay, poison)
        a, o = arena_in(x, ld_in, b_in, poison), arena_out(REC_S, T, ld_out, b_out)
        run(torch, what, lib().sts_diff_at_lag, (a.ptr, o.ptr, REC_S, T, ld_in, ld_out, lag, start, None), [a], [o])
        assert_bits(o.data(), np.array([oracle.differences_at_lag(r, lag, start=start) for r in x]), what)


@LAYOUT
def test_ewma_remove_out_of_place(torch, lay):
    for T, poison in cases(REC_T):
        x, sm, _, _ = rec_case(T)
        ld_in, ld_out, b_in, b_out = la.layout(lay, T)
        what = "ewma_remove T=%d %s %s" % (T, lay, poison)
        a, o = arena_in(x, ld_in, b_in, poison), arena_out(REC_S, T, ld_out, b_out)
        smd = dvec(torch, sm)
        run(torch, what, lib().sts_ewma_remove, (a.ptr, o.ptr, REC_S, T, ld_in, ld_out, smd.data_ptr(), None), [a], [o])
        assert_bits(o.data(), np.array([oracle.ewma_remove(r, v) for r, v in zip(x, sm)]), what)


@LAYOUT
@pytest.mark.parametrize("p", [1, 8, 16])
def test_ar_remove_out_of_place(torch, p, lay):
    for T, poison in cases(REC_T):
        x, _, c, coefs = rec_case(T)
        coef = coefs[p]
        ld_in, ld_out, b_in, b_out = la.layout(lay, T)
        what = "ar_remove p=%d T=%d %s %s" % (p, T, lay, poison)
        a, o = arena_in(x, ld_in, b_in, poison), arena_out(REC_S, T, ld_out, b_out)
        cd, fd = dvec(torch, c), dvec(torch, coef)
        run(torch, what, lib().sts_ar_remove,
            (a.ptr, o.ptr, REC_S, T, ld_in, ld_out, cd.data_ptr(), fd.data_ptr(), p, None), [a], [o])
        assert_bits(o.data(), np.array([oracle.ar_remove(x[s], c[s], coef[s]) for s in range(REC_S)]), what)


@LAYOUT
def test_ewma_add_and_ar_add(torch, lay):
    # recur_kernel's 16-B | 8-B chunk forms and recur_row_kernel (EWMA add, 16-B aligned rows)
    for T, poison in cases(REC_T):
        x, sm, c, coefs = rec_case(T)
        ld_in, ld_out, b_in, b_out = la.layout(lay, T)
        what = "T=%d %s %s" % (T, lay, poison)
        a, o, smd = arena_in(x, ld_in, b_in, poison), arena_out(REC_S, T, ld_out, b_out), dvec(torch, sm)
        run(torch, "ewma_add " + what, lib().sts_ewma_add, (a.ptr, o.ptr, REC_S, T, ld_in, ld_out, smd.data_ptr(), None),
            [a], [o])
        assert_bits(o.data(), np.array([oracle.ewma_add(r, v) for r, v in zip(x, sm)]), "ewma_add " + what)
        for p in (1, 8):
            o, cd, fd = arena_out(REC_S, T, ld_out, b_out), dvec(torch, c), dvec(torch, coefs[p])
            run(torch, "ar_add p=%d %s" % (p, what), lib().sts_ar_add,
                (a.ptr, o.ptr, REC_S, T, ld_in, ld_out, cd.data_ptr(), fd.data_ptr(), p, None), [a], [o])
            assert_bits(o.data(), np.array([oracle.ar_add(x[s], c[s], coefs[p][s]) for s in range(REC_S)]),
                        "ar_add p=%d %s" % (p, what))


@cache
def c2_case(method, T, lag):
    rng = np.random.default_rng(7 + 3 * T + lag)              # test_recur_fill_diff_ewma's panels
    x = 100 + rng.standard_normal((REC_S, T)).cumsum(axis=1)
    x[rng.random((REC_S, T)) < 0.2] = NaN
    x[0, : min(T, 5)] = NaN                                   # leading NaN run
    x[2, :] = NaN                                             # all-NaN series
    sm = rng.uniform(0.05, 0.95, REC_S)
    fill = {"previous": oracle.fill_previous, "linear": oracle.fill_linear}[method]
    ref = np.array([oracle.ewma_add(oracle.differences_at_lag(fill(r), lag), v) for r, v in zip(x, sm)])
    return x, sm, ref


@LAYOUT
@pytest.mark.parametrize("method", ["previous", "linear"])
def test_fill_diff_ewma(torch, method, lay):
    # C2.  previous, lag <= 32: the fused recurrence kernels; linear: the composition fill (tile /
    # segment kernel into a packed scratch panel) -> diff_kernel -> EWMA add in place on `out`
    for T, lag, poison in cases(REC_T, (1, 3)):
        x, sm, ref = c2_case(method, T, lag)
        ld_in, ld_out, b_in, b_out = la.layout(lay, T)
        what = "fill_diff_ewma %s T=%d lag=%d %s %s" % (method, T, lag, lay, poison)
        a, o = arena_in(x, ld_in, b_in, poison), arena_out(REC_S, T, ld_out, b_out)
        smd, e = dvec(torch, sm), err_dev(torch, REC_S)
        run(torch, what, lib().sts_fill_diff_ewma,
            (a.ptr, o.ptr, REC_S, T, ld_in, ld_out, oracle.FILL_METHODS[method], lag, smd.data_ptr(), e.data_ptr(), None),
            [a], [o])
        assert (e.cpu().numpy() == 0).all(), what
        assert_bits(o.data(), ref, what)


# ---------------- EWMA fit / sse / gradient, seriesStats: bit-exact ----------------
# ewma_fit_kernel and stats_fast_kernel read whole 128-B lines of a row's own addresses (up to 15
# doubles before the first and after the last element: inside the red zones); results swept by
# test_stats_and_ewma_row_alignments, here the red zones and the untouched input.
EW_S = 7


@cache
def ewma_case(T):
    rng = np.random.default_rng(1000 + T)
    x = np.cumsum(rng.standard_normal((EW_S, T)), axis=1) + 50 + rng.uniform(-5, 5, (EW_S, 1))
    sm = rng.uniform(0.05, 1.5, EW_S)
    fit, err = oracle.panel_ewma_fit(x)
    sse = np.array([oracle.ewma_sse(r, q) for r, q in zip(x, sm)])
    grad = np.array([oracle.ewma_gradient(r, q) for r, q in zip(x, sm)])
    stats = np.array([oracle.stat_counter(r)[1:] for r in x])
    return x, sm, fit, err, sse, grad, stats


@LAYOUT
def test_ewma_fit_and_series_stats(torch, lay):
    for T, poison in cases((64, 65)):
        x, sm, rfit, rerr, rsse, rgrad, rstats = ewma_case(T)
        ld, _, base, _ = la.layout(lay, T)
        what = "T=%d %s %s" % (T, lay, poison)
        a = arena_in(x, ld, base, poison)
        fit, e = vec_out(EW_S), err_dev(torch, EW_S)
        run(torch, "ewma_fit " + what, lib().sts_ewma_fit, (a.ptr, EW_S, T, ld, fit.ptr, e.data_ptr(), None), [a], [fit])
        assert np.array_equal(e.cpu().numpy(), rerr), what
        assert_bits(fit.data().ravel(), rfit, "ewma_fit " + what)
        sse, grad, smd = vec_out(EW_S), vec_out(EW_S), dvec(torch, sm)
        run(torch, "ewma_sse_gradient " + what, lib().sts_ewma_sse_gradient,
            (a.ptr, EW_S, T, ld, smd.data_ptr(), sse.ptr, grad.ptr, None), [a], [sse, grad])
        assert_bits(sse.data().ravel(), rsse, "sse " + what)
        assert_bits(grad.data().ravel(), rgrad, "gradient " + what)
        stats = vec_out(EW_S * 4)
        run(torch, "series_stats " + what, lib().sts_series_stats, (a.ptr, EW_S, T, ld, stats.ptr, None), [a], [stats])
        assert_bits(stats.data().reshape(EW_S, 4), rstats, "series_stats " + what)


# ---------------- GARCH / ARGARCH: bit-exact against the restatement ----------------
GARCH_T = [63, 64, 101]


def _garch_rows(S, T, seed):
    from test_garch import garch_panel
    return garch_panel(S, T, seed)


@cache
def garch_effects_case(T):
    S = 5
    x = _garch_rows(S, T, 21 + T)
    rng = np.random.default_rng(9 + T)
    c, phi = rng.uniform(-1, 1, S), rng.uniform(-0.5, 0.5, S)
    om, al, be = rng.uniform(0.05, 0.4, S), rng.uniform(0.05, 0.3, S), rng.uniform(0.1, 0.5, S)
    R = range(S)
    ref = {
        "loglik": np.array([oracle.garch_loglik(x[s], om[s], al[s], be[s]) for s in R]),
        "grad": np.array([oracle.garch_gradient(x[s], om[s], al[s], be[s]) for s in R]),
        "garch_remove": np.array([oracle.garch_remove(x[s], om[s], al[s], be[s]) for s in R]),
        "garch_add": np.array([oracle.garch_add(x[s], om[s], al[s], be[s]) for s in R]),
        "argarch_remove": np.array([oracle.argarch_remove(x[s], c[s], phi[s], om[s], al[s], be[s]) for s in R]),
        "argarch_add": np.array([oracle.argarch_add(x[s], c[s], phi[s], om[s], al[s], be[s]) for s in R]),
        "argarch_remove_inplace": np.array([oracle.argarch_remove(x[s].copy(), c[s], phi[s], om[s], al[s], be[s],
                                                                  inplace=True) for s in R]),
    }
    return x, (c, phi, om, al, be), ref


@LAYOUT
def test_garch_effects(torch, lay):
    S = 5
    for T, poison in cases(GARCH_T):
        x, (c, phi, om, al, be), ref = garch_effects_case(T)
        ld_in, ld_out, b_in, b_out = la.layout(lay, T)
        what = "T=%d %s %s" % (T, lay, poison)
        keep = [dvec(torch, v) for v in (c, phi, om, al, be)]
        pc, pphi, pom, pal, pbe = [t.data_ptr() for t in keep]
        a = arena_in(x, ld_in, b_in, poison)
        ll, g = vec_out(S), vec_out(3 * S)
        par = dvec(torch, np.stack([om, al, be], axis=1))
        run(torch, "garch_loglik_gradient " + what, lib().sts_garch_loglik_gradient,
            (a.ptr, S, T, ld_in, par.data_ptr(), ll.ptr, g.ptr, None), [a], [ll, g])
        assert_bits(ll.data().ravel(), ref["loglik"], "loglik " + what)
        assert_bits(g.data().reshape(S, 3), ref["grad"], "gradient " + what)
        L = lib()
        for name, fn, extra in (("garch_remove", L.sts_garch_remove, (pom, pal, pbe)),
                                ("garch_add", L.sts_garch_add, (pom, pal, pbe)),
                                ("argarch_remove", L.sts_argarch_remove, (pc, pphi, pom, pal, pbe)),
                                ("argarch_add", L.sts_argarch_add, (pc, pphi, pom, pal, pbe))):
            o = arena_out(S, T, ld_out, b_out)
            run(torch, name + " " + what, fn, (a.ptr, o.ptr, S, T, ld_in, ld_out) + extra + (None,), [a], [o])
            assert_bits(o.data(), ref[name], name + " " + what)
            if name.endswith("remove"):          # dest eq ts
                ip = arena_in(x, ld_in, b_in, poison)
                run(torch, name + " in place " + what, fn, (ip.ptr, ip.ptr, S, T, ld_in, ld_in) + extra + (None,), [], [ip])
                assert_bits(ip.data(), ref["argarch_remove_inplace" if name == "argarch_remove" else name],
                            name + " in place " + what)


@cache
def garch_fit_case(T):
    S = 3
    x = _garch_rows(S, T, 21 + S)
    par, err = oracle.panel_garch_fit(x)
    from mt19937 import MersenneTwister
    from test_garch import argarch_sample
    y = np.vstack([argarch_sample(1.0 + 0.1 * s, 0.3 - 0.05 * (s % 5), 0.2, 0.3, 0.4, T, MersenneTwister(40 + s))
                   for s in range(S)])
    rc = np.empty(S)
    rphi = np.empty(S)
    for s in range(S):
        rc[s], co = oracle.ar_fit(y[s], 1, False)
        rphi[s] = co[0]
    return x, par, err, y, rc, rphi


@LAYOUT
def test_garch_fits(torch, lay):
    S = 3
    for T, poison in cases(GARCH_T):
        x, rpar, rerr, y, rc, rphi = garch_fit_case(T)
        ld, _, base, _ = la.layout(lay, T)
        what = "T=%d %s %s" % (T, lay, poison)
        a, par, e = arena_in(x, ld, base, poison), vec_out(3 * S), err_dev(torch, S)
        run(torch, "garch_fit " + what, lib().sts_garch_fit, (a.ptr, S, T, ld, par.ptr, e.data_ptr(), None), [a], [par])
        assert np.array_equal(e.cpu().numpy(), rerr), ("garch_fit " + what, e.cpu().numpy(), rerr)
        assert_bits(par.data().reshape(S, 3), rpar, "garch_fit " + what)
        a, par, e = arena_in(y, ld, base, poison), vec_out(3 * S), err_dev(torch, S)
        c, phi = vec_out(S), vec_out(S)
        run(torch, "argarch_fit " + what, lib().sts_argarch_fit,
            (a.ptr, S, T, ld, c.ptr, phi.ptr, par.ptr, e.data_ptr(), None), [a], [c, phi, par])
        gc, gphi = c.data().ravel(), phi.data().ravel()
        assert np.allclose(gc, rc, rtol=RTOL, atol=0) and np.allclose(gphi, rphi, rtol=RTOL, atol=0), "argarch AR stage " + what
        # GARCH stage: bit-exact given the device's own (c, phi) residuals
        resid = np.array([oracle.ar_remove(y[s], gc[s], [gphi[s]]) for s in range(S)])
        rpar2, rerr2 = oracle.panel_garch_fit(resid)
        assert np.array_equal(e.cpu().numpy(), rerr2), ("argarch_fit " + what, e.cpu().numpy(), rerr2)
        assert_bits(par.data().reshape(S, 3), rpar2, "argarch_fit " + what)


# ---------------- instants (f3, f4): bit-exact copies ----------------
# S, T, both ld even and 16-B aligned panels: the 16-B forms (sts_instants.hip); S = 5, odd T, odd
# ld or a skewed base: their 8-B fallbacks.  The transposed output is T x ld_out with padding and
# red zones of its own.
@cache
def instants_case(S, T):
    rng = np.random.default_rng(S * 7 + T)
    x = rng.standard_normal((S, T))
    x[rng.random((S, T)) < 0.03] = NaN
    x[S - 1, T - 1] = NaN                       # the last element before the back red zone
    x[:, 0] = 1.0
    gathered, active = oracle.remove_instants_with_nans(x)
    return x, np.isnan(x).any(axis=0).astype(np.uint8), gathered, active, oracle.to_instants(x)


@LAYOUT
def test_instants(torch, lay):
    for S, T, poison in cases((5, 6), (15, 16, 17, 129, 130)):
        x, rflags, rgather, active, rinst = instants_case(S, T)
        n = active.size
        ld_in, ld_gather, b_in, b_out = la.layout(lay, T, T_out=n)
        what = "S=%d T=%d %s %s" % (S, T, lay, poison)
        a = arena_in(x, ld_in, b_in, poison)
        # flags: T bytes between two guards; NaN poison in the padding must not set a flag
        fl = torch.zeros(T + 128, dtype=torch.uint8, device="cuda:0")
        fl[:64] = 7
        fl[64 + T:] = 7
        run(torch, "nan_instants " + what, lib().sts_nan_instants, (a.ptr, S, T, ld_in, fl.data_ptr() + 64, None), [a])
        h = fl.cpu().numpy()
        assert (h[:64] == 7).all() and (h[64 + T:] == 7).all(), "nan_instants wrote outside flags[0, T) " + what
        assert np.array_equal(h[64:64 + T], rflags), "nan_instants " + what
        o, act = arena_out(S, n, ld_gather, b_out), dvec(torch, active, np.int64)
        run(torch, "gather_instants " + what, lib().sts_gather_instants,
            (a.ptr, o.ptr, S, ld_in, ld_gather, act.data_ptr(), n, None), [a], [o])
        assert_bits(o.data(), rgather, "gather_instants " + what)
        ld_t = la.layout(lay, T, T_out=S)[1]
        tr = arena_out(T, S, ld_t, b_out)
        run(torch, "to_instants " + what, lib().sts_to_instants, (a.ptr, tr.ptr, S, T, ld_in, ld_t, None), [a], [tr])
        assert_bits(tr.data(), rinst, "to_instants " + what)


# ---------------- ingest / egress and the generators ----------------
# wire: 8-B loads / stores when bytes + val_off[s] is 8-aligned (8-byte keys), byte-wise otherwise
# (3..5-byte keys); T <= 4096: the one-wave-per-record kernels, 4097: the grid kernels
@cache
def wire_case(T, aligned):
    from sparkts import io as sio
    S = 5
    rng = np.random.default_rng(31 + T)
    keys = ["k%07d" % i for i in range(S)] if aligned else ["k%d" % i + "x" * (i % 3 + 1) for i in range(S)]
    x = rng.standard_normal((S, T)) * 1e3
    x.ravel()[rng.random(S * T) < 0.05] = NaN
    x[0, 0] = -0.0
    data = oracle.wire_records(keys, x)
    _, T2, val_off = sio.wire_scan(data)
    assert T2 == T and np.all((val_off % 8 == 0) == aligned)
    return x, np.frombuffer(data, dtype=np.uint8), np.asarray(val_off, dtype=np.int64)


@LAYOUT
def test_wire_decode_encode(torch, lay):
    S, G = 5, 64
    for T, aligned, poison in cases((7, 390, 4097), (True, False)):
        x, data, val_off = wire_case(T, aligned)
        ld, _, base, _ = la.layout(lay, T)
        what = "T=%d aligned=%s %s %s" % (T, aligned, lay, poison)
        raw = torch.full((data.size + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda:0")
        raw[G:G + data.size] = torch.as_tensor(data.copy(), device="cuda:0")
        off = dvec(torch, val_off, np.int64)
        o = arena_out(S, T, ld, base)
        before = raw.cpu().numpy()
        run(torch, "wire_decode " + what, lib().sts_wire_decode,
            (raw.data_ptr() + G, off.data_ptr(), S, T, o.ptr, ld, None), [], [o])
        assert np.array_equal(raw.cpu().numpy(), before), "wire_decode wrote to its input " + what
        assert_bits(o.data(), x, "wire_decode " + what)
        # encode: the value blocks scrambled, headers and guards as they are
        a = arena_in(x, ld, base, poison)
        scr = data.copy()
        for v in val_off:
            scr[v:v + 8 * T] = 0xA5
        raw[G:G + data.size] = torch.as_tensor(scr, device="cuda:0")
        run(torch, "wire_encode " + what, lib().sts_wire_encode,
            (a.ptr, S, T, ld, off.data_ptr(), raw.data_ptr() + G, None), [a])
        assert np.array_equal(raw.cpu().numpy(), before), "wire_encode " + what


@LAYOUT
def test_observations_to_panel(torch, lay):
    S, T, n = 5, 37, 600
    rng = np.random.default_rng(8)
    sid = rng.integers(0, S, n).astype(np.int32)
    loc = rng.integers(-3, T, n).astype(np.int64)           # negative: not in the index, dropped
    loc[loc < 0] = -1
    val = rng.standard_normal(n)
    ref = np.full((S, T), NaN)
    for i in range(n):                                      # the last observation of a cell wins
        if loc[i] >= 0:
            ref[sid[i], loc[i]] = val[i]
    assert np.isnan(ref).any() and (~np.isnan(ref)).any()
    ld, _, base, _ = la.layout(lay, T)
    sd, ldv, vd = dvec(torch, sid, np.int32), dvec(torch, loc, np.int64), dvec(torch, val)
    for (poison,) in cases():
        o = la.carve(S, T, ld, base, la.POISONS[poison])    # the padding is the caller's
        run(torch, "observations " + lay, lib().sts_observations_to_panel,
            (sd.data_ptr(), ldv.data_ptr(), vd.data_ptr(), n, o.ptr, S, T, ld, None), [], [o])
        assert_bits(o.data(), ref, "observations %s %s" % (lay, poison))
        assert np.array_equal(np.isnan(o.data()), np.isnan(ref))


@LAYOUT
def test_generators(torch, lay):
    S, s0 = 5, 3
    for T in (37, 1001):
        ld, _, base, _ = la.layout(lay, T)
        o = arena_out(S, T, ld, base)
        run(torch, "gen_panel T=%d %s" % (T, lay), lib().sts_gen_panel, (o.ptr, s0, S, T, ld, 123, 0.3, None), [], [o])
        assert_bits(o.data(), oracle.gen_panel(123, S, T, 0.3, s0=s0), "gen_panel T=%d %s" % (T, lay))
        o, c, phi = arena_out(S, T, ld, base), vec_out(S), vec_out(S * 5)
        run(torch, "gen_ar_panel T=%d %s" % (T, lay), lib().sts_gen_ar_panel,
            (o.ptr, c.ptr, phi.ptr, s0, S, T, ld, 77, 5, None), [], [o, c, phi])
        assert_bits(o.data(), oracle.gen_ar_panel(77, S, T, 5, s0=s0), "gen_ar_panel T=%d %s" % (T, lay))


# ---------------- _host variants: one ld, numpy arenas, pageable and pinned ----------------

class Pinned:
    """float64 numpy view of pinned host memory from sts_host_alloc."""

    def __init__(self, n):
        self.p = ctypes.c_void_p()
        assert lib().sts_host_alloc(8 * n, ctypes.byref(self.p)) == 0
        self.a = np.frombuffer((ctypes.c_char * (8 * n)).from_address(self.p.value), dtype=np.float64)

    def free(self):
        if self.p.value:
            lib().sts_host_free(self.p)
            self.p = ctypes.c_void_p()


class HostArenas:
    """numpy arenas in pageable or pinned memory; frees the pinned blocks at exit."""

    def __init__(self, pinned):
        self.pinned, self.blocks = pinned, []

    def carve(self, S, T, ld, poison, data=None, red=la.RED):
        raw = None
        if self.pinned:
            b = Pinned(2 * red + 3 + S * ld + la.LINE)
            self.blocks.append(b)
            raw = b.a
        return la.carve_np(S, T, ld, 3, poison, red=red, data=data, raw=raw)

    def vec(self, n):
        return self.carve(1, n, n, la.OUT_FILL, red=64)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.blocks:
            b.free()


def run_host(what, fn, args, ins=(), outs=()):
    before_in = [a.snapshot() for a in ins]
    before_out = [a.snapshot() for a in outs]
    st = fn(*args)
    assert st == 0, (what, st, lib().sts_last_error())
    for a, snap in zip(ins, before_in):
        a.verify_all(snap, what + ": host input")
    for a, snap in zip(outs, before_out):
        a.verify_outside(snap, what + ": host output")


def P(a):
    return a.ctypes.data


HOST_S, HOST_T = 5, 65


def _host_autocorr(H, x, a, ld):
    K = 20
    acf = H.vec(HOST_S * K)
    run_host("autocorr_host", lib().sts_autocorr_host, (a.ptr, HOST_S, HOST_T, ld, K, acf.ptr), [a], [acf])
    assert_rel(acf.data().reshape(HOST_S, K), np.array([oracle.autocorr(r, K) for r in x]), what="autocorr_host")


def _host_diff(H, x, a, ld):
    o = H.carve(HOST_S, HOST_T, ld, la.OUT_FILL)
    run_host("diff_at_lag_host", lib().sts_diff_at_lag_host, (a.ptr, o.ptr, HOST_S, HOST_T, ld, 3, 7), [a], [o])
    assert_bits(o.data(), np.array([oracle.differences_at_lag(r, 3, start=7) for r in x]), "diff_at_lag_host")


def _host_lag(H, x, a, ld):
    ref = np.concatenate([oracle.lag(r, 2, True).T.ravel() for r in x])
    o = H.vec(ref.size)
    run_host("lag_matrix_host", lib().sts_lag_matrix_host, (a.ptr, o.ptr, HOST_S, HOST_T, ld, 2, 1), [a], [o])
    assert_bits(o.data().ravel(), ref, "lag_matrix_host")


def _host_ewma(H, x, a, ld):
    sm = np.linspace(0.1, 0.9, HOST_S)
    for name, fn, orc in (("ewma_add_host", lib().sts_ewma_add_host, oracle.ewma_add),
                          ("ewma_remove_host", lib().sts_ewma_remove_host, oracle.ewma_remove)):
        o = H.carve(HOST_S, HOST_T, ld, la.OUT_FILL)
        run_host(name, fn, (a.ptr, o.ptr, HOST_S, HOST_T, ld, P(sm)), [a], [o])
        assert_bits(o.data(), np.array([orc(r, v) for r, v in zip(x, sm)]), name)
    fit, err = H.vec(HOST_S), np.full(HOST_S, -1, np.int32)
    run_host("ewma_fit_host", lib().sts_ewma_fit_host, (a.ptr, HOST_S, HOST_T, ld, fit.ptr, P(err)), [a], [fit])
    rfit, rerr = oracle.panel_ewma_fit(x)
    assert np.array_equal(err, rerr)
    assert_bits(fit.data().ravel(), rfit, "ewma_fit_host")


def _host_ar(H, x, a, ld):
    p = 3
    rc = np.empty(HOST_S)
    rcoef = np.empty((HOST_S, p))
    for s in range(HOST_S):
        rc[s], rcoef[s] = oracle.ar_fit(x[s], p, False)
    for fused in (False, True):
        c, coef, err = H.vec(HOST_S), H.vec(HOST_S * p), np.full(HOST_S, -1, np.int32)
        if fused:
            o = H.carve(HOST_S, HOST_T, ld, la.OUT_FILL)
            run_host("ar_fit_remove_host", lib().sts_ar_fit_remove_host,
                     (a.ptr, o.ptr, HOST_S, HOST_T, ld, p, 0, c.ptr, coef.ptr, P(err)), [a], [o, c, coef])
        else:
            run_host("ar_fit_host", lib().sts_ar_fit_host, (a.ptr, HOST_S, HOST_T, ld, p, 0, c.ptr, coef.ptr, P(err)),
                     [a], [c, coef])
        assert (err == 0).all()
        gc, gcoef = c.data().ravel(), coef.data().reshape(HOST_S, p)
        assert_rel(gcoef, rcoef, what="ar_fit_host coef")
        assert_rel(gc, rc, what="ar_fit_host c")
        if fused:
            assert_bits(o.data(), np.array([oracle.ar_remove(x[s], gc[s], gcoef[s]) for s in range(HOST_S)]),
                        "ar_fit_remove_host residuals")
    cm, cf = np.linspace(-1, 1, HOST_S), np.linspace(-0.3, 0.3, HOST_S * p).reshape(HOST_S, p)
    for name, fn, orc in (("ar_remove_host", lib().sts_ar_remove_host, oracle.ar_remove),
                          ("ar_add_host", lib().sts_ar_add_host, oracle.ar_add)):
        o = H.carve(HOST_S, HOST_T, ld, la.OUT_FILL)
        run_host(name, fn, (a.ptr, o.ptr, HOST_S, HOST_T, ld, P(cm), P(cf), p), [a], [o])
        assert_bits(o.data(), np.array([orc(x[s], cm[s], cf[s]) for s in range(HOST_S)]), name)


def _host_garch(H, x, a, ld):
    par, err = H.vec(3 * HOST_S), np.full(HOST_S, -1, np.int32)
    run_host("garch_fit_host", lib().sts_garch_fit_host, (a.ptr, HOST_S, HOST_T, ld, par.ptr, P(err)), [a], [par])
    rpar, rerr = oracle.panel_garch_fit(x)
    assert np.array_equal(err, rerr)
    assert_bits(par.data().reshape(HOST_S, 3), rpar, "garch_fit_host")
    c, phi, par, err = H.vec(HOST_S), H.vec(HOST_S), H.vec(3 * HOST_S), np.full(HOST_S, -1, np.int32)
    run_host("argarch_fit_host", lib().sts_argarch_fit_host, (a.ptr, HOST_S, HOST_T, ld, c.ptr, phi.ptr, par.ptr, P(err)),
             [a], [c, phi, par])
    gc, gphi = c.data().ravel(), phi.data().ravel()
    fits = [oracle.ar_fit(r, 1, False) for r in x]
    assert np.allclose(gc, [f[0] for f in fits], rtol=RTOL, atol=0)
    assert np.allclose(gphi, [f[1][0] for f in fits], rtol=RTOL, atol=0)
    rpar, rerr = oracle.panel_garch_fit(np.array([oracle.ar_remove(x[s], gc[s], [gphi[s]]) for s in range(HOST_S)]))
    assert np.array_equal(err, rerr)
    assert_bits(par.data().reshape(HOST_S, 3), rpar, "argarch_fit_host")


def _ar_remove_in_place(r, c, coef):
    """dest eq ts: ts(i - j - 1) is already dest(i - j - 1) (the recurrence test_recur_shapes.py builds)"""
    r = r.copy()
    for i in range(r.size):
        v = r[i] - c
        for j in range(min(len(coef), i)):
            v -= r[i - j - 1] * coef[j]
        r[i] = v
    return r


def _dest_is_ts(fn, r, *model):
    """an oracle recurrence with dest = ts, on a copy of the row"""
    r = r.copy()
    fn(r, *model, dest=r)
    return r


def _host_in_place(H, x, a, ld):
    # in == out: one device region per chunk for both, copied in and copied out from there
    p = 3
    sm = np.linspace(0.1, 0.9, HOST_S)
    cm, cf = np.linspace(-1, 1, HOST_S), np.linspace(-0.3, 0.3, HOST_S * p).reshape(HOST_S, p)
    rows = range(HOST_S)
    for name, fn, tail, ref in (
            ("diff_at_lag_host", lib().sts_diff_at_lag_host, (3, 7),
             [oracle.differences_at_lag(r.copy(), 3, start=7, inplace=True) for r in x]),
            ("ewma_add_host", lib().sts_ewma_add_host, (P(sm),), [_dest_is_ts(oracle.ewma_add, x[s], sm[s]) for s in rows]),
            ("ewma_remove_host", lib().sts_ewma_remove_host, (P(sm),),
             [_dest_is_ts(oracle.ewma_remove, x[s], sm[s]) for s in rows]),
            ("ar_add_host", lib().sts_ar_add_host, (P(cm), P(cf), p),
             [oracle.ar_add(x[s].copy(), cm[s], cf[s], inplace=True) for s in rows]),
            ("ar_remove_host", lib().sts_ar_remove_host, (P(cm), P(cf), p),
             [_ar_remove_in_place(x[s], cm[s], cf[s]) for s in rows])):
        io = H.carve(HOST_S, HOST_T, ld, la.OUT_FILL, data=x)
        run_host(name + " in place", fn, (io.ptr, io.ptr, HOST_S, HOST_T, ld) + tail, [], [io])
        assert_bits(io.data(), np.array(ref), name + " in place")


def _host_optional(H, x, a, ld):
    # pvalue == NULL stays NULL on the device: the statistic is the one of the call with a p-value array
    for name, fn, head, tail in (("adf_test_host", lib().sts_adf_test_host, (2, 1), (None,)),
                                 ("lb_test_host", lib().sts_lb_test_host, (5,), ())):
        got = []
        for with_p in (True, False):
            stat, pv = H.vec(HOST_S), H.vec(HOST_S)
            outs = [stat, pv] if with_p else [stat]
            run_host(name, fn, (a.ptr, HOST_S, HOST_T, ld) + head + (stat.ptr, pv.ptr if with_p else None) + tail,
                     [a], outs)
            got.append(stat.data().copy())
            assert np.isfinite(got[-1]).all(), name
            if with_p:
                p = pv.data().ravel()
                assert ((p >= 0) & (p <= 1)).all(), (name, p)
        assert_bits(got[1], got[0], name + " without pvalue")


def _host_ar_p0(H, x, a, ld):
    # p = 0: no coefficients, coef == NULL (the wrapper's dummy coefficient row)
    cm = np.linspace(-1, 1, HOST_S)
    for name, fn, orc in (("ar_remove_host", lib().sts_ar_remove_host, oracle.ar_remove),
                          ("ar_add_host", lib().sts_ar_add_host, oracle.ar_add)):
        o = H.carve(HOST_S, HOST_T, ld, la.OUT_FILL)
        run_host(name + " p = 0", fn, (a.ptr, o.ptr, HOST_S, HOST_T, ld, P(cm), None, 0), [a], [o])
        assert_bits(o.data(), np.array([orc(x[s], cm[s], []) for s in range(HOST_S)]), name + " p = 0")


HOST_OPS = {"autocorr": _host_autocorr, "diff_at_lag": _host_diff, "lag_matrix": _host_lag, "ewma": _host_ewma,
            "ar": _host_ar, "garch": _host_garch, "in_place": _host_in_place, "optional_outputs": _host_optional,
            "ar_p0": _host_ar_p0}


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("op", sorted(HOST_OPS))
def test_host_variants(torch, op, pinned):
    # one ld = T + 3 for every panel of the call, the base 3 doubles into a 128-B line
    ld = HOST_T + 3
    if op == "garch":
        x = _garch_rows(HOST_S, HOST_T, 33)
    else:
        x = oracle.gen_ar_panel(7, HOST_S, HOST_T, 3) + 0.01 * np.sin(np.arange(HOST_T))[None, :]
    for (poison,) in cases():
        with HostArenas(pinned) as H:
            a = H.carve(HOST_S, HOST_T, ld, la.POISONS[poison], data=x)
            HOST_OPS[op](H, x, a, ld)
