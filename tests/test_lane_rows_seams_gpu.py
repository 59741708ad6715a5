"""The seams of the lane-per-series loop (csrc/sts_lane_rows.hpp: stream_rows, map_rows) on every
entry point whose kernel runs it -- or, for the GARCH fit, the ARIMA forecast and the GARCH
samplers, keeps the same loop written out.  Needs an MI355X.

A 64-lane workgroup of that loop owns SPW series (16, 32 or 64) and moves their SPW x CH block (CH
32, 64 or 128 steps) through LDS; the row and the column of an element are computed independently,
so each seam appears once in the shapes (S, T) and not in every combination:

  S  15 16 17   31 32 33   63 64 65      SPW - 1, SPW, SPW + 1
  T  31 32 33   63 64 65   127 128 129   CH - 1, CH, CH + 1;   257: a third chunk with one step in it

together with (1, 1).  An operator with a minimum length leaves out the shapes below it: the ARGARCH
effects and every ARIMA operator leave out (1, 1) (ARIMA needs d + max(p, q) + 1 steps), and the
fits run the two shapes the issue names, (33, 65) and (65, 129).  sts_ewma_add and the fused
fill-diff-EWMA run (3, 1025) too: up to 1024 steps their 16-byte-aligned rows go to the whole-row
kernel, so only there does the even pitch reach the 16-byte chunk kernel.

Every case runs at three pitches: packed (ld = T), "even" (even ld_in and ld_out: on the 16-byte
aligned bases torch allocates, the sts_recur.hip operators take the 16-byte kernel) and "odd" (odd
ld_in and ld_out: the 8-byte kernel).  Out of place ld_in = ld_out + 2.  The input's pad columns hold
NaN; every output is pre-filled with a sentinel, pad columns and a tail past the last row included,
and every pad and tail element must still hold it afterwards (an in-place panel's pads hold the
sentinel).  The elements have the bits of the references the operators' own tests use (oracle.*,
tests/arima_ref.py, tests/sample_ref.py).  One test id is one operator x one pitch; references are
computed once per shape and shared.

The fits put the ballot's `want` mask to work: each panel holds one series with a NaN, which leaves
after the first round with TooManyEvaluations and makes a hole in the mask, and series that converge
after different numbers of evaluations (asserted on the references' counts).  Parameters are
compared bit for bit, the per-series status, and the evaluation counts where the entry point returns
them (ARIMA).
"""
import ctypes
import functools

import numpy as np
import pytest

import arima_ref as ar
import oracle
import sample_ref as sr
from stream_gate import dev, vp
from test_arima import arma_panel, random_coef, ref_fit, ref_lib, starts  # noqa: F401
from test_garch import garch_panel
from test_recur_shapes import assert_bits

pytestmark = pytest.mark.gpu

SENT = -3.0e55
TAIL = 8                    # sentinel elements past the last output row
SHAPES = [(1, 1), (15, 31), (16, 32), (17, 33), (31, 63), (32, 64), (33, 65), (63, 127), (64, 128), (65, 129), (2, 257)]
LONG = SHAPES[1:]
ROWS = SHAPES + [(3, 1025)]
FIT_SHAPES = [(33, 65), (65, 129)]
PITCHES = ["packed", "even", "odd"]
SEED = 0x9E3779B97F4A7C15
TOO_MANY_EVALUATIONS = ar.TOO_MANY_EVALUATIONS
cache = functools.lru_cache(maxsize=None)


def ld_of(T, pitch):
    return {"packed": T, "even": T + 2 + (T & 1), "odd": T + 1 + (T & 1)}[pitch]


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


def L():
    from sparkts import _native
    return _native.lib()


def gauss(S, T, seed):
    return np.random.default_rng(seed).standard_normal((S, T))


def in_panel(torch, x, ld):
    a = torch.full((x.shape[0], ld), float("nan"), dtype=torch.float64, device="cuda:0")
    a[:, :x.shape[1]] = dev(torch, x)
    return a


def sentinels(torch, n, dtype=None):
    return torch.full((n + TAIL,), SENT if dtype is None else -77, dtype=dtype or torch.float64, device="cuda:0")


def check_panel(o, rows, T_out, ld_out, ref, what):
    got = o.cpu().numpy()
    panel = got[:rows * ld_out].reshape(rows, ld_out)
    assert_bits(panel[:, :T_out], ref, what)
    assert (panel[:, T_out:] == SENT).all(), what + ": a pad column was written"
    assert (got[rows * ld_out:] == SENT).all(), what + ": written past the last row"


# ---------------- map form ----------------
# A case is (x, ref, aux, call, in_place): the host input panel, the expected output panel, host
# arrays the call takes besides, call(lib, in, ld_in, out, ld_out, *aux) -> status.

def garch_par(S, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, S), rng.uniform(-0.5, 0.5, S), rng.uniform(0.05, 0.4, S), rng.uniform(0.05, 0.3, S),
            rng.uniform(0.1, 0.5, S))


@cache
def ewma_add(S, T):
    x, sm = gauss(S, T, 1) + 10, np.random.default_rng(2).uniform(0.05, 0.95, S)
    ref = np.array([oracle.ewma_add(r, v) for r, v in zip(x, sm)])
    return x, ref, [sm], lambda lib, a, ldi, o, ldo, s: lib.sts_ewma_add(a, o, S, T, ldi, ldo, s, None), False


@cache
def ewma_remove_in_place(S, T):
    x, sm = gauss(S, T, 3) + 10, np.random.default_rng(4).uniform(0.05, 0.95, S)
    ref = x.copy()
    for r, v in zip(ref, sm):
        oracle.ewma_remove(r, v, dest=r)
    return x, ref, [sm], lambda lib, a, ldi, o, ldo, s: lib.sts_ewma_remove(a, o, S, T, ldi, ldo, s, None), True


def ar_case(S, T, p, seed):
    rng = np.random.default_rng(seed)
    return gauss(S, T, seed + 1), rng.standard_normal(S), rng.uniform(-0.3, 0.3, (S, p))


@cache
def ar_add(S, T, p):
    x, c, coef = ar_case(S, T, p, 5)
    ref = np.array([oracle.ar_add(x[s], c[s], coef[s]) for s in range(S)])
    return x, ref, [c, coef], lambda lib, a, ldi, o, ldo, cd, fd: lib.sts_ar_add(a, o, S, T, ldi, ldo, cd, fd, p, None), False


@cache
def ar_remove_in_place(S, T, p):
    x, c, coef = ar_case(S, T, p, 7)
    ref = x.copy()
    for s in range(S):          # dest eq ts: the lags read the values already overwritten
        r = ref[s]
        for i in range(T):
            v = r[i] - c[s]
            for j in range(min(p, i)):
                v -= r[i - j - 1] * coef[s, j]
            r[i] = v
    return x, ref, [c, coef], lambda lib, a, ldi, o, ldo, cd, fd: lib.sts_ar_remove(a, o, S, T, ldi, ldo, cd, fd, p, None), True


@cache
def diff_in_place(S, T, lag):
    x = gauss(S, T, 9)
    ref = np.array([oracle.differences_at_lag(r.copy(), lag, start=lag, inplace=True) for r in x])
    return x, ref, [], lambda lib, a, ldi, o, ldo: lib.sts_diff_at_lag(a, o, S, T, ldi, ldo, lag, lag, None), True


@cache
def inverse_diff(S, T, lag):
    x = gauss(S, T, 10)
    ref = np.array([oracle.inverse_differences_at_lag(r, lag) for r in x])
    return x, ref, [], lambda lib, a, ldi, o, ldo: lib.sts_inverse_diff_at_lag(a, o, S, T, ldi, ldo, lag, lag, None), False


@cache
def diff_order_d(S, T, d):
    x = gauss(S, T, 11).cumsum(axis=1)
    ref = np.array([oracle.differences_of_order_d(r, d) for r in x])
    return x, ref, [], lambda lib, a, ldi, o, ldo: lib.sts_diff_order_d(a, o, S, T, ldi, ldo, d, None), False


@cache
def inverse_diff_order_d(S, T, d):
    x = gauss(S, T, 12)
    ref = np.array([ar.inverse_differences_of_order_d(r, d) for r in x])
    return x, ref, [], lambda lib, a, ldi, o, ldo: lib.sts_inverse_diff_order_d(a, o, S, T, ldi, ldo, d, None), False


@cache
def fill_diff_ewma(S, T, lag):
    rng = np.random.default_rng(13)
    x = 100 + rng.standard_normal((S, T)).cumsum(axis=1)
    x[rng.random((S, T)) < 0.2] = np.nan
    x[0, :min(T, 5)] = np.nan
    sm = rng.uniform(0.05, 0.95, S)
    ref = np.array([oracle.ewma_add(oracle.differences_at_lag(oracle.fill_previous(r), lag), v) for r, v in zip(x, sm)])
    return x, ref, [sm], lambda lib, a, ldi, o, ldo, s: lib.sts_fill_diff_ewma(a, o, S, T, ldi, ldo, 3, lag, s, None,
                                                                               None), False


def garch_effect(name, fn, with_ar, in_place=False):
    @cache
    def case(S, T):
        x = gauss(S, T, 14)
        par = garch_par(S, 15)
        use = par if with_ar else par[2:]
        kw = {"inplace": True} if in_place else {}
        ref = np.array([fn(x[s].copy(), *[float(v[s]) for v in use], **kw) for s in range(S)])
        return x, ref, list(use), lambda lib, a, ldi, o, ldo, *pd: getattr(lib, name)(a, o, S, T, ldi, ldo, *pd, None), in_place
    return case


def arima_effect(name, fn):
    @cache
    def case(S, T, p, d, q, icpt):
        x = arma_panel(16, S, T, min(p, 2), min(q, 2), level=2.0, d=d)
        coef = random_coef(17, S, p, q, icpt) * 0.8
        ref = np.array([fn(p, d, q, coef[s], icpt, x[s]) for s in range(S)])
        return x, ref, [coef], lambda lib, a, ldi, o, ldo, cd: getattr(lib, name)(a, o, S, T, ldi, ldo, p, d, q, icpt, cd,
                                                                                  None), False
    return case


@cache
def arima_forecast(S, T, p, d, q, icpt, nf):
    x = arma_panel(18, S, T, min(p, 2), min(q, 2), level=2.0, d=d)
    coef = random_coef(19, S, p, q, icpt) * 0.8
    ref = np.array([ar.forecast(p, d, q, coef[s], icpt, x[s], nf) for s in range(S)])
    return x, ref, [coef], lambda lib, a, ldi, o, ldo, cd: lib.sts_arima_forecast(a, o, S, T, ldi, ldo, p, d, q, icpt, cd,
                                                                                  nf, None), False


ARMA, ARIMA_ = (1, 0, 1, 1), (2, 1, 2, 0)      # d = 0: the kernels read and write the caller's panels themselves
ARIMA_LONG = [s for s in LONG if s[1] >= 1 + 2 + 1]

# operator -> [(case builder, its arguments after (S, T), the shapes it runs at)]
MAP_OPS = {
    "ewma_add": [(ewma_add, (), ROWS)],
    "ewma_remove_in_place": [(ewma_remove_in_place, (), SHAPES)],
    "ar_add": [(ar_add, (1,), SHAPES), (ar_add, (3,), SHAPES)],
    "ar_remove_in_place": [(ar_remove_in_place, (1,), SHAPES), (ar_remove_in_place, (3,), SHAPES)],
    "diff_in_place": [(diff_in_place, (1,), SHAPES), (diff_in_place, (3,), LONG)],
    "inverse_diff": [(inverse_diff, (1,), SHAPES), (inverse_diff, (3,), LONG)],
    "diff_order_d": [(diff_order_d, (2,), SHAPES)],
    "inverse_diff_order_d": [(inverse_diff_order_d, (2,), SHAPES)],
    "fill_diff_ewma": [(fill_diff_ewma, (1,), ROWS), (fill_diff_ewma, (8,), LONG)],
    "garch_remove": [(garch_effect("sts_garch_remove", oracle.garch_remove, False), (), SHAPES)],
    "garch_add": [(garch_effect("sts_garch_add", oracle.garch_add, False), (), SHAPES)],
    "argarch_remove": [(garch_effect("sts_argarch_remove", oracle.argarch_remove, True), (), LONG)],
    "argarch_remove_in_place": [(garch_effect("sts_argarch_remove", oracle.argarch_remove, True, True), (), LONG)],
    "argarch_add": [(garch_effect("sts_argarch_add", oracle.argarch_add, True), (), LONG)],
    "arima_remove": [(arima_effect("sts_arima_remove", ar.remove_effects), o, ARIMA_LONG) for o in (ARMA, ARIMA_)],
    # add with d = 1 runs the integrate pass in place on the output panel
    "arima_add_integrate": [(arima_effect("sts_arima_add", ar.add_effects), o, ARIMA_LONG) for o in (ARMA, ARIMA_)],
    "arima_forecast": [(arima_forecast, ARMA + (nf,), ARIMA_LONG) for nf in (0, 1, 65)] + [(arima_forecast, ARIMA_ + (65,),
                                                                                           ARIMA_LONG)],
}


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("op", sorted(MAP_OPS))
def test_map_form(torch, op, pitch):
    for build, args, shapes in MAP_OPS[op]:
        for S, T in shapes:
            x, ref, aux, call, in_place = build(S, T, *args)
            what = "%s%s S=%d T=%d %s" % (op, args, S, T, pitch)
            T_out = ref.shape[1]
            assert ref.shape[0] == S and T_out >= T, what
            ld_out = ld_of(T_out, pitch)
            o = sentinels(torch, S * ld_out)
            if in_place:
                ld_in, a = ld_out, o
                o[:S * ld_out].view(S, ld_out)[:, :T] = dev(torch, x)
            else:
                ld_in = ld_of(T, pitch) + (0 if pitch == "packed" else 2)
                a = in_panel(torch, x, ld_in)
            more = [dev(torch, v) for v in aux]
            st = call(L(), vp(a), ld_in, vp(o), ld_out, *[vp(v) for v in more])
            assert st == 0, (what, st, L().sts_last_error())
            torch.cuda.synchronize()
            check_panel(o, S, T_out, ld_out, ref, what)
            if not in_place:
                assert_bits(a.cpu().numpy()[:, :T], x, what + ": the input")


# ---------------- sample form ----------------

@cache
def sample_case(S, n):
    g = sr.normal_panel(SEED, 3, S, 1, n)          # s0 = 3, t0 = 1: the first pair of every row is half outside
    par = garch_par(S, 20)
    garch = np.array([sr.garch_sample(g[s], par[2][s], par[3][s], par[4][s]) for s in range(S)])
    argarch = np.array([sr.garch_sample(g[s], par[2][s], par[3][s], par[4][s], par[0][s], par[1][s]) for s in range(S)])
    return par, garch, argarch


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("kind", ["garch", "argarch"])
def test_sample_form(torch, kind, pitch):
    for S, n in SHAPES:
        par, garch, argarch = sample_case(S, n)
        what = "%s sample S=%d n=%d %s" % (kind, S, n, pitch)
        ld = ld_of(n, pitch)
        o = sentinels(torch, S * ld)
        use = [dev(torch, v) for v in (par if kind == "argarch" else par[2:])]
        fn = L().sts_argarch_sample if kind == "argarch" else L().sts_garch_sample
        st = fn(vp(o), 3, S, n, ld, *[vp(v) for v in use], 1, ctypes.c_uint64(SEED), None)
        assert st == 0, (what, st, L().sts_last_error())
        torch.cuda.synchronize()
        check_panel(o, S, n, ld, argarch if kind == "argarch" else garch, what)


# ---------------- pass form: one evaluation per series ----------------

def check_vector(o, n, ref, what):
    got = o.cpu().numpy()
    assert_bits(got[:n], np.asarray(ref, dtype=np.float64).ravel(), what)
    assert (got[n:] == SENT).all(), what + ": written past the last series"


@cache
def ewma_eval(S, T):
    x, sm = gauss(S, T, 21) + 10, np.random.default_rng(22).uniform(0.05, 0.95, S)
    return x, sm, [oracle.ewma_sse(r, v) for r, v in zip(x, sm)], [oracle.ewma_gradient(r, v) for r, v in zip(x, sm)]


@cache
def garch_eval(S, T):
    x = gauss(S, T, 23)
    par = np.stack(garch_par(S, 24)[2:], axis=1)
    return (x, par, [oracle.garch_loglik(x[s], *par[s]) for s in range(S)],
            np.array([oracle.garch_gradient(x[s], *par[s]) for s in range(S)]))


@cache
def arima_eval(S, T, p, d, q, icpt):
    x = arma_panel(25, S, T, p, q, level=1.0, d=d)
    coef = random_coef(26, S, p, q, icpt)
    return (x, coef, [ar.loglik_css(p, d, q, coef[s], icpt, x[s]) for s in range(S)],
            np.array([ar.gradient_css(p, d, q, coef[s], icpt, x[s]) for s in range(S)]))


def eval_call(op, S, T):
    """-> (x, parameters, value, gradient, call(lib, in, ld, parameters, value, gradient))"""
    if op == "ewma_sse_gradient":
        return ewma_eval(S, T) + (lambda lib, a, ld, p, f, g: lib.sts_ewma_sse_gradient(a, S, T, ld, p, f, g, None),)
    if op == "garch_loglik_gradient":
        return garch_eval(S, T) + (lambda lib, a, ld, p, f, g: lib.sts_garch_loglik_gradient(a, S, T, ld, p, f, g, None),)
    p, d, q, icpt = ARMA if op == "arma_css" else ARIMA_
    return arima_eval(S, T, p, d, q, icpt) + (lambda lib, a, ld, c, f, g: lib.sts_arima_css_loglik_gradient(
        a, S, T, ld, p, d, q, icpt, c, f, g, None),)


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("op", ["ewma_sse_gradient", "garch_loglik_gradient", "arma_css", "arima_css"])
def test_pass_form(torch, op, pitch):
    for S, T in (ARIMA_LONG if op.endswith("css") else SHAPES):
        x, par, f_ref, g_ref, call = eval_call(op, S, T)
        what = "%s S=%d T=%d %s" % (op, S, T, pitch)
        ld = ld_of(T, pitch)
        a, pd = in_panel(torch, x, ld), dev(torch, par)
        ng = np.asarray(g_ref).size
        f, g = sentinels(torch, S), sentinels(torch, ng)
        st = call(L(), vp(a), ld, vp(pd), vp(f), vp(g))
        assert st == 0, (what, st, L().sts_last_error())
        torch.cuda.synchronize()
        check_vector(f, S, f_ref, what + ": the value")
        check_vector(g, ng, g_ref, what + ": the gradient")


# ---------------- pass form with the want mask at work: the fits ----------------

NAN_ROW = 5


def mixed(x):
    """series s scaled by 2^(s % 5 - 2) -- other optimizer paths, other numbers of rounds -- and one NaN"""
    x = x * np.ldexp(1.0, np.arange(len(x)) % 5 - 2)[:, None]
    x[NAN_ROW, x.shape[1] // 2] = np.nan
    return x


@cache
def ewma_fit_case(S, T):
    x = mixed(100 + gauss(S, T, 27).cumsum(axis=1) + 3 * gauss(S, T, 28) * (np.arange(S) % 3)[:, None])
    fits = [oracle.ewma_fit(r) for r in x]
    return x, fits


@cache
def garch_fit_case(S, T):
    x = mixed(garch_panel(S, T, 29))
    return x, oracle.panel_garch_fit(x), [oracle.garch_fit(r) for r in x]


def assert_holes(status, evals, what):
    assert status[NAN_ROW] == TOO_MANY_EVALUATIONS, what
    assert len({e for s, e in zip(status, evals) if s == 0}) >= 3, what + ": the series leave in the same round"


@pytest.mark.parametrize("pitch", PITCHES)
def test_ewma_fit_mask(torch, pitch):
    for S, T in FIT_SHAPES:
        x, fits = ewma_fit_case(S, T)
        what = "ewma fit S=%d T=%d %s" % (S, T, pitch)
        assert_holes([f[0] for f in fits], [f[2] for f in fits], what)
        ld = ld_of(T, pitch)
        a, sm, err = in_panel(torch, x, ld), sentinels(torch, S), sentinels(torch, S, torch.int32)
        assert L().sts_ewma_fit(vp(a), S, T, ld, vp(sm), vp(err), None) == 0, what
        torch.cuda.synchronize()
        check_vector(sm, S, [f[1] if f[0] == 0 else np.nan for f in fits], what)
        e = err.cpu().numpy()
        assert e[:S].tolist() == [f[0] for f in fits] and (e[S:] == -77).all(), what


@pytest.mark.parametrize("pitch", PITCHES)
def test_garch_fit_mask(torch, pitch):
    for S, T in FIT_SHAPES:
        x, (rpar, rerr), fits = garch_fit_case(S, T)
        what = "garch fit S=%d T=%d %s" % (S, T, pitch)
        assert_holes(rerr, [f[2] for f in fits], what)
        ld = ld_of(T, pitch)
        a, par, err = in_panel(torch, x, ld), sentinels(torch, 3 * S), sentinels(torch, S, torch.int32)
        assert L().sts_garch_fit(vp(a), S, T, ld, vp(par), vp(err), None) == 0, what
        torch.cuda.synchronize()
        check_vector(par, 3 * S, np.where((rerr == 0)[:, None], rpar, np.nan), what)
        e = err.cpu().numpy()
        assert np.array_equal(e[:S], rerr) and (e[S:] == -77).all(), what


@cache
def arima_fit_case(S, T):
    p, d, q, icpt = ARMA
    x = arma_panel(30, S, T, p, q, level=5.0, d=d)
    x[NAN_ROW, T // 2] = np.nan
    with np.errstate(all="ignore"):
        return x, starts(p, d, q, x, icpt=bool(icpt))


@pytest.mark.parametrize("pitch", PITCHES)
def test_arima_fit_mask(torch, ref_lib, pitch):
    p, d, q, icpt = ARMA
    n = ar.n_coef(p, q, icpt)
    for S, T in FIT_SHAPES:
        x, init = arima_fit_case(S, T)
        what = "arima fit S=%d T=%d %s" % (S, T, pitch)
        want = arima_fit_reference(ref_lib, S, T)
        assert_holes([w[0] for w in want], [w[2] for w in want], what)
        ld = ld_of(T, pitch)
        a, i0 = in_panel(torch, x, ld), dev(torch, init)
        coef, err, ev = sentinels(torch, S * n), sentinels(torch, S, torch.int32), sentinels(torch, S, torch.int32)
        assert L().sts_arima_fit_css(vp(a), S, T, ld, p, d, q, icpt, vp(i0), vp(coef), vp(err), vp(ev), None) == 0, what
        torch.cuda.synchronize()
        check_vector(coef, S * n, np.array([w[1] if w[0] == 0 else np.full(n, np.nan) for w in want]), what)
        e, v = err.cpu().numpy(), ev.cpu().numpy()
        assert e[:S].tolist() == [w[0] for w in want] and (e[S:] == -77).all(), what
        assert v[:S].tolist() == [w[2] for w in want] and (v[S:] == -77).all(), what


_ARIMA_FITS = {}


def arima_fit_reference(ref_lib, S, T):
    if (S, T) not in _ARIMA_FITS:
        p, d, q, icpt = ARMA
        x, init = arima_fit_case(S, T)
        with np.errstate(all="ignore"):
            _ARIMA_FITS[S, T] = [ref_fit(ref_lib, p, d, q, icpt, x[s], init[s]) for s in range(S)]
    return _ARIMA_FITS[S, T]
