"""ARIMA(p, d, q) with MA terms: the "css-cgd" fit, the CSS likelihood, the Hannan-Rissanen start,
remove / add and forecast (S/models/ARIMA.scala).  The checker is tests/arima_ref.py, a float64
restatement of the reference's loops and of commons-math3's optimizer.

CPU (no GPU):
* restatement anchors: the restated gradient against finite differences of the restated
  likelihood, the bounds of the reference's own ARIMASuite on fits produced by the host build
  of the device state machine, the add / remove round trip, stationarity / invertibility;
* the state machine (csrc/sts_arima_opt.hpp + sts_arima_eval.hpp compiled for the host) against the straight-line optimizer over the pure-Python evaluation:
  status, coefficient bits, evaluation count; and its complete output, passes over the series
  included, against the recorded tests/golden/cg_paths.json;
* tests/native/arima_ref_eval.cpp (the same straight-line evaluation in C, used to drive the
  straight-line optimizer quickly in the GPU tests) bit for bit against the Python evaluation.
GPU: the HIP path through the mirror and the C ABI -- likelihood / gradient, fits, effects and
forecasts bit-exact against the restatement; the Hannan-Rissanen start within 1e-10.
"""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import arima_ref as ar
import oracle
from layout_arena import OUT_FILL, POISONS, bits, carve, layout
from mt19937 import MersenneTwister

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "native", "arima_sm_harness.cpp")
REF_EVAL = os.path.join(ROOT, "tests", "native", "arima_ref_eval.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
PATHS = os.path.join(GOLDEN, "cg_paths.json")
CHUNK = 64          # sts::kArimaChunk, the fit kernel's LDS chunk length


def data_set(i):
    return np.loadtxt(os.path.join(GOLDEN, "R_ARIMA_DataSet%d.csv" % i))


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def arma_panel(seed, S, T, p, q, level=0.0, d=0):
    """S stationary, invertible ARMA(p, q) series around `level`, integrated d times"""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(S):
        phi = rng.uniform(-0.5, 0.5, p)
        theta = rng.uniform(-0.5, 0.5, q)
        if p and np.abs(phi).sum() > 0.8:
            phi *= 0.8 / np.abs(phi).sum()
        if q and np.abs(theta).sum() > 0.8:
            theta *= 0.8 / np.abs(theta).sum()
        e = rng.standard_normal(T + 60)
        y = np.zeros(T + 60)
        for t in range(4, T + 60):
            y[t] = e[t] + sum(phi[j] * y[t - 1 - j] for j in range(p)) + sum(theta[j] * e[t - 1 - j] for j in range(q))
        y = y[60:] + level
        for _ in range(d):
            y = np.cumsum(y)
        rows.append(y)
    return np.array(rows)


def start_for(p, q, icpt, y):
    """the restated Hannan-Rissanen start, or a constant where it does not exist"""
    n = ar.n_coef(p, q, icpt)
    try:
        b = ar.hannan_rissanen(p, q, y, icpt)
        if np.isfinite(b).all():
            return b
    except (ar.Singular, ValueError, oracle.OracleError):
        pass
    return np.full(n, 0.1)


# ---------------- native helpers (host builds, as tests/test_garch.py does) ----------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("arima") / "arima_sm")
    build_harness(gxx, out)
    return out


def build_harness(gxx, out):
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "spark-timeseries_amd", "csrc"), HARNESS, "-o", out])


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    oracle.lib()
    out = str(tmp_path_factory.mktemp("arima_ref") / "libarima_ref_eval.so")
    lib_dir = os.path.join(ROOT, "oracle", "_build")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", REF_EVAL,
                           "-L", lib_dir, "-lsts_oracle", "-Wl,-rpath," + lib_dir, "-o", out])
    return ctypes.CDLL(out)


def harness_lines(harness, p, q, icpt, Y, init):
    """the harness's output, one line per row of Y: status, coefficient bits, evaluations, passes"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    init = np.ascontiguousarray(init, dtype=np.float64)
    inp = "%d %d %d %d %d\n" % (p, q, int(bool(icpt)), Y.shape[0], Y.shape[1])
    inp += " ".join("%x" % v for v in Y.view(np.uint64).ravel()) + "\n"
    inp += " ".join("%x" % v for v in init.view(np.uint64).ravel())
    return subprocess.run([harness], input=inp, capture_output=True, text=True, check=True).stdout.splitlines()


def run_harness(harness, p, q, icpt, Y, init):
    """-> list of (status, coefficients, evaluations, passes) per row of Y (already differenced)"""
    res = []
    for line in harness_lines(harness, p, q, icpt, Y, init):
        f = line.split()
        n = len(f) - 3
        coef = np.array([int(x, 16) for x in f[1:1 + n]], dtype=np.uint64).view(np.float64)
        res.append((int(f[0]), coef, int(f[1 + n]), int(f[2 + n])))
    return res


def ref_fit(ref_lib, p, d, q, icpt, ts, init):
    """the straight-line optimizer of arima_ref over the C evaluation -> (status, coef, evals)"""
    y = ar.diffed(ts, d)
    return ar.fit_css_cgd(p, q, icpt, y, init, ev=ar.CEval(ref_lib, p, q, icpt, y))


# ---------------- CPU: restatement anchors ----------------

@pytest.mark.parametrize("T", [200, 201])
@pytest.mark.parametrize("p,q", [(1, 1), (2, 2)])
def test_gradient_is_the_likelihoods_derivative(p, q, T):
    """Even n: the restated gradient is the central finite difference of the restated likelihood
    within 1e-6 relative.  Odd n: the likelihood's `(-n / 2)` is Int division while the gradient
    uses n, so the finite difference is (n - 1) / n of the gradient; that ratio is asserted."""
    y = arma_panel(11 * p + q, 1, T, p, q, level=2.0)[0]
    coef = np.concatenate([[1.7], np.full(p, 0.15), np.full(q, -0.2)]) + 0.05 * np.arange(1 + p + q)
    g = ar.gradient_css_arma(p, q, coef, True, y)
    fd = np.zeros_like(g)
    for j in range(coef.size):
        h = 1e-5 * max(1.0, abs(coef[j]))
        up, dn = coef.copy(), coef.copy()
        up[j] += h
        dn[j] -= h
        fd[j] = (ar.loglik_css_arma(p, q, up, True, y) - ar.loglik_css_arma(p, q, dn, True, y)) / (up[j] - dn[j])
    want = g if T % 2 == 0 else g * (T - 1) / T
    rel = np.abs(fd - want) / np.abs(want)
    print("p=%d q=%d T=%d gradient %s fd %s rel %s" % (p, q, T, g, fd, rel))
    assert (rel <= 1e-6).all()


def test_c_evaluation_is_the_python_evaluation(ref_lib):
    rng = np.random.default_rng(5)
    for p, q, icpt, T in ((1, 1, True, 50), (2, 2, True, 51), (0, 1, True, 30), (4, 4, True, 80), (1, 2, False, 40),
                          (3, 1, True, 3), (0, 0, True, 20)):
        y = arma_panel(T + p, 1, T, p, q, level=1.0)[0]
        ev = ar.CEval(ref_lib, p, q, icpt, y)
        for _ in range(3):
            coef = rng.uniform(-0.5, 0.5, ar.n_coef(p, q, icpt))
            assert same_bits([ev.loglik(coef)], [ar.loglik_css_arma(p, q, coef, icpt, y)])
            assert same_bits(ev.gradient(coef), ar.gradient_css_arma(p, q, coef, icpt, y))


def fit_from_hr(harness, p, d, q, icpt, ts):
    y = ar.diffed(ts, d)
    init = ar.hannan_rissanen(p, q, y, icpt)
    st, coef, ev, _ = run_harness(harness, p, q, icpt, y[None, :], init[None, :])[0]
    assert st == ar.OK
    return coef


def test_suite_data_set_1(harness):
    # T/models/ARIMASuite.scala "compare with R" (1, 0, 1)
    c, a, m = fit_from_hr(harness, 1, 0, 1, True, data_set(1))
    assert abs(a - 0.3) <= 0.05 and abs(m - 0.7) <= 0.05


def test_suite_data_set_2(harness):
    # "Fitting an integrated time series of order 3"
    c, m = fit_from_hr(harness, 0, 3, 1, True, data_set(2))
    assert abs(m - 0.2) <= 0.05


def sample(p, d, q, coef, icpt, n, rand):
    """ARIMAModel.sample (:517-520)"""
    return ar.add_effects(p, d, q, coef, icpt, [rand.next_gaussian() for _ in range(n)])


def test_suite_sampled_model_is_recovered(harness):
    truth = np.array([8.2, 0.2, 0.5, 0.3, 0.1])
    ts = sample(2, 1, 2, truth, True, 1000, MersenneTwister(10))
    got = fit_from_hr(harness, 2, 1, 2, True, ts)
    assert abs(got[0] - truth[0]) <= 1
    assert (np.abs(got[1:] - truth[1:]) <= 0.1).all()


def test_suite_arima_is_arma_of_the_differences(harness):
    truth = np.array([0.3, 0.7, 0.1])
    ts = sample(1, 1, 2, truth, False, 1000, MersenneTwister(10))
    arima = fit_from_hr(harness, 1, 1, 2, False, ts)
    arma = fit_from_hr(harness, 1, 0, 2, False, oracle.differences_of_order_d(ts, 1)[1:])
    assert (np.abs(arima - truth) <= 0.05).all()
    assert same_bits(arima, arma)


def test_suite_arima_000_is_the_mean(harness):
    rand = MersenneTwister(10)
    ts = np.array([rand.next_gaussian() for _ in range(100)])
    got = fit_from_hr(harness, 0, 0, 0, True, ts)
    assert abs(got[0] - ts.sum() / ts.size) <= 1e-4


def test_suite_add_then_remove_round_trip():
    rand = MersenneTwister(20)
    coef = [8.3, 0.1, 0.2, 0.3]
    noise = np.array([rand.next_gaussian() for _ in range(100)])
    back = ar.remove_effects(1, 1, 2, coef, True, ar.add_effects(1, 1, 2, coef, True, noise))
    assert (np.abs(back - noise) < 1e-4).all()


def test_suite_stationarity_and_invertibility():
    from sparkts.models.ARIMA import ARIMAModel
    for p, q, coef, stationary, invertible in ((1, 0, [0.2, 1.5], False, True), (0, 1, [0.13, 1.8], True, False),
                                               (2, 0, [0.003359, 1.545, -0.5646], True, True),
                                               (1, 1, [-0.09341, 0.857361, -0.300821], True, True)):
        m = ARIMAModel(p, 0, q, np.array(coef), True)
        assert m.isStationary() is stationary and m.isInvertible() is invertible
    panel = ARIMAModel(1, 0, 1, np.array([[0.0, 1.5, 0.3], [0.0, 0.5, 1.8]]))
    assert list(panel.isStationary()) == [False, True] and list(panel.isInvertible()) == [True, False]


# ---------------- CPU: the state machine against the straight-line optimizer ----------------

MACHINE_CASES = [(1, 1, True, 250), (1, 1, True, 65), (1, 1, True, 24), (2, 2, True, 250), (2, 2, True, 65),
                 (0, 1, True, 65), (0, 1, True, 24), (3, 1, True, 250), (3, 1, True, 24), (0, 0, True, 65),
                 (1, 2, False, 250), (1, 2, False, 24),
                 # the bracket's parabolic point lies between xB and xC and xB beats it; it beats neither
                 (1, 1, False, 40), (0, 2, True, 12)]


def machine_case(p, q, icpt, T):
    y = arma_panel(1000 * p + 100 * q + T, 1, T, p, q, level=3.0)[0]
    return y, start_for(p, q, icpt, y)


@pytest.mark.parametrize("p,q,icpt,T", MACHINE_CASES)
def test_state_machine_matches_straight_line_optimizer(harness, p, q, icpt, T):
    y, init = machine_case(p, q, icpt, T)
    st, coef, ev, _ = run_harness(harness, p, q, icpt, y[None, :], init[None, :])[0]
    rst, rcoef, rev = ar.fit_css_cgd(p, q, icpt, y, init)
    assert (st, ev) == (rst, rev)
    assert same_bits(coef, rcoef)


def edge_series(kind, T=24):
    y = arma_panel(77, 1, T, 1, 1, level=1.0)[0]
    if kind == "nan":
        y[T // 2] = np.nan
    elif kind == "constant":
        y[:] = 4.25
    return y


EDGE_CASES = [("nan", 1, 1), ("constant", 1, 1), ("short", 3, 1)]


def edge_case(kind, p, q):
    y = edge_series(kind)[:3] if kind == "short" else edge_series(kind)
    return y, np.full(1 + p + q, 0.1)


@pytest.mark.parametrize("kind,p,q", EDGE_CASES)
def test_state_machine_edge_series(harness, kind, p, q):
    """A series with a NaN runs to TooManyEvaluations; a constant one and one no longer than
    max(p, q) (every likelihood NaN) end however the reference's optimizer ends on them."""
    y, init = edge_case(kind, p, q)
    st, coef, ev, _ = run_harness(harness, p, q, True, y[None, :], init[None, :])[0]
    rst, rcoef, rev = ar.fit_css_cgd(p, q, True, y, init)
    print(kind, "status", st, "evaluations", ev)
    assert (st, ev) == (rst, rev)
    assert same_bits(coef, rcoef)
    if kind == "nan":
        assert st == ar.TOO_MANY_EVALUATIONS


def path_cases():
    """name -> (p, q, icpt, y, init): the inputs whose complete harness lines
    tests/golden/cg_paths.json records"""
    cases = {"p%d_q%d_icpt%d_T%d" % (p, q, icpt, T): (p, q, icpt, *machine_case(p, q, icpt, T))
             for p, q, icpt, T in MACHINE_CASES}
    cases.update(("edge_" + kind, (p, q, True, *edge_case(kind, p, q))) for kind, p, q in EDGE_CASES)
    return cases


def test_optimizer_paths_are_the_recorded_ones(harness):
    """Status, point bits, evaluations AND passes, character for character: the passes are what
    the evaluation caches decide and what the device time follows.

    The passes of edge_nan and edge_constant also depend on something no cache decides: once the
    point and the direction are NaN, `point + t * dir` compares equal to the point, bit for bit,
    only when the sum keeps the point's NaN payload rather than the direction's, and which
    operand's payload an x86 addsd keeps is the compiler's choice of operand order.  Status,
    coefficients and evaluations are the same either way.  A difference in these two lines alone
    points at how g++ ordered `g + beta * dir` in arima_advance, not at the cache: naming the
    gradient in a local before the restart test was enough to flip it (3420 -> 9870 passes)."""
    with open(PATHS) as f:
        golden = json.load(f)["arima"]
    cases = path_cases()
    assert sorted(golden) == sorted(cases)
    for name, (p, q, icpt, y, init) in cases.items():
        assert harness_lines(harness, p, q, icpt, y[None, :], init[None, :]) == golden[name], name


# ---------------- the Hannan-Rissanen inputs of the GPU test ----------------

HR_SHAPE = (16, 250)
HR_ORDERS = [(1, 0, 1), (2, 1, 2), (0, 0, 1), (3, 0, 1)]
HR_LEVELS = [0.0, 8.2, 50.0]


def hr_panel(p, d, q, level):
    return arma_panel(1000 + int(level) + 7 * p + q, HR_SHAPE[0], HR_SHAPE[1], p, q, level=level, d=d)


@pytest.mark.parametrize("level", HR_LEVELS)
@pytest.mark.parametrize("p,d,q", HR_ORDERS)
def test_hannan_rissanen_inputs_stay_under_the_condition_cap(p, d, q, level):
    """The seeds of test_gpu_hannan_rissanen_start keep the restated second-stage design's
    column-scaled condition number at most 1e4 (checked here, where no GPU is needed)."""
    x = hr_panel(p, d, q, level)
    conds = [ar.scaled_condition(ar.hr_design(p, q, ar.diffed(row, d), True)[1]) for row in x]
    print("p=%d d=%d q=%d level=%g: condition numbers up to %.3g" % (p, d, q, level, max(conds)))
    assert max(conds) <= 1e4


# ---------------- errors that need no device ----------------

def test_refused_orders_and_methods():
    from sparkts.errors import IllegalArgumentException, UnsupportedOperationException
    from sparkts.models.ARIMA import ARIMA, ARIMAModel
    ts = np.zeros(50)
    with pytest.raises(IllegalArgumentException):
        ARIMA.fitModelCSS(5, 0, 1, ts)
    with pytest.raises(IllegalArgumentException):
        ARIMA.fitModelCSS(0, 0, 0, ts, includeIntercept=False)
    with pytest.raises(UnsupportedOperationException):
        ARIMA.fitModelCSS(1, 0, 1, ts, method="css-bobyqa")
    with pytest.raises(UnsupportedOperationException, match="fitModelCSS"):
        ARIMA.fitModel(1, 0, 1, ts)
    with pytest.raises(IllegalArgumentException):
        ARIMAModel(1, 0, 5, np.zeros(7)).forecast(ts, 3)


# ---------------- GPU ----------------

def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


def host(t):
    return t.detach().cpu().numpy()


def random_coef(seed, S, p, q, icpt=True):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (S, ar.n_coef(p, q, icpt)))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [200, 201])
@pytest.mark.parametrize("p,d,q", [(1, 0, 1), (2, 1, 2), (0, 2, 1), (4, 0, 4)])
def test_gpu_likelihood_and_gradient_bit_exact(p, d, q, T):
    from sparkts.models.ARIMA import ARIMAModel
    S = 40
    x = arma_panel(3 + p + 10 * q + T, S, T, p, q, level=1.0, d=d)
    coef = random_coef(T + p, S, p, q)
    m = ARIMAModel(p, d, q, dev(coef), True)
    ll = host(m.logLikelihoodCSS(dev(x)))
    g = host(m.gradientlogLikelihoodCSS(dev(x)))
    rll = np.array([ar.loglik_css(p, d, q, coef[s], True, x[s]) for s in range(S)])
    rg = np.array([ar.gradient_css(p, d, q, coef[s], True, x[s]) for s in range(S)])
    assert same_bits(ll, rll)
    assert same_bits(g, rg)


def check_fit(ref_lib, p, d, q, x, init, icpt=True):
    import torch
    from sparkts.models.ARIMA import ARIMA
    S = x.shape[0]
    err = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    m = ARIMA.fitModelCSS(p, d, q, dev(x), includeIntercept=icpt, userInitParams=init, errors=err)
    coef, ev, err = host(m.coefficients), host(m.evaluations), host(err)
    statuses = []
    for s in range(S):
        rst, rcoef, rev = ref_fit(ref_lib, p, d, q, icpt, x[s], init[s])
        statuses.append(rst)
        assert (int(err[s]), int(ev[s])) == (rst, rev), s
        if rst == ar.OK:
            assert same_bits(coef[s], rcoef), s
        else:
            assert np.isnan(coef[s]).all(), s
    return statuses


def starts(p, d, q, x, icpt=True):
    return np.array([start_for(p, q, icpt, ar.diffed(row, d)) for row in x])


@pytest.mark.gpu
def test_gpu_fit_panel_with_nan_and_constant_series(ref_lib):
    p, d, q = 1, 0, 1
    x = arma_panel(21, 70, 250, p, q, level=5.0)
    x[17, 100] = np.nan
    x[40, :] = -2.5
    st = check_fit(ref_lib, p, d, q, x, starts(p, d, q, x))
    assert st[17] == ar.TOO_MANY_EVALUATIONS and st.count(ar.OK) >= 68


@pytest.mark.gpu
@pytest.mark.parametrize("S,T", [(33, 65), (5, 4)])
def test_gpu_fit_212(ref_lib, S, T):
    # T = 4 is max(p, q) + 1 + d: one residual per series
    p, d, q = 2, 1, 2
    x = arma_panel(31 + T, S, T, p, q, level=1.0, d=d)
    check_fit(ref_lib, p, d, q, x, starts(p, d, q, x))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_gpu_fit_around_the_lds_chunk(ref_lib, T):
    p, d, q = 1, 0, 1
    x = arma_panel(41 + T, 6, T, p, q, level=-3.0)
    check_fit(ref_lib, p, d, q, x, starts(p, d, q, x))


@pytest.mark.gpu
def test_gpu_fit_data_set_1(ref_lib):
    x = data_set(1)[None, :]
    st = check_fit(ref_lib, 1, 0, 1, x, starts(1, 0, 1, x))
    assert st == [ar.OK]


@pytest.mark.gpu
def test_gpu_fit_without_intercept(ref_lib):
    p, d, q = 1, 1, 2
    x = arma_panel(51, 9, 120, p, q, d=d)
    check_fit(ref_lib, p, d, q, x, starts(p, d, q, x, icpt=False), icpt=False)


@pytest.mark.gpu
@pytest.mark.parametrize("level", HR_LEVELS)
@pytest.mark.parametrize("p,d,q", HR_ORDERS)
def test_gpu_hannan_rissanen_start(p, d, q, level):
    """1e-10 relative (the project's OLS bar) to the restated start, against the largest
    coefficient magnitude of the series; the restated second-stage design's column-scaled
    condition number is at most 1e4 for every series compared (none is skipped)."""
    import torch
    from sparkts import _native
    from sparkts._panel import Panel, ptr
    S, T = HR_SHAPE
    x = hr_panel(p, d, q, level)
    t = dev(x)
    pn = Panel(t)
    n = ar.n_coef(p, q, True)
    init = torch.empty((S, n), dtype=torch.float64, device="cuda:0")
    err = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    st = _native.lib().sts_arima_hr_init(ptr(t), S, T, pn.ld, p, d, q, 1, ptr(init), ptr(err), pn.stream)
    assert st == 0 and not host(err).any()
    got = host(init)
    worst, worst_cond = 0.0, 0.0
    for s in range(S):
        y = ar.diffed(x[s], d)
        resp, X = ar.hr_design(p, q, y, True)
        cond = ar.scaled_condition(X)
        worst_cond = max(worst_cond, cond)
        assert cond <= 1e4, (s, cond)
        ref = ar.hannan_rissanen(p, q, y, True)
        worst = max(worst, np.abs(got[s] - ref).max() / np.abs(ref).max())
    print("p=%d d=%d q=%d level=%g: worst relative error %.3g, worst condition number %.3g"
          % (p, d, q, level, worst, worst_cond))
    assert worst <= 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("p,d,q", [(1, 0, 1), (2, 1, 2)])
def test_gpu_fit_from_its_own_start(ref_lib, p, d, q):
    """The optimizer stage bit-exact given the device's start (as test_gpu_argarch_fit treats
    its AR stage)."""
    import torch
    from sparkts.models.ARIMA import ARIMA
    S = 20
    x = arma_panel(61 + p, S, 250, p, q, level=8.2, d=d)
    err = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    m = ARIMA.fitModelCSS(p, d, q, dev(x), errors=err)
    init, coef, ev, err = host(m.initParams), host(m.coefficients), host(m.evaluations), host(err)
    n_ok = 0
    for s in range(S):
        # a wild start (near-cancelling AR and MA roots) can run the reference out of evaluations
        rst, rcoef, rev = ref_fit(ref_lib, p, d, q, True, x[s], init[s])
        assert (int(err[s]), int(ev[s])) == (rst, rev), s
        if rst == ar.OK:
            n_ok += 1
            assert same_bits(coef[s], rcoef), s
        else:
            assert np.isnan(coef[s]).all(), s
    assert n_ok >= S - 2


@pytest.mark.gpu
def test_gpu_fit_ar_only_is_fitmodel():
    from sparkts.models.ARIMA import ARIMA
    x = dev(arma_panel(71, 8, 120, 2, 0, level=1.0, d=1))
    a, b = ARIMA.fitModelCSS(2, 1, 0, x), ARIMA.fitModel(2, 1, 0, x)
    assert same_bits(host(a.coefficients), host(b.coefficients))


EFFECT_ORDERS = [(1, 1, 2), (2, 0, 0), (0, 1, 1), (4, 2, 4)]


def effect_case(p, d, q, short):
    S = 37
    T = d + max(p, q) + 1 if short else 300
    x = arma_panel(81 + p + q + T, S, T, min(p, 2), min(q, 2), level=2.0, d=d)
    coef = random_coef(91 + T, S, p, q) * 0.8
    return S, T, x, coef


@pytest.mark.gpu
@pytest.mark.parametrize("short", [False, True])
@pytest.mark.parametrize("p,d,q", EFFECT_ORDERS)
def test_gpu_remove_and_add_bit_exact(p, d, q, short):
    import torch
    from sparkts.models.ARIMA import ARIMAModel
    S, T, x, coef = effect_case(p, d, q, short)
    m = ARIMAModel(p, d, q, dev(coef), True)
    ref_rm = np.array([ar.remove_effects(p, d, q, coef[s], True, x[s]) for s in range(S)])
    ref_add = np.array([ar.add_effects(p, d, q, coef[s], True, x[s]) for s in range(S)])
    for fn, ref in ((m.removeTimeDependentEffects, ref_rm), (m.addTimeDependentEffects, ref_add)):
        ts = dev(x)
        out = fn(ts, torch.zeros_like(ts))
        assert same_bits(host(out), ref)
        assert same_bits(host(ts), x)
        assert same_bits(host(fn(ts, ts)), ref)      # dest is ts: the out-of-place result


@pytest.mark.gpu
@pytest.mark.parametrize("n_future", [0, 1, 7])
@pytest.mark.parametrize("short", [False, True])
@pytest.mark.parametrize("p,d,q", EFFECT_ORDERS)
def test_gpu_forecast_bit_exact(p, d, q, short, n_future):
    from sparkts.models.ARIMA import ARIMAModel
    S, T, x, coef = effect_case(p, d, q, short)
    got = host(ARIMAModel(p, d, q, dev(coef), True).forecast(dev(x), n_future))
    ref = np.array([ar.forecast(p, d, q, coef[s], True, x[s], n_future) for s in range(S)])
    assert got.shape == (S, T + n_future)
    assert same_bits(got, ref)


@pytest.mark.gpu
def test_gpu_forecast_d3_fitted_part_within_2_ulp():
    """d = 3: the order of Breeze's sum over the three difference levels (:591) is not pinned, so
    the fitted part [d, T - d) is held to 2 ulp; everything else holds no such sum and is exact."""
    from sparkts.models.ARIMA import ARIMAModel
    p, d, q, S, T, nf = 1, 3, 1, 37, 300, 7
    x = arma_panel(101, S, T, p, q, level=0.5, d=d)
    coef = random_coef(102, S, p, q) * 0.8
    got = host(ARIMAModel(p, d, q, dev(coef), True).forecast(dev(x), nf))
    ref = np.array([ar.forecast(p, d, q, coef[s], True, x[s], nf) for s in range(S)])
    fitted = slice(d, T - d)
    ulps = np.abs(got[:, fitted].view(np.int64) - ref[:, fitted].view(np.int64))
    print("d = 3 fitted part: max ulp distance", ulps.max())
    assert ulps.max() <= 2
    assert same_bits(got[:, :d], ref[:, :d]) and same_bits(got[:, T - d:], ref[:, T - d:])


# ---- layout: padded and odd-base panels (tests/layout_arena.py) ----

def _abi():
    from sparkts import _native
    _native.ensure_device(0)
    return _native.lib()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["even", "skew"])
@pytest.mark.parametrize("op", ["remove", "add", "forecast"])
def test_gpu_layout_effects_and_forecast(op, name):
    import torch
    lib = _abi()
    p, d, q, S, T, nf = 1, 1, 2, 5, 70, 3
    TO = T + nf if op == "forecast" else T
    x = arma_panel(111, S, T, p, q, level=1.0, d=d)
    coef = dev(random_coef(112, S, p, q) * 0.8)

    def run(ld_in, ld_out, base_in, base_out, poison):
        a_in = carve(S, T, ld_in, base_in, poison, data=x)
        a_out = carve(S, TO, ld_out, base_out, OUT_FILL)
        s_in, s_out = a_in.snapshot(), a_out.snapshot()
        if op == "forecast":
            st = lib.sts_arima_forecast(a_in.ptr, a_out.ptr, S, T, ld_in, ld_out, p, d, q, 1, coef.data_ptr(), nf, None)
        else:
            fn = lib.sts_arima_remove if op == "remove" else lib.sts_arima_add
            st = fn(a_in.ptr, a_out.ptr, S, T, ld_in, ld_out, p, d, q, 1, coef.data_ptr(), None)
        assert st == 0
        torch.cuda.synchronize()
        a_in.verify_all(s_in)
        a_out.verify_outside(s_out)
        return a_out.data()

    packed = run(T, TO, 0, 0, POISONS["nan"])
    for poison in POISONS.values():
        assert same_bits(run(*layout(name, T, TO), poison), packed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["even", "skew"])
def test_gpu_layout_likelihood_and_fit(name):
    import torch
    lib = _abi()
    p, d, q, S, T = 1, 1, 1, 5, 70
    n = 3
    x = arma_panel(121, S, T, p, q, level=1.0, d=d)
    init = dev(starts(p, d, q, x))

    def run(ld_in, base_in, poison):
        a_in = carve(S, T, ld_in, base_in, poison, data=x)
        snap = a_in.snapshot()
        out = torch.full((2, S, n), OUT_FILL, dtype=torch.float64, device="cuda:0")
        ll = torch.full((S,), OUT_FILL, dtype=torch.float64, device="cuda:0")
        ev = torch.zeros(S, dtype=torch.int32, device="cuda:0")
        err = torch.zeros(S, dtype=torch.int32, device="cuda:0")
        assert lib.sts_arima_fit_css(a_in.ptr, S, T, ld_in, p, d, q, 1, init.data_ptr(), out[0].data_ptr(),
                                     err.data_ptr(), ev.data_ptr(), None) == 0
        assert lib.sts_arima_css_loglik_gradient(a_in.ptr, S, T, ld_in, p, d, q, 1, init.data_ptr(), ll.data_ptr(),
                                                 out[1].data_ptr(), None) == 0
        torch.cuda.synchronize()
        a_in.verify_all(snap)
        assert not host(err).any()
        return np.concatenate([host(out).ravel(), host(ll)]), host(ev)

    packed, pev = run(T, 0, POISONS["nan"])
    for poison in POISONS.values():
        ld_in, _, base_in, _ = layout(name, T)
        res, ev = run(ld_in, base_in, poison)
        assert same_bits(res, packed) and (ev == pev).all()
