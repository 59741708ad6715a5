"""Every ARIMA order, chunk seam and poisoned neighbour on the device.  Needs an MI355X.

csrc/sts_arima.hip indexes its per-lane arrays (phi[4], theta[4], hist, ma, the ring in LDS, the
Hannan-Rissanen kernel's fixed slots) by guarded constants in unrolled loops, shifts every
coefficient by the intercept flag, and streams rows through LDS in 64-step chunks.  A wrong
guard shows only at the order that uses the slot, a wrong shift only without intercept, a wrong
carry only at a seam.  So:

  2. all 49 (p, q, intercept) orders, d cycling through 0, 1, 2, through the likelihood and the
     gradient, the fit, remove / add and forecast: bit for bit the restatement (tests/arima_ref.py;
     the C evaluation where test_arima_orders_cpu.py anchors it), with the differenced length and
     T around the chunk and the forecasts' forward phase starting, ending and spanning on every
     side of a chunk's edge;
  3. the Hannan-Rissanen start as a reduction at the header's bar (1e-10 of the series' largest
     coefficient on designs conditioned at most 1e4, per-series status 0): every order, two
     blocks, padded and odd-base layouts, data scaled by 2^+-300;
  4. ten poison rows in lanes 0, 1, 31, 32, 63 of the fit's 64-series waves and at the edges of
     the 32-series effects waves: the clean series are bit-identical to the same call on the
     clean panel, and every series, the poisoned ones included, equals the restatement.

The inputs, their seeds and the CPU-side facts (condition cap, convergence share, what the
restated fit does on the poisons) live in tests/test_arima_orders_cpu.py.
"""
import numpy as np
import pytest

import arima_ref as ar
import layout_arena as la
import test_arima_orders_cpu as oc
import test_scale_cpu as sc
from test_arima import (_abi, arma_panel, check_fit, dev, host, random_coef, ref_fit, ref_lib,  # noqa: F401
                        same_bits, starts)
from test_isolation_gpu import LANE_SLOTS, POISONS, SINGULAR, clean_mask

pytestmark = pytest.mark.gpu
cache = sc.cache

ORDERS = oc.ORDERS
CASES = list(enumerate(ORDERS))
S_WAVES = 97                      # one full css wave + 33 lanes; three full effects waves + 1 lane
HR_BAR = 1e-10


def case_id(c):
    return oc.order_id(c[1])


def torch_i32(S, fill=0):
    import torch
    return torch.full((S,), fill, dtype=torch.int32, device="cuda:0")


def torch_f64(shape, fill=la.OUT_FILL):
    import torch
    return torch.full(shape, fill, dtype=torch.float64, device="cuda:0")


def sync():
    import torch
    torch.cuda.synchronize()


# ---------------- 2. every order, bit for bit ----------------

@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_likelihood_and_gradient_every_order(ref_lib, case):
    from sparkts.models.ARIMA import ARIMAModel
    i, (p, q, icpt) = case
    d, N = oc.diff_order(p, q), 64 + i % 2
    S, T = S_WAVES, d + N
    x = arma_panel(5000 + i, S, T, p, q, level=1.0, d=d)
    coef = random_coef(5100 + i, S, p, q, icpt)
    m = ARIMAModel(p, d, q, dev(coef), bool(icpt))
    ll = host(m.logLikelihoodCSS(dev(x)))
    g = host(m.gradientlogLikelihoodCSS(dev(x)))
    evs = [ar.CEval(ref_lib, p, q, icpt, ar.diffed(x[s], d)) for s in range(S)]
    assert same_bits(ll, np.array([evs[s].loglik(coef[s]) for s in range(S)]))
    assert same_bits(g, np.array([evs[s].gradient(coef[s]) for s in range(S)]))


def fit_abi(p, d, q, icpt, x, init):
    """sts_arima_fit_css -> (coefficients, status, evaluations) per series"""
    S, T = x.shape
    n = ar.n_coef(p, q, icpt)
    t, i0 = dev(x), dev(init)
    coef, err, ev = torch_f64((S, n)), torch_i32(S), torch_i32(S)
    assert _abi().sts_arima_fit_css(t.data_ptr(), S, T, T, p, d, q, icpt, i0.data_ptr(), coef.data_ptr(),
                                    err.data_ptr(), ev.data_ptr(), None) == 0
    sync()
    return host(coef), host(err), host(ev)


def assert_fit_is(got, want):
    """got: fit_abi's triple; want: [(status, coefficients, evaluations)] of the restatement"""
    coef, err, ev = got
    for s, (rst, rcoef, rev) in enumerate(want):
        assert (int(err[s]), int(ev[s])) == (rst, rev), s
        if rst == ar.OK:
            assert same_bits(coef[s], rcoef), s
        else:
            assert np.isnan(coef[s]).all(), s


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_fit_every_order(ref_lib, case):
    """ARIMA.fitModelCSS hands p > 0, q = 0 to the AR path as the reference does (:84-90), so
    for those orders the same assertions run on sts_arima_fit_css itself."""
    i, (p, q, icpt) = case
    d = oc.diff_order(p, q)
    x = oc.fit_panel(p, q, icpt)
    init = starts(p, d, q, x, icpt=bool(icpt))
    if p > 0 and q == 0:
        want = oc.fit_reference(ref_lib, (p, q, icpt))
        assert_fit_is(fit_abi(p, d, q, icpt, x, init), want)
        statuses = [st for st, _, _ in want]
    else:
        statuses = check_fit(ref_lib, p, d, q, x, init, icpt=bool(icpt))
    assert statuses.count(ar.OK) >= 8


EFFECT_T = [64, 65, 129]
for _T in range(3):     # every T meets at least 15 orders and both intercept settings
    assert sum(i % 3 == _T for i, _ in CASES) >= 15 and {o[2] for i, o in CASES if i % 3 == _T} == {0, 1}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_remove_and_add_every_order(case):
    import torch
    from sparkts.models.ARIMA import ARIMAModel
    i, (p, q, icpt) = case
    d, S, T = oc.diff_order(p, q), S_WAVES, EFFECT_T[i % 3]
    x = arma_panel(5200 + i, S, T, min(p, 2), min(q, 2), level=2.0, d=d)
    coef = random_coef(5300 + i, S, p, q, icpt) * 0.8
    m = ARIMAModel(p, d, q, dev(coef), bool(icpt))
    ref_rm = np.array([ar.remove_effects(p, d, q, coef[s], icpt, x[s]) for s in range(S)])
    ref_add = np.array([ar.add_effects(p, d, q, coef[s], icpt, x[s]) for s in range(S)])
    for fn, ref in ((m.removeTimeDependentEffects, ref_rm), (m.addTimeDependentEffects, ref_add)):
        ts = dev(x)
        out = fn(ts, torch.zeros_like(ts))
        assert same_bits(host(out), ref)
        assert same_bits(host(ts), x)
        assert same_bits(host(fn(ts, ts)), ref)      # dest is ts: the out-of-place result


# (T, n_future); T = None is the shortest legal series, d + max(p, q) + 1.  Every order runs
# every seam.
FORECAST_SEAMS = [(60, 4),      # TO ends on a chunk's last step
                  (60, 5),      # ... one step past it
                  (64, 1),      # the forward phase starts on a chunk's first step
                  (63, 70),     # the forward phase spans a whole chunk; d = 2: the tail integration is longer than one
                  (None, 130)]  # the shortest series with a three-chunk forward curve


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_forecast_every_order_and_seam(case):
    from sparkts.models.ARIMA import ARIMAModel
    i, (p, q, icpt) = case
    d, S = oc.diff_order(p, q), S_WAVES
    full = arma_panel(5400 + i, S, 64, min(p, 2), min(q, 2), level=2.0, d=d)
    coef = random_coef(5500 + i, S, p, q, icpt) * 0.8
    m = ARIMAModel(p, d, q, dev(coef), bool(icpt))
    for T, nf in FORECAST_SEAMS:
        T = d + max(p, q) + 1 if T is None else T
        x = np.ascontiguousarray(full[:, :T])
        got = host(m.forecast(dev(x), nf))
        ref = np.array([ar.forecast(p, d, q, coef[s], icpt, x[s], nf) for s in range(S)])
        assert got.shape == (S, T + nf)
        assert same_bits(got, ref), (T, nf)


# ---------------- 3. the Hannan-Rissanen start as a pinned reduction ----------------

def hr_call(x, p, d, q, icpt, ld=None, ptr=None):
    """sts_arima_hr_init on a packed copy of x (or on the panel at ptr / ld) -> (start, status)"""
    S, T = x.shape
    t = dev(x) if ptr is None else None
    init, err = torch_f64((S, ar.n_coef(p, q, icpt))), torch_i32(S)
    st = _abi().sts_arima_hr_init(t.data_ptr() if ptr is None else ptr, S, T, T if ld is None else ld, p, d, q, icpt,
                                  init.data_ptr(), err.data_ptr(), None)
    assert st == 0
    sync()
    return host(init), host(err)


def hr_worst(got, x, p, d, q, icpt, rows=None):
    """-> (worst error relative to the series' largest restated coefficient, worst condition
    number) over the rows; every row's condition number is asserted, none is skipped"""
    worst, worst_cond = 0.0, 0.0
    for s in range(len(x)) if rows is None else rows:
        y = ar.diffed(x[s], d)
        cond = ar.scaled_condition(ar.hr_design(p, q, y, icpt)[1])
        assert cond <= oc.HR_CAP, (s, cond)
        ref = ar.hannan_rissanen(p, q, y, icpt)
        worst = max(worst, np.abs(got[s] - ref).max() / np.abs(ref).max())
        worst_cond = max(worst_cond, cond)
    return worst, worst_cond


@pytest.mark.parametrize("order", ORDERS, ids=oc.order_id)
def test_gpu_hr_start_every_order(order):
    p, q, icpt = order
    worst, worst_cond = 0.0, 0.0
    for level in oc.HR_LEVELS:
        for d in oc.HR_DIFFS:
            x = oc.hr_panel(p, q, level, d)
            got, err = hr_call(x, p, d, q, icpt)
            assert not err.any(), (level, d, err)
            w, c = hr_worst(got, x, p, d, q, icpt)
            worst, worst_cond = max(worst, w), max(worst_cond, c)
    print("p=%d q=%d icpt=%d: worst relative error %.3g, worst condition number %.3g" % (p, q, icpt, worst, worst_cond))
    assert worst <= HR_BAR


@pytest.mark.parametrize("p,d,q,icpt,level", oc.HR_LANES)
def test_gpu_hr_start_two_blocks(p, d, q, icpt, level):
    x = oc.hr_lane_panel(p, d, q, level)
    assert len(x) == 130
    got, err = hr_call(x, p, d, q, icpt)
    assert not err.any()
    worst, worst_cond = hr_worst(got, x, p, d, q, icpt)
    print("p=%d d=%d q=%d icpt=%d S=130: worst relative error %.3g, worst condition number %.3g"
          % (p, d, q, icpt, worst, worst_cond))
    assert worst <= HR_BAR


@pytest.mark.parametrize("name", ["even", "skew"])
@pytest.mark.parametrize("p,d,q,icpt", [(2, 0, 2, 1), (4, 1, 3, 0)])   # d = 0: the kernels read the arena itself
def test_gpu_hr_start_layouts(p, d, q, icpt, name):
    S, T = 5, 70
    x = np.ascontiguousarray(oc.hr_panel(p, q, 8.2, d)[:S, :T])

    def run(ld_in, base_in, poison):
        a_in = la.carve(S, T, ld_in, base_in, poison, data=x)
        snap = a_in.snapshot()
        got, err = hr_call(x, p, d, q, icpt, ld=ld_in, ptr=a_in.ptr)
        a_in.verify_all(snap)
        assert not err.any()
        return got

    packed = run(T, 0, la.POISONS["nan"])
    assert np.isfinite(packed).all()
    for poison in la.POISONS.values():
        ld_in, _, base_in, _ = la.layout(name, T)
        assert same_bits(run(ld_in, base_in, poison), packed)


@pytest.mark.parametrize("k", oc.HR_SCALES)
@pytest.mark.parametrize("icpt", [1, 0])
@pytest.mark.parametrize("p,d,q", oc.HR_SCALED)
def test_gpu_hr_start_scaled(p, d, q, icpt, k):
    """The panel times 2^k, k = +-300 (Gram entries near 2^+-600).  Expected: the restated start
    of the unscaled panel with its intercept times 2^k -- the restatement on the scaled panel is
    exactly that (test_restated_hr_start_is_equivariant_under_power_of_two_scaling), so |k| is
    not lowered.  The device's intercept is brought back by 2^-k (exact) before the comparison:
    measured against a largest coefficient of 8.2 * 2^300 the other coefficients would not count."""
    worst, worst_cond = 0.0, 0.0
    for level in oc.HR_LEVELS:
        x = oc.hr_panel(p, q, level, d)
        got, err = hr_call(sc.scaled(x, k), p, d, q, icpt)
        assert not err.any(), (level, err)
        if icpt:
            got[:, 0] = np.ldexp(got[:, 0], -k)
        w, c = hr_worst(got, x, p, d, q, icpt)
        worst, worst_cond = max(worst, w), max(worst_cond, c)
    print("p=%d d=%d q=%d icpt=%d k=%d: worst relative error %.3g, worst condition number %.3g"
          % (p, d, q, icpt, k, worst, worst_cond))
    assert worst <= HR_BAR


# ---------------- 4. poisoned neighbours ----------------

OK_ROWS = clean_mask(oc.NEIGHBOUR_SHAPE[0], LANE_SLOTS)
NF = 7


@cache
def neighbour_starts(p, d, q, icpt):
    """-> the restated starts of (the clean panel, the poisoned panel); the clean rows are shared"""
    with np.errstate(all="ignore"):
        bad = starts(p, d, q, oc.neighbour_poisoned(p, d, q)[LANE_SLOTS], icpt=bool(icpt))
    clean = starts(p, d, q, oc.neighbour_clean(p, d, q), icpt=bool(icpt))
    x = clean.copy()
    x[LANE_SLOTS] = bad
    return sc.frozen(clean, x)


def both_panels(p, d, q):
    return oc.neighbour_clean(p, d, q), oc.neighbour_poisoned(p, d, q)


@pytest.mark.parametrize("p,d,q,icpt", oc.NEIGHBOUR_ORDERS)
def test_gpu_neighbours_fit(ref_lib, p, d, q, icpt):
    """The poisoned lanes run 10001 evaluations while their neighbours finish in about a hundred:
    the wave streams one lane's row for thousands of rounds."""
    clean, x = both_panels(p, d, q)
    i0, i1 = neighbour_starts(p, d, q, icpt)
    r0 = fit_abi(p, d, q, icpt, clean, i0)
    r1 = fit_abi(p, d, q, icpt, x, i1)
    for a, b in zip(r0, r1):
        assert same_bits(a[OK_ROWS], b[OK_ROWS])
    with np.errstate(all="ignore"):
        want = [ref_fit(ref_lib, p, d, q, icpt, x[s], i1[s]) for s in range(len(x))]
    assert_fit_is(r1, want)
    facts = [(int(r1[1][s]), int(r1[2][s])) for s in LANE_SLOTS]
    assert facts == oc.POISON_FITS[(p, d, q, icpt)]
    assert sum(st == ar.OK for st, _, _ in want) >= 2 * OK_ROWS.sum() // 3      # (the part-2 floor, 8 of 12)


@pytest.mark.parametrize("p,d,q,icpt", oc.NEIGHBOUR_ORDERS)
def test_gpu_neighbours_likelihood_and_gradient(ref_lib, p, d, q, icpt):
    clean, x = both_panels(p, d, q)
    S, T = x.shape
    n = ar.n_coef(p, q, icpt)
    coef = random_coef(5600 + p, S, p, q, icpt)
    c = dev(coef)
    out = []
    for panel in (clean, x):
        t, ll, g = dev(panel), torch_f64((S,)), torch_f64((S, n))
        assert _abi().sts_arima_css_loglik_gradient(t.data_ptr(), S, T, T, p, d, q, icpt, c.data_ptr(), ll.data_ptr(),
                                                    g.data_ptr(), None) == 0
        sync()
        out.append((host(ll), host(g)))
    assert same_bits(out[1][0][OK_ROWS], out[0][0][OK_ROWS]) and same_bits(out[1][1][OK_ROWS], out[0][1][OK_ROWS])
    with np.errstate(all="ignore"):
        evs = [ar.CEval(ref_lib, p, q, icpt, ar.diffed(x[s], d)) for s in range(S)]
        want = np.array([evs[s].loglik(coef[s]) for s in range(S)])
        assert same_bits(out[1][0], want)
        assert same_bits(out[1][1], np.array([evs[s].gradient(coef[s]) for s in range(S)]))
    # (the overflowing, infinite and NaN rows have no likelihood; the underflowing and constant ones may)
    assert np.isfinite(want[OK_ROWS]).all()
    none = [s for s, name in zip(LANE_SLOTS, POISONS) if "x2^5" in name or "x2^6" in name or "inf" in name or "NaN" in name]
    assert len(none) == 7 and np.isnan(want[none]).all()


@pytest.mark.parametrize("op", ["remove", "add", "forecast"])
@pytest.mark.parametrize("p,d,q,icpt", oc.NEIGHBOUR_ORDERS)
def test_gpu_neighbours_effects_and_forecast(p, d, q, icpt, op):
    clean, x = both_panels(p, d, q)
    S, T = x.shape
    TO = T + NF if op == "forecast" else T
    coef = random_coef(5700 + p, S, p, q, icpt) * 0.8
    c = dev(coef)
    out = []
    for panel in (clean, x):
        t, o = dev(panel), torch_f64((S, TO))
        if op == "forecast":
            st = _abi().sts_arima_forecast(t.data_ptr(), o.data_ptr(), S, T, T, TO, p, d, q, icpt, c.data_ptr(), NF, None)
        else:
            fn = _abi().sts_arima_remove if op == "remove" else _abi().sts_arima_add
            st = fn(t.data_ptr(), o.data_ptr(), S, T, T, TO, p, d, q, icpt, c.data_ptr(), None)
        assert st == 0
        sync()
        assert same_bits(host(t), panel)
        out.append(host(o))
    assert same_bits(out[1][OK_ROWS], out[0][OK_ROWS])
    f = {"remove": lambda s: ar.remove_effects(p, d, q, coef[s], icpt, x[s]),
         "add": lambda s: ar.add_effects(p, d, q, coef[s], icpt, x[s]),
         "forecast": lambda s: ar.forecast(p, d, q, coef[s], icpt, x[s], NF)}[op]
    with np.errstate(all="ignore"):
        want = np.array([f(s) for s in range(S)])
    assert same_bits(out[1], want)
    assert np.isfinite(want[OK_ROWS]).all()


@pytest.mark.parametrize("p,d,q,icpt", oc.NEIGHBOUR_ORDERS)
def test_gpu_neighbours_hr_start(p, d, q, icpt):
    """Clean rows: bit-identical to the clean panel's call and within the bar.  Poisoned rows:
    where the restatement fails (an exception of either regression, or a start that is not
    finite) the coefficients are NaN and the status is the AR stage's where that stage set one
    (the oracle's AR fit of the row says which), else 0 or STS_ERR_SINGULAR; where it does not
    fail the row meets the bar like a clean one."""
    clean, x = both_panels(p, d, q)
    g0, e0 = hr_call(clean, p, d, q, icpt)
    g1, e1 = hr_call(x, p, d, q, icpt)
    assert not e0.any() and not e1[OK_ROWS].any()
    assert same_bits(g1[OK_ROWS], g0[OK_ROWS])
    good = list(np.flatnonzero(OK_ROWS))
    failed = 0
    for s, name in zip(LANE_SLOTS, POISONS):
        y = ar.diffed(x[s], d)
        with np.errstate(all="ignore"):
            ar_status = int(sc.ar_ref(y[None, :], max(p, q) + 1, False)[2][0])
        if oc.hr_ref(p, q, icpt, y) is not None:
            assert e1[s] == 0, (name, e1[s])
            good.append(s)
            continue
        failed += 1
        assert np.isnan(g1[s]).all(), (name, g1[s])
        assert e1[s] in ((ar_status,) if ar_status else (0, SINGULAR)), (name, e1[s], ar_status)
    assert failed >= 6
    worst, worst_cond = hr_worst(g1, x, p, d, q, icpt, rows=good)
    print("p=%d d=%d q=%d icpt=%d next to poisons: worst relative error %.3g, worst condition number %.3g"
          % (p, d, q, icpt, worst, worst_cond))
    assert worst <= HR_BAR


def test_gpu_neighbours_fit_from_the_devices_own_start():
    """ARIMA.fitModelCSS with the Hannan-Rissanen start of the device on the poisoned panel: the
    clean rows' coefficients, initParams, evaluations and status are those of the clean panel's call."""
    from sparkts.models.ARIMA import ARIMA
    p, d, q = 1, 1, 1
    out = []
    for panel in both_panels(p, d, q):
        err = torch_i32(len(panel))
        m = ARIMA.fitModelCSS(p, d, q, dev(panel), errors=err)
        out.append((host(m.coefficients), host(m.initParams), host(m.evaluations), host(err)))
    for a, b in zip(*out):
        assert same_bits(a[OK_ROWS], b[OK_ROWS])
    assert (out[0][3] == 0).sum() >= 2 * OK_ROWS.sum() // 3
    assert np.isfinite(out[1][0][OK_ROWS & (out[1][3] == 0)]).all()
