"""CPU anchors of tests/test_arima_orders_gpu.py: all 49 ARIMA orders, and the facts the GPU file
leans on, checked where no GPU is needed.

The GPU file compares the HIP kernels of csrc/sts_arima.hip with tests/arima_ref.py through
three shortcuts, and each is pinned here for exactly the inputs it is used on:

* the C evaluation (tests/native/arima_ref_eval.cpp) drives the restated optimizer and checks
  the likelihood kernel: bit for bit the Python evaluation for every order, at differenced
  lengths around the LDS chunk and at the shortest one;
* the Hannan-Rissanen bar of include/sts.h (1e-10) holds on designs whose column-scaled
  condition number is at most 1e4: asserted for every series of every panel the GPU file sends
  to sts_arima_hr_init, none skipped; and the restated start is equivariant under a scaling by
  2^k to 1e-12, which is what lets the GPU file pin the start at 2^+-300;
* the restated fit's (status, evaluations) on the ten poison rows, and the share of series on
  which it converges, so that the GPU file compares with recorded facts.

This module also owns the inputs (ORDERS, the panels and their seeds); the GPU file imports them.
"""
import numpy as np
import pytest

import arima_ref as ar
import oracle
import test_scale_cpu as sc
from test_arima import arma_panel, ref_fit, ref_lib, same_bits, starts  # noqa: F401  (ref_lib: a fixture)
from test_isolation_gpu import LANE_SLOTS, POISONS, poison_rows

cache = sc.cache

# (p, q, include_intercept): the 49 orders sts_arima_* accept; d cycles through 0, 1, 2 over them
ORDERS = [(p, q, icpt) for icpt in (1, 0) for p in range(5) for q in range(5) if icpt + p + q >= 1]
assert len(ORDERS) == 49


def diff_order(p, q):
    return (p + q) % 3


def order_id(o):
    return "p%dq%d%s" % (o[0], o[1], "c" if o[2] else "n")


# ---------------- the inputs of the GPU file ----------------

HR_SHAPE = (16, 250)
HR_LEVELS = [0.0, 8.2]
HR_DIFFS = [0, 1]
HR_LANES = [(4, 0, 4, 1, 0.0), (2, 1, 1, 0, 8.2)]   # (p, d, q, icpt, level) at S = 130: two full waves and two lanes
HR_SCALED = [(2, 1, 2), (4, 0, 4)]           # (p, d, q), both intercept settings
HR_SCALES = [-300, 300]
HR_CAP = 1e4                                 # include/sts.h: the condition number the 1e-10 bar is stated for
NEIGHBOUR_ORDERS = [(1, 1, 1, 1), (2, 0, 2, 0)]   # (p, d, q, icpt)
NEIGHBOUR_SHAPE = (130, 120)
FIT_S = 12


@cache
def hr_panel(p, q, level, d):
    return sc.frozen(arma_panel(2400 + int(level) + 7 * p + q, HR_SHAPE[0], HR_SHAPE[1], p, q, level=level, d=d))


@cache
def hr_lane_panel(p, d, q, level):
    return sc.frozen(arma_panel(2700 + 7 * p + q, 130, HR_SHAPE[1], p, q, level=level, d=d))


@cache
def fit_panel(p, q, icpt):
    d = diff_order(p, q)
    return sc.frozen(arma_panel(3000 + 10 * p + q + icpt, FIT_S, 130 + d, p, q, level=1.5, d=d))


@cache
def neighbour_clean(p, d, q):
    S, T = NEIGHBOUR_SHAPE
    return sc.frozen(arma_panel(4000 + 10 * p + q, S, T, p, q, level=1.0, d=d))


@cache
def neighbour_poisoned(p, d, q):
    x = np.array(neighbour_clean(p, d, q))
    x[LANE_SLOTS] = poison_rows(NEIGHBOUR_SHAPE[1])
    return sc.frozen(x)


def hr_ref(p, q, icpt, y):
    """-> the restated start of one differenced series, or None where the restatement fails: the
    AR stage's or the OLS's Singular / not-enough-data error, or a start that is not finite"""
    try:
        with np.errstate(all="ignore"):
            b = ar.hannan_rissanen(p, q, y, icpt)
    except (ar.Singular, ValueError, oracle.OracleError):
        return None
    return b if np.isfinite(b).all() else None


def hr_conditions(p, q, icpt, x, d):
    return np.array([ar.scaled_condition(ar.hr_design(p, q, ar.diffed(row, d), icpt)[1]) for row in x])


# ---------------- 1. the C evaluation is the Python evaluation, every order ----------------

@pytest.mark.parametrize("order", ORDERS, ids=order_id)
def test_c_evaluation_is_the_python_evaluation_every_order(ref_lib, order):
    p, q, icpt = order
    rng = np.random.default_rng(500 + 25 * p + 5 * q + icpt)
    for N in (max(p, q) + 1, 63, 64, 65):
        y = arma_panel(600 + N + p + 5 * q, 1, N, p, q, level=1.0)[0]
        ev = ar.CEval(ref_lib, p, q, icpt, y)
        for _ in range(2):
            coef = rng.uniform(-0.5, 0.5, ar.n_coef(p, q, icpt))
            assert same_bits([ev.loglik(coef)], [ar.loglik_css_arma(p, q, coef, icpt, y)]), N
            assert same_bits(ev.gradient(coef), ar.gradient_css_arma(p, q, coef, icpt, y)), N


# ---------------- 2. the Hannan-Rissanen inputs stay under the condition cap ----------------

@pytest.mark.parametrize("order", ORDERS, ids=order_id)
def test_hr_inputs_stay_under_the_condition_cap(order):
    """Every series of every panel of test_gpu_hr_start_every_order, none skipped."""
    p, q, icpt = order
    worst = 0.0
    for level in HR_LEVELS:
        for d in HR_DIFFS:
            conds = hr_conditions(p, q, icpt, hr_panel(p, q, level, d), d)
            worst = max(worst, conds.max())
            assert (conds <= HR_CAP).all(), (level, d, int(conds.argmax()), conds.max())
    print("p=%d q=%d icpt=%d: condition numbers up to %.3g" % (p, q, icpt, worst))


@pytest.mark.parametrize("p,d,q,icpt,level", HR_LANES)
def test_hr_lane_inputs_stay_under_the_condition_cap(p, d, q, icpt, level):
    conds = hr_conditions(p, q, icpt, hr_lane_panel(p, d, q, level), d)
    print("p=%d d=%d q=%d icpt=%d S=130: condition numbers up to %.3g" % (p, d, q, icpt, conds.max()))
    assert (conds <= HR_CAP).all(), (int(conds.argmax()), conds.max())


@pytest.mark.parametrize("p,d,q,icpt", NEIGHBOUR_ORDERS)
def test_hr_neighbour_inputs_stay_under_the_condition_cap(p, d, q, icpt):
    conds = hr_conditions(p, q, icpt, neighbour_clean(p, d, q), d)
    print("p=%d d=%d q=%d icpt=%d S=130 T=120: condition numbers up to %.3g" % (p, d, q, icpt, conds.max()))
    assert (conds <= HR_CAP).all(), (int(conds.argmax()), conds.max())


@pytest.mark.parametrize("icpt", [1, 0])
@pytest.mark.parametrize("p,d,q", HR_SCALED)
def test_restated_hr_start_is_equivariant_under_power_of_two_scaling(p, d, q, icpt):
    """The restatement on a panel scaled by 2^k against the restatement on the unscaled panel with
    its intercept multiplied by 2^k: within 1e-12 of the series' largest coefficient, with the
    scaled intercept brought back by 2^-k (exact), at k = +-300.  This is the reference that sets
    the range of test_gpu_hr_start_scaled; |k| did not have to be lowered."""
    worst = 0.0
    for level in HR_LEVELS:
        x = hr_panel(p, q, level, d)
        for k in HR_SCALES:
            for row in x:
                want = ar.hannan_rissanen(p, q, ar.diffed(row, d), icpt)
                got = ar.hannan_rissanen(p, q, ar.diffed(sc.scaled(row, k), d), icpt)
                if icpt:
                    got[0] = np.ldexp(got[0], -k)
                worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print("p=%d d=%d q=%d icpt=%d: restatement scaled vs unscaled, worst %.3g" % (p, d, q, icpt, worst))
    assert worst <= 1e-12


# ---------------- 3. what the restated fit does on the poisons ----------------

TME = ar.TOO_MANY_EVALUATIONS
# (p, d, q, icpt) -> the restated (status, evaluations) per row of POISONS at T = 120, from the
# restated start (test_arima.start_for: a constant 0.1 where Hannan-Rissanen does not exist)
# (recorded from the restatement: every row, the constant one included, runs out of evaluations)
POISON_FITS = {
    (1, 1, 1, 1): [(TME, 10001)] * len(POISONS),
    (2, 0, 2, 0): [(TME, 10001)] * len(POISONS),
}


@pytest.mark.parametrize("p,d,q,icpt", NEIGHBOUR_ORDERS)
def test_restated_fit_on_the_poisons(ref_lib, p, d, q, icpt):
    rows = poison_rows(NEIGHBOUR_SHAPE[1])
    with np.errstate(all="ignore"):
        init = starts(p, d, q, rows, icpt=bool(icpt))
        got = [ref_fit(ref_lib, p, d, q, icpt, rows[i], init[i]) for i in range(len(rows))]
    facts = [(st, ev) for st, _, ev in got]
    for name, fact in zip(POISONS, facts):
        print("ARIMA(%d,%d,%d) icpt=%d %-16s status %d evaluations %d" % (p, d, q, icpt, name, fact[0], fact[1]))
    assert facts == POISON_FITS[(p, d, q, icpt)]
    # the six out-of-range rows run out of evaluations
    assert all(f == (TME, 10001) for f in facts[:len(sc.OUT_OF_RANGE)])


# ---------------- 4. the fit panels converge for most series ----------------

@cache
def fit_reference(ref_lib, order):
    """-> [(status, coefficients, evaluations)] of the restated fit from the restated start"""
    p, q, icpt = order
    d = diff_order(p, q)
    x = fit_panel(p, q, icpt)
    init = starts(p, d, q, x, icpt=bool(icpt))
    return [ref_fit(ref_lib, p, d, q, icpt, x[s], init[s]) for s in range(len(x))]


@pytest.mark.parametrize("order", ORDERS, ids=order_id)
def test_fit_panels_converge_for_most_series(ref_lib, order):
    """The reference alone: at least 8 of the 12 series of every part-2 fit panel end OK (the rest
    at TooManyEvaluations; the GPU file still compares their status and evaluation count)."""
    statuses = [st for st, _, _ in fit_reference(ref_lib, order)]
    print("p=%d q=%d icpt=%d: statuses %s" % (order + (statuses,)))
    assert set(statuses) <= {ar.OK, TME}
    assert statuses.count(ar.OK) >= 8
