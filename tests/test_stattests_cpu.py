"""CPU checks of the statistical tests' checker and boundary (no GPU): the restatement in
tests/stattests_ref.py against the reference's own known answers, its p-value functions against
scipy, its float64 rounding against 60-digit mpmath on the rows the GPU tests use, the committed
fixtures, and the C ABI of the eight new entry points.
"""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import stattests_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ["sts_adf_test", "sts_kpss_test", "sts_dw_test", "sts_lb_test",
               "sts_adf_test_host", "sts_kpss_test_host", "sts_dw_test_host", "sts_lb_test_host"]


def kats():
    with open(os.path.join(GOLDEN, "stattests_kats.json")) as f:
        return json.load(f)


def test_kpss_known_answers():
    # TimeSeriesStatisticalTestsSuite.scala:131-142
    k = kats()["kpss_r_equivalence"]
    x = np.array(k["series"])
    assert ref.kpss_lag(x.size) == k["lag"]
    assert abs(ref.kpss_stat(x, "c") - k["c"]) <= k["tolerance"]
    assert abs(ref.kpss_stat(x, "ct") - k["ct"]) <= k["tolerance"]


def test_ljung_box_suite_replay():
    # TimeSeriesStatisticalTestsSuite.scala:87-101 with commons-math3's MersenneTwister(5)
    import mt19937
    k = kats()["ljung_box"]
    rand = mt19937.MersenneTwister(k["mersenne_twister_seed"])
    indep = np.array([rand.next_gaussian() for _ in range(k["n"])])
    stat1 = ref.lb_stat(indep, k["independent_max_lag"])
    assert ref.chi2_sf(stat1, k["independent_max_lag"]) > k["p_threshold"]
    dep = np.empty(k["n"])
    prior = 0.0
    for i, cur in enumerate(indep):
        prior = prior * k["coef"] + cur
        dep[i] = prior
    stat2 = ref.lb_stat(dep, k["dependent_max_lag"])
    assert ref.chi2_sf(stat2, k["dependent_max_lag"]) < k["p_threshold"]


def test_durbin_watson_of_noise_and_of_its_running_sum():
    e = np.random.RandomState(11).standard_normal(500)
    assert 1.5 < ref.dw_stat(e) < 2.5
    assert ref.dw_stat(np.cumsum(e)) < 0.5


def test_chi2_tail_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    for dof in (1, 2, 5, 20, 60, 70, 200):
        for x in (1e-3, 0.5, 1.0, dof - 0.5, dof + 0.5, dof * 1.0, 2.0 * dof, 5.0 * dof + 30):
            assert abs(ref.chi2_sf(x, dof) - stats.chi2.sf(x, dof)) <= 1e-12, (dof, x)


def test_normal_cdf_and_mackinnon_against_scipy():
    special = pytest.importorskip("scipy.special")
    for z in np.linspace(-9, 9, 73):
        assert abs(ref.norm_cdf(float(z)) - special.ndtr(z)) <= 1e-12
    for reg in ref.REGRESSIONS:
        star, lo, hi, small, large = ref.MACKINNON[reg]
        assert ref.mackinnon_p(lo - 1e-9, reg) == 0.0
        if math.isfinite(hi):
            assert ref.mackinnon_p(hi + 1e-9, reg) == 1.0
        # both polynomial branches, evaluated as the paper writes them: c0 + c1 tau + c2 tau^2 (+ c3 tau^3)
        tau = star - 0.75
        assert abs(ref.mackinnon_p(tau, reg) - special.ndtr(small[0] + small[1] * tau + small[2] * tau ** 2)) <= 1e-12
        tau = star + 0.5
        z = large[0] + large[1] * tau + large[2] * tau ** 2 + large[3] * tau ** 3
        assert abs(ref.mackinnon_p(tau, reg) - special.ndtr(z)) <= 1e-12
        # a p-value rises with tau inside each branch
        grid = np.linspace(max(lo, -12.0), star, 40)
        p = [ref.mackinnon_p(float(t), reg) for t in grid]
        assert all(b >= a for a, b in zip(p, p[1:]))


# the well-posed ordinary rows of tests/test_stattests_gpu.py, a few series each
ORDINARY_EXACT = [(T, kind, lag, reg) for T in (20, 64, 390)
                  for (kind, lag, reg) in (("adf", 0, "nc"), ("adf", 1, "c"), ("adf", 5, "ct"), ("adf", 1, "ctt"),
                                           ("kpss", 0, "c"), ("kpss", 0, "ct"))]


@pytest.mark.parametrize("T,kind,lag,reg", ORDINARY_EXACT)
def test_restatement_rounding_on_ordinary_rows(T, kind, lag, reg):
    """The 1e-10 bar of the GPU tests is not spent on the checker's own rounding: on ordinary rows
    the float64 restatement is within 1e-12 relative of exact arithmetic."""
    pytest.importorskip("mpmath")
    x = ref.ordinary_panel(100 + T, 3, T)
    for s in range(3):
        r64 = ref.ref_stat(kind, lag, reg, x[s])
        ex = ref.exact_stat(kind, lag, reg, x[s])
        print(T, kind, lag, reg, s, abs(r64 - ex) / abs(ex))
        assert abs(r64 - ex) <= 1e-12 * abs(ex)


def test_exact_fixture_regenerates():
    """tests/golden/stattests_exact.json: the rows regenerate from their seeds, and (a sample of
    the rows; tools/gen_stattests_golden.py --check does all of them) the 60-digit values too."""
    pytest.importorskip("mpmath")
    with open(os.path.join(GOLDEN, "stattests_exact.json")) as f:
        doc = json.load(f)
    assert len(doc["rows"]) == len(ref.HARD_ROWS)
    assert doc["stats"] == ["%s_%d_%s" % st for st in ref.HARD_STATS]
    for i, row in enumerate(doc["rows"]):
        x = ref.hard_row(i)
        assert (row["level"], row["drift"], row["noise"], row["kind"], row["T"]) == ref.HARD_ROWS[i]
        assert float(x[0]).hex() == row["x0"] and float(x[-1]).hex() == row["xlast"]
    for i in (0, 7, 22):
        x = ref.hard_row(i)
        for st in ref.HARD_STATS:
            assert float(ref.exact_stat(st[0], st[1], st[2], x)).hex() == doc["rows"][i]["exact"]["%s_%d_%s" % st]


def test_new_entry_points_cross_the_abi():
    """The four device and four `_host` entry points are declared in sts.h, exported by the
    library and bound by the ctypes mirror."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sts.h")).read(), flags=re.S)
    declared = set(re.findall(r"\bint\s+(sts_\w+)\s*\(", text))
    from sparkts import _native
    lib = os.path.join(ROOT, "spark-timeseries_amd", "build", "libsts_hip.so")
    exported = set(re.findall(r" T (sts_\w+)", subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()))
    for name in NEW_SYMBOLS + ["sts_regression_from_name"]:
        assert name in declared, name
        assert name in exported, name
        assert name in _native.SIGNATURES, name
    handle = _native.load_library()
    assert [handle.sts_regression_from_name(n) for n in (b"nc", b"c", b"ct", b"ctt", b"t")] == [0, 1, 2, 3, -2]


def test_argument_errors_need_no_device():
    from sparkts.errors import IllegalArgumentException
    from sparkts.stats import TimeSeriesStatisticalTests as tst
    with pytest.raises(IllegalArgumentException, match="requirement failed: trend must be c or ct"):
        tst.kpsstest(np.arange(10.0), "ctt")
    with pytest.raises(IllegalArgumentException, match="is not c, ct, or ctt"):
        tst.adftest(np.arange(30.0), 1, "t")
    assert not hasattr(tst, "bgtest") and not hasattr(tst, "bptest")
