"""include/sts_regress.h without a GPU: the numpy restatement of commons-math3's OLS with intercept
(tests/factor_ols_ref.py) against the 60-digit fixture and against the residuals the reference's
suite builds, and the guards tests/test_abi.py gives sts.h, for the fifth header:

* every function of sts_regress.h is exported by libsts_hip.so and bound in
  _native.REGRESS_SIGNATURES with the header's arity;
* every call-level error the header lists comes back with its status before any device action, from
  the device entry point and from its `_host` twin, outputs untouched; an empty call is STS_OK;
* the mirror raises the matching exception before any native call.

Bars of the restatement against the fixture.  The project's 1e-10 on every row, with two
exceptions that are the reference's own error, not this project's: (a) coefficients and standard
errors of the two collinear rows, bounded by the design's conditioning, 16 kappa 2^-53 = 1.8e-9 with
kappa = 1e6; (b) factors at level 1e6 and the near-exact fit at level 1e4.  A Householder QR of the
UNCENTRED design [1, F] has kappa about level / spread = 1e6 on the first, and on the second forms
residuals of size 1e-4 as differences of values of size 1e4 rounded at 1e4 * 2^-53 = 1e-12, i.e.
1e-8 of a residual per operation; over a few operations per element that is a few 1e-8.  These rows
are held to 1e-7 (measured: 2.1e-9 and 3.6e-8, residuals), which shows only that restatement and
fixture describe the same regression; the device is held to 1e-10 against the fixture there
(tests/test_factor_ols_gpu.py).
"""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bgbp_ref as br
import factor_ols_ref as fr
import test_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sts_regress.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "factor_ols_exact.json")
LOOSE_ROWS = ("factor_level_1e6", "near_exact_level_1e4")

lib = test_abi.lib


def golden():
    doc = json.load(open(GOLDEN))
    out = []
    for row in doc["rows"]:
        out.append({k: np.array([float.fromhex(v) for v in row["exact"][k]]) for k in ("beta", "beta_lo", "se", "stats")})
        out[-1]["name"], out[-1]["T"] = row["name"], row["T"]
        out[-1]["probe"] = [float.fromhex(row[k]) for k in ("y0", "ylast", "f_last")]
    assert doc["k"] == fr.HARD_K and [(r["name"], r["T"]) for r in out] == fr.HARD_ROWS
    return out


# ---------------- the restatement ----------------

@pytest.mark.parametrize("i", range(len(fr.HARD_ROWS)), ids=["%s-%d" % r for r in fr.HARD_ROWS])
def test_restatement_against_the_exact_fixture(i):
    g = golden()[i]
    y, F = fr.hard_row(i)
    assert [y[0], y[-1], F[-1, -1]] == g["probe"], "the row is not the fixture's"
    f = fr.ols(y, F)
    errs = {"beta": fr.rel(f.beta, g["beta"]), "se": fr.rel(f.se, g["se"]), "stats": fr.rel(f.stats, g["stats"]),
            "resid": fr.resid_err(f.resid, fr.exact_resid(y, F, g["beta"], g["beta_lo"]))}
    print(g["name"], g["T"], errs)
    loose = g["name"] in LOOSE_ROWS
    for key, e in errs.items():
        bar = 1e-7 if loose else fr.KAPPA_BAR if fr.collinear(i) and key in ("beta", "se") else fr.BAR
        assert e <= bar, (key, e, bar)


def test_fixture_is_what_the_generator_writes():
    pytest.importorskip("mpmath")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_factor_ols_golden.py"), "--check"])
    # the residuals the tests form from the fixture's 106-bit coefficients are the 60-digit ones, bit for bit
    for i in (1, 10):
        y, F = fr.hard_row(i)
        ex = fr.exact(y, F)
        assert np.array_equal(fr.exact_resid(y, F, ex.beta, ex.beta_lo), ex.resid)


def test_restatement_reproduces_the_suites_first_stage_residuals(monkeypatch):
    calls = []
    first_stage = br._first_stage_residuals

    def spy(y, X):
        calls.append((np.array(y), np.array(X), first_stage(y, X)))
        return calls[-1][2]

    monkeypatch.setattr(br, "_first_stage_residuals", spy)
    br.suite_bg()
    br.suite_bp()
    assert len(calls) == 4
    for y, X, res in calls:
        f = fr.ols(y, X)
        assert np.array_equal(f.resid.view(np.uint64), res.view(np.uint64))
        # and the quantities hang together: X'e = 0, R^2 = 1 - rss / tss
        assert abs(f.resid.sum()) < 1e-10 and abs(X[:, 0] @ f.resid) < 1e-10
        assert f.rss == br.ref._seq(res * res) and abs(f.r2 - br.r_squared(y, X)) == 0.0


def test_restatement_of_the_effects_pair():
    Y, F = fr.panel(11, 3, 9, 2, per_series=True)
    beta = np.array([[1.0, 2.0, -3.0], [0.5, 0.25, 4.0], [0.0, 1e-3, 1e3]])
    for s in range(3):
        for t in range(9):
            fit = (beta[s, 0] + beta[s, 1] * F[s, t, 0]) + beta[s, 2] * F[s, t, 1]
            assert fr.remove(Y, beta, F)[s, t] == Y[s, t] - fit and fr.add(Y, beta, F)[s, t] == Y[s, t] + fit
    assert np.array_equal(fr.remove(Y[0], beta[0], F[0]), fr.remove(Y, beta, F)[0])
    assert np.array_equal(fr.add(Y, beta[1], F[1]), fr.add(Y, np.tile(beta[1], (3, 1)), np.tile(F[1], (3, 1, 1))))


# ---------------- the header's guards ----------------

def declared(monkeypatch):
    monkeypatch.setattr(test_abi, "HEADER", HEADER)
    return test_abi.declared()


def test_library_exports_every_declared_symbol(lib, monkeypatch):
    d = declared(monkeypatch)
    assert sorted(d) == ["sts_factor_add", "sts_factor_add_host", "sts_factor_ols", "sts_factor_ols_host",
                         "sts_factor_remove", "sts_factor_remove_host"], sorted(d)
    out = subprocess.check_output(["nm", "-D", "--defined-only", test_abi.LIB]).decode()
    missing = set(d) - set(re.findall(r" T (sts_\w+)", out))
    assert not missing, missing


def test_bindings_match_header_arity(lib, monkeypatch):
    from sparkts import _native
    d = declared(monkeypatch)
    assert set(d) == set(_native.REGRESS_SIGNATURES), set(d) ^ set(_native.REGRESS_SIGNATURES)
    for table in (_native.SIGNATURES, _native.TRANSFORM_SIGNATURES, _native.SAMPLE_SIGNATURES, _native.INDEX_SIGNATURES):
        assert not set(d) & set(table)
    for name, n in d.items():
        assert len(_native.REGRESS_SIGNATURES[name][1]) == n, name
        assert getattr(lib, name).argtypes == _native.REGRESS_SIGNATURES[name][1], name
        assert getattr(lib, name).restype is ctypes.c_int
    assert d["sts_factor_ols"] == 16 and d["sts_factor_remove"] == d["sts_factor_add"] == 13
    text = open(HEADER).read()
    assert "#ifndef STS_REGRESS_H" in text and 'extern "C"' in text and '#include "sts.h"' in text
    assert "sts_factor" not in open(os.path.join(ROOT, "include", "sts.h")).read()


# ---------------- argument errors need no device ----------------

def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


S, T, K = 3, 12, 3
Y, F = fr.panel(3, S, T, K)
FT = np.ascontiguousarray(F.T)               # (k, T): the C ABI's factor rows
FS = np.ascontiguousarray(np.stack([F.T] * S))


def _outs():
    return np.full((S, K + 1), 7.0), np.full((S, K + 1), 7.0), np.full((S, 4), 7.0), np.full((S, T), 7.0)


# (what, overrides of the good call, status)
OLS_ERRORS = [
    ("k=0", dict(k=0), fr.BAD_ARG),
    ("k=9", dict(k=9), fr.BAD_ARG),
    ("ld<T", dict(ld=T - 1), fr.BAD_ARG),
    ("ld_f<T", dict(ld_f=T - 1), fr.BAD_ARG),
    ("fs-overlaps", dict(fs=(K - 1) * T + T - 1), fr.BAD_ARG),
    ("fs<0", dict(fs=-1), fr.BAD_ARG),
    ("ld_b<k+1", dict(ld_b=K), fr.BAD_ARG),
    ("ld_r<T", dict(ld_r=T - 1), fr.BAD_ARG),
    ("null-y", dict(y=None), fr.BAD_ARG),
    ("null-factors", dict(f=None), fr.BAD_ARG),
    ("null-beta", dict(beta=None), fr.BAD_ARG),
    ("T=k+1", dict(T=K + 1, ld=T, ld_f=T), fr.NOT_ENOUGH_DATA),
    ("T=k", dict(T=K, ld=T, ld_f=T), fr.NOT_ENOUGH_DATA),
]


@pytest.mark.parametrize("what,over,status", OLS_ERRORS, ids=[e[0] for e in OLS_ERRORS])
def test_ols_argument_errors_need_no_device(lib, what, over, status):
    beta, se, stats, resid = _outs()
    a = dict(y=Y, S=S, T=T, ld=T, f=FT, k=K, ld_f=T, fs=0, beta=beta, ld_b=K + 1, ld_r=T)
    a.update(over)
    r = lib.sts_factor_ols(_p(a["y"]), a["S"], a["T"], a["ld"], _p(a["f"]), a["k"], a["ld_f"], a["fs"], _p(a["beta"]),
                           a["ld_b"], _p(se), _p(stats), _p(resid), a["ld_r"], None, None)
    assert r == status, (r, lib.sts_last_error())
    assert lib.sts_last_error()
    if what not in ("ld_b<k+1", "ld_r<T"):      # the host form has neither argument
        r = lib.sts_factor_ols_host(_p(a["y"]), a["S"], a["T"], a["ld"], _p(a["f"]), a["k"], a["ld_f"], a["fs"],
                                    _p(a["beta"]), _p(se), _p(stats), _p(resid), None)
        assert r == status, (r, lib.sts_last_error())
    for o in (beta, se, stats, resid):
        assert (o == 7.0).all()


EFFECT_ERRORS = [
    ("k=0", dict(k=0), fr.BAD_ARG),
    ("k=9", dict(k=9), fr.BAD_ARG),
    ("ld_in<T", dict(ld_in=T - 1), fr.BAD_ARG),
    ("ld_out<T", dict(ld_out=T - 1), fr.BAD_ARG),
    ("ld_f<T", dict(ld_f=T - 1), fr.BAD_ARG),
    ("fs-overlaps", dict(fs=K * T - 1), fr.BAD_ARG),
    ("ld_b<k+1", dict(ld_b=K), fr.BAD_ARG),
    ("null-in", dict(x=None), fr.BAD_ARG),
    ("null-out", dict(out=None), fr.BAD_ARG),
    ("null-factors", dict(f=None), fr.BAD_ARG),
    ("null-beta", dict(beta=None), fr.BAD_ARG),
]


@pytest.mark.parametrize("name", ["sts_factor_remove", "sts_factor_add"])
@pytest.mark.parametrize("what,over,status", EFFECT_ERRORS, ids=[e[0] for e in EFFECT_ERRORS])
def test_effects_argument_errors_need_no_device(lib, name, what, over, status):
    out = np.full((S, T), 7.0)
    beta = np.ones((S, K + 1))
    a = dict(x=Y, out=out, ld_in=T, ld_out=T, f=FT, k=K, ld_f=T, fs=0, beta=beta, ld_b=K + 1)
    a.update(over)
    r = getattr(lib, name)(_p(a["x"]), _p(a["out"]), S, T, a["ld_in"], a["ld_out"], _p(a["f"]), a["k"], a["ld_f"],
                           a["fs"], _p(a["beta"]), a["ld_b"], None)
    assert r == status, (r, lib.sts_last_error())
    assert lib.sts_last_error()
    if what not in ("ld_out<T", "ld_b<k+1"):
        r = getattr(lib, name + "_host")(_p(a["x"]), _p(a["out"]), S, T, a["ld_in"], _p(a["f"]), a["k"], a["ld_f"],
                                         a["fs"], _p(a["beta"]))
        assert r == status, (r, lib.sts_last_error())
    assert (out == 7.0).all()


def test_layout_errors_and_empty_calls_need_no_device(lib):
    beta, se, stats, resid = _outs()
    x = Y.copy()
    # an in-place effects call with two leading dimensions; residuals on top of y
    assert lib.sts_factor_remove(_p(x), _p(x), S, T // 2, T, T - 1, _p(FT), K, T, 0, _p(beta), K + 1, None) == fr.BAD_ARG
    assert lib.sts_factor_ols(_p(x), S, T, T, _p(FT), K, T, 0, _p(beta), K + 1, None, None, _p(x), T, None,
                              None) == fr.BAD_ARG
    # per-series factors at the smallest stride that does not overlap pass validation only as far
    # as the device: nothing to check here without one.  Nothing to do: answered before any device action
    assert lib.sts_factor_ols(_p(Y), 0, T, T, _p(FT), K, T, 0, _p(beta), K + 1, _p(se), _p(stats), _p(resid), T, None,
                              None) == 0
    assert lib.sts_factor_ols(None, 0, T, T, None, K, T, 0, None, K + 1, None, None, None, T, None, None) == 0
    assert lib.sts_factor_ols_host(_p(Y), 0, T, T, _p(FT), K, T, 0, _p(beta), _p(se), _p(stats), _p(resid), None) == 0
    for fn in (lib.sts_factor_remove, lib.sts_factor_add):
        assert fn(_p(Y), _p(resid), 0, T, T, T, _p(FT), K, T, 0, _p(beta), K + 1, None) == 0
        assert fn(_p(Y), _p(resid), S, 0, T, T, _p(FT), K, T, 0, _p(beta), K + 1, None) == 0
    for fn in (lib.sts_factor_remove_host, lib.sts_factor_add_host):
        assert fn(_p(Y), _p(resid), 0, T, T, _p(FT), K, T, 0, _p(beta)) == 0
    assert np.array_equal(x, Y)
    for o in (beta, se, stats, resid):
        assert (o == 7.0).all()


def test_mirror_raises_the_matching_exception(lib):
    from sparkts import models, stats
    from sparkts.errors import IllegalArgumentException, MathIllegalArgumentException
    from sparkts.timeseriesrdd import TimeSeriesRDD
    assert stats.ols is stats.regression.ols and "ols" in stats.__all__ and "OLSResult" in stats.__all__
    assert issubclass(models.FactorRegressionModel, models.TimeSeriesModel)
    with pytest.raises(IllegalArgumentException, match="factors must be"):
        stats.ols(Y, F[:, 0])
    with pytest.raises(IllegalArgumentException, match="do not match"):
        stats.ols(Y, F[:-1])
    with pytest.raises(IllegalArgumentException, match="need a panel"):
        stats.ols(Y[0], np.stack([F] * S))
    with pytest.raises(IllegalArgumentException, match="at most 8"):
        stats.ols(Y, np.zeros((T, 9)))
    with pytest.raises(MathIllegalArgumentException, match="not enough data"):
        stats.ols(Y[:, :K + 1], F[:K + 1])
    with pytest.raises(IllegalArgumentException, match="do not match"):
        TimeSeriesRDD(None, None, Y).regress(F[:-1])
    m = models.FactorRegressionModel(np.ones(K), F)
    with pytest.raises(IllegalArgumentException, match="coefficients of shape"):
        m.removeTimeDependentEffects(Y)
    with pytest.raises(IllegalArgumentException, match="coefficients of shape"):
        models.FactorRegressionModel(np.ones((S + 1, K + 1)), F).addTimeDependentEffects(Y)
    with pytest.raises(IllegalArgumentException, match="do not match"):
        models.FactorRegressionModel(np.ones(K + 1), F[:-1]).addTimeDependentEffects(Y)
    good = models.FactorRegressionModel(np.ones(K + 1), F)
    import torch
    with pytest.raises(IllegalArgumentException, match="destTs must be of ts's kind"):
        good.removeTimeDependentEffects(Y, torch.zeros((S, T), dtype=torch.float64))
    with pytest.raises(IllegalArgumentException, match="destTs of shape"):
        good.removeTimeDependentEffects(Y, np.zeros((S, T + 1)))
    for bad in (np.zeros((S, 2 * T))[:, ::2], np.zeros((S, T), dtype=np.float32), [[0.0] * T] * S):
        with pytest.raises(IllegalArgumentException, match="contiguous float64 panel"):
            good.addTimeDependentEffects(Y, bad)
    # bgtest / bptest keep their own messages
    with pytest.raises(IllegalArgumentException, match="bptest: factors must be"):
        stats.bptest(Y, F[:, 0])
