"""include/sts_transforms.h without a GPU: the numpy restatement (tests/transforms_ref.py) against
the reference suite's known answers and properties, and the guards tests/test_abi.py and
tests/test_stream_table.py give sts.h, for the sibling header:

* every function of sts_transforms.h is exported by libsts_hip.so and bound in
  _native.TRANSFORM_SIGNATURES with the header's arity (parsed as test_abi.declared does);
* every one that ends in `void* stream` has a row in tests/test_transforms_stream_gpu.py, no stale rows;
* every argument error the header lists comes back with its status before any device action, from
  the device entry point and from its `_host` twin, and the mirror raises the matching exception.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import test_abi
import transforms_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sts_transforms.h")
KATS = os.path.join(ROOT, "tests", "golden", "transforms_kats.json")
BAD_ARG, UNSUPPORTED, REQUIREMENT = 1, 3, 5


def declared(monkeypatch):
    """test_abi.declared's parse, pointed at the sibling header"""
    monkeypatch.setattr(test_abi, "HEADER", HEADER)
    return test_abi.declared()


def stream_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(m.group(2) for m in re.finditer(r"\b(int|const char\*)\s+(sts_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
                  if re.search(r"void\s*\*\s*stream\s*$", m.group(3).strip()))


lib = test_abi.lib


def nan_list(v):
    return np.array([np.nan if e is None else e for e in v], dtype=np.float64)


# ---------------- the restatement ----------------

def test_restatement_reproduces_the_known_answers():
    k = json.load(open(KATS))
    assert len(k["upsample"]) == 2 and len(k["downsample"]) == 2 and len(k["lastNotNaN"]) == 3
    for c in k["upsample"]:
        got = tr.upsample(nan_list(c["values"]), c["n"], c["phase"], c["use_zero"])[0]
        assert np.array_equal(got.view(np.uint64), nan_list(c["expected"]).view(np.uint64)), c
    for c in k["downsample"]:
        got = tr.downsample(nan_list(c["values"]), c["n"], c["phase"])[0]
        assert np.array_equal(got, nan_list(c["expected"])), c
    for c in k["lastNotNaN"]:
        assert int(tr.last_not_nan(nan_list(c["values"]))[0]) == c["expected"], c


def test_restatement_has_the_suites_properties():
    x = np.random.default_rng(10).standard_normal((3, 100))
    # "differencing at lag": lag 5 inverts within 1e-6, and diffed(10) is sampled(10) - sampled(5)
    diffed = tr.differences_at_lag(x, 5)
    assert np.abs(tr.inverse_differences_at_lag(diffed, 5) - x).max() <= 1e-6
    assert np.array_equal(diffed[:, 10], x[:, 10] - x[:, 5]) and np.array_equal(diffed[:, 99], x[:, 99] - x[:, 94])
    # "differencing of order d"
    assert np.abs(tr.differences_of_order_d(x, 1) - tr.differences_at_lag(x, 1)).max() <= 1e-6
    d5 = tr.differences_of_order_d(x, 5)
    assert np.abs(tr.inverse_differences_of_order_d(d5, 5) - x).max() <= 1e-6
    d6, one_more = tr.differences_of_order_d(x, 6), tr.differences_of_order_d(d5, 1)
    assert np.abs(d6[:, 6:] - one_more[:, 6:]).max() <= 1e-6
    # TimeSeriesRDD.differences(n) is Breeze's recursive diff: the order-n differences from position n on
    for n in (0, 1, 2, 5):
        assert np.array_equal(tr.breeze_diff(x, n), tr.differences_of_order_d(x, n)[:, n:])


def test_restatement_edges():
    nan = np.nan
    x = np.array([[nan, nan, 2.0, nan, 0.0, -0.0, nan]])
    assert tr.first_not_nan(x)[0] == 2 and tr.last_not_nan(x)[0] == 5
    assert tr.first_not_nan(np.full((1, 4), nan))[0] == 4 and tr.last_not_nan(np.full((1, 4), nan))[0] == -1
    assert np.array_equal(tr.trim_leading(x[0])[:1], [2.0]) and tr.trim_leading(np.full(3, nan)).size == 0
    assert tr.trim_trailing(x[0]).size == 5            # 0 until lastNotNaN: the last valid value goes too
    assert tr.trim_trailing(np.array([1.0, nan])).size == 0
    assert np.array_equal(tr.fill_previous(x)[0, 2:], [2.0, 2.0, 0.0, -0.0, -0.0])
    q = tr.quotients(np.array([[1.0, 0.0, -0.0, 4.0]]), 1)
    assert q[0, 0] == 0.0 and np.isnan(q[0, 1]) and np.isneginf(q[0, 2])
    assert tr.downsample(x, 3, 7).shape == (1, 0) and tr.downsample(x, 3, 8).shape == (1, 0)
    with pytest.raises(IndexError):
        tr.upsample(x, 2, 2)


# ---------------- the header's guards ----------------

def test_library_exports_every_declared_symbol(lib, monkeypatch):
    d = declared(monkeypatch)
    assert len(d) == 18 and "sts_fill_quotients" in d and "sts_first_last_not_nan_host" in d, sorted(d)
    out = subprocess.check_output(["nm", "-D", "--defined-only", test_abi.LIB]).decode()
    missing = set(d) - set(re.findall(r" T (sts_\w+)", out))
    assert not missing, missing


def test_bindings_match_header_arity(lib, monkeypatch):
    from sparkts import _native
    d = declared(monkeypatch)
    assert set(d) == set(_native.TRANSFORM_SIGNATURES), set(d) ^ set(_native.TRANSFORM_SIGNATURES)
    assert not set(d) & set(_native.SIGNATURES)
    for name, n in d.items():
        assert len(_native.TRANSFORM_SIGNATURES[name][1]) == n, name
        assert getattr(lib, name).argtypes == _native.TRANSFORM_SIGNATURES[name][1], name
    if os.path.exists(_native.AB_LIB_PATH):
        assert _native.load_variant(_native.AB_LIB_PATH).sts_quotients.argtypes is not None


def test_every_stream_entry_point_has_a_row():
    import test_transforms_stream_gpu as ts
    names = stream_entry_points()
    assert len(names) == 9 and not [n for n in names if n.endswith("_host")], names
    covered = {n for t in ts.TABLE for n in t[1]}
    assert not sorted(set(names) - covered), "no row in test_transforms_stream_gpu.TABLE for %s" % sorted(set(names) - covered)
    assert not sorted(covered - set(names)), "stale rows: %s" % sorted(covered - set(names))
    assert len(set(ts.IDS)) == len(ts.IDS)
    # every entry point is held to "returns while the gate is shut"; the one row that may wait says why
    assert set(ts.ASYNC) == set(names)
    assert set(ts.SYNC) == {"fill_quotients-null-err"}, sorted(ts.SYNC)
    assert "ErrSink::finish()" in ts.SYNC["fill_quotients-null-err"]


# ---------------- argument errors need no device ----------------

def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


S, T = 3, 10
X = np.arange(S * T, dtype=np.float64).reshape(S, T) + 1.0
O = np.zeros((S, 4 * T))

# (name, extra arguments after the panels, expected status); the device form takes (in, out, S, T, ld_in,
# ld_out, *extra, stream), the host form (in, out, S, T, ld, *extra)
ERRORS = [
    ("sts_quotients", (-1, 0), BAD_ARG),
    ("sts_quotients", (T + 1, 1), BAD_ARG),
    ("sts_fill_quotients", (3, -1, 1, None), BAD_ARG),
    ("sts_fill_quotients", (3, T + 1, 1, None), BAD_ARG),
    ("sts_fill_quotients", (7, 1, 1, None), UNSUPPORTED),
    ("sts_downsample", (0, 0), BAD_ARG),
    ("sts_downsample", (2, -1), BAD_ARG),
    ("sts_upsample", (0, 0, 0), BAD_ARG),
    ("sts_upsample", (3, 3, 0), BAD_ARG),
    ("sts_upsample", (3, -1, 1), BAD_ARG),
    ("sts_inverse_diff_at_lag", (3, 2), REQUIREMENT),
    ("sts_inverse_diff_at_lag", (-1, 2), BAD_ARG),
    ("sts_diff_order_d", (-1,), BAD_ARG),
    ("sts_inverse_diff_order_d", (-1,), BAD_ARG),
]


@pytest.mark.parametrize("name,extra,status", ERRORS, ids=["%s%s" % (e[0][4:], list(e[1])) for e in ERRORS])
def test_argument_errors_need_no_device(lib, name, extra, status):
    before = O.copy()
    assert getattr(lib, name)(_p(X), _p(O), S, T, T, 4 * T, *extra, None) == status, lib.sts_last_error()
    assert lib.sts_last_error()
    assert getattr(lib, name + "_host")(_p(X), _p(O), S, T, T, *extra) == status, lib.sts_last_error()
    assert np.array_equal(O, before)


def test_layout_errors_and_empty_calls_need_no_device(lib):
    f = np.zeros(S, dtype=np.int64)
    assert lib.sts_quotients(_p(X), _p(O), S, T, T, T - 4, 3, 0, None) == BAD_ARG        # ld_out < T - lag
    assert lib.sts_quotients(_p(X), _p(X), S, T, T, T, 0, 0, None) == BAD_ARG            # out aliases in
    assert lib.sts_first_last_not_nan(_p(X), S, T, T - 1, _p(f), None, None) == BAD_ARG  # ld < T
    assert lib.sts_diff_order_d(_p(X), _p(X), S, T, T, T, 1, None) == BAD_ARG
    # nothing to write: answered before any device action
    assert lib.sts_quotients(_p(X), _p(O), S, T, T, 0, T, 1, None) == 0                  # lag == T
    assert lib.sts_quotients_host(_p(X), _p(O), S, T, T, T, 1) == 0
    assert lib.sts_downsample(_p(X), _p(O), S, T, T, 0, 3, T, None) == 0                 # phase >= T: newLen 0
    assert lib.sts_downsample_host(_p(X), _p(O), S, T, T, 3, T + 1) == 0
    assert lib.sts_inverse_diff_at_lag(_p(X), _p(O), S, T, T, T, 0, 0, None) == 0        # lag 0: dest untouched
    assert lib.sts_inverse_diff_at_lag_host(_p(X), _p(O), S, T, T, 0, 2) == 0
    assert lib.sts_first_last_not_nan(_p(X), S, T, T, None, None, None) == 0
    assert not O.any()


def test_mirror_raises_the_matching_exception(lib):
    from sparkts import UnivariateTimeSeries as uts
    from sparkts import pipelines
    from sparkts.errors import IllegalArgumentException, UnsupportedOperationException
    from sparkts.timeseriesrdd import TimeSeriesRDD
    for name in ("quotients", "price2ret", "fillWithDefault", "downsample", "upsample", "firstNotNaN", "lastNotNaN",
                 "trimLeading", "trimTrailing", "inverseDifferencesAtLag", "differencesOfOrderD",
                 "inverseDifferencesOfOrderD"):
        assert name in uts.__all__ and callable(getattr(uts, name)), name
    x = X[0]
    with pytest.raises(IllegalArgumentException, match="lag"):
        uts.quotients(x, T + 1)
    with pytest.raises(IllegalArgumentException, match="lag"):
        uts.price2ret(X, -1)
    with pytest.raises(IllegalArgumentException, match="at least 1"):
        uts.downsample(x, 0)
    with pytest.raises(IllegalArgumentException, match="phase"):
        uts.downsample(x, 2, -1)
    with pytest.raises(IllegalArgumentException, match="phase"):
        uts.upsample(x, 3, 3)
    with pytest.raises(IllegalArgumentException, match="starting index cannot be less than lag"):
        uts.inverseDifferencesAtLag(x, 3, startIndex=1)
    with pytest.raises(IllegalArgumentException, match="order"):
        uts.differencesOfOrderD(X, -1)
    with pytest.raises(IllegalArgumentException, match="order"):
        uts.inverseDifferencesOfOrderD(x, -2)
    with pytest.raises(UnsupportedOperationException):
        pipelines.fill_returns("cubic")
    with pytest.raises(IllegalArgumentException, match="lag"):
        pipelines.fill_returns("previous", T + 1)(X)
    rdd = TimeSeriesRDD(list(range(T)), ["a", "b", "c"], X)
    with pytest.raises(IllegalArgumentException):
        rdd.differences(T + 1)
    with pytest.raises(IllegalArgumentException, match="lag"):
        rdd.quotients(T + 1)
    assert np.array_equal(rdd.findSeries("b"), X[1])
    with pytest.raises(KeyError):
        rdd.findSeries("z")
    # nothing to compute: no device needed, the reference's empty results
    assert uts.quotients(x, T).shape == (0,) and uts.downsample(X, 3, T).shape == (S, 0)
