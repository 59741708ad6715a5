"""include/sts_cross.h without a GPU: the guards tests/test_abi.py gives sts.h, for the sixth header,
and the numpy restatement of its definition (tests/cross_ref.py) against exact arithmetic.

* every function of sts_cross.h is exported by libsts_hip.so and bound in _native.CROSS_SIGNATURES
  with the header's arity and argument types;
* sts_cross_kind_from_name maps "cov" and "corr" and rejects anything else;
* every call-level error the header lists comes back with its status before any device action, from
  the device entry point and from its `_host` twin, a sentinel-filled out untouched;
* the mirror raises before any native call;
* the restatement against the 60-digit fixture and against np.cov / np.corrcoef on ordinary data, and
  within the numeric bar on the hard families at T = 2520 -- where MLlib's one-pass formula, restated
  beside it, is off by orders of magnitude on the series far from their own level.

Bar: |got - exact| <= 1e-10 sqrt(C_ii C_jj) / (T - 1) for COV (Cauchy-Schwarz on the rounding of a
centred sum) and 1e-10 absolute for CORR.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cross_ref as cr
import test_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sts_cross.h")
BAD_ARG, NOT_ENOUGH_DATA = 1, 7
SENTINEL = -3.0e55

lib = test_abi.lib


def declared(monkeypatch):
    monkeypatch.setattr(test_abi, "HEADER", HEADER)
    return test_abi.declared()


# ---------------- the header and its bindings ----------------

def test_library_exports_every_declared_symbol(lib, monkeypatch):
    d = declared(monkeypatch)
    assert sorted(d) == ["sts_cross_kind_from_name", "sts_cross_moments", "sts_cross_moments_host"], sorted(d)
    out = subprocess.check_output(["nm", "-D", "--defined-only", test_abi.LIB]).decode()
    missing = set(d) - set(re.findall(r" T (sts_\w+)", out))
    assert not missing, missing


def test_bindings_match_header_arity_and_types(lib, monkeypatch):
    from sparkts import _native
    d = declared(monkeypatch)
    assert set(d) == set(_native.CROSS_SIGNATURES), set(d) ^ set(_native.CROSS_SIGNATURES)
    for table in (_native.SIGNATURES, _native.TRANSFORM_SIGNATURES, _native.SAMPLE_SIGNATURES, _native.INDEX_SIGNATURES,
                  _native.REGRESS_SIGNATURES):
        assert not set(d) & set(table)
    for name, n in d.items():
        assert len(_native.CROSS_SIGNATURES[name][1]) == n, name
        assert getattr(lib, name).argtypes == _native.CROSS_SIGNATURES[name][1], name
        assert getattr(lib, name).restype is ctypes.c_int
    assert d["sts_cross_moments"] == 13 and d["sts_cross_moments_host"] == 11 and d["sts_cross_kind_from_name"] == 1
    # the argument types, from the header's own text: pointers void*, int64_t c_int64, int c_int
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("sts_cross_moments", "sts_cross_moments_host"):
        args = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1).split(",")
        want = [ctypes.c_void_p if "*" in a else ctypes.c_int64 if "int64_t" in a else ctypes.c_int for a in args]
        assert _native.CROSS_SIGNATURES[name][1] == want, name
    assert "#ifndef STS_CROSS_H" in text and 'extern "C"' in text and '#include "sts.h"' in text
    assert "sts_cross" not in open(os.path.join(ROOT, "include", "sts.h")).read()
    m = re.search(r"typedef enum \{ STS_CROSS_COV = (\d), STS_CROSS_CORR = (\d) \} sts_cross_kind;", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (_native.CROSS_COV, _native.CROSS_CORR) == (0, 1)


def test_kind_names(lib):
    assert lib.sts_cross_kind_from_name(b"cov") == 0 and lib.sts_cross_kind_from_name(b"corr") == 1
    for bad in (b"", b"COV", b"covariance", b"pearson", b"corr ", None):
        assert lib.sts_cross_kind_from_name(bad) == -2, bad


# ---------------- argument errors need no device ----------------

def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class Args:
    """a valid call on host memory (never dereferenced: every guard comes before any device action)"""

    def __init__(self, with_y, entry="device"):
        self.entry = entry
        self.Sx, self.T, self.ld_x, self.Sy, self.ld_y, self.kind = 3, 9, 11, (2 if with_y else 0), (10 if with_y else 0), 0
        self.x = np.arange(3 * 11, dtype=np.float64)
        self.y = np.arange(2 * 10, dtype=np.float64) if with_y else None
        self.cols = 2 if with_y else 3
        self.ld_o = self.cols + 1 if entry == "device" else self.cols      # the host twin's out is packed
        self.out = np.full(3 * self.ld_o, SENTINEL)
        self.mean_x = np.full(3, SENTINEL)
        self.mean_y = np.full(2, SENTINEL) if with_y else None
        self.px, self.py, self.pout, self.pmx, self.pmy = _p(self.x), _p(self.y), _p(self.out), _p(self.mean_x), _p(self.mean_y)

    def device(self, lib):
        return lib.sts_cross_moments(self.px, self.Sx, self.T, self.ld_x, self.py, self.Sy, self.ld_y, self.kind, self.pout,
                                     self.ld_o, self.pmx, self.pmy, None)

    def host(self, lib):
        return lib.sts_cross_moments_host(self.px, self.Sx, self.T, self.ld_x, self.py, self.Sy, self.ld_y, self.kind,
                                          self.pout, self.pmx, self.pmy)

    def untouched(self):
        return all((a == SENTINEL).all() for a in (self.out, self.mean_x, self.mean_y) if a is not None)


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _overlap_x(a):
    a.pout = ctypes.c_void_p(a.x.ctypes.data + 8 * ((a.Sx - 1) * a.ld_x + a.T - 1))      # element (Sx - 1, T - 1) of x


def _overlap_y(a):
    a.pout = ctypes.c_void_p(a.y.ctypes.data - 8 * ((a.Sx - 1) * a.ld_o + a.cols - 1))  # out's last element is y's first


# (id, needs y, mutation, status, applies to the packed-out host twin)
GUARDS = [
    ("null_x", False, _set(px=None), BAD_ARG, True),
    ("null_out", False, _set(pout=None), BAD_ARG, True),
    ("Sx_0", False, _set(Sx=0), BAD_ARG, True),
    ("Sx_negative", True, _set(Sx=-1), BAD_ARG, True),
    ("Sy_0_with_y", True, _set(Sy=0), BAD_ARG, True),
    ("ld_x_below_T", False, _set(ld_x=8), BAD_ARG, True),
    ("ld_y_below_T", True, _set(ld_y=8), BAD_ARG, True),
    ("ld_o_below_Sy", True, _set(ld_o=1), BAD_ARG, False),
    ("ld_o_below_Sx_symmetric", False, _set(ld_o=2), BAD_ARG, False),
    ("kind_2", False, _set(kind=2), BAD_ARG, True),
    ("kind_negative", True, _set(kind=-1), BAD_ARG, True),
    ("mean_y_without_y", False, _set(pmy=ctypes.c_void_p(8)), BAD_ARG, True),
    ("out_overlaps_x", False, _overlap_x, BAD_ARG, True),
    ("out_is_x", True, lambda a: setattr(a, "pout", a.px), BAD_ARG, True),
    ("out_overlaps_y", True, _overlap_y, BAD_ARG, True),
    ("T_1", False, _set(T=1), NOT_ENOUGH_DATA, True),
    ("T_0", True, _set(T=0), NOT_ENOUGH_DATA, True),
    ("T_negative", False, _set(T=-3), BAD_ARG, True),
]


GUARD_CALLS = [(g, e) for g in GUARDS for e in ("device", "host") if e == "device" or g[4]]


@pytest.mark.parametrize("case,entry", GUARD_CALLS, ids=["%s-%s" % (g[0], e) for g, e in GUARD_CALLS])
def test_call_level_errors_leave_the_outputs_untouched(lib, case, entry):
    name, with_y, mutate, status, _ = case
    a = Args(with_y, entry)
    mutate(a)
    assert getattr(a, entry)(lib) == status, (name, lib.sts_last_error())
    assert b"cross_moments" in lib.sts_last_error()
    assert a.untouched()


def test_ignored_arguments_of_the_symmetric_form_are_ignored(lib):
    """y == NULL: Sy and ld_y are ignored, so nonsense there does not turn a bad call good or a
    guard off -- the call still gets as far as its next guard (T < 2 here), not BAD_ARG"""
    a = Args(False)
    a.Sy, a.ld_y, a.T = -5, -7, 1
    assert a.device(lib) == NOT_ENOUGH_DATA and a.host(lib) == NOT_ENOUGH_DATA and a.untouched()


def test_mirror_raises_before_any_native_call(lib, monkeypatch):
    from sparkts import stats
    from sparkts.errors import IllegalArgumentException, MathIllegalArgumentException
    from sparkts.timeseriesrdd import TimeSeriesRDD

    def boom(*a, **k):
        raise AssertionError("native call")
    monkeypatch.setattr(lib, "sts_cross_moments_host", boom)
    monkeypatch.setattr(lib, "sts_cross_moments", boom)
    x = np.arange(12.0).reshape(3, 4)
    with pytest.raises(IllegalArgumentException):
        stats.cov(x, np.zeros((2, 5)))                       # another T
    with pytest.raises(IllegalArgumentException):
        stats.corr(np.zeros((2, 3, 4)))                      # not a panel
    with pytest.raises(IllegalArgumentException):
        stats.corr(x, np.zeros((2, 2, 4)))
    with pytest.raises(IllegalArgumentException):
        stats.cov(np.zeros((0, 4)))
    with pytest.raises(MathIllegalArgumentException):
        stats.cov(np.zeros((3, 1)))
    with pytest.raises(IllegalArgumentException):
        stats.cross.cross_moments(x, kind="spearman")
    rdd = TimeSeriesRDD(None, ["a", "b", "c"], x)
    with pytest.raises(IllegalArgumentException):
        rdd.covariance(TimeSeriesRDD(None, ["d"], np.zeros((1, 5))))
    with pytest.raises(IllegalArgumentException):
        rdd.correlation(np.zeros((5, 2)))                    # (T, k) with another T
    with pytest.raises(IllegalArgumentException):
        rdd.correlation(np.zeros(4))


# ---------------- the restatement ----------------

def test_fixture_is_what_the_generator_writes():
    pytest.importorskip("mpmath")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "cross_ref.py"), "--check"])


@pytest.mark.parametrize("name", cr.FAMILIES)
def test_restatement_against_the_exact_fixture(name):
    g = cr.load_golden()[name]
    x, y = cr.golden_case(name)
    assert x.shape[0] <= 8 and x.shape[1] <= 64
    assert [x[0, 0], x[-1, -1], y[-1, -1]] == g["probe"], "the case is not the fixture's"
    for form, yy in (("sym", None), ("cross", y)):
        for kind in ("cov", "corr"):
            out, mx, my = cr.moments(x, yy, kind)
            e = cr.errors(out, g[form], kind)
            print(name, form, kind, e)
            assert e <= 3e-15, (name, form, kind, e)      # where the issue measured the restatement
            assert cr.mean_error(mx, g[form]["mean_x"], x) <= cr.mean_bar(x.shape[1])
            if yy is not None:
                assert cr.mean_error(my, g[form]["mean_y"], y) <= cr.mean_bar(x.shape[1])
    s = cr.moments(x, None, "corr")[0]
    assert (np.diag(s) == 1.0).all() and s.min() <= -1.0 + 1e-6       # the pair at -1


def test_restatement_against_numpy_on_ordinary_data():
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((7, 130)), rng.standard_normal((3, 130))
    assert np.allclose(cr.moments(x)[0], np.cov(x), rtol=1e-12, atol=1e-14)
    assert np.allclose(cr.moments(x, kind="corr")[0], np.corrcoef(x), rtol=1e-12, atol=1e-14)
    full = np.cov(np.vstack([x, y]))
    assert np.allclose(cr.moments(x, y)[0], full[:7, 7:], rtol=1e-12, atol=1e-14)
    full = np.corrcoef(np.vstack([x, y]))
    assert np.allclose(cr.moments(x, y, "corr")[0], full[:7, 7:], rtol=1e-12, atol=1e-14)
    assert np.array_equal(cr.moments(x)[1], x.sum(axis=1) / 130)


def test_restatement_rules():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((5, 40))
    x[1, 0] = np.nan
    x[2] = 0.1                      # a constant whose mean does not round to itself
    x[3, 39] = np.inf
    for kind in ("cov", "corr"):
        s, mx, _ = cr.moments(x, None, kind)
        assert np.isnan(s[[1, 3]]).all() and np.isnan(s[:, [1, 3]]).all() and np.isnan(mx[[1, 3]]).all()
        keep = [0, 4]
        if kind == "cov":
            assert (s[2, keep] == 0).all() and not np.signbit(s[2, keep]).any() and s[2, 2] == 0
        else:
            assert np.isnan(s[2]).all() and np.isnan(s[:, 2]).all() and s[0, 0] == s[4, 4] == 1.0
        clean = cr.moments(x[keep], None, kind)[0]
        assert np.allclose(s[np.ix_(keep, keep)], clean, rtol=1e-13, atol=0)    # numpy's own order: not bits
        c = cr.moments(x[keep], x, kind)[0]
        assert np.isnan(c[:, [1, 3]]).all()
        assert np.allclose(c[:, keep], cr.moments(x[keep], x[keep], kind)[0], rtol=1e-13, atol=0)
        ex = cr.exact(x, None)
        assert cr.errors(s, ex, kind) <= 3e-15


@pytest.mark.parametrize("name", cr.FAMILIES)
def test_restatement_holds_the_bar_on_the_hard_families(name):
    pytest.importorskip("mpmath")
    x = cr.family(name, cr.HARD_T)
    ex = cr.exact(x)
    for kind in ("cov", "corr"):
        e = cr.errors(cr.moments(x, None, kind)[0], ex, kind)
        print(name, kind, "restatement", e)
        assert e <= cr.BAR
    if name in ("walks_1e6", "level_1e9", "level_1e12"):
        # what the correction (and the centring before the products) buys: MLlib's formula misses the bar
        with np.errstate(all="ignore"):
            e1 = np.nanmax(np.abs(cr.one_pass(x) - ex["cov"]) / ex["scale"])
        print(name, "one-pass", e1)
        assert e1 > 1e3 * cr.BAR
