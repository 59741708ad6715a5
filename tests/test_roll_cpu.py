"""include/sts_roll.h without a GPU: the guards tests/test_abi.py gives sts.h, for the seventh header,
and the numpy restatement of its definition (tests/roll_ref.py) against exact arithmetic.

* every function of sts_roll.h is exported by libsts_hip.so and bound in _native.ROLL_SIGNATURES with
  the header's arity and argument types; nothing of it appears in sts.h;
* the enum values and both *_from_name functions behave as declared;
* every call-level error the header lists comes back with its status before any device action, from
  the device entry points and from their `_host` twins, a sentinel-filled out untouched;
* the restatement equals the scalar loop bit for bit, and sits within the header's bars of exact
  rational arithmetic on the hard families at windows 2, 5, 20, 252 and 1024;
* the properties the header promises hold for the restatement: shift purity, truncation = NaN
  padding, the constant rule, an infinity does not outlive its windows, COV(x, x) = VAR(x) and
  BETA(x, x) = 1;
* the difference of two cumulative sums misses the bar on the level-1e9 family.

Bars (the header's ACCURACY): |M2 - exact| <= 1e-10 M2_exact; |Cxy - exact| <= 1e-10 sqrt(M2x M2y);
|mean - exact| <= 1e-10 max |x| over the window.  Worst values measured with this file (python -m
pytest tests/test_roll_cpu.py -s): M2 1.8e-14, Cxy 4.7e-15, mean 1.7e-14 (all on flat stretches beside jumps).
"""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import roll_ref as rr
import test_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sts_roll.h")
BAD_ARG = 1
SENTINEL = -3.0e55

lib = test_abi.lib


def declared(monkeypatch):
    monkeypatch.setattr(test_abi, "HEADER", HEADER)
    return test_abi.declared()


# ---------------- the header and its bindings ----------------

NAMES = ["sts_roll_op_from_name", "sts_roll_pair", "sts_roll_pair_host", "sts_roll_pair_op_from_name", "sts_roll_stat",
         "sts_roll_stat_host"]


def test_library_exports_every_declared_symbol(lib, monkeypatch):
    d = declared(monkeypatch)
    assert sorted(d) == NAMES, sorted(d)
    out = subprocess.check_output(["nm", "-D", "--defined-only", test_abi.LIB]).decode()
    missing = set(d) - set(re.findall(r" T (sts_\w+)", out))
    assert not missing, missing


def test_bindings_match_header_arity_and_types(lib, monkeypatch):
    from sparkts import _native
    d = declared(monkeypatch)
    assert set(d) == set(_native.ROLL_SIGNATURES), set(d) ^ set(_native.ROLL_SIGNATURES)
    for table in (_native.SIGNATURES, _native.TRANSFORM_SIGNATURES, _native.SAMPLE_SIGNATURES, _native.INDEX_SIGNATURES,
                  _native.REGRESS_SIGNATURES, _native.CROSS_SIGNATURES):
        assert not set(d) & set(table)
    for name, n in d.items():
        assert len(_native.ROLL_SIGNATURES[name][1]) == n, name
        assert getattr(lib, name).argtypes == _native.ROLL_SIGNATURES[name][1], name
        assert getattr(lib, name).restype is ctypes.c_int
    assert (d["sts_roll_stat"], d["sts_roll_pair"], d["sts_roll_stat_host"], d["sts_roll_pair_host"]) == (10, 13, 8, 11)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("sts_roll_stat", "sts_roll_pair", "sts_roll_stat_host", "sts_roll_pair_host"):
        args = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1).split(",")
        want = [ctypes.c_void_p if "*" in a else ctypes.c_int64 if "int64_t" in a else ctypes.c_int for a in args]
        assert _native.ROLL_SIGNATURES[name][1] == want, name
    assert "#ifndef STS_ROLL_H" in text and 'extern "C"' in text and '#include "sts.h"' in text
    assert "sts_roll" not in open(os.path.join(ROOT, "include", "sts.h")).read().lower()
    assert int(re.search(r"#define STS_ROLL_MAX_WINDOW (\d+)", text).group(1)) == _native.ROLL_MAX_WINDOW == rr.MAX_WINDOW
    assert re.search(r"#define STS_ROLL_TILE (\d+)", text) and re.search(r"#define STS_ROLL_CHAINS (\d+)", text)


def test_enums_and_names(lib):
    from sparkts import _native
    text = open(HEADER).read()
    ops = re.search(r"typedef enum \{([^}]*)\} sts_roll_op;", text).group(1)
    pops = re.search(r"typedef enum \{([^}]*)\} sts_roll_pair_op;", text).group(1)
    got = {k.strip(): int(v) for k, v in (e.split("=") for e in ops.split(","))}
    assert got == {"STS_ROLL_" + n.upper(): i for i, n in enumerate(rr.OPS)}
    got = {k.strip(): int(v) for k, v in (e.split("=") for e in pops.split(","))}
    assert got == {"STS_ROLL_" + n.upper(): i for i, n in enumerate(rr.PAIR_OPS)}
    assert _native.ROLL_OPS == rr.OPS and _native.ROLL_PAIR_OPS == rr.PAIR_OPS
    for i, n in enumerate(rr.OPS):
        assert lib.sts_roll_op_from_name(n.encode()) == i
        assert lib.sts_roll_pair_op_from_name(n.encode()) == -2
    for i, n in enumerate(rr.PAIR_OPS):
        assert lib.sts_roll_pair_op_from_name(n.encode()) == i
        assert lib.sts_roll_op_from_name(n.encode()) == -2
    for bad in (b"", b"SUM", b"sum ", b"variance", b"median", None):
        assert lib.sts_roll_op_from_name(bad) == -2 and lib.sts_roll_pair_op_from_name(bad) == -2, bad


# ---------------- argument errors need no device ----------------

def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class Args:
    """a valid call on host memory (never dereferenced: every guard comes before any device action)"""

    def __init__(self, pair, Sy=None):
        self.pair = pair
        self.S, self.T, self.ld_x, self.ld_out, self.window, self.min_periods, self.op = 3, 9, 11, 10, 4, 2, 1
        self.Sy = self.S if Sy is None else Sy
        self.ld_y = 12
        self.x = np.arange(3 * 11, dtype=np.float64)
        self.y = np.arange(3 * 12, dtype=np.float64)
        self.out = np.full(3 * 11, SENTINEL)
        self.px, self.py, self.pout = _p(self.x), _p(self.y), _p(self.out)

    def device(self, lib):
        if self.pair:
            return lib.sts_roll_pair(self.px, self.py, self.Sy, self.ld_y, self.pout, self.S, self.T, self.ld_x, self.ld_out,
                                     self.window, self.min_periods, self.op, None)
        return lib.sts_roll_stat(self.px, self.pout, self.S, self.T, self.ld_x, self.ld_out, self.window, self.min_periods,
                                 self.op, None)

    def host(self, lib):
        if self.pair:
            return lib.sts_roll_pair_host(self.px, self.py, self.Sy, self.ld_y, self.pout, self.S, self.T, self.ld_x,
                                          self.window, self.min_periods, self.op)
        return lib.sts_roll_stat_host(self.px, self.pout, self.S, self.T, self.ld_x, self.window, self.min_periods, self.op)

    def untouched(self):
        return bool((self.out == SENTINEL).all())


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _overlap_x(a):
    a.pout = ctypes.c_void_p(a.x.ctypes.data + 8 * ((a.S - 1) * a.ld_x + a.T - 1))       # element (S - 1, T - 1) of x


def _overlap_y(a):
    a.pout = ctypes.c_void_p(a.y.ctypes.data + 8 * (a.T - 1))                            # the last step of y's first row


# (id, which entry points: "stat" / "pair" / "both", mutation, applies to the host twin)
GUARDS = [
    ("null_x", "both", _set(px=None), True),
    ("null_out", "both", _set(pout=None), True),
    ("null_y", "pair", _set(py=None), True),
    ("S_0", "both", _set(S=0, Sy=0), True),
    ("S_negative", "both", _set(S=-1, Sy=-1), True),
    ("T_0", "both", _set(T=0), True),
    ("T_negative", "both", _set(T=-2), True),
    ("ld_x_below_T", "both", _set(ld_x=8), True),
    ("ld_out_below_T", "both", _set(ld_out=8), False),
    ("ld_y_below_T", "pair", _set(ld_y=8), True),
    ("window_0", "both", _set(window=0, min_periods=1), True),
    ("window_negative", "both", _set(window=-4), True),
    ("window_above_cap", "both", _set(window=rr.MAX_WINDOW + 1), True),
    ("min_periods_0", "both", _set(min_periods=0), True),
    ("min_periods_above_window", "both", _set(min_periods=5), True),
    ("op_negative", "both", _set(op=-1), True),
    ("op_7", "stat", _set(op=7), True),
    ("op_3", "pair", _set(op=3), True),
    ("Sy_2", "pair", _set(Sy=2), True),
    ("Sy_0", "pair", _set(Sy=0), True),
    ("out_is_x", "both", lambda a: setattr(a, "pout", a.px), True),
    ("out_overlaps_x", "both", _overlap_x, True),
    ("out_is_y", "pair", lambda a: setattr(a, "pout", a.py), True),
    ("out_overlaps_y", "pair", _overlap_y, True),
    ("out_overlaps_shared_y", "pair", lambda a: (_set(Sy=1)(a), _overlap_y(a)), True),
]

GUARD_CALLS = [(g, kind, e) for g in GUARDS for kind in ("stat", "pair") if g[1] in (kind, "both")
               for e in ("device", "host") if e == "device" or g[3]]


@pytest.mark.parametrize("case,kind,entry", GUARD_CALLS, ids=["%s-%s-%s" % (g[0], k, e) for g, k, e in GUARD_CALLS])
def test_call_level_errors_leave_the_output_untouched(lib, case, kind, entry):
    name, _, mutate, _ = case
    a = Args(kind == "pair")
    mutate(a)
    assert getattr(a, entry)(lib) == BAD_ARG, (name, lib.sts_last_error())
    assert b"roll_" + kind.encode() in lib.sts_last_error()
    assert a.untouched()


def test_mirror_raises_before_any_native_call(lib, monkeypatch):
    from sparkts import rolling
    from sparkts.errors import IllegalArgumentException
    from sparkts.timeseriesrdd import TimeSeriesRDD

    def boom(*a, **k):
        raise AssertionError("native call")
    for fn in ("sts_roll_stat", "sts_roll_stat_host", "sts_roll_pair", "sts_roll_pair_host"):
        monkeypatch.setattr(lib, fn, boom)
    x = np.arange(12.0).reshape(3, 4)
    with pytest.raises(IllegalArgumentException):
        rolling.roll(x, "median", 2)
    with pytest.raises(IllegalArgumentException):
        rolling.roll(x, "cov", 2)                            # a pair op without other
    with pytest.raises(IllegalArgumentException):
        rolling.roll(x, "sum", 2, other=x)                   # a single op with other
    with pytest.raises(IllegalArgumentException):
        rolling.roll(np.zeros((2, 3, 4)), "sum", 2)
    with pytest.raises(IllegalArgumentException):
        rolling.roll(x, "beta", 2, other=np.zeros(5))        # another T
    with pytest.raises(IllegalArgumentException):
        rolling.roll(x, "beta", 2, other=np.zeros((2, 4)))   # another S
    with pytest.raises(IllegalArgumentException):
        rolling.roll(np.zeros((0, 4)), "sum", 2)
    rdd = TimeSeriesRDD(None, ["a", "b", "c"], x)
    with pytest.raises(IllegalArgumentException):
        rdd.rollBeta(np.zeros((4, 1)), 2)
    with pytest.raises(IllegalArgumentException):
        rdd.rollCov(TimeSeriesRDD(None, ["d"], np.zeros((1, 4))), 2)


# ---------------- the restatement ----------------

def noise(seed, S, T):
    return np.random.default_rng([91, seed, S, T]).standard_normal((S, T))


def holes(x, seed, p=0.15):
    x = x.copy()
    x[np.random.default_rng([92, seed]).random(x.shape) < p] = np.nan
    return x


def test_restatement_is_the_scalar_loop_bit_for_bit():
    x, y = holes(noise(1, 3, 40), 1), holes(noise(2, 3, 40), 2)
    x[0, 5], x[0, 6], x[1, 9:14] = 0.0, -0.0, 0.25
    y[2, 3] = np.inf
    for w in (1, 2, 3, 7, 45):
        m = rr.moments(x, w, y)
        ms = rr.moments(x, w)
        for s in range(3):
            for t in range(40):
                one = rr.scalar(rr.window_of(x[s], t, w), rr.window_of(y[s], t, w))
                solo = rr.scalar(rr.window_of(x[s], t, w))
                for k in ("sum", "mean", "min", "max", "M2", "M2y", "Cxy"):
                    assert rr.same_bits(m[k][s, t], one[k]), (w, s, t, k, m[k][s, t], one[k])
                for k in ("sum", "mean", "min", "max", "M2"):
                    assert rr.same_bits(ms[k][s, t], solo[k]), (w, s, t, k)
                assert m["n"][s, t] == one["n"] and ms["n"][s, t] == solo["n"]


WINDOWS = (2, 5, 20, 252, 1024)
T_HARD = 1100
WORST = {"M2": 0.0, "Cxy": 0.0, "mean": 0.0}


@pytest.mark.parametrize("name", rr.FAMILIES)
def test_restatement_against_exact_arithmetic(name):
    x = rr.family(name, T_HARD, S=1)[0]
    y = rr.family(name, T_HARD, S=1, seed=1)[0]
    for w in WINDOWS:
        m = rr.moments(x, w, y)
        ms = rr.moments(x, w)
        for t in sorted({w // 2, w - 1, (w + T_HARD) // 2, T_HARD - 1}):
            ex = rr.exact(rr.window_of(x, t, w), rr.window_of(y, t, w))
            for key, got, exact, scale2 in (("M2", ms["M2"][0, t], ex["M2"], ex["M2"] * ex["M2"]),
                                            ("M2", m["M2y"][0, t], ex["M2y"], ex["M2y"] * ex["M2y"]),
                                            ("Cxy", m["Cxy"][0, t], ex["Cxy"], ex["M2"] * ex["M2y"]),
                                            ("mean", ms["mean"][0, t], ex["mean"], ex["maxabs"] * ex["maxabs"])):
                err = Fraction(float(got)) - exact
                if scale2 == 0:
                    assert err == 0, (name, w, t, key, float(got))
                    continue
                rel = float(err * err / scale2) ** 0.5
                WORST[key] = max(WORST[key], rel)
                assert rel <= rr.BAR, (name, w, t, key, rel)
    print(name, "worst so far", WORST)


def test_cumulative_sums_miss_the_bar_at_level_1e9():
    """the bar has teeth: the variance from differences of two cumulative sums, on the same family"""
    x = rr.family("walk_1e9", T_HARD, S=1)[0]
    w = 20
    cs = rr.cumsum_var(x, w)
    worst = 0.0
    for t in (w - 1, 300, 700, T_HARD - 1):
        ex = rr.exact(rr.window_of(x, t, w))
        worst = max(worst, abs(float((Fraction(float(cs[t])) * (w - 1) - ex["M2"]) / ex["M2"])))
    print("cumulative-sum variance, level 1e9, window 20: worst relative error of M2 %.3g" % worst)
    assert worst > 1e6 * rr.BAR


def test_shift_purity_and_truncation():
    x = holes(noise(3, 2, 90), 3)
    k = 13
    shifted = np.concatenate([np.full((2, k), np.nan), x], axis=1)
    other = noise(4, 2, 90)
    oshift = np.concatenate([noise(5, 2, k), other], axis=1)
    for w in (1, 4, 30, 100):
        for mp in sorted({1, (w + 1) // 2, w}):
            for op in rr.OPS:
                a, b = rr.stat(x, op, w, mp), rr.stat(shifted, op, w, mp)
                assert rr.same_bits(a, b[:, k:]), (op, w, mp)       # truncation = NaN padding = a shift by k
            for op in rr.PAIR_OPS:
                a, b = rr.pair(x, other, op, w, mp), rr.pair(shifted, oshift, op, w, mp)
                assert rr.same_bits(a, b[:, k:]), (op, w, mp)


def test_constant_rule():
    x = np.full((1, 30), 0.1)               # a constant whose mean does not round to itself
    x[0, 20:] = np.arange(10) * 0.3
    y = noise(6, 1, 30)
    for w in (3, 7):
        flat = slice(w - 1, 20)
        for op, want in (("var", 0.0), ("std", 0.0)):
            v = rr.stat(x, op, w)[0, flat]
            assert (v == want).all() and not np.signbit(v).any()
        assert np.isnan(rr.stat(x, "zscore", w)[0, flat]).all()
        c = rr.pair(x, y, "cov", w)[0, flat]
        assert (c == 0.0).all() and not np.signbit(c).any()
        assert (rr.pair(y, x, "cov", w)[0, flat] == 0.0).all()
        assert np.isnan(rr.pair(x, y, "corr", w)[0, flat]).all() and np.isnan(rr.pair(y, x, "corr", w)[0, flat]).all()
        assert np.isnan(rr.pair(y, x, "beta", w)[0, flat]).all()            # the slope on a constant
        b = rr.pair(x, y, "beta", w)[0, flat]
        assert (b == 0.0).all() and not np.signbit(b).any()                   # a constant on noise
        assert (rr.stat(x, "var", w)[0, 21:] > 0).all()
        # without the rule 0.1's windows would not be exact zeros
        m = rr.moments(x, 3)
        assert m["M2"][0, 5] == 0.0


def test_an_infinity_does_not_outlive_its_windows():
    x, y = noise(7, 1, 60), noise(8, 1, 60)
    for bad in (np.inf, -np.inf):
        xi = x.copy()
        xi[0, 25] = bad
        for w in (1, 5, 12):
            hit = np.zeros(60, dtype=bool)
            hit[25:25 + w] = True
            for op in rr.OPS:
                a, b = rr.stat(x, op, w)[0], rr.stat(xi, op, w)[0]
                assert rr.same_bits(a[~hit], b[~hit]), (op, w)
                if op in ("var", "std", "zscore") and w > 1:
                    assert np.isnan(b[hit]).all(), (op, w)
                if op == "sum":
                    assert (b[hit] == bad).all()
            for op in rr.PAIR_OPS:
                for a, b in ((rr.pair(x, y, op, w)[0], rr.pair(xi, y, op, w)[0]), (rr.pair(y, x, op, w)[0], rr.pair(y, xi, op, w)[0])):
                    assert rr.same_bits(a[~hit], b[~hit]) and np.isnan(b[hit]).all(), (op, w)


def test_cov_of_a_series_with_itself_is_its_variance_and_beta_is_one():
    for name in ("returns", "walk_1e9", "scaled_down"):
        x = holes(rr.family(name, 300, S=2), 9, 0.05)
        for w in (2, 5, 60):
            mp = max(2, w // 2)
            var, cov, beta = rr.stat(x, "var", w, mp), rr.pair(x, x, "cov", w, mp), rr.pair(x, x, "beta", w, mp)
            assert rr.same_bits(var, cov), (name, w)
            pos = ~np.isnan(var) & (var > 0)
            assert pos.any() and (beta[pos] == 1.0).all(), (name, w)
            corr = rr.pair(x, x, "corr", w, mp)
            assert (np.abs(corr[pos] - 1.0) <= 4 * np.finfo(float).eps).all()


def test_restatement_against_numpy_on_ordinary_data():
    x, y = noise(10, 2, 200), noise(11, 2, 200)
    w = 20
    sw = np.lib.stride_tricks.sliding_window_view
    full = slice(w - 1, None)
    assert np.allclose(rr.stat(x, "mean", w)[:, full], sw(x, w, axis=1).mean(-1), rtol=1e-13)
    assert np.allclose(rr.stat(x, "var", w)[:, full], sw(x, w, axis=1).var(-1, ddof=1), rtol=1e-12)
    assert np.array_equal(rr.stat(x, "max", w)[:, full], sw(x, w, axis=1).max(-1))
    assert np.array_equal(rr.stat(x, "min", w)[:, full], sw(x, w, axis=1).min(-1))
    cx, cy = sw(x, w, axis=1), sw(y, w, axis=1)
    dx, dy = cx - cx.mean(-1, keepdims=True), cy - cy.mean(-1, keepdims=True)
    cov = (dx * dy).sum(-1) / (w - 1)
    assert np.allclose(rr.pair(x, y, "cov", w)[:, full], cov, rtol=1e-11, atol=1e-15)
    assert np.allclose(rr.pair(x, y, "beta", w)[:, full], cov / cy.var(-1, ddof=1), rtol=1e-11, atol=1e-15)
    assert np.allclose(rr.pair(x, y, "corr", w)[:, full], cov / (cx.std(-1, ddof=1) * cy.std(-1, ddof=1)), rtol=1e-11, atol=1e-15)
    assert np.isnan(rr.stat(x, "mean", w)[:, :w - 1]).all() and not np.isnan(rr.stat(x, "mean", w, 1)).any()
    assert np.isnan(rr.stat(x, "var", 1, 1)).all()          # one value has no variance
    z = np.zeros(4)
    z[1] = -0.0
    assert np.signbit(rr.stat(z, "min", 2)[1:3]).all() and not np.signbit(rr.stat(z, "max", 2)).any()
    assert np.signbit(rr.stat(np.array([-0.0, -0.0]), "sum", 2, 1)).all()
