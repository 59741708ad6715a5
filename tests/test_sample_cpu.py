"""include/sts_sample.h without a GPU.

* The stream: csrc/sts_normal.hpp compiled for the host (tests/native/normal_harness.cpp) gives the
  bits of tests/sample_ref.py on a grid of seeds, series and positions and on hand-picked
  mantissas at every region boundary; the same program built with -fsanitize=address,undefined
  runs clean.  sample_ref's Philox reproduces oracle.gen_panel, its PPND16 agrees with CPython's C
  routine within 16 ulp, and its normals have the moments of N(0, 1).
* GARCHSuite's properties (S/../models/GARCHSuite.scala) on reference samples.
* The guards tests/test_abi.py and tests/test_stream_table.py give sts.h, for this header.
* The mirror's argument handling that needs no device.
"""
import ctypes
import math
import os
import re
import shutil
import statistics
import subprocess

import numpy as np
import pytest

import oracle
import sample_ref as sr
import test_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sts_sample.h")
HARNESS = os.path.join(ROOT, "tests", "native", "normal_harness.cpp")
BAD_ARG = 1
SEEDS = (5, 0xC0FFEE1234567890)          # the second has a high key word
SERIES = (0, 1, 2 ** 32 + 3)
STEPS = (0, 1, 2, 3, 2 ** 33 + 1)
RUN0, RUN = 1000, 4096                   # 4096 consecutive steps

# the last mantissa of the lower tail / of the central region (|u - 0.5| <= 0.425 flips between m and m + 1),
# the first mantissa with r = sqrt(-log u) <= 5, the extremes and the middle; test_region_boundaries
# checks that they sit where this says
M_LOWER, M_UPPER, M_R5 = 337769972052786, 4165829655317708, 62546
MANTISSAS = [M_LOWER - 1, M_LOWER, M_LOWER + 1, M_LOWER + 2, M_UPPER - 1, M_UPPER, M_UPPER + 1, M_UPPER + 2,
             M_R5 - 2, M_R5 - 1, M_R5, M_R5 + 1, 2 ** 52 - 1 - M_R5, 2 ** 52 - M_R5, 0, 2 ** 52 - 1, 2 ** 51, 2 ** 51 - 1, 1]

lib = test_abi.lib


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ulps(a, b):
    """distance in units of the last place between doubles of one sign"""
    a, b = bits(a).astype(np.int64), bits(b).astype(np.int64)
    return np.abs(a - b)


# ---------------- the stream ----------------

def build_harness(tmp, flags, name):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp / name)
    subprocess.check_call([gxx, "-std=c++17", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "spark-timeseries_amd", "csrc"), HARNESS, "-o", out])
    return out


@pytest.fixture(scope="module")
def grid():
    """(records for the harness, sample_ref's values)"""
    recs, want = [], []
    for seed in SEEDS:
        for g in SERIES:
            t = np.array(list(STEPS) + list(range(RUN0, RUN0 + RUN)), dtype=np.uint64)
            recs += ["z %x %x %x" % (seed, g, int(v)) for v in t]
            want.append(sr.normals(seed, np.uint64(g), t))
    recs += ["m %x" % m for m in MANTISSAS]
    want.append(np.array([sr.normal_of_m(m) for m in MANTISSAS]))
    return "%d\n%s\n" % (len(recs), "\n".join(recs)), np.concatenate(want)


def run_harness(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return np.array([int(b, 16) for b in out.stdout.split()], dtype=np.uint64).view(np.float64)


def test_host_normal_is_bit_exact(tmp_path, grid):
    text, want = grid
    got = run_harness(build_harness(tmp_path, ["-O2"], "normal"), text)
    sr.assert_bits(got, want, "sts_normal.hpp on the host")
    k = len(MANTISSAS)
    assert got[-k + MANTISSAS.index(0)] == -sr.EXTREME and got[-k + MANTISSAS.index(2 ** 52 - 1)] == sr.EXTREME
    assert np.isfinite(got).all() and np.abs(got).max() <= sr.EXTREME


def test_host_normal_under_sanitizers(tmp_path, grid):
    """the stand-alone program with AddressSanitizer and UBSan: clean exit, the same bits"""
    text, want = grid
    exe = build_harness(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "normal_san")
    sr.assert_bits(run_harness(exe, text), want, "sts_normal.hpp under ASan + UBSan")


def test_region_boundaries():
    q = lambda m: sr.uniform(m) - 0.5
    assert abs(q(M_LOWER)) > 0.425 >= abs(q(M_LOWER + 1)) and abs(q(M_UPPER)) <= 0.425 < abs(q(M_UPPER + 1))
    r = lambda m: math.sqrt(-oracle.fdlibm_log(sr.uniform(m)))
    assert r(M_R5 - 1) > 5.0 >= r(M_R5)
    assert sr.uniform(0) == 2.0 ** -53 and sr.uniform(2 ** 52 - 1) == 1.0 - 2.0 ** -53
    # symmetric about 0.5: m and 2^52 - 1 - m give u and 1 - u, and z is odd
    for m in MANTISSAS:
        assert sr.uniform(2 ** 52 - 1 - m) == 1.0 - sr.uniform(m)
        assert sr.normal_of_m(2 ** 52 - 1 - m) == -sr.normal_of_m(m)


def test_philox_reproduces_the_panel_generator():
    """sample_ref.philox against oracle.gen_panel (sts_gen.hip's stream: counter (t, s), u from 53 bits)"""
    seed, S, T, s0 = 0x1234567890ABCDEF, 5, 12, 2 ** 32 + 1
    want = oracle.gen_panel(seed, S, T, 0.0, s0=s0)
    s = np.arange(S, dtype=np.uint64) + np.uint64(s0)
    u53 = lambda w: (((w[0] >> np.uint64(5)) << np.uint64(26)) | (w[1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53
    key = (seed & 0xFFFFFFFF, seed >> 32)
    us = u53(sr.philox(0xFFFFFFFF, 0xFFFFFFFF, s & sr.M32, s >> np.uint64(32), *key))
    t = np.arange(T, dtype=np.uint64)[None, :]
    sg = np.broadcast_to(s[:, None], (S, T))
    u = u53(sr.philox(np.broadcast_to(t, (S, T)), np.zeros((S, T), dtype=np.uint64), sg & sr.M32, sg >> np.uint64(32), *key))
    got = ((100.0 + 10.0 * us)[:, None] + np.arange(T, dtype=np.float64)[None, :] / float(T)) + (u - 0.5)
    sr.assert_bits(got, want, "philox")
    # and the sampling stream is another one: bit 63 of the counter
    assert not np.array_equal(sr.words(seed, s[0], 0)[0], sr.philox(0, 0, s[0] & sr.M32, s[0] >> np.uint64(32), *key)[0])


def test_ppnd16_against_cpython():
    """4e5 values of u: 2e5 anywhere, 1e5 among the 2^20 smallest mantissas and 1e5 among the 2^20
    largest (both tail rationals: r = 5 is crossed at m = 62546), the extremes included.  Bar: 16 ulp.
    With math.log this restatement IS the C routine, bit for bit (asserted below); moving every log by
    one ulp -- more than fdlibm differs from glibc -- moves the result by at most 8 ulp, measured on
    the CPU; 16 doubles that."""
    rng = np.random.default_rng(241)
    m = np.concatenate([rng.integers(0, 2 ** 52, 200000), rng.integers(0, 2 ** 20, 100000),
                        2 ** 52 - 1 - rng.integers(0, 2 ** 20, 100000)])
    m[:4] = [0, 2 ** 52 - 1, 2 ** 20 - 1, 2 ** 52 - 2 ** 20]
    inv = statistics.NormalDist().inv_cdf
    u = [sr.uniform(v) for v in m]
    want = np.array([inv(v) for v in u])
    got = np.array([sr.ppnd16(v) for v in u])
    d = ulps(got, want)
    print("ppnd16 vs statistics.NormalDist.inv_cdf: max %d ulp, %d of %d differ" % (d.max(), (d > 0).sum(), d.size))
    assert np.array_equal(np.signbit(got), np.signbit(want)) and d.max() <= 16
    same = np.array([sr.ppnd16(v, math.log) for v in u[:100000:7] + u[200000::7]])
    assert np.array_equal(bits(same), bits(np.concatenate([want[:100000:7], want[200000::7]])))


def lag1(a):
    a = a - a.mean()
    return float((a[1:] * a[:-1]).sum() / (a * a).sum())


def test_moments():
    """5 sigma bounds for N iid N(0, 1) values (derived, not measured): the mean has variance 1 / N,
    the sample variance 2 / N, a lag-1 autocorrelation 1 / N"""
    N = 2 ** 18
    z = sr.normal_panel(2024, 0, 1, 0, N)[0]
    print("mean %.3g  var - 1 %.3g  lag-1 along t %.3g" % (z.mean(), z.var() - 1.0, lag1(z)))
    assert abs(z.mean()) < 5.0 / math.sqrt(N)
    assert abs(z.var() - 1.0) < 5.0 * math.sqrt(2.0 / N)
    assert abs(lag1(z)) < 5.0 / math.sqrt(N)                      # adjacent t: the two halves of a call, and calls
    zs = sr.normals(2024, np.arange(N, dtype=np.uint64), np.uint64(6))
    print("lag-1 across series %.3g" % lag1(zs))
    assert abs(lag1(zs)) < 5.0 / math.sqrt(N)                     # adjacent series at a fixed t


# ---------------- GARCHSuite on reference samples ----------------

N_SUITE, SEED_SUITE = 10000, 5


@pytest.fixture(scope="module")
def garch_ts():
    return sr.garch_sample(sr.normal_panel(SEED_SUITE, 0, 1, 0, N_SUITE)[0], .2, .3, .4)


def test_suite_log_likelihood(garch_ts):
    """GARCHSuite.scala:23-39"""
    right = oracle.garch_loglik(garch_ts, .2, .3, .4)
    w1, w2, w3 = (oracle.garch_loglik(garch_ts, *p) for p in ((.3, .4, .5), (.25, .35, .45), (.1, .2, .3)))
    assert right > w1 and right > w2 and right > w3 and w2 > w1
    assert garch_ts[0] == 0.0 and not np.signbit(garch_ts[0])


def test_suite_gradient(garch_ts):
    """GARCHSuite.scala:41-55"""
    assert (oracle.garch_gradient(garch_ts, .2 + .1, .3 + .05, .4 + .1) < 0.0).all()
    assert (oracle.garch_gradient(garch_ts, .2 - .1, .3 - .05, .4 - .1) > 0.0).all()


def test_suite_standardize_and_filter():
    """GARCHSuite.scala:99-111, on the draws a second call of the same generator takes"""
    g = sr.normal_panel(SEED_SUITE, 0, 1, N_SUITE, N_SUITE)[0]
    ts = sr.garch_sample(g, .2, .3, .4, 40.0, .4)
    std = oracle.argarch_remove(ts, 40.0, .4, .2, .3, .4)
    back = oracle.argarch_add(std, 40.0, .4, .2, .3, .4)
    assert (np.abs(back - ts) < .001).all()


def test_sampler_is_not_add_effects():
    """sampleWithVariances is another recurrence than addTimeDependentEffects: element 0 is 0.0 and the
    variance sums in another order"""
    g = sr.normal_panel(3, 0, 1, 0, 64)[0]
    ts, add = sr.garch_sample(g, .2, .3, .4), oracle.garch_add(g, .2, .3, .4)
    assert ts[0] == 0.0 and add[0] != 0.0 and not np.array_equal(ts[1:], add[1:])
    # unchecked parameters give the reference's NaN / inf: alpha + beta > 1 -> h_0 < 0 -> NaN from step 0 on
    bad = sr.garch_sample(g, .2, .7, .6)
    assert bad[0] == 0.0 and np.isnan(bad[1:]).all()
    assert np.isnan(sr.garch_sample(g, np.nan, .3, .4)[1:]).all()


# ---------------- the header's guards ----------------

def declared(monkeypatch):
    monkeypatch.setattr(test_abi, "HEADER", HEADER)
    return test_abi.declared()


def stream_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(m.group(2) for m in re.finditer(r"\b(int|const char\*)\s+(sts_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
                  if re.search(r"void\s*\*\s*stream\s*$", m.group(3).strip()))


NAMES = ["sts_ar_sample", "sts_argarch_sample", "sts_arima_sample", "sts_garch_sample", "sts_sample_normal"]


def test_library_exports_every_declared_symbol(lib, monkeypatch):
    d = declared(monkeypatch)
    assert sorted(d) == NAMES, sorted(d)
    out = subprocess.check_output(["nm", "-D", "--defined-only", test_abi.LIB]).decode()
    missing = set(d) - set(re.findall(r" T (sts_\w+)", out))
    assert not missing, missing


def test_bindings_match_header_arity(lib, monkeypatch):
    from sparkts import _native
    d = declared(monkeypatch)
    assert set(d) == set(_native.SAMPLE_SIGNATURES), set(d) ^ set(_native.SAMPLE_SIGNATURES)
    assert not set(d) & (set(_native.SIGNATURES) | set(_native.TRANSFORM_SIGNATURES))
    for name, n in d.items():
        assert len(_native.SAMPLE_SIGNATURES[name][1]) == n, name
        assert getattr(lib, name).argtypes == _native.SAMPLE_SIGNATURES[name][1], name
    if os.path.exists(_native.AB_LIB_PATH):
        assert _native.load_variant(_native.AB_LIB_PATH).sts_garch_sample.argtypes is not None


def test_every_stream_entry_point_has_a_row():
    import test_sample_stream_gpu as ts
    names = stream_entry_points()
    assert names == NAMES, names                       # all five end in `void* stream`; no _host forms
    covered = {n for t in ts.TABLE for n in t[1]}
    assert not sorted(set(names) - covered), "no row in test_sample_stream_gpu.TABLE for %s" % sorted(set(names) - covered)
    assert not sorted(covered - set(names)), "stale rows: %s" % sorted(covered - set(names))
    assert len(set(ts.IDS)) == len(ts.IDS)
    # none takes err_per_series: every one is held to "returns while the gate is shut"
    assert set(ts.ASYNC) == set(names) and not ts.SYNC


# ---------------- argument errors and empty calls need no device ----------------

def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


S, N = 3, 10
O = np.zeros((S, 2 * N))
V = np.full(S, 0.25)
COEF = np.full((S, 4), 0.1)


def calls(lib, out=O, s0=0, S_=S, n=N, ld=2 * N, t0=0, v=V, coef=COEF, p=2, d=1, q=1):
    """every entry point with the same shape arguments -> {name: status}"""
    o, vv, cf, seed = _p(out), _p(v), _p(coef), 7
    return {
        "sts_sample_normal": lib.sts_sample_normal(o, s0, S_, n, ld, t0, seed, None),
        "sts_garch_sample": lib.sts_garch_sample(o, s0, S_, n, ld, vv, vv, vv, t0, seed, None),
        "sts_argarch_sample": lib.sts_argarch_sample(o, s0, S_, n, ld, vv, vv, vv, vv, vv, t0, seed, None),
        "sts_ar_sample": lib.sts_ar_sample(o, s0, S_, n, ld, vv, cf, p, t0, seed, None),
        "sts_arima_sample": lib.sts_arima_sample(o, s0, S_, n, ld, p, d, q, 1, cf, t0, seed, None),
    }


@pytest.mark.parametrize("kw", [dict(s0=-1), dict(t0=-1), dict(ld=N - 1), dict(n=-1), dict(S_=-1), dict(out=None),
                                dict(n=2 ** 31, ld=2 ** 31)], ids=lambda k: ",".join("%s=%s" % i for i in k.items()))
def test_argument_errors_need_no_device(lib, kw):
    for name, st in calls(lib, **kw).items():
        assert st == BAD_ARG, (name, st, lib.sts_last_error())
        assert lib.sts_last_error()
    assert not O.any()


def test_model_errors_and_empty_calls_need_no_device(lib):
    o, v, cf = _p(O), _p(V), _p(COEF)
    # NULL parameter arrays with S > 0
    assert lib.sts_garch_sample(o, 0, S, N, N, v, None, v, 0, 7, None) == BAD_ARG
    assert lib.sts_argarch_sample(o, 0, S, N, N, None, v, v, v, v, 0, 7, None) == BAD_ARG
    assert lib.sts_argarch_sample(o, 0, S, N, N, v, v, v, v, None, 0, 7, None) == BAD_ARG
    assert lib.sts_ar_sample(o, 0, S, N, N, None, cf, 2, 0, 7, None) == BAD_ARG
    assert lib.sts_ar_sample(o, 0, S, N, N, v, None, 2, 0, 7, None) == BAD_ARG
    assert lib.sts_arima_sample(o, 0, S, N, N, 1, 0, 1, 1, None, 0, 7, None) == BAD_ARG
    # the order limits of the _add entry points
    assert lib.sts_ar_sample(o, 0, S, N, N, v, cf, -1, 0, 7, None) == BAD_ARG
    assert lib.sts_arima_sample(o, 0, S, N, N, 5, 0, 0, 1, cf, 0, 7, None) == BAD_ARG       # p > STS_ARIMA_MAX_ORDER
    assert lib.sts_arima_sample(o, 0, S, N, N, 1, N + 1, 0, 1, cf, 0, 7, None) == BAD_ARG   # d > n
    assert lib.sts_arima_sample(o, 0, S, N, N, 0, 0, 0, 0, cf, 0, 7, None) == BAD_ARG       # no coefficients
    assert lib.sts_arima_sample(o, 0, S, 0, N, 1, 1, 0, 1, cf, 0, 7, None) == BAD_ARG       # d > n at n == 0 too
    assert lib.sts_last_error()
    # nothing to write: STS_OK before any device action, NULL everything allowed at S == 0
    for kw in (dict(S_=0), dict(n=0), dict(S_=0, out=None, v=None, coef=None), dict(n=0, ld=0, out=None)):
        for name, st in calls(lib, d=0, **kw).items():
            assert st == 0, (name, kw, st, lib.sts_last_error())
    assert not O.any()


# ---------------- the mirror ----------------

def test_mirror_wants_the_philox_generator():
    import random as pyrandom
    from sparkts.models import ARIMAModel, ARModel, ARGARCHModel, EWMAModel, GARCHModel
    models = [GARCHModel(.2, .3, .4), ARGARCHModel(0.0, .1, .2, .3, .4), ARModel(1.0, [.5, .1]),
              ARIMAModel(1, 1, 1, [0.1, 0.5, 0.2])]
    for m in models:
        for rand in (pyrandom.Random(5), np.random.default_rng(5), None, 5):
            with pytest.raises(TypeError, match="PhiloxGenerator"):
                m.sample(10, rand)
    assert not hasattr(EWMAModel(0.5), "sample")      # no sample in the reference, none here


def test_generator_bookkeeping():
    from sparkts.errors import IllegalArgumentException
    from sparkts.random import PhiloxGenerator
    g = PhiloxGenerator(5)
    assert (g.seed, g.first_series, g.position) == (5, 0, 0)
    assert g.take(10) == 0 and g.position == 10
    assert g.take(0) == 10 and g.take(7) == 10 and g.position == 17
    h = PhiloxGenerator(2 ** 64 - 1, first_series=2 ** 40)
    assert (h.seed, h.first_series, h.position) == (2 ** 64 - 1, 2 ** 40, 0)
    for bad in (lambda: PhiloxGenerator(-1), lambda: PhiloxGenerator(2 ** 64), lambda: PhiloxGenerator(1, -1),
                lambda: g.take(-1)):
        with pytest.raises(IllegalArgumentException):
            bad()
    assert g.position == 17


def test_shape_rules_of_paths():
    from sparkts.random import path_count
    scalars = [(.2, "omega", 0), (np.float64(.3), "alpha", 0), (.4, "beta", 0)]
    assert path_count(scalars, None, "t") == (1, True)             # (n,)
    assert path_count(scalars, 64, "t") == (64, False)             # (P, n): one model, P streams
    assert path_count(scalars, 1, "t") == (1, False)               # (1, n), not (n,)
    per = [(np.full(7, .2), "omega", 0), (.3, "alpha", 0), (np.full(7, .4), "beta", 0)]
    assert path_count(per, None, "t") == (7, False)                # (S, n); scalars broadcast
    assert path_count([(np.zeros(3), "coefficients", 1)], 5, "t") == (5, False)
    assert path_count([(np.zeros((4, 3)), "coefficients", 1), (1.0, "c", 0)], None, "t") == (4, False)
    with pytest.raises(ValueError, match="paths"):
        path_count(per, 3, "t")
    with pytest.raises(ValueError, match="disagree"):
        path_count([(np.zeros(3), "omega", 0), (np.zeros(4), "alpha", 0)], None, "t")
    with pytest.raises(ValueError, match="shape"):
        path_count([(np.zeros((2, 2, 2)), "coefficients", 1)], None, "t")
    with pytest.raises(ValueError, match="negative"):
        path_count(scalars, -1, "t")
