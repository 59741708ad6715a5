"""sts_factor_ols, sts_factor_remove / sts_factor_add and their `_host` twins on the device, against
tests/factor_ols_ref.py (commons-math3's OLS with intercept restated in numpy) and the 60-digit
fixture tests/golden/factor_ols_exact.json.

Shapes.  T in {k + 2 (the minimum), 63, 64, 65, 390, 2560, 2561, 5000} and both sides of every seam
of the dispatch (sts::ols_regime), named in SEAMS below:
  stage   shared factors: (4 + k) T doubles fit the 60 KB of LDS of the several-waves-per-workgroup
          kernel (regime 0), or the one-wave kernel reads the basis from the scratch (regime 1);
  own     per-series factors: (1 + k) T doubles fit 48 KB and the wave builds its basis in LDS
          (regime 2), or the basis goes to the scratch (regime 1);
  wave    T <= 2560 one wave per series, beyond 256-thread sweeps (regime 3).
Two more seams of the launcher (sts_regress.hip launch_ols_kernel / launch_ols):
  unroll  k <= 4 takes the kernels whose per-factor registers are unrolled to 4, k >= 5 those unrolled
          to 8: K_SEAM = (4, 5) run in regimes 0 / 2 (T = 64, 390) and 3 (T = 2561), shared and per series;
  spw     in regime 0 a wave walks clamp(S / 8192, 1, 8) series (integer division): one below 16384
          series, two from there, eight from 65536: test_series_per_wave_seam (S = 16383 / 16384 /
          16389 / 32771) and test_several_series_per_wave (S = 65573).
k in {1, 3, 8}; S in {1, 3, 130}, the smaller two as prefixes of the largest (their bits must be
its bits); shared and per-series factors.  For T > 700 the restatement is evaluated for eight
series spread over the panel (it is a Python loop), the other series are held to the S = 3 bits
and to finiteness.

Bars.  Ordinary panels: 1e-10 relative to the restatement for coefficients, standard errors, rss,
tss, R^2 and sigma^2; residuals within 1e-10 rms of the restatement's.  Hard rows: the same 1e-10
against the EXACT values of the fixture, except coefficients and standard errors of the two
collinear rows, 16 kappa 2^-53 = 1.8e-9 (kappa = 1e6 by construction).  Scaled inputs: the same
bars against the scaled reference.  Effects: bit-exact.

Measured maxima on an MI355X are recorded in DESIGN.md section 5.20.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import bgbp_ref as br
import factor_ols_ref as fr
import layout_arena as la
import stream_gate as sg

pytestmark = pytest.mark.gpu
cache = functools.lru_cache(maxsize=None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_WAVE = 2560
POISON_OUT = -3.0e55
K_LIST = [1, 3, 8]
MODES = ["shared", "per_series"]
S_BIG = 130


def stage_seam(k):      # regime 0 / 1
    return (60 * 1024 // 8) // (4 + k)


def own_seam(k):        # regime 2 / 1 (beyond the one-wave limit for k = 1: no seam of its own)
    return (48 * 1024 // 8) // (1 + k)


SEAMS = {k: sorted(t for s in (stage_seam(k), own_seam(k)) if s < ONE_WAVE for t in (s, s + 1)) for k in K_LIST}
assert SEAMS == {1: [1536, 1537], 3: [1097, 1098, 1536, 1537], 8: [640, 641, 682, 683]}, SEAMS
T_COMMON = ["min", 63, 64, 65, 390, ONE_WAVE, ONE_WAVE + 1, 5000]


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


@pytest.fixture(scope="module")
def delay(torch):
    return sg.calibrate(torch)[0]


def lib():
    from sparkts import _native
    return _native.lib()


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def hv(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def dev(torch, a, dtype=np.float64):
    return torch.as_tensor(np.array(a, dtype=dtype, order="C"), device="cuda:0")


def factor_panel(F):
    """(T, k) -> (k, T), ld_f = T, fs = 0; (S, T, k) -> (S, k, T), ld_f = T, fs = k T"""
    F = np.asarray(F, dtype=np.float64)
    if F.ndim == 2:
        return np.ascontiguousarray(F.T), F.shape[1], F.shape[0], 0
    return np.ascontiguousarray(F.transpose(0, 2, 1)), F.shape[2], F.shape[1], F.shape[1] * F.shape[2]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Out:
    pass


def fit(torch, Y, F, se=True, stats=True, resid=True, err=True, host=False):
    """-> Out with status, beta, se, stats, resid, err (numpy; None where not asked for)"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    S, T = Y.shape
    fp, k, ld_f, fs = factor_panel(F)
    L, o = lib(), Out()
    if host:
        mk = lambda shape, on: np.full(shape, POISON_OUT) if on else None
        o.beta, o.se, o.stats, o.resid = mk((S, k + 1), True), mk((S, k + 1), se), mk((S, 4), stats), mk((S, T), resid)
        o.err = np.full(S, -7, dtype=np.int32) if err else None
        o.status = L.sts_factor_ols_host(hv(Y), S, T, T, hv(fp), k, ld_f, fs, hv(o.beta), hv(o.se), hv(o.stats),
                                         hv(o.resid), hv(o.err))
        return o
    mk = lambda shape, on: torch.full(shape, POISON_OUT, dtype=torch.float64, device="cuda:0") if on else None
    beta, dse, dstats, dres = mk((S, k + 1), True), mk((S, k + 1), se), mk((S, 4), stats), mk((S, T), resid)
    derr = torch.full((S,), -7, dtype=torch.int32, device="cuda:0") if err else None
    dy, df = dev(torch, Y), dev(torch, fp)
    o.status = L.sts_factor_ols(vp(dy), S, T, T, vp(df), k, ld_f, fs, vp(beta), k + 1, vp(dse), vp(dstats), vp(dres), T,
                                vp(derr), None)
    torch.cuda.synchronize()
    get = lambda t: None if t is None else t.cpu().numpy()
    o.beta, o.se, o.stats, o.resid, o.err = get(beta), get(dse), get(dstats), get(dres), get(derr)
    return o


def effects(torch, add, X, beta, F, inplace=False, host=False):
    X = np.ascontiguousarray(X, dtype=np.float64)
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    S, T = X.shape
    fp, k, ld_f, fs = factor_panel(F)
    L = lib()
    if host:
        x = X.copy()
        out = x if inplace else np.full((S, T), POISON_OUT)
        fn = L.sts_factor_add_host if add else L.sts_factor_remove_host
        assert fn(hv(x), hv(out), S, T, T, hv(fp), k, ld_f, fs, hv(beta)) == 0, L.sts_last_error()
        return out
    dx, df, db = dev(torch, X), dev(torch, fp), dev(torch, beta)
    out = dx if inplace else torch.full((S, T), POISON_OUT, dtype=torch.float64, device="cuda:0")
    fn = L.sts_factor_add if add else L.sts_factor_remove
    assert fn(vp(dx), vp(out), S, T, T, T, vp(df), k, ld_f, fs, vp(db), k + 1, None) == 0, L.sts_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_fit(o, want, rows, what, coef_bar=fr.BAR, bar=fr.BAR):
    """o's rows `rows` against want = (beta, se, stats, resid) of those rows"""
    e = {"beta": fr.rel(o.beta[rows], want[0]), "se": fr.rel(o.se[rows], want[1]), "stats": fr.rel(o.stats[rows], want[2]),
         "resid": fr.resid_err(o.resid[rows], want[3])}
    print("%s: max errors %s" % (what, {k: "%.2g" % v for k, v in e.items()}))
    assert e["beta"] <= coef_bar and e["se"] <= coef_bar, (what, e)
    assert e["stats"] <= bar and e["resid"] <= bar, (what, e)


# ---- ordinary panels ----

def real_T(T, k):
    return k + 2 if T == "min" else T


@cache
def inputs(T, k, mode):
    Y, F = fr.panel(9000 + 11 * T + k, S_BIG, T, k, per_series=(mode == "per_series"))
    rows = list(range(S_BIG)) if T <= 700 else [0, 1, 2, 31, 64, 65, 128, 129]
    want = fr.ols_panel(Y[rows], F if F.ndim == 2 else F[rows])
    for a in (Y, F) + want:
        a.setflags(write=False)
    return Y, F, rows, want


K_SEAM = (4, 5)         # the unroll seam of launch_ols_kernel
CASES = [(T, k) for k in K_LIST for T in T_COMMON + SEAMS[k]] + [(T, k) for k in K_SEAM for T in (64, 390, ONE_WAVE + 1)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,k", CASES, ids=["T%s-k%d" % c for c in CASES])
def test_ordinary(torch, T, k, mode):
    T = real_T(T, k)
    Y, F, rows, want = inputs(T, k, mode)
    big = fit(torch, Y, F)
    assert big.status == 0 and not big.err.any(), lib().sts_last_error()
    assert_fit(big, want, rows, "T=%d k=%d %s S=%d" % (T, k, mode, S_BIG))
    for a in (big.beta, big.se, big.stats, big.resid):
        assert np.isfinite(a).all()
    for S in (1, 3):       # results do not depend on S
        small = fit(torch, Y[:S], F if F.ndim == 2 else F[:S])
        assert small.status == 0
        for name in ("beta", "se", "stats", "resid", "err"):
            assert same(getattr(small, name), getattr(big, name)[:S]), (name, S)


def test_several_series_per_wave(torch):
    """From 16384 series a wave of the several-waves kernel walks more than one, 8 from 65536; here 8,
    and the last workgroup is partial.  The first 100 series, two of them poisoned, have the bits of a
    call of their own (one series per wave); series across the panel against the restatement."""
    S, T, k = 65536 + 37, 65, 3
    Y, F = fr.panel(1234, S, T, k)
    Y[33, 7] = np.nan
    Y[34, :] = -1.5
    o = fit(torch, Y, F)
    head = fit(torch, Y[:100], F)
    assert o.status == 0 and head.status == 0 and not o.err.any()
    for name in ("beta", "se", "stats", "resid"):
        assert same(getattr(o, name)[:100], getattr(head, name)), name
    assert np.isnan(o.beta[33]).all() and o.beta[34, 0] == -1.5 and np.isnan(o.stats[34, 2])
    rows = [0, 1, 35, 4097, 32768, 65535, 65536, S - 1]
    assert_fit(o, fr.ols_panel(Y[rows], F), rows, "S=%d" % S)
    ok = np.ones(S, dtype=bool)
    ok[[33, 34]] = False
    assert np.isfinite(o.beta[ok]).all() and np.isfinite(o.stats[ok]).all() and np.isfinite(o.resid[ok]).all()


def test_series_per_wave_seam(torch):
    """Both sides of the first step of the spw seam, and a value between the ends: 16383 series run one
    series per wave, 16384 (every workgroup full) and 16389 (a partial last workgroup) two, 32771 four.
    Every call has the bits of the next larger call's prefix; series across the largest panel and at
    the ends of the others against the restatement."""
    sizes = [16383, 16384, 16389, 32771]
    T, k = 65, 3
    Y, F = fr.panel(4321, sizes[-1], T, k)
    Y[16380, 3] = np.nan                       # a poisoned series beside the step
    outs = [fit(torch, Y[:S], F) for S in sizes]
    for o in outs:
        assert o.status == 0 and not o.err.any()
    for small, big, S in zip(outs, outs[1:], sizes):
        for name in ("beta", "se", "stats", "resid"):
            assert same(getattr(small, name), getattr(big, name)[:S]), (name, S)
    rows = [0, 8191, 8192, 16379, 16381, 16382, 16383, 16384, 16388, 16389, 32767, 32770]
    assert_fit(outs[-1], fr.ols_panel(Y[rows], F), rows, "spw seam")
    assert np.isnan(outs[-1].beta[16380]).all() and np.isnan(outs[-1].resid[16380]).all()
    ok = np.ones(sizes[-1], dtype=bool)
    ok[16380] = False
    assert np.isfinite(outs[-1].beta[ok]).all() and np.isfinite(outs[-1].stats[ok]).all()


# ---- hard rows against the exact fixture ----

@cache
def golden():
    """-> per hard row (beta, se, stats, resid), exact; the residuals from the 106-bit coefficients"""
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "factor_ols_exact.json")))
    out = []
    for i, r in enumerate(doc["rows"]):
        e = {key: np.array([float.fromhex(v) for v in r["exact"][key]]) for key in ("beta", "beta_lo", "se", "stats")}
        out.append((e["beta"], e["se"], e["stats"], fr.exact_resid(*fr.hard_row(i), e["beta"], e["beta_lo"])))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("i", range(len(fr.HARD_ROWS)), ids=["%s-%d" % r for r in fr.HARD_ROWS])
def test_hard_rows(torch, i, mode):
    """Each row beside an ordinary neighbour on either side (S = 3), shared and as per-series copies."""
    y, F = fr.hard_row(i)
    T = y.size
    Yn, _ = fr.panel(77 + i, 2, T, fr.HARD_K)
    Y = np.stack([Yn[0], y, Yn[1]])
    o = fit(torch, Y, F if mode == "shared" else np.stack([F] * 3))
    assert o.status == 0 and not o.err.any()
    want = tuple(a[None] for a in golden()[i])
    assert_fit(o, want, [1], "%s T=%d %s" % (fr.HARD_ROWS[i] + (mode,)), coef_bar=fr.KAPPA_BAR if fr.collinear(i) else fr.BAR)


# ---- shared against per-series copies ----

@pytest.mark.parametrize("T,k,same_regime", [(390, 3, False), (2000, 3, True), (2561, 8, True), (640, 8, False)])
def test_shared_and_replicated_factors_agree(torch, T, k, same_regime):
    """Regimes 1 and 3 serve both kinds of factors from bases the same kernel built: bit for bit.
    Regime 0 (shared) and regime 2 (own basis in LDS) build them with 256 and 64 threads: the bar."""
    Y, F = fr.panel(4100 + T, 5, T, k)
    a, b = fit(torch, Y, F), fit(torch, Y, np.stack([F] * 5))
    assert a.status == 0 and b.status == 0
    if same_regime:
        for name in ("beta", "se", "stats", "resid"):
            assert same(getattr(a, name), getattr(b, name)), name
    else:
        assert_fit(b, (a.beta, a.se, a.stats, a.resid), slice(None), "per-series copies against shared, T=%d" % T)


def test_basis_chunk_seam(torch):
    """Per-series factors one chunk of scratch bases and more: k = 8, T = 8192 is 512 KB (+ 1.2 KB) per
    basis, 510 bases to the 256 MB bound, so S = 600 takes two chunks (510 + 90).  The series around the seam and
    at the ends against the restatement; every series against a call of its own (S = 1)."""
    S, T, k = 600, 8192, 8
    rng = np.random.RandomState(99)
    F = rng.standard_normal((S, T, k))
    Y = fr.INTERCEPT + np.einsum("stk,k->st", F, fr.COEF[:k]) + rng.standard_normal((S, T))
    o = fit(torch, Y, F)
    assert o.status == 0 and not o.err.any()
    rows = [0, 509, 510, 511, 599]
    assert_fit(o, fr.ols_panel(Y[rows], F[rows]), rows, "chunk seam")
    for s in rows:
        one = fit(torch, Y[s:s + 1], F[s:s + 1])
        for name in ("beta", "se", "stats", "resid"):
            assert same(getattr(one, name)[0], getattr(o, name)[s]), (name, s)
    assert np.isfinite(o.beta).all() and np.isfinite(o.resid).all() and (o.stats[:, 2] > 0.5).all()


# ---- scaled inputs ----

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T,k", [(390, 3), (65, 8), (2561, 1)])
def test_scaled_series_and_factors(torch, T, k, mode):
    Y, F, rows, want = inputs(T, k, mode)
    for p in (300, -300):
        c = 2.0 ** p
        o = fit(torch, Y * c, F)
        assert o.status == 0
        sc = np.array([c * c, c * c, 1.0, c * c])
        assert_fit(o, (want[0] * c, want[1] * c, want[2] * sc, want[3] * c), rows, "y * 2^%d T=%d k=%d %s" % (p, T, k, mode))
    for p in (100, -100):
        c = 2.0 ** p
        o = fit(torch, Y, F * c)
        assert o.status == 0
        cs = np.concatenate([[1.0], np.full(k, 1.0 / c)])
        assert_fit(o, (want[0] * cs, want[1] * cs, want[2], want[3]), rows, "F * 2^%d T=%d k=%d %s" % (p, T, k, mode))


# ---- isolation: poisoned neighbours in the same workgroup / wave batch ----

@pytest.mark.parametrize("T,k", [(390, 3), (1537, 3), (2561, 3)], ids=["regimes0+2", "regime1", "regime3"])
@pytest.mark.parametrize("mode", MODES)
def test_poisoned_neighbours(torch, T, k, mode):
    """40 series: with four waves a workgroup and up to 8 series a wave (one below 16384 series), series
    s shares its workgroup with s +- 1 .. 3.  Poisoned: NaN, +-Inf, bit-constant, and (per series)
    duplicated and constant own factors.  Good series keep the bits of a run without them."""
    S = 40
    Y, F = fr.panel(600 + T, S, T, k, per_series=(mode == "per_series"))
    clean = fit(torch, Y, F)
    assert clean.status == 0 and not clean.err.any()
    Yp, Fp = Y.copy(), F.copy()
    Yp[5, T // 2] = np.nan
    Yp[6, 1] = np.inf
    Yp[9, T - 1] = -np.inf
    Yp[10, :] = 3.25
    bad = {5: "nan", 6: "nan", 9: "nan", 10: "const"}
    if mode == "per_series":
        Fp[14, :, 2] = Fp[14, :, 0]
        Fp[17, :, 1] = -4.5
        Fp[18, T // 3, 0] = np.nan
        bad.update({14: "singular", 17: "singular", 18: "nan"})
    o = fit(torch, Yp, Fp)
    assert o.status == 0
    for s in range(S):
        kind = bad.get(s)
        if kind is None:
            for name in ("beta", "se", "stats", "resid", "err"):
                assert same(getattr(o, name)[s], getattr(clean, name)[s]), (name, s)
        elif kind == "const":
            assert o.err[s] == 0
            assert o.beta[s, 0] == 3.25 and not o.beta[s, 1:].any() and not o.se[s].any()
            assert not o.resid[s].any() and o.stats[s, 0] == 0 and o.stats[s, 1] == 0 and o.stats[s, 3] == 0
            assert np.isnan(o.stats[s, 2])
        else:
            assert o.err[s] == (fr.SINGULAR if kind == "singular" else 0), (s, o.err[s])
            for name in ("beta", "se", "stats", "resid"):
                assert np.isnan(getattr(o, name)[s]).all(), (name, s)
    # err_per_series NULL: the first failing series is the call's status
    if mode == "per_series":
        assert fit(torch, Yp, Fp, err=False).status == fr.SINGULAR


def test_shared_singular_and_nan_factors(torch):
    Y, F = fr.panel(31, 9, 390, 3)
    Fd = F.copy()
    Fd[:, 1] = Fd[:, 0]
    o = fit(torch, Y, Fd)
    assert o.status == 0 and (o.err == fr.SINGULAR).all()
    Fn = F.copy()
    Fn[7, 0] = np.nan           # in the FIRST column: the later ones are not NaN by themselves
    o2 = fit(torch, Y, Fn)
    assert o2.status == 0 and not o2.err.any()
    Fn2 = F.copy()
    Fn2[7, 2] = np.nan          # in the LAST column: the basis' earlier columns stay finite
    o3 = fit(torch, Y, Fn2)
    assert o3.status == 0 and not o3.err.any()
    for r in (o, o2, o3):
        for name in ("beta", "se", "stats", "resid"):
            assert np.isnan(getattr(r, name)).all(), name


# ---- optional outputs ----

@pytest.mark.parametrize("T,k,mode", [(390, 3, "shared"), (390, 3, "per_series"), (1200, 8, "shared"), (2561, 1, "per_series")])
def test_optional_outputs(torch, T, k, mode):
    Y, F = fr.panel(800 + T, 7, T, k, per_series=(mode == "per_series"))
    full = fit(torch, Y, F)
    assert full.status == 0
    for drop in ("se", "stats", "resid", "err"):
        o = fit(torch, Y, F, **{drop: False})
        assert o.status == 0 and getattr(o, drop) is None
        for name in ("beta", "se", "stats", "resid", "err"):
            if name != drop:
                assert same(getattr(o, name), getattr(full, name)), (drop, name)
    o = fit(torch, Y, F, se=False, stats=False, resid=False, err=False)
    assert o.status == 0 and same(o.beta, full.beta)


# ---- layout ----

@pytest.mark.parametrize("poison", list(la.POISONS))
@pytest.mark.parametrize("lay", ["odd", "skew"])
@pytest.mark.parametrize("T,k,mode", [(65, 3, "shared"), (65, 3, "per_series"), (1098, 3, "shared"), (2561, 2, "per_series")])
def test_layout(torch, T, k, mode, lay, poison):
    """Padded ld, ld_r, ld_b, ld_f, an fs with slack and odd 8-byte-aligned bases: the packed call's
    bits, nothing outside the contract written, no input written, and (a NaN poison would reach a sum)
    nothing beyond row ends read."""
    S = 6
    pv = la.POISONS[poison]
    per = mode == "per_series"
    Y, F = fr.panel(1200 + T, S, T, k, per_series=per)
    packed = fit(torch, Y, F)
    assert packed.status == 0
    ld, ld_r, bi, bo = la.layout(lay, T)
    ld_f, ld_b = T + 3, k + 1 + 2
    ay = la.carve(S, T, ld, bi, pv, data=Y)
    fp = factor_panel(F)[0].reshape(-1, T)                        # (k, T) or (S k, T) rows
    af = la.carve(fp.shape[0] + (S if per else 0), T, ld_f, 3, pv)   # per series: k rows + one slack row each
    nrow = k + 1 if per else k
    for s in range(S if per else 1):
        af.view[s * nrow:s * nrow + k] = torch.as_tensor(fp[s * k:(s + 1) * k])
    fs = nrow * ld_f if per else 0
    ab, ase = la.carve(S, k + 1, ld_b, 1, la.OUT_FILL), la.carve(S, k + 1, ld_b, 1, la.OUT_FILL)
    ast, ar = la.carve(S, 4, 4, 5, la.OUT_FILL), la.carve(S, T, ld_r, bo, la.OUT_FILL)
    err = torch.full((S,), -7, dtype=torch.int32, device="cuda:0")
    ins, outs = [(a, a.snapshot()) for a in (ay, af)], [(a, a.snapshot()) for a in (ab, ase, ast, ar)]
    st = lib().sts_factor_ols(ay.ptr, S, T, ld, af.ptr, k, ld_f, fs, ab.ptr, ld_b, ase.ptr, ast.ptr, ar.ptr, ld_r, vp(err),
                              None)
    torch.cuda.synchronize()
    assert st == 0, lib().sts_last_error()
    for a, snap in ins:
        a.verify_all(snap)
    for a, snap in outs:
        a.verify_outside(snap)
    for a, name in ((ab, "beta"), (ase, "se"), (ast, "stats"), (ar, "resid")):
        assert same(a.data(), getattr(packed, name)), name
    assert not err.cpu().numpy().any()
    # the effects pair in the same arenas (out of place into the residual arena, then in place)
    beta = packed.beta
    for add in (False, True):
        fn = lib().sts_factor_add if add else lib().sts_factor_remove
        want = (fr.add if add else fr.remove)(Y, beta, F)
        snap = ar.snapshot()
        assert fn(ay.ptr, ar.ptr, S, T, ld, ld_r, af.ptr, k, ld_f, fs, ab.ptr, ld_b, None) == 0
        torch.cuda.synchronize()
        ar.verify_outside(snap)
        assert same(ar.data(), want)
    for a, snap in ins:
        a.verify_all(snap)
    snap = ay.snapshot()
    assert lib().sts_factor_remove(ay.ptr, ay.ptr, S, T, ld, ld, af.ptr, k, ld_f, fs, ab.ptr, ld_b, None) == 0
    torch.cuda.synchronize()
    ay.verify_outside(snap)
    assert same(ay.data(), fr.remove(Y, beta, F))


# ---- host path ----

@pytest.mark.parametrize("T,k,mode", [(390, 3, "shared"), (390, 3, "per_series"), (2561, 8, "shared")])
def test_host_path_has_the_device_bits(torch, T, k, mode):
    Y, F = fr.panel(1500 + T, 11, T, k, per_series=(mode == "per_series"))
    d, h = fit(torch, Y, F), fit(torch, Y, F, host=True)
    assert d.status == 0 and h.status == 0, lib().sts_last_error()
    for name in ("beta", "se", "stats", "resid", "err"):
        assert same(getattr(h, name), getattr(d, name)), name
    h2 = fit(torch, Y, F, host=True, se=False, resid=False, err=False)
    assert h2.status == 0 and same(h2.beta, d.beta) and same(h2.stats, d.stats)
    for add in (False, True):
        want = (fr.add if add else fr.remove)(Y, d.beta, F)
        assert same(effects(torch, add, Y, d.beta, F, host=True), want)
        assert same(effects(torch, add, Y, d.beta, F, host=True, inplace=True), want)


# ---- effects ----

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [1, 63, 64, 65, 2561])
def test_effects_are_bit_exact(torch, T, mode):
    """The shared element-parallel launcher does not slice its launches: S is chosen so that the panel
    takes several workgroups of 2048 elements with a partial last one."""
    k = 3
    S = 4099 if T == 1 else 67
    rng = np.random.RandomState(40 + T)
    F = rng.standard_normal((S, T, k) if mode == "per_series" else (T, k))
    X = rng.standard_normal((S, T)) * 10.0
    X[1, 0] = np.nan
    beta = rng.standard_normal((S, k + 1)) * np.array([100.0, 1.0, 1e-3, 1e3])
    rem = effects(torch, False, X, beta, F)
    assert same(rem, fr.remove(X, beta, F))
    assert same(effects(torch, True, X, beta, F), fr.add(X, beta, F))
    assert same(effects(torch, False, X, beta, F, inplace=True), rem)
    assert same(effects(torch, True, X, beta, F, inplace=True), fr.add(X, beta, F))
    back = effects(torch, True, rem, beta, F)
    fitv = fr.fit_values(beta, F)
    assert same(back, (X - fitv) + fitv)


# ---- stream order ----

def _gate_case(torch, which, v, per):
    S, T, k = 9, 129, 3
    gen = lambda seed: fr.panel(seed, S, T, k, per_series=per)
    trip = [gen(300 + v), gen(350 + v), gen(390 + v)]
    gy = sg.GIn(torch, *[t[0] for t in trip])
    gf = sg.GIn(torch, *[factor_panel(t[1])[0] for t in trip])
    fs = k * T if per else 0
    mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda:0")
    Y, F = trip[0]
    if which == "ols":
        beta, se, stats, resid = mk(S, k + 1), mk(S, k + 1), mk(S, 4), mk(S, T)
        err = torch.empty((S,), dtype=torch.int32, device="cuda:0")

        def call(st):
            return lib().sts_factor_ols(vp(gy.buf), S, T, T, vp(gf.buf), k, T, fs, vp(beta), k + 1, vp(se), vp(stats),
                                        vp(resid), T, vp(err), st)

        def check(outs, host):
            want = fr.ols_panel(Y, F)
            o = Out()
            o.beta, o.se, o.stats, o.resid = outs[:4]
            assert_fit(o, want, slice(None), "gated ols")
            assert not outs[4].any()
        return sg.Case([gy, gf], [beta, se, stats, resid, err], call, check)
    gb = sg.GIn(torch, *[fr.ols_panel(*t)[0] for t in trip])
    out = mk(S, T)
    fn = lib().sts_factor_add if which == "add" else lib().sts_factor_remove

    def call(st):
        return fn(vp(gy.buf), vp(out), S, T, T, T, vp(gf.buf), k, T, fs, vp(gb.buf), k + 1, st)

    def check(outs, host):
        beta = fr.ols_panel(Y, F)[0]
        assert same(outs[0], (fr.add if which == "add" else fr.remove)(Y, beta, F))
    return sg.Case([gy, gf, gb], [out], call, check)


@pytest.mark.parametrize("per", [False, True], ids=MODES)
@pytest.mark.parametrize("which", ["ols", "remove", "add"])
def test_gated_call_is_stream_ordered(torch, delay, which, per):
    """Every `void* stream` entry point of sts_regress.h behind a delayed stream (tests/stream_gate.py):
    the plain call's bits, nothing written late, and the call returned while the gate was shut."""
    case = _gate_case(torch, which, 0, per)
    st, res, host = sg.plain(torch, case)
    assert st == 0, lib().sts_last_error()
    case.check([r.cpu().numpy() for r in res], host)
    t = sg.enqueue(torch, case, torch.cuda.Stream(), delay)
    pending = t.pending_at_return
    late = sg.finish(torch, t)
    assert t.status == 0
    for i, (s, r) in enumerate(zip(t.snaps, res)):
        assert sg.same_bits(s, r), "%s: output %d of the gated call differs from the plain call" % (which, i)
    assert not late, late
    assert pending, "%s is expected to return before its work ran" % which


def test_every_stream_entry_point_is_gated():
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sts_regress.h")).read(), flags=re.S)
    names = sorted(m.group(1) for m in re.finditer(r"\bint\s+(sts_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
                   if re.search(r"void\s*\*\s*stream\s*$", m.group(2).strip()))
    assert names == ["sts_factor_add", "sts_factor_ols", "sts_factor_remove"]


def test_mirror_on_a_side_stream(torch, delay):
    """stats.ols and the model's effects on a non-default current stream, behind a delay: the plain
    call's bits, and the panel call returns while the gate is shut (it takes the status array)."""
    from sparkts import stats
    from sparkts.models import FactorRegressionModel
    trip = [fr.panel(s, 9, 390, 3) for s in (1, 2, 3)]
    g = sg.GIn(torch, *[t[0] for t in trip])
    Fd = dev(torch, trip[0][1])

    def run(x):
        r = stats.ols(x, Fd)
        m = FactorRegressionModel(r.coefficients, Fd)
        return [r.coefficients, r.standardErrors, r.rSquared, r.residuals.clone(), m.removeTimeDependentEffects(x)]

    g.buf.copy_(g.real)
    torch.cuda.synchronize()
    want = [t.cpu().numpy() for t in run(g.buf)]
    torch.cuda.synchronize()
    g.buf.copy_(g.decoy)
    torch.cuda.synchronize()
    stream, ev = torch.cuda.Stream(), torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(delay)
        ev.record(stream)
        g.buf.copy_(g.real, non_blocking=True)
        res = run(g.buf)
        shut_after = not ev.query()
        g.buf.copy_(g.decoy2, non_blocking=True)
        got = [t.cpu().numpy() for t in res]
    stream.synchronize()
    torch.cuda.synchronize()
    assert shut_after, "the mirror is expected to return without waiting for the device"
    for a, b in zip(got, want):
        assert same(a, b)
    ref = fr.ols_panel(*trip[0])
    assert fr.rel(want[0], ref[0]) <= fr.BAR and fr.resid_err(want[3], ref[3]) <= fr.BAR
    assert same(want[4], fr.remove(trip[0][0], want[0], trip[0][1]))


# ---- the mirror, end to end ----

def test_regress_then_bgtest_and_bptest_on_the_device(torch):
    """rdd.regress(F).residuals.bgtest(F, 5) / .bptest(F) agree with bgtest / bptest fed the
    restatement's residuals within t5 / t6's own bar (1e-10 relative on ordinary rows)."""
    from sparkts import stats
    from sparkts.timeseriesrdd import TimeSeriesRDD
    S, T, k = 12, 390, 3
    F = br.factors(5, T, k)
    e = br.bg_resid(6, S, T) * (1.0 + 1.5 * (F[:, 0] > 0))
    Y = fr.INTERCEPT + F @ fr.COEF[:k] + e
    Fd = dev(torch, F)
    rdd = TimeSeriesRDD("idx", ["k%d" % s for s in range(S)], dev(torch, Y))
    r = rdd.regress(Fd)
    assert isinstance(r.residuals, TimeSeriesRDD) and r.residuals.keys == rdd.keys and r.residuals.index == "idx"
    want = fr.ols_panel(Y, F)
    assert fr.rel(r.coefficients.cpu().numpy(), want[0]) <= fr.BAR
    assert fr.rel(r.standardErrors.cpu().numpy(), want[1]) <= fr.BAR
    assert fr.resid_err(r.residuals.data.cpu().numpy(), want[3]) <= fr.BAR
    assert not r.errors.cpu().numpy().any()
    n = float(T)
    adj = 1.0 - want[2][:, 0] * (n - 1.0) / (want[2][:, 1] * (n - k - 1.0))
    assert fr.rel(r.adjustedRSquared.cpu().numpy(), adj) <= fr.BAR
    assert fr.rel(r.regressionStandardError.cpu().numpy(), np.sqrt(want[2][:, 3])) <= fr.BAR
    assert fr.rel(r.tStatistics.cpu().numpy(), want[0] / want[1]) <= 2 * fr.BAR
    bg, bg_p = r.residuals.bgtest(Fd, 5)
    bp, bp_p = r.residuals.bptest(Fd)
    want_bg = np.array([br.bg_stat(row, F, 5) for row in want[3]])
    want_bp = np.array([br.bp_stat(row, F) for row in want[3]])
    assert fr.rel(bg.cpu().numpy(), want_bg) <= fr.BAR and fr.rel(bp.cpu().numpy(), want_bp) <= fr.BAR
    # one series, numpy (the host path): floats and 1-D arrays; no residuals when not asked for
    one = stats.ols(Y[0], F, residuals=False)
    assert one.residuals is None and isinstance(one.rSquared, float) and one.coefficients.shape == (k + 1,)
    assert fr.rel(one.coefficients, want[0][0]) <= fr.BAR and abs(one.rSquared - want[2][0, 2]) <= fr.BAR
    from sparkts.errors import SingularMatrixException
    with pytest.raises(SingularMatrixException):
        stats.ols(Y[0], np.column_stack([F[:, 0], F[:, 0]]))


def test_factor_regression_model(torch):
    from sparkts.models import FactorRegression, FactorRegressionModel
    Y, F = fr.panel(71, 5, 200, 2)
    Yd, Fd = dev(torch, Y), dev(torch, F)
    m = FactorRegression.fitModel(Yd, Fd)
    beta = m.coefficients.cpu().numpy()
    assert fr.rel(beta, fr.ols_panel(Y, F)[0]) <= fr.BAR
    assert same(m.removeTimeDependentEffects(Yd).cpu().numpy(), fr.remove(Y, beta, F))
    dest = Yd.clone()
    assert m.addTimeDependentEffects(dest, dest) is dest and same(dest.cpu().numpy(), fr.add(Y, beta, F))
    # one coefficient vector for the whole panel, out of sample, numpy (host path), one series
    Y2, F2 = fr.panel(72, 4, 50, 2)
    m2 = FactorRegressionModel(beta[0], F2)
    assert same(m2.removeTimeDependentEffects(Y2), fr.remove(Y2, beta[0], F2))
    assert same(m2.addTimeDependentEffects(Y2[1]), fr.add(Y2[1], beta[0], F2))
