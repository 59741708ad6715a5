"""include/sts_sample.h on an MI355X: bit-exact parity of the five entry points with the
restatement (tests/sample_ref.py), the shard / chunk identities of the stream, the launch shapes
only a very large S reaches, the panel-layout contract and the mirror.

The restatement is computed once per (t0, s0) at the largest shape (130 x 129): every sampler is
causal along time and independent across series, so the result of a smaller call is the block
[:S, :n] of the largest one -- which is itself one of the properties under test.
"""
import ctypes

import numpy as np
import pytest

import layout_arena as la
import oracle
import sample_ref as sr

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15               # both key words in use
SS = (1, 63, 64, 65, 130)               # a lane, a wave less one, a wave, a wave and one, two waves and two
NS = (1, 2, 3, 63, 64, 65, 129)         # below / at / above the kernel's 32-step chunk and the 64-step store row
T0S = (0, 1, 2 ** 33 + 1)               # odd: every Philox pair straddles the kernel's column pairs
S0S = (0, 7)
SMAX, NMAX = max(SS), max(NS)
COMBOS = [(t0, s0) for t0 in T0S for s0 in S0S]
SENT = -3.0e55
BAD_ARG = 1
BAD_ROW, NAN_ROW = 5, 40                # alpha + beta > 1; NaN omega: their wave neighbours stay bit-exact

ARIMA_ORDERS = [(0, 0, 1, 1), (0, 0, 1, 0), (2, 1, 2, 1), (2, 1, 2, 0), (4, 2, 4, 1), (4, 2, 4, 0)]   # p, d, q, intercept
AR_ORDERS = (1, 5)
_MEMO = {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


def L():
    from sparkts import _native
    return _native.lib()


def vp(t):
    return None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


# ---------------- models: per-series parameters (row s of a call takes row r0 + s) ----------------

def host_params(kind):
    """kind -> list of (SMAX, ...) arrays, fixed for the module"""
    def make():
        rng = np.random.default_rng(sum(map(ord, str(kind))))
        if kind == "normal":
            return []
        if kind in ("garch", "argarch"):
            om, al, be = rng.uniform(0.05, 0.3, SMAX), rng.uniform(0.05, 0.45, SMAX), rng.uniform(0.05, 0.45, SMAX)
            al[BAD_ROW], be[BAD_ROW] = 0.7, 0.6
            om[NAN_ROW] = np.nan
            if kind == "garch":
                return [om, al, be]
            return [rng.uniform(-1.0, 40.0, SMAX), rng.uniform(-0.6, 0.6, SMAX), om, al, be]
        if kind[0] == "ar":
            return [rng.uniform(-1.0, 1.0, SMAX), rng.uniform(-0.15, 0.15, (SMAX, kind[1]))]
        p, d, q, icpt = kind[1:]
        return [rng.uniform(-0.2, 0.2, (SMAX, icpt + p + q))]
    return memo(("params", kind), make)


def draws(t0, s0):
    """reference draws of global series s0 .. s0 + SMAX at positions t0 .. t0 + NMAX (one table per t0)"""
    allg = memo(("draws", t0), lambda: sr.normal_panel(SEED, 0, SMAX + max(S0S), t0, NMAX))
    return allg[s0:s0 + SMAX]


def reference(kind, t0, s0):
    def make():
        g, par = draws(t0, s0), host_params(kind)
        if kind == "normal":
            return g
        if kind == "garch":
            return np.array([sr.garch_sample(g[s], par[0][s], par[1][s], par[2][s]) for s in range(SMAX)])
        if kind == "argarch":
            return np.array([sr.garch_sample(g[s], par[2][s], par[3][s], par[4][s], par[0][s], par[1][s]) for s in range(SMAX)])
        if kind[0] == "ar":
            return np.array([sr.ar_sample(g[s], par[0][s], par[1][s]) for s in range(SMAX)])
        p, d, q, icpt = kind[1:]
        return np.array([sr.arima_sample(g[s], p, d, q, par[0][s], bool(icpt)) for s in range(SMAX)])
    return memo(("ref", kind, t0, s0), make)


def dev_params(torch, kind, r0, S):
    if kind == "normal":
        return []
    return [dev(torch, a[r0:r0 + S]) for a in host_params(kind)]


def call(torch, kind, out_ptr, s0, S, n, ld, t0, r0=0, seed=SEED, par=None):
    """the entry point of `kind` on rows r0 .. r0 + S of the module's parameters -> status"""
    par = dev_params(torch, kind, r0, S) if par is None else par
    tail = (t0, ctypes.c_uint64(seed), None)
    o = vp(out_ptr)
    if kind == "normal":
        return L().sts_sample_normal(o, s0, S, n, ld, *tail)
    if kind == "garch":
        return L().sts_garch_sample(o, s0, S, n, ld, *[vp(x) for x in par], *tail)
    if kind == "argarch":
        return L().sts_argarch_sample(o, s0, S, n, ld, *[vp(x) for x in par], *tail)
    if kind[0] == "ar":
        return L().sts_ar_sample(o, s0, S, n, ld, vp(par[0]), vp(par[1]), kind[1], *tail)
    p, d, q, icpt = kind[1:]
    return L().sts_arima_sample(o, s0, S, n, ld, p, d, q, icpt, vp(par[0]), *tail)


def ok(st):
    assert st == 0, (st, L().sts_last_error())


def run(torch, kind, s0, S, n, t0, r0=0):
    out = torch.full((S, n), SENT, dtype=torch.float64, device="cuda:0")
    ok(call(torch, kind, out, s0, S, n, n, t0, r0))
    torch.cuda.synchronize()
    return out.cpu().numpy()


KINDS = ["normal", "garch", "argarch"] + [("ar", p) for p in AR_ORDERS]
kid = lambda k: k if isinstance(k, str) else "-".join(map(str, k))


# ---------------- parity ----------------

def check_shapes(torch, kind, t0, s0):
    want = reference(kind, t0, s0)
    d = kind[2] if kind[0] == "arima" else 0
    for S in SS:
        for n in NS:
            what = "%s S=%d n=%d t0=%d s0=%d" % (kid(kind), S, n, t0, s0)
            if n < d:      # sts_arima_add's rule: d within [0, n]; nothing is written
                out = torch.full((S, n), SENT, dtype=torch.float64, device="cuda:0")
                assert call(torch, kind, out, s0, S, n, n, t0) == BAD_ARG, what
                assert bool((out == SENT).all()), what
                continue
            got = run(torch, kind, s0, S, n, t0)
            sr.assert_bits(got, want[:S, :n], what)
            if kind in ("garch", "argarch"):
                assert not np.signbit(got[:, 0]).any() and (got[:, 0] == 0.0).all(), what     # +0.0, NaN rows too


@pytest.mark.parametrize("t0,s0", COMBOS)
@pytest.mark.parametrize("kind", KINDS, ids=kid)
def test_parity(torch, kind, t0, s0):
    check_shapes(torch, kind, t0, s0)


@pytest.mark.parametrize("i", range(len(ARIMA_ORDERS)), ids=lambda i: "%d-%d-%d-icpt%d" % ARIMA_ORDERS[i])
def test_parity_arima(torch, i):
    """every order on every shape, each at one of the six (t0, s0): the restatement is pure Python"""
    check_shapes(torch, ("arima",) + ARIMA_ORDERS[i], *COMBOS[i])


def test_poisoned_series_sit_where_the_reference_has_them(torch):
    """alpha + beta > 1 gives h_0 < 0: NaN from step 1 on; a NaN omega likewise; their neighbours are
    ordinary series (and bit-exact: test_parity)"""
    for kind in ("garch", "argarch"):
        want = reference(kind, 1, 7)
        got = run(torch, kind, 7, SMAX, NMAX, 1)
        for r in (BAD_ROW, NAN_ROW):
            assert got[r, 0] == 0.0 and np.isnan(got[r, 1:]).all() and np.isnan(want[r, 1:]).all()
            assert np.isfinite(got[[r - 1, r + 1]]).all()


# ---------------- shard and chunk identities ----------------

ALL_KINDS = KINDS + [("arima",) + ARIMA_ORDERS[2]]


@pytest.mark.parametrize("kind", ALL_KINDS, ids=kid)
def test_shards_stack(torch, kind):
    """(s0 = 0, S = 130) is (0, 64) stacked on (64, 66): a shard regenerates its rows anywhere"""
    n, t0 = 65, 1
    whole = run(torch, kind, 0, 130, n, t0)
    parts = np.concatenate([run(torch, kind, 0, 64, n, t0), run(torch, kind, 64, 66, n, t0, r0=64)])
    sr.assert_bits(parts, whole, "shards of %s" % kid(kind))


@pytest.mark.parametrize("t0", T0S)
def test_chunks_join(torch, t0):
    """[t0, t0 + 129) is [t0, t0 + 64) followed by [t0 + 64, t0 + 129)"""
    whole = run(torch, "normal", 7, 65, 129, t0)
    halves = np.concatenate([run(torch, "normal", 7, 65, 64, t0), run(torch, "normal", 7, 65, 65, t0 + 64)], axis=1)
    sr.assert_bits(halves, whole, "chunks at t0=%d" % t0)


# ---------------- the mirror ----------------

def test_generator_advances(torch):
    """two calls on one generator: two different panels, the reference at positions 0 and n"""
    from sparkts.models import GARCHModel
    from sparkts.random import PhiloxGenerator
    n, P, first = 65, 9, 7
    gen = PhiloxGenerator(SEED, first_series=first)
    m = GARCHModel(.2, .3, .4)
    a, b = m.sample(n, gen, paths=P), m.sample(n, gen, paths=P)
    assert tuple(a.shape) == tuple(b.shape) == (P, n) and a.is_cuda and gen.position == 2 * n
    raw = gen.normal(P, n, device="cuda:0")
    assert gen.position == 3 * n
    a, b, raw = a.cpu().numpy(), b.cpu().numpy(), raw.cpu().numpy()
    assert not np.array_equal(a[:, 1:], b[:, 1:])
    for k, got in enumerate((a, b)):
        g = sr.normal_panel(SEED, first, P, k * n, n)
        sr.assert_bits(got, np.array([sr.garch_sample(g[j], .2, .3, .4) for j in range(P)]), "call %d" % k)
    sr.assert_bits(raw, sr.normal_panel(SEED, first, P, 2 * n, n), "PhiloxGenerator.normal")


def test_mirror_shapes_and_values(torch):
    from sparkts.models import ARGARCHModel, ARIMAModel, ARModel, GARCHModel
    from sparkts.random import PhiloxGenerator
    n, S = 33, 6
    g1 = sr.normal_panel(11, 3, S, 0, n)
    # scalar parameters -> (n,)
    y = ARGARCHModel(40.0, .4, .2, .3, .4).sample(n, PhiloxGenerator(11, 3))
    assert tuple(y.shape) == (n,)
    sr.assert_bits(y.cpu().numpy(), sr.garch_sample(g1[0], .2, .3, .4, 40.0, .4), "ARGARCHModel scalar")
    y = ARModel(1.5, [.5, -.2, .1]).sample(n, PhiloxGenerator(11, 3), paths=S)
    assert tuple(y.shape) == (S, n)
    sr.assert_bits(y.cpu().numpy(), np.array([sr.ar_sample(g1[j], 1.5, [.5, -.2, .1]) for j in range(S)]), "ARModel paths")
    # per-series parameters -> (S, n), device tensors or host arrays
    om, al, be = host_params("garch")
    y = GARCHModel(dev(torch, om[:S]), al[:S], be[:S]).sample(n, PhiloxGenerator(11, 3))
    assert tuple(y.shape) == (S, n)
    sr.assert_bits(y.cpu().numpy(), np.array([sr.garch_sample(g1[j], om[j], al[j], be[j]) for j in range(S)]), "GARCHModel panel")
    coef = host_params(("arima", 2, 1, 2, 1))[0][:S]
    y = ARIMAModel(2, 1, 2, dev(torch, coef), True).sample(n, PhiloxGenerator(11, 3))
    assert tuple(y.shape) == (S, n)
    sr.assert_bits(y.cpu().numpy(), np.array([sr.arima_sample(g1[j], 2, 1, 2, coef[j], True) for j in range(S)]), "ARIMAModel panel")
    y = ARIMAModel(0, 0, 1, [0.4], False).sample(n, PhiloxGenerator(11, 3))
    assert tuple(y.shape) == (n,)
    sr.assert_bits(y.cpu().numpy(), sr.arima_sample(g1[0], 0, 0, 1, [0.4], False), "ARIMAModel scalar")
    with pytest.raises(ValueError, match="paths"):
        GARCHModel(dev(torch, om[:S]), .3, .4).sample(n, PhiloxGenerator(1), paths=3)


def test_sample_then_fit_round_trip(torch):
    """GARCHModel(.2, .3, .4).sample(10000, rand, paths = 64) -> GARCH.fitModel, as GARCHSuite's "fit
    model" (GARCHSuite.scala:57-71).  The suite's own assertions are one-sided (model.omega - omega <
    .1, model.alpha - alpha < .02, model.beta - beta < .02) and are applied to the mean of the 64 fits
    as they stand.  Read two-sided they fail on the REFERENCE: run through the oracle on the CPU
    (sample_ref paths, oracle.garch_fit) the 64 fits of this seed average omega 0.2401, alpha 0.2566,
    beta 0.3588 with standard deviations 0.0086, 0.0035, 0.0175 -- commons-math3's optimizer stops
    there for every path, since GARCHModel.gradient orders its components (alpha, beta, omega) while
    the point is (omega, alpha, beta) -- so no seed brings |alpha - 0.3| under 0.02.  What ties the
    device to the reference exactly: the first paths' fits have the oracle's bits."""
    from sparkts.models import GARCH, GARCHModel
    from sparkts.random import PhiloxGenerator
    n, P, seed = 10000, 64, 5
    panel = GARCHModel(.2, .3, .4).sample(n, PhiloxGenerator(seed), paths=P)
    assert tuple(panel.shape) == (P, n) and bool((panel[:, 0] == 0.0).all())
    fit = GARCH.fitModel(panel)
    par = np.stack([fit.omega.cpu().numpy(), fit.alpha.cpu().numpy(), fit.beta.cpu().numpy()], axis=1)
    mean = par.mean(axis=0)
    print("mean of %d fits: omega %.4f alpha %.4f beta %.4f" % (P, *mean))
    assert np.isfinite(par).all()
    assert mean[0] - .2 < .1 and mean[1] - .3 < .02 and mean[2] - .4 < .02
    assert np.abs(mean - np.array([0.2401, 0.2566, 0.3588])).max() < 2e-3        # the oracle's means above
    g = sr.normal_panel(seed, 0, 2, 0, n)
    got = panel[:2].cpu().numpy()
    for j in range(2):
        ts = sr.garch_sample(g[j], .2, .3, .4)
        sr.assert_bits(got[j], ts, "path %d" % j)
        st, rpar, _ = oracle.garch_fit(ts)
        assert st == 0
        sr.assert_bits(par[j], rpar, "fit of path %d" % j)


# ---------------- launch shapes of a very large S ----------------

@pytest.mark.parametrize("S", [65537, 64 * 65535 + 1])
def test_large_S(torch, S):
    """more series than a grid dimension's 65 535 (x 64 lanes): the kernels index by blockIdx.x alone, in
    64-bit arithmetic.  n = 3 keeps the panel at 1.6 / 101 MB; the first, last and boundary series against
    the restatement, every element written."""
    n, t0, s0 = 3, 2 ** 33 + 1, 7
    rows = sorted({0, 1, 63, 64, 65534, 65535, 65536, S - 2, S - 1} | ({64 * 65535 - 1, 64 * 65535} if S > 64 * 65535 else set()))
    g = sr.normals(SEED, (np.array(rows, dtype=np.uint64) + np.uint64(s0))[:, None],
                   (np.arange(n, dtype=np.uint64) + np.uint64(t0))[None, :])
    om = torch.full((S,), .2, dtype=torch.float64, device="cuda:0")
    al, be = torch.full_like(om, .3), torch.full_like(om, .4)
    c, phi = torch.full_like(om, 40.0), torch.full_like(om, .4)
    out = torch.full((S, n), SENT, dtype=torch.float64, device="cuda:0")
    idx = torch.as_tensor(rows, device="cuda:0")
    for kind, par, ref in (("normal", [], lambda r: r),
                           ("garch", [om, al, be], lambda r: sr.garch_sample(r, .2, .3, .4)),
                           ("argarch", [c, phi, om, al, be], lambda r: sr.garch_sample(r, .2, .3, .4, 40.0, .4))):
        out.fill_(SENT)
        ok(call(torch, kind, out, s0, S, n, n, t0, par=par))
        torch.cuda.synchronize()
        assert not bool((out == SENT).any()), kind
        sr.assert_bits(out[idx].cpu().numpy(), np.array([ref(r) for r in g]), "%s S=%d" % (kind, S))
    del out, om, al, be, c, phi
    torch.cuda.empty_cache()


# ---------------- the layout contract ----------------

@pytest.mark.parametrize("poison", sorted(la.POISONS))
@pytest.mark.parametrize("lay", la.LAYOUT_NAMES)
def test_layouts(torch, lay, poison):
    """ld > n, an odd 8-byte base, rows at every offset inside a 128-B line: the block (s, i < n) has the
    restatement's bits, and the padding, the skew and the red zones keep theirs"""
    S, n, t0, s0 = 65, 65, 1, 7
    _, ld, _, base = la.layout(lay, n)
    for kind in ALL_KINDS:
        a = la.carve(S, n, ld, base, la.POISONS[poison])
        snap = a.snapshot()
        ok(call(torch, kind, a.ptr, s0, S, n, ld, t0))
        torch.cuda.synchronize()
        what = "%s %s %s" % (kid(kind), lay, poison)
        a.verify_outside(snap, what)
        sr.assert_bits(a.data(), reference(kind, t0, s0)[:S, :n], what)
