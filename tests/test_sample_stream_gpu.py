"""The stream contract of include/sts.h on the entry points of include/sts_sample.h, which takes it
over verbatim: one gated row per entry point on the gate of tests/stream_gate.py, run as
tests/test_transforms_stream_gpu.py runs its rows.  Needs an MI355X.

Every row's snapshot must be bit-identical to the same call made plainly, whose result in turn is
the restatement's (tests/sample_ref.py); the output must hold the sentinel afterwards; and the
call must return while the gate is still shut: no entry point here takes err_per_series, so none
may wait.  The gated inputs are the per-series parameter arrays (decoys: other valid models);
sts_sample_normal has no input and is caught running early by the sentinel written behind the gate.
tests/test_sample_cpu.py checks that no entry point of the header lacks a row.
"""
import ctypes

import numpy as np
import pytest

import sample_ref as sr
import stream_gate as sg
from stream_gate import Case, vp

pytestmark = pytest.mark.gpu

S, N = 13, 390          # the C2 row length; 13 series: one partly filled wave
S0, T0, SEED = 7, 2 ** 33 + 1, 0x5EED5EED5EED
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


@pytest.fixture(scope="module")
def delay(torch):
    return sg.calibrate(torch)[0]


def L():
    from sparkts import _native
    return _native.lib()


def draws(v):
    """the call's draws; v moves the seed so the two calls of a two-stream case differ"""
    return memo(("draws", v), lambda: sr.normal_panel(SEED + v, S0, S, T0, N))


def params(k, width=None, lo=0.05, hi=0.3):
    """a valid per-series parameter array (seeded by k): values in [lo, hi)"""
    rng = np.random.default_rng(7000 + k)
    return rng.uniform(lo, hi, (S,) if width is None else (S, width))


def gparams(torch, k, **kw):
    return sg.GIn(torch, params(k, **kw), params(100 + k, **kw), params(200 + k, **kw))


def out(torch):
    return torch.empty((S, N), dtype=torch.float64, device="cuda:0")


def tail(v, st):
    return (T0, ctypes.c_uint64(SEED + v), st)


TABLE = []      # (id, entry points covered, build(torch, v) -> Case, sync)


def row(ident, *covers, sync=None):
    def deco(build):
        TABLE.append((ident, covers, build, sync))
        return build
    return deco


@row("sample_normal", "sts_sample_normal")
def _b(torch, v):
    o = out(torch)

    def check(outs, host):
        sr.assert_bits(outs[0], draws(v), "sample_normal")
    return Case([], [o], lambda st: L().sts_sample_normal(vp(o), S0, S, N, N, *tail(v, st)), check)


@row("garch_sample", "sts_garch_sample")
def _b(torch, v):
    g = [gparams(torch, 10 * v + j) for j in range(3)]
    o = out(torch)
    want = memo(("garch", v), lambda: np.array([sr.garch_sample(draws(v)[s], *(params(10 * v + j)[s] for j in range(3)))
                                                for s in range(S)]))

    def check(outs, host):
        sr.assert_bits(outs[0], want, "garch_sample")
    return Case(g, [o], lambda st: L().sts_garch_sample(vp(o), S0, S, N, N, *[vp(x.buf) for x in g], *tail(v, st)), check)


@row("argarch_sample", "sts_argarch_sample")
def _b(torch, v):
    g = [gparams(torch, 10 * v + j) for j in range(5)]          # c, phi, omega, alpha, beta
    o = out(torch)

    def ref():
        c, phi, om, al, be = (params(10 * v + j) for j in range(5))
        return np.array([sr.garch_sample(draws(v)[s], om[s], al[s], be[s], c[s], phi[s]) for s in range(S)])
    want = memo(("argarch", v), ref)

    def check(outs, host):
        sr.assert_bits(outs[0], want, "argarch_sample")
    return Case(g, [o], lambda st: L().sts_argarch_sample(vp(o), S0, S, N, N, *[vp(x.buf) for x in g], *tail(v, st)), check)


@row("ar_sample", "sts_ar_sample")
def _b(torch, v):
    p = 5
    gc, gf = gparams(torch, 10 * v), gparams(torch, 10 * v + 1, width=p, lo=-0.15, hi=0.15)
    o = out(torch)
    want = memo(("ar", v), lambda: np.array([sr.ar_sample(draws(v)[s], params(10 * v)[s],
                                                          params(10 * v + 1, width=p, lo=-0.15, hi=0.15)[s])
                                             for s in range(S)]))

    def check(outs, host):
        sr.assert_bits(outs[0], want, "ar_sample")
    return Case([gc, gf], [o], lambda st: L().sts_ar_sample(vp(o), S0, S, N, N, vp(gc.buf), vp(gf.buf), p, *tail(v, st)),
                check)


@row("arima_sample", "sts_arima_sample")      # the draws, the ARMA pass and two integration sweeps on one stream
def _b(torch, v):
    p, d, q = 2, 2, 2
    kw = dict(width=1 + p + q, lo=-0.2, hi=0.2)
    gf = gparams(torch, 10 * v + 2, **kw)
    o = out(torch)
    want = memo(("arima", v), lambda: np.array([sr.arima_sample(draws(v)[s], p, d, q, params(10 * v + 2, **kw)[s], True)
                                                for s in range(S)]))

    def check(outs, host):
        sr.assert_bits(outs[0], want, "arima_sample")
    return Case([gf], [o], lambda st: L().sts_arima_sample(vp(o), S0, S, N, N, p, d, q, 1, vp(gf.buf), *tail(v, st)), check)


IDS = [t[0] for t in TABLE]
SYNC = {t[0]: t[3] for t in TABLE if t[3] is not None}
ASYNC = sorted({name for t in TABLE if t[3] is None for name in t[1]})


def build(ident, torch, v):
    case = next(t[2] for t in TABLE if t[0] == ident)(torch, v)
    case.sync = SYNC.get(ident)
    return case


def run_plain(torch, case, what):
    st, res, host = sg.plain(torch, case)
    assert st == case.status, (what, st, L().sts_last_error())
    case.check([t.cpu().numpy() for t in res], host)
    return res, host


def assert_ticket(torch, t, res, host, what):
    late = sg.finish(torch, t)
    assert t.status == t.case.status, (what, t.status, L().sts_last_error())
    for i, (s, r) in enumerate(zip(t.snaps, res)):
        assert sg.same_bits(s, r), "%s: output %d of the gated call differs from the plain call" % (what, i)
    assert not late, "%s: outputs %s were written after the snapshot" % (what, late)


@pytest.mark.parametrize("ident", IDS)
def test_gated_call_is_stream_ordered(torch, delay, ident):
    case = build(ident, torch, 0)
    res, host = run_plain(torch, case, ident)
    t = sg.enqueue(torch, case, torch.cuda.Stream(), delay)
    pending = t.pending_at_return
    assert_ticket(torch, t, res, host, ident)
    print("%s: returned %s the gate opened" % (ident, "before" if pending else "after"))
    assert pending, "%s is expected to be asynchronous but returned after the delay had run out" % ident


@pytest.mark.parametrize("ident", ["ar_sample", "arima_sample"])
def test_two_streams(torch, delay, ident):
    """the rows of more than one launch, two calls on two streams in flight together"""
    a, b = build(ident, torch, 0), build(ident, torch, 1)
    ra, ha = run_plain(torch, a, ident + " [a]")
    rb, hb = run_plain(torch, b, ident + " [b]")
    ta = sg.enqueue(torch, a, torch.cuda.Stream(), delay)
    tb = sg.enqueue(torch, b, torch.cuda.Stream(), delay)
    assert_ticket(torch, ta, ra, ha, ident + " [a]")
    assert_ticket(torch, tb, rb, hb, ident + " [b]")
