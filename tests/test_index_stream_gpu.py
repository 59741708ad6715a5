"""The stream contract of include/sts.h on the entry points of include/sts_index.h, which takes it
over verbatim: one gated row per entry point whose last parameter is `void* stream`, on the gate of
tests/stream_gate.py, run exactly as tests/test_transforms_stream_gpu.py runs its rows.  Needs an
MI355X.

Every row's snapshots must be bit-identical to the same call made plainly, whose result in turn is
the restatement's (tests/index_ref.py), every output must hold the sentinel afterwards, and the call
must return while the gate is still shut: no entry point of this header waits.
tests/test_index_cpu.py checks that no stream entry point of the header lacks a row.
"""
import numpy as np
import pytest

import index_ref as ir
import stream_gate as sg
from stream_gate import Case, vp

pytestmark = pytest.mark.gpu

S, T_IN, T_OUT = 13, 390, 401
DEFAULT = 47.0
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


def panel(k):
    return memo(("panel", k), lambda: ir.hard_panel(S, T_IN, 7000 + k))


def gin(torch, v):
    return sg.GIn(torch, panel(v), panel(50 + v), panel(90 + v))


def out(torch, shape, dtype=None):
    return torch.empty(shape, dtype=dtype or torch.float64, device="cuda:0")


def a_map(k):
    rng = np.random.default_rng(300 + k)
    return np.where(rng.random(T_OUT) < 0.2, -1, rng.integers(0, T_IN + 4, size=T_OUT)).astype(np.int64)


BDAYS = (ir.millis("2015-04-06") + 9 * ir.H, 300, ("businessDays", 2))


def some_instants(k):
    rng = np.random.default_rng(500 + k)
    return np.sort(rng.integers(-10 ** 12, 10 ** 12, size=T_IN)).astype(np.int64)


def some_queries(k, instants):
    rng = np.random.default_rng(600 + k)
    pick = np.asarray(instants, dtype=np.int64)[rng.integers(0, len(instants), size=T_OUT)]
    return pick + rng.integers(0, 2, size=T_OUT) * rng.integers(-1, 2, size=T_OUT)


TABLE = []      # (id, entry points covered, build(torch, v) -> Case)


def row(ident, *covers):
    def deco(build):
        TABLE.append((ident, covers, build))
        return build
    return deco


@row("rebase_shift-even", "sts_rebase_shift")
def _b(torch, v):
    g, o = gin(torch, v), out(torch, (S, T_OUT))

    def check(outs, host):
        ir.assert_bits(outs[0], ir.gather_panel(panel(v), ir.shift_map(T_IN, T_OUT, -4), DEFAULT), "shift -4")
    return Case([g], [o], lambda st: L().sts_rebase_shift(vp(g.buf), vp(o), S, T_IN, T_OUT, T_IN, T_OUT, -4, DEFAULT, st), check)


@row("rebase_shift-odd", "sts_rebase_shift")
def _b(torch, v):
    g, o = gin(torch, v), out(torch, (S, T_OUT))

    def check(outs, host):
        ir.assert_bits(outs[0], ir.gather_panel(panel(v), ir.shift_map(T_IN, T_OUT, 3), DEFAULT), "shift 3")
    return Case([g], [o], lambda st: L().sts_rebase_shift(vp(g.buf), vp(o), S, T_IN, T_OUT, T_IN, T_OUT, 3, DEFAULT, st), check)


@row("rebase_map", "sts_rebase_map")
def _b(torch, v):
    g, o = gin(torch, v), out(torch, (S, T_OUT))
    m = sg.GIn(torch, a_map(v), a_map(50 + v), a_map(90 + v), dtype=np.int64)

    def check(outs, host):
        ir.assert_bits(outs[0], ir.gather_panel(panel(v), a_map(v), DEFAULT), "map")
    return Case([g, m], [o], lambda st: L().sts_rebase_map(vp(g.buf), vp(o), S, T_IN, T_OUT, T_IN, T_OUT, vp(m.buf),
                                                           DEFAULT, st), check)


@row("align_uniform", "sts_align_uniform")
def _b(torch, v):
    lengths = [0, 100, 1, 390, 64, 0, 7]
    offsets = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    n = int(offsets[-1])
    flat = lambda k: panel(k).reshape(-1)[:n]
    starts = lambda k: np.array([0, -3 + k, 0, 5, -60, 2, 1 - k], dtype=np.int64)
    vals = sg.GIn(torch, flat(v), flat(50 + v), flat(90 + v))
    sl = sg.GIn(torch, starts(v), starts(5 + v), starts(9 + v), dtype=np.int64)
    off = sg.dev(torch, offsets, np.int64)
    o = out(torch, (len(lengths), T_OUT))

    def check(outs, host):
        for s in range(len(lengths)):
            r = flat(v)[offsets[s]:offsets[s + 1]]
            ir.assert_bits(outs[0][s], ir.gather(r, ir.shift_map(len(r), T_OUT, int(starts(v)[s])), DEFAULT), "align %d" % s)
    return Case([vals, sl], [o], lambda st: L().sts_align_uniform(vp(vals.buf), vp(off), vp(sl.buf), len(lengths), T_OUT,
                                                                  vp(o), T_OUT, DEFAULT, st), check)


@row("index_instants-uniform", "sts_index_instants")
def _b(torch, v):
    o = out(torch, (BDAYS[1],), torch.int64)

    def check(outs, host):
        assert outs[0].tolist() == ir.u_instants(BDAYS)
    return Case([], [o], lambda st: L().sts_index_instants(2, BDAYS[0], BDAYS[1], BDAYS[2][1], None, 0, vp(o), st), check)


@row("index_instants-irregular", "sts_index_instants")
def _b(torch, v):
    g = sg.GIn(torch, some_instants(v), some_instants(50 + v), some_instants(90 + v), dtype=np.int64)
    o = out(torch, (T_IN,), torch.int64)

    def check(outs, host):
        assert np.array_equal(outs[0], some_instants(v))
    return Case([g], [o], lambda st: L().sts_index_instants(3, 0, 0, 1, vp(g.buf), T_IN, vp(o), st), check)


@row("index_locs-uniform", "sts_index_locs")
def _b(torch, v):
    inst = ir.u_instants(BDAYS)
    q = sg.GIn(torch, some_queries(v, inst), some_queries(50 + v, inst), some_queries(90 + v, inst), dtype=np.int64)
    o = out(torch, (T_OUT,), torch.int64)

    def check(outs, host):
        assert outs[0].tolist() == [ir.u_loc(BDAYS, int(t)) for t in some_queries(v, inst)]
    return Case([q], [o], lambda st: L().sts_index_locs(vp(q.buf), T_OUT, 2, BDAYS[0], BDAYS[1], BDAYS[2][1], None, 0,
                                                        vp(o), st), check)


@row("index_locs-irregular", "sts_index_locs")
def _b(torch, v):
    g = sg.GIn(torch, some_instants(v), some_instants(50 + v), some_instants(90 + v), dtype=np.int64)
    q = sg.GIn(torch, some_queries(v, some_instants(v)), some_queries(50 + v, some_instants(50 + v)),
               some_queries(90 + v, some_instants(90 + v)), dtype=np.int64)
    o = out(torch, (T_OUT,), torch.int64)

    def check(outs, host):
        inst = some_instants(v).tolist()
        assert outs[0].tolist() == [ir.i_loc(inst, int(t)) for t in some_queries(v, some_instants(v))]
    return Case([g, q], [o], lambda st: L().sts_index_locs(vp(q.buf), T_OUT, 3, 0, 0, 1, vp(g.buf), T_IN, vp(o), st), check)


IDS = [t[0] for t in TABLE]


def build(ident, torch, v):
    return next(t[2] for t in TABLE if t[0] == ident)(torch, v)


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
    assert pending, "%s is expected to be asynchronous but returned after the delay had run out" % ident


@pytest.mark.parametrize("ident", ["rebase_map", "index_locs-irregular"])
def test_two_streams(torch, delay, ident):
    """two calls on two streams in flight together"""
    a, b = build(ident, torch, 0), build(ident, torch, 1)
    ra, ha = run_plain(torch, a, ident + " [a]")
    rb, hb = run_plain(torch, b, ident + " [b]")
    ta = sg.enqueue(torch, a, torch.cuda.Stream(), delay)
    tb = sg.enqueue(torch, b, torch.cuda.Stream(), delay)
    assert_ticket(torch, ta, ra, ha, ident + " [a]")
    assert_ticket(torch, tb, rb, hb, ident + " [b]")
