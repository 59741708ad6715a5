"""The stream contract of include/sts.h on the entry points of include/sts_transforms.h, which
takes it over verbatim: one gated row per entry point whose last parameter is `void* stream`, on the
gate of tests/stream_gate.py, run exactly as tests/test_stream_order_gpu.py runs its rows (same
helpers).  Needs an MI355X.

Every row's snapshots must be bit-identical to the same call made plainly, whose result in turn is
the restatement's (tests/transforms_ref.py), every output must hold the sentinel afterwards, and
the call must return while the gate is still shut.  The one exception is listed in SYNC with its
reason: sts_fill_quotients given err_per_series == NULL waits in ErrSink::finish().
tests/test_transforms_cpu.py checks that no stream entry point of the header lacks a row.
"""
import numpy as np
import pytest

import stream_gate as sg
import transforms_ref as tr
from stream_gate import Case, vp

pytestmark = pytest.mark.gpu

S, T = 13, 390          # one row of every kind of tr.hard_panel, the C2 row length
SYNC_NULL_ERR = ("err_per_series == NULL: ErrSink::finish() synchronises (sts_api.cpp, 'wait and turn the first "
                 "failing series into a status')")
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
    return memo(("panel", k), lambda: tr.hard_panel(S, T, 4000 + k))


def gin(torch, v):
    """the gated input panel: real = panel(v), decoys from other seeds (same kinds of rows)"""
    return sg.GIn(torch, panel(v), panel(50 + v), panel(90 + v))


def out(torch, shape, dtype=None):
    return torch.empty(shape, dtype=dtype or torch.float64, device="cuda:0")


TABLE = []      # (id, entry points covered, build(torch, v) -> Case, sync)


def row(ident, *covers, sync=None):
    def deco(build):
        TABLE.append((ident, covers, build, sync))
        return build
    return deco


def simple(ident, name, width, args, ref):
    """a row of a panel -> panel entry point: name(in, out, S, T, ld_in, ld_out, *args, stream)"""
    @row(ident, name)
    def _b(torch, v):
        g = gin(torch, v)
        o = out(torch, (S, width))
        want = memo((ident, v), lambda: ref(panel(v)))

        def check(outs, host):
            tr.assert_bits(outs[0], want, ident)
        return Case([g], [o], lambda st: getattr(L(), name)(vp(g.buf), vp(o), S, T, T, width, *args, st), check)


simple("quotients", "sts_quotients", T - 5, (5, 0), lambda x: tr.quotients(x, 5))
simple("fill_with_default", "sts_fill_with_default", T, (-2.5,), lambda x: tr.fill_with_default(x, -2.5))
simple("downsample", "sts_downsample", (T - 2 + 6) // 7, (7, 2), lambda x: tr.downsample(x, 7, 2))
simple("upsample", "sts_upsample", 3 * T, (3, 2, 0), lambda x: tr.upsample(x, 3, 2))
simple("inverse_diff_at_lag-5", "sts_inverse_diff_at_lag", T, (5, 8), lambda x: tr.inverse_differences_at_lag(x, 5, 8))
simple("inverse_diff_at_lag-40", "sts_inverse_diff_at_lag", T, (40, 40), lambda x: tr.inverse_differences_at_lag(x, 40))
simple("diff_order_d-5", "sts_diff_order_d", T, (5,), lambda x: tr.differences_of_order_d(x, 5))
simple("diff_order_d-9", "sts_diff_order_d", T, (9,), lambda x: tr.differences_of_order_d(x, 9))        # sweeps + scratch
simple("inverse_diff_order_d-5", "sts_inverse_diff_order_d", T, (5,), lambda x: tr.inverse_differences_of_order_d(x, 5))
simple("inverse_diff_order_d-9", "sts_inverse_diff_order_d", T, (9,), lambda x: tr.inverse_differences_of_order_d(x, 9))


@row("first_last_not_nan", "sts_first_last_not_nan")
def _b(torch, v):
    g = gin(torch, v)
    f, l = out(torch, (S,), torch.int64), out(torch, (S,), torch.int64)

    def check(outs, host):
        assert np.array_equal(outs[0], tr.first_not_nan(panel(v))) and np.array_equal(outs[1], tr.last_not_nan(panel(v)))
    return Case([g], [f, l], lambda st: L().sts_first_last_not_nan(vp(g.buf), S, T, T, vp(f), vp(l), st), check)


def fill_quotients(ident, method, lag, null_err):
    """previous / lag 1: the one-pass kernel; linear: fill into stream-ordered scratch, then quotients"""
    @row(ident, "sts_fill_quotients", sync=SYNC_NULL_ERR if null_err else None)
    def _b(torch, v):
        g = gin(torch, v)
        w = T - lag
        o, e = out(torch, (S, w)), out(torch, (S,), torch.int32)

        def want():
            # the filled panel from sts_fill itself (plainly, synchronised), the quotients restated
            x = torch.as_tensor(panel(v), device="cuda:0")
            f, fe = torch.empty_like(x), torch.zeros(S, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            assert L().sts_fill(vp(x), vp(f), S, T, T, T, method, vp(fe), None) == 0
            torch.cuda.synchronize()
            return tr.quotients(f.cpu().numpy(), lag, True), fe.cpu().numpy()
        ref, rerr = memo((ident, v), want)

        def check(outs, host):
            tr.assert_bits(outs[0], ref, ident)
            if not null_err:
                assert np.array_equal(outs[1], rerr)
        outs = [o] if null_err else [o, e]
        return Case([g], outs, lambda st: L().sts_fill_quotients(vp(g.buf), vp(o), S, T, T, w, method, lag, 1,
                                                                 None if null_err else vp(e), st), check)


fill_quotients("fill_quotients-previous", 3, 1, False)
fill_quotients("fill_quotients-linear", 0, 1, False)
fill_quotients("fill_quotients-null-err", 3, 1, True)

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
    if case.sync is None:
        assert pending, "%s is expected to be asynchronous but returned after the delay had run out" % ident


@pytest.mark.parametrize("ident", ["fill_quotients-previous", "fill_quotients-linear", "diff_order_d-9"])
def test_two_streams(torch, delay, ident):
    """the rows with scratch or an error array, two calls on two streams in flight together"""
    a, b = build(ident, torch, 0), build(ident, torch, 1)
    ra, ha = run_plain(torch, a, ident + " [a]")
    rb, hb = run_plain(torch, b, ident + " [b]")
    ta = sg.enqueue(torch, a, torch.cuda.Stream(), delay)
    tb = sg.enqueue(torch, b, torch.cuda.Stream(), delay)
    assert_ticket(torch, ta, ra, ha, ident + " [a]")
    assert_ticket(torch, tb, rb, hb, ident + " [b]")
