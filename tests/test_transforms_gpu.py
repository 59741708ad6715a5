"""include/sts_transforms.h on an MI355X: bit-exact parity of every device entry point, its `_host`
twin and the Python mirror with the restatement (tests/transforms_ref.py) -- every non-NaN element
has the reference's bits, NaN sits exactly where the reference has NaN.

Shapes are the smallest that reach every path: S around the 16-series chunks and 64-series waves /
workgroups of the kernels, T around the 64-step rounds and 128-step chunks plus the C2 length 390
and one four-digit length, lags around the 32-step history of the one-lane recurrences and of the
one-pass fill + quotients kernel, orders around the 8 levels of the one-pass order-d lanes.  One
panel of S = 130 per T (tr.hard_panel: NaN runs at the head, the tail and inside, all-NaN and
single-valid series, +-0.0, +-inf, subnormals, 2^+-400, zero divisors) and its references are
computed once; a smaller S is its first rows, since the series are independent.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

import layout_arena as la
import transforms_ref as tr
from transforms_ref import assert_bits

pytestmark = pytest.mark.gpu

SS = [1, 15, 16, 17, 63, 64, 65, 130]
TS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 390, 1025]
SMAX = max(SS)
METHODS = {"none": -1, "linear": 0, "nearest": 1, "next": 2, "previous": 3, "spline": 4}
FILL = la.OUT_FILL


def lags(T):
    return sorted({l for l in (0, 1, 2, 5, 31, 32, 33, T - 1, T) if 0 <= l <= T})


def resamplings(T):
    return [(1, 0), (2, 1), (3, 0), (3, 2), (7, 6), (3, T), (3, T + 1)]


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


def P(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data)


@lru_cache(maxsize=None)
def panel(T):
    x = tr.hard_panel(SMAX, T, 7000 + T)
    x.setflags(write=False)
    return x


@lru_cache(maxsize=None)
def dpanel(T):
    import torch as _t
    return _t.as_tensor(panel(T).copy(), device="cuda:0")


def dev(torch, name, xd, S, width, args, status=0):
    """name(in, out, S, T, T, width, *args, NULL) on the first S rows of the device panel xd"""
    T = xd.shape[1]
    o = torch.full((S, width), FILL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = getattr(L(), name)(P(xd), P(o), S, T, T, width, *args, None)
    torch.cuda.synchronize()
    assert st == status, (name, S, T, args, st, L().sts_last_error())
    return o.cpu().numpy()


def host(name, x, width, args, status=0):
    S, T = x.shape
    o = np.full((S, width), FILL)
    st = getattr(L(), name + "_host")(P(np.ascontiguousarray(x)), P(o), S, T, T, *args)
    assert st == status, (name, S, T, args, st, L().sts_last_error())
    return o


def mirror_in(torch, T, S):
    """a series for S == 1, else a panel, on the device"""
    return dpanel(T)[0] if S == 1 else dpanel(T)[:S]


def mirror_out(y, S):
    y = y.cpu().numpy()
    return y.reshape(1, -1) if S == 1 else y


# ---------------- r1: quotients / price2ret ----------------

@pytest.mark.parametrize("T", TS)
def test_quotients(torch, T):
    from sparkts import UnivariateTimeSeries as uts
    x, xd = panel(T), dpanel(T)
    for lag in lags(T):
        for m1 in (0, 1):
            ref = tr.quotients(x, lag, bool(m1))
            for S in SS:
                assert_bits(dev(torch, "sts_quotients", xd, S, T - lag, (lag, m1)), ref[:S], "quotients S=%d lag=%d" % (S, lag))
            assert_bits(host("sts_quotients", x[:17], T - lag, (lag, m1)), ref[:17], "quotients_host lag=%d" % lag)
            for S in (1, 65):
                f = uts.price2ret if m1 else uts.quotients
                assert_bits(mirror_out(f(mirror_in(torch, T, S), lag), S), ref[:S], "mirror quotients lag=%d" % lag)
    assert_bits(uts.quotients(x[:3], min(1, T)), tr.quotients(x[:3], min(1, T)), "mirror, host path")


# ---------------- r2: fill + quotients ----------------

@lru_cache(maxsize=None)
def filled(T, method):
    """sts_fill of the whole panel, with its error array -> (filled, err) on the host"""
    import torch as _t
    xd = dpanel(T)
    if method == "none":
        return panel(T), np.zeros(SMAX, dtype=np.int32)
    f, e = _t.full_like(xd, FILL), _t.full((SMAX,), -1, dtype=_t.int32, device="cuda:0")
    _t.cuda.synchronize()
    assert L().sts_fill(P(xd), P(f), SMAX, T, T, T, METHODS[method], P(e), None) == 0
    _t.cuda.synchronize()
    return f.cpu().numpy(), e.cpu().numpy()


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("T", TS)
def test_fill_quotients(torch, T, method):
    """the fused call == sts_fill followed by sts_quotients, bit for bit, err_per_series included,
    with err_per_series given and NULL; fill("previous") and none also against the restatement"""
    x, xd = panel(T), dpanel(T)
    f, ferr = filled(T, method)
    fd = torch.as_tensor(np.array(f), device="cuda:0")
    code = METHODS[method]
    if method == "previous":
        assert_bits(f, tr.fill_previous(x), "sts_fill previous")
    for lag in lags(T):
        w = T - lag
        ref = tr.quotients(f, lag, True)
        for S in (SS if method in ("previous", "none") else (1, 17, SMAX)):
            two = dev(torch, "sts_quotients", fd, S, w, (lag, 1))
            assert_bits(two, ref[:S], "fill then quotients vs the restatement")
            e = torch.full((S,), -1, dtype=torch.int32, device="cuda:0")
            got = dev(torch, "sts_fill_quotients", xd, S, w, (code, lag, 1, P(e)))
            what = "fill_quotients %s S=%d T=%d lag=%d" % (method, S, T, lag)
            assert_bits(got, two, what)
            assert np.array_equal(e.cpu().numpy(), ferr[:S]), (what, e.cpu().numpy(), ferr[:S])
            bad = ferr[:S][ferr[:S] != 0]
            got = dev(torch, "sts_fill_quotients", xd, S, w, (code, lag, 1, None), status=int(bad[0]) if bad.size else 0)
            assert_bits(got, two, what + " (NULL err)")
        herr = np.full(17, -1, dtype=np.int32)
        assert_bits(host("sts_fill_quotients", x[:17], w, (code, lag, 0, P(herr))), tr.quotients(f[:17], lag, False),
                    "fill_quotients_host %s lag=%d" % (method, lag))
        assert np.array_equal(herr, ferr[:17])


def test_fill_quotients_mirror(torch):
    from sparkts import pipelines
    T = 390
    x = panel(T)
    for S in (1, 65):
        got = pipelines.fill_quotients(mirror_in(torch, T, S), "previous", 1)
        assert_bits(mirror_out(got, S), tr.quotients(tr.fill_previous(x[:S]), 1, True), "mirror fill_quotients")
    assert_bits(pipelines.fill_returns("previous", 2)(x[:5]), tr.quotients(tr.fill_previous(x[:5]), 2, True), "host path")


# ---------------- r3: fillWithDefault ----------------

@pytest.mark.parametrize("T", TS)
def test_fill_with_default(torch, T):
    from sparkts import UnivariateTimeSeries as uts
    x, xd = panel(T), dpanel(T)
    for filler in (0.0, -0.0, 7.5, np.inf, np.nan):
        ref = tr.fill_with_default(x, filler)
        for S in SS:
            assert_bits(dev(torch, "sts_fill_with_default", xd, S, T, (filler,)), ref[:S], "fillWithDefault S=%d" % S)
        # in place
        y = xd[:65].clone()
        torch.cuda.synchronize()
        assert L().sts_fill_with_default(P(y), P(y), 65, T, T, T, filler, None) == 0
        torch.cuda.synchronize()
        assert_bits(y.cpu().numpy(), ref[:65], "fillWithDefault in place")
        assert_bits(host("sts_fill_with_default", x[:17], T, (filler,)), ref[:17], "fillWithDefault_host")
        h = x[:17].copy()
        assert L().sts_fill_with_default_host(P(h), P(h), 17, T, T, filler) == 0
        assert_bits(h, ref[:17], "fillWithDefault_host in place")
        for S in (1, 65):
            assert_bits(mirror_out(uts.fillWithDefault(mirror_in(torch, T, S), filler), S), ref[:S], "mirror fillWithDefault")


# ---------------- r4: downsample / upsample ----------------

@pytest.mark.parametrize("T", TS)
def test_resample(torch, T):
    from sparkts import UnivariateTimeSeries as uts
    x, xd = panel(T), dpanel(T)
    for n, phase in resamplings(T):
        ref = tr.downsample(x, n, phase)
        w = ref.shape[1]
        for S in SS:
            assert_bits(dev(torch, "sts_downsample", xd, S, w, (n, phase)), ref[:S], "downsample S=%d n=%d ph=%d" % (S, n, phase))
        assert_bits(host("sts_downsample", x[:17], w, (n, phase)), ref[:17], "downsample_host")
        for S in (1, 65):
            assert_bits(mirror_out(uts.downsample(mirror_in(torch, T, S), n, phase), S), ref[:S], "mirror downsample")
        if phase >= n:
            continue        # upsample: STS_ERR_BAD_ARG (tests/test_transforms_cpu.py)
        for zero in (0, 1):
            ref = tr.upsample(x, n, phase, bool(zero))
            want_fill = np.float64(0.0 if zero else np.nan).view(np.uint64)
            for S in SS:
                got = dev(torch, "sts_upsample", xd, S, T * n, (n, phase, zero))
                assert_bits(got, ref[:S], "upsample S=%d n=%d ph=%d" % (S, n, phase))
                off = np.ones(T * n, dtype=bool)
                off[phase::n] = False
                assert (got[:, off].view(np.uint64) == want_fill).all(), "the filler is +0.0 or the quiet NaN"
            assert_bits(host("sts_upsample", x[:17], T * n, (n, phase, zero)), ref[:17], "upsample_host")
            for S in (1, 65):
                assert_bits(mirror_out(uts.upsample(mirror_in(torch, T, S), n, phase, bool(zero)), S), ref[:S], "mirror upsample")


# ---------------- r5: firstNotNaN / lastNotNaN, trims ----------------

@pytest.mark.parametrize("T", TS)
def test_first_last(torch, T):
    from sparkts import UnivariateTimeSeries as uts
    x, xd = panel(T), dpanel(T)
    rf, rl = tr.first_not_nan(x), tr.last_not_nan(x)
    for S in SS:
        f = torch.full((S,), -7, dtype=torch.int64, device="cuda:0")
        l = torch.full((S,), -7, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        assert L().sts_first_last_not_nan(P(xd), S, T, T, P(f), P(l), None) == 0
        assert L().sts_first_last_not_nan(P(xd), S, T, T, None, None, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(f.cpu().numpy(), rf[:S]) and np.array_equal(l.cpu().numpy(), rl[:S]), (S, T)
        f.fill_(-7)
        torch.cuda.synchronize()
        assert L().sts_first_last_not_nan(P(xd), S, T, T, None, P(l), None) == 0      # either pointer may be NULL
        torch.cuda.synchronize()
        assert (f.cpu().numpy() == -7).all() and np.array_equal(l.cpu().numpy(), rl[:S])
    hf, hl = np.full(17, -7, dtype=np.int64), np.full(17, -7, dtype=np.int64)
    assert L().sts_first_last_not_nan_host(P(np.ascontiguousarray(x[:17])), 17, T, T, P(hf), P(hl)) == 0
    assert np.array_equal(hf, rf[:17]) and np.array_equal(hl, rl[:17])
    assert L().sts_first_last_not_nan_host(P(np.ascontiguousarray(x[:17])), 17, T, T, P(hf), None) == 0
    # the mirror: an int for a series, an (S,) array for a panel; the trims and their quirk
    assert uts.firstNotNaN(xd[1]) == rf[1] and uts.lastNotNaN(xd[2]) == rl[2] and isinstance(uts.firstNotNaN(xd[1]), int)
    assert np.array_equal(uts.firstNotNaN(xd[:65]).cpu().numpy(), rf[:65])
    assert np.array_equal(uts.lastNotNaN(x[:17]), rl[:17])
    lead, trail = uts.trimLeading(xd[:17]), uts.trimTrailing(xd[:17])
    for s in range(17):
        assert_bits(lead[s].cpu().numpy(), tr.trim_leading(x[s]), "trimLeading")
        assert_bits(trail[s].cpu().numpy(), tr.trim_trailing(x[s]), "trimTrailing")
    assert_bits(uts.trimTrailing(x[0]), tr.trim_trailing(x[0]), "trimTrailing of a series")
    assert uts.trimTrailing(x[4]).shape == (0,) and uts.trimLeading(x[4]).shape == (0,)      # the all-NaN series


# ---------------- r6: inverseDifferencesAtLag ----------------

@pytest.mark.parametrize("T", TS)
def test_inverse_diff_at_lag(torch, T):
    from sparkts import UnivariateTimeSeries as uts
    x, xd = panel(T), dpanel(T)
    for lag in lags(T):
        for start in (lag, lag + 3):
            # lag 0 leaves dest untouched: the pre-filled output stays
            ref = tr.inverse_differences_at_lag(x, lag, start) if lag else np.full_like(x, FILL)
            what = "inverseDifferencesAtLag T=%d lag=%d start=%d" % (T, lag, start)
            for S in SS:
                assert_bits(dev(torch, "sts_inverse_diff_at_lag", xd, S, T, (lag, start)), ref[:S], what + " S=%d" % S)
            assert_bits(host("sts_inverse_diff_at_lag", x[:17], T, (lag, start)), ref[:17], what + " host")
            if not lag:
                continue
            for S in (17, 65):      # in place: the same bits
                y = xd[:S].clone()
                torch.cuda.synchronize()
                assert L().sts_inverse_diff_at_lag(P(y), P(y), S, T, T, T, lag, start, None) == 0
                torch.cuda.synchronize()
                assert_bits(y.cpu().numpy(), ref[:S], what + " in place")
            h = x[:17].copy()
            assert L().sts_inverse_diff_at_lag_host(P(h), P(h), 17, T, T, lag, start) == 0
            assert_bits(h, ref[:17], what + " host, in place")
        ref = tr.inverse_differences_at_lag(x, lag)
        for S in (1, 65):
            assert_bits(mirror_out(uts.inverseDifferencesAtLag(mirror_in(torch, T, S), lag), S), ref[:S], "mirror")
        y = xd[:17].clone()
        assert uts.inverseDifferencesAtLag(y, lag, destTs=y, startIndex=lag + 3) is y
        assert_bits(y.cpu().numpy(), tr.inverse_differences_at_lag(x[:17], lag, lag + 3) if lag else x[:17], "mirror, destTs is ts")


# ---------------- r7: differencesOfOrderD / inverseDifferencesOfOrderD ----------------

@pytest.mark.parametrize("T", TS)
def test_order_d(torch, T):
    from sparkts import UnivariateTimeSeries as uts
    x, xd = panel(T), dpanel(T)
    for d in (0, 1, 2, 5, 8, 9):
        for name, fn, mir in (("sts_diff_order_d", tr.differences_of_order_d, uts.differencesOfOrderD),
                              ("sts_inverse_diff_order_d", tr.inverse_differences_of_order_d, uts.inverseDifferencesOfOrderD)):
            ref = fn(x, d)
            for S in SS:
                assert_bits(dev(torch, name, xd, S, T, (d,)), ref[:S], "%s T=%d d=%d S=%d" % (name, T, d, S))
            assert_bits(host(name, x[:17], T, (d,)), ref[:17], name + "_host")
            for S in (1, 65):
                assert_bits(mirror_out(mir(mirror_in(torch, T, S), d), S), ref[:S], "mirror " + name)


# ---------------- launch shapes: more series than one grid dimension of small blocks ----------------

def test_many_short_series(torch):
    S, T = 65537, 5
    x = tr.hard_panel(S, T, 11)
    xd = torch.as_tensor(x, device="cuda:0")
    fp = tr.fill_previous(x)
    assert_bits(dev(torch, "sts_quotients", xd, S, T - 1, (1, 1)), tr.quotients(x, 1, True), "quotients")
    e = torch.full((S,), -1, dtype=torch.int32, device="cuda:0")
    assert_bits(dev(torch, "sts_fill_quotients", xd, S, T - 2, (3, 2, 1, P(e))), tr.quotients(fp, 2, True), "fill_quotients")
    assert not e.cpu().numpy().any()
    assert_bits(dev(torch, "sts_fill_quotients", xd, S, T - 1, (2, 1, 0, P(e))),
                tr.quotients(tr.fill_previous(x[:, ::-1])[:, ::-1], 1, False), "fill_quotients next")
    assert_bits(dev(torch, "sts_fill_with_default", xd, S, T, (1.5,)), tr.fill_with_default(x, 1.5), "fillWithDefault")
    assert_bits(dev(torch, "sts_downsample", xd, S, 2, (2, 1)), tr.downsample(x, 2, 1), "downsample")
    assert_bits(dev(torch, "sts_upsample", xd, S, 2 * T, (2, 1, 0)), tr.upsample(x, 2, 1), "upsample")
    assert_bits(dev(torch, "sts_inverse_diff_at_lag", xd, S, T, (2, 2)), tr.inverse_differences_at_lag(x, 2), "inverse diff")
    assert_bits(dev(torch, "sts_diff_order_d", xd, S, T, (2,)), tr.differences_of_order_d(x, 2), "order d")
    assert_bits(dev(torch, "sts_inverse_diff_order_d", xd, S, T, (3,)), tr.inverse_differences_of_order_d(x, 3), "inverse order d")
    f, l = (torch.full((S,), -7, dtype=torch.int64, device="cuda:0") for _ in range(2))
    torch.cuda.synchronize()
    assert L().sts_first_last_not_nan(P(xd), S, T, T, P(f), P(l), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(f.cpu().numpy(), tr.first_not_nan(x)) and np.array_equal(l.cpu().numpy(), tr.last_not_nan(x))


# ---------------- the layout contract ----------------

LAY_S = 17
# (name, width(T), extra arguments, reference)
LAYOUT_OPS = [
    ("sts_quotients", lambda T: T - 2, (2, 1), lambda x: tr.quotients(x, 2, True)),
    ("sts_fill_with_default", lambda T: T, (2.5,), lambda x: tr.fill_with_default(x, 2.5)),
    ("sts_downsample", lambda T: (T - 1 + 2) // 3, (3, 1), lambda x: tr.downsample(x, 3, 1)),
    ("sts_upsample", lambda T: 2 * T, (2, 1, 0), lambda x: tr.upsample(x, 2, 1)),
    ("sts_inverse_diff_at_lag", lambda T: T, (2, 3), lambda x: tr.inverse_differences_at_lag(x, 2, 3)),
    ("sts_inverse_diff_at_lag", lambda T: T, (40, 40), lambda x: tr.inverse_differences_at_lag(x, 40, 40)),
    ("sts_diff_order_d", lambda T: T, (3,), lambda x: tr.differences_of_order_d(x, 3)),
    ("sts_diff_order_d", lambda T: T, (9,), lambda x: tr.differences_of_order_d(x, 9)),
    ("sts_inverse_diff_order_d", lambda T: T, (3,), lambda x: tr.inverse_differences_of_order_d(x, 3)),
    ("sts_inverse_diff_order_d", lambda T: T, (9,), lambda x: tr.inverse_differences_of_order_d(x, 9)),
]


def checked(torch, what, call, ins, outs):
    before_in = [a.snapshot() for a in ins]
    before_out = [a.snapshot() for a in outs]
    torch.cuda.synchronize()
    st = call()
    assert st == 0, (what, st, L().sts_last_error())
    torch.cuda.synchronize()
    for a, snap in zip(ins, before_in):
        a.verify_all(snap, what + ": input arena")
    for a, snap in zip(outs, before_out):
        a.verify_outside(snap, what + ": output arena")


@pytest.mark.parametrize("poison", sorted(la.POISONS))
@pytest.mark.parametrize("lay", la.LAYOUT_NAMES)
def test_layout(torch, lay, poison):
    """every layout of tests/layout_arena.py, both poisons: results from the elements alone, nothing
    written outside the output block, inputs untouched"""
    vp = ctypes.c_void_p
    for T in (65, 390):
        x = np.array(panel(T)[:LAY_S])
        for name, width, args, ref in LAYOUT_OPS:
            w = width(T)
            ld_in, ld_out, b_in, b_out = la.layout(lay, T, w)
            a = la.carve(LAY_S, T, ld_in, b_in, la.POISONS[poison], data=x)
            o = la.carve(LAY_S, w, ld_out, b_out, la.OUT_FILL)
            what = "%s%s T=%d %s %s" % (name, list(args), T, lay, poison)
            checked(torch, what, lambda: getattr(L(), name)(vp(a.ptr), vp(o.ptr), LAY_S, T, ld_in, ld_out, *args, None), [a], [o])
            assert_bits(o.data(), ref(x), what)
        # in place on a padded panel: (s, t < T) only
        ld_in, _, b_in, _ = la.layout(lay, T)
        for name, args, ref in (("sts_fill_with_default", (2.5,), lambda v: tr.fill_with_default(v, 2.5)),
                                ("sts_inverse_diff_at_lag", (5, 5), lambda v: tr.inverse_differences_at_lag(v, 5)),
                                ("sts_inverse_diff_at_lag", (33, 36), lambda v: tr.inverse_differences_at_lag(v, 33, 36))):
            a = la.carve(LAY_S, T, ld_in, b_in, la.POISONS[poison], data=x)
            what = "%s%s in place T=%d %s %s" % (name, list(args), T, lay, poison)
            checked(torch, what, lambda: getattr(L(), name)(vp(a.ptr), vp(a.ptr), LAY_S, T, ld_in, ld_in, *args, None), [], [a])
            assert_bits(a.data(), ref(x), what)
        # the fused call: the one-pass kernel (previous, lags 1 and 32) and the composition (linear; previous, lag 33)
        for method, lag in (("previous", 1), ("previous", 32), ("previous", 33), ("linear", 1), ("spline", 2)):
            w = T - lag
            ld_in, ld_out, b_in, b_out = la.layout(lay, T, w)
            a = la.carve(LAY_S, T, ld_in, b_in, la.POISONS[poison], data=x)
            o = la.carve(LAY_S, w, ld_out, b_out, la.OUT_FILL)
            e = torch.full((LAY_S,), -1, dtype=torch.int32, device="cuda:0")
            what = "fill_quotients %s lag=%d T=%d %s %s" % (method, lag, T, lay, poison)
            checked(torch, what, lambda: L().sts_fill_quotients(vp(a.ptr), vp(o.ptr), LAY_S, T, ld_in, ld_out, METHODS[method],
                                                               lag, 1, P(e), None), [a], [o])
            f, ferr = filled(T, method)
            assert_bits(o.data(), tr.quotients(f[:LAY_S], lag, True), what)
            assert np.array_equal(e.cpu().numpy(), ferr[:LAY_S])
        # firstNotNaN / lastNotNaN: per-series outputs with red zones of their own
        ld_in, _, b_in, _ = la.layout(lay, T)
        a = la.carve(LAY_S, T, ld_in, b_in, la.POISONS[poison], data=x)
        f, l = (torch.full((LAY_S + 2,), -7, dtype=torch.int64, device="cuda:0") for _ in range(2))
        checked(torch, "first_last", lambda: L().sts_first_last_not_nan(vp(a.ptr), LAY_S, T, ld_in, vp(f.data_ptr() + 8),
                                                                       vp(l.data_ptr() + 8), None), [a], [])
        f, l = f.cpu().numpy(), l.cpu().numpy()
        assert np.array_equal(f[1:-1], tr.first_not_nan(x)) and np.array_equal(l[1:-1], tr.last_not_nan(x)), (lay, poison)
        assert f[0] == f[-1] == l[0] == l[-1] == -7


# ---------------- isolation ----------------

def test_isolation(torch):
    """a good series keeps its bits when every other series of its wave, chunk and workgroup is
    all-NaN or non-finite"""
    T = 390
    good = 100.0 + np.random.default_rng(5).standard_normal(T).cumsum()
    good[10:14] = np.nan
    one = good.reshape(1, T)
    gd = torch.as_tensor(one, device="cuda:0")
    ops = [("sts_quotients", T - 1, (1, 1)), ("sts_fill_quotients", T - 1, (3, 1, 1, None)),
           ("sts_fill_quotients", T - 2, (0, 2, 1, None)), ("sts_fill_with_default", T, (0.5,)),
           ("sts_downsample", 130, (3, 0)), ("sts_upsample", 2 * T, (2, 0, 1)), ("sts_inverse_diff_at_lag", T, (1, 1)),
           ("sts_inverse_diff_at_lag", T, (33, 33)), ("sts_diff_order_d", T, (3,)), ("sts_inverse_diff_order_d", T, (8,))]
    alone = [dev(torch, name, gd, 1, w, args) for name, w, args in ops]
    for junk in (np.nan, np.inf, -np.inf):
        for pos in (0, 15, 16, 63, 64, 129):
            x = np.full((SMAX, T), junk)
            x[pos] = good
            xd = torch.as_tensor(x, device="cuda:0")
            for (name, w, args), ref in zip(ops, alone):
                got = dev(torch, name, xd, SMAX, w, args)
                assert np.array_equal(got[pos].view(np.uint64), ref[0].view(np.uint64)), (name, args, junk, pos)
            f, l = (torch.full((SMAX,), -7, dtype=torch.int64, device="cuda:0") for _ in range(2))
            torch.cuda.synchronize()
            assert L().sts_first_last_not_nan(P(xd), SMAX, T, T, P(f), P(l), None) == 0
            torch.cuda.synchronize()
            assert int(f[pos]) == 0 and int(l[pos]) == T - 1
