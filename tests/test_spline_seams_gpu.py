"""fill("spline") (csrc/sts_spline.hip) at its seams.  Random panels of a few dozen rows almost
never put a knot at a chosen offset of its 8-step chunk next to a gap of a chosen length, a gap of
hundreds of steps beside dense neighbours, or three knots in one chunk; tests/spline_patterns.py
does (tests/test_spline_patterns_cpu.py proves the placement).  Here every pattern runs through
sts_fill(method 4) in the three layouts that launch_spline's dispatch rule tells apart:

    lds       128-B aligned base, ld_in and ld_out even      spline_lds_kernel (odd T: its tail path)
    odd_ld    aligned base, ld_in and ld_out odd             spline_fill_kernel
    skewed    even ld, the panel starts one double later     spline_fill_kernel

The input lies in a NaN-poisoned arena, the output arena holds a sentinel, err holds -1.
Expectation: err is the oracle's vector for all S rows; accepted rows have the oracle's bits,
refused rows their raw input bits; every double outside the output's (s, t < T) -- row padding,
skew, red zones -- still holds the sentinel; the input arena is unchanged.  All three layouts
against one reference, so the two kernels also agree with each other.
"""
from functools import lru_cache

import numpy as np
import pytest

import layout_arena as la
import oracle
import seg_patterns as segp
import spline_patterns as sp

pytestmark = pytest.mark.gpu

SPLINE = 4   # STS_FILL_SPLINE
PANELS = dict(sp.all_panels())
LAYOUTS = ["lds", "odd_ld", "skewed"]


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


def lib():
    from sparkts import _native
    return _native.lib()


def layout(name, T):
    """(ld_in, ld_out, offset in doubles from a 128-B aligned address)"""
    if name == "lds":
        ld = T + (T & 1)
        return ld, ld + 2, 0
    if name == "odd_ld":
        ld = T + 1 - (T & 1)
        return ld, ld + 2, 0
    ld = T + (T & 1)
    return ld, ld + 2, 1


def takes_lds_form(ld_in, ld_out, offset):
    """launch_spline's rule: 16-B row pieces on both sides."""
    return ld_in % 2 == 0 and ld_out % 2 == 0 and offset % 2 == 0


@lru_cache(maxsize=None)
def reference(name):
    out, err = oracle.panel_fill(PANELS[name].x, "spline")
    out.setflags(write=False)
    err.setflags(write=False)
    return out, err


def run(torch, x, ld_in, ld_out, offset, K=0):
    """-> (filled (S, T), err (S,), acf (S, K) or None); asserts that nothing outside the output
    elements and nothing of the input changed."""
    S, T = x.shape
    a = la.carve(S, T, ld_in, offset, float("nan"), data=np.array(x))
    o = la.carve(S, T, ld_out, offset, la.OUT_FILL)
    err = torch.full((S,), -1, dtype=torch.int32, device="cuda:0")
    sa, so = a.snapshot(), o.snapshot()
    if K:
        acf = torch.full((S, K), la.OUT_FILL, dtype=torch.float64, device="cuda:0")
        st = lib().sts_fill_autocorr(a.ptr, o.ptr, S, T, ld_in, ld_out, SPLINE, K, acf.data_ptr(), err.data_ptr(), None)
    else:
        acf = None
        st = lib().sts_fill(a.ptr, o.ptr, S, T, ld_in, ld_out, SPLINE, err.data_ptr(), None)
    assert st == 0, lib().sts_last_error()
    torch.cuda.synchronize()
    o.verify_outside(so, "spline output")
    a.verify_all(sa, "spline input")
    return o.data(), err.cpu().numpy(), (None if acf is None else acf.cpu().numpy())


def compare(name, what, got, gerr):
    p = PANELS[name]
    ref, rerr = reference(name)
    assert np.array_equal(gerr, rerr), "%s: err %s, oracle %s" % (what, gerr.tolist(), rerr.tolist())
    want = np.where(p.reject[:, None], p.x, ref)      # a refused row keeps its raw bits
    bad = la.bits(got) != la.bits(want)
    # a NaN that the arithmetic produced -- only in [first knot, last knot) of a row declared
    # non-finite -- is a NaN in both, whatever its sign and payload (as in tests/test_spline.py);
    # a raw NaN is copied and keeps its bits
    for r in np.flatnonzero(p.nonfinite & ~p.reject):
        k = sp.knots_of(p.x[r])
        bad[r, k[0]:k[-1]] &= ~(np.isnan(got[r, k[0]:k[-1]]) & np.isnan(want[r, k[0]:k[-1]]))
    if bad.any():
        r, t = (int(v) for v in np.argwhere(bad)[0])
        k = sp.knots_of(p.x[r])
        left = int(k[k <= t][-1]) if (k <= t).any() else -1
        raise AssertionError(
            "%s: %d values differ in rows %s, first at row %d (%s, meta %r) step %d (left knot %d, storage class %s): "
            "got %r, oracle %r" % (what, int(bad.sum()), np.flatnonzero(bad.any(axis=1))[:8].tolist(), r,
                                   "refused" if p.reject[r] else "accepted", p.meta[r], t, left,
                                   sp.store_class(left, t) if left >= 0 else None, float(got[r, t]), float(want[r, t])))


def test_the_layouts_reach_both_kernels():
    for T in (40, 41, 96):
        assert takes_lds_form(*layout("lds", T))
        assert not takes_lds_form(*layout("odd_ld", T)) and layout("odd_ld", T)[0] % 2 == 1
        assert not takes_lds_form(*layout("skewed", T)) and layout("skewed", T)[0] % 2 == 0
        assert all(layout(n, T)[0] >= T for n in LAYOUTS)
    assert layout("lds", 41) == (42, 44, 0)       # odd T at an even pitch: the single-element tail


@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("name", list(PANELS))
def test_every_pattern(torch, name, lay):
    x = PANELS[name].x
    ld_in, ld_out, offset = layout(lay, x.shape[1])
    got, gerr, _ = run(torch, x, ld_in, ld_out, offset)
    compare(name, "%s %s" % (name, lay), got, gerr)


@pytest.mark.parametrize("name", ["gap_by_offset", "long_gaps_beside_dense", "long_gaps_every_row"])
def test_fill_autocorr_composes_the_same_fill(torch, name):
    """sts_fill_autocorr(method 4) is the spline kernel, then the ACF of its output: the same bits,
    and an ACF within the contract of tests/test_acf_robust.py (identical NaN pattern,
    |got - ref| <= 1e-10 |ref| + noise_floor(lag))."""
    K = 5
    x = PANELS[name].x
    ref, rerr = reference(name)
    assert not rerr.any()
    got, gerr, acf = run(torch, x, *layout("lds", x.shape[1]), K=K)
    compare(name, "%s fill_autocorr" % name, got, gerr)
    racf = np.array([oracle.autocorr(r, K) for r in ref])
    floor = np.array([segp.noise_floor(r, K) for r in ref])
    assert np.isfinite(racf).all()
    e = segp.within(acf, racf, floor)
    assert e <= 1.0, "%s: ACF error %.3g x (1e-10 rel + noise floor)" % (name, e)
