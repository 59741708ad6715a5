"""Self-test of tests/layout_arena.py on numpy arenas (no GPU): the views sit at the byte
offsets asked for, verify passes on an untouched arena, and verify fails when one element is
flipped in each of row padding, skew, front red zone and back red zone."""
import numpy as np
import pytest

import layout_arena as la

S, T = 5, 13


@pytest.mark.parametrize("name", la.LAYOUT_NAMES)
@pytest.mark.parametrize("poison", sorted(la.POISONS))
def test_views_sit_at_the_offsets_asked_for(name, poison):
    ld_in, ld_out, b_in, b_out = la.layout(name, T)
    x = np.arange(S * T, dtype=np.float64).reshape(S, T)
    for ld, base in ((ld_in, b_in), (ld_out, b_out)):
        a = la.carve_np(S, T, ld, base, la.POISONS[poison], data=x)
        assert a.ld == ld and a.view.shape == (S, T)
        assert a.view.strides == (8 * ld, 8)
        assert a.ptr == a.view.ctypes.data
        assert a.ptr % 8 == 0 and a.ptr % 128 == (8 * base) % 128
        assert a.ptr - a.flat.ctypes.data == 8 * (la.RED + base)
        assert a.flat.size == 2 * la.RED + base + S * ld
        # the data is where element (s, t) = p[s * ld + t] says, the rest is poison
        h = a.host()
        for s in range(S):
            assert np.array_equal(h[a.off + s * ld: a.off + s * ld + T], x[s])
        out = h[~a.inside_mask()]
        assert out.size == a.flat.size - S * T
        assert np.array_equal(la.bits(out), la.bits(np.full(out.size, la.POISONS[poison])))
        assert np.array_equal(a.data(), x)


def test_named_layouts_are_the_documented_ones():
    assert la.layout("packed", 10) == (10, 10, 0, 0)
    assert la.layout("even", 10) == (12, 14, 0, 0)
    assert la.layout("odd", 10) == (11, 13, 0, 0)
    assert la.layout("in_fast_out_slow", 10) == (12, 12, 0, 1)
    assert la.layout("in_slow_out_fast", 10) == (12, 12, 1, 0)
    assert la.layout("skew", 10, T_out=4) == (15, 11, 5, 15)
    assert len({la.POISONS["sentinel"], la.OUT_FILL}) == 2 and np.isnan(la.POISONS["nan"])


@pytest.mark.parametrize("poison", sorted(la.POISONS))
def test_verify_passes_untouched_and_inside_writes(poison):
    a = la.carve_np(S, T, T + 3, 5, la.POISONS[poison])
    snap = a.snapshot()
    a.verify_all(snap)
    a.verify_outside(snap)
    a.view[...] = 1.0                      # an output may change every (s, t < T)
    a.verify_outside(snap)
    with pytest.raises(AssertionError, match=r"element \(0, 0\)"):
        a.verify_all(snap)                 # an input may change nothing


def _zones(a):
    n = a.S * a.ld
    return {
        "row 1 padding": a.off + 1 * a.ld + a.T,            # first pad element of a middle row
        "row %d padding" % (a.S - 1): a.off + n - 1,        # last pad element of the last row
        "skew": a.off - 1,
        "front red zone": 0,
        "front red zone,": a.red - 1,
        "back red zone": a.off + n,
        "back red zone,": a.flat.size - 1,
    }


@pytest.mark.parametrize("poison", sorted(la.POISONS))
@pytest.mark.parametrize("zone", ["row 1 padding", "row 4 padding", "skew", "front red zone", "front red zone,",
                                  "back red zone", "back red zone,"])
def test_verify_catches_one_flipped_element(poison, zone):
    a = la.carve_np(S, T, T + 3, 5, la.POISONS[poison], data=np.ones((S, T)))
    snap = a.snapshot()
    i = _zones(a)[zone]
    a.flat.view(np.uint64)[i] ^= np.uint64(1)               # one bit: a NaN stays a NaN
    with pytest.raises(AssertionError, match=zone.rstrip(",")):
        a.verify_outside(snap)
    with pytest.raises(AssertionError, match=zone.rstrip(",")):
        a.verify_all(snap)
    a.flat.view(np.uint64)[i] ^= np.uint64(1)
    a.verify_outside(snap)
    a.verify_all(snap)


def test_carve_inside_caller_memory():
    raw = np.zeros(2 * la.RED + 3 + 4 * 9 + la.LINE)
    a = la.carve_np(4, 7, 9, 3, la.OUT_FILL, raw=raw)
    assert raw.ctypes.data <= a.flat.ctypes.data < raw.ctypes.data + 128
    assert (a.ptr - 8 * 3) % 128 == 0
    assert (a.host() == la.OUT_FILL).all()
