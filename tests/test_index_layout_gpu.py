"""The panel-layout contract of include/sts.h on the rebasing entry points of include/sts_index.h
(i3 sts_rebase_shift, i4 sts_rebase_map, i5 sts_align_uniform), which takes it over verbatim: the
padded, odd-strided and skewed arenas of tests/layout_arena.py, with a NaN and a finite sentinel in
everything that is not an element.  Padding, red zones and inputs must keep their bits, and the
elements must be those of the dense call (tests/index_ref.py).  Needs an MI355X.
"""
import ctypes

import numpy as np
import pytest

import index_ref as ir
import layout_arena as la

pytestmark = pytest.mark.gpu

S = 67                      # more series than one workgroup of the gather takes
SHAPES = [(129, 127), (64, 65), (130, 64), (1, 2), (300, 1030)]     # (T_in, T_out); the last takes the gather's tile kernel
DEFAULT = 47.0


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


def run(torch, what, fn, args, ins, outs):
    before_in = [a.snapshot() for a in ins]
    before_out = [a.snapshot() for a in outs]
    torch.cuda.synchronize()
    st = fn(*args)
    assert st == 0, (what, st, lib().sts_last_error())
    torch.cuda.synchronize()
    for a, snap in zip(ins, before_in):
        a.verify_all(snap, what + ": input arena")
    for a, snap in zip(outs, before_out):
        a.verify_outside(snap, what + ": output arena")


CASES = [(lay, poison, shape) for lay in la.LAYOUT_NAMES for poison in la.POISONS for shape in SHAPES]
IDS = ["%s-%s-%dto%d" % (c[0], c[1], c[2][0], c[2][1]) for c in CASES]


@pytest.mark.parametrize("lay,poison,shape", CASES, ids=IDS)
def test_rebase_layouts(torch, lay, poison, shape):
    T_in, T_out = shape
    x = ir.hard_panel(S, T_in, 31 + T_in)
    ld_in, ld_out, b_in, b_out = la.layout(lay, T_in, T_out)
    a = la.carve(S, T_in, ld_in, b_in, la.POISONS[poison], data=x)
    for start in (-3, -2, 0, 1, 2, T_in - 1):
        o = la.carve(S, T_out, ld_out, b_out, la.OUT_FILL)
        what = "shift %s %s %s start=%d" % (lay, poison, shape, start)
        run(torch, what, lib().sts_rebase_shift, (a.ptr, o.ptr, S, T_in, T_out, ld_in, ld_out, start, DEFAULT, None), [a], [o])
        ir.assert_bits(o.data(), ir.gather_panel(x, ir.shift_map(T_in, T_out, start), DEFAULT), what)
    rng = np.random.default_rng(T_out)
    m = np.where(rng.random(T_out) < 0.2, -1, rng.integers(0, T_in + 3, size=T_out)).astype(np.int64)
    md = la.carve(1, T_out, T_out, 1, 0.0, red=64)          # the map in an arena of its own: never written
    md.view.view(torch.int64).copy_(torch.as_tensor(m).reshape(1, -1))
    o = la.carve(S, T_out, ld_out, b_out, la.OUT_FILL)
    what = "map %s %s %s" % (lay, poison, shape)
    run(torch, what, lib().sts_rebase_map, (a.ptr, o.ptr, S, T_in, T_out, ld_in, ld_out, md.ptr, DEFAULT, None), [a, md], [o])
    ir.assert_bits(o.data(), ir.gather_panel(x, m, DEFAULT), what)


@pytest.mark.parametrize("lay,poison", [(l, p) for l in la.LAYOUT_NAMES for p in la.POISONS])
def test_align_layouts(torch, lay, poison):
    T_out = 65
    lengths = [0, 7, 64, 1, 130, 0, 65, 3, 0]
    starts = [0, -2, 1, 0, 60, 3, -64, 5, -1]
    n = len(lengths)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    flat = ir.hard_panel(1, int(offsets[-1]), 5)
    _, ld_out, b_in, b_out = la.layout(lay, T_out)
    vals = la.carve(1, flat.shape[1], flat.shape[1], b_in, la.POISONS[poison], data=flat)   # poison around the values
    off = torch.as_tensor(offsets, device="cuda:0")
    sl = torch.as_tensor(np.array(starts, dtype=np.int64), device="cuda:0")
    o = la.carve(n, T_out, ld_out, b_out, la.OUT_FILL)
    what = "align %s %s" % (lay, poison)
    run(torch, what, lib().sts_align_uniform, (vals.ptr, ctypes.c_void_p(off.data_ptr()), ctypes.c_void_p(sl.data_ptr()), n,
                                               T_out, o.ptr, ld_out, DEFAULT, None), [vals], [o])
    got = o.data()
    for s in range(n):
        row = flat[0, offsets[s]:offsets[s + 1]]
        ir.assert_bits(got[s], ir.gather(row, ir.shift_map(len(row), T_out, starts[s]), DEFAULT), "%s series %d" % (what, s))
    assert np.array_equal(off.cpu().numpy(), offsets) and sl.cpu().numpy().tolist() == starts
