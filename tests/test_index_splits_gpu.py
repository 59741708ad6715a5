"""The large-S launch splits of include/sts_index.h's rebasing entry points (i3, i4, i5): S = 65 536 +
3 and S = 64 x 65 535 + 3 series of 3 steps -- the sizes at which the other entry points split their
launches; these kernels index series through one grid dimension and need no split, which is what
this pins -- about 100 MB per panel at the larger size.  The first and last
rows and the rows on both sides of each split boundary are checked exactly against
tests/index_ref.py on the host; a 64-bit checksum over the bits, and a device-side comparison with
the same rule written in torch indexing, cover the rest.  Needs an MI355X.
"""
import ctypes

import numpy as np
import pytest

import index_ref as ir

pytestmark = pytest.mark.gpu

T_IN, T_OUT = 4, 3
SIZES = (65536 + 3, 64 * 65535 + 3)
DEFAULT = -0.0


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
    return ctypes.c_void_p(t.data_ptr())


def rows_to_check(S):
    edge = [0, 1, S - 2, S - 1]
    for b in (65535, 65536, 64 * 65535):
        edge += [b - 1, b, b + 1]
    return sorted({s for s in edge if 0 <= s < S})


def source(torch, S):
    """x(s, t) = 4 s + t + 0.25: every element distinct and exact"""
    return (torch.arange(S * T_IN, dtype=torch.float64, device="cuda:0") + 0.25).view(S, T_IN)


def expected(torch, x, m):
    """the gather rule in torch indexing, on the device"""
    S = x.shape[0]
    want = torch.full((S, len(m)), DEFAULT, dtype=torch.float64, device="cuda:0")
    for j, k in enumerate(m):
        if 0 <= k < x.shape[1]:
            want[:, j] = x[:, k]
    return want


def verify(torch, got, x, m, what):
    want = expected(torch, x, m)
    gb, wb = got.view(torch.int64), want.view(torch.int64)
    assert int(gb.sum().item()) == int(wb.sum().item()), what + ": checksum"
    assert bool(torch.equal(gb, wb)), what
    rows = rows_to_check(x.shape[0])
    idx = torch.as_tensor(rows, device="cuda:0")
    ir.assert_bits(got[idx].cpu().numpy(), ir.gather_panel(x[idx].cpu().numpy(), m, DEFAULT), what + ": boundary rows")


@pytest.mark.parametrize("S", SIZES)
def test_rebase_shift_and_map_splits(torch, S):
    x = source(torch, S)
    out = torch.empty((S, T_OUT), dtype=torch.float64, device="cuda:0")
    for start in (1, -1, 2):
        out.fill_(7.0)
        assert L().sts_rebase_shift(vp(x), vp(out), S, T_IN, T_OUT, T_IN, T_OUT, start, DEFAULT, None) == 0, L().sts_last_error()
        verify(torch, out, x, ir.shift_map(T_IN, T_OUT, start), "shift %d S=%d" % (start, S))
    for m in ([3, -1, 0], [4, 2, 2]):
        out.fill_(7.0)
        md = torch.as_tensor(np.array(m, dtype=np.int64), device="cuda:0")
        assert L().sts_rebase_map(vp(x), vp(out), S, T_IN, T_OUT, T_IN, T_OUT, vp(md), DEFAULT, None) == 0, L().sts_last_error()
        verify(torch, out, x, m, "map %s S=%d" % (m, S))


@pytest.mark.parametrize("S", SIZES)
def test_align_uniform_splits(torch, S):
    """series s has 1 + s % 4 values and start_loc (s % 3) - 1; its values are s + t / 8"""
    s = torch.arange(S, dtype=torch.int64, device="cuda:0")
    lengths = 1 + s % 4
    offsets = torch.zeros(S + 1, dtype=torch.int64, device="cuda:0")
    offsets[1:] = torch.cumsum(lengths, 0)
    starts = s % 3 - 1
    owner = torch.repeat_interleave(s, lengths)
    within = torch.arange(owner.numel(), dtype=torch.int64, device="cuda:0") - offsets[owner]
    vals = owner.double() + within.double() / 8
    out = torch.full((S, T_OUT), 7.0, dtype=torch.float64, device="cuda:0")
    st = L().sts_align_uniform(vp(vals), vp(offsets), vp(starts), S, T_OUT, vp(out), T_OUT, DEFAULT, None)
    assert st == 0, L().sts_last_error()
    j = torch.arange(T_OUT, dtype=torch.int64, device="cuda:0")
    k = j[None, :] + starts[:, None]
    hit = (k >= 0) & (k < lengths[:, None])
    want = torch.where(hit, s[:, None].double() + k.double() / 8, torch.full_like(out, DEFAULT))
    assert int(out.view(torch.int64).sum().item()) == int(want.view(torch.int64).sum().item())
    assert bool(torch.equal(out.view(torch.int64), want.view(torch.int64)))
    hv, ho, hs = vals.cpu().numpy(), offsets.cpu().numpy(), starts.cpu().numpy()
    got = out[torch.as_tensor(rows_to_check(S), device="cuda:0")].cpu().numpy()
    for i, r in enumerate(rows_to_check(S)):
        row = hv[ho[r]:ho[r + 1]]
        ir.assert_bits(got[i], ir.gather(row, ir.shift_map(len(row), T_OUT, int(hs[r])), DEFAULT), "align row %d" % r)
