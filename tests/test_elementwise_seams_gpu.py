"""The seams of the element-parallel loop (csrc/sts_elementwise.hpp for_each_out) on every entry
point whose kernel runs it.  Needs an MI355X.

The operators' own tests run them at shapes like 7 x 390: one workgroup and a bit.  A workgroup of
the loop owns one chunk of 256 threads x 8 = 2048 consecutive output elements, and split() turns an
element's index g into (row, column) with a double reciprocal and a fix-up, so the places where it
can go wrong are the seams, pinned here as the shape (rows, row length) of the panel the loop walks:

  (1, 1)        the smallest panel
  (2, 1024)     n is exactly one chunk
  (3, 683)      n = 2049: one element into a second workgroup
  (5, 4099)     a row longer than two chunks, prime: split()'s fix-up branches are taken
  (4100, 1)     row length 1: the row index carries everything

Every operator runs these as its INPUT shape (lag 1, p 1, n 2, phase 1; where that leaves no output
at T = 1 -- quotients, lag matrix, downsample -- the T = 1 shapes are left out for that operator),
and the operators whose output row is not their input row run them once more as the OUTPUT shape
(quotients and the lag matrix from T + 1 steps, downsample from 2 T + 1, upsample with n = 1), so
that n, not only S * T, sits on each seam.  sts_rebase_map walks 16 elements per thread (chunks of
4096) while the whole map fits LDS (T_out <= 1024): (4, 1024) and (17, 241) are its one chunk and
one element more, and (65, 1025) is the first row length of map_kernel, with two row tiles.

Each case runs packed and with padded pitches ld_in = T_in + 3, ld_out = T_out + 1.  The input's pad
columns hold NaN; the output is pre-filled with a sentinel, pad columns and a tail past the last row
included.  The elements must have the bits of the references the operators' own tests use (oracle.*,
tests/transforms_ref.py, tests/index_ref.py) and every pad and tail element must keep the sentinel.
One test id is one operator x one pitch; references are computed once per case and shared.
"""
import functools

import numpy as np
import pytest

import index_ref as ir
import oracle
import transforms_ref as tr
from stream_gate import dev, vp
from test_layout_gpu import assert_bits as oracle_bits

pytestmark = pytest.mark.gpu

SENT = -3.0e55
TAIL = 8                    # sentinel elements past the last output row
DEFAULT = 47.0
FILLER = 7.25
SHAPES = [(1, 1), (2, 1024), (3, 683), (5, 4099), (4100, 1)]
LONG = [(S, T) for S, T in SHAPES if T > 1]
cache = functools.lru_cache(maxsize=None)


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


# A case is (x, ref, assert_bits, aux, call): the host input panel, the expected output panel, the
# reference's own comparison, host arrays the call takes besides (uploaded as they are), and
# call(lib, in, ld_in, out, ld_out, *aux) -> status.

def gauss(S, T, seed):
    return np.random.default_rng(seed).standard_normal((S, T)) + 10


@cache
def diff_at_lag(S, T):
    x = gauss(S, T, 1)
    ref = np.array([oracle.differences_at_lag(r, 1, start=1) for r in x])
    return x, ref, oracle_bits, [], lambda lib, a, ldi, o, ldo: lib.sts_diff_at_lag(a, o, S, T, ldi, ldo, 1, 1, None)


@cache
def ewma_remove(S, T):
    x = gauss(S, T, 2)
    sm = np.random.default_rng(3).uniform(0.05, 0.95, S)
    ref = np.array([oracle.ewma_remove(r, v) for r, v in zip(x, sm)])
    return x, ref, oracle_bits, [sm], lambda lib, a, ldi, o, ldo, s: lib.sts_ewma_remove(a, o, S, T, ldi, ldo, s, None)


@cache
def ar_remove(S, T):
    x = gauss(S, T, 4)
    rng = np.random.default_rng(5)
    c, coef = rng.standard_normal(S), rng.uniform(-0.3, 0.3, (S, 1))
    ref = np.array([oracle.ar_remove(x[s], c[s], coef[s]) for s in range(S)])
    return x, ref, oracle_bits, [c, coef], lambda lib, a, ldi, o, ldo, cd, fd: lib.sts_ar_remove(
        a, o, S, T, ldi, ldo, cd, fd, 1, None)


@cache
def lag_matrix(S, T, inc):
    """the output has no pitch: one packed row of S * ncols * (T - 1) elements"""
    x = gauss(S, T, 6)
    ref = np.concatenate([oracle.lag(r, 1, bool(inc)).T.ravel() for r in x]).reshape(1, -1)
    return x, ref, oracle_bits, [], lambda lib, a, ldi, o, ldo: lib.sts_lag_matrix(a, o, S, T, ldi, 1, inc, None)


@cache
def quotients(S, T):
    x = tr.hard_panel(S, T, 7)
    return x, tr.quotients(x, 1, True), tr.assert_bits, [], lambda lib, a, ldi, o, ldo: lib.sts_quotients(
        a, o, S, T, ldi, ldo, 1, 1, None)


@cache
def fill_with_default(S, T):
    x = tr.hard_panel(S, T, 8)
    return x, tr.fill_with_default(x, FILLER), tr.assert_bits, [], lambda lib, a, ldi, o, ldo: lib.sts_fill_with_default(
        a, o, S, T, ldi, ldo, FILLER, None)


@cache
def downsample(S, T):
    x = tr.hard_panel(S, T, 9)
    return x, tr.downsample(x, 2, 1), tr.assert_bits, [], lambda lib, a, ldi, o, ldo: lib.sts_downsample(
        a, o, S, T, ldi, ldo, 2, 1, None)


@cache
def upsample(S, T, n):
    x = tr.hard_panel(S, T, 10)
    return x, tr.upsample(x, n, n - 1), tr.assert_bits, [], lambda lib, a, ldi, o, ldo: lib.sts_upsample(
        a, o, S, T, ldi, ldo, n, n - 1, 0, None)


@cache
def rebase_shift(S, T, start):
    x = ir.hard_panel(S, T, 11)
    ref = ir.gather_panel(x, ir.shift_map(T, T, start), DEFAULT)
    return x, ref, ir.assert_bits, [], lambda lib, a, ldi, o, ldo: lib.sts_rebase_shift(
        a, o, S, T, T, ldi, ldo, start, DEFAULT, None)


@cache
def rebase_map(S, T):
    x = ir.hard_panel(S, T, 12)
    rng = np.random.default_rng(13 + T)
    m = np.where(rng.random(T) < 0.2, -1, rng.integers(0, T + 3, size=T)).astype(np.int64)
    return x, ir.gather_panel(x, m, DEFAULT), ir.assert_bits, [m], lambda lib, a, ldi, o, ldo, md: lib.sts_rebase_map(
        a, o, S, T, T, ldi, ldo, md, DEFAULT, None)


@cache
def align_uniform(S, T):
    """the input is the ragged series back to back (no pitch): lengths 0 .. 2 T, starts either side of 0"""
    rng = np.random.default_rng(14 + S)
    lengths = rng.integers(0, 2 * T + 1, S)
    lengths[0] = max(lengths[0], 1)
    starts = rng.integers(-(T // 2) - 1, T // 2 + 2, S).astype(np.int64)
    offsets = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    flat = ir.hard_panel(1, int(offsets[-1]), 15)
    ref = np.array([ir.gather(flat[0, offsets[s]:offsets[s + 1]], ir.shift_map(int(lengths[s]), T, int(starts[s])), DEFAULT)
                    for s in range(S)])
    return flat, ref, ir.assert_bits, [offsets, starts], lambda lib, a, ldi, o, ldo, od, sd: lib.sts_align_uniform(
        a, od, sd, S, T, o, ldo, DEFAULT, None)


def out_shapes(t_in):
    return [(S, t_in(T)) for S, T in SHAPES]


# operator -> [(case builder, its arguments after (S, T), the (S, T_in) it runs at)]
OPS = {
    "diff_at_lag": [(diff_at_lag, (), SHAPES)],
    "ewma_remove": [(ewma_remove, (), SHAPES)],
    "ar_remove": [(ar_remove, (), SHAPES)],
    "lag_matrix": [(lag_matrix, (1,), LONG), (lag_matrix, (0,), out_shapes(lambda T: T + 1))],
    "quotients": [(quotients, (), LONG + out_shapes(lambda T: T + 1))],
    "fill_with_default": [(fill_with_default, (), SHAPES)],
    "downsample": [(downsample, (), LONG + out_shapes(lambda T: 2 * T + 1))],
    "upsample": [(upsample, (2,), SHAPES), (upsample, (1,), SHAPES)],
    "rebase_shift": [(rebase_shift, (1,), SHAPES), (rebase_shift, (-1,), SHAPES)],
    "rebase_map": [(rebase_map, (), SHAPES + [(4, 1024), (17, 241), (65, 1025)])],
    "align_uniform": [(align_uniform, (), SHAPES)],
}


@pytest.mark.parametrize("padded", [False, True], ids=["packed", "padded"])
@pytest.mark.parametrize("op", sorted(OPS))
def test_seams(torch, op, padded):
    for build, args, shapes in OPS[op]:
        for S, T in shapes:
            x, ref, assert_bits, aux, call = build(S, T, *args)
            what = "%s%s S=%d T=%d %s" % (op, args, S, T, "padded" if padded else "packed")
            rows, T_out = ref.shape
            assert rows * T_out > 0, what
            ld_in, ld_out = x.shape[1] + (3 if padded else 0), T_out + (1 if padded else 0)
            a = torch.full((x.shape[0], ld_in), float("nan"), dtype=torch.float64, device="cuda:0")
            a[:, :x.shape[1]] = dev(torch, x)
            o = torch.full((rows * ld_out + TAIL,), SENT, dtype=torch.float64, device="cuda:0")
            more = [dev(torch, v, v.dtype) for v in aux]
            st = call(L(), vp(a), ld_in, vp(o), ld_out, *[vp(v) for v in more])
            assert st == 0, (what, st, L().sts_last_error())
            torch.cuda.synchronize()
            got = o.cpu().numpy()
            panel = got[:rows * ld_out].reshape(rows, ld_out)
            assert_bits(panel[:, :T_out], ref, what)
            assert (panel[:, T_out:] == SENT).all(), what + ": a pad column was written"
            assert (got[rows * ld_out:] == SENT).all(), what + ": written past the last row"
