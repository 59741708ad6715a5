"""The one-wave kernels of csrc/sts_short.hip at their lane-block seams.  Lane l owns the steps
[l B, l B + B) of the series, B = 8, 16, 24, 32 or 40 by length and lag count (launch_short_m), and
short_fill handles a NaN run block by block.  tests/seg_patterns.py (short_panel) places one run per
row against the B of the shape under test: from a block's last step, to a block's first step, over
exactly one, two and five blocks (the lanes between have an empty mask), into the last occupied block
up to T - 1 (lane 63's at T = 512 and 2560), all of lane 0's block but index 0 (fill('nearest')
never takes index 0 as an end), and a linear run of 33 or more steps over three or more blocks.

The product dispatch runs its default form; the A/B build runs both STS_SHORT_PAIR forms
(short_fill_acf_kernel, short_pair_kernel), on 9 rows (the last pair's second wave is empty) and
on one.  Fill bit-exact, err exact, the ACF by the contract of tests/test_acf_robust.py.
"""
import pytest

import seg_patterns as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


def check(torch, T, K, method, what, rows=None):
    x = sp.short_panel(T, K).x
    xr = x if rows is None else x[rows]
    got = sp.run_device(torch, xr, method, K)
    sp.compare(xr, got, sp.short_reference(T, K, method), K,
               "%s T=%d K=%d B=%d %s rows %s" % (what, T, K, sp.short_block(T, K), method, sp.SHORT_ROWS), rows=rows)


@pytest.mark.parametrize("method", sp.METHODS)
@pytest.mark.parametrize("T,K", sp.SHORT_SHAPES)
def test_block_seams_product_dispatch(torch, T, K, method):
    check(torch, T, K, method, "product")


@pytest.mark.parametrize("method", sp.METHODS)
@pytest.mark.parametrize("T,K", sp.SHORT_SHAPES)
def test_block_seams_both_forms(torch, ab_lib, T, K, method):
    for pair in (0, 1):
        ab_lib(STS_SHORT_PAIR=pair)
        check(torch, T, K, method, "STS_SHORT_PAIR=%d" % pair)
        check(torch, T, K, method, "STS_SHORT_PAIR=%d" % pair, rows=slice(7, 8))
        check(torch, T, K, method, "STS_SHORT_PAIR=%d" % pair, rows=slice(2, 8))
