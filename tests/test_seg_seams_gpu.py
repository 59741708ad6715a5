"""The segment kernel (csrc/sts_seg.hip) at its tile, word and long-run seams.  Every sts_fill,
sts_fill_autocorr and sts_autocorr call with T <= 16 384 on a 16-byte aligned panel runs it, and
random NaNs almost never reach its seams: 65 NaNs in one 512-step tile, a fully NaN validity word,
a look-ahead into each register, half and lane of the next tile, a run whose 33rd step is the
first step of a tile.  tests/seg_patterns.py places NaNs there (tests/test_seg_patterns_cpu.py
proves the placement); here every pattern runs through the product library and dispatch:

  seg_kernel<0>  K = 0           seg_kernel<2>  K = 20 (T > 2560: not the short kernel)
  seg_kernel<4>  K = 25, 60      fused finalize: last tile in ring slot 1 (T_A = 2760) and slot 0
                                 (T_B = 3272, the copy-up); unfused: T = 2600 (last tile < 64 steps),
                                 T <= 2 K, and the A/B build's multi-segment decompositions

Expectation: err (pre-filled with 99) is the oracle's vector; rows without an error have the
oracle's bits; the ACF meets the contract of tests/test_acf_robust.py (restated in
tests/seg_patterns.py, not loosened): identical NaN pattern, |got - ref| <= 1e-10 |ref| +
noise_floor(lag).  A mismatch is reported as tile, word, bit and t - L.
"""
import numpy as np
import pytest

import seg_patterns as sp
from seg_patterns import T_A, T_B

pytestmark = pytest.mark.gpu

KS = [0, 20, 60]
KS_A = [0, 20, 25, 60]     # 25: the first lag count on seg_kernel<4>


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


def check(torch, name, T, method, K, pad=0, what=""):
    x = sp.panel(name, T).x
    got = sp.run_device(torch, x, method, K, pad)
    sp.compare(x, got, sp.reference(name, T, method, K), K, "%s%s T=%d %s K=%d" % (what, name, T, method, K))


@pytest.mark.parametrize("method", sp.METHODS)
@pytest.mark.parametrize("name", sp.ALL)
def test_every_pattern(torch, name, method):
    """T_A: six tiles, the last (200 steps) in ring slot 1.  seg_kernel<0>, <2> and <4>, fused finalize."""
    for K in KS_A:
        check(torch, name, T_A, method, K)


@pytest.mark.parametrize("method", sp.METHODS)
@pytest.mark.parametrize("name", sp.SUBSET)
def test_subset_last_tile_in_slot_0(torch, name, method):
    """T_B: seven tiles; the fused finalize copies the last tile's y up from ring slot 0."""
    for K in KS:
        check(torch, name, T_B, method, K)


@pytest.mark.parametrize("method", sp.METHODS)
def test_padded_rows_nothing_past_T(torch, method):
    """ld = T + 8 on both sides: run_device asserts that every output pad element keeps its sentinel."""
    for name in ("n129", "nan_tile", "to_end", "ahead_none3", "edges4", "sparse", "word7", "pair_w7"):
        for K in (0, 20):
            check(torch, name, T_A, method, K, pad=8, what="ld=T+8 ")
    check(torch, "to_end", T_B, method, 60, pad=8, what="ld=T+8 ")


@pytest.mark.parametrize("method", sp.METHODS)
@pytest.mark.parametrize("T", sp.END_T)
def test_series_ends(torch, T, method):
    """The partial last tile: clamped loads, phantom steps kept out of the NaN list (hiw).  Odd T at an
    even pitch (ld = T + 1), which keeps the rows on the segment kernel; T <= 2 K and a last tile below
    64 steps take the unfused finalize."""
    p, names = sp.ends_panel(T)
    for K in [0] + [K for K in (20, 60) if T > K + 1]:
        got = sp.run_device(torch, p.x, method, K)
        sp.compare(p.x, got, sp.ends_reference(T, method, K), K, "ends %s T=%d %s K=%d" % (names, T, method, K))


@pytest.mark.parametrize("method", sp.METHODS)
@pytest.mark.parametrize("T,K", [(2600, 20), (2600, 60), (100, 60), (120, 60), (40, 20)])
def test_unfused_finalize(torch, T, K, method):
    """The same kernel writing partials for acf_finalize_kernel: the last tile holds 40 steps
    (T = 2600), or T <= 2 K."""
    assert T - (T - 1) // sp.W * sp.W < 64 or T <= 2 * K
    p, names = sp.ends_panel(T)
    got = sp.run_device(torch, p.x, method, K)
    sp.compare(p.x, got, sp.ends_reference(T, method, K), K, "unfused %s T=%d %s K=%d" % (names, T, method, K))


@pytest.mark.parametrize("method", sp.METHODS)
def test_largest_series(torch, method):
    """T = 16 384, 32 tiles: interior rows of three patterns in tiles 15 / 16 and 28 / 29, and the four
    long gaps test_parity_gpu.py checked at T = 16 000."""
    p = sp.big_panel()
    for K in (0, 60):
        got = sp.run_device(torch, p.x, method, K)
        sp.compare(p.x, got, sp.big_reference(method, K), K, "T=16384 %s K=%d" % (method, K))


@pytest.mark.parametrize("method", sp.METHODS)
def test_rows_per_launch(torch, method):
    """A workgroup holds four independent waves: S = 1, and S % 4 = 1, 2, 3 (the normal panels
    hold 5 rows)."""
    for name in ("n129", "ahead_f255", "edges3", "full_word3"):
        x = sp.panel(name, T_A).x
        for rows in (slice(1, 2), slice(0, 2), slice(1, 4), slice(0, 5)):
            for K in (0, 60):
                got = sp.run_device(torch, x[rows], method, K)
                sp.compare(x[rows], got, sp.reference(name, T_A, method, K), K,
                           "%s rows %s %s K=%d" % (name, rows, method, K), rows=rows)
    x = sp.panel("none", T_A).x
    for K in (0, 20):     # 7 rows: two workgroups, the second with three waves
        x7 = np.concatenate([sp.panel("n65", T_A).x, x[:2]])
        ref = [None if a is None else np.concatenate([a, b[:2]])
               for a, b in zip(sp.reference("n65", T_A, method, K), sp.reference("none", T_A, method, K))]
        sp.compare(x7, sp.run_device(torch, x7, method, K), ref, K, "7 rows %s K=%d" % (method, K))


@pytest.mark.parametrize("method", sp.METHODS)
@pytest.mark.parametrize("tiles", [1, 2, 3])
def test_ab_segment_decompositions(torch, ab_lib, tiles, method):
    """The A/B build with the series cut into segments of 1, 2 or 3 tiles (3: a seam at step 1536, the
    interior odd home): the scan_back start of a segment, a look-ahead tile outside the segment,
    partials + acf_finalize_kernel.  Fills bit-exact, the ACF by the contract."""
    ab_lib(STS_TILE_KERNEL="seg", STS_NO_SHORT="1", STS_SEG_TILES=tiles)
    for name in sp.SUBSET + ["back3", "nan_tile", "chain33_at511", "straddle_33_1", "sparse"]:
        for K in KS:
            check(torch, name, T_A, method, K, what="STS_SEG_TILES=%d " % tiles)
