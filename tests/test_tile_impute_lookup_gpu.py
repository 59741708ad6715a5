"""The tile kernel's imputation phase (sts_tile.hip, phase 4) finds the word of NaN-list entry idx
with a two-level count over the word offsets (wcoarse: every 8th word; then the 8 entries of that
group) instead of a binary search.  These panels put the NaNs where that lookup can go wrong:
list lengths around the 256 threads of a workgroup, NaNs only in the first / last word, only in
coarse groups 0 and 8, only in the ACF's look-ahead reach, a fully-NaN word (the offsets jump by
64), runs across tile and chunk boundaries, long-run chains, whole-NaN tiles, the series' ends.

T = 20 480 is 5 tiles of 4 096 (edge, 3 interior register-prefetched, edge); T = 69 700 is 18
tiles, i.e. two 16-tile workgroups per series with the ACF (a chunk boundary at step 65 536, and
the cached slow-path scans).  Both are above the 16 384 switch to the tile kernel.

Expectation: the filled panel has the oracle's bits, the error codes are the oracle's, and the
ACF meets the tolerance contract of tests/test_acf_robust.py (restated below, not loosened):
|got - ref| <= 1e-10 |ref| + noise_floor(lag), identical NaN pattern.
"""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

NaN = float("nan")
TW, HB = 4096, 64          # tile width, look-back halo: tile k's word w holds steps 4096 k - 64 + 64 w ...
RTOL = 1e-10
METHODS = ["linear", "previous", "next", "nearest"]


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


# ---- the tolerance contract of tests/test_acf_robust.py (noise_floor / within), restated ----

def noise_floor(x, K):
    x = np.asarray(x, dtype=np.float64)
    T = x.size
    out = np.zeros(K)
    for i in range(1, K + 1):
        a, b = x[i:], x[:T - i]
        d1, d2 = a - a.mean(), b - b.mean()
        den = np.sqrt((d1 * d1).sum()) * np.sqrt((d2 * d2).sum())
        out[i - 1] = 64 * np.finfo(float).eps * np.sqrt(T - i) * np.abs(d1 * d2).sum() / den if den > 0 else 0.0
    return out


def within(got, ref, floor):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs"
    fin = ~np.isnan(ref)
    if not fin.any():
        return 0.0
    diff = np.abs(got[fin] - ref[fin])
    den = RTOL * np.abs(ref[fin]) + floor[fin]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(diff == 0.0, 0.0, diff / den).max())


# ---- NaN patterns: step offsets relative to the first step of a tile (negative: its look-back) ----

def spaced(n):
    """n isolated NaNs inside the tile (every third step from offset 8)."""
    return [8 + 3 * i for i in range(n)]


PATTERNS = {
    "one": [1808],
    "n255": spaced(255),
    "n256": spaced(256),
    "n257": spaced(257),
    # word 1 of the extended tile = the tile's first 64 steps; word 64 = its last 64
    "first_word": [0, 1, 2, 3, 10] + list(range(20, 30)) + [63],
    "last_word": [TW - 64 + o for o in [0, 5, 6, 7] + list(range(40, 51)) + [62, 63]],
    # the ACF's reach past the written range (80 steps), and one step past it (clipped by need())
    "lookahead": [TW + 2] + list(range(TW + 12, TW + 16)) + [TW + 72, TW + 79, TW + 82],
    # coarse group 0 = words 0..7 (offsets -64 .. 447), group 8 = words 64..67
    "groups_0_8": [-3, 5, 70, 71, 200, 440, 447] + [TW - 64 + 9, TW - 1, TW + 1, TW + 70],
    # word 10 (offsets 576 .. 639) all NaN, then single NaNs: the word offsets jump by 64
    "full_word": list(range(576, 640)) + [648, 650, 700, 703, 900, 2000, 4000],
    "run_tile_edge": list(range(TW - 8, TW + 8)),
    "run40": list(range(808, 848)),
    "run300": list(range(TW - 188, TW + 112)),     # longer than both halos
    "nan_tile": list(range(0, TW)),
}
SUBSET = ["n256", "n257", "groups_0_8", "full_word", "run300", "iid30"]


def base_rows(S, T, seed):
    rng = np.random.default_rng(seed)
    x = 100.0 + np.cumsum(0.01 * rng.standard_normal((S, T)), axis=1)
    x[:, 900:1400] = x[:, 900:901]       # a plateau: linear increments of exactly 0
    return x


@functools.lru_cache(maxsize=None)
def panel(name, T):
    """4 series: the pattern in an interior tile, in the first tile, in the last (clipped at
    T), and in every second tile at once (so it also sits next to the chunk boundary)."""
    ntiles = (T + TW - 1) // TW
    if name in ("iid5", "iid30"):
        return oracle.gen_panel(7 if name == "iid5" else 8, 4, T, 0.05 if name == "iid5" else 0.30)
    if name == "none":
        return base_rows(3, T, 1)
    if name == "ends":
        x = base_rows(4, T, 2)
        x[0, :100] = NaN                 # leading run
        x[1, T - 100:] = NaN             # trailing run
        x[2, :5000] = NaN                # leading / trailing runs longer than a tile
        x[2, T - 5000:] = NaN
        x[3, 1:] = NaN                   # only x[0] valid: fillNearest's "all NaNs" error
        return x
    if name == "chunk_run300":           # across the tile AND chunk boundary at step 16 x 4096
        x = base_rows(3, T, 3)
        edge = 16 * TW if T > 16 * TW else 3 * TW
        x[0, edge - 136:edge + 164] = NaN
        x[1, edge - 299:edge + 1] = NaN
        x[2, edge - 1:edge + 299] = NaN
        return x
    if name == "extreme":                # increments outside [2^-900, 2^700], zero and tiny ones
        x = oracle.gen_panel(9, 4, T, 0.05)
        x[0] = np.where(np.arange(T) % 2 == 0, 1e250, -1e250) * np.where(np.isnan(x[0]), NaN, 1.0)
        x[1] = x[1] * 1e-300
        x[2] = np.where(np.isnan(x[2]), NaN, 3.0)
        x[3] = x[3] * 4e-320
        return x
    offs = np.array(PATTERNS[name])
    x = base_rows(4, T, len(name) + 10 * len(offs))
    homes = [[2], [0], [ntiles - 1], list(range(1, ntiles, 2))]
    for row, tiles in enumerate(homes):
        for k in tiles:
            t = k * TW + offs
            t = t[(t >= 0) & (t < T)]
            x[row, t] = NaN
    return x


def run(torch, x, method, K):
    from sparkts import _native
    from sparkts import UnivariateTimeSeries as uts
    lib = _native.lib()
    S, T = x.shape
    xd = torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")
    filled = torch.empty_like(xd)
    err = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    code = uts.fill_method_code(method)
    if K > 0:
        acf = torch.empty((S, K), dtype=torch.float64, device="cuda:0")
        st = lib.sts_fill_autocorr(xd.data_ptr(), filled.data_ptr(), S, T, T, T, code, K, acf.data_ptr(),
                                   err.data_ptr(), None)
    else:
        acf = None
        st = lib.sts_fill(xd.data_ptr(), filled.data_ptr(), S, T, T, T, code, err.data_ptr(), None)
    assert st == 0, lib.sts_last_error()
    torch.cuda.synchronize()
    return filled.cpu().numpy(), (None if acf is None else acf.cpu().numpy()), err.cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(name, T, method, K):
    x = panel(name, T)
    if K > 0:
        rf, racf, rerr = oracle.panel_fill_autocorr(x, method, K, threads=4)
        floor = np.array([noise_floor(r, K) if e == 0 else np.zeros(K) for r, e in zip(rf, rerr)])
    else:
        rf, rerr = oracle.panel_fill(x, method, threads=4)
        racf = floor = None
    return rf, racf, rerr, floor


def check(torch, name, T, method, K):
    x = panel(name, T)
    rf, racf, rerr, floor = reference(name, T, method, K)
    gf, gacf, gerr = run(torch, x, method, K)
    assert np.array_equal(gerr, rerr), "error codes %s, oracle %s" % (gerr, rerr)
    ok = rerr == 0
    bad = np.flatnonzero(gf[ok].view(np.uint64) != rf[ok].view(np.uint64))
    assert bad.size == 0, "%s T=%d %s K=%d: %d filled values differ, first at flat index %d" % (
        name, T, method, K, bad.size, bad[0])
    if K > 0 and ok.any():
        with np.errstate(all="ignore"):
            e = within(gacf[ok], racf[ok], floor[ok])
        assert e <= 1.0, "%s T=%d %s K=%d: ACF error %.3g x (1e-10 rel + noise floor)" % (name, T, method, K, e)


def test_patterns_hold_what_they_claim():
    """The counted patterns put exactly that many NaNs into the interior tile's list range
    [tile start, tile end + reach), and the word patterns sit in the words they name."""
    for n in (255, 256, 257):
        x = panel("n%d" % n, 20480)
        assert int(np.isnan(x[0, 2 * TW:3 * TW + 80]).sum()) == n
        assert int(np.isnan(x[0]).sum()) == n
    words = lambda name: set((np.array(PATTERNS[name]) + HB) // 64)   # noqa: E731
    assert words("first_word") == {1} and words("last_word") == {64}
    assert words("lookahead") == {65, 66}
    assert all(w < 8 or w >= 64 for w in words("groups_0_8")) and {0, 7, 64, 66} <= words("groups_0_8")
    assert np.isnan(panel("nan_tile", 20480)[0, 2 * TW:3 * TW]).all()


ALL = ["none", "ends", "chunk_run300", "iid5", "iid30"] + list(PATTERNS)


@pytest.mark.parametrize("T", [20480, 69700])
@pytest.mark.parametrize("name", ALL)
def test_linear_acf60_every_pattern(torch, name, T):
    check(torch, name, T, "linear", 60)


@pytest.mark.parametrize("K", [0, 20])
@pytest.mark.parametrize("name", SUBSET + ["ends", "chunk_run300", "nan_tile", "run40"])
def test_linear_fill_only_and_acf20(torch, name, K):
    check(torch, name, 69700 if name == "chunk_run300" else 20480, "linear", K)


@pytest.mark.parametrize("K", [0, 20, 60])
@pytest.mark.parametrize("method", ["previous", "next", "nearest"])
@pytest.mark.parametrize("name", SUBSET + ["ends"])
def test_other_fills_subset(torch, name, method, K):
    check(torch, name, 20480, method, K)


@pytest.mark.parametrize("method", METHODS)
def test_other_fills_chunk_boundary(torch, method):
    check(torch, "chunk_run300", 69700, method, 60)


def test_linear_extreme_increments(torch):
    """fill('linear') increments that are 0, subnormal, tiny and > 2^700: the division of the
    increment has the oracle's bits for every numerator."""
    check(torch, "extreme", 20480, "linear", 0)
