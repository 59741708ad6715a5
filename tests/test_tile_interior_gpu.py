"""The tile kernel (sts_tile.hip) runs a chunk of 16 tiles as: the series' first tile in the
general form, a loop of INTERIOR tiles (full 4 096-step tiles away from the series' ends, the row
16-B aligned, the output row null or 16-B aligned: every bound a constant, scalar-base loads and
stores), and the series' last tiles in the general form again.  These panels put the seams of
that split where it can go wrong:

  T = 16 385   the smallest T on the tile kernel: tiles 1, 2 interior, 3 full but too close to
               the end, 4 a single step
  T = 20 480   exactly five tiles (1 .. 3 interior)
  T = 65 536   one full chunk, whose last tile ends the series
  T = 65 537   a second workgroup whose only tile is one step
  T = 69 632   a second workgroup of one full last tile
  T = 130 864  two chunks, the last tile 3 888 steps (the bench shape's)
  row pitch T, T + 2 (even: every row aligned), T + 1 (odd rows unaligned: general form only)
  out null (ACF only), out offset by 8 bytes (general form only)
  K = 20, 60, 61 (2 / 4 shifted MFMAs, the Toeplitz scheme), K = 0 for the four fills, the lag matrix

Every panel has a NaN row first and a +-inf row last, as neighbours of the rows checked.

Expectation: the filled rows have the oracle's bits, the error codes are the oracle's, and the
ACF meets the tolerance contract of tests/test_acf_robust.py and tests/test_parity_gpu.py
(restated below, not loosened): |got - ref| <= 1e-10 |ref| + noise_floor(lag), identical NaN
pattern.
"""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

NaN = float("nan")
TW = 4096
CHUNK = 16 * TW
RTOL = 1e-10
SIZES = [16385, 20480, 65536, 65537, 69632, 2 * CHUNK - 208]
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


# ---- the panel: row 0 NaN, rows 1 .. 4 checked, row 5 +-inf ----

@functools.lru_cache(maxsize=None)
def panel(T):
    rng = np.random.default_rng(T)
    x = np.empty((6, T))
    x[1:5] = 100.0 + np.cumsum(0.01 * rng.standard_normal((4, T)), axis=1)
    x[0] = NaN
    x[5] = np.where(np.arange(T) % 2 == 0, np.inf, -np.inf)
    # row 1: no NaNs.  row 2: 5 % NaN
    m = rng.random(T) < 0.05
    m[:2] = False
    m[-1] = False
    x[2, m] = NaN
    # row 3: a run across a tile seam, a 300-step run inside interior tiles (the long-run chain),
    # a run across the chunk seam
    x[3, 2 * TW - 8:2 * TW + 8] = NaN
    x[3, TW + 1000:TW + 1300] = NaN
    if T > CHUNK + 200:
        x[3, CHUNK - 150:CHUNK + 150] = NaN
    # row 4: leading and trailing runs, and a run across the seam to the last tile
    x[4, :100] = NaN
    x[4, T - 100:] = NaN
    last = (T - 1) // TW * TW
    x[4, last - 20:min(last + 20, T - 200)] = NaN
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(T, method, K):
    x = panel(T)
    if K > 0:
        rf, racf, rerr = oracle.panel_fill_autocorr(x, method, K, threads=4)
        with np.errstate(all="ignore"):
            floor = np.array([noise_floor(r, K) if 1 <= i <= 4 and e == 0 else np.zeros(K)
                              for i, (r, e) in enumerate(zip(rf, rerr))])
    else:
        rf, rerr = oracle.panel_fill(x, method, threads=4)
        racf = floor = None
    return rf, racf, rerr, floor


def run(torch, x, method, K, pitch=0, out="aligned"):
    """fill (+ ACF) with rows `pitch` doubles past T apart; out: "aligned", "off8" (the output
    panel starts 8 bytes past a 16-B boundary) or "null" (method None only)."""
    from sparkts import _native
    from sparkts import UnivariateTimeSeries as uts
    lib = _native.lib()
    S, T = x.shape
    ld = T + pitch
    xd = torch.full((S, ld), 7.0, dtype=torch.float64, device="cuda:0")
    xd[:, :T] = torch.as_tensor(np.array(x), device="cuda:0")
    buf = torch.full((S * ld + 2,), -7.0, dtype=torch.float64, device="cuda:0")
    assert buf.data_ptr() % 16 == 0 and xd.data_ptr() % 16 == 0
    off = 1 if out == "off8" else 0
    outp = None if out == "null" else buf.data_ptr() + 8 * off
    err = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    code = -1 if method is None else uts.fill_method_code(method)
    if K > 0:
        acf = torch.empty((S, K), dtype=torch.float64, device="cuda:0")
        st = lib.sts_fill_autocorr(xd.data_ptr(), outp, S, T, ld, ld, code, K, acf.data_ptr(), err.data_ptr(), None)
    else:
        acf = None
        st = lib.sts_fill(xd.data_ptr(), outp, S, T, ld, ld, code, err.data_ptr(), None)
    assert st == 0, lib.sts_last_error()
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    filled = b[off:off + S * ld].reshape(S, ld)
    if out != "null":
        # nothing written outside the rows: the pitch gap and the words around the panel
        assert (filled[:, T:] == -7.0).all() and (b[:off] == -7.0).all() and (b[off + S * ld - pitch:] == -7.0).all()
    return filled[:, :T], (None if acf is None else acf.cpu().numpy()), err.cpu().numpy()


def check(torch, T, method, K, pitch=0, out="aligned"):
    x = panel(T)
    rf, racf, rerr, floor = reference(T, method, K)
    gf, gacf, gerr = run(torch, x, method, K, pitch, out)
    assert np.array_equal(gerr, rerr), "error codes %s, oracle %s" % (gerr, rerr)
    ok = rerr == 0
    bad = np.flatnonzero(gf[ok].view(np.uint64) != rf[ok].view(np.uint64))
    assert bad.size == 0, "T=%d %s K=%d pitch=%d %s: %d filled values differ, first at flat index %d" % (
        T, method, K, pitch, out, bad.size, bad[0])
    if K > 0:
        rows = [i for i in range(1, 5) if ok[i]]
        with np.errstate(all="ignore"):
            e = within(gacf[rows], racf[rows], floor[rows])
        print("T=%d %s K=%d pitch=%d %s: worst ACF error %.3g x bound" % (T, method, K, pitch, out, e))
        assert e <= 1.0, "T=%d %s K=%d pitch=%d %s: ACF error %.3g x (1e-10 rel + noise floor)" % (
            T, method, K, pitch, out, e)


def test_panel_holds_what_it_claims():
    for T in SIZES:
        x = panel(T)
        assert np.isnan(x[0]).all() and np.isinf(x[5]).all() and not np.isnan(x[1]).any()
        assert 0.03 < np.isnan(x[2]).mean() < 0.07
        assert np.isnan(x[3, 2 * TW - 1]) and np.isnan(x[3, 2 * TW]) and np.isnan(x[3, TW + 1000:TW + 1300]).all()
        if T > CHUNK + 200:
            assert np.isnan(x[3, CHUNK - 1]) and np.isnan(x[3, CHUNK])
        assert np.isnan(x[4, 0]) and np.isnan(x[4, T - 1])
    assert SIZES[-1] % TW == 3888


@pytest.mark.parametrize("pitch", [0, 2, 1])
@pytest.mark.parametrize("T", SIZES)
def test_linear_acf60(torch, T, pitch):
    check(torch, T, "linear", 60, pitch)


@pytest.mark.parametrize("K", [20, 61])
@pytest.mark.parametrize("T", [16385, 69632, 2 * CHUNK - 208])
def test_linear_other_lag_counts(torch, T, K):
    check(torch, T, "linear", K)


@pytest.mark.parametrize("K", [0, 60])
@pytest.mark.parametrize("T", [20480, 65537])
def test_out_offset_by_8_bytes(torch, T, K):
    check(torch, T, "linear", K, 0, "off8")


@pytest.mark.parametrize("K", [20, 60, 61])
@pytest.mark.parametrize("T", [20480, 2 * CHUNK - 208])
def test_out_null_acf_only(torch, T, K):
    """autocorr alone (no fill, no output panel) of the oracle's filled rows."""
    rf, _, _, _ = reference(T, "linear", 60)
    x = np.array(panel(T))
    x[1:5] = rf[1:5]
    x[4, :100] = x[4, 100]          # linear leaves leading / trailing runs NaN
    x[4, T - 100:] = x[4, T - 101]
    _, racf, _ = oracle.panel_fill_autocorr(x, None, K, threads=4)
    _, gacf, _ = run(torch, x, None, K, 0, "null")
    rows = [1, 2, 3, 4]
    floor = np.array([noise_floor(x[i], K) for i in rows])
    e = within(gacf[rows], racf[rows], floor)
    print("T=%d K=%d ACF only: worst error %.3g x bound" % (T, K, e))
    assert e <= 1.0


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("T", [20480, 69632])
def test_four_fills_alone(torch, T, method):
    check(torch, T, method, 0)
    check(torch, T, method, 0, 1)


@pytest.mark.parametrize("include_original", [0, 1])
@pytest.mark.parametrize("T", [20480, 65537])
def test_lag_matrix_10(torch, T, include_original):
    from sparkts import _native
    from sparkts import UnivariateTimeSeries as uts
    lib = _native.lib()
    x = panel(T)
    S, L = x.shape[0], 10
    rf, _, rerr, _ = reference(T, "linear", 0)
    ncols, rows = L + include_original, T - L
    xd = torch.as_tensor(np.array(x), device="cuda:0")
    filled = torch.empty_like(xd)
    lm = torch.full((S * rows * ncols + 2,), -7.0, dtype=torch.float64, device="cuda:0")
    err = torch.zeros(S, dtype=torch.int32, device="cuda:0")
    st = lib.sts_fill_lag_matrix(xd.data_ptr(), filled.data_ptr(), lm.data_ptr(), S, T, T, T,
                                 uts.fill_method_code("linear"), L, include_original, err.data_ptr(), None)
    assert st == 0, lib.sts_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(err.cpu().numpy(), rerr)
    assert np.array_equal(filled.cpu().numpy().view(np.uint64), rf.view(np.uint64))
    got = lm.cpu().numpy()
    assert (got[S * rows * ncols:] == -7.0).all()
    got = got[:S * rows * ncols].reshape(S, ncols, rows)          # column-major per series
    for s in range(S):
        ref = oracle.lag(rf[s], L, bool(include_original)).T        # (ncols, rows)
        assert np.array_equal(got[s].view(np.uint64), np.ascontiguousarray(ref).view(np.uint64)), "series %d" % s
