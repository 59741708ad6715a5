"""The launch paths that only very large S reaches (a grid dimension's 65 535 limit), each at a
tiny T so that the panel stays small.  Needs an MI355X.

  launch_acf_wide's finalize slices         S = 65 541 > 65 535, K = 64       (sts_acf_wide.hip)
  launch_nan_instants' and
  launch_transpose's slices                 S > 64 * 65 535 = 4 194 240       (sts_instants.hip)
  gen_grid's z dimension                    S = 131 073: three z-slices       (sts_gen.hip)
  per_series_grid's slices                  S > 65 535: fill_nan_kernel of sts_observations_to_panel,
                                            wire decode / encode past kRowT = 4096 (sts_ingest.hip)

All but gen_grid walk the series range with for_series_slices (sts_internal.hpp); what differs is the
lambda each hands it.  Each path is a few lines of pointer arithmetic per slice (F + s0 * ld, acf + s0 * K, out + s ...),
where one wrong offset gives plausible numbers: the data is built so that every row's expected
result is known on the device -- a tiling (row s equals row s mod 64 / mod 8), a formula
(x[s, t] = 8 s + t, exact in binary64) or the bit-exact CPU generator -- outputs are pre-filled with
a sentinel, and everything is compared on the device; only the seam rows and the rows checked
against the oracle come to the host.
"""
import numpy as np
import pytest

import oracle
from stream_gate import dev, same_bits, vp
from test_layout_gpu import assert_bits

pytestmark = pytest.mark.gpu

SENT = -3.0e55
GRID_Y = 65535
NaN = np.nan


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


@pytest.fixture(autouse=True)
def report_memory(torch, request):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    print("%s: peak device memory %.0f MB" % (request.node.name, torch.cuda.max_memory_allocated() / 1e6))
    torch.cuda.empty_cache()


def L():
    from sparkts import _native
    return _native.lib()


def ok(status):
    assert status == 0, (status, L().sts_last_error())


def full(torch, shape, dtype=None, value=SENT):
    return torch.full(shape, value, dtype=dtype or torch.float64, device="cuda:0")


def same_or_both_nan(torch, a, b):
    return bool(((a.view(torch.int64) == b.view(torch.int64)) | (torch.isnan(a) & torch.isnan(b))).all())


# ---------------- wide ACF: the finalize and the exact loop in slices of 65 535 series ----------------
ACF_S, ACF_K, TILE = 65541, 64, 64


def acf_base(T, nans):
    """64 distinct series: the nine far-from-level rows of test_acf_robust.py, the two that rule 3
    flags first (rows 0 and 1: once tiled they sit in both slices, the second slice being rows
    63, 0, 1, 2, 3, 4 of the tile), and 55 AR(1) rows"""
    from test_acf_robust import ar1, hard_rows, with_nans
    rng = np.random.default_rng(900 + T)
    hard = hard_rows(T, 40 + T)[[7, 8, 0, 1, 2, 3, 4, 5, 6]]
    x = np.vstack([hard] + [10.0 + ar1(rng, T, 0.9)[None, :] for _ in range(TILE - 9)])
    return with_nans(x, rng) if nans else x


def assert_rule3_on_both_sides(src, T):
    """the restated rule 3 (test_acf_robust.suspect_lags) flags a row of the tile that lands in the
    second slice and one that lands only in the first: the `exact + s0` offset carries flags"""
    if T <= 2 * ACF_K:
        return                                      # the exact loop runs for every row: no flags
    from test_acf_robust import robust_shift, suspect_lags
    with np.errstate(all="ignore"):
        flagged = [bool(suspect_lags(r, ACF_K, robust_shift(r)).any()) for r in src]
    second = [(GRID_Y + i) % TILE for i in range(ACF_S - GRID_Y)]
    assert any(flagged[r] for r in second), flagged
    assert any(f for r, f in enumerate(flagged) if r not in second), flagged


def tiled(torch, base, S):
    reps = (S + base.shape[0] - 1) // base.shape[0]
    return base.repeat(reps, 1)[:S].contiguous()


def assert_tiles(torch, got, what):
    """every row of got equals row s mod 64, bit for bit (on the device); seam rows on failure"""
    want = tiled(torch, got[:TILE], got.shape[0])
    if not same_bits(got, want):
        bad = (got.view(torch.int64) != want.view(torch.int64)).any(dim=1).nonzero().flatten()
        seam = got[GRID_Y - 1:GRID_Y + 2].cpu().numpy()
        raise AssertionError("%s: %d rows differ from row s mod %d, first %s; rows around the seam at %d: %s" % (
            what, bad.numel(), TILE, bad[:5].tolist(), GRID_Y, seam[:, :3].tolist()))


def check_acf_rows(got64, ref, src, what):
    from test_acf_robust import noise_floor, within
    e = within(got64, ref, np.array([noise_floor(r, ACF_K) for r in src]))
    assert e <= 1.0, "%s: error %.3g x (1e-10 rel + noise floor)" % (what, e)


@pytest.mark.parametrize("T", [130, 100])       # T > 2K: acf_wide_kernel + sliced finalize; T <= 2K: sliced exact loop
def test_wide_acf_slices(torch, T):
    S, K = ACF_S, ACF_K
    # sts_autocorr on the raw panel
    base = acf_base(T, False)
    assert_rule3_on_both_sides(base, T)
    x = tiled(torch, dev(torch, base), S)
    acf = full(torch, (S, K))
    ok(L().sts_autocorr(vp(x), S, T, T, K, vp(acf), None))
    torch.cuda.synchronize()
    assert_tiles(torch, acf, "autocorr T=%d" % T)
    check_acf_rows(acf[:TILE].cpu().numpy(), np.array([oracle.autocorr(r, K) for r in base]), base, "autocorr T=%d" % T)
    # sts_fill_autocorr (linear): the filled panel, then the same wide path on it
    base = acf_base(T, True)
    rf, racf, rerr = oracle.panel_fill_autocorr(base, "linear", K)
    assert (rerr == 0).all()
    assert_rule3_on_both_sides(rf, T)
    x = tiled(torch, dev(torch, base), S)
    filled, acf = full(torch, (S, T)), full(torch, (S, K))
    err = full(torch, (S,), torch.int32, -7)
    ok(L().sts_fill_autocorr(vp(x), vp(filled), S, T, T, T, 0, K, vp(acf), vp(err), None))
    torch.cuda.synchronize()
    assert bool((err == 0).all())
    assert_bits(filled[:TILE].cpu().numpy(), rf, "filled rows 0-63")
    assert_tiles(torch, filled, "filled T=%d" % T)
    assert_tiles(torch, acf, "fill_autocorr T=%d" % T)
    check_acf_rows(acf[:TILE].cpu().numpy(), racf, rf, "fill_autocorr T=%d" % T)


# ---------------- NaN instants, gather, transpose past 64 * 65 535 series ----------------
SLICE = 64 * GRID_Y                             # 4 194 240: the first series of the second slice


@pytest.mark.parametrize("S,T", [(SLICE + 130, 6), (SLICE + 131, 5)])     # the 16-byte | the 8-byte kernels
def test_instants_slices(torch, S, T):
    x = (torch.arange(S, dtype=torch.float64, device="cuda:0") * 8.0)[:, None] + torch.arange(
        T, dtype=torch.float64, device="cuda:0")[None, :]
    assert x.is_contiguous() and float(x[S - 1, T - 1]) == 8.0 * (S - 1) + T - 1
    x[5, 1] = NaN
    x[SLICE, 3] = NaN
    x[S - 1, 4] = NaN
    want_flags = [0, 1, 0, 1, 1, 0][:T]
    keep = [t for t in range(T) if not want_flags[t]]
    flags = torch.zeros(T, dtype=torch.uint8, device="cuda:0")           # "zero them first" (sts.h)
    ok(L().sts_nan_instants(vp(x), S, T, T, vp(flags), None))
    active, n_dev = full(torch, (T,), torch.int64, -7), full(torch, (1,), torch.int64, -7)
    ok(L().sts_active_instants(vp(flags), T, vp(active), vp(n_dev), None))
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == want_flags
    n = int(n_dev.item())
    assert n == len(keep) and active[:n].cpu().tolist() == keep
    out = full(torch, (S, n))
    ok(L().sts_gather_instants(vp(x), vp(out), S, T, n, vp(active), n, None))
    torch.cuda.synchronize()
    want = x[:, keep].contiguous()
    assert same_bits(out, want), "gather_instants; rows around the slice seam: %s" % out[SLICE - 1:SLICE + 2].cpu().tolist()
    del out, want
    tr = full(torch, (T, S))
    ok(L().sts_to_instants(vp(x), vp(tr), S, T, T, S, None))
    torch.cuda.synchronize()
    want = x.t().contiguous()
    assert same_bits(tr, want), (
        "to_instants; columns around the slice seam: %s" % tr[:, SLICE - 1:SLICE + 2].cpu().tolist())


# ---------------- generators: three z-slices ----------------

def test_generator_z_slices(torch):
    S, s0 = 2 * GRID_Y + 3, 5
    assert S == 131073
    o = full(torch, (S, 8))
    ok(L().sts_gen_panel(vp(o), s0, S, 8, 8, 123, 0.3, None))
    torch.cuda.synchronize()
    ref = dev(torch, oracle.gen_panel(123, S, 8, 0.3, s0=s0))
    assert bool(torch.isnan(ref).any())
    # bit for bit, a NaN matching any NaN: the project's assert_bits convention (a missing value has
    # no payload to agree on)
    assert same_or_both_nan(torch, o, ref), "gen_panel; rows around the seams: %s" % o[[GRID_Y - 1, GRID_Y, 2 * GRID_Y]].cpu().tolist()
    T, p = 16, 5
    o, c, phi = full(torch, (S, T)), full(torch, (S,)), full(torch, (S, p))
    ok(L().sts_gen_ar_panel(vp(o), vp(c), vp(phi), s0, S, T, T, 77, p, None))
    torch.cuda.synchronize()
    ref = dev(torch, oracle.gen_ar_panel(77, S, T, p, s0=s0))
    assert same_bits(o, ref), "gen_ar_panel; rows around the seams: %s" % o[[GRID_Y - 1, GRID_Y, 2 * GRID_Y]].cpu().tolist()
    # the parameters against the CPU generator at the seams of the three z-slices and on a stride
    rows = sorted({0, 1, GRID_Y - 1, GRID_Y, GRID_Y + 1, 2 * GRID_Y - 1, 2 * GRID_Y, S - 1} | set(range(0, S, 997)))
    want = [oracle.gen_ar_params(77, s0 + s, p) for s in rows]
    assert_bits(c[rows].cpu().numpy(), np.array([w[0] for w in want]), "gen_ar_panel c")
    assert_bits(phi[rows].cpu().numpy(), np.array([w[1] for w in want]), "gen_ar_panel phi")
    assert bool((c == 1.0).all()) and not bool((phi == SENT).any())


# ---------------- observations: the NaN fill in slices of 65 535 series ----------------

def test_observations_slices(torch):
    S, T, n = ACF_S, 3, 4000
    rng = np.random.default_rng(11)
    sid = rng.integers(0, GRID_Y, n).astype(np.int32)
    loc = rng.integers(0, T, n).astype(np.int64)
    # 600 observations in the second slice (six series): its last series and its column 0 get none,
    # so 8 of its 18 cells keep the NaN that only the second launch of fill_nan_kernel writes
    sid[:600] = rng.integers(GRID_Y, S - 1, 600)
    loc[:600] = rng.integers(1, T, 600)
    sid[600:620] = -1 - rng.integers(0, 5, 20)               # negative ids
    loc[620:660] = -1 - rng.integers(0, 3, 40)               # not in the index
    loc[660:700] = T + rng.integers(0, 3, 40)                # past the end
    sid[700:740], loc[700:740] = GRID_Y, 1                   # duplicates of one cell, at the seam
    sid[740:780], loc[740:780] = 1234, 2                     # and of one in the first slice
    val = rng.standard_normal(n)
    assert (sid >= GRID_Y).sum() >= 500
    ref = np.full((S, T), NaN)                               # a NaN panel, the last writer wins
    for i in range(n):
        if 0 <= sid[i] < S and 0 <= loc[i] < T:
            ref[sid[i], loc[i]] = val[i]
    assert np.isnan(ref[GRID_Y:]).sum() >= 8 and (~np.isnan(ref[GRID_Y:])).sum() >= 8
    o = full(torch, (S, T))
    sd, ld, vd = dev(torch, sid, np.int32), dev(torch, loc, np.int64), dev(torch, val)
    ok(L().sts_observations_to_panel(vp(sd), vp(ld), vp(vd), n, vp(o), S, T, T, None))
    torch.cuda.synchronize()
    got = o.cpu().numpy()
    assert_bits(got, ref, "observations")
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and not (got[GRID_Y - 2:] == SENT).any()


# ---------------- wire decode / encode: the per-series grid in slices (the one test that needs GBs) ----------------

def test_wire_slices(torch):
    """S = 65 544 records of T = 4097 values (one past kRowT): a 2.15 GB panel and as large an
    encoded buffer, allocated, run and freed here (peak 4.6 GB with the comparison masks)."""
    S, T, R = 65544, 4097, 8
    rng = np.random.default_rng(5)
    x = rng.standard_normal((R, T)) * 1e3
    x.ravel()[rng.random(R * T) < 0.05] = NaN
    x[0, 0] = -0.0
    blocks = x.astype(">f8").view(np.uint8).reshape(R, 8 * T)
    # 8 records back to back, records 2 and 5 at offsets = 4 mod 8 (the byte-load form)
    off, pos = [], 0
    for i in range(R):
        pos += ((4 if i in (2, 5) else 0) - pos) % 8
        off.append(pos)
        pos += 8 * T + 3                                     # a few header bytes in between
    assert all(b >= a + 8 * T for a, b in zip(off, off[1:])) and [o % 8 for o in off] == [0, 0, 4, 0, 0, 4, 0, 0]
    data = np.full(off[-1] + 8 * T, 0x5A, np.uint8)
    for i, o in enumerate(off):
        data[o:o + 8 * T] = blocks[i]
    raw = dev(torch, data, np.uint8)
    val_off = dev(torch, np.array(off, np.int64)[np.arange(S) % R], np.int64)
    panel = full(torch, (S, T))
    ok(L().sts_wire_decode(vp(raw), vp(val_off), S, T, vp(panel), T, None))
    torch.cuda.synchronize()
    rows = dev(torch, x)
    assert S % R == 0
    same = panel.view(S // R, R, T).view(torch.int64) == rows.view(torch.int64)[None]
    assert bool(same.all()), "wire_decode: rows %s differ from record s mod 8" % (
        (~same).any(dim=2).nonzero()[:5].tolist())
    del same
    # encode into a fresh buffer, one block per series, distinct and increasing offsets
    enc_off = torch.arange(S, dtype=torch.int64, device="cuda:0") * (8 * T)
    enc = full(torch, (S * 8 * T,), torch.uint8, 0xA5)
    ok(L().sts_wire_encode(vp(panel), S, T, T, vp(enc_off), vp(enc), None))
    torch.cuda.synchronize()
    want = dev(torch, blocks, np.uint8).view(torch.int64)    # (8, T) words of the records' value bytes
    same = enc.view(torch.int64).view(S // R, R, T) == want[None]
    assert bool(same.all()), "wire_encode: blocks %s differ from the records' value bytes" % (
        (~same).any(dim=2).nonzero()[:5].tolist())
    del same, enc, panel
