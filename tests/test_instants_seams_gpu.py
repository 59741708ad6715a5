"""removeInstantsWithNaNs' device chain (csrc/sts_instants.hip) at its seams:

  sts_nan_instants     256 instants per workgroup (512 in the 16-B form: even T and ld, aligned
                       base), groups of 64 series in grid.y
  sts_active_instants  count_active_kernel: blocks of 4 096 instants; scan_counts_kernel: an
                       exclusive scan in groups of 256 blocks with a carry between the groups (the
                       second group starts at T > 4 096 x 256 = 1 048 576); write_active_kernel:
                       passes of 256 instants, ranked by ballot across four waves
  sts_gather_instants  one wave per row, four rows per workgroup, passes of 512 kept instants

Random NaNs put a kept instant on a block, pass or wave edge only by chance, and no other test
gives the compaction more than 18 blocks.  Everything here is index-driven: every comparison is
exact, the references are np.flatnonzero(flags == 0), x[:, active] and the oracle.
"""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

BLOCK, PASS, GROUP = 4096, 256, 256
SEAM = BLOCK * GROUP                     # instants per scan group
T_ALL = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, SEAM - 1, SEAM, SEAM + 1, BLOCK * 513 + 7]
T_FULL = [4097, SEAM + 1, BLOCK * 513 + 7]
SENTINEL = -7.25e77


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------- sts_active_instants on flag arrays ----------------

def _nonzero(T):
    """The values a dropped instant's flag takes: the kernels test !flags[t], not flags[t] == 1."""
    return np.array([1, 2, 255], dtype=np.uint8)[np.arange(T) % 3]


def _keep_where(T, keep):
    f = _nonzero(T)
    f[keep] = 0
    return f


def _rng(T, salt):
    return np.random.default_rng(T * 16 + salt)


FLAG_PATTERNS = {
    "all_kept": lambda T: np.zeros(T, dtype=np.uint8),
    "none_kept": lambda T: _nonzero(T),
    "first_dropped": lambda T: _keep_where(T, np.arange(T) > 0),
    "last_dropped": lambda T: _keep_where(T, np.arange(T) < T - 1),
    "block_edges_kept": lambda T: _keep_where(T, np.isin(np.arange(T) % BLOCK, [0, BLOCK - 1])),
    "wave_edges_kept": lambda T: _keep_where(T, np.isin(np.arange(T) % PASS, [0, 63, 64, 127, 128, 191, 192, 255])),
    "odd_blocks_dropped": lambda T: _keep_where(T, (np.arange(T) // BLOCK) % 2 == 0),
    "first_group_dropped": lambda T: _keep_where(T, np.arange(T) >= SEAM),
    "only_first_group_kept": lambda T: _keep_where(T, np.arange(T) < SEAM),
    "half": lambda T: _keep_where(T, _rng(T, 1).random(T) < 0.5),
    "one_in_1000_dropped": lambda T: _keep_where(T, _rng(T, 2).random(T) >= 0.001),
    "one_in_1000_kept": lambda T: _keep_where(T, _rng(T, 3).random(T) < 0.001),
}
EVERY_T = ["all_kept", "half", "first_dropped", "last_dropped", "block_edges_kept", "wave_edges_kept"]


def test_flag_patterns_hold_what_they_name():
    """No device work: the patterns, at a length past the carry seam."""
    T = SEAM + BLOCK + 5
    t = np.arange(T)
    f = {n: p(T) for n, p in FLAG_PATTERNS.items()}
    assert all(v.dtype == np.uint8 and v.shape == (T,) for v in f.values())
    assert set(np.unique(f["none_kept"])) == {1, 2, 255} and not f["all_kept"].any()
    assert np.array_equal(np.flatnonzero(f["first_dropped"]), [0]) and np.array_equal(np.flatnonzero(f["last_dropped"]), [T - 1])
    kept = np.flatnonzero(f["block_edges_kept"] == 0)
    assert set(kept % BLOCK) == {0, BLOCK - 1} and kept.size == 2 * (T // BLOCK) + 1
    assert set(np.flatnonzero(f["wave_edges_kept"] == 0) % PASS) == {0, 63, 64, 127, 128, 191, 192, 255}
    counts = np.add.reduceat((f["odd_blocks_dropped"] == 0).astype(np.int64), np.arange(0, T, BLOCK))
    assert (counts[1::2] == 0).all() and (counts[0:-1:2] == BLOCK).all()
    assert f["first_group_dropped"][:SEAM].all() and not f["first_group_dropped"][SEAM:].any()
    assert not f["only_first_group_kept"][:SEAM].any() and f["only_first_group_kept"][SEAM:].all()
    assert 0.49 < (f["half"] == 0).mean() < 0.51
    assert 0.0005 < (f["one_in_1000_dropped"] != 0).mean() < 0.002 and 0.0005 < (f["one_in_1000_kept"] == 0).mean() < 0.002
    assert (BLOCK * 513 + 7 + BLOCK - 1) // BLOCK > 2 * GROUP and t[-1] // BLOCK >= GROUP


def active_instants(torch, flags):
    T = flags.size
    fd = torch.as_tensor(flags, device="cuda:0")
    active = torch.full((T,), -7, dtype=torch.int64, device="cuda:0")
    n_dev = torch.full((1,), -7, dtype=torch.int64, device="cuda:0")
    st = lib().sts_active_instants(fd.data_ptr(), T, active.data_ptr(), n_dev.data_ptr(), None)
    assert st == 0, lib().sts_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(fd.cpu().numpy(), flags), "the flags changed"
    return active.cpu().numpy(), int(n_dev.item())


def check_active(torch, name, T):
    flags = FLAG_PATTERNS[name](T)
    want = np.flatnonzero(flags == 0)
    got, n = active_instants(torch, flags)
    what = "%s T=%d" % (name, T)
    assert n == want.size, "%s: n_active %d, expected %d" % (what, n, want.size)
    if not np.array_equal(got[:n], want):
        j = int(np.flatnonzero(got[:n] != want)[0])
        raise AssertionError("%s: %d kept instants differ, first active[%d] = %d, expected %d (block %d, pass %d, lane %d)" % (
            what, int((got[:n] != want).sum()), j, got[j], want[j], want[j] // BLOCK, want[j] % BLOCK // PASS, want[j] % PASS))
    assert (got[n:] == -7).all(), "%s: active[n_active:] written" % what


@pytest.mark.parametrize("T", T_ALL)
def test_active_instants(torch, T):
    for name in (FLAG_PATTERNS if T in T_FULL else EVERY_T):
        check_active(torch, name, T)


# ---------------- sts_nan_instants ----------------

NAN_T = [1, 2, 255, 256, 257, 511, 512, 513, 514, 1025]
NAN_LAYOUTS = ["even_ld", "ld_T_plus_1"]


def nan_ld(lay, T):
    return T + (T & 1) + 2 if lay == "even_ld" else T + 1


def flag_buffer(torch, T, preset=()):
    fl = torch.zeros(T + 128, dtype=torch.uint8, device="cuda:0")
    fl[:64] = 7
    fl[64 + T:] = 7
    for t in preset:
        fl[64 + t] = 1
    return fl


def nan_instants(torch, xd, S, T, ld, fl):
    st = lib().sts_nan_instants(xd.data_ptr(), S, T, ld, fl.data_ptr() + 64, None)
    assert st == 0, lib().sts_last_error()
    h = fl.cpu().numpy()
    assert (h[:64] == 7).all() and (h[64 + T:] == 7).all(), "nan_instants wrote outside flags[0, T)"
    return h[64:64 + T]


@pytest.mark.parametrize("lay", NAN_LAYOUTS)
@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_nan_instants_single_nan(torch, S, lay):
    """One NaN at (s, t), one call per position on fresh flags between two guards: exactly flag t
    is set.  The row padding holds NaN and must never set one."""
    for T in NAN_T:
        ld = nan_ld(lay, T)
        # launch_nan_instants: the 16-B form for even T and even ld on an aligned base, else the 8-B one
        assert ld > T and (T % 2 == 0 and ld % 2 == 0) == (lay == "even_ld" and T % 2 == 0)
        host = np.full((S, ld), np.nan)
        host[:, :T] = np.random.default_rng(S * 2000 + T).standard_normal((S, T))
        xd = torch.as_tensor(host, device="cuda:0")
        assert xd.data_ptr() % 16 == 0
        assert not nan_instants(torch, xd, S, T, ld, flag_buffer(torch, T)).any(), "a flag without a NaN"
        rows = sorted({s for s in (0, 63, 64, S - 1) if 0 <= s < S})
        cols = sorted({t for t in (0, 1, 254, 255, 256, 510, 511, 512, T - 2, T - 1) if 0 <= t < T})
        for s in rows:
            for t in cols:
                keep = float(host[s, t])
                xd[s, t] = float("nan")
                got = nan_instants(torch, xd, S, T, ld, flag_buffer(torch, T))
                xd[s, t] = keep
                assert np.array_equal(np.flatnonzero(got), [t]) and got[t] == 1, (
                    "S=%d T=%d ld=%d NaN at (%d, %d): flags set at %s" % (S, T, ld, s, t, np.flatnonzero(got).tolist()))


@pytest.mark.parametrize("lay", NAN_LAYOUTS)
def test_nan_instants_only_ever_sets(torch, lay):
    """Flags combine by OR: pre-set flags survive a NaN-free panel, two panels give the union."""
    S, T = 65, 514
    ld = nan_ld(lay, T)
    rng = np.random.default_rng(77)
    clean = np.full((S, ld), np.nan)
    clean[:, :T] = rng.standard_normal((S, T))
    preset = (0, 255, 513)
    fl = flag_buffer(torch, T, preset)
    got = nan_instants(torch, torch.as_tensor(clean, device="cuda:0"), S, T, ld, fl)
    assert np.array_equal(np.flatnonzero(got), preset)
    a, b = clean.copy(), clean.copy()
    a[[0, 64, 3], [1, 256, 511]] = np.nan
    b[[63, 64, 7], [256, 512, 2]] = np.nan
    fl = flag_buffer(torch, T)
    nan_instants(torch, torch.as_tensor(a, device="cuda:0"), S, T, ld, fl)
    got = nan_instants(torch, torch.as_tensor(b, device="cuda:0"), S, T, ld, fl)
    assert np.array_equal(np.flatnonzero(got), [1, 2, 256, 511, 512]) and set(got) == {0, 1}


# ---------------- sts_gather_instants ----------------

@pytest.mark.parametrize("S", [1, 3, 4, 5, 9])
def test_gather_instants(torch, S):
    T = 2100
    rng = np.random.default_rng(S)
    x = rng.standard_normal((S, T))
    x[rng.random((S, T)) < 0.01] = np.nan      # NaNs are copied like any other bits
    x[0, 0] = -0.0
    xd = torch.as_tensor(x, device="cuda:0")
    for n in (1, 63, 64, 65, 511, 512, 513, 1024, 1025):
        if n == 1:      # one kept instant cannot be both ends: the last for odd S, the first for even S
            active = np.array([T - 1 if S % 2 else 0], dtype=np.int64)
        else:
            mid = np.sort(rng.choice(np.arange(1, T - 1), size=n - 2, replace=False))
            active = np.concatenate(([0], mid, [T - 1])).astype(np.int64)
        assert active.size == n and (np.diff(active) > 0).all()
        assert n == 1 or (active[0] == 0 and active[-1] == T - 1)
        ld_out = n + 3
        out = torch.full((S, ld_out), SENTINEL, dtype=torch.float64, device="cuda:0")
        ad = torch.as_tensor(active, device="cuda:0")
        st = lib().sts_gather_instants(xd.data_ptr(), out.data_ptr(), S, T, ld_out, ad.data_ptr(), n, None)
        assert st == 0, lib().sts_last_error()
        o = out.cpu().numpy()
        assert np.array_equal(bits(o[:, :n]), bits(x[:, active])), "gather S=%d n=%d" % (S, n)
        assert (o[:, n:] == SENTINEL).all(), "gather S=%d n=%d wrote its padding" % (S, n)
        assert np.array_equal(ad.cpu().numpy(), active) and np.array_equal(bits(xd.cpu().numpy()), bits(x))


# ---------------- the chain, past the carry seam ----------------

def test_chain_past_the_carry_seam(torch):
    """S = 2, T = 4 096 x 256 + 5: 257 blocks, the last one in the scan's second group."""
    from sparkts.timeseriesrdd import TimeSeriesRDD
    S, T = 2, SEAM + 5
    x = np.arange(S * T, dtype=np.float64).reshape(S, T) * 0.5
    x[0, ::3] = np.nan
    x[1, [0, 4095, 4096, SEAM - 1, SEAM, T - 1]] = np.nan
    want, wactive = oracle.remove_instants_with_nans(x)
    assert wactive[-1] >= SEAM and want.shape == (S, wactive.size)
    xd = torch.as_tensor(x, device="cuda:0")
    fl = flag_buffer(torch, T)
    flags = nan_instants(torch, xd, S, T, T, fl)
    assert np.array_equal(flags, np.isnan(x).any(axis=0).astype(np.uint8))
    active, n = active_instants(torch, flags)
    assert n == wactive.size and np.array_equal(active[:n], wactive) and (active[n:] == -7).all()
    out = torch.full((S, n + 3), SENTINEL, dtype=torch.float64, device="cuda:0")
    ad = torch.as_tensor(active[:n], device="cuda:0")
    assert lib().sts_gather_instants(xd.data_ptr(), out.data_ptr(), S, T, n + 3, ad.data_ptr(), n, None) == 0, \
        lib().sts_last_error()
    o = out.cpu().numpy()
    assert np.array_equal(bits(o[:, :n]), bits(want)) and (o[:, n:] == SENTINEL).all()
    # the same through the mirror
    rdd = TimeSeriesRDD(None, ["a", "b"], xd).removeInstantsWithNaNs()
    assert np.array_equal(bits(rdd.data.cpu().numpy()), bits(want))
    assert np.array_equal(np.asarray(rdd.index), wactive)
