"""include/sts_roll.h on the device: sts_roll_stat / sts_roll_pair (csrc/sts_roll.hip) against the numpy
restatement of the header's definition (tests/roll_ref.py, which tests/test_roll_cpu.py holds to exact
arithmetic), at every seam of the kernel, beside poisoned rows, in awkward layouts, behind a delayed
stream and through the `_host` twins.

Bars.  SUM, MEAN, VAR, MIN, MAX, COV and BETA: bit for bit (a NaN must be a NaN in the same place; the
sign and payload of a NaN that arithmetic made differ between processors and are not compared).  STD,
ZSCORE and CORR: within 4 units of the last place, NaN positions exact and |CORR| <= 1: each sqrt may
be off by 1 ulp, and CORR puts two of them through one product and one quotient.

Seams.  STS_ROLL_TILE and STS_ROLL_MAX_WINDOW are read from the header.  A workgroup owns TILE steps
of one row, or R = (TILE + MAX_WINDOW - 1) // (T + window - 1) whole rows when T <= TILE (rows()
below restates the header's formula); a launch holds 65 535 workgroups along the series, so the
launch loop first turns at S > 65 535 R.  TILE - 1, TILE and TILE + 1 exceed the window cap and are
pruned from the windows; 1023 stands in beside 1024.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import layout_arena as la
import roll_ref as rr
import stream_gate as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sts_roll.h")).read()
TILE, MAXW = (int(re.search(r"#define STS_ROLL_%s (\d+)" % n, HEADER).group(1)) for n in ("TILE", "MAX_WINDOW"))
CAP = TILE + MAXW - 1
EXACT_OPS = ("sum", "mean", "var", "min", "max", "cov", "beta")
ULP_OPS = ("std", "zscore", "corr")
ALL_OPS = rr.OPS + rr.PAIR_OPS
ULPS = 4
POISON_OUT = -3.0e55
WINDOWS = sorted(w for w in {1, 2, 3, 7, 64, TILE - 1, TILE, TILE + 1, MAXW - 1, MAXW} if w <= MAXW)
T_LONG = 2 * TILE + 3


def rows(T, w):
    """rows per workgroup, the header's formula"""
    return CAP // (T + w - 1) if T <= TILE else 1


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


@pytest.fixture(scope="module")
def delay(torch):
    return sg.calibrate(torch)[0]


def lib():
    from sparkts import _native
    return _native.lib()


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def hv(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def dev(torch, a):
    return torch.as_tensor(np.array(a, dtype=np.float64, order="C"), device="cuda:0")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """strictly the same bits: two device results"""
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def noise(seed, S, T):
    return np.random.default_rng([78, seed, S, T]).standard_normal((S, T))


def holes(x, seed, p=0.05):
    x = x.copy()
    x[np.random.default_rng([79, seed]).random(x.shape) < p] = np.nan
    return x


def run(torch, x, op, w, mp=None, y=None, host=False):
    """one call on packed panels -> numpy (S, T); x / y numpy or device tensors, y (S, T) or (T,)"""
    mp = w if mp is None else mp
    L = lib()
    pair = op in rr.PAIR_OPS
    code = (rr.PAIR_OPS if pair else rr.OPS).index(op)
    S, T = x.shape
    Sy = 0 if y is None else (1 if len(y.shape) == 1 else y.shape[0])
    if host:
        x = np.ascontiguousarray(x)
        out = np.full((S, T), POISON_OUT)
        if pair:
            y = np.ascontiguousarray(y)
            st = L.sts_roll_pair_host(hv(x), hv(y), Sy, T, hv(out), S, T, T, w, mp, code)
        else:
            st = L.sts_roll_stat_host(hv(x), hv(out), S, T, T, w, mp, code)
        assert st == 0, L.sts_last_error()
        return out
    dx = x if hasattr(x, "data_ptr") else dev(torch, x)
    out = torch.full((S, T), POISON_OUT, dtype=torch.float64, device="cuda:0")
    if pair:
        dy = y if hasattr(y, "data_ptr") else dev(torch, y)
        st = L.sts_roll_pair(vp(dx), vp(dy), Sy, T, vp(out), S, T, T, T, w, mp, code, None)
    else:
        st = L.sts_roll_stat(vp(dx), vp(out), S, T, T, T, w, mp, code, None)
    assert st == 0, L.sts_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_all(torch, x, y, w, mp, ops=ALL_OPS, host=False):
    dx, dy = (x, y) if host else (dev(torch, x), None if y is None else dev(torch, y))
    return {op: run(torch, dx, op, w, mp, dy if op in rr.PAIR_OPS else None, host) for op in ops}


def ref_all(x, y, w, mp, ops=ALL_OPS):
    """the restatement of every op, the window passes made once for the single ops and once for the pairs"""
    out = {}
    if any(op in rr.OPS for op in ops):
        m = rr.moments(x, w)
        out.update({op: rr.stat(x, op, w, mp, m) for op in ops if op in rr.OPS})
    if any(op in rr.PAIR_OPS for op in ops):
        m = rr.moments(x, w, y)
        out.update({op: rr.pair(x, y, op, w, mp, m) for op in ops if op in rr.PAIR_OPS})
    return out


def check(got, want, op, what=""):
    assert got.shape == want.shape
    assert not (got == POISON_OUT).any(), (what, op, "an output was not written")
    if op in EXACT_OPS:
        assert rr.same_bits(got, want), (what, op, "differs at", np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4])
    else:
        d = rr.ulp_diff(got, want)
        assert d <= ULPS, (what, op, d)
        if op == "corr" and not np.isnan(got).all():
            assert np.nanmax(np.abs(got)) <= 1.0


def check_all(got, want, what=""):
    for op in got:
        check(got[op], want[op], op, what)


# ---------------- every op at every window ----------------

@functools.lru_cache(maxsize=None)
def long_panel():
    x = holes(noise(1, 3, T_LONG), 1, 0.01)
    y = holes(noise(2, 3, T_LONG), 2, 0.01)
    x[2, 100:140] = 0.1                        # constant windows for the small windows
    x[1, 7], x[1, 8] = 0.0, -0.0
    return x, y


@pytest.mark.parametrize("w", WINDOWS)
def test_every_op_at_every_window(torch, w):
    x, y = long_panel()
    mp = (w + 1) // 2
    got, want = run_all(torch, x, y, w, mp), ref_all(x, y, w, mp)
    check_all(got, want, "w=%d" % w)
    exact = [op for op in ULP_OPS if rr.same_bits(got[op], want[op])]
    print("w=%d: bit-equal among the 4-ulp ops: %s" % (w, exact))


# ---------------- lengths and counts ----------------

def lengths(w):
    return sorted(T for T in {1, w - 1, w, w + 1, TILE - 1, TILE, TILE + 1, T_LONG} if T >= 1)


LENGTH_CASES = [(w, T) for w in (1, 7, 64, MAXW) for T in lengths(w)]


@pytest.mark.parametrize("w,T", LENGTH_CASES)
def test_lengths_and_series_counts(torch, w, T):
    """T either side of the window and of the tile; S = 1 and either side of the rows a workgroup
    owns.  The reference is made once for the largest S; a row's results do not depend on S."""
    R = rows(T, w)
    counts = sorted({1, max(R - 1, 1), R, R + 1})
    if T == T_LONG:
        counts = [1, 2]
    S_top = counts[-1]
    x, y = holes(noise(3, S_top, T), 3), holes(noise(4, S_top, T), 4)
    mp = min(w, 2)
    want = ref_all(x, y, w, mp)
    for S in counts:
        got = run_all(torch, x[:S], y[:S], w, mp)
        check_all(got, {op: v[:S] for op, v in want.items()}, "w=%d T=%d S=%d R=%d" % (w, T, S, R))


def test_more_series_than_one_launch_holds(torch):
    """S = 70 000 x T = 8, and the smallest panel at which the launch loop turns: two rows per
    workgroup at window 1024 and T = 4, so S = 2 x 65 535 + 3.  Every window there is the whole prefix
    of its row, which the restatement evaluates at window T."""
    for S, T, w in ((70000, 8, 3), (2 * 65535 + 3, 4, MAXW)):
        assert w < T or S > 65535 * rows(T, w)
        x, y = holes(noise(5, S, T), 5, 0.1), noise(6, T, 1)[:, 0]
        ops = ("sum", "var", "max", "zscore", "beta")
        got, want = run_all(torch, x, y, w, 1, ops), ref_all(x, y, min(w, T), 1, ops)
        check_all(got, want, "S=%d" % S)


# ---------------- NaNs ----------------

@pytest.mark.parametrize("w", [3, 64])
def test_nans_at_the_tile_seam_runs_and_an_empty_row(torch, w):
    offs = [-2, -1, 0, 1, 2]
    x = noise(7, len(offs) + 3, T_LONG)
    for i, o in enumerate(offs):
        x[i, TILE + o] = np.nan                                  # one NaN at each offset around the seam
    x[5, TILE - w - 5:TILE + 9] = np.nan                         # a run longer than the window, across the seam
    x[5, 20:20 + 2 * w] = np.nan
    x[6] = np.nan                                                # an empty row
    x[7, :w + 3] = np.nan                                        # missing from the start
    y = noise(8, x.shape[0], T_LONG)
    y[0, TILE - 1] = np.nan                                      # pairwise validity
    for mp in sorted({1, (w + 1) // 2, w}):
        got, want = run_all(torch, x, y, w, mp), ref_all(x, y, w, mp)
        check_all(got, want, "w=%d mp=%d" % (w, mp))
        for op in ALL_OPS:
            assert np.isnan(got[op][6]).all()
            assert np.isnan(got[op][5, TILE - 5:TILE + 9]).all()


# ---------------- infinities and poisoned neighbours ----------------

@pytest.mark.parametrize("bad", [np.inf, -np.inf])
def test_an_infinity_costs_its_own_windows_only(torch, bad):
    x, y = noise(9, 2, TILE + 40), noise(10, 2, TILE + 40)
    xi = x.copy()
    pos = TILE - 3
    xi[0, pos] = bad
    for w in (1, 5, 64):
        hit = np.zeros(x.shape, dtype=bool)
        hit[0, pos:pos + w] = True
        clean, dirty = run_all(torch, x, y, w, w), run_all(torch, xi, y, w, w)
        swapped = run_all(torch, y, xi, w, w, rr.PAIR_OPS)
        swapped_clean = run_all(torch, y, x, w, w, rr.PAIR_OPS)
        check_all(dirty, ref_all(xi, y, w, w), "inf w=%d" % w)
        for op in ALL_OPS:
            assert same(clean[op][~hit], dirty[op][~hit]), (op, w)
        for op in rr.PAIR_OPS:
            assert same(swapped[op][~hit], swapped_clean[op][~hit]), (op, w)
            assert np.isnan(dirty[op][hit]).all() and np.isnan(swapped[op][hit]).all()
        assert (dirty["sum"][hit] == bad).all() and (dirty["max" if bad > 0 else "min"][hit] == bad).all()


@pytest.mark.parametrize("T", [24, 390])
def test_poisoned_neighbours_change_no_bit(torch, T):
    """rows of NaN, of infinities and of 1e308 (whose sums overflow) between the clean rows, in the
    same wave (T = 24: a wave spans three rows) and the same workgroup"""
    w = 5
    clean = holes(noise(11, 6, T), 11)
    yc = noise(12, 6, T)
    S = 12
    x, y = np.empty((S, T)), np.empty((S, T))
    x[0::2], y[0::2] = clean, yc
    x[1], x[3], x[5], x[7], x[9], x[11] = np.nan, np.inf, 1e308, -np.inf, -1e308, np.nan
    y[1::2] = x[1::2][::-1]
    assert rows(T, w) >= 7
    alone, mixed = run_all(torch, clean, yc, w, 2), run_all(torch, x, y, w, 2)
    for op in ALL_OPS:
        assert same(alone[op], mixed[op][0::2]), op
    check_all(mixed, ref_all(x, y, w, 2), "poisoned neighbours")


# ---------------- layout ----------------

@pytest.mark.parametrize("pname", list(la.POISONS))
@pytest.mark.parametrize("lay", la.LAYOUT_NAMES)
@pytest.mark.parametrize("T", [390, TILE + 5])
def test_layout(torch, T, lay, pname):
    """ld_in != ld_out > T with poisoned gaps that survive, bases that are 8-byte but not 16-byte
    aligned, red zones around the output, the inputs unchanged: the packed call's bits"""
    pv = la.POISONS[pname]
    S, w, mp = 5, 20, 3
    x, y = holes(noise(13, S, T), 13), noise(14, S, T)
    ld_x, ld_o, bi, bo = la.layout(lay, T)
    for op in ("mean", "zscore", "min", "corr"):
        pair = op in rr.PAIR_OPS
        want = run(torch, x, op, w, mp, y if pair else None)
        ax = la.carve(S, T, ld_x, bi, pv, data=x)
        ay = la.carve(S, T, ld_x + 3, (bi + 1) % 16, pv, data=y) if pair else None
        ao = la.carve(S, T, ld_o, bo, la.OUT_FILL)
        ins = [a for a in (ax, ay) if a is not None]
        snaps, snap_o = [a.snapshot() for a in ins], ao.snapshot()
        P = ctypes.c_void_p
        if pair:
            st = lib().sts_roll_pair(P(ax.ptr), P(ay.ptr), S, ld_x + 3, P(ao.ptr), S, T, ld_x, ld_o, w, mp,
                                     rr.PAIR_OPS.index(op), None)
        else:
            st = lib().sts_roll_stat(P(ax.ptr), P(ao.ptr), S, T, ld_x, ld_o, w, mp, rr.OPS.index(op), None)
        assert st == 0, lib().sts_last_error()
        torch.cuda.synchronize()
        assert same(ao.data(), want), (op, lay)
        ao.verify_outside(snap_o)
        for a, s in zip(ins, snaps):
            a.verify_all(s)


# ---------------- purity across placements ----------------

def test_the_same_row_elsewhere_gives_the_same_bits(torch):
    w, mp = 20, 5
    row, yrow = holes(noise(15, 1, 300), 15)[0], noise(16, 1, 300)[0]
    base = run_all(torch, row[None], yrow[None], w, mp)
    # at another t offset: behind k missing steps, and behind k steps of data (the windows that do
    # not reach them), across the tile seam
    k = TILE - 100
    for front in (np.full(k, np.nan), noise(17, 1, k)[0]):
        x2, y2 = np.concatenate([front, row])[None], np.concatenate([noise(18, 1, k)[0], yrow])[None]
        far = run_all(torch, x2, y2, w, mp)
        lo = 0 if np.isnan(front).all() else w - 1
        for op in ALL_OPS:
            assert same(far[op][0, k + lo:], base[op][0, lo:]), op
    # under another S, among other rows, after a permutation
    S = 2 * rows(300, w) + 3
    x, y = holes(noise(19, S, 300), 19), noise(20, S, 300)
    x[S - 2], y[S - 2] = row, yrow
    full = run_all(torch, x, y, w, mp)
    perm = np.random.default_rng(21).permutation(S)
    shuffled = run_all(torch, x[perm], y[perm], w, mp)
    for op in ALL_OPS:
        assert same(full[op][S - 2], base[op][0]), op
        assert same(shuffled[op], full[op][perm]), op
    # under another ld: covered with the packed call's bits by test_layout


def test_shared_factor_equals_its_copies_and_the_host_path(torch):
    S, T, w, mp = 2 * rows(390, 20) + 1, 390, 20, 10
    x, f = holes(noise(22, S, T), 22), holes(noise(23, 1, T), 23, 0.02)[0]
    shared = run_all(torch, x, f, w, mp, rr.PAIR_OPS)
    copies = run_all(torch, x, np.tile(f, (S, 1)), w, mp, rr.PAIR_OPS)
    host_shared = run_all(torch, x, f, w, mp, rr.PAIR_OPS, host=True)
    host_copies = run_all(torch, x, np.tile(f, (S, 1)), w, mp, rr.PAIR_OPS, host=True)
    for op in rr.PAIR_OPS:
        assert same(shared[op], copies[op]) and same(shared[op], host_shared[op]) and same(shared[op], host_copies[op]), op
    single = run_all(torch, x, None, w, mp, rr.OPS)
    host_single = run_all(torch, x, None, w, mp, rr.OPS, host=True)
    for op in rr.OPS:
        assert same(single[op], host_single[op]), op
    check_all(shared, ref_all(x, f, w, mp, rr.PAIR_OPS), "shared factor")


# ---------------- the hard families ----------------

@pytest.mark.parametrize("name", ["walk_1e9", "walk_1e9_fine", "scaled_up", "scaled_down", "ulps_1e9", "flat_jumps"])
def test_hard_families(torch, name):
    x = rr.family(name, T_LONG, S=2)
    y = rr.family(name, T_LONG, S=2, seed=1)
    for w in (20, 252):
        got, want = run_all(torch, x, y, w, w), ref_all(x, y, w, w)
        check_all(got, want, "%s w=%d" % (name, w))
        if name == "flat_jumps" and w == 20:
            v = got["var"][:, w - 1:]
            assert (v == 0).any() and not np.signbit(v[v == 0]).any()


# ---------------- stream order ----------------

def _gate_case(torch, pair):
    S, T, w, mp = 9, TILE + 300, 64, 8
    gx = sg.GIn(torch, *[holes(noise(s, S, T), s) for s in (30, 31, 32)])
    gy = sg.GIn(torch, *[noise(s, 1, T)[0] for s in (33, 34, 35)]) if pair else None
    out = torch.empty((S, T), dtype=torch.float64, device="cuda:0")
    op = "beta" if pair else "zscore"

    def call(st):
        if pair:
            return lib().sts_roll_pair(vp(gx.buf), vp(gy.buf), 1, 0, vp(out), S, T, T, T, w, mp, rr.PAIR_OPS.index(op), st)
        return lib().sts_roll_stat(vp(gx.buf), vp(out), S, T, T, T, w, mp, rr.OPS.index(op), st)

    def check_(outs, host):
        x = gx.real.cpu().numpy()
        y = gy.real.cpu().numpy() if pair else None
        check(outs[0], ref_all(x, y, w, mp, (op,))[op], op, "gated")
    return sg.Case([g for g in (gx, gy) if g], [out], call, check_)


@pytest.mark.parametrize("pair", [False, True], ids=["stat", "pair"])
def test_gated_call_is_stream_ordered(torch, delay, pair):
    """The `void* stream` entry points of sts_roll.h behind a delayed stream (tests/stream_gate.py):
    the plain call's bits, nothing written late, and the call returned while the gate was shut."""
    case = _gate_case(torch, pair)
    st, res, host = sg.plain(torch, case)
    assert st == 0, lib().sts_last_error()
    case.check([r.cpu().numpy() for r in res], host)
    t = sg.enqueue(torch, case, torch.cuda.Stream(), delay)
    pending = t.pending_at_return
    late = sg.finish(torch, t)
    assert t.status == 0
    for i, (s, r) in enumerate(zip(t.snaps, res)):
        assert sg.same_bits(s, r), "output %d of the gated call differs from the plain call" % i
    assert not late, late
    assert pending, "the call is expected to return before its work ran"
