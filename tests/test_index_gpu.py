"""The five device entry points of include/sts_index.h against tests/index_ref.py, on bits.  Needs
an MI355X.

Shapes S in {1, 2, 65, 257} x T_in, T_out in {0, 1, 2, 63, 64, 65, 127, 129, 1000}: empty rows, rows
shorter than a wave and around one, odd and even row pitches (dense, so ld = T) with odd and even
shifts, more than one workgroup.  The gather has two kernels, split at 1024 columns: the threshold and the longer
rows' tile (256 columns x 64 series) have a test of their own.  The payloads of index_ref.hard_panel (a NaN with a payload, a signalling NaN,
-0.0, +-inf, a subnormal) must arrive unchanged, and the defaults NaN, 47.0 and -0.0 with their bits.
"""
import ctypes

import numpy as np
import pytest

import index_ref as ir

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 127, 129, 1000)
SERIES = (1, 2, 65, 257)
DEFAULTS = (float("nan"), 47.0, -0.0)
OUT_FILL = -3.0e55
D, H = ir.D, ir.H


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
    return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())


def dev(torch, a, dtype=np.float64):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda:0")


PANEL = ir.hard_panel(max(SERIES), max(SIZES), 20150410)


def shifts(T_in, T_out):
    return sorted({-T_out - 1, -T_out, -3, -1, 0, 1, 2, T_in - 1, T_in, T_in + 2})


@pytest.mark.parametrize("S", SERIES)
def test_rebase_shift(torch, S):
    lib, calls = L(), 0
    for T_in in SIZES:
        host = np.ascontiguousarray(PANEL[:S, :T_in])
        x = dev(torch, host)
        for T_out in SIZES:
            out = torch.empty((S, T_out), dtype=torch.float64, device="cuda:0")
            for start in shifts(T_in, T_out):
                default = DEFAULTS[calls % 3]
                calls += 1
                out.fill_(OUT_FILL)
                st = lib.sts_rebase_shift(vp(x), vp(out), S, T_in, T_out, T_in, T_out, start, default, None)
                assert st == 0, lib.sts_last_error()
                want = ir.gather_panel(host, ir.shift_map(T_in, T_out, start), default)
                ir.assert_bits(out.cpu().numpy(), want, "shift S=%d T_in=%d T_out=%d start=%d" % (S, T_in, T_out, start))
    assert calls >= 81 * 8


def maps(T_in, T_out, rng):
    j = np.arange(T_out, dtype=np.int64)
    holes = np.where(rng.random(T_out) < 0.3, -1 - j, np.sort(rng.integers(0, max(T_in, 1), size=T_out)) if T_in else -1 - j)
    if T_in and T_out:
        inc = np.unique(rng.integers(0, T_in, size=T_out))            # strictly increasing, then holes between
        strict = np.full(T_out, -1, dtype=np.int64)
        strict[np.sort(rng.choice(T_out, size=inc.size, replace=False))] = inc
    else:
        strict = np.full(T_out, -1, dtype=np.int64)
    repeated = (j // 3) * 2 if T_in else -j - 1                        # a target with duplicate instants
    past = np.where(j % 2 == 0, T_in, T_in + 5)                        # must give default
    past[::5] = np.minimum(j[::5], max(T_in - 1, 0)) if T_in else T_in
    return {"absent": np.full(T_out, -1, dtype=np.int64), "identity": j, "holes": strict, "mixed": holes,
            "repeated": repeated, "past_the_end": past, "extremes": np.where(j % 2 == 0, -2 ** 63, 2 ** 63 - 1)}


@pytest.mark.parametrize("S", SERIES)
def test_rebase_map(torch, S):
    lib, calls = L(), 0
    rng = np.random.default_rng(S)
    for T_in in SIZES:
        host = np.ascontiguousarray(PANEL[:S, :T_in])
        x = dev(torch, host)
        for T_out in SIZES:
            out = torch.empty((S, T_out), dtype=torch.float64, device="cuda:0")
            for name, m in maps(T_in, T_out, rng).items():
                m = np.ascontiguousarray(m, dtype=np.int64)
                default = DEFAULTS[calls % 3]
                calls += 1
                out.fill_(OUT_FILL)
                md = dev(torch, m, np.int64)
                st = lib.sts_rebase_map(vp(x), vp(out), S, T_in, T_out, T_in, T_out,
                                        ctypes.c_void_p(md.data_ptr()), default, None)
                assert st == 0, lib.sts_last_error()
                want = ir.gather_panel(host, m, default)
                ir.assert_bits(out.cpu().numpy(), want, "map %s S=%d T_in=%d T_out=%d" % (name, S, T_in, T_out))
                assert np.array_equal(md.cpu().numpy(), m)


@pytest.mark.parametrize("T_out", [1023, 1024, 1025, 1279, 1280, 1281])
def test_rebase_map_at_the_kernel_threshold_and_tile(torch, T_out):
    """rows of up to 1024 columns keep the whole map in LDS, longer ones take the tile kernel (256
    columns x 64 series per workgroup): both sides of the threshold, one column fewer and one more
    than a whole number of tiles, one series fewer and one more than a tile's 64"""
    lib = L()
    rng = np.random.default_rng(T_out)
    for S in (63, 64, 65, 129):
        host = ir.hard_panel(S, 300, T_out + S)
        x = dev(torch, host)
        for name, m in maps(300, T_out, rng).items():
            m = np.ascontiguousarray(m, dtype=np.int64)
            md = dev(torch, m, np.int64)
            out = torch.full((S, T_out), OUT_FILL, dtype=torch.float64, device="cuda:0")
            assert lib.sts_rebase_map(vp(x), vp(out), S, 300, T_out, 300, T_out, vp(md), -0.0, None) == 0, lib.sts_last_error()
            ir.assert_bits(out.cpu().numpy(), ir.gather_panel(host, m, -0.0), "map %s S=%d T_out=%d" % (name, S, T_out))


@pytest.mark.parametrize("T_out", SIZES)
def test_align_uniform(torch, T_out):
    lib = L()
    rng = np.random.default_rng(T_out)
    # a leading and a trailing empty series; every length mixed; start_loc negative, positive, past the end
    lengths = [0, 1000, 1, 7, 0, 64, 1000, 7, 64, 1, 1000, 64, 7, 0]
    starts = [0, 0, -3, 2, 5, -1, 990, 7, -T_out - 1, 1, -500, 64, -6, 3]
    starts += [int(v) for v in rng.integers(-70, 70, size=len(lengths))]
    lengths = lengths[:-1] + lengths + [0]
    starts = starts[:len(lengths)]
    S = len(lengths)
    offsets = np.zeros(S + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    flat = ir.hard_panel(1, int(offsets[-1]), 77)[0]
    vals, off, sl = dev(torch, flat), dev(torch, offsets, np.int64), dev(torch, starts, np.int64)
    for default in DEFAULTS:
        out = torch.full((S, T_out), OUT_FILL, dtype=torch.float64, device="cuda:0")
        st = lib.sts_align_uniform(vp(vals), vp(off), vp(sl), S, T_out, vp(out), T_out, default, None)
        assert st == 0, lib.sts_last_error()
        got = out.cpu().numpy()
        for s in range(S):
            row = flat[offsets[s]:offsets[s + 1]]
            ir.assert_bits(got[s], ir.gather(row, ir.shift_map(len(row), T_out, starts[s]), default),
                           "align T_out=%d series %d (len %d, start %d)" % (T_out, s, len(row), starts[s]))
    assert np.array_equal(vals.cpu().numpy().view(np.uint64), flat.view(np.uint64))


# ---------------- i1 / i2 ----------------

COUNTS = (0, 1, 63, 64, 65, 10007)


def timestamps(rng, index, n):
    """drawn from the index, from 1 ms beside its instants, before first, after last, and from every
    day of the week around it (weekends earlier than first included)"""
    inst = ir.instants_of(index)
    base = inst if inst else [index[0] if ir.is_uniform(index) else 0]
    pool = list(inst) + [t + 1 for t in base] + [t - 1 for t in base]
    pool += [base[0] - k * D for k in range(1, 15)] + [base[-1] + k * D for k in range(1, 15)]
    pool += [t + k * H for t in base[:50] for k in (-24, -1, 1, 24, 48, 72)]
    pool += [-2 ** 63, 2 ** 63 - 1, 0, -1]
    return np.array([pool[i] for i in rng.integers(0, len(pool), size=n)], dtype=np.int64)


def index_args(index, inst_d):
    if ir.is_uniform(index):
        return (ir.KIND_CODE[index[2][0]], index[0], index[1], index[2][1], None, 0)
    return (3, 0, 0, 1, vp(inst_d), len(index))


def check_index(torch, rng, index, counts=COUNTS):
    lib = L()
    inst = ir.instants_of(index)
    inst_d = None if ir.is_uniform(index) else dev(torch, inst, np.int64)
    out = torch.full((len(inst) + 3,), -7, dtype=torch.int64, device="cuda:0")
    assert lib.sts_index_instants(*index_args(index, inst_d), ctypes.c_void_p(out.data_ptr()), None) == 0, lib.sts_last_error()
    assert out.cpu().numpy().tolist() == inst + [-7] * 3, "instants of %s" % (ir.to_string(index)[:80],)
    for n in counts:
        q = timestamps(rng, index, n)
        qd = dev(torch, q, np.int64)
        loc = torch.full((n + 3,), -7, dtype=torch.int64, device="cuda:0")
        st = lib.sts_index_locs(vp(qd), n, *index_args(index, inst_d), ctypes.c_void_p(loc.data_ptr()), None)
        assert st == 0, lib.sts_last_error()
        want = [ir.loc_of(index, int(t)) for t in q]
        got = loc.cpu().numpy().tolist()
        assert got[n:] == [-7] * 3
        bad = [i for i in range(n) if got[i] != want[i]]
        assert not bad, "locs of %s: t=%d gives %d, want %d" % (ir.to_string(index)[:80], q[bad[0]], got[bad[0]], want[bad[0]])
        assert np.array_equal(qd.cpu().numpy(), q)


@pytest.mark.parametrize("kind", ir.KINDS)
def test_uniform_instants_and_locs(torch, kind):
    rng = np.random.default_rng(len(kind))
    for step in (1, 2, 5, 7):
        for start in (ir.millis("2015-04-10") + 9 * H + 30 * 60000, ir.millis("1969-12-29"), ir.millis("1931-03-02") + 1):
            if kind == "businessDays":
                start = ir.next_business_day(start)
            check_index(torch, rng, (start, 257, (kind, step)))
        check_index(torch, rng, (ir.millis("1969-12-31"), 1, (kind, step)), counts=(65,))
        check_index(torch, rng, (ir.millis("1969-12-31"), 0, (kind, step)), counts=(65,))


@pytest.mark.parametrize("dups", [False, True], ids=["distinct", "duplicates"])
def test_irregular_instants_and_locs(torch, dups):
    rng = np.random.default_rng(11 + dups)
    for size in (0, 1, 2, 1000):
        t = np.sort(rng.integers(-30 * 365 * D, 30 * 365 * D, size=size) // 1000 * 1000)
        if dups and size >= 2:
            t[1::3] = t[0::3][:len(t[1::3])]
            t.sort()
        check_index(torch, rng, [int(v) for v in t], counts=COUNTS if size == 1000 else (0, 1, 65))
