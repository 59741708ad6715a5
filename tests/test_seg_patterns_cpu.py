"""tests/seg_patterns.py without a GPU: every pattern holds what its name says (NaN counts, the
words hit, the first valid step of the look-ahead tile, the split of the straddling runs), and
the two conditions that keep the GPU tests from hiding a failure: the oracle reports an error on
exactly the declared rows, and every row declared interior has an all-finite ACF at K = 60 under
all four fills (so the ACF comparison is never vacuous)."""
import numpy as np
import pytest

import seg_patterns as sp
from seg_patterns import LONG, T_A, T_B, W, WORD, WORDS

ODD0 = sp.ODD_HOME * W      # first step of the interior odd home


def tile(name, row=1, T=T_A, k=sp.ODD_HOME, n=1):
    """NaN flags of tiles k .. k + n - 1 of one row."""
    return np.isnan(sp.panel(name, T).x[row, k * W:(k + n) * W])


def runs_of(row):
    """(start, length) of every NaN run of a row (or of its NaN flags)."""
    nan = np.concatenate(([False], row if row.dtype == bool else np.isnan(row), [False]))
    d = np.diff(nan.astype(np.int8))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return [(int(a), int(b - a)) for a, b in zip(starts, ends)]


def words_hit(flags):
    return {w for w in range(flags.size // WORD) if flags[w * WORD:(w + 1) * WORD].any()}


def test_geometry():
    assert W == 512 and WORD == 64 and LONG == 32 and WORDS == 8
    for T, ntiles, last, slot in ((T_A, 6, 200, 1), (T_B, 7, 200, 0)):
        assert (T + W - 1) // W == ntiles and T - (ntiles - 1) * W == last and (ntiles - 1) & 1 == slot
        assert T > 2560 and T % 2 == 0 and last >= 64      # seg_kernel<2> at K = 20, fused finalize
        assert sp.home_tiles(T) == [[0], [3], [2], [ntiles - 1], list(range(1, ntiles, 2))]
    assert sp.T_BIG == 32 * W


def test_base_rows():
    for T in (T_A, T_B, sp.T_BIG):
        x = sp.base_rows(3, T, 4)
        assert np.isfinite(x).all()
        assert (np.diff(x, axis=1) == 0.0).sum() >= 3 * 100            # the plateau
    x = sp.panel("none", T_A).x
    assert not np.isnan(x).any() and sp.interior(sp.panel("none", T_A)).all()


@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129])
def test_list_lengths(n):
    for row, k in ((0, 0), (1, sp.ODD_HOME), (2, sp.EVEN_HOME)):
        x = sp.panel("n%d" % n, T_A).x[row]
        assert int(np.isnan(x).sum()) == n == int(np.isnan(x[k * W:(k + 1) * W]).sum())
        assert all(length == 1 for _, length in runs_of(x))            # isolated
    assert sp.PATTERNS["n%d" % n].claim["count"] == n


def test_nearly_and_wholly_nan_tiles():
    for v in (0, 255, 511):
        f = tile("n511_valid%d" % v)
        assert int(f.sum()) == W - 1 and not f[v]
    assert tile("nan_tile").all()
    x = sp.panel("nan_tile", T_A).x[1]
    assert int(np.isnan(x).sum()) == W


def test_word_placement():
    for name in ("word0", "word7", "full_word3", "full_words_0_7", "bit0_each_word", "bit63_each_word"):
        f = tile(name)
        claim = sp.PATTERNS[name].claim
        assert words_hit(f) == claim["words"], name
        for w in claim.get("full_words", ()):
            assert f[w * WORD:(w + 1) * WORD].all(), name
        if "bits" in claim:
            assert {int(t) % WORD for t in np.flatnonzero(f)} == claim["bits"] and int(f.sum()) == WORDS
    f = tile("full_word3")
    assert int(f[:3 * WORD].sum()) == 0 and int(f[4 * WORD:].sum()) == 7    # the prefix counts jump by 64
    for w in (0, 3, 7):
        f = tile("pair_w%d" % w, n=2)
        assert list(np.flatnonzero(f)) == [WORD * w + 63, WORD * w + 64]
    assert WORD * 7 + 64 == W                                            # pair_w7 straddles the tile edge


@pytest.mark.parametrize("f", sp.LOOKAHEAD_F)
def test_lookahead_first_valid(f):
    for T, row, k in ((T_A, 1, sp.ODD_HOME), (T_A, 2, sp.EVEN_HOME), (T_A, 0, 0), (T_B, 1, sp.ODD_HOME)):
        x = sp.panel("ahead_f%d" % f, T).x[row]
        assert np.isnan(x[(k + 1) * W - 40:(k + 1) * W + f]).all() and not np.isnan(x[(k + 1) * W - 41])
        nxt = x[(k + 1) * W:(k + 2) * W]
        assert int(np.flatnonzero(~np.isnan(nxt))[0]) == f               # first valid step of tile k + 1
        t = (k + 1) * W + f
        assert abs(x[t] - x[t + 1]) > 0.2                                # distinct from its neighbour
        assert runs_of(x) == [((k + 1) * W - 40, 40 + f)]
    # every register (p >> 7), lane parity ((p & 127) >> 1) & 1 and half (p & 1) of pick_reg
    assert {p >> 7 for p in sp.LOOKAHEAD_F} == {0, 1, 2, 3}
    assert {(p & 1, ((p & 127) >> 1) & 1) for p in sp.LOOKAHEAD_F} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_lookahead_beyond_one_tile():
    for n in (2, 3):
        x = sp.panel("ahead_none%d" % n, T_A).x[2]                       # even home: tile 2
        assert runs_of(x) == [(3 * W - 40, 40 + (n - 1) * W + 100)]
        assert np.isnan(x[3 * W:(2 + n) * W]).all()                      # tiles k + 1 .. all NaN
        assert not np.isnan(x[(2 + n) * W + 100]) and sp.interior(sp.panel("ahead_none%d" % n, T_A))[2]
    p = sp.panel("to_end", T_A)
    assert runs_of(p.x[1]) == [(ODD0 + W // 2, T_A - ODD0 - W // 2)] and not p.leading.any()
    assert list(p.trailing) == [True, True, True, False, True]     # the last tile holds 200 steps: no stamp


def test_lookback():
    for n in (1, 2, 3):
        p = sp.panel("back%d" % n, T_A)
        x = p.x[1]                                                       # odd home: tile 3
        assert runs_of(x) == [(ODD0 - n * W + 300, n * W - 300 + 10)]
        last_valid = ODD0 - n * W + 299
        assert last_valid // W == sp.ODD_HOME - n and sp.interior(p)[1]
        for k in range(sp.ODD_HOME - n + 1, sp.ODD_HOME):
            assert np.isnan(x[k * W:(k + 1) * W]).all()                  # whole-NaN tiles between
    for name, n in (("lead_half", W // 2), ("lead_1", W), ("lead_2half", 5 * W // 2)):
        p = sp.panel(name, T_A)
        assert runs_of(p.x[0]) == [(0, n)] and p.leading[0] and not p.leading[1:].any()
    p = sp.panel("sparse", T_A)
    assert list(np.flatnonzero(~np.isnan(p.x[0]))) == [0, T_A - 1]
    assert list(np.flatnonzero(~np.isnan(p.x[1]))) == [0]
    assert list(p.nearest_err) == [False, True]


def test_long_runs():
    for n in (31, 32, 33, 34, 65):
        assert runs_of(sp.panel("run%d" % n, T_A).x[1]) == [(ODD0 + 100, n)]
    for name in ("run32_16_16", "run33_17_16"):
        f = tile(name)
        claim = sp.PATTERNS[name].claim
        assert {w: int(f[w * WORD:(w + 1) * WORD].sum()) for w in words_hit(f)} == claim["per_word"]
        assert [length for _, length in runs_of(f)] == [claim["run"]]
    assert max(sp.PATTERNS["run32_16_16"].claim["per_word"].values()) <= LONG // 2
    assert max(sp.PATTERNS["run33_17_16"].claim["per_word"].values()) == LONG // 2 + 1
    for a, b in sp.STRADDLES:
        x = sp.panel("straddle_%d_%d" % (a, b), T_A).x[1]
        edge = ODD0 + W
        assert runs_of(x) == [(edge - a, a + b)]                         # a steps before the edge, b after
    # the 33rd step past the last valid index (edge - a - 1) is step q = LONG - a of the next tile
    q33 = {LONG - a for a, b in sp.STRADDLES if a + b > LONG}
    assert q33 >= {-1, 0, 1} and set(sp.STRADDLES) >= {(16, 16), (16, 17), (20, 14), (30, 3), (3, 30), (33, 1)}
    x = sp.panel("chain33_at511", T_A).x[1]
    (start, length), = runs_of(x)
    assert (start - 1) + LONG + 1 == ODD0 + W - 1 and length > LONG + 1   # the 33rd step is offset 511
    assert [length for _, length in runs_of(sp.panel("two_long_runs", T_A).x[1])] == [40, 40]
    assert runs_of(sp.panel("long_to_tile_end", T_A).x[1]) == [(ODD0 + W - 40, 40)]
    assert runs_of(sp.panel("long_from_tile_start", T_A).x[1]) == [(ODD0, 40)]


def test_runs_over_tile_edges_use_both_carry_slots():
    """For n = 2, 3, 4 tile edges an interior row holds one run that starts in an even tile, and one
    that starts in an odd tile."""
    for n in (2, 3, 4):
        seen = set()
        for name in ("edges%d" % n, "edges%d_next" % n):
            for T in (T_A, T_B):
                p = sp.panel(name, T)
                for row in np.flatnonzero(sp.interior(p)[:4]):
                    for start, length in runs_of(p.x[row]):
                        if (start + length - 1) // W - start // W == n:
                            seen.add((start // W) & 1)
        assert seen == {0, 1}, (n, seen)


def test_extreme_panel():
    p = sp.panel("extreme", T_A)
    x = p.x
    v = ~np.isnan(x)
    assert p.degenerate.all() and np.isnan(x).any(axis=1).all()
    assert set(np.abs(x[0][v[0]])) == {1e250} and set(x[2][v[2]]) == {3.0}
    assert 0 < np.abs(x[1][v[1]]).max() < 1e-290 and 0 < np.abs(x[3][v[3]]).max() < 1e-300


def test_series_ends():
    assert sorted(sp.END_T) == sorted([1536 + r for r in (0, 1, 2, 63, 64, 65, 127, 128, 129, 511)] +
                                      [1, 2, 3, 511, 512, 513, 1025])
    for T in sp.END_T + [2600, 100, 120]:
        p, names = sp.ends_panel(T)
        for row, n in enumerate(names):
            nan = np.flatnonzero(np.isnan(p.x[row]))
            want = {"last1": [T - 1], "last2": [T - 2, T - 1], "last70": list(range(T - 70, T)), "first": [0],
                    "none": []}[n]
            assert list(nan) == want, (T, n)
        assert names[-1] == "none" and (T < 72 or names == sp.END_ROWS)
    assert 2600 - 5 * W == 40                                            # the unfused finalize: last tile < 64


def test_big_panel():
    p = sp.big_panel()
    assert p.x.shape == (10, sp.T_BIG) and sp.interior(p).all()
    for i, name in enumerate(sp.BIG_PATTERNS):
        for j, k in enumerate((15, 28)):
            nan = np.flatnonzero(np.isnan(p.x[2 * i + j]))
            assert list(nan - k * W) == sp.PATTERNS[name].offs
    for row, (a, b) in zip(range(6, 10), sp.PARITY_GAPS):
        assert runs_of(p.x[row]) == [(a, b - a)]


# ---- the two conditions ----

EVERY_PANEL = ([(n, T_A) for n in sp.ALL] + [(n, T_B) for n in sp.SUBSET])


@pytest.mark.parametrize("method", sp.METHODS)
def test_oracle_errs_on_exactly_the_declared_rows(method):
    for name, T in EVERY_PANEL:
        p = sp.panel(name, T)
        err = sp.reference(name, T, method, 0)[2]
        want = p.nearest_err if method == "nearest" else np.zeros(len(err), bool)
        assert np.array_equal(err != 0, want), (name, T, method, err)
    for T in sp.END_T + [2600, 100, 120]:
        assert not sp.ends_reference(T, method, 0)[2].any(), (T, method)
    assert not sp.big_reference(method, 0)[2].any()
    for T, K in sp.SHORT_SHAPES:
        assert not sp.short_reference(T, K, method)[2].any(), (T, K, method)
    # the only declared row: "only index 0 valid"
    declared = [(n, T) for n, T in EVERY_PANEL if sp.panel(n, T).nearest_err.any()]
    assert declared == [("sparse", T_A)]


@pytest.mark.parametrize("method", sp.METHODS)
def test_interior_rows_have_a_finite_acf(method):
    for name, T in EVERY_PANEL:
        p = sp.panel(name, T)
        acf = sp.reference(name, T, method, 60)[1]
        inner = sp.interior(p)
        assert np.isfinite(acf[inner]).all(), (name, T, method)
        nan_rows = np.isnan(acf).any(axis=1)
        assert not (nan_rows & inner).any()
    assert np.isfinite(sp.big_reference(method, 60)[1]).all()
    for T, K in sp.SHORT_SHAPES:
        p = sp.short_panel(T, K)
        assert np.isfinite(sp.short_reference(T, K, method)[1][sp.interior(p)]).all(), (T, K, method)
    # every stamped pattern but the run to T - 1 keeps an interior row among its first three homes at T_A or T_B
    for name in sp.PATTERNS:
        if name != "to_end":
            assert any(sp.interior(sp.panel(name, T))[:3].any() for T in (T_A, T_B)), name


def test_short_shapes_select_every_block_size():
    assert {sp.short_block(T, K) for T, K in sp.SHORT_SHAPES} == {8, 16, 24, 32, 40}
    assert [sp.short_block(T, K) for T, K in sp.SHORT_SHAPES[:5]] == [8, 16, 24, 32, 40]
    for T, K in sp.SHORT_SHAPES:
        B = sp.short_block(T, K)
        assert T % 2 == 0 and 128 <= T <= 2560 and 0 < K <= 24 and T > 2 * K and 64 * B >= T
        r = sp.short_runs(T, B)
        x = sp.short_panel(T, K).x
        for row, name in enumerate(sp.SHORT_ROWS):
            a, b = r[name]
            assert runs_of(x[row]) == ([(a, b - a)] if b > a else []), (T, K, name)
            assert 0 <= a and b <= T
        assert r["from_block_last"][0] % B == B - 1 and (r["to_block_first"][1] - 1) % B == 0
        for name, n in (("one_block", 1), ("two_blocks", 2), ("five_blocks", 5)):
            a, b = r[name]
            assert a % B == 0 and b - a == n * B
        a, b = r["into_last_block"]
        assert b == T and a // B == (T - 1) // B - 1
        assert r["lane0_but_index0"] == (1, B)
        a, b = r["long_three_blocks"]
        assert b - a > LONG and (b - 1) // B - a // B >= 2
    # lane 63's block inside the series
    assert any((T - 1) // sp.short_block(T, K) == 63 for T, K in sp.SHORT_SHAPES)
    assert len(sp.SHORT_ROWS) % 2 == 1                                    # an odd S: the last pair has an empty wave
