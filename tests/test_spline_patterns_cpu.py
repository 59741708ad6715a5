"""tests/spline_patterns.py without a GPU: every pattern holds what its name says (gap lengths, the
knot's offset in its chunk, the first and last knot), the storage classes it declares are the ones
the model derives from its NaNs, and the conditions that keep the GPU tests from hiding a failure:
the oracle refuses exactly the declared rows, fills every step of [first knot, last knot) of the
others with a finite value (unless the row is declared non-finite) and leaves every other step's
raw bits alone."""
import numpy as np
import pytest

import oracle
import spline_patterns as sp
from spline_patterns import CHUNK, DIRECT, RC, RR

PANELS = sp.all_panels()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_store_class_is_the_kernels_branch():
    """p < t0 + 8 -> Rc, p < t0 + 16 -> Rr, else direct, with t0 the first step of the knot's chunk."""
    for t in range(0, 40):
        t0 = t // CHUNK * CHUNK
        for p in range(t + 1, t + 60):
            want = RC if p < t0 + CHUNK else RR if p < t0 + 2 * CHUNK else DIRECT
            assert sp.store_class(t, p) == want == min(2, p // 8 - t // 8)
    assert sp.store_class(15, 16, chunk=16) == RR and sp.store_class(0, 15, chunk=16) == RC


def test_walk_is_exact():
    x = sp.walk(3, 400, 9)
    assert np.isfinite(x).all() and np.array_equal(x * 8.0, np.round(x * 8.0))
    assert np.array_equal(x, sp.walk(3, 400, 9)) and not np.array_equal(x, sp.walk(3, 400, 10))


@pytest.mark.parametrize("name,p", PANELS, ids=[n for n, _ in PANELS])
def test_oracle_accepts_and_fills_what_the_panel_declares(name, p):
    S, T = p.x.shape
    assert p.reject.shape == p.nonfinite.shape == (S,) and len(p.classes) == len(p.meta) == S
    out, err = oracle.panel_fill(p.x, "spline")
    assert np.array_equal(err != 0, p.reject), (name, np.flatnonzero((err != 0) != p.reject))
    assert set(err[p.reject]) <= {oracle.ERR_TOO_FEW_POINTS}
    for r in range(S):
        k = sp.knots_of(p.x[r])
        assert p.reject[r] == (k.size < 3)
        assert p.classes[r] == sp.classes_of(p.x[r]), (name, r)
        if p.reject[r]:
            assert not p.classes[r]
            continue
        lo, hi = int(k[0]), int(k[-1])
        assert np.array_equal(bits(out[r, :lo]), bits(p.x[r, :lo])), (name, r, "before the first knot")
        assert np.array_equal(bits(out[r, hi:]), bits(p.x[r, hi:])), (name, r, "from the last knot on")
        if not p.nonfinite[r]:
            assert np.isfinite(out[r, lo:hi]).all(), (name, r)


@pytest.mark.parametrize("knot0", [32, 40])
def test_gap_by_offset(knot0):
    p = sp.gap_by_offset(knot0)
    assert (knot0 // CHUNK) % 2 == (knot0 == 40)                        # the knot's chunk in LDS tile 0, tile 1
    assert p.x.shape == (112, 96) == (CHUNK * len(sp.GAP_LENGTHS), sp.GAP_T)
    assert p.x.shape[0] > sp.WAVE and p.x.shape[0] % sp.WAVE != 0       # a partial second workgroup
    assert not p.reject.any() and not p.nonfinite.any()
    assert sorted(set(p.meta)) == [(k, n) for k in range(8) for n in sp.GAP_LENGTHS]
    reached = set()
    for r, (k, n) in enumerate(p.meta):
        assert sp.runs_of(p.x[r]) == [(knot0 + 1 + k, n)]               # one gap, right after the knot at knot0 + k
        assert sp.interior_gaps(p.x[r]) == [(knot0 + k, n)] and (knot0 + k) % CHUNK == k
        reached |= {(k, c) for c in p.classes[r]}
    want = {(k, c) for k in range(8) for c in (RC, RR, DIRECT)} - {(7, RC)}
    assert reached == want and len(want) == 23
    # every offset has a gap that stops inside the right chunk and one that crosses both boundaries
    for k in range(8):
        cls = [sp.gap_classes(knot0 + k, n) for kk, n in p.meta if kk == k]
        assert any(RR in c and DIRECT not in c for c in cls) and any({RR, DIRECT} <= c for c in cls)


def test_long_gaps_beside_dense():
    p = sp.long_gaps_beside_dense()
    assert p.x.shape == (64, 400) and not p.reject.any()
    long_rows = [r for r in range(64) if DIRECT in p.classes[r]]
    assert tuple(long_rows) == sp.LONG_ROWS == (0, 1, 31, 62, 63)
    starts, ends = set(), set()
    for r in range(64):
        g = sp.interior_gaps(p.x[r])
        assert g == p.meta[r]
        if r not in sp.LONG_ROWS:
            assert not np.isnan(p.x[r]).any() and not p.classes[r]      # fully dense
            continue
        assert p.classes[r] == {RC, RR, DIRECT} or (g[0][0] % 8 == 7 and p.classes[r] == {RR, DIRECT})
        for t, n in g:
            assert 191 <= n <= 300 and (n - 2 * CHUNK) // CHUNK > 20    # direct stores over > 20 flushed chunks
            starts.add(t % 8); ends.add((t + n + 1) % 8)
    assert len(p.meta[31]) == 2 and sum(200 <= n <= 300 for r in sp.LONG_ROWS for _, n in p.meta[r]) == 5
    assert len(starts) >= 4 and len(ends) >= 4                          # different offsets in their chunks
    q = sp.long_gaps_beside_dense(True)
    assert q.x.shape == (64, 400) and not q.reject.any()
    for r in range(64):
        (t, n), = sp.interior_gaps(q.x[r])
        assert t + n + 1 == 300 + r % 17 and 200 <= n <= 300 and DIRECT in q.classes[r]
    assert len({sp.interior_gaps(q.x[r])[0][0] % 8 for r in range(64)}) == 8


@pytest.mark.parametrize("T", [sp.ENDS_T] + sp.S_SEAMS_T)
def test_ends(T):
    p = sp.ends(T)
    firsts, lasts, threes, kinds = [], [], [], [m[0] for m in p.meta]
    for r, m in enumerate(p.meta):
        k = sp.knots_of(p.x[r])
        if m[0] == "first":
            assert k[0] == m[1] and k[-1] == T - 1 and k.size == T - m[1]; firsts.append(m[1])
        elif m[0] == "last":
            assert k[0] == 0 and k[-1] == m[1] and k.size == m[1] + 1; lasts.append(m[1])
        elif m[0] == "three":
            assert tuple(k) == m[1] and not p.reject[r]; threes.append(m[1])
        elif m[0] == "two":
            assert tuple(k) == m[1] and p.reject[r]
        else:
            assert m == ("none",) and k.size == 0 and p.reject[r]
    assert firsts == list(range(18)) and lasts == [T - 1 - j for j in range(18)]
    assert (0, T // 2, T - 1) in threes
    assert [kn for kn in threes if len({t // 8 for t in kn}) == 1] == [(8, 9, 15), (9, 11, 12)]
    assert sum(1 for kn in threes if [t // 8 for t in kn] == list(range(kn[0] // 8, kn[0] // 8 + 3))) >= 3
    assert "two" in kinds and "none" in kinds
    # the refused rows lie between accepted ones
    for r in np.flatnonzero(p.reject):
        assert 0 < r and not p.reject[r - 1] and (r + 1 == len(kinds) or not p.reject[r + 1])


def test_degenerate_coefficients():
    p = sp.degenerate_coefficients()
    x = dict(zip(p.meta, p.x))
    assert list(p.meta) == sp.DEGENERATE_ROWS and not p.reject.any()
    assert [m for m, nf in zip(p.meta, p.nonfinite) if nf] == ["inf_knot"]
    for r in p.x:
        assert sp.interior_gaps(r) == [(5, 1), (10, 8), (29, 17)]
        assert sp.classes_of(r) == {RC, RR, DIRECT}
    k = sp.knots_of(p.x[0])
    assert (x["constant"][k] == 7.5).all()
    assert (x["constant_neg_zero"][k] == 0.0).all() and np.signbit(x["constant_neg_zero"][k]).all()
    assert np.array_equal(x["ramp"][k], k.astype(float)) and np.array_equal(x["square"][k], (k * k).astype(float))
    assert 20 in k and np.signbit(x["ramp_neg_zero"][20]) and x["ramp_neg_zero"][20] == 0.0
    assert not np.signbit(x["ramp_pos_zero"][20]) and x["ramp_pos_zero"][20] == 0.0
    assert np.signbit(x["ramp_down_neg_zero"][20]) and x["ramp_down_neg_zero"][21] == -1.0
    assert np.isposinf(x["inf_knot"][29]) and np.isnan(x["inf_knot"][30])
    assert np.all(np.abs(x["far_level"][k] - 1e6) < 200) and np.all(x["far_level"][k] % 0.125 == 0)
    assert np.all(x["tiny"][k] * 2.0 ** 1000 == x["huge"][k] * 2.0 ** -900)
    assert np.all(np.abs(x["subnormal"][k]) < np.finfo(float).tiny) and np.all(x["subnormal"][k] != 0)
    # the oracle trims: a constant row returns its knots' own bits, sign of zero included; the lines are exact
    out, _ = oracle.panel_fill(p.x, "spline")
    o = dict(zip(p.meta, out))
    assert (bits(o["constant"][:63]) == bits(7.5)).all()
    assert (bits(o["constant_neg_zero"][:63]) == bits(-0.0)).all()
    assert np.array_equal(o["ramp"][:63], np.arange(63.0))


@pytest.mark.parametrize("T", sp.T_SEAMS)
def test_t_seams(T):
    p = sp.t_seams(T)
    assert p.x.shape == (sp.T_SEAMS_S, T) and sp.T_SEAMS_S > sp.WAVE
    frac = np.isnan(p.x).mean()
    assert 0.2 < frac < 0.4
    assert (~p.reject).sum() >= 10, "too few accepted rows at T = %d" % T
    if T >= 2 * CHUNK:
        assert any(RR in c for c in p.classes)
    if T > 2 * CHUNK + 1:
        assert any(RC in c for c in p.classes) and p.reject.sum() < sp.T_SEAMS_S // 2


def test_t_seams_cover_every_chunk_boundary():
    assert sp.T_SEAMS == [3, 4, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33]
    for c in (CHUNK, sp.CHUNK_FALLBACK):
        for m in (c, 2 * c):
            assert {m - 1, m, m + 1} <= set(sp.T_SEAMS)
    assert any(T % 2 for T in sp.T_SEAMS) and any(T % 2 == 0 for T in sp.T_SEAMS)


@pytest.mark.parametrize("T", sp.S_SEAMS_T)
def test_s_seams(T):
    base = sp.ends(T)
    n = base.x.shape[0]
    assert n < 63                                   # every S but 1 repeats the whole set
    for S in sp.S_SEAMS:
        p = sp.s_seams(S, T)
        assert p.x.shape == (S, T)
        for r in range(S):
            assert np.array_equal(bits(p.x[r]), bits(base.x[r % n])) and p.reject[r] == base.reject[r % n]
    assert sp.S_SEAMS == [1, 63, 64, 65, 128, 129]
