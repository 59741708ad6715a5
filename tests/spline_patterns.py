"""NaN patterns aimed at the structure of fill("spline") (csrc/sts_spline.hip).  No GPU is needed to
build them: tests/test_spline_patterns_cpu.py asserts that every pattern holds what its name says,
and tests/test_spline_seams_gpu.py runs them through both kernels.

spline_lds_kernel gives 64 series to a one-wave workgroup and walks them in chunks of CHUNK = 8
steps.  Its backward sweep reaches a knot at step t, evaluates the knot's polynomial at every gap
step p in (t, next knot) and stores the value in one of three places:

    class 0 (Rc)      p lies in the knot's own chunk: the current LDS tile
    class 1 (Rr)      p lies in the chunk to its right: the other LDS tile, not yet flushed
    class 2 (direct)  p lies further right: a global store over a chunk that was flushed already,
                      behind a wait for those flushes that only the lanes with such a gap ask for

store_class() restates that three-way branch.  The global-memory form (spline_fill_kernel, any odd
leading dimension or misaligned base) walks chunks of 16 steps, 256 series per workgroup.  In both,
steps before the first knot and from the last knot on keep their raw bits, and a row with fewer
than three knots keeps all of them and reports STS_ERR_TOO_FEW_POINTS.

A builder returns a Panel: x (S, T), reject (S,) the rows the oracle must refuse, classes (one set
of storage classes per row, of the LDS form), nonfinite (S,) rows whose filled steps need not be
finite, and meta, one entry per row saying what was stamped into it.
"""
import functools
from collections import namedtuple

import numpy as np

NaN = float("nan")
CHUNK = 8            # spline_lds_kernel's steps per chunk
CHUNK_FALLBACK = 16  # spline_fill_kernel's
WAVE = 64            # series per workgroup of the LDS form
RC, RR, DIRECT = 0, 1, 2

Panel = namedtuple("Panel", "x reject classes nonfinite meta")

GAP_LENGTHS = [1, 2, 6, 7, 8, 9, 14, 15, 16, 17, 23, 24, 25, 40]
GAP_T, GAP_KNOT0 = 96, 32
LONG_T, LONG_ROWS = 400, (0, 1, 31, 62, 63)
ENDS_T, ENDS_J = 64, 18
T_SEAMS = [3, 4, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33]
T_SEAMS_S = 70       # two workgroups of the LDS form, the second with 6 rows
S_SEAMS = [1, 63, 64, 65, 128, 129]
S_SEAMS_T = [40, 41]
DEGENERATE_T = 64
# (left knot, length): offsets 5, 2 and 5 in their chunks; the longest reaches all three classes
DEGENERATE_GAPS = [(5, 1), (10, 8), (29, 17)]


def store_class(t_knot, p, chunk=CHUNK):
    """Where the backward sweep puts gap step p of the knot at t_knot: 0 Rc, 1 Rr, 2 direct."""
    return min(2, p // chunk - t_knot // chunk)


def knots_of(row):
    return np.flatnonzero(~np.isnan(row))


def runs_of(row):
    """(start, length) of every NaN run of a row."""
    nan = np.concatenate(([False], np.isnan(row), [False]))
    d = np.diff(nan.astype(np.int8))
    return [(int(a), int(b - a)) for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1))]


def interior_gaps(row):
    """(left knot, length) of every NaN run between two knots of a row the spline accepts."""
    k = knots_of(row)
    if k.size < 3:
        return []
    return [(int(a), int(b - a - 1)) for a, b in zip(k[:-1], k[1:]) if b - a > 1]


def classes_of(row, chunk=CHUNK):
    """The storage classes the LDS form's backward sweep takes on this row."""
    return frozenset(store_class(t, p, chunk) for t, n in interior_gaps(row) for p in range(t + 1, t + 1 + n))


def gap_classes(t, n, chunk=CHUNK):
    return frozenset(store_class(t, p, chunk) for p in range(t + 1, t + 1 + n))


def walk(S, T, seed, level=100.0):
    """An exact random walk: steps are multiples of 1/8 below 2^7, so every partial sum is exact."""
    rng = np.random.default_rng(seed)
    return level + np.cumsum(rng.integers(-8, 9, size=(S, T)) / 8.0, axis=1)


def gap(row, t, n):
    """A gap of n steps right after the knot at t."""
    row[t + 1:t + 1 + n] = NaN


def _panel(x, classes=None, nonfinite=(), meta=None):
    x = np.ascontiguousarray(x, dtype=np.float64)
    S = x.shape[0]
    reject = np.array([knots_of(r).size < 3 for r in x], dtype=bool)
    if classes is None:
        classes = [classes_of(r) for r in x]
    nf = np.zeros(S, dtype=bool)
    nf[list(nonfinite)] = True
    x.setflags(write=False)
    return Panel(x, reject, list(classes), nf, list(meta) if meta is not None else [None] * S)


# ---- the patterns ----

@functools.lru_cache(maxsize=None)
def gap_by_offset(knot0=GAP_KNOT0):
    """One gap per row right after the knot at step knot0 + k, k = 0..7, of every length in
    GAP_LENGTHS: 112 rows (two workgroups, the second with 48 rows).  knot0 = 32 is the first step
    of chunk 4 (LDS tile 0), 40 of chunk 5 (tile 1).  meta: (k, length)."""
    assert knot0 % CHUNK == 0
    meta = [(k, n) for k in range(CHUNK) for n in GAP_LENGTHS]
    x = walk(len(meta), GAP_T, 101 + knot0)
    classes = []
    for r, (k, n) in enumerate(meta):
        gap(x[r], knot0 + k, n)
        classes.append(gap_classes(knot0 + k, n))
    return _panel(x, classes, meta=meta)


# (left knot, length) per long row; T = 400 cannot hold two gaps of 200 steps next to three knots, so
# row 31's second gap is the longest that fits: 191 steps, direct stores over 22 flushed chunks
LONG_GAPS = {0: [(50, 250)], 1: [(3, 300)], 31: [(1, 191), (193, 203)], 62: [(95, 200)], 63: [(36, 277)]}


@functools.lru_cache(maxsize=None)
def long_gaps_beside_dense(every_row=False):
    """T = 400, 64 rows.  Rows 0, 1, 31, 62 and 63 hold gaps of 191 to 300 steps (row 31 two of
    them) that start and end at different offsets in their chunks; every other row is dense, so the
    wait before the direct stores is divergent and a store over a neighbour's row shows.
    every_row: a gap in all 64 rows instead, row r's ending at the knot 300 + r % 17.
    meta: the row's [(left knot, length)]."""
    x = walk(WAVE, LONG_T, 202)
    if every_row:
        gaps = {r: [(50 + r % 13, 300 + r % 17 - (50 + r % 13) - 1)] for r in range(WAVE)}
    else:
        gaps = LONG_GAPS
    meta, classes = [], []
    for r in range(WAVE):
        g = gaps.get(r, [])
        for t, n in g:
            gap(x[r], t, n)
        meta.append(list(g))
        classes.append(frozenset().union(*[gap_classes(t, n) for t, n in g]) if g else frozenset())
    return _panel(x, classes, meta=meta)


def _three(T, knots, base):
    row = np.full(T, NaN)
    row[list(knots)] = base[list(knots)]
    return row


THREE_IN_ONE_CHUNK = [(8, 9, 15), (9, 11, 12)]
THREE_IN_THREE_CHUNKS = [(7, 8, 16), (5, 12, 20), (0, 15, 23), (16, 31, 32)]


def ends_rows(T):
    """-> (rows, meta).  meta: ("first", j), ("last", T - 1 - j), ("three", knots), ("two", knots)
    or ("none",).  A rejected row follows every fifth accepted one."""
    base = walk(1, T, 300 + T)[0]
    good = []
    for j in range(ENDS_J):
        a = base.copy(); a[:j] = NaN; good.append((a, ("first", j)))
    for j in range(ENDS_J):
        a = base.copy(); a[T - j:] = NaN; good.append((a, ("last", T - 1 - j)))
    for kn in [(0, T // 2, T - 1)] + THREE_IN_ONE_CHUNK + THREE_IN_THREE_CHUNKS:
        good.append((_three(T, kn, base), ("three", kn)))
    two = [(0, T - 1), (7, 8), (8, 15), (T - 2, T - 1), (3, 20)]
    rows, meta, bad = [], [], 0
    for i, (a, m) in enumerate(good):
        rows.append(a); meta.append(m)
        if i % 5 == 4:
            if bad % 2 == 0:
                kn = two[(bad // 2) % len(two)]
                b = np.full(T, NaN); b[list(kn)] = base[list(kn)]
                rows.append(b); meta.append(("two", kn))
            else:
                rows.append(np.full(T, NaN)); meta.append(("none",))
            bad += 1
    return np.array(rows), meta


@functools.lru_cache(maxsize=None)
def ends(T=ENDS_T):
    x, meta = ends_rows(T)
    return _panel(x, meta=meta)


DEGENERATE_ROWS = ["constant", "constant_neg_zero", "ramp", "square", "ramp_neg_zero", "ramp_pos_zero",
                   "ramp_down_neg_zero", "inf_knot", "far_level", "tiny", "subnormal", "huge"]


@functools.lru_cache(maxsize=None)
def degenerate_coefficients():
    """Rows whose polynomials lose coefficients (b = c = d = 0: the trailing-zero trim returns the
    knot itself, with its sign of zero; c = d = 0: the line), signed zeros on knots, a non-finite
    knot, and levels where the products round far from 1.  Every row holds gaps of 1, 8 and 17
    steps.  meta: the row's name."""
    T = DEGENERATE_T
    i = np.arange(T, dtype=np.float64)
    w = walk(1, T, 404)[0]
    rows = {
        "constant": np.full(T, 7.5),
        "constant_neg_zero": np.full(T, -0.0),
        "ramp": i.copy(),
        "square": i * i,
        "ramp_neg_zero": i - 20.0,
        "ramp_pos_zero": i - 20.0,
        "ramp_down_neg_zero": 20.0 - i,
        "inf_knot": w.copy(),
        "far_level": w - 100.0 + (1e6 + 0.25),
        "tiny": w * 2.0 ** -1000,
        "subnormal": w * 2.0 ** -1060,
        "huge": w * 2.0 ** 900,
    }
    rows["ramp_neg_zero"][20] = -0.0
    rows["ramp_down_neg_zero"][20] = -0.0
    rows["inf_knot"][DEGENERATE_GAPS[2][0]] = np.inf
    x = np.array([rows[n] for n in DEGENERATE_ROWS])
    for r in x:
        for t, n in DEGENERATE_GAPS:
            gap(r, t, n)
    return _panel(x, nonfinite=[DEGENERATE_ROWS.index("inf_knot")], meta=DEGENERATE_ROWS)


@functools.lru_cache(maxsize=None)
def t_seams(T):
    """70 rows of T steps with 30 % NaN: the LDS chunk of 8, the fallback's of 16 and the
    single-element tail of an odd T.  Short rows are often refused; reject says which."""
    x = walk(T_SEAMS_S, T, 500 + T).copy()
    x[np.random.default_rng(600 + T).random(x.shape) < 0.3] = NaN
    return _panel(x)


@functools.lru_cache(maxsize=None)
def s_seams(S, T):
    """The rows of ends(T), repeated to S rows: one row, a workgroup less one, exactly one, one
    more, two, two and one."""
    p = ends(T)
    idx = np.arange(S) % p.x.shape[0]
    return _panel(p.x[idx], meta=[p.meta[i] for i in idx])


def all_panels():
    """(name, Panel) of every panel the GPU tests run."""
    out = [("gap_by_offset", gap_by_offset()),
           ("gap_by_offset_odd_chunk", gap_by_offset(GAP_KNOT0 + CHUNK)),
           ("long_gaps_beside_dense", long_gaps_beside_dense()),
           ("long_gaps_every_row", long_gaps_beside_dense(True)),
           ("ends", ends()),
           ("degenerate_coefficients", degenerate_coefficients())]
    out += [("t_seams_%d" % T, t_seams(T)) for T in T_SEAMS]
    out += [("s_seams_%dx%d" % (S, T), s_seams(S, T)) for T in S_SEAMS_T for S in S_SEAMS]
    return out
