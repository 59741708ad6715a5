"""NaN patterns aimed at the geometry of the wave-private segment kernel (csrc/sts_seg.hip) and
of the one-wave short kernel (csrc/sts_short.hip).  No GPU is needed to build them:
tests/test_seg_patterns_cpu.py asserts that every pattern holds what its name says, and
tests/test_seg_seams_gpu.py / tests/test_short_seams_gpu.py run them on the device.

The segment kernel walks a series in tiles of W = 512 steps, each of eight 64-bit validity
words; the NaN list of a tile is imputed 64 entries at a time; the look-ahead reaches one tile
(in registers), then a global scan with a one-entry cache; linear runs longer than LONG = 32
steps past their last valid index take a chain path that is carried over tile edges by tile
parity.  A pattern is a list of step offsets relative to the first step of a tile ("home"); a
panel stamps it into one row per home:

    row 0  tile 0            row 3  the last (partial) tile, clipped at T
    row 1  the interior odd tile (tile 3)       row 4  every second tile at once (1, 3, 5, ...)
    row 2  the interior even tile (tile 2)

Offsets below 0 or from W up reach into the neighbouring tiles.  T_A = 2760 is six tiles (the
last holds 200 steps and ends in ring slot 1), T_B = 3272 seven (the last in slot 0: the fused
finalize's copy-up).  A row whose stamp hits index 0 is "leading", one whose stamp hits T - 1 is
"trailing" (fill('linear') leaves such a run NaN, so its ACF may be NaN); every other row is
"interior" and must have an all-finite ACF under all four fills.
"""
import functools
from collections import namedtuple

import numpy as np

import oracle

NaN = float("nan")
W, WORD, LONG = 512, 64, 32
WORDS = W // WORD
T_A, T_B = 2760, 3272
T_BIG = 16384
METHODS = ["linear", "previous", "next", "nearest"]
RTOL = 1e-10
HOMES = ["tile0", "odd", "even", "last", "alternate"]
ODD_HOME, EVEN_HOME = 3, 2


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


# ---- the patterns ----

# offs: NaN offsets from the home tile's first step; bump: offsets whose (valid) value is moved
# away from its neighbours; claim: what tests/test_seg_patterns_cpu.py asserts about the pattern
Pat = namedtuple("Pat", "offs bump claim")


def _pat(offs, bump=(), **claim):
    return Pat(sorted(set(int(o) for o in offs)), tuple(bump), claim)


def spaced(n):
    """n isolated NaNs inside the tile (every third step from offset 8)."""
    return [8 + 3 * i for i in range(n)]


def _all_but(v):
    return [o for o in range(W) if o != v]


LOOKAHEAD_F = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 383, 384, 510, 511]
# (a, b): a steps before the tile edge, b after it; a run longer than LONG has its 33rd step at
# q = LONG - a of the next tile ((32, 2): q = 0, (31, 3): q = 1; (33, 1): the previous tile's last step)
STRADDLES = [(16, 16), (16, 17), (20, 14), (30, 3), (3, 30), (33, 1), (32, 2), (31, 3)]

PATTERNS = {}
# list length against the 64-lane stride of the imputation loop
for _n in (63, 64, 65, 127, 128, 129):
    PATTERNS["n%d" % _n] = _pat(spaced(_n), count=_n)
# 511 NaNs and one valid step; a whole-NaN tile
for _v in (0, 255, 511):
    PATTERNS["n511_valid%d" % _v] = _pat(_all_but(_v), count=W - 1, valid=_v)
PATTERNS["nan_tile"] = _pat(range(W), count=W)
# word placement
PATTERNS["word0"] = _pat([0, 1, 2, 3, 10] + list(range(20, 30)) + [63], words={0})
PATTERNS["word7"] = _pat([7 * WORD + o for o in [0, 5, 6, 7] + list(range(40, 51)) + [62, 63]], words={7})
PATTERNS["full_word3"] = _pat(list(range(3 * WORD, 4 * WORD)) + [264, 266, 300, 319, 320, 400, 500],
                              words={3, 4, 5, 6, 7}, full_words={3})
PATTERNS["full_words_0_7"] = _pat(list(range(WORD)) + list(range(7 * WORD, W)), words={0, 7}, full_words={0, 7})
PATTERNS["bit0_each_word"] = _pat([WORD * w for w in range(WORDS)], words=set(range(WORDS)), bits={0})
PATTERNS["bit63_each_word"] = _pat([WORD * w + 63 for w in range(WORDS)], words=set(range(WORDS)), bits={63})
for _w in (0, 3, 7):     # bit 63 of word w and bit 0 of word w + 1 (w = 7: across the tile edge)
    PATTERNS["pair_w%d" % _w] = _pat([WORD * _w + 63, WORD * _w + 64], count=2, pair=_w)
# look-ahead: a run over the last 40 steps of tile k whose first valid successor is offset f of
# tile k + 1 (every register, half and lane parity of pick_reg), or lies in tile k + 2 / k + 3
# (the global scan, then its cache), or does not exist
for _f in LOOKAHEAD_F:
    PATTERNS["ahead_f%d" % _f] = _pat(range(W - 40, W + _f), bump=[W + _f], ahead=_f)
PATTERNS["ahead_none2"] = _pat(range(W - 40, 2 * W + 100), bump=[2 * W + 100], ahead_tiles=2)
PATTERNS["ahead_none3"] = _pat(range(W - 40, 3 * W + 100), bump=[3 * W + 100], ahead_tiles=3)
PATTERNS["to_end"] = _pat(range(W // 2, 64 * W), to_end=True)
# look-back: the last valid step 1, 2, 3 tiles back (whole-NaN tiles between); leading runs
for _n in (1, 2, 3):
    PATTERNS["back%d" % _n] = _pat(range(-_n * W + 300, 10), bump=[-_n * W + 299], back=_n)
PATTERNS["lead_half"] = _pat(range(0, W // 2), lead=W // 2)
PATTERNS["lead_1"] = _pat(range(0, W), lead=W)
PATTERNS["lead_2half"] = _pat(range(0, 5 * W // 2), lead=5 * W // 2)
# the long-run chain of fill('linear'): more than LONG steps past the last valid index
for _n in (31, 32, 33, 34, 65):
    PATTERNS["run%d" % _n] = _pat(range(100, 100 + _n), run=_n)
PATTERNS["run32_16_16"] = _pat(range(48, 80), run=32, per_word={0: 16, 1: 16})      # never flagged
PATTERNS["run33_17_16"] = _pat(range(47, 80), run=33, per_word={0: 17, 1: 16})      # flagged by word 0
for _a, _b in STRADDLES:                                  # a steps before the tile edge, b after it
    PATTERNS["straddle_%d_%d" % (_a, _b)] = _pat(range(W - _a, W + _b), split=(_a, _b))
PATTERNS["chain33_at511"] = _pat(range(W - 1 - LONG, W + 8), step33=W - 1)
for _n in (2, 3, 4):     # over n tile edges, from the home tile and from the tile after it
    PATTERNS["edges%d" % _n] = _pat(range(400, _n * W + 50), edges=_n)
    PATTERNS["edges%d_next" % _n] = _pat(range(W + 400, (_n + 1) * W + 50), edges=_n)
PATTERNS["two_long_runs"] = _pat(list(range(50, 90)) + list(range(300, 340)), runs=[40, 40])
PATTERNS["long_to_tile_end"] = _pat(range(W - 40, W), run=40)
PATTERNS["long_from_tile_start"] = _pat(range(0, 40), run=40)

# panels that are not stamped: see panel()
SPECIAL = ["none", "sparse", "extreme"]
ALL = SPECIAL + list(PATTERNS)
# the subset run at T_B and through the A/B decompositions
SUBSET = (["n63", "n64", "n65", "n127", "n128", "n129", "full_word3"] + ["ahead_f%d" % f for f in LOOKAHEAD_F] +
          ["ahead_none2", "ahead_none3", "edges2", "edges3", "edges4", "edges2_next", "edges3_next", "edges4_next"])
# the gaps of test_parity_gpu.py's segment-kernel tail (T = 16 000), kept in the big panel
PARITY_GAPS = [(40, 15950), (100, 133), (511, 545), (1000, 9000)]
BIG_PATTERNS = ["n129", "ahead_f255", "edges3"]


def base_rows(S, T, seed):
    """100 + a random walk; index 0 and T - 1 valid; one plateau (linear increments of exactly 0)."""
    rng = np.random.default_rng(seed)
    x = 100.0 + np.cumsum(0.01 * rng.standard_normal((S, T)), axis=1)
    a = min(900, T // 3)
    b = min(a + 500, T // 3 + T // 4)
    if b > a:
        x[:, a:b] = x[:, a:a + 1]
    return x


def home_tiles(T):
    ntiles = (T + W - 1) // W
    return [[0], [min(ODD_HOME, ntiles - 1)], [min(EVEN_HOME, ntiles - 1)], [ntiles - 1], list(range(1, ntiles, 2))]


Panel = namedtuple("Panel", "x leading trailing degenerate nearest_err")


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100003


@functools.lru_cache(maxsize=None)
def panel(name, T):
    """The panel of one pattern: x (S, T) and, per row, whether a stamped NaN sits on index 0
    (leading) or T - 1 (trailing), whether the row is numerically degenerate (its ACF is not
    required to be finite), and whether fill('nearest') must report "all NaNs" for it."""
    if name == "none":
        x = base_rows(3, T, 1)
        return _declare(x)
    if name == "sparse":
        x = base_rows(2, T, 2)
        x[0, 1:T - 1] = NaN              # only indices 0 and T - 1 valid
        x[1, 1:] = NaN                   # only index 0 valid: fillNearest's "all NaNs" error
        return _declare(x, nearest_err=[1])
    if name == "extreme":                # increments outside [2^-900, 2^700], zero and tiny ones
        x = oracle.gen_panel(9, 4, T, 0.05)
        x[0] = np.where(np.arange(T) % 2 == 0, 1e250, -1e250) * np.where(np.isnan(x[0]), NaN, 1.0)
        x[1] = x[1] * 1e-300
        x[2] = np.where(np.isnan(x[2]), NaN, 3.0)
        x[3] = x[3] * 4e-320
        return _declare(x, degenerate=range(4))
    p = PATTERNS[name]
    homes = home_tiles(T)
    x = base_rows(len(homes), T, _seed(name))
    for row, tiles in enumerate(homes):
        for k in tiles:
            for o in p.bump:
                if 0 <= k * W + o < T:
                    x[row, k * W + o] += 0.37
        for k in tiles:
            t = k * W + np.array(p.offs)
            t = t[(t >= 0) & (t < T)]
            x[row, t] = NaN
    return _declare(x)


def _declare(x, degenerate=(), nearest_err=()):
    x.setflags(write=False)
    S = x.shape[0]
    deg = np.zeros(S, bool)
    deg[list(degenerate)] = True
    nerr = np.zeros(S, bool)
    nerr[list(nearest_err)] = True
    return Panel(x, np.isnan(x[:, 0]), np.isnan(x[:, -1]), deg, nerr)


def interior(p):
    """Rows whose ACF must be finite under every fill."""
    return ~(p.leading | p.trailing | p.degenerate | p.nearest_err)


# ---- series ends ----

END_R = [0, 1, 2, 63, 64, 65, 127, 128, 129, 511]
END_T = [3 * W + r for r in END_R] + [1, 2, 3, 511, 512, 513, 1025]
END_ROWS = ["last1", "last2", "last70", "first", "none"]


@functools.lru_cache(maxsize=None)
def ends_panel(T):
    """Rows "the last 1 / 2 / 70 steps NaN", "the first step NaN", "no NaN".  A row that would
    leave fill('nearest') without a valid step after index 0 is left out (short T)."""
    names = [n for n, need in zip(END_ROWS, (3, 4, 72, 2, 1)) if T >= need]
    x = base_rows(len(names), T, 5 + T)
    for row, n in enumerate(names):
        if n.startswith("last"):
            x[row, T - int(n[4:]):] = NaN
        elif n == "first":
            x[row, 0] = NaN
    return _declare(x), names


@functools.lru_cache(maxsize=None)
def big_panel():
    """T = 16 384 (32 tiles, the segment kernel's largest series): the interior odd (tile 15) and even
    (tile 28) rows of three patterns, and the four long gaps of test_parity_gpu.py's T = 16 000 check."""
    T = T_BIG
    x = base_rows(2 * len(BIG_PATTERNS) + len(PARITY_GAPS), T, 77)
    row = 0
    for name in BIG_PATTERNS:
        p = PATTERNS[name]
        for k in (15, 28):
            for o in p.bump:
                x[row, k * W + o] += 0.37
            x[row, k * W + np.array(p.offs)] = NaN
            row += 1
    for a, b in PARITY_GAPS:
        x[row, a:b] = NaN
        row += 1
    return _declare(x)


# ---- references (computed once, shared, read-only) ----

def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def reference_of(x, method, K):
    if K > 0:
        rf, racf, rerr = oracle.panel_fill_autocorr(x, method, K, threads=4)
        with np.errstate(all="ignore"):
            floor = np.array([noise_floor(r, K) if e == 0 else np.zeros(K) for r, e in zip(rf, rerr)])
    else:
        rf, rerr = oracle.panel_fill(x, method, threads=4)
        racf = floor = None
    return _freeze(rf, racf, rerr, floor)


@functools.lru_cache(maxsize=None)
def reference(name, T, method, K):
    return reference_of(panel(name, T).x, method, K)


@functools.lru_cache(maxsize=None)
def ends_reference(T, method, K):
    return reference_of(ends_panel(T)[0].x, method, K)


@functools.lru_cache(maxsize=None)
def big_reference(method, K):
    return reference_of(big_panel().x, method, K)


def where(x_row, t):
    """The segment kernel's coordinates of step t of a raw row, for an assertion message."""
    nan = np.isnan(x_row)
    prev = np.flatnonzero(~nan[:t + 1])
    L = int(prev[-1]) if prev.size else -1
    nxt = np.flatnonzero(~nan[t:])
    N = t + int(nxt[0]) if nxt.size else x_row.size
    q = t % W
    return "t=%d (tile %d, word %d, bit %d), L=%d, t-L=%d, N=%d, raw %s" % (
        t, t // W, q // WORD, q % WORD, L, t - L, N, "NaN" if nan[t] else "valid")


# ---- the one-wave short kernel: lane l owns the steps [l B, l B + B) ----

def short_block(T, K):
    """launch_short_m's block size B for a series of T steps and K lags."""
    need = (T + 63) // 64
    km = max(8, (K + 3) // 4 * 4)
    nb = max(need, km)
    for B in (8, 16, 24, 32):
        if nb <= B:
            return B
    return 40


# (T, K): every B (8, 16, 24, 32, 40); 130: B = 8 with most lanes empty; 512 and 2560: lane 63's
# block is inside the series (B = 8 and 40); (500, 20): B = 24 set by the lag window, not by T
SHORT_SHAPES = [(500, 8), (1000, 16), (1500, 20), (2000, 20), (2500, 20), (130, 8), (512, 8), (2560, 20), (500, 20)]
SHORT_ROWS = ["from_block_last", "to_block_first", "one_block", "two_blocks", "five_blocks", "into_last_block",
              "lane0_but_index0", "long_three_blocks", "none"]


def short_runs(T, B):
    """name -> (first NaN, one past the last NaN), placed against the lane blocks of B steps."""
    lb = (T - 1) // B                                     # the last occupied block (lane 63 when T > 63 B)
    n = max(LONG + 1, B + 4)
    return {
        "from_block_last": (3 * B - 1, 3 * B + 3),        # starts at a block's last step
        "to_block_first": (4 * B - 3, 4 * B + 1),         # ends at a block's first step
        "one_block": (5 * B, 6 * B),
        "two_blocks": (5 * B, 7 * B),
        "five_blocks": (5 * B, 10 * B),
        "into_last_block": (lb * B - 3, T),               # enters the last block and reaches T - 1
        "lane0_but_index0": (1, B),
        "long_three_blocks": (11 * B - 2, 11 * B - 2 + n),   # >= 33 steps over >= 3 blocks
        "none": (0, 0),
    }


@functools.lru_cache(maxsize=None)
def short_panel(T, K):
    B = short_block(T, K)
    runs = short_runs(T, B)
    x = base_rows(len(SHORT_ROWS), T, 900 + T + K)
    for row, name in enumerate(SHORT_ROWS):
        a, b = runs[name]
        x[row, a:b] = NaN
    return _declare(x)


@functools.lru_cache(maxsize=None)
def short_reference(T, K, method):
    return reference_of(short_panel(T, K).x, method, K)


# ---- running a panel on the device and comparing it with its reference ----

SENTINEL = -7.25e77


def run_device(torch, x, method, K, pad=0):
    """sts_fill (K = 0) or sts_fill_autocorr through the library the sparkts mirror is bound to.
    The rows are T steps at a pitch of ld = T (+ 1 when T is odd, so the rows stay 16-byte aligned
    and on the segment kernel) + pad; the input's pad holds NaN, the output is pre-filled with a
    sentinel that every pad element must still hold, err with 99."""
    from sparkts import _native
    from sparkts import UnivariateTimeSeries as uts
    lib = _native.lib()
    S, T = x.shape
    ld = T + (T & 1) + pad
    xin = np.full((S, ld), NaN)
    xin[:, :T] = x
    xd = torch.as_tensor(xin, device="cuda:0")
    filled = torch.full((S, ld), SENTINEL, dtype=torch.float64, device="cuda:0")
    err = torch.full((S,), 99, dtype=torch.int32, device="cuda:0")
    code = uts.fill_method_code(method)
    stream = torch.cuda.current_stream().cuda_stream
    if K > 0:
        acf = torch.full((S, K), SENTINEL, dtype=torch.float64, device="cuda:0")
        st = lib.sts_fill_autocorr(xd.data_ptr(), filled.data_ptr(), S, T, ld, ld, code, K, acf.data_ptr(),
                                   err.data_ptr(), stream)
    else:
        acf = None
        st = lib.sts_fill(xd.data_ptr(), filled.data_ptr(), S, T, ld, ld, code, err.data_ptr(), stream)
    assert st == 0, lib.sts_last_error()
    torch.cuda.synchronize()
    out = filled.cpu().numpy()
    assert (out[:, T:] == SENTINEL).all(), "written past T (ld = %d, T = %d)" % (ld, T)
    return out[:, :T], (None if acf is None else acf.cpu().numpy()), err.cpu().numpy()


def compare(x, got, ref, K, what, rows=None):
    """err exact; rows without an error bit for bit; their ACF by the contract.  rows: the rows
    of the reference that x / got hold (default: all)."""
    gf, gacf, gerr = got
    rf, racf, rerr, floor = ref
    if rows is not None:
        rf, rerr = rf[rows], rerr[rows]
        if K > 0:
            racf, floor = racf[rows], floor[rows]
    assert np.array_equal(gerr, rerr), "%s: error codes %s, oracle %s" % (what, gerr, rerr)
    ok = rerr == 0
    bad = (gf.view(np.uint64) != rf.view(np.uint64)) & ok[:, None]
    if bad.any():
        r, t = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d filled values differ, first in row %d at %s: got %r, oracle %r" % (
            what, int(bad.sum()), r, where(x[r], t), float(gf[r, t]), float(rf[r, t])))
    if K > 0 and ok.any():
        with np.errstate(all="ignore"):
            e = within(gacf[ok], racf[ok], floor[ok])
        assert e <= 1.0, "%s: ACF error %.3g x (1e-10 rel + noise floor)" % (what, e)
