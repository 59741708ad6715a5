"""Plain-Python restatement of the date-time index semantics of include/sts_index.h: scalar code
with loops over Python ints, independent of sparkts/datetimeindex.py and of csrc/sts_index.hpp.

Everything is UTC, int milliseconds since the epoch, with Java's truncating division (tdiv / tmod).
A frequency is a pair (kind, n), kind one of "days", "hours", "businessDays"; a uniform index is a
tuple (start, periods, (kind, n)); an irregular index is a list of instants, non-decreasing.
"""
import datetime

import numpy as np

D = 86400000
H = 3600000
KINDS = ("days", "hours", "businessDays")
KIND_CODE = {"days": 0, "hours": 1, "businessDays": 2, "irregular": 3}


class IllegalArgument(ValueError):
    """where the reference throws IllegalArgumentException"""


def tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def tmod(a, b):
    return a - tdiv(a, b) * b


def day_of_week(t):
    """Monday = 1 .. Sunday = 7"""
    return ((t // D + 3) % 7) + 1


def advance(freq, t, k):
    kind, n = freq
    if kind == "days":
        return t + k * n * D
    if kind == "hours":
        return t + k * n * H
    dow = day_of_week(t)
    if dow > 5:
        raise IllegalArgument("%d is not a business day" % t)
    total = k * n
    standard = tdiv(total, 5) * 2
    remaining = tmod(total, 5)
    extra = 2 if dow + remaining > 5 else 0
    return t + (total + standard + extra) * D


def difference(freq, a, b):
    kind, n = freq
    if kind == "days":
        return tdiv(tdiv(b - a, D), n)
    if kind == "hours":
        return tdiv(tdiv(b - a, H), n)
    if b < a:
        return -difference(freq, b, a)
    between = tdiv(b - a, D)
    dow = day_of_week(a)
    if dow > 5:
        raise IllegalArgument("%d is not a business day" % a)
    standard = tdiv(between, 7) * 2
    remaining = tmod(between, 7)
    extra = 2 if dow + remaining > 5 else 0
    return tdiv(between - standard - extra, n)


def next_business_day(t):
    dow = day_of_week(t)
    return t + 2 * D if dow == 6 else (t + D if dow == 7 else t)


# ---- uniform ----

def u_at(u, loc):
    start, periods, freq = u
    return advance(freq, start, loc)


def u_last(u):
    return u_at(u, u[1] - 1)


def u_loc(u, t):
    """locAtDateTime; -1 where the reference's scalar code throws (include/sts_index.h)"""
    start, periods, freq = u
    try:
        loc = difference(freq, start, t)
    except IllegalArgument:
        return -1
    if 0 <= loc < periods and u_at(u, loc) == t:
        return loc
    return -1


def u_instants(u):
    return [u_at(u, i) for i in range(u[1])]


def u_islice(u, lo, hi):
    return (advance(u[2], u[0], lo), hi - lo, u[2])


def u_slice(u, start, end):
    return (start, difference(u[2], start, end) + 1, u[2])


def uniform_to(start, end, freq):
    return (start, difference(freq, start, end) + 1, freq)


# ---- irregular ----

def i_loc(instants, t):
    """the first location holding t, else -(insertion point) - 1"""
    for i, v in enumerate(instants):
        if v == t:
            return i
        if v > t:
            return -i - 1
    return -len(instants) - 1


def i_slice(instants, start, end):
    """the instants in [start, end]"""
    return [v for v in instants if start <= v <= end]


# ---- either kind ----

def is_uniform(index):
    return isinstance(index, tuple)


def instants_of(index):
    return u_instants(index) if is_uniform(index) else list(index)


def loc_of(index, t):
    return u_loc(index, t) if is_uniform(index) else i_loc(index, t)


def start_loc(src, tgt):
    """uniform -> uniform: the location of tgt's first in src (negative: before it)"""
    if src[2] != tgt[2]:
        raise IllegalArgument("frequencies differ")
    freq = src[2]
    if tgt[0] >= src[0]:
        loc = difference(freq, src[0], tgt[0])
        if advance(freq, src[0], loc) != tgt[0]:
            raise IllegalArgument("firsts not on a common grid")
        return loc
    loc = difference(freq, tgt[0], src[0])
    if advance(freq, tgt[0], loc) != src[0]:
        raise IllegalArgument("firsts not on a common grid")
    return -loc


def rebase_map(src, tgt):
    """m[j]: the first location of target instant j in the source, negative where absent"""
    if is_uniform(src) and is_uniform(tgt):
        sl = start_loc(src, tgt)
        return [j + sl if 0 <= j + sl < src[1] else -1 for j in range(tgt[1])]
    return [loc_of(src, t) for t in instants_of(tgt)]


def gather(row, m, default):
    """out[j] = row[m[j]] where 0 <= m[j] < len(row), else default -- on bits"""
    bits = np.asarray(row, dtype=np.float64).view(np.uint64)
    d = np.array([default], dtype=np.float64).view(np.uint64)[0]
    out = np.empty(len(m), dtype=np.uint64)
    for j, k in enumerate(m):
        out[j] = bits[k] if 0 <= k < len(bits) else d
    return out.view(np.float64)


def gather_panel(x, m, default):
    """gather() for every row of a panel at once: the map is the restatement's, the copy is numpy's
    column selection on bits"""
    bits = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    S, T = bits.shape
    m = np.asarray(m, dtype=np.int64).reshape(-1)
    d = np.array([default], dtype=np.float64).view(np.uint64)[0]
    out = np.full((S, m.size), d, dtype=np.uint64)
    hit = (m >= 0) & (m < T)
    out[:, hit] = bits[:, m[hit]]
    return out.view(np.float64)


def shift_map(T_in, T_out, start):
    return [j + start if 0 <= j + start < T_in else -1 for j in range(T_out)]


def rebase(src, tgt, row, default):
    return gather(row, rebase_map(src, tgt), default)


def assert_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    assert not bad.any(), "%s: %d elements differ, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[0].tolist())


# ---- strings ----

def iso(t):
    """Joda's DateTime.toString in UTC for years 1..9999"""
    days, ms = divmod(t, D)
    d = datetime.date.fromordinal(days + 719163)
    return "%04d-%02d-%02dT%02d:%02d:%02d.%03dZ" % (d.year, d.month, d.day, ms // H, ms // 60000 % 60, ms // 1000 % 60,
                                                    ms % 1000)


def millis(text):
    """a date 'y-m-d' (unpadded allowed), optionally 'Thh:mm:ss.mmmZ', in UTC"""
    date, _, clock = text.rstrip("Z").partition("T")
    y, m, d = (int(p) for p in date.split("-"))
    t = (datetime.date(y, m, d).toordinal() - 719163) * D
    if clock:
        hms, _, frac = clock.partition(".")
        parts = [int(p) for p in hms.split(":")] + [0, 0]
        t += parts[0] * H + parts[1] * 60000 + parts[2] * 1000 + (int((frac + "000")[:3]) if frac else 0)
    return t


def to_string(index):
    if is_uniform(index):
        return "uniform,%s,%d,%s %d" % (iso(index[0]), index[1], index[2][0], index[2][1])
    return ",".join(["irregular"] + [iso(t) for t in index])


def from_string(text):
    tok = text.split(",")
    if tok[0] == "uniform":
        kind, n = tok[3].split(" ")
        if kind not in KINDS:
            raise IllegalArgument("Frequency %s not recognized" % kind)
        return (millis(tok[1]), int(tok[2]), (kind, int(n)))
    if tok[0] == "irregular":
        return [millis(t) for t in tok[1:]]
    raise IllegalArgument("DateTimeIndex type %s not recognized" % tok[0])


# ---- payloads every copy must keep ----

def hard_panel(S, T, seed):
    """finite values with NaN of a non-default payload, -0.0, +-inf and a subnormal sprinkled in"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((S, T))
    special = np.array([0x7FF8DEADBEEF0001, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                        0x0000000000000123, 0xFFF4000000000002], dtype=np.uint64).view(np.float64)
    if x.size:
        flat = x.reshape(-1)
        pos = rng.choice(flat.size, size=min(flat.size, max(1, flat.size // 7)), replace=False)
        flat[pos] = special[np.arange(pos.size) % special.size]
    return x
