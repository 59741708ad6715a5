"""numpy restatement of the panel transforms of include/sts_transforms.h, written from the
loops of S/UnivariateTimeSeries.scala (S/ = src/main/scala/com/cloudera/sparkts/ in the reference).

Every function takes a panel (S, T) and treats its rows independently: the element-wise IEEE
operations (one correctly rounded binary64 / + - per element, as the JVM's) are vectorised across
series, and every loop over time that carries a dependence stays a sequential Python loop in the
reference's order.  No oracle, no device, nothing read from outside this file.
"""
import numpy as np


def _panel(x):
    a = np.array(x, dtype=np.float64)
    return a.reshape(1, -1) if a.ndim == 1 else a


def quotients(x, lag, minus_one=False):
    """:45-63  ret(i) = ts(i + lag) / ts(i) [- 1.0], i < T - lag"""
    x = _panel(x)
    T = x.shape[1]
    assert 0 <= lag <= T
    with np.errstate(all="ignore"):
        q = x[:, lag:] / x[:, :T - lag]
        return q - 1.0 if minus_one else q


def fill_previous(x):
    """:194-204"""
    r = _panel(x).copy()
    filler = np.full(r.shape[0], np.nan)
    for i in range(r.shape[1]):
        filler = np.where(np.isnan(r[:, i]), filler, r[:, i])
        r[:, i] = filler
    return r


def fill_with_default(x, filler):
    """:233-241"""
    r = _panel(x).copy()
    r[np.isnan(r)] = filler
    return r


def downsample(x, n, phase=0):
    """:308-321"""
    x = _panel(x)
    T = x.shape[1]
    new_len = max(int(np.ceil((T - phase) / float(n))), 0)
    out = np.zeros((x.shape[0], new_len))
    i = phase
    for j in range(new_len):
        out[:, j] = x[:, i]
        i += n
    return out


def upsample(x, n, phase=0, use_zero=False):
    """:331-345"""
    x = _panel(x)
    T = x.shape[1]
    out = np.full((x.shape[0], T * n), 0.0 if use_zero else np.nan)
    i = phase
    for j in range(T):
        out[:, i] = x[:, j]          # IndexError where the reference runs off its array
        i += n
    return out


def first_not_nan(x):
    """:119-128"""
    x = _panel(x)
    out = np.empty(x.shape[0], dtype=np.int64)
    for s, row in enumerate(x):
        i = 0
        while i < row.size and np.isnan(row[i]):
            i += 1
        out[s] = i
    return out


def last_not_nan(x):
    """:130-139"""
    x = _panel(x)
    out = np.empty(x.shape[0], dtype=np.int64)
    for s, row in enumerate(x):
        i = row.size - 1
        while i >= 0 and np.isnan(row[i]):
            i -= 1
        out[s] = i
    return out


def trim_leading(row):
    """:98-105"""
    row = np.asarray(row, dtype=np.float64)
    start = int(first_not_nan(row)[0])
    return row[start:] if start < row.size else np.zeros(0)


def trim_trailing(row):
    """:110-117 (the reference's own bounds: 0 until lastNotNaN)"""
    row = np.asarray(row, dtype=np.float64)
    end = int(last_not_nan(row)[0])
    return row[:end] if end > 0 else np.zeros(0)


def differences_at_lag(x, lag, start=None, dest=None):
    """:356-376; dest may be x itself (in place)"""
    x = _panel(x) if dest is None or dest is not x else x
    start = lag if start is None else start
    assert start >= lag
    d = x.copy() if dest is None else dest
    if lag == 0:
        return d
    with np.errstate(all="ignore"):
        for i in range(x.shape[1]):
            d[:, i] = x[:, i] if i < start else x[:, i] - x[:, i - lag]
    return d


def inverse_differences_at_lag(x, lag, start=None, dest=None):
    """:397-417; dest may be x itself (in place)"""
    x = _panel(x) if dest is None or dest is not x else x
    start = lag if start is None else start
    assert start >= lag
    a = x.copy() if dest is None else dest
    if lag == 0:
        return a
    with np.errstate(all="ignore"):
        for i in range(x.shape[1]):
            a[:, i] = x[:, i] if i < start else x[:, i] + a[:, i - lag]
    return a


def differences_of_order_d(x, d):
    """:438-450, ping-pong buffers included"""
    x = _panel(x)
    diffed, orig = x.copy(), x.copy()
    for i in range(1, d + 1):
        orig, diffed = diffed, orig
        differences_at_lag(orig, 1, i, dest=diffed)
    return diffed


def inverse_differences_of_order_d(x, d):
    """:459-465"""
    a = _panel(x).copy()
    for i in range(d, 0, -1):
        inverse_differences_at_lag(a, 1, i, dest=a)
    return a


def breeze_diff(x, n):
    """breeze.linalg.diff(v, n): n times v(i + 1) - v(i) (TimeSeriesRDD.differences)"""
    v = _panel(x)
    with np.errstate(all="ignore"):
        for _ in range(n):
            v = v[:, 1:] - v[:, :-1]
    return v


def hard_panel(S, T, seed):
    """The test panel: Gaussian prices around 100 with, cycling over the series, NaN runs at the
    head, the tail and inside, an all-NaN series, a single-valid series, +-0.0, +-inf, subnormals,
    values at 2^+-400 and zeros where a quotient divides by them."""
    rng = np.random.default_rng(seed)
    x = 100.0 + rng.standard_normal((S, T))
    for s in range(S):
        k = s % 12
        r = x[s]
        if k == 1:
            r[:max(1, T // 3)] = np.nan
        elif k == 2:
            r[T - max(1, T // 4):] = np.nan
        elif k == 3:
            r[T // 3: T // 3 + max(1, T // 5)] = np.nan
            r[rng.random(T) < 0.3] = np.nan
        elif k == 4:
            r[:] = np.nan
        elif k == 5:
            r[:] = np.nan
            r[T // 2] = 3.5
        elif k == 6:
            r[::3] = 0.0
            r[1::7] = -0.0
        elif k == 7:
            r[::5] = np.inf
            r[2::11] = -np.inf
        elif k == 8:
            r[:] = rng.standard_normal(T) * 5e-324 * 1000
            r[::4] = 5e-324
        elif k == 9:
            r[:] = rng.standard_normal(T) * 2.0 ** 400
        elif k == 10:
            r[:] = rng.standard_normal(T) * 2.0 ** -400
            r[rng.random(T) < 0.1] = np.nan
        elif k == 11:
            r[rng.random(T) < 0.5] = np.nan
    return x


def assert_bits(got, ref, what=""):
    """the bar of sts_transforms.h: every non-NaN element has the reference's bits (signed zeros and
    infinities included) and NaN sits exactly where the reference has NaN"""
    got = np.ascontiguousarray(got, dtype=np.float64)
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    same = (got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))
    if not same.all():
        idx = np.argwhere(~same)[:5]
        raise AssertionError("%s: %d mismatches, first %s got %s ref %s" % (
            what, (~same).sum(), idx.tolist(), [got[tuple(i)] for i in idx], [ref[tuple(i)] for i in idx]))
