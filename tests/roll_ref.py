"""The definition of include/sts_roll.h restated in numpy, and evaluated exactly.

moments() walks the steps of all windows at once: step k of every window is one column slice of the
NaN-padded panel, and the updates of one step are whole-array operations in the header's order, so
every output goes through the scalar loop's operations one by one -- numpy does not contract a
multiply and an add -- and the result is bit-identical to that loop (scalar() is the loop itself, for
one window; tests/test_roll_cpu.py holds the two together).  stat() / pair() derive the ten ops.

exact() evaluates one window in fractions.Fraction: the mean, M2 = sum (x - mean)^2 and
Cxy = sum (x - mean_x)(y - mean_y) of the valid steps, without any rounding.

A helper, not a test.
"""
from fractions import Fraction

import numpy as np

OPS = ("sum", "mean", "var", "std", "min", "max", "zscore")
PAIR_OPS = ("cov", "corr", "beta")
MAX_WINDOW = 1024
BAR = 1e-10


def _as_panel(x):
    x = np.asarray(x, dtype=np.float64)
    return (x.reshape(1, -1), True) if x.ndim == 1 else (x, False)


def _padded(x, w):
    S, T = x.shape
    xp = np.full((S, T + w - 1), np.nan)
    xp[:, w - 1:] = x
    return xp


def moments(x, window, y=None):
    """every quantity of the definition for every window of the (S, T) panel x (against y: (S, T) or
    a shared (T,) factor): a dict of (S, T) arrays n, sum, mean, min, max, M2 and, with y, the y side
    and Cxy.  Nothing of min_periods here."""
    x, _ = _as_panel(x)
    S, T = x.shape
    w = int(window)
    assert 1 <= w <= MAX_WINDOW
    xp = _padded(x, w)
    yp = None
    if y is not None:
        y = np.asarray(y, dtype=np.float64)
        y = np.broadcast_to(y, x.shape) if y.ndim == 1 else y
        assert y.shape == x.shape
        yp = _padded(y, w)
        bad = np.isnan(xp) | np.isnan(yp)
        xp = np.where(bad, np.nan, xp)
        yp = np.where(bad, np.nan, yp)
    with np.errstate(all="ignore"):
        def first_pass(p):
            s = np.zeros((S, T))
            n = np.zeros((S, T), dtype=np.int64)
            lo, hi = np.zeros((S, T)), np.zeros((S, T))
            for k in range(w):
                v = p[:, k:k + T]
                ok = ~np.isnan(v)
                started = n > 0
                s = np.where(ok, np.where(started, s + v, v), s)
                take_lo = ok & (~started | (v < lo) | ((v == lo) & np.signbit(v)))
                take_hi = ok & (~started | (v > hi) | ((v == hi) & ~np.signbit(v)))
                lo = np.where(take_lo, v, lo)
                hi = np.where(take_hi, v, hi)
                n = n + ok
            none = n == 0
            return np.where(none, np.nan, s), n, np.where(none, np.nan, lo), np.where(none, np.nan, hi)

        sx, n, lox, hix = first_pass(xp)
        dn = n.astype(np.float64)
        px = sx / dn
        m = {"n": n, "sum": sx, "mean": px, "min": lox, "max": hix}
        if yp is not None:
            sy, _, loy, hiy = first_pass(yp)
            py = sy / dn
        rx, qx = np.zeros((S, T)), np.zeros((S, T))
        ry, qy, c = np.zeros((S, T)), np.zeros((S, T)), np.zeros((S, T))
        for k in range(w):
            v = xp[:, k:k + T]
            ok = ~np.isnan(v)
            d = v - px
            rx = np.where(ok, rx + d, rx)
            qx = np.where(ok, qx + d * d, qx)
            if yp is not None:
                e = yp[:, k:k + T] - py
                ry = np.where(ok, ry + e, ry)
                qy = np.where(ok, qy + e * e, qy)
                c = np.where(ok, c + d * e, c)

        def m2(q, r, lo, hi):
            const = (lo == hi) & np.isfinite(lo)
            v = q - (r * r) / dn
            v = np.where(const, 0.0, v)
            return np.where(v < 0.0, 0.0, v), const

        m["M2"], cx = m2(qx, rx, lox, hix)
        if yp is not None:
            m["M2y"], cy = m2(qy, ry, loy, hiy)
            m["mean_y"] = py
            fx = np.isfinite(lox) & np.isfinite(hix)
            fy = np.isfinite(loy) & np.isfinite(hiy)
            cxy = c - (rx * ry) / dn
            m["Cxy"] = np.where((cx & fy) | (cy & fx), 0.0, cxy)
    return m


def _gate(v, n, need):
    return np.where(n < need, np.nan, v)


def stat(x, op, window, min_periods=None, m=None):
    """the (S, T) result of a single-panel op (a 1-D x gives a 1-D result)"""
    xx, squeeze = _as_panel(x)
    mp = int(window) if min_periods is None else int(min_periods)
    assert 1 <= mp <= window
    m = moments(xx, window) if m is None else m
    n = m["n"]
    with np.errstate(all="ignore"):
        if op in ("sum", "mean", "min", "max"):
            out = _gate(m[op], n, mp)
        else:
            var = _gate(m["M2"] / (n.astype(np.float64) - 1.0), n, max(mp, 2))
            if op == "var":
                out = var
            else:
                sd = np.sqrt(var)
                out = sd if op == "std" else np.where(sd == 0.0, np.nan, (xx - m["mean"]) / sd)
    return out[0] if squeeze else out


def pair(x, y, op, window, min_periods=None, m=None):
    xx, squeeze = _as_panel(x)
    mp = int(window) if min_periods is None else int(min_periods)
    assert 1 <= mp <= window
    m = moments(xx, window, y) if m is None else m
    n = m["n"]
    with np.errstate(all="ignore"):
        if op == "cov":
            v = m["Cxy"] / (n.astype(np.float64) - 1.0)
        elif op == "corr":
            v = m["Cxy"] / (np.sqrt(m["M2"]) * np.sqrt(m["M2y"]))
            v = np.where(v > 1.0, 1.0, np.where(v < -1.0, -1.0, v))
        else:
            v = m["Cxy"] / m["M2y"]
        out = _gate(v, n, max(mp, 2))
    return out[0] if squeeze else out


def scalar(xs, ys=None):
    """the definition as the scalar loop, for ONE window given as its steps in ascending order (NaN
    for a step before the series start): a dict of Python floats like moments()'s entries"""
    xs = [float(v) for v in xs]
    ys = None if ys is None else [float(v) for v in ys]
    idx = [i for i, v in enumerate(xs) if v == v and (ys is None or ys[i] == ys[i])]
    n = len(idx)
    nan = float("nan")
    if n == 0:
        return {"n": 0, "sum": nan, "mean": nan, "min": nan, "max": nan, "M2": nan, "M2y": nan, "Cxy": nan}
    f = np.float64

    def side(vals):
        s = lo = hi = f(vals[idx[0]])
        for i in idx[1:]:
            v = f(vals[i])
            s = s + v
            if v < lo or (v == lo and np.signbit(v)):
                lo = v
            if v > hi or (v == hi and not np.signbit(v)):
                hi = v
        return s, lo, hi

    with np.errstate(all="ignore"):
        sx, lox, hix = side(xs)
        dn = f(n)
        px = sx / dn
        out = {"n": n, "sum": float(sx), "mean": float(px), "min": float(lox), "max": float(hix)}
        if ys is not None:
            sy, loy, hiy = side(ys)
            py = sy / dn
        rx = qx = ry = qy = c = f(0.0)
        for i in idx:
            d = f(xs[i]) - px
            rx = rx + d
            qx = qx + d * d
            if ys is not None:
                e = f(ys[i]) - py
                ry = ry + e
                qy = qy + e * e
                c = c + d * e

        def m2(q, r, lo, hi):
            const = lo == hi and np.isfinite(lo)
            v = f(0.0) if const else q - (r * r) / dn
            return (f(0.0) if v < 0.0 else v), const

        M2, cx = m2(qx, rx, lox, hix)
        out["M2"] = float(M2)
        if ys is not None:
            M2y, cy = m2(qy, ry, loy, hiy)
            out["M2y"] = float(M2y)
            fx, fy = np.isfinite(lox) and np.isfinite(hix), np.isfinite(loy) and np.isfinite(hiy)
            out["Cxy"] = 0.0 if (cx and fy) or (cy and fx) else float(c - (rx * ry) / dn)
    return out


def exact(xs, ys=None):
    """one window in exact rational arithmetic (finite values): Fractions n, mean, M2, maxabs and,
    with ys, M2y and Cxy"""
    idx = [i for i, v in enumerate(xs) if v == v and (ys is None or ys[i] == ys[i])]
    X = [Fraction(float(xs[i])) for i in idx]
    n = len(X)
    out = {"n": n}
    if n == 0:
        return out
    mx = sum(X) / n
    out["mean"] = mx
    out["maxabs"] = max(abs(v) for v in X)
    out["M2"] = sum((v - mx) * (v - mx) for v in X)
    if ys is not None:
        Y = [Fraction(float(ys[i])) for i in idx]
        my = sum(Y) / n
        out["M2y"] = sum((v - my) * (v - my) for v in Y)
        out["Cxy"] = sum((a - mx) * (b - my) for a, b in zip(X, Y))
    return out


def window_of(row, t, window):
    """the steps of W(t) in ascending order, NaN before the series start"""
    row = np.asarray(row, dtype=np.float64)
    lo = t - window + 1
    return [float("nan")] * max(0, -lo) + [float(v) for v in row[max(lo, 0):t + 1]]


# ---------------- the hard families ----------------

FAMILIES = ("walk_1e9", "walk_1e9_fine", "returns", "scaled_up", "scaled_down", "ulps_1e9", "flat_jumps")


def family(name, T, S=2, seed=0):
    """(S, T) rows of a hard family, from a seed"""
    rng = np.random.default_rng([1009, FAMILIES.index(name), seed, T])
    z = rng.standard_normal((S, T))
    if name == "walk_1e9":
        return 1e9 + np.cumsum(z, axis=1)
    if name == "walk_1e9_fine":
        return 1e9 + np.cumsum(1e-3 * z, axis=1)
    if name == "returns":
        return 0.01 * z
    if name == "scaled_up":
        return np.ldexp(100.0 + np.cumsum(z, axis=1), 400)
    if name == "scaled_down":
        return np.ldexp(100.0 + np.cumsum(z, axis=1), -400)
    if name == "ulps_1e9":
        return 1e9 + np.spacing(1e9) * rng.integers(-3, 4, size=(S, T))
    if name == "flat_jumps":
        lvl = np.cumsum(rng.standard_normal((S, T)) * (rng.random((S, T)) < 0.02), axis=1)
        return 1e9 + 0.1 * np.round(lvl * 10)
    raise KeyError(name)


def cumsum_var(x, window):
    """what the library refuses: the variance from differences of two cumulative sums (full windows;
    NaN elsewhere)"""
    x, squeeze = _as_panel(x)
    w = int(window)
    c1 = np.concatenate([np.zeros((x.shape[0], 1)), np.cumsum(x, axis=1)], axis=1)
    c2 = np.concatenate([np.zeros((x.shape[0], 1)), np.cumsum(x * x, axis=1)], axis=1)
    out = np.full(x.shape, np.nan)
    s1 = c1[:, w:] - c1[:, :-w]
    s2 = c2[:, w:] - c2[:, :-w]
    with np.errstate(all="ignore"):
        out[:, w - 1:] = (s2 - s1 * s1 / w) / (w - 1)
    return out[0] if squeeze else out


def same_bits(a, b):
    """bit-identical where neither is NaN, NaN in the same places (the payload and sign of a NaN that
    arithmetic made differ between processors)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    ua = np.ascontiguousarray(a).view(np.uint64)
    ub = np.ascontiguousarray(b).view(np.uint64)
    return bool(np.array_equal(ua[~na], ub[~na]))


def ulp_diff(a, b):
    """the largest distance in units of the last place where neither is NaN; inf when the NaN
    positions differ"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    if a.shape != b.shape or not np.array_equal(na, nb):
        return float("inf")
    a, b = a[~na], b[~na]
    if a.size == 0:
        return 0.0
    inf = np.isinf(a) | np.isinf(b)
    if not np.array_equal(a[inf], b[inf]):
        return float("inf")
    a, b = a[~inf], b[~inf]
    if a.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))))
