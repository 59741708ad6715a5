"""The definition of include/sts_cross.h restated in numpy, its 60-digit twin, the input families the
tests hold the device to, and (under __main__) the writer of tests/golden/cross_exact.json.

Definition (per pair of series x_i of x and y_j of y, T steps):
    mu_i = (sum_t x_i[t]) / T,  z_i = x_i - mu_i,  r_i = sum_t z_i[t]     (w_j, q_j for y_j)
    C_ij = sum_t z_i[t] w_j[t] - r_i q_j / T                              corrected two-pass
    COV  = C_ij / (T - 1),   CORR = clamp(C_ij / (sqrt(C_ii) sqrt(C'_jj)), -1, 1)
Rules: a series with a non-finite value has NaN in its row (symmetric form: and column) and a NaN
mean; a bit-constant series (max == min) has COV +0.0 and CORR NaN, its diagonal included; the
symmetric CORR diagonal is exactly 1.0 otherwise.

moments() is that, in float64, with numpy's own summation order: it says what is computed, not in
which order, so the device is compared to it within the numeric bar, never bit for bit.  exact() is
the same definition in mpmath (the correction term vanishes in exact arithmetic) rounded once.
one_pass() is MLlib's (X'X - n m m') / (n - 1), kept to show what the correction buys.
"""
import json
import os

import numpy as np

BAR = 1e-10                     # the project's bar: relative to sqrt(C_ii C_jj) / (T - 1) for COV, absolute for CORR
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cross_exact.json")
FAMILIES = ("returns", "walks_1e6", "level_1e9", "level_1e12", "near_minus_one", "scaled_down", "scaled_up")
GOLDEN_T = 64
HARD_T = 2520


def family(name, T, seed=0):
    """(S, T) with 4 <= S <= 6; one series is the negative of another (correlation -1), or in
    near_minus_one within 1e-6 of it."""
    rng = np.random.default_rng([FAMILIES.index(name), T, seed])
    n = rng.standard_normal((5, T))
    if name == "returns":
        x = 0.01 * n
    elif name == "walks_1e6":
        x = 1e6 + np.cumsum(n, axis=1)
    elif name == "level_1e9":
        x = 1e9 + 1e-3 * n
    elif name == "level_1e12":
        x = 1e12 + 1e-2 * n
    elif name == "near_minus_one":
        x = 0.01 * n
        x[1] = -x[0] + 1e-3 * 0.01 * n[1]      # 1 + corr about 5e-7
        return np.ascontiguousarray(x[:4])
    elif name == "scaled_down":
        x = 0.01 * n * 2.0 ** -400
    elif name == "scaled_up":
        x = 0.01 * n * 2.0 ** 400
    else:
        raise KeyError(name)
    return np.ascontiguousarray(np.vstack([x, -x[0]]))


def flags(x):
    """per series: 0 ordinary, 1 bit-constant, 2 a non-finite value"""
    x = np.asarray(x, dtype=np.float64)
    bad = ~np.isfinite(x).all(axis=1)
    with np.errstate(invalid="ignore"):
        const = x.max(axis=1) == x.min(axis=1)
    return np.where(bad, 2, np.where(const, 1, 0))


def _rules(out, fx, fy, kind, symmetric):
    out = np.array(out, dtype=np.float64)
    cx, cy = (fx == 1)[:, None], (fy == 1)[None, :]
    out[np.broadcast_to(cx | cy, out.shape)] = np.nan if kind == "corr" else 0.0
    out[fx == 2, :] = np.nan
    out[:, fy == 2] = np.nan
    if symmetric and kind == "corr":
        d = np.arange(out.shape[0])
        ok = fx == 0
        out[d[ok], d[ok]] = 1.0
    return out


def _centre(x):
    T = x.shape[1]
    with np.errstate(all="ignore"):
        mu = x.sum(axis=1) / T
        z = x - mu[:, None]
        return mu, z, z.sum(axis=1)


def moments(x, y=None, kind="cov"):
    """-> (out, mean_x, mean_y or None): the restatement"""
    x = np.asarray(x, dtype=np.float64)
    sym = y is None
    y = x if sym else np.asarray(y, dtype=np.float64)
    T = x.shape[1]
    fx, fy = flags(x), flags(y)
    with np.errstate(all="ignore"):
        mu, z, r = _centre(np.where(np.isfinite(x), x, 0.0))
        nu, w, q = _centre(np.where(np.isfinite(y), y, 0.0))
        C = z @ w.T - np.outer(r, q) / T
        if kind == "cov":
            out = C / (T - 1)
        else:
            cii = (z * z).sum(axis=1) - r * r / T
            cjj = (w * w).sum(axis=1) - q * q / T
            out = np.clip(C / (np.sqrt(cii)[:, None] * np.sqrt(cjj)[None, :]), -1.0, 1.0)
    mu = np.where(fx == 2, np.nan, mu)
    nu = np.where(fy == 2, np.nan, nu)
    return _rules(out, fx, fy, kind, sym), mu, (None if sym else nu)


def restated(x, y=None):
    """exact()'s dict from the restatement: the reference of the shapes that 60-digit arithmetic is too
    slow for.  It sits within 3e-15 of exact() on every family (tests/test_cross_cpu.py), five orders
    below the bar."""
    x = np.asarray(x, dtype=np.float64)
    cov, mx, my = moments(x, y, "cov")
    corr = moments(x, y, "corr")[0]
    vx = np.diag(moments(x, None, "cov")[0])
    vy = vx if y is None else np.diag(moments(y, None, "cov")[0])
    with np.errstate(all="ignore"):
        scale = np.sqrt(vx)[:, None] * np.sqrt(vy)[None, :]
    return {"cov": cov, "corr": corr, "scale": scale, "mean_x": mx, "mean_y": my}


def one_pass(x, kind="cov"):
    """MLlib's RowMatrix.computeCovariance: (X'X - n m m') / (n - 1)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    m = x.sum(axis=1) / n
    c = (x @ x.T - n * np.outer(m, m)) / (n - 1)
    if kind == "cov":
        return c
    with np.errstate(all="ignore"):
        s = np.sqrt(np.diag(c))
        return c / np.outer(s, s)


def exact(x, y=None, dps=60):
    """-> dict(cov, corr, scale, mean_x, mean_y): the definition in dps-digit arithmetic, rounded
    once; scale = sqrt(C_ii C'_jj) / (T - 1), what the COV bar is relative to.  Series that the rules
    override (non-finite, constant) take no part in the arithmetic."""
    import mpmath as mp
    x = np.asarray(x, dtype=np.float64)
    sym = y is None
    yy = x if sym else np.asarray(y, dtype=np.float64)
    T = x.shape[1]
    fx, fy = flags(x), flags(yy)
    with mp.workdps(dps):
        def centred(a, f):
            rows, means = [], []
            for s in range(a.shape[0]):
                if f[s] == 2:
                    rows.append(None)
                    means.append(mp.nan)
                    continue
                v = [mp.mpf(float(t)) for t in a[s]]
                m = mp.fsum(v) / T
                rows.append([t - m for t in v])
                means.append(m)
            return rows, means
        zx, mx = centred(x, fx)
        zy, my = (zx, mx) if sym else centred(yy, fy)
        sxx = [mp.fsum(t * t for t in r) if r is not None else mp.nan for r in zx]
        syy = sxx if sym else [mp.fsum(t * t for t in r) if r is not None else mp.nan for r in zy]
        Sx, Sy = x.shape[0], yy.shape[0]
        cov, corr, scale = (np.full((Sx, Sy), np.nan) for _ in range(3))
        for i in range(Sx):
            if zx[i] is None:
                continue
            for j in range(Sy):
                if zy[j] is None:
                    continue
                if sym and j < i:
                    cov[i, j], corr[i, j], scale[i, j] = cov[j, i], corr[j, i], scale[j, i]
                    continue
                c = mp.fsum(a * b for a, b in zip(zx[i], zy[j]))
                root = mp.sqrt(sxx[i] * syy[j])
                cov[i, j] = float(c / (T - 1))
                scale[i, j] = float(root / (T - 1))
                corr[i, j] = float(c / root) if root != 0 else np.nan
        fl = lambda v: np.array([float(t) for t in v])
        return {"cov": _rules(cov, fx, fy, "cov", sym), "corr": _rules(np.clip(corr, -1.0, 1.0), fx, fy, "corr", sym),
                "scale": scale, "mean_x": fl(mx), "mean_y": None if sym else fl(my)}


def errors(got, ex, kind):
    """the largest error of `got` in units of the bar's scale, over the entries that are numbers in
    the exact result; the NaN patterns must agree"""
    got = np.asarray(got, dtype=np.float64)
    want = ex[kind]
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern"
    fin = ~np.isnan(want)
    if not fin.any():
        return 0.0
    d = np.abs(got[fin] - want[fin])
    if kind == "cov":
        sc = ex["scale"][fin]
        zero = sc == 0
        assert (d[zero] == 0).all(), "covariance against a constant series is exactly 0"
        d = d[~zero] / sc[~zero]
    return float(d.max()) if d.size else 0.0


def mean_bar(T):
    """any order of summing T values is within T 2^-53 sum |x| of their sum: per unit of max |x|, for the mean"""
    return T * 2.0 ** -53


def mean_error(got, want, x):
    """largest |mean - exact| per unit of the series' max |x|, over the finite series; NaN where exact is"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern of the means"
    fin = ~np.isnan(want)
    if not fin.any():
        return 0.0
    top = np.abs(np.asarray(x, dtype=np.float64)[fin]).max(axis=1)
    return float((np.abs(got[fin] - want[fin]) / np.where(top == 0, 1.0, top)).max())


# ---------------- the golden file: every family at GOLDEN_T steps, symmetric and against a second panel ----------------

def golden_case(name):
    x = family(name, GOLDEN_T)
    y = family(name, GOLDEN_T, seed=1)[:3]
    return x, y


def build_golden():
    hexl = lambda a: [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]
    rows = []
    for name in FAMILIES:
        x, y = golden_case(name)
        s, c = exact(x), exact(x, y)
        rows.append({"name": name, "T": GOLDEN_T, "Sx": int(x.shape[0]), "Sy": int(y.shape[0]),
                     "probe": hexl([x[0, 0], x[-1, -1], y[-1, -1]]),
                     "sym": {k: hexl(s[k]) for k in ("cov", "corr", "scale", "mean_x")},
                     "cross": {k: hexl(c[k]) for k in ("cov", "corr", "scale", "mean_x", "mean_y")}})
    return {"dps": 60, "rows": rows}


def load_golden():
    doc = json.load(open(GOLDEN))
    out = {}
    for row in doc["rows"]:
        un = lambda v, shape: np.array([float.fromhex(t) for t in v]).reshape(shape)
        Sx, Sy = row["Sx"], row["Sy"]
        g = {"probe": [float.fromhex(t) for t in row["probe"]]}
        for form, cols in (("sym", Sx), ("cross", Sy)):
            g[form] = {k: un(row[form][k], (Sx, cols)) for k in ("cov", "corr", "scale")}
            g[form]["mean_x"] = un(row[form]["mean_x"], (Sx,))
            g[form]["mean_y"] = un(row[form]["mean_y"], (Sy,)) if form == "cross" else None
        out[row["name"]] = g
    return out


if __name__ == "__main__":
    import sys
    doc = build_golden()
    if "--check" in sys.argv:
        assert json.load(open(GOLDEN)) == doc, "tests/golden/cross_exact.json is not what cross_ref.py writes"
    else:
        with open(GOLDEN, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
