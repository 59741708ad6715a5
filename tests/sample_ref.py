"""Checker for include/sts_sample.h (helper module, not collected): the stream z(seed, series, t)
and the four `sample` loops of the reference, restated in float64 Python.

* philox: Philox4x32-10 in numpy uint64 arithmetic (cross-checked against oracle.gen_panel by
  tests/test_sample_cpu.py);
* ppnd16: Wichura's AS 241 PPND16 with the coefficients and the branch structure of CPython's
  statistics._normal_dist_inv_cdf, math.log replaced by oracle.fdlibm_log;
* garch_sample / argarch_sample: GARCHModel.sample and ARGARCHModel.sample
  (S/models/GARCH.scala:162-183, :235-256) in the source's operand order;
* ar_sample / arima_sample: addTimeDependentEffects(vec, vec) on the reference Gaussians
  (S/models/Autoregression.scala:90-93, S/models/ARIMA.scala:517-520) through oracle.ar_add and
  tests/arima_ref.py.

Python floats are IEEE binary64 and nothing here contracts.
"""
import math

import numpy as np

import arima_ref
import oracle

M32 = np.uint64(0xFFFFFFFF)
EXTREME = 8.209536151601386     # |z| at m = 0 and m = 2^52 - 1


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit words held in uint64 -> four arrays of words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0) & M32, np.uint64(k1) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & M32, n2, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def words(seed, g, t):
    """the four words of the pair of step t of series g (arrays broadcast)"""
    g, t = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(t, dtype=np.uint64))
    k = (t >> np.uint64(1)) | np.uint64(1 << 63)
    seed = int(seed) & (2 ** 64 - 1)
    return philox(k & M32, k >> np.uint64(32), g & M32, g >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)


def mantissa(seed, g, t):
    """m of step t: 52 bits from words (0, 1) for an even t, (2, 3) for an odd one"""
    w = words(seed, g, t)
    odd = (np.asarray(t, dtype=np.uint64) & np.uint64(1)).astype(bool)
    wa, wb = np.where(odd, w[2], w[0]), np.where(odd, w[3], w[1])
    return ((wa >> np.uint64(6)) << np.uint64(26)) | (wb >> np.uint64(6))


def uniform(m):
    return float(2 * int(m) + 1) * 2.0 ** -53       # 2m + 1 < 2^53: the conversion is exact


A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
     1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
     5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
     3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
     6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
     2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
     1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


def horner(c, r):
    v = c[0] * r + c[1]
    for a in c[2:]:
        v = v * r + a
    return v


def ppnd16(p, log=None):
    """AS 241 PPND16 of p; log defaults to oracle.fdlibm_log"""
    log = oracle.fdlibm_log if log is None else log
    q = p - 0.5
    if abs(q) <= 0.425:
        r = 0.180625 - q * q
        return (horner(A, r) * q) / horner(B, r)
    r = p if q <= 0.0 else 1.0 - p
    r = math.sqrt(-log(r))
    if r <= 5.0:
        r = r - 1.6
        x = horner(C, r) / horner(D, r)
    else:
        r = r - 5.0
        x = horner(E, r) / horner(F, r)
    return -x if q < 0.0 else x


def normal_of_m(m, log=None):
    return ppnd16(uniform(m), log)


def normals(seed, g, t):
    """z(seed, g, t) for broadcast arrays of series and steps -> float64 array of their shape"""
    m = mantissa(seed, g, t)
    flat = np.array([normal_of_m(v) for v in m.ravel()], dtype=np.float64)
    return flat.reshape(m.shape)


def normal_panel(seed, s0, S, t0, n):
    """what sts_sample_normal(out, s0, S, n, ld, t0, seed) writes"""
    g = (np.arange(S, dtype=np.uint64) + np.uint64(s0))[:, None]
    t = (np.arange(n, dtype=np.uint64) + np.uint64(t0))[None, :]
    return normals(seed, g, t)


def garch_sample(g, omega, alpha, beta, c=None, phi=None):
    """sampleWithVariances(n, rand)._1 with rand.nextGaussian() = g[0], g[1], ...; ARGARCH when c
    and phi are given.  Scala's  omega + beta * variances(i-1) + alpha * eta * eta  groups as
    (omega + beta * h) + ((alpha * eta) * eta), and  c + phi * ts(i - 1) + eta  as (c + phi * ts) + eta."""
    omega, alpha, beta = float(omega), float(alpha), float(beta)
    n = len(g)
    ts = [0.0] * n
    with np.errstate(all="ignore"):
        h = float(np.float64(omega) / np.float64(1.0 - alpha - beta))     # IEEE division: no ZeroDivisionError
        eta = float(np.sqrt(np.float64(h))) * float(g[0])                 # sqrt of a negative: NaN, no ValueError
        for i in range(1, n):
            h = (omega + beta * h) + (alpha * eta) * eta
            eta = float(np.sqrt(np.float64(h))) * float(g[i])
            ts[i] = eta if c is None else (float(c) + float(phi) * ts[i - 1]) + eta
    return np.array(ts, dtype=np.float64)


def ar_sample(g, c, coef):
    return oracle.ar_add(np.array(g, dtype=np.float64), float(c), np.asarray(coef, dtype=np.float64), inplace=True)


def arima_sample(g, p, d, q, coef, icpt):
    return arima_ref.add_effects(p, d, q, coef, icpt, g)


def assert_bits(got, want, what=""):
    """every non-NaN element (signed zeros, infinities) has the reference's bits, NaN sits where it has NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN at other places (first %s)" % (what, np.argwhere(gn != wn)[:1].tolist())
    bad = (np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(want).view(np.uint64)) & ~wn
    assert not bad.any(), "%s: %d elements differ, first at %s: %r != %r" % (
        what, int(bad.sum()), np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0])
