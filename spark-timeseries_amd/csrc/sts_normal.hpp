// sts_normal.hpp -- the reproducible standard normal z(seed, series, t) of include/sts_sample.h,
// plain C++ for host and device (tests/native/normal_harness.cpp compiles it for the host and
// tests/sample_ref.py restates it; all three agree bit for bit).
//
//   words   Philox4x32-10, key = (lo32 seed, hi32 seed) as sts_gen.hip keys its stream, counter =
//           (lo32 k, hi32 k, lo32 g, hi32 g) with g the GLOBAL series index and k = (t >> 1) | 2^63.
//           Bit 63 keeps the stream apart from sts_gen_panel's under the same seed: its counters
//           are t < T < 2^31 and ~0, and t >> 1 < 2^62 never sets the bits below bit 63 to ones.
//           One call feeds two adjacent steps: an even t takes words 0 and 1, an odd t words 2 and 3.
//   uniform m = ((wa >> 6) << 26) | (wb >> 6), 52 bits; u = (2m + 1) 2^-53: exact, inside (0, 1),
//           symmetric about 0.5, and 1 - u is exact too.
//   normal  Wichura's AS 241 PPND16 of u (Applied Statistics 37 (3), 1988): the central rational
//           for |u - 0.5| <= 0.425, else r = sqrt(-log(min(u, 1 - u))) and the two tail rationals
//           split at r <= 5.  + - * / only (IEEE division, built without contraction),
//           __builtin_sqrt (correctly rounded) and the fdlibm log of sts_fdlibm.hpp.  The extreme
//           values are +-8.209536151601386 (m = 0 and m = 2^52 - 1); log(0) is never reached.
//
// The three regions are each a ratio of two degree-7 Horner chains, written as branches: a wave
// nearly always holds lanes of the central region and of the first tail (15 % of the draws), so it
// runs both; selecting each lane's 16 coefficients instead costs two v_cndmask_b32 per coefficient,
// 32 full-rate VALU instructions against the 28 full-rate FP64 instructions of the second chain.
#pragma once
#include <stdint.h>

#include "sts_fdlibm.hpp"

namespace sts {

STS_FD_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                    uint32_t out[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0;
        const uint32_t n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// the four words shared by the steps 2k' and 2k' + 1 of series g (t >> 1 == k')
STS_FD_HD inline void normal_words(uint64_t seed, uint64_t g, uint64_t t, uint32_t w[4]) {
    const uint64_t k = (t >> 1) | ((uint64_t)1 << 63);
    philox4x32_10((uint32_t)k, (uint32_t)(k >> 32), (uint32_t)g, (uint32_t)(g >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), w);
}

STS_FD_HD inline double uniform_of_m(uint64_t m) { return (double)(2 * m + 1) * 0x1p-53; }

STS_FD_HD inline double uniform52(uint32_t wa, uint32_t wb) {
    return uniform_of_m(((uint64_t)(wa >> 6) << 26) | (uint64_t)(wb >> 6));
}

// AS 241 PPND16; the coefficients and the branch structure of CPython's
// statistics._normal_dist_inv_cdf (mu = 0, sigma = 1 dropped: 0.0 + x * 1.0 is x for x != -0.0)
STS_FD_HD inline double ppnd16(double p) {
    const double q = p - 0.5;
    const double aq = q < 0.0 ? -q : q;
    if (aq <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r +
                                 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                               1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                             1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r +
                                 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                               5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                             4.2313330701600911252e+1) * r + 1.0);
        return num / den;
    }
    double r = q <= 0.0 ? p : 1.0 - p;
    r = __builtin_sqrt(-fdlibm_log(r));
    double num, den;
    if (r <= 5.0) {
        r = r - 1.6;
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r +
                    2.41780725177450611770e-1) * r + 1.27045825245236838258e+0) * r +
                  3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r +
                    1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
                  6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                2.05319162663775882187e+0) * r + 1.0);
    } else {
        r = r - 5.0;
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r +
                    1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
                  2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r +
                    1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
                  1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                5.99832206555887937690e-1) * r + 1.0);
    }
    const double x = num / den;
    return q < 0.0 ? -x : x;
}

// the draw of step t from the words of its pair
STS_FD_HD inline double normal_of_words(const uint32_t w[4], uint64_t t) {
    return (t & 1) ? ppnd16(uniform52(w[2], w[3])) : ppnd16(uniform52(w[0], w[1]));
}

STS_FD_HD inline double normal_z(uint64_t seed, uint64_t g, uint64_t t) {
    uint32_t w[4];
    normal_words(seed, g, t, w);
    return normal_of_words(w, t);
}

}  // namespace sts
