/*
 * sts_sample.h -- the samplers of libsts_hip.so: `sample(n, rand)` of the reference's ARModel,
 * ARIMAModel, GARCHModel and ARGARCHModel for whole panels, drawn from a seeded counter-based
 * stream so that any shard of any path can be regenerated on any rank.  (EWMAModel has no
 * sample in the reference and none here.)
 *
 * A sibling of sts.h, like sts_transforms.h.  The panel layout contract, the stream contract and
 * the error contract of sts.h hold here VERBATIM: series-contiguous fp64 panels with any 8-byte
 * aligned base and any ld >= n; nothing outside the output block (s, i < n) is written; every
 * launch of a call is queued on `stream` (NULL = hipStreamPerThread) and the call returns without
 * waiting (no entry point here takes err_per_series); every function returns an sts_status and
 * sts_last_error() gives the thread-local message.  The guards of sts.h (tests/test_abi.py,
 * tests/test_stream_table.py) have twins for this header in tests/test_sample_cpu.py, the stream
 * rows live in tests/test_sample_stream_gpu.py, and the bindings in sparkts/_native.py
 * SAMPLE_SIGNATURES.
 *
 *   S/ = src/main/scala/com/cloudera/sparkts/ in the reference, as in sts.h.
 *
 * ---- The stream: z(seed, series, t) ----
 * The reference takes whatever commons-math3 RandomGenerator the caller hands it and calls
 * nextGaussian() n times.  This engine's generator is a pure function of (seed, global series
 * index, position), defined once in csrc/sts_normal.hpp and restated in tests/sample_ref.py:
 *   words    Philox4x32-10, key = (lo32 seed, hi32 seed), counter = (lo32 k, hi32 k, lo32 g, hi32 g)
 *            with g the global series index and k = (t >> 1) | 2^63.  Bit 63 keeps the stream
 *            disjoint from sts_gen_panel's under the same seed.  An even t takes words 0 and 1 of
 *            the call, an odd t words 2 and 3.
 *   uniform  m = ((wa >> 6) << 26) | (wb >> 6) (52 bits), u = (2m + 1) * 2^-53: exact, in (0, 1).
 *   normal   z = Wichura's AS 241 PPND16 of u, in IEEE binary64 with + - * / only, true division,
 *            no FMA contraction, a correctly rounded sqrt and fdlibm's log (StrictMath.log).
 *            |z| <= 8.209536151601386.
 * Every entry point takes
 *   s0    the global index of the call's first series: a shard regenerates its rows anywhere;
 *   t0    the position of the first draw in each series' stream: a caller that advances t0 by n
 *         after each call gets independent paths, like a stateful RandomGenerator;
 *   seed, stream   last.
 * Series s of a call consumes the draws g_i = z(seed, s0 + s, t0 + i), i < n, and nothing else.
 *
 * Arithmetic: every result is BIT-EXACT against the restatement: each non-NaN element (signed
 * zeros and infinities included) has its bits and NaN appears exactly where it has NaN.  Model
 * parameters are NOT validated: a non-stationary set gives the NaNs and infinities the reference's
 * arithmetic gives, in the same places.
 *
 * Common argument rules: out is (S, n) with ld >= n; S, n >= 0; n within the reference's Int range;
 * s0 < 0, t0 < 0, or a NULL parameter array with S > 0 -> STS_ERR_BAD_ARG.  S == 0 or n == 0
 * returns STS_OK and writes nothing (the reference's GARCH samplers index variances(0) of an empty
 * array at n == 0 and throw; its AR / ARIMA samplers return an empty vector).  Parameter arrays are
 * device arrays with one entry (one row) per series, as on the `_add` entry points of sts.h.
 * Argument errors are reported before any device is needed.
 *
 * `_host` variants and JNI bindings do not exist for these entry points: the
 * paths are made where they are consumed, on the device.
 */
#ifndef STS_SAMPLE_H
#define STS_SAMPLE_H

#include "sts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- m1: the raw panel of draws: out(s, i) = z(seed, s0 + s, t0 + i). */
int sts_sample_normal(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, int64_t t0, uint64_t seed,
                      void* stream);

/* ---- m2: GARCHModel.sample(n, rand) (S/models/GARCH.scala:162-183), one fused kernel: the draws
 *      never reach HBM.  NOT addTimeDependentEffects of the draws:
 *   h_0 = omega / (1 - alpha - beta);  eta = sqrt(h_0) * g_0  (consumed);  out(s, 0) = +0.0
 *   h_i = (omega + beta * h_{i-1}) + (alpha * eta) * eta;  eta = sqrt(h_i) * g_i;  out(s, i) = eta */
int sts_garch_sample(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, const double* omega,
                     const double* alpha, const double* beta, int64_t t0, uint64_t seed, void* stream);

/* ---- m3: ARGARCHModel.sample(n, rand) (S/models/GARCH.scala:235-256): the same variance
 *      recurrence with out(s, i) = (c + phi * out(s, i - 1)) + eta for i >= 1, out(s, 0) = +0.0. */
int sts_argarch_sample(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, const double* c,
                       const double* phi, const double* omega, const double* alpha, const double* beta,
                       int64_t t0, uint64_t seed, void* stream);

/* ---- m4: ARModel.sample(n, rand) (S/models/Autoregression.scala:90-93): addTimeDependentEffects(
 *      vec, vec) of the draws -- m1 into out, then sts_ar_add in place, both queued on `stream`.
 * c: S intercepts, coef: S x p; p < 0 -> STS_ERR_BAD_ARG, as sts_ar_add. */
int sts_ar_sample(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, const double* c,
                  const double* coef, int p, int64_t t0, uint64_t seed, void* stream);

/* ---- m5: ARIMAModel.sample(n, rand) (S/models/ARIMA.scala:517-520): m1 into out, then
 *      sts_arima_add in place, both queued on `stream`.  coef: S x ((include_intercept ? 1 : 0) +
 *      p + q); the order limits and argument checks are those of sts_arima_add (0 <= p, q <=
 *      STS_ARIMA_MAX_ORDER, 0 <= d <= n, at least one coefficient). */
int sts_arima_sample(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, int p, int d, int q,
                     int include_intercept, const double* coef, int64_t t0, uint64_t seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STS_SAMPLE_H */
