/*
 * sts_regress.h -- batched OLS regression of a panel on factors: the regression whose residuals
 * t5 / t6 of sts.h (sts_bp_test, sts_bg_test) take, and the effects pair that applies fitted
 * coefficients to other data.
 *
 * A sibling of sts.h.  The panel layout contract, the stream contract and the error contract of
 * sts.h hold here VERBATIM (series-contiguous fp64 panels with any 8-byte aligned base and any
 * ld >= T; results depend only on the elements (s, t < T); nothing outside the documented output
 * blocks is written and no input is written; every launch, memset, copy and scratch allocation of a
 * call is queued on `stream`, NULL = hipStreamPerThread, and the call returns without waiting unless
 * it takes err_per_series and is given NULL; every function returns an sts_status and
 * sts_last_error() gives the thread-local message).  The FACTOR PANEL layout is that of t5 / t6,
 * verbatim: factor j (0 <= j < k) of series s at time t is factors[s*fs + j*ld_f + t], ld_f >= T,
 * never written, nothing outside the T elements of a factor row is read; fs == 0 is ONE factor
 * matrix shared by the whole panel, fs != 0 per-series factors with fs >= (k - 1)*ld_f + T;
 * 1 <= k <= STS_MAX_FACTORS.  A Breeze DenseMatrix(T, k)'s `data` is this layout with ld_f = T
 * (INTEGRATION.md).  The guards of sts.h have twins for this header in
 * tests/test_factor_ols_cpu.py, and the bindings live in sparkts/_native.py REGRESS_SIGNATURES.
 *
 * The reference has no such operator of its own: its suite computes these regressions with
 * commons-math3 3.4.1 OLSMultipleLinearRegression (TimeSeriesStatisticalTestsSuite.scala:39-45,
 * 72-78), and that class with intercept is what the results are held to (1e-10 relative on
 * ordinary inputs).  JNI bindings do not exist for these entry points.
 */
#ifndef STS_REGRESS_H
#define STS_REGRESS_H

#include "sts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- g1: OLS with intercept of every series on 1, F_0 .. F_{k-1}, n = T rows.
 * beta:   S x (k+1), row s at beta + s*ld_b, ld_b >= k+1, the intercept first: the order of
 *         estimateRegressionParameters() after newSampleData(y, x) with intercept.
 * stderr: optional, S x (k+1) at the same ld_b: sqrt(sigma2 [(X'X)^-1]_ii),
 *         estimateRegressionParametersStandardErrors().
 * stats:  optional, S x 4 packed: rss (calculateResidualSumOfSquares), tss (the centred second
 *         moment, calculateTotalSumOfSquares), r2 (calculateRSquared) and
 *         sigma2 = rss / (T - k - 1) (estimateErrorVariance).
 * resid:  optional, the S x T residual panel, ld_r >= T: estimateResiduals().
 * err_per_series: optional, as everywhere in sts.h.
 *
 * k outside [1, STS_MAX_FACTORS], ld < T, ld_f < T, 0 < fs < (k - 1)*ld_f + T (or fs < 0),
 * ld_b < k + 1, ld_r < T, a null y / factors / beta -> STS_ERR_BAD_ARG.  T <= k + 1 ->
 * STS_ERR_NOT_ENOUGH_DATA (parity note of t5 / t6: the reference throws below equality only and
 * returns noise at equality).  Call-level errors leave the outputs untouched.
 * Per series: any NaN (or infinity) among the series' values or the factor rows it reads -> every
 * output of the series is NaN, its residual row included, status 0.  A rank-deficient design (a
 * constant or duplicated factor, by the 2^-40 rule of t5 / t6) -> STS_ERR_SINGULAR in
 * err_per_series and NaN outputs.  A bit-constant series is not an error: the factor coefficients
 * are 0, the intercept is the constant, residuals, rss, tss, sigma2 and the standard errors are 0
 * and r2 is NaN (the reference's 0 / 0).
 * Results do not depend on S, on neighbouring series or on whether the same factors arrive shared
 * or per series (bit for bit within one kernel regime, within the bar across regimes). */
int sts_factor_ols(const double* y, int64_t S, int64_t T, int64_t ld, const double* factors, int k,
                   int64_t ld_f, int64_t fs, double* beta, int64_t ld_b, double* stderr_out,
                   double* stats, double* resid, int64_t ld_r, int32_t* err_per_series,
                   void* stream);

/* ---- g2: the effects pair.  out(s, t) = in(s, t) - fit (remove) or in(s, t) + fit (add) with
 * fit = ((b0 + b1*f0[t]) + b2*f1[t]) + ..., formed left to right in that order without
 * contraction, b = beta + s*ld_b (ld_b >= k + 1, intercept first).  BIT-EXACT.  The coefficients
 * need not come from a fit on this data (out-of-sample hedged returns).  out == in with
 * ld_out == ld_in is allowed; NaNs propagate by arithmetic.  k, ld_f, fs, ld_b as in g1. */
int sts_factor_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                      int64_t ld_out, const double* factors, int k, int64_t ld_f, int64_t fs,
                      const double* beta, int64_t ld_b, void* stream);
int sts_factor_add(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                   int64_t ld_out, const double* factors, int k, int64_t ld_f, int64_t fs,
                   const double* beta, int64_t ld_b, void* stream);

/* ---- host-buffer variants: the staging pipeline of sts.h.  y / in, out and resid use the one
 * ld; beta and stderr are packed (ld_b = k + 1), stats is S x 4.  A shared factor matrix
 * (fs == 0) is copied to the device once; per-series factors travel with their series. ---- */
int sts_factor_ols_host(const double* y, int64_t S, int64_t T, int64_t ld, const double* factors,
                        int k, int64_t ld_f, int64_t fs, double* beta, double* stderr_out,
                        double* stats, double* resid, int32_t* err_per_series);
int sts_factor_remove_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld,
                           const double* factors, int k, int64_t ld_f, int64_t fs,
                           const double* beta);
int sts_factor_add_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld,
                        const double* factors, int k, int64_t ld_f, int64_t fs, const double* beta);

#ifdef __cplusplus
}
#endif
#endif /* STS_REGRESS_H */
