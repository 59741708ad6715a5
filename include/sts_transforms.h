/*
 * sts_transforms.h -- the panel transforms of libsts_hip.so: the operators of
 * UnivariateTimeSeries and TimeSeriesRDD that turn a price panel into something a fit can
 * take (returns, resampling, NaN trimming, inverse and order-d differencing).
 *
 * A sibling of sts.h.  The panel layout contract, the stream contract and the error
 * contract of sts.h hold here VERBATIM: series-contiguous fp64 panels with any 8-byte
 * aligned base and any ld >= T; results depend only on the elements (s, t < T); nothing
 * outside the documented output block is written and no input is written; reads stay
 * inside the 128-byte lines the panel touches; every launch, memset, copy and scratch
 * allocation of a call is queued on `stream` (NULL = hipStreamPerThread) and the call
 * returns without waiting, unless it takes err_per_series and is given NULL; every function
 * returns an sts_status and sts_last_error() gives the thread-local message.  The guards of
 * sts.h (tests/test_abi.py, tests/test_stream_table.py) have twins for this header in
 * tests/test_transforms_cpu.py, and the bindings live in sparkts/_native.py
 * TRANSFORM_SIGNATURES.
 *
 *   S/ = src/main/scala/com/cloudera/sparkts/ in the reference, as in sts.h.
 *
 * Arithmetic: IEEE binary64, true division, no FMA contraction.  Every result is BIT-EXACT:
 * each non-NaN element (signed zeros and infinities included) has the reference's bits and
 * NaN appears exactly where the reference has NaN.
 *
 * JNI bindings do not exist for these entry points.
 */
#ifndef STS_TRANSFORMS_H
#define STS_TRANSFORMS_H

#include "sts.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- r1: UnivariateTimeSeries.quotients(ts, lag) and price2ret(ts, lag)
 *      (S/UnivariateTimeSeries.scala:45-63); TimeSeriesRDD.returnRates is price2ret(_, 1).
 * out(s, i) = in(s, i + lag) / in(s, i), minus 1.0 when minus_one != 0, for i < T - lag: out has
 * T - lag columns, ld_out >= T - lag, and must not alias in.  lag outside [0, T] ->
 * STS_ERR_BAD_ARG; lag == T writes nothing. */
int sts_quotients(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                  int lag, int minus_one, void* stream);

/* ---- r2: fillts(method) (S/UnivariateTimeSeries.scala:141-297) followed by r1: the fused
 *      TimeSeriesRDD.fill(method) -> returnRates / quotients(lag).
 * method is any sts_fill_method, STS_FILL_NONE included (then this is r1).  Per-series fill
 * errors exactly as sts_fill reports them (err_per_series: device, S entries, optional; NULL ->
 * the call waits and returns the first failing status); a failing series' quotients are those of
 * what sts_fill leaves in its row.  STS_FILL_PREVIOUS with 1 <= lag <= 32 is ONE pass over HBM
 * (S*T read, S*(T - lag) written, no scratch); every other method or lag fills into
 * stream-ordered scratch and runs r1 on it.  The result is sts_fill then sts_quotients, bit for
 * bit. */
int sts_fill_quotients(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                       int64_t ld_out, int method, int lag, int minus_one, int32_t* err_per_series,
                       void* stream);

/* ---- r3: UnivariateTimeSeries.fillWithDefault(values, filler)
 *      (S/UnivariateTimeSeries.scala:233-241): NaN -> filler, everything else copied.
 * out == in with ld_out == ld_in is allowed. */
int sts_fill_with_default(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                          int64_t ld_out, double filler, void* stream);

/* ---- r4: UnivariateTimeSeries.downsample(values, n, phase) and upsample(values, n, phase,
 *      useZero) (S/UnivariateTimeSeries.scala:308-345).
 * downsample: out(s, j) = in(s, phase + j*n) for j < newLen = ceil((T - phase) / n); newLen is 0
 * when phase >= T.  n < 1 or phase < 0 -> STS_ERR_BAD_ARG.  ld_out >= newLen.
 * upsample: out has T*n columns (ld_out >= T*n, T*n within the reference's Int range);
 * out(s, phase + j*n) = in(s, j) and every other element is a quiet NaN, or +0.0 when use_zero
 * != 0.  n < 1 or phase outside [0, n) -> STS_ERR_BAD_ARG (the reference runs off its array).
 * out must not alias in. */
int sts_downsample(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                   int n, int phase, void* stream);
int sts_upsample(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                 int n, int phase, int use_zero, void* stream);

/* ---- r5: UnivariateTimeSeries.firstNotNaN / lastNotNaN (S/UnivariateTimeSeries.scala:119-139),
 *      what trimLeading / trimTrailing (:98-117) and TimeSeriesRDD.filterStartingBefore /
 *      filterEndingAfter (S/TimeSeriesRDD.scala:115-126) are built on.
 * first[s] = the first t with a non-NaN value, T for an all-NaN series; last[s] = the last such
 * t, -1 for an all-NaN series.  Device int64 arrays of S entries; either may be NULL. */
int sts_first_last_not_nan(const double* in, int64_t S, int64_t T, int64_t ld, int64_t* first,
                           int64_t* last, void* stream);

/* ---- r6: UnivariateTimeSeries.inverseDifferencesAtLag(diffedTs, destTs, lag, startIndex)
 *      (S/UnivariateTimeSeries.scala:397-417; the (diffedTs, lag) wrapper :425-427 is start = lag).
 * out(i) = i < start ? in(i) : in(i) + out(i - lag), sequential along each chain.  out == in
 * (same pointer and ld) gives the same bits.  start < lag -> STS_ERR_REQUIREMENT; lag == 0
 * leaves out untouched (:404-405). */
int sts_inverse_diff_at_lag(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                            int64_t ld_out, int lag, int start, void* stream);

/* ---- r7: UnivariateTimeSeries.differencesOfOrderD(ts, d) and inverseDifferencesOfOrderD(
 *      diffedTs, d) (S/UnivariateTimeSeries.scala:438-465): d sweeps of differencesAtLag(_, _, 1, i),
 *      i = 1..d, and of inverseDifferencesAtLag(_, _, 1, i), i = d..1; the same subtractions /
 *      additions in the same order.  Full length: the first d elements are kept as the sweeps
 *      leave them.  d < 0 -> STS_ERR_BAD_ARG; d == 0 copies.  out must not alias in (the
 *      reference returns a copy). */
int sts_diff_order_d(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                     int64_t ld_out, int d, void* stream);
int sts_inverse_diff_order_d(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                             int64_t ld_out, int d, void* stream);

/* ---- host-buffer variants: the staging pipeline of sts.h ("host-buffer variants").  Panels of
 * the input's width use the input's ld; an output of another width (quotients, resampling) is
 * packed, ld = its width. ---- */
int sts_quotients_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int lag,
                       int minus_one);
int sts_fill_quotients_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld,
                            int method, int lag, int minus_one, int32_t* err_per_series);
int sts_fill_with_default_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld,
                               double filler);
int sts_downsample_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int n,
                        int phase);
int sts_upsample_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int n,
                      int phase, int use_zero);
int sts_first_last_not_nan_host(const double* in, int64_t S, int64_t T, int64_t ld, int64_t* first,
                                int64_t* last);
int sts_inverse_diff_at_lag_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld,
                                 int lag, int start);
int sts_diff_order_d_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int d);
int sts_inverse_diff_order_d_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld,
                                  int d);

#ifdef __cplusplus
}
#endif
#endif /* STS_TRANSFORMS_H */
