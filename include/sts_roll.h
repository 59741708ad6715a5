/*
 * sts_roll.h -- rolling-window statistics of a panel, alone (sum, mean, var, std, min, max, zscore)
 * and against a second panel or one shared factor (cov, corr, beta): what a user of a price or
 * returns panel computes between returnRates and a fit -- rolling volatility, rolling z-scores,
 * rolling maxima for drawdowns, rolling beta against a market factor.
 *
 * A sibling of sts.h.  The panel layout contract, the stream contract and the error contract of
 * sts.h hold here VERBATIM (series-contiguous fp64 panels with any 8-byte aligned base and any
 * ld >= T; results depend only on the elements (s, t < T); nothing outside the documented output
 * blocks is written and no input is written; every launch of a call is queued on `stream`,
 * NULL = hipStreamPerThread, and the call returns without waiting; every function returns an
 * sts_status and sts_last_error() gives the thread-local message).  The guards of sts.h have twins
 * for this header in tests/test_roll_cpu.py, and the bindings live in sparkts/_native.py
 * ROLL_SIGNATURES.  JNI bindings do not exist for these entry points.
 *
 * DEFINITION.  out is (S, T), as long as the input: out(s, t) belongs to the trailing window
 * W(t) = [max(0, t - window + 1), t] of series s.  All arithmetic is IEEE binary64 without FMA
 * contraction, in exactly this order.  A step u of the window is VALID when x[u] is not NaN (for the
 * pair ops: neither x[u] nor y[u] is NaN); n is the number of valid steps and every sum runs over
 * the valid steps in ascending u.
 *     n < min_periods      -> quiet NaN
 *     SUM     s = the first valid value, then s = s + x[u]
 *     MEAN    p = s / (double)n
 *     MIN/MAX the bits of an element of the window; among values that compare equal -0.0 wins MIN
 *             and +0.0 wins MAX
 *     VAR     n < 2 -> NaN.  r = sum (x - p), q = sum (x - p) * (x - p), both started from +0.0;
 *             M2 = q - (r * r) / n; M2 is exactly +0.0 when the window's min equals its max and is
 *             finite (the bit-constant rule of sts_cross.h: fill("previous") makes such windows);
 *             a negative M2 is clamped to +0.0; VAR = M2 / (n - 1)
 *     STD     sqrt(VAR)
 *     ZSCORE  (x[t] - p) / STD: NaN when x[t] is NaN, and NaN where STD is 0 (a constant window: p
 *             need not round to the constant, so the quotient alone would be an infinity)
 *     pair    px, py, rx, ry, M2x, M2y as above over the pairwise-valid steps (n < 2 -> NaN);
 *             c = sum (x - px) * (y - py); Cxy = c - (rx * ry) / n, exactly +0.0 when one side is
 *             constant by the rule above and the other holds no infinity
 *             COV  = Cxy / (n - 1)
 *             CORR = Cxy / (sqrt(M2x) * sqrt(M2y)), clamped to [-1, 1]; NaN (0 / 0) when a side
 *                    is constant
 *             BETA = Cxy / M2y, the slope of x on y; NaN when y is constant
 * An infinity is an ordinary value and whatever the formulas give is the result: SUM is +-inf or
 * NaN, VAR and the pair ops are NaN through inf - inf.
 * window > T is legal: every window is then truncated.  The window is capped at
 * STS_ROLL_MAX_WINDOW because this definition makes an output cost O(window).
 *
 * PURITY.  out(s, t) is a function of the ordered valid values of its own window, of x[t] for
 * ZSCORE, of window, min_periods and the op, and of nothing else: not of t, T, S, any ld or Sy, not
 * of where the row sits in the panel, of what its neighbours hold or of tile and launch
 * boundaries.  Every window is evaluated directly, in the order above; no sum is slid, differenced
 * or shared between windows.  So a window truncated at the series start equals a full window whose
 * missing part is NaN; a series shifted by k steps gives shifted bits; and a non-finite element
 * costs exactly the windows that contain it -- no other output changes by a bit.
 *
 * ACCURACY.  Against exact rational arithmetic the definition stays within 1e-10 of the window's
 * own M2 for VAR's M2, of sqrt(M2x M2y) for Cxy and of max |x| over the window for MEAN, also on
 * price walks at level 1e9 and on data scaled by 2^400 or 2^-400 (measured worst cases: DESIGN.md
 * section 5.22); the difference of two cumulative sums does not.
 */
#ifndef STS_ROLL_H
#define STS_ROLL_H

#include "sts.h"

#define STS_ROLL_MAX_WINDOW 1024

/* Tuning sizes of csrc/sts_roll.hip (build-time -D overrides; the tests read them here).  A
 * workgroup owns STS_ROLL_TILE consecutive steps of one row and loads them with their window - 1
 * halo; when T <= STS_ROLL_TILE it owns whole rows instead, as many as fit its buffer:
 *     rows per workgroup = (STS_ROLL_TILE + STS_ROLL_MAX_WINDOW - 1) / (T + window - 1).
 * Every thread carries STS_ROLL_CHAINS outputs at a time as independent chains. */
#ifndef STS_ROLL_TILE
#define STS_ROLL_TILE 2048
#endif
#ifndef STS_ROLL_CHAINS
#define STS_ROLL_CHAINS 4
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { STS_ROLL_SUM = 0, STS_ROLL_MEAN = 1, STS_ROLL_VAR = 2, STS_ROLL_STD = 3, STS_ROLL_MIN = 4, STS_ROLL_MAX = 5, STS_ROLL_ZSCORE = 6 } sts_roll_op;
typedef enum { STS_ROLL_COV = 0, STS_ROLL_CORR = 1, STS_ROLL_BETA = 2 } sts_roll_pair_op;
int sts_roll_op_from_name(const char* name);       /* "sum" "mean" "var" "std" "min" "max" "zscore"; -2 otherwise */
int sts_roll_pair_op_from_name(const char* name);  /* "cov" "corr" "beta"; -2 otherwise */

/* ---- r1: out(s, t) at out + s*ld_out + t = op over the trailing window of in(s, .).
 * A null pointer, S < 1, T < 1, ld_in < T, ld_out < T, window outside [1, STS_ROLL_MAX_WINDOW],
 * min_periods outside [1, window], op outside sts_roll_op, out overlapping in (an in-place call
 * included) -> STS_ERR_BAD_ARG.  Call-level errors leave the output untouched. */
int sts_roll_stat(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                  int window, int min_periods, int op, void* stream);

/* ---- r2: the pair ops of x(s, .) against y(s, .) (Sy == S, rows ld_y apart) or against the one
 * shared factor y[0 .. T) (Sy == 1; ld_y is ignored).  The guards of r1 for x, y and out, and:
 * Sy not in {1, S}, ld_y < T when Sy == S and S > 1, op outside sts_roll_pair_op, out overlapping
 * x or y -> STS_ERR_BAD_ARG. */
int sts_roll_pair(const double* x, const double* y, int64_t Sy, int64_t ld_y, double* out, int64_t S, int64_t T,
                  int64_t ld_x, int64_t ld_out, int window, int min_periods, int op, void* stream);

/* ---- host-buffer variants: the staging pipeline of sts.h's _host entry points by chunks of
 * series (x and out share ld; a shared factor is uploaded once); bit-identical to the device path. ---- */
int sts_roll_stat_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int window, int min_periods,
                       int op);
int sts_roll_pair_host(const double* x, const double* y, int64_t Sy, int64_t ld_y, double* out, int64_t S, int64_t T,
                       int64_t ld, int window, int min_periods, int op);

#ifdef __cplusplus
}
#endif
#endif /* STS_ROLL_H */
