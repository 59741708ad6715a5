/*
 * sts_cross.h -- covariance and correlation matrices of a panel (every series against every other)
 * and of two panels (every series of x against every series of y): what the reference hands to
 * MLlib (toRowMatrix().computeCovariance(), Statistics.corr on the instants) after fill ->
 * returnRates, or after regress(F).residuals.
 *
 * A sibling of sts.h.  The panel layout contract, the stream contract and the error contract of
 * sts.h hold here VERBATIM (series-contiguous fp64 panels with any 8-byte aligned base and any
 * ld >= T; results depend only on the elements (s, t < T); nothing outside the documented output
 * blocks is written and no input is written; every launch and scratch allocation of a call is
 * queued on `stream`, NULL = hipStreamPerThread, and the call returns without waiting; every
 * function returns an sts_status and sts_last_error() gives the thread-local message).  The guards
 * of sts.h have twins for this header in tests/test_cross_cpu.py, and the bindings live in
 * sparkts/_native.py CROSS_SIGNATURES.  JNI bindings do not exist for these entry points.
 *
 * DEFINITION.  With mu_i = (sum_t x_i[t]) / T, z_i[t] = x_i[t] - mu_i and r_i = sum_t z_i[t]
 * (w_j, q_j the same quantities of y_j):
 *     C_ij = sum_t z_i[t] w_j[t] - r_i q_j / T          the corrected two-pass form
 *     COV  = C_ij / (T - 1)
 *     CORR = C_ij / (sqrt(C_ii) sqrt(C'_jj)), clamped to [-1, 1]   (the two roots are multiplied,
 *            not the two sums: data scaled by 2^-400 or 2^400 keep their digits)
 * and mean_x / mean_y receive mu.  This is NOT MLlib's one-pass (X'X - n m m') / (n - 1), which
 * loses every digit on series far from their own level; the results are held to
 * exact arithmetic: |COV - exact| <= 1e-10 sqrt(C_ii C'_jj) / (T - 1), |CORR - exact| <= 1e-10.
 *
 * PER SERIES (there is no err_per_series: nothing here is a per-series error).
 *   - A series with a non-finite value among its T elements: NaN in its whole row (and, in the
 *     symmetric form, its column), NaN mean.  No other entry changes by a bit.
 *   - A bit-constant series (max == min): COV is exactly +0.0 against every finite series, CORR is
 *     NaN, the diagonal included (commons-math3 PearsonsCorrelation's 0 / 0).
 *   - The symmetric CORR diagonal is exactly 1.0 for every other finite series.
 *
 * REPRODUCIBILITY.  out(i, j) is a function of the bits of row i, the bits of row j, T and kind,
 * and of nothing else: not of Sx, Sy or any ld, not of where the two rows sit in their panels, not
 * of what their neighbours hold, and not of whether y is NULL or a bit-copy of x (the CORR diagonal
 * excepted: exactly 1.0 is the symmetric form's rule).  So the symmetric output is exactly
 * symmetric, and a row permutation of x permutes the output bit for bit.  Sums over T are closed at
 * multiples of STS_CROSS_SPLIT steps (boundaries that depend on T alone) and merged in ascending
 * order without floating-point atomics, whether one workgroup walks them all or one each.
 */
#ifndef STS_CROSS_H
#define STS_CROSS_H

#include "sts.h"

/* Tuning sizes of csrc/sts_cross.hip (build-time -D overrides; the tests read them here): the
 * square output tile of a workgroup, the steps of T one LDS stage holds, and the steps after which
 * a partial sum over T is closed. */
#ifndef STS_CROSS_TILE
#define STS_CROSS_TILE 64
#endif
#ifndef STS_CROSS_CHUNK
#define STS_CROSS_CHUNK 16
#endif
#ifndef STS_CROSS_SPLIT
#define STS_CROSS_SPLIT 8192
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { STS_CROSS_COV = 0, STS_CROSS_CORR = 1 } sts_cross_kind;
int sts_cross_kind_from_name(const char* name);          /* "cov" / "corr"; -2 otherwise */

/* ---- c1: out(i, j), 0 <= i < Sx, 0 <= j < Sy, at out + i*ld_o + j, ld_o >= Sy.
 * y == NULL: the symmetric form (Sy, ld_y ignored; Sy := Sx, y := x); only the tiles on or above
 * the diagonal are computed and the others are their mirror.
 * mean_x (Sx), mean_y (Sy): optional outputs; mean_y must be NULL when y is NULL.
 *
 * A null x or out, Sx < 1, Sy < 1 with y, ld_x < T, ld_y < T with y, ld_o < Sy, kind outside the
 * enum, mean_y without y, out overlapping an input -> STS_ERR_BAD_ARG.  T < 2 ->
 * STS_ERR_NOT_ENOUGH_DATA.  Call-level errors leave the outputs untouched. */
int sts_cross_moments(const double* x, int64_t Sx, int64_t T, int64_t ld_x,
                      const double* y, int64_t Sy, int64_t ld_y, int kind,
                      double* out, int64_t ld_o, double* mean_x, double* mean_y, void* stream);

/* ---- host-buffer variant: out packed (ld_o = Sy, or Sx in the symmetric form).  A matrix needs
 * every series of both panels, so the panels are copied to the device whole (row by row, only the
 * T elements of a row are read), not in chunks of series.  Bit-identical to the device path. ---- */
int sts_cross_moments_host(const double* x, int64_t Sx, int64_t T, int64_t ld_x,
                           const double* y, int64_t Sy, int64_t ld_y, int kind,
                           double* out, double* mean_x, double* mean_y);

#ifdef __cplusplus
}
#endif
#endif /* STS_CROSS_H */
