// sts_stream.hip -- element-parallel streaming operators (no recurrence):
//   differencesAtLag (out of place)  S/UnivariateTimeSeries.scala:356-376
//   EWMAModel.removeTimeDependentEffects (out of place)  S/models/EWMA.scala:125-133
//   ARModel.removeTimeDependentEffects (out of place)    S/models/Autoregression.scala:60-73
//   Lag.lagMatTrimBoth (standalone)                      S/Lag.scala:62-77
// Each output element depends on a few inputs at fixed backward offsets, so threads
// map to consecutive steps (coalesced along time) and the backward re-reads are L1/L2
// hits.  The arithmetic is written in the reference's order and the library is built
// with -ffp-contract=off, so every result is bit-exact.
#include "sts_elementwise.hpp"
#include "sts_internal.hpp"

#include <hip/hip_runtime.h>

namespace sts {
namespace {

__global__ __launch_bounds__(kThreads) void diff_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                        int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                                                        double rT, int lag, int start) {
    for_each_out(S, T, rT, [=](int64_t s, int64_t t) {
        const double* x = in + s * ld_in;
        out[s * ld_out + t] = (t < start) ? x[t] : x[t] - x[t - lag];
    });
}

__global__ __launch_bounds__(kThreads) void ewma_remove_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                               int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                                                               double rT, const double* __restrict__ sm) {
    for_each_out(S, T, rT, [=](int64_t s, int64_t t) {
        const double* x = in + s * ld_in;
        const double sv = sm[s];
        // dest(i) = (ts(i) - (1 - smoothing) * ts(i - 1)) / smoothing,   EWMA.scala:131
        out[s * ld_out + t] = (t == 0) ? x[0] : (x[t] - (1.0 - sv) * x[t - 1]) / sv;
    });
}

__global__ __launch_bounds__(kThreads) void ar_remove_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                             int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                                                             double rT, const double* __restrict__ c,
                                                             const double* __restrict__ coef, int p) {
    for_each_out<kPerThread, 2>(S, T, rT, [=](int64_t s, int64_t t) {
        const double* x = in + s * ld_in;
        const double* cf = coef + s * p;
        // dest(i) = ts(i) - c; dest(i) -= ts(i - j - 1) * coefficients(j)   Autoregression.scala:64-68
        double d = x[t] - c[s];
        for (int k = 0; k < p && t - k - 1 >= 0; k++) d -= x[t - k - 1] * cf[k];
        out[s * ld_out + t] = d;
    });
}

// out for series s: (T - p) x ncols column-major at out + s * (T - p) * ncols;
// M(r, c - init) = x(r + p - c)
__global__ __launch_bounds__(kThreads) void lagmat_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                          int64_t S, int64_t T, int64_t ld_in, int p, int init,
                                                          int ncols, double rR) {
    const int64_t rows = T - p;
    for_each_out(S * (int64_t)ncols, rows, rR, [=](int64_t col, int64_t r, int64_t g) {   // col = s * ncols + k
        const int64_t s = col / ncols;
        const int k = (int)(col - s * ncols);
        const int c = k + init;
        out[g] = in[s * ld_in + r + p - c];
    });
}

}  // namespace

hipError_t launch_diff(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                       int lag, int start, hipStream_t st) {
    return launch_elementwise(diff_kernel, S * T, kChunk, st, in, out, S, T, ld_in, ld_out, 1.0 / (double)T, lag, start);
}

hipError_t launch_ewma_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                              int64_t ld_out, const double* sm, hipStream_t st) {
    return launch_elementwise(ewma_remove_kernel, S * T, kChunk, st, in, out, S, T, ld_in, ld_out, 1.0 / (double)T, sm);
}

hipError_t launch_ar_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                            int64_t ld_out, const double* c, const double* coef, int p, hipStream_t st) {
    return launch_elementwise(ar_remove_kernel, S * T, kChunk, st, in, out, S, T, ld_in, ld_out, 1.0 / (double)T, c,
                              coef, p);
}

hipError_t launch_lagmat(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int max_lag,
                         int include_original, hipStream_t st) {
    const int64_t rows = T - max_lag;
    const int ncols = max_lag + (include_original ? 1 : 0);
    return launch_elementwise(lagmat_kernel, S * ncols * rows, kChunk, st, in, out, S, T, ld_in, max_lag,
                              include_original ? 0 : 1, ncols, 1.0 / (double)rows);
}

}  // namespace sts
