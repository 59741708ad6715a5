// sts_transforms.hip -- the panel transforms of include/sts_transforms.h that are not recurrences
// (those are RecurLane ops in sts_recur.hip), bit-exact by construction:
//   quotients / price2ret                 S/UnivariateTimeSeries.scala:45-63
//   fillPrevious -> quotients, one pass   S/UnivariateTimeSeries.scala:194-204, :45-63
//   fillWithDefault                       S/UnivariateTimeSeries.scala:233-241
//   downsample / upsample                 S/UnivariateTimeSeries.scala:308-345
//   firstNotNaN / lastNotNaN              S/UnivariateTimeSeries.scala:119-139
// The streaming kernels are output-driven like sts_stream.hip's: threads map to consecutive output
// steps, every output element is written exactly once by a coalesced store, and only elements
// (s, t < T) are read.  The library is built with -ffp-contract=off and without fast-math, so
// a / b is the IEEE division and a / b - 1.0 stays a division and a subtraction.
#include "sts_elementwise.hpp"
#include "sts_internal.hpp"

#include <hip/hip_runtime.h>

namespace sts {
namespace {

constexpr int kWaves = kThreads / 64;   // wave-per-series kernels: series per workgroup

// ret(i) = ts(i + lag) / ts(i) [- 1.0], i < To = T - lag
__global__ __launch_bounds__(kThreads) void quotients_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                             int64_t S, int64_t To, int64_t ld_in, int64_t ld_out,
                                                             double rTo, int lag, bool minus_one) {
    for_each_out(S, To, rTo, [=](int64_t s, int64_t i) {
        const double* x = in + s * ld_in;
        const double q = x[i + lag] / x[i];
        out[s * ld_out + i] = minus_one ? q - 1.0 : q;
    });
}

// result(i) = if (result(i).isNaN) filler else result(i); in place allowed (element-wise)
__global__ __launch_bounds__(kThreads) void fill_default_kernel(const double* in, double* out, int64_t S, int64_t T,
                                                                int64_t ld_in, int64_t ld_out, double rT, double filler) {
    for_each_out(S, T, rT, [=](int64_t s, int64_t t) {
        const double v = in[s * ld_in + t];
        out[s * ld_out + t] = (v != v) ? filler : v;
    });
}

// sampledValues(j) = values(phase + j * n), j < To
__global__ __launch_bounds__(kThreads) void downsample_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                              int64_t S, int64_t To, int64_t ld_in, int64_t ld_out,
                                                              double rTo, int n, int phase) {
    for_each_out(S, To, rTo, [=](int64_t s, int64_t i) { out[s * ld_out + i] = in[s * ld_in + phase + i * n]; });
}

// sampledValues(phase + j * n) = values(j), the filler elsewhere; i < To = T * n, so (i - phase) / n < T
__global__ __launch_bounds__(kThreads) void upsample_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                            int64_t S, int64_t To, int64_t ld_in, int64_t ld_out,
                                                            double rTo, int n, int phase, double filler) {
    for_each_out(S, To, rTo, [=](int64_t s, int64_t i) {
        const int64_t k = i - phase;
        const int64_t q = k / n;
        const bool hit = k >= 0 && q * n == k;
        out[s * ld_out + i] = hit ? in[s * ld_in + q] : filler;
    });
}

__device__ __forceinline__ unsigned long long lanes_upto(int lane) {   // bits 0..lane
    return lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
}

// fillPrevious -> quotients(lag) [- 1.0], 1 <= lag <= 64, one wave per series, 64 steps per round:
//  * fillPrevious: a step's filled value is the value of the nearest valid step at or below it in
//    the round (ballot + one shuffle), else the carry of the rounds before (wave-uniform);
//  * the filled value `lag` steps back: lane - lag of this round's filled values, or of the round
//    before's (kept in a register), by one shuffle each at the same source lane (lane - lag mod 64);
//  * the quotient of step t lands at column t - lag: 64 consecutive doubles per store instruction,
//    8-byte stores, since the shift breaks any 16-byte alignment the row had.
// The next round's load is issued before this round's shuffles.  Steps t >= T are never read.
__global__ __launch_bounds__(kThreads) void fill_prev_quotients_kernel(const double* __restrict__ in,
                                                                       double* __restrict__ out, int64_t S, int64_t T,
                                                                       int64_t ld_in, int64_t ld_out, int lag,
                                                                       bool minus_one) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (s >= S) return;   // wave-uniform
    const double* x = in + s * ld_in;
    double* y = out + s * ld_out;
    const double kNaN = __builtin_nan("");
    const int src_back = (lane - lag) & 63;
    double carry = kNaN;      // fillPrevious' filler entering the round
    double fprev = kNaN;      // the round before's filled values
    double nxt = lane < T ? x[lane] : kNaN;
    for (int64_t tc = 0; tc < T; tc += 64) {
        const int64_t t = tc + lane;
        const double v = nxt;
        const int64_t tn = t + 64;
        nxt = tn < T ? x[tn] : kNaN;
        const unsigned long long valid = __ballot(v == v);   // steps past T hold NaN: never a source
        const unsigned long long below = valid & lanes_upto(lane);
        const double near = __shfl(v, below ? 63 - __builtin_clzll(below) : lane);
        const double f = below ? near : carry;
        const double last = __shfl(v, valid ? 63 - __builtin_clzll(valid) : 0);
        carry = valid ? last : carry;
        const double h_cur = __shfl(f, src_back), h_old = __shfl(fprev, src_back);
        const double h = lane >= lag ? h_cur : h_old;
        fprev = f;
        if (t < T && t >= lag) {
            const double q = f / h;
            y[t - lag] = minus_one ? q - 1.0 : q;
        }
    }
}

// firstNotNaN / lastNotNaN: one wave per series, 64 steps per ballot from each end, stopping at
// the first hit; only elements t < T are read
__global__ __launch_bounds__(kThreads) void first_last_kernel(const double* __restrict__ in, int64_t S, int64_t T,
                                                              int64_t ld, int64_t* __restrict__ first,
                                                              int64_t* __restrict__ last) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (s >= S) return;   // wave-uniform
    const double* x = in + s * ld;
    if (first) {
        int64_t f = T;
        for (int64_t tc = 0; tc < T; tc += 64) {
            const int64_t t = tc + lane;
            const double v = t < T ? x[t] : __builtin_nan("");
            const unsigned long long m = __ballot(v == v);
            if (m) {
                f = tc + __builtin_ctzll(m);
                break;
            }
        }
        if (lane == 0) first[s] = f;
    }
    if (last) {
        int64_t l = -1;
        for (int64_t hi = T; hi > 0; hi -= 64) {
            const int64_t t = hi - 1 - lane;   // lane 0 looks at the highest step
            const double v = t >= 0 ? x[t] : __builtin_nan("");
            const unsigned long long m = __ballot(v == v);
            if (m) {
                l = hi - 1 - __builtin_ctzll(m);
                break;
            }
        }
        if (lane == 0) last[s] = l;
    }
}

inline dim3 grid_waves(int64_t S) { return dim3((unsigned)((S + kWaves - 1) / kWaves)); }

}  // namespace

hipError_t launch_quotients(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int lag,
                            bool minus_one, hipStream_t st) {
    const int64_t To = T - lag;
    if (S <= 0 || To <= 0) return hipSuccess;
    return launch_elementwise(quotients_kernel, S * To, kChunk, st, in, out, S, To, ld_in, ld_out, 1.0 / (double)To, lag,
                              minus_one);
}

hipError_t launch_fill_prev_quotients(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                                      int lag, bool minus_one, hipStream_t st) {
    if (S <= 0 || T - lag <= 0) return hipSuccess;
    if (lag < 1 || lag > kFillQuotMaxLag) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fill_prev_quotients_kernel, grid_waves(S), dim3(kThreads), 0, st, in, out, S, T, ld_in, ld_out,
                       lag, minus_one);
    return hipGetLastError();
}

hipError_t launch_fill_default(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                               double filler, hipStream_t st) {
    return launch_elementwise(fill_default_kernel, S * T, kChunk, st, in, out, S, T, ld_in, ld_out, 1.0 / (double)T,
                              filler);
}

hipError_t launch_downsample(const double* in, double* out, int64_t S, int64_t T_out, int64_t ld_in, int64_t ld_out, int n,
                             int phase, hipStream_t st) {
    if (S <= 0 || T_out <= 0) return hipSuccess;
    return launch_elementwise(downsample_kernel, S * T_out, kChunk, st, in, out, S, T_out, ld_in, ld_out,
                              1.0 / (double)T_out, n, phase);
}

hipError_t launch_upsample(const double* in, double* out, int64_t S, int64_t T_out, int64_t ld_in, int64_t ld_out, int n,
                           int phase, double filler, hipStream_t st) {
    if (S <= 0 || T_out <= 0) return hipSuccess;
    return launch_elementwise(upsample_kernel, S * T_out, kChunk, st, in, out, S, T_out, ld_in, ld_out,
                              1.0 / (double)T_out, n, phase, filler);
}

hipError_t launch_first_last(const double* in, int64_t S, int64_t T, int64_t ld, int64_t* first, int64_t* last,
                             hipStream_t st) {
    if (S <= 0 || (!first && !last)) return hipSuccess;
    hipLaunchKernelGGL(first_last_kernel, grid_waves(S), dim3(kThreads), 0, st, in, S, T, ld, first, last);
    return hipGetLastError();
}

}  // namespace sts
