// sts_sample.hip -- the samplers of include/sts_sample.h, bit-exact against tests/sample_ref.py:
//   the panel of draws z(seed, series, t)   sts_normal.hpp
//   GARCHModel.sample                       S/models/GARCH.scala:162-183
//   ARGARCHModel.sample                     S/models/GARCH.scala:235-256
// ARModel.sample and ARIMAModel.sample are the draw panel followed by the in-place add kernels
// (sts_api.cpp), as the reference's sample is addTimeDependentEffects(vec, vec).
//
// One Philox call feeds the two steps 2k and 2k + 1 of a series, so both kernels walk PAIRS of
// absolute steps and drop the halves that fall outside [t0, t0 + n): an odd t0 costs one extra
// call per row (per row and chunk in the fused kernel), never another stream.
#include "sts_internal.hpp"
#include "sts_lane_rows.hpp"
#include "sts_normal.hpp"

#include <hip/hip_runtime.h>

namespace sts {
namespace {

constexpr int kThreads = 256;

// out(s, i) = z(seed, s0 + s, t0 + i).  One thread per (series, pair): thread j of a row holds the
// steps 2 (k0 + j) and 2 (k0 + j) + 1, k0 = t0 >> 1, so consecutive threads store consecutive 16 B.
__global__ __launch_bounds__(kThreads) void sample_normal_kernel(SampleArgs a, int64_t pairs, double rpairs) {
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= a.S * pairs) return;
    // (s, j) of g by a double reciprocal + fix-up (sts_transforms.hip split)
    int64_t s = (int64_t)((double)g * rpairs);
    int64_t b = s * pairs;
    if (b > g) { s--; b -= pairs; }
    else if (b + pairs <= g) { s++; b += pairs; }
    const int64_t j = g - b;
    const uint64_t t = (((uint64_t)a.t0 >> 1) + (uint64_t)j) << 1;   // the pair's even step
    const int64_t i = (int64_t)(t - (uint64_t)a.t0);                 // its column: -1 for the first pair of an odd t0
    uint32_t w[4];
    normal_words(a.seed, (uint64_t)(a.s0 + s), t, w);
    double* row = a.out + s * a.ld;
    if (i >= 0) row[i] = normal_of_words(w, 0);
    if (i + 1 < a.n) row[i + 1] = normal_of_words(w, 1);
}

// GARCHModel.sample / ARGARCHModel.sample: one lane per series, SPW series per wave, CH steps per
// chunk, in the shape of garch_effects_kernel (sts_garch.hip) with the store half of map_rows
// (sts_lane_rows.hpp) written out: over map_rows itself this kernel ran 0.9 % slower.  Where
// garch_effects_kernel loads its rows from HBM, each lane here GENERATES its row's draws into the LDS
// tile; the recurrence then runs over the row in place, and the tile leaves by coalesced stores:
// only the paths touch HBM.
//   variances(0) = omega / (1 - alpha - beta);  eta = sqrt(variances(0)) * g(0);  ts(0) stays 0.0
//   variances(i) = omega + beta * variances(i - 1) + alpha * eta * eta        (Scala: left to right)
//   eta = sqrt(variances(i)) * g(i);  ts(i) = eta   |   c + phi * ts(i - 1) + eta
// No parameter is validated: the reference's arithmetic, NaN and infinities included.
template <bool AR, int SPW = 64, int CH = 32>
__global__ __launch_bounds__(64) void garch_sample_kernel(SampleArgs a) {
    static_assert(SPW == 64 && 64 % CH == 0, "a lane per row; whole rows per store instruction");
    constexpr int kRow = CH + 1;
    constexpr int NST = SPW * CH / 64;
    __shared__ double tile[SPW * kRow];
    const int lane = threadIdx.x;
    const int64_t sb = (int64_t)blockIdx.x * SPW;
    const int64_t sl = sb + lane;
    const bool live = sl < a.S;
    const int ns = (a.S - sb < SPW) ? (int)(a.S - sb) : SPW;
    const int64_t n = a.n;
    double c = 0.0, phi = 0.0, omega = 0.0, alpha = 0.0, beta = 0.0;
    if (live) {
        omega = a.omega[sl];
        alpha = a.alpha[sl];
        beta = a.beta[sl];
        if (AR) {
            c = a.c[sl];
            phi = a.phi[sl];
        }
    }
    const uint64_t gs = (uint64_t)(a.s0 + sl);
    double* myrow = tile + lane * kRow;
    double eta = 0.0, h = 0.0, prevY = 0.0;
    for (int64_t tc = 0; tc < n; tc += CH) {
        const int len = (n - tc < CH) ? (int)(n - tc) : CH;
        if (live) {
            // the draws of columns [0, len): absolute steps [ta, ta + len), pair by pair
            const uint64_t ta = (uint64_t)a.t0 + (uint64_t)tc;
            const uint64_t te = ta + (uint64_t)len;
            for (uint64_t t = ta & ~(uint64_t)1; t < te; t += 2) {
                uint32_t w[4];
                normal_words(a.seed, gs, t, w);
                if (t >= ta) myrow[(int)(t - ta)] = normal_of_words(w, 0);
                if (t + 1 < te) myrow[(int)(t + 1 - ta)] = normal_of_words(w, 1);
            }
            for (int cc = 0; cc < len; cc++) {
                const double g = myrow[cc];
                double y;
                if (tc + cc == 0) {
                    h = omega / (1.0 - alpha - beta);
                    eta = __builtin_sqrt(h) * g;
                    y = 0.0;
                } else {
                    h = (omega + beta * h) + (alpha * eta) * eta;
                    eta = __builtin_sqrt(h) * g;
                    y = AR ? (c + phi * prevY) + eta : eta;
                }
                prevY = y;
                myrow[cc] = y;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NST; i++) {
            const int row = (i * 64 + lane) / CH, col = (i * 64 + lane) % CH;
            if (row < ns && col < len) a.out[(sb + row) * a.ld + tc + col] = tile[row * kRow + col];
        }
        __syncthreads();
    }
}

constexpr int kSampleSpw = 64, kSampleCh = 32;   // garch_sample_kernel's shape

}  // namespace

hipError_t launch_sample_normal(const SampleArgs& a, hipStream_t st) {
    if (a.S <= 0 || a.n <= 0) return hipSuccess;
    const int64_t pairs = (int64_t)((((uint64_t)a.t0 + (uint64_t)a.n - 1) >> 1) - ((uint64_t)a.t0 >> 1)) + 1;
    const int64_t blocks = (a.S * pairs + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_normal_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, a, pairs,
                       1.0 / (double)pairs);
    return hipGetLastError();
}

hipError_t launch_garch_sample(bool ar, const SampleArgs& a, hipStream_t st) {
    if (a.S <= 0 || a.n <= 0) return hipSuccess;
    if (ar) return launch_lane_rows(garch_sample_kernel<true, kSampleSpw, kSampleCh>, a.S, kSampleSpw, st, a);
    return launch_lane_rows(garch_sample_kernel<false, kSampleSpw, kSampleCh>, a.S, kSampleSpw, st, a);
}

}  // namespace sts
