// sts_regress.hip -- batched OLS with intercept of a panel on factors (include/sts_regress.h g1) and
// the effects pair that applies fitted coefficients (g2).  What the results are held to is
// commons-math3 3.4.1 OLSMultipleLinearRegression with intercept.
//
// Numerical form.  The factors' centred columns get the orthonormal basis Q
// of sts_factor_basis.hpp, the one bgtest / bptest use, with the triangular factor kept: F_c = Q R.
// With y_c the series centred on y - y[0] (and the rounding-level rest of its mean taken out of the
// intercept and the residuals):
//   c = Q'y_c,  beta_F = R^-1 c,  b0 = ybar - beta_F . fbar,  resid = y_c - sum_j c_j q_j (explicit),
//   rss = sum resid^2 (never tss - ess),  r2 = ess / tss with ess = sum c_j^2,
//   se_F[j]^2 = sigma2 |row j of R^-1|^2,  se_0^2 = sigma2 (1 / T + |R^-T fbar|^2).
// Everything that depends on the factors alone (Q, R^-1, fbar, the row norms, 1/T + |R^-T fbar|^2)
// is built once per factor matrix (FactorBasisArgs::aux).
//
// One kernel body, four regimes (ols_regime):
//   0  shared factors whose basis fits LDS next to kHotWaves series: the hot path.  A workgroup of
//      kHotWaves waves stages the basis in LDS once, then every wave walks several series on its own
//      (no barrier after the staging): a series comes from HBM once, into the wave's LDS row, and the
//      mean, projection and residual sweeps run there.
//   1  one wave per series, the series in LDS, the basis read from the scratch through the caches
//      (shared factors with a longer T; per-series factors that do not fit LDS).
//   2  per-series factors that fit LDS behind the series: the wave builds its own basis there.
//   3  T > kStatOneWave: 256 threads per series sweep global memory as often as needed (correct at
//      any T, not tuned; neither is regime 1).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sts_elementwise.hpp"
#include "sts_factor_basis.hpp"
#include "sts_internal.hpp"
#include "sts_wgsum.hpp"

// the hot path's shape: waves per workgroup and the most series one wave walks (0 waves: regime 0 is
// never taken -- one 64-thread workgroup per series, the other form measured in section 5.20)
#ifndef STS_OLS_WAVES
#define STS_OLS_WAVES 4
#endif
#ifndef STS_OLS_SPW
#define STS_OLS_SPW 8
#endif

namespace sts {
namespace {

constexpr int kHotWaves = STS_OLS_WAVES > 0 ? STS_OLS_WAVES : 1;
constexpr int kHotSeriesPerWave = STS_OLS_SPW;
constexpr size_t kStageLds = 60 << 10;      // regime 0: basis + kHotWaves series

// The fit of one series by NT threads (tid of them): g its T values, Q / aux its basis, ys its LDS
// row when YLDS; k <= KB, the bound the per-factor registers are unrolled to.  Every reduced value is
// uniform over the NT threads.
template <int NT, bool YLDS, int KB>
__device__ __forceinline__ void ols_fit(const OlsArgs& a, int64_t s, int tid, const double* __restrict__ g,
                                        const double* Q, const double* aux, bool singular, double* ys, double* red) {
    const int64_t T = a.T;
    const int k = a.f.k;
    double* beta = a.beta + s * a.ld_b;
    double* se = a.se ? a.se + s * a.ld_b : nullptr;
    double* stats = a.stats ? a.stats + s * 4 : nullptr;
    double* resid = a.resid ? a.resid + s * a.ld_r : nullptr;
    if (singular) {   // uniform
        if (resid)
            for (int64_t t = tid; t < T; t += NT) resid[t] = NAN;
        if (tid == 0) {
            for (int c = 0; c <= k; c++) {
                beta[c] = NAN;
                if (se) se[c] = NAN;
            }
            if (stats)
                for (int c = 0; c < 4; c++) stats[c] = NAN;
            if (a.err) a.err[s] = STS_ERR_SINGULAR;
        }
        return;
    }
    const double dn = (double)T;
    // sweep 1: the mean on y - y[0], so that the level does not eat the spread's digits
    const double y0 = g[0];
    double acc = 0.0;
    for (int64_t t = tid; t < T; t += NT) {
        const double d = g[t] - y0;
        if constexpr (YLDS) ys[t] = d;   // each thread reads back its own steps
        acc += d;
    }
    const double mu1 = bsum<NT>(acc, red) / dn;
    // sweep 2: what is left of the mean (a second centring: rounding noise of the first, it moves the
    // intercept alone and is left out of the sums below, where it enters squared or against the
    // centred q), the centred total and the components on the basis -- one tree for all of them
    double sums[KB + 2];
#pragma unroll
    for (int c = 0; c < KB + 2; c++) sums[c] = 0.0;
    for (int64_t t = tid; t < T; t += NT) {
        double v;
        if constexpr (YLDS) ys[t] = v = ys[t] - mu1;
        else v = (g[t] - y0) - mu1;
        sums[0] += v;
        sums[1] += v * v;
#pragma unroll
        for (int c = 0; c < KB; c++)
            if (c < k) sums[2 + c] += Q[(int64_t)c * T + t] * v;
    }
    bsum_many<NT>(sums, k + 2, red);
    const double mu2 = sums[0] / dn;
    // sweep 3: the residuals, explicitly
    double rss = 0.0;
    for (int64_t t = tid; t < T; t += NT) {
        double r;
        if constexpr (YLDS) r = ys[t] - mu2;
        else r = ((g[t] - y0) - mu1) - mu2;
#pragma unroll
        for (int c = 0; c < KB; c++)
            if (c < k) r -= sums[2 + c] * Q[(int64_t)c * T + t];
        rss += r * r;
        if (resid) resid[t] = r;
    }
    rss = bsum<NT>(rss, red);
    if (tid != 0) return;
    double ess = 0.0, dot = 0.0;
    const double sigma2 = rss / (double)(T - k - 1);
#pragma unroll
    for (int i = 0; i < KB; i++)
        if (i < k) {
            double b = 0.0;
#pragma unroll
            for (int j = i; j < KB; j++)
                if (j < k) b += aux[kAuxRinv + i * kMaxFactors + j] * sums[2 + j];
            beta[1 + i] = b;
            if (se) se[1 + i] = sqrt(sigma2 * aux[kAuxRow2 + i]);
            dot += b * aux[kAuxMean + i];
            ess += sums[2 + i] * sums[2 + i];
        }
    beta[0] = (y0 + (mu1 + mu2)) - dot;
    if (se) se[0] = sqrt(sigma2 * aux[kAuxH]);
    if (stats) {
        stats[0] = rss;
        stats[1] = ess != ess ? NAN : sums[1];   // a NaN among the factors: every output is NaN
        stats[2] = ess / sums[1];                // a bit-constant series: the reference's 0 / 0
        stats[3] = sigma2;
    }
}

// QMODE 0: basis in the scratch; 1: the shared basis and its aux staged in LDS in front of the NW series rows;
// 2: the series' own basis built in LDS behind its row.  NW > 1 only with NT = 64 (independent waves).
template <int NT, int NW, bool YLDS, int QMODE, int KB>
__global__ __launch_bounds__(NT* NW) void ols_kernel(OlsArgs a, int64_t s0, int64_t ns, int spw) {
    extern __shared__ double dyn[];
    static_assert(NW == 1 || NT == 64, "several series per workgroup: one wave each");
    double* red = nullptr;
    if constexpr (NT > 64) {
        __shared__ double red_s[(KB + 2) * 4];
        red = red_s;
    }
    const int tid = NW > 1 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int w = NW > 1 ? (int)(threadIdx.x >> 6) : 0;
    const int64_t T = a.T;
    const int k = a.f.k;
    bool shared_singular = false;
    if constexpr (QMODE == 1) {
        const int64_t nq = (int64_t)k * T;
        for (int64_t i = threadIdx.x; i < nq; i += NT * NW) dyn[i] = a.f.basis[i];
        for (int i = threadIdx.x; i < kAuxR; i += NT * NW) dyn[nq + i] = a.f.aux[i];   // what the fits read of it
        shared_singular = a.f.info[0] != 0;
        __syncthreads();
    }
    double* ys = QMODE == 1 ? dyn + (int64_t)k * T + kAuxR + (int64_t)w * T : dyn;
    const int64_t first = (int64_t)blockIdx.x * NW * spw;
    for (int i = 0; i < spw; i++) {
        const int64_t b = first + (int64_t)i * NW + w;
        if (b >= ns) break;   // uniform over the series' threads
        const int64_t s = s0 + b;
        const double* Q;
        const double* aux;
        bool singular;
        if constexpr (QMODE == 2) {
            double* q = dyn + T;
            double* ax = q + (int64_t)k * T;
            singular = build_basis<NT, true>(a.f.factors + s * a.f.fs, a.f.ld_f, k, T, q, ax, red);
            __syncthreads();   // thread 0's aux
            Q = q;
            aux = ax;
        } else {
            aux = QMODE == 1 ? dyn + (int64_t)k * T : a.f.aux + b * a.f.aux_stride;
            singular = QMODE == 1 ? shared_singular : a.f.info[b * a.f.info_stride] != 0;
            Q = QMODE == 1 ? dyn : a.f.basis + b * a.f.basis_stride;
        }
        ols_fit<NT, YLDS, KB>(a, s, tid, a.y + s * a.ld, Q, aux, singular, ys, red);
    }
}

// out = in -/+ ((b0 + b1 f0[t]) + b2 f1[t]) + ..., left to right (no contraction: -ffp-contract=off)
template <bool ADD>
__global__ __launch_bounds__(kThreads) void factor_effects_kernel(const double* in, double* out, int64_t S, int64_t T,
                                                                  int64_t ld_in, int64_t ld_out,
                                                                  const double* __restrict__ factors, int k,
                                                                  int64_t ld_f, int64_t fs,
                                                                  const double* __restrict__ beta, int64_t ld_b,
                                                                  double rT) {
    for_each_out(S, T, rT, [=](int64_t s, int64_t t) {
        const double* b = beta + s * ld_b;
        const double* f = factors + s * fs + t;
        double fit = b[0];
        for (int j = 0; j < k; j++) fit = fit + b[1 + j] * f[(int64_t)j * ld_f];
        const double v = in[s * ld_in + t];
        out[s * ld_out + t] = ADD ? v + fit : v - fit;
    });
}

}  // namespace

int ols_regime(int64_t T, int k, int64_t fs) {
    if (T > kStatOneWave) return 3;
    if (fs == 0) return STS_OLS_WAVES > 0 && (size_t)(kHotWaves + k) * (size_t)T * sizeof(double) <= kStageLds ? 0 : 1;
    return own_basis_fits(T, k, T, fs) ? 2 : 1;
}

// the kernel of a regime, its per-factor registers unrolled to 4 (k <= 4) or to kMaxFactors
template <int NT, int NW, bool YLDS, int QMODE>
static void launch_ols_kernel(const OlsArgs& a, int64_t s0, int64_t ns, int spw, int64_t blocks, size_t lds, hipStream_t st) {
    if (a.f.k <= 4)
        hipLaunchKernelGGL((ols_kernel<NT, NW, YLDS, QMODE, 4>), dim3((unsigned)blocks), dim3(NT * NW), lds, st, a, s0, ns, spw);
    else
        hipLaunchKernelGGL((ols_kernel<NT, NW, YLDS, QMODE, kMaxFactors>), dim3((unsigned)blocks), dim3(NT * NW), lds, st, a,
                           s0, ns, spw);
}

hipError_t launch_ols(const OlsArgs& a, int64_t s0, int64_t ns, hipStream_t st) {
    const size_t row = (size_t)a.T * sizeof(double);
    switch (ols_regime(a.T, a.f.k, a.f.fs)) {
    case 0: {
        // enough workgroups to fill the chip before a wave takes a second series
        const int64_t want = ns / ((int64_t)kHotWaves * 2048);
        const int spw = (int)(want < 1 ? 1 : want > kHotSeriesPerWave ? kHotSeriesPerWave : want);
        const int64_t per = (int64_t)kHotWaves * spw;
        launch_ols_kernel<64, kHotWaves, true, 1>(a, s0, ns, spw, (ns + per - 1) / per,
                                                  (size_t)(kHotWaves + a.f.k) * row + kAuxR * sizeof(double), st);
        break;
    }
    case 1:
        launch_ols_kernel<64, 1, true, 0>(a, s0, ns, 1, ns, row, st);
        break;
    case 2:
        launch_ols_kernel<64, 1, true, 2>(a, s0, ns, 1, ns, (size_t)(1 + a.f.k) * row + kOlsAux * sizeof(double), st);
        break;
    default:
        launch_ols_kernel<kLongThreads, 1, false, 0>(a, s0, ns, 1, ns, 0, st);
    }
    return hipGetLastError();
}

hipError_t launch_factor_effects(bool add, const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                                 int64_t ld_out, const double* factors, int k, int64_t ld_f, int64_t fs,
                                 const double* beta, int64_t ld_b, hipStream_t st) {
    if (S <= 0 || T <= 0) return hipSuccess;
    const double rT = 1.0 / (double)T;
    if (add)
        return launch_elementwise(factor_effects_kernel<true>, S * T, kChunk, st, in, out, S, T, ld_in, ld_out, factors, k,
                                  ld_f, fs, beta, ld_b, rT);
    return launch_elementwise(factor_effects_kernel<false>, S * T, kChunk, st, in, out, S, T, ld_in, ld_out, factors, k,
                              ld_f, fs, beta, ld_b, rT);
}

}  // namespace sts
