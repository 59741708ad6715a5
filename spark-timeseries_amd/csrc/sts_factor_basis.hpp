// sts_factor_basis.hpp -- the orthonormal basis of a factor matrix's centred columns, shared by
// Breusch-Godfrey / Breusch-Pagan (sts_stattests.hip) and the factor OLS (sts_regress.hip):
// F_c = Q R by twice-applied modified Gram-Schmidt (DESIGN.md sections 5.15 and 5.20).  The tests need
// Q alone; the fit also keeps R and the column means and derives its coefficients' map from them.
#pragma once

#include <cstdint>

#include "sts_internal.hpp"
#include "sts_wgsum.hpp"

namespace sts {

// A remainder of at most this share of the centred column counts as none: twice-applied
// Gram-Schmidt leaves rounding noise of a few ulps of the column where exact arithmetic leaves 0
// (a duplicated factor), and a factor collinear to 1e-6 leaves a million times the bound.
constexpr double kBasisTol2 = 0x1p-80;   // (2^-40)^2, on squared norms

// FactorBasisArgs::aux, per basis; rows of the k x k blocks are kMaxFactors apart
constexpr int kAuxRinv = 0;     // R^-1, upper triangle
constexpr int kAuxMean = 64;    // fbar
constexpr int kAuxRow2 = 72;    // |row i of R^-1|^2
constexpr int kAuxH = 80;       // 1 / n + |R^-T fbar|^2 (81: reserved)
constexpr int kAuxR = 88;       // R itself (working storage of the builder)
constexpr int kOlsAux = 152;
static_assert(kAuxR + kMaxFactors * kMaxFactors == kOlsAux && kMaxFactors == 8, "aux layout");

// What the fit derives from a full-rank R and the means, by the thread that kept them: R^-1 by back
// substitution per unit column, its squared row norms and 1 / n + |R^-T fbar|^2
__device__ __forceinline__ void basis_fit_terms(double* aux, int k, int64_t n) {
    const double* R = aux + kAuxR;
    double* inv = aux + kAuxRinv;
    for (int c = 0; c < k; c++)
        for (int r = c; r >= 0; r--) {
            double v = r == c ? 1.0 : 0.0;
            for (int j = r + 1; j <= c; j++) v -= R[r * kMaxFactors + j] * inv[j * kMaxFactors + c];
            inv[r * kMaxFactors + c] = v / R[r * kMaxFactors + r];
        }
    double h = 0.0;
    for (int i = 0; i < k; i++) {
        double r2 = 0.0, wi = 0.0;
        for (int j = i; j < k; j++) r2 += inv[i * kMaxFactors + j] * inv[i * kMaxFactors + j];
        for (int r = 0; r <= i; r++) wi += inv[r * kMaxFactors + i] * aux[kAuxMean + r];   // (R^-T fbar)[i]
        aux[kAuxRow2 + i] = r2;
        h += wi * wi;
    }
    aux[kAuxH] = 1.0 / (double)n + h;
}

// The orthonormal basis of one factor matrix: Q (k x n, row c at Q + c * n; global scratch or LDS),
// from rows 0..n of the k factor rows at F; true when the factors are rank deficient.  Each thread
// owns its rows i = tid, tid + NT, .. of every column, so the in-place sweeps need no ordering
// between threads; only the dot products cross lanes.  KEEP_R: thread 0 also keeps the column means
// and the triangular factor in aux (R[c][j] the sum of the two coefficients of column j on q_c,
// R[j][j] the remaining norm) and, at full rank, derives the fit's terms from them; it alone writes
// and re-reads aux, and callers order it against the other threads' reads.
template <int NT, bool KEEP_R>
__device__ __forceinline__ bool build_basis(const double* __restrict__ F, int64_t ld_f, int k, int64_t n, double* Q,
                                            double* aux, double* red) {
    const int tid = threadIdx.x;
    const double dn = (double)n;
    for (int j = 0; j < k; j++) {
        const double* __restrict__ f = F + (int64_t)j * ld_f;
        double* q = Q + (int64_t)j * n;
        // centred column: sums on f - f[0] so that the level does not eat the spread's digits
        const double f0 = f[0];
        double acc = 0.0;
        for (int64_t i = tid; i < n; i += NT) acc += f[i] - f0;
        const double mu = bsum<NT>(acc, red) / dn;
        acc = 0.0;
        for (int64_t i = tid; i < n; i += NT) {
            const double v = (f[i] - f0) - mu;
            q[i] = v;
            acc += v;
        }
        const double mu2 = bsum<NT>(acc, red) / dn;
        acc = 0.0;
        for (int64_t i = tid; i < n; i += NT) {
            const double v = q[i] - mu2;
            q[i] = v;
            acc += v * v;
        }
        const double c2 = bsum<NT>(acc, red);
        if constexpr (KEEP_R)
            if (tid == 0) aux[kAuxMean + j] = f0 + (mu + mu2);
        // modified Gram-Schmidt against the earlier columns, twice
        for (int pass = 0; pass < 2; pass++)
            for (int c = 0; c < j; c++) {
                const double* qc = Q + (int64_t)c * n;
                acc = 0.0;
                for (int64_t i = tid; i < n; i += NT) acc += qc[i] * q[i];
                const double d = bsum<NT>(acc, red);
                for (int64_t i = tid; i < n; i += NT) q[i] -= d * qc[i];
                if constexpr (KEEP_R)
                    if (tid == 0) aux[kAuxR + c * kMaxFactors + j] = pass == 0 ? d : aux[kAuxR + c * kMaxFactors + j] + d;
            }
        acc = 0.0;
        for (int64_t i = tid; i < n; i += NT) acc += q[i] * q[i];
        const double w2 = bsum<NT>(acc, red);
        if (w2 <= kBasisTol2 * c2) return true;   // uniform; NaN passes (NaN in, NaN out, status 0)
        const double w = sqrt(w2);
        for (int64_t i = tid; i < n; i += NT) q[i] /= w;
        if constexpr (KEEP_R)
            if (tid == 0) aux[kAuxR + j * kMaxFactors + j] = w;
    }
    if constexpr (KEEP_R)
        if (tid == 0) basis_fit_terms(aux, k, n);
    return false;
}

// One workgroup per factor matrix, into the scratch: f.basis, f.info (0 or STS_ERR_SINGULAR), f.aux
template <int NT, bool KEEP_R>
__global__ __launch_bounds__(NT) void factor_basis_kernel(FactorBasisArgs f, int64_t s0) {
    __shared__ double red[4];
    const int64_t b = blockIdx.x;
    const bool singular = build_basis<NT, KEEP_R>(f.factors + (s0 + b) * f.fs + f.lo, f.ld_f, f.k, f.n,
                                                  f.basis + b * f.basis_stride,
                                                  KEEP_R ? f.aux + b * f.aux_stride : nullptr, red);
    if (threadIdx.x == 0) f.info[b] = singular ? STS_ERR_SINGULAR : 0;
}

}  // namespace sts
