// sts_stattests.hip -- batched TimeSeriesStatisticalTests (S/stats/TimeSeriesStatisticalTests.scala):
// dwtest (:241-252), kpsstest (:359-421), adftest (:204-232), the lbtest epilogue (:289-298) and the
// p-values (MacKinnon 1994 for ADF, the chi-squared upper tail for Ljung-Box).
//
// One workgroup owns one series.  Series of up to kStatOneWave steps take a one-wave workgroup
// that loads the series once into LDS (plain coalesced 8-byte loads: any base / ld the layout
// contract allows, and no read outside the elements) and makes every further sweep there;
// longer series take a 256-thread workgroup that sweeps global memory as often as the method
// needs (the re-reads hit the caches; correct at any T, not tuned).  Durbin-Watson needs one sweep
// and no LDS in either form.
//
// Numerics (statistical tests): KPSS and ADF never form x - fitted in plain
// arithmetic.  Every detrended value is x - (t0 + t1 u + t2 f2(u)) evaluated with error-free
// transformations (TwoSum, FMA products) on centred orthogonal polynomials u = i - (n-1)/2,
// f2 = u^2 - (n^2-1)/12, so a series at level 1e6 with noise 1e-2 keeps its residuals to an ulp
// of the RESIDUAL.  KPSS refines (a, b) once from the residuals' own sums (its cumulative sum
// turns a constant residual offset into a first-order error).  ADF is the Frisch-Waugh two-pass
// form, twice: detrend every column, then take the lags out of the level and the response.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sts_factor_basis.hpp"
#include "sts_internal.hpp"
#include "sts_wgsum.hpp"

namespace sts {
namespace {

constexpr int kMaxCols = 33;   // ADF: 31 lags + level + response

// ---- workgroup-wide inclusive scan (the sums: sts_wgsum.hpp) ----
template <int NT>
__device__ __forceinline__ double bscan(double v, double* red, double& total) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    if constexpr (NT > 64) {
        const int w = threadIdx.x >> 6;
        __syncthreads();
        if (lane == 63) red[w] = v;
        __syncthreads();
        double pre = 0.0, tot = 0.0;
#pragma unroll
        for (int i = 0; i < NT / 64; i++) {
            const double r = red[i];
            if (i < w) pre += r;
            tot += r;
        }
        total = tot;
        return v + pre;
    } else {
        total = __shfl(v, 63, 64);
        return v;
    }
}

// a - b = s + e exactly (Knuth TwoSum; -ffp-contract=off keeps it as written)
__device__ __forceinline__ double two_diff(double a, double b, double& e) {
    const double s = a - b;
    const double bb = s - a;
    e = (a - (s - bb)) - (b + bb);
    return s;
}

// x - (t0 + t1 u + t2 f2), rounded once at the size of the result
__device__ __forceinline__ double detr(double x, double t0, double t1, double t2, double u, double f2) {
    double e0, e1, e2;
    double s = two_diff(x, t0, e0);
    const double p1 = t1 * u, q1 = fma(t1, u, -p1);
    s = two_diff(s, p1, e1);
    const double p2 = t2 * f2, q2 = fma(t2, f2, -p2);
    s = two_diff(s, p2, e2);
    return s + (((e0 + e1) + e2) - (q1 + q2));
}

// ---- Durbin-Watson (:241-252): sum (e_i - e_{i-1})^2 / sum e_i^2, one sweep ----
template <int NT>
__global__ __launch_bounds__(NT) void dw_kernel(StatArgs a) {
    __shared__ double red[4];
    const int64_t s = blockIdx.x;
    const double* __restrict__ g = a.in + s * a.ld;
    const int64_t T = a.T;
    double num = 0.0, den = 0.0;
    for (int64_t t = threadIdx.x; t < T; t += NT) {
        const double x = g[t];
        den += x * x;
        if (t > 0) {
            const double d = x - g[t - 1];
            num += d * d;
        }
    }
    num = bsum<NT>(num, red);
    den = bsum<NT>(den, red);
    if (threadIdx.x == 0) a.stat[s] = num / den;
}

// ---- KPSS (:359-421) ----
template <int NT, bool LDS>
__global__ __launch_bounds__(NT) void kpss_kernel(StatArgs a) {
    extern __shared__ double dyn[];
    __shared__ double red[4];
    const int64_t s = blockIdx.x;
    const double* __restrict__ g = a.in + s * a.ld;
    const int64_t T = a.T;
    const int tid = threadIdx.x;
    const bool ct = a.q == 2;
    if constexpr (LDS) {
        for (int64_t t = tid; t < T; t += NT) dyn[t] = g[t];
        __syncthreads();
    }
    auto X = [&](int64_t t) -> double {
        if constexpr (LDS) return dyn[t];
        else return g[t];
    };
    const double n = (double)T, mid = 0.5 * (n - 1.0), N1 = n * (n * n - 1.0) / 12.0;
    // sweep 1: (a0, b0) of x = a + b u, u = t - mid (the span of 1 and t = 1..T), sums taken on
    // x - x[0] so that the level does not eat the slope's digits
    const double x0 = X(0);
    double s0 = 0.0, s1 = 0.0;
    for (int64_t t = tid; t < T; t += NT) {
        const double d = X(t) - x0, u = (double)t - mid;
        s0 += d;
        s1 += u * d;
    }
    s0 = bsum<NT>(s0, red);
    const double a0 = x0 + s0 / n;
    double b0 = 0.0;
    if (ct) b0 = bsum<NT>(s1, red) / N1;
    // refinement: what is left of (1, u) in the residuals
    double r0 = 0.0, r1 = 0.0;
    for (int64_t t = tid; t < T; t += NT) {
        const double u = (double)t - mid, e = detr(X(t), a0, b0, 0.0, u, 0.0);
        r0 += e;
        r1 += u * e;
    }
    const double da = bsum<NT>(r0, red) / n;
    double db = 0.0;
    if (ct) db = bsum<NT>(r1, red) / N1;
    auto resid = [&](int64_t t) -> double {
        const double u = (double)t - mid;
        return (detr(X(t), a0, b0, 0.0, u, 0.0) - da) - db * u;
    };
    if constexpr (LDS) {   // residuals replace the series (each thread rewrites its own steps)
        for (int64_t t = tid; t < T; t += NT) dyn[t] = resid(t);
        __syncthreads();
    }
    auto E = [&](int64_t t) -> double {
        if constexpr (LDS) return dyn[t];
        else return resid(t);
    };
    // sweep 2: sum of squared running sums, tile by tile with a carry
    double carry = 0.0, acc = 0.0;
    for (int64_t base = 0; base < T; base += NT) {
        const int64_t t = base + tid;
        double tot;
        const double c = bscan<NT>(t < T ? E(t) : 0.0, red, tot) + carry;
        if (t < T) acc += c * c;
        carry += tot;
    }
    const double s2 = bsum<NT>(acc, red);
    // Newey-West (:395-421): lag products 0..L, Bartlett weights
    double c0 = 0.0;
    for (int64_t t = tid; t < T; t += NT) {
        const double e = E(t);
        c0 += e * e;
    }
    c0 = bsum<NT>(c0, red);
    const int L = a.L;
    double terms = 0.0;
    for (int i = 1; i <= L; i++) {
        double ci = 0.0;
        for (int64_t t = (int64_t)i + tid; t < T; t += NT) ci += E(t) * E(t - i);
        ci = bsum<NT>(ci, red);
        terms += ci * (1.0 - (double)i / (double)(L + 1));
    }
    const double lrv = (terms * 2.0) / n + c0 / n;
    if (tid == 0) a.stat[s] = (s2 / lrv) / (n * n);
}

// Cholesky of the lag block G[0..nl)[0..nl) of a Gram matrix, one thread per row; rows nl..m, the
// right-hand sides, become L^-1 X_lags' of them.  The diagonal goes to dg unless it is null.  True
// (uniform) at an exactly zero or negative pivot, the reference's SingularMatrixException; NaN
// pivots pass (NaN in, NaN out, status 0).
__device__ __forceinline__ bool lag_cholesky(double (*G)[kMaxCols + 1], int nl, int m, double* dg) {
    const int tid = threadIdx.x;
    for (int j = 0; j < nl; j++) {
        double d2 = G[j][j];
        for (int c = 0; c < j; c++) d2 -= G[j][c] * G[j][c];
        if (d2 <= 0.0) return true;
        const double d = sqrt(d2);
        if (tid > j && tid < m) {
            double v = G[tid][j];
            for (int c = 0; c < j; c++) v -= G[tid][c] * G[j][c];
            G[tid][j] = v / d;
        }
        if (dg && tid == 0) dg[j] = d;
        __syncthreads();
    }
    return false;
}

// ---- ADF (:204-232), Frisch-Waugh two-pass ----
// Rows i = 0..n-1 (n = T - 1 - p), d[t] = y[t+1] - y[t]:
//   level    y[p + i]            (the reference's column 0)
//   lag j    d[p + i - j]        j = 1..p (lagMatTrimBoth(diff, p, true) columns 1..p)
//   response d[p + i]
// each detrended against the q trend columns (1, r, r^2 -> the orthogonal 1, u, u^2 - m2).
// Then Frisch-Waugh once more, on the lags: Cholesky of the lags' Gram matrix alone gives the
// regressions of the level and of the response on the lags; their residuals e and f are formed
// explicitly row by row, and beta_0 = e'f / e'e, RSS = sum (f - beta_0 e)^2, [(X'X)^-1]_00 = 1 / e'e.
// An error in the lag regressions enters e'e, e'f and RSS only squared (e and f stay orthogonal to
// the lags to first order), so the statistic does not see the square of the design's condition
// number -- which a Cholesky factor of the whole Gram matrix does at nObs - k = 1.
template <int NT, bool LDS>
__global__ __launch_bounds__(NT) void adf_kernel(StatArgs a) {
    extern __shared__ double dyn[];
    __shared__ double red[4];
    __shared__ double rho[kMaxCols][3];
    __shared__ double G[kMaxCols][kMaxCols + 1];
    __shared__ double dg[kMaxCols], gam[2][kMaxCols];
    const int64_t s = blockIdx.x;
    const double* __restrict__ g = a.in + s * a.ld;
    const int64_t T = a.T;
    const int tid = threadIdx.x, p = a.p, q = a.q;
    const int64_t nr = T - 1 - p;
    double* A = dyn;        // LDS form: y[0..T), later the detrended differences [0..T-1)
    double* B = dyn + T;    // LDS form: the detrended level column [0..nr)
    if constexpr (LDS) {
        for (int64_t t = tid; t < T; t += NT) A[t] = g[t];
        __syncthreads();
    }
    auto Y = [&](int64_t t) -> double {
        if constexpr (LDS) return A[t];
        else return g[t];
    };
    const double n = (double)nr, mid = 0.5 * (n - 1.0), m2 = (n * n - 1.0) / 12.0;
    const double N1 = n * (n * n - 1.0) / 12.0, N2 = n * (n * n - 1.0) * (n * n - 4.0) / 180.0;
    // level column: its trend coefficients (sums on y - y[p]), then the detrended values
    double th0 = 0.0, th1 = 0.0, th2 = 0.0;
    if (q >= 1) {
        const double y0 = Y(p);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int64_t i = tid; i < nr; i += NT) {
            const double d = Y(p + i) - y0, u = (double)i - mid;
            s0 += d;
            s1 += u * d;
            s2 += (u * u - m2) * d;
        }
        th0 = y0 + bsum<NT>(s0, red) / n;
        if (q >= 2) th1 = bsum<NT>(s1, red) / N1;
        if (q >= 3) th2 = bsum<NT>(s2, red) / N2;
    }
    auto lev_raw = [&](int64_t i) -> double {
        const double u = (double)i - mid;
        return detr(Y(p + i), th0, th1, th2, u, u * u - m2);
    };
    // differences: one trend fitted on the response window and removed from every d[t]; each
    // column's own (small) remainder rho is projected out below
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    if (q >= 1) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int64_t i = tid; i < nr; i += NT) {
            const double d = Y(p + i + 1) - Y(p + i), u = (double)i - mid;
            s0 += d;
            s1 += u * d;
            s2 += (u * u - m2) * d;
        }
        g0 = bsum<NT>(s0, red) / n;
        if (q >= 2) g1 = bsum<NT>(s1, red) / N1;
        if (q >= 3) g2 = bsum<NT>(s2, red) / N2;
    }
    auto dl_raw = [&](int64_t t) -> double {
        const double u = (double)(t - p) - mid;
        return detr(Y(t + 1) - Y(t), g0, g1, g2, u, u * u - m2);
    };
    if constexpr (LDS) {
        for (int64_t i = tid; i < nr; i += NT) B[i] = lev_raw(i);
        // in place, tile by tile: a tile reads y[base .. base + NT] before it writes [base, base + NT)
        for (int64_t base = 0; base < T - 1; base += NT) {
            const int64_t t = base + tid;
            const double v = t < T - 1 ? dl_raw(t) : 0.0;
            __syncthreads();
            if (t < T - 1) A[t] = v;
            __syncthreads();
        }
    }
    auto LEV = [&](int64_t i) -> double {
        if constexpr (LDS) return B[i];
        else return lev_raw(i);
    };
    auto DL = [&](int64_t t) -> double {
        if constexpr (LDS) return A[t];
        else return dl_raw(t);
    };
    // rho[j]: what window j (rows of d shifted back by j; j = 0 is the response) still holds of the trend
    for (int j = 0; j <= p; j++) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        if (q >= 1)
            for (int64_t i = tid; i < nr; i += NT) {
                const double d = DL(p + i - j), u = (double)i - mid;
                s0 += d;
                s1 += u * d;
                s2 += (u * u - m2) * d;
            }
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;
        if (q >= 1) r0 = bsum<NT>(s0, red) / n;
        if (q >= 2) r1 = bsum<NT>(s1, red) / N1;
        if (q >= 3) r2 = bsum<NT>(s2, red) / N2;
        if (tid == 0) {
            rho[j][0] = r0;
            rho[j][1] = r1;
            rho[j][2] = r2;
        }
    }
    __syncthreads();
    // Gram matrix of the detrended lag columns (c < p is lag c + 1) with the level (c == p) and the
    // response (c == p + 1) as right-hand sides
    const int m = p + 2;
    auto shift_of = [&](int c) -> int { return c < p ? c + 1 : 0; };
    auto COL = [&](int c, int js, int64_t i, double u, double f2) -> double {
        return c == p ? LEV(i) : DL(p + i - js) - (rho[js][0] + rho[js][1] * u + rho[js][2] * f2);
    };
    for (int ca = 0; ca < p; ca++) {
        const int ja = shift_of(ca);
        for (int cb = ca; cb < m; cb++) {
            const int jb = shift_of(cb);
            double acc = 0.0;
            for (int64_t i = tid; i < nr; i += NT) {
                const double u = (double)i - mid, f2 = u * u - m2;
                acc += COL(ca, ja, i, u, f2) * COL(cb, jb, i, u, f2);
            }
            acc = bsum<NT>(acc, red);
            if (tid == 0) {
                G[ca][cb] = acc;
                G[cb][ca] = acc;
            }
        }
    }
    __syncthreads();
    // rows p and p + 1 become L^-1 X_lags' (level, response)
    bool singular = lag_cholesky(G, p, m, dg);
    // back substitution: gam[w] = the lag coefficients of the level (w = 0) and the response (w = 1)
    if (!singular && tid < 2) {
        for (int c = p - 1; c >= 0; c--) {
            double v = G[p + tid][c];
            for (int k = c + 1; k < p; k++) v -= G[k][c] * gam[tid][k];
            gam[tid][c] = v / dg[c];
        }
    }
    __syncthreads();
    auto EF = [&](int64_t i, double& e, double& f) {
        const double u = (double)i - mid, f2 = u * u - m2;
        e = LEV(i);
        f = COL(p + 1, 0, i, u, f2);
        for (int c = 0; c < p; c++) {
            const double v = COL(c, c + 1, i, u, f2);
            e -= gam[0][c] * v;
            f -= gam[1][c] * v;
        }
    };
    double see = 0.0, sef = 0.0, rss = 0.0;
    if (!singular) {
        for (int64_t i = tid; i < nr; i += NT) {
            double e, f;
            EF(i, e, f);
            see += e * e;
            sef += e * f;
        }
        see = bsum<NT>(see, red);
        sef = bsum<NT>(sef, red);
        if (see <= 0.0) singular = true;   // the level column itself is in the span of the others
    }
    if (!singular) {
        const double beta = sef / see;
        for (int64_t i = tid; i < nr; i += NT) {
            double e, f;
            EF(i, e, f);
            const double r = f - beta * e;
            rss += r * r;
        }
        rss = bsum<NT>(rss, red);
        const double dof = n - (double)(1 + p + q);
        if (tid == 0) a.stat[s] = beta / sqrt(rss / dof / see);
    } else if (tid == 0) {
        a.stat[s] = NAN;
        if (a.err) a.err[s] = STS_ERR_SINGULAR;
    }
}

// ---- p-values ----

// MacKinnon (1994), table for N = 1 (one I(1) series): per regression tau*, tau_min, tau_max, the
// small-p quadratic and the large-p cubic in tau, constant term first.
struct MacKinnon {
    double star, lo, hi, small[3], large[4];
};
__constant__ MacKinnon kMacKinnon[4] = {
    /* nc  */ {-1.04, -19.04, INFINITY, {0.6344, 1.2378, 3.2496e-2}, {0.4797, 9.3557e-1, -0.6999e-1, 3.3066e-2}},
    /* c   */ {-1.61, -18.83, 2.74, {2.1659, 1.4412, 3.8269e-2}, {1.7339, 9.3202e-1, -1.2745e-1, -1.0368e-2}},
    /* ct  */ {-2.89, -16.18, 0.7, {3.2512, 1.6047, 4.9588e-2}, {2.5261, 6.1654e-1, -3.7956e-1, -6.0285e-2}},
    /* ctt */ {-3.21, -17.17, 0.54, {4.0003, 1.658, 4.8288e-2}, {3.0778, 4.9529e-1, -4.1477e-1, -5.9359e-2}},
};

__global__ void adf_pvalue_kernel(const double* __restrict__ stat, double* __restrict__ pv, int64_t S, int reg) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const MacKinnon& mk = kMacKinnon[reg];
    const double tau = stat[s];
    double r;
    if (tau > mk.hi) r = 1.0;
    else if (tau < mk.lo) r = 0.0;
    else {
        double z;
        if (tau <= mk.star) z = (mk.small[2] * tau + mk.small[1]) * tau + mk.small[0];
        else z = ((mk.large[3] * tau + mk.large[2]) * tau + mk.large[1]) * tau + mk.large[0];
        r = 0.5 * erfc(-z / 1.4142135623730951);
    }
    pv[s] = r;
}

// regularised lower incomplete gamma P(a, x): the series below a + 1, a continued fraction for
// the upper tail above (modified Lentz), both cut at 1e-15 relative
__device__ double gamma_p(double a, double x) {
    if (x != x) return x;
    if (x <= 0.0) return 0.0;
    if (isinf(x)) return 1.0;
    const double lead = exp(-x + a * log(x) - lgamma(a));
    if (x < a + 1.0) {
        double ap = a, term = 1.0 / a, sum = term;
        for (int it = 0; it < 100000; it++) {
            ap += 1.0;
            term *= x / ap;
            sum += term;
            if (fabs(term) < fabs(sum) * 1e-15) break;
        }
        return sum * lead;
    }
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int it = 1; it < 100000; it++) {
        const double an = -(double)it * ((double)it - a);
        b += 2.0;
        d = an * d + b;
        if (fabs(d) < tiny) d = tiny;
        c = b + an / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1e-15) break;
    }
    return 1.0 - lead * h;
}

// Ljung-Box epilogue (:289-298), one lane per series
__global__ void lb_kernel(const double* __restrict__ acf, int64_t S, int64_t T, int K, double* __restrict__ stat,
                          double* __restrict__ pv) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double* r = acf + s * (int64_t)K;
    double sum = 0.0;
    for (int k = 0; k < K; k++) sum += (r[k] * r[k]) / (double)(T - k - 1);
    const double q = (double)T * (double)(T + 2) * sum;
    stat[s] = q;
    if (pv) pv[s] = 1.0 - gamma_p(0.5 * (double)K, 0.5 * q);
}

// ---- Breusch-Pagan (:311-319) and Breusch-Godfrey (:266-278): n R^2 of an OLS with intercept ----
// The regressors are 1, the k factors (rows lo..lo+n of each factor row; lo = maxLag for BG, 0 for
// BP) and, for BG, the lags e[t-1]..e[t-L] of the response e[L..T).  R^2 is formed as the
// explained sum of squares over the centred total, a sum of non-negative terms:
//   ESS = sum_c (q_c . y)^2 + |Lz^-1 Z'z_0|^2,     R^2 = ESS / (y . y)
// with y the centred response, q_1..q_k an orthonormal basis of the centred factors
// (factor_basis_kernel), z_j the lag-j window with its mean and its q components taken out, z_0
// the response treated alike and Lz the Cholesky factor of the lags' Gram matrix Z'Z alone (as
// adf_kernel).  No term is a difference of large numbers, so R^2 keeps its relative accuracy
// where 1 - RSS / TSS and a pivot of the whole Gram matrix lose theirs.

// The basis of a stat kernel's series: OWN builds it from the series' own factors into LDS behind
// the series (per-series factors that fit, one-wave form); otherwise it is in the scratch.  False
// when the factors are rank deficient (the statistic is then NaN, the status STS_ERR_SINGULAR).
template <int NT, bool OWN>
__device__ __forceinline__ bool series_basis(const BgBpArgs& a, int64_t s, int64_t b, double* lds, double* red,
                                             const double*& Q) {
    bool singular;
    if constexpr (OWN) {
        singular = build_basis<NT, false>(a.f.factors + s * a.f.fs + a.f.lo, a.f.ld_f, a.f.k, a.f.n, lds, nullptr, red);
        Q = lds;
    } else {
        singular = a.f.info[b * a.f.info_stride] != 0;
        Q = a.f.basis + b * a.f.basis_stride;
    }
    if (singular && threadIdx.x == 0) {
        a.stat[s] = NAN;
        if (a.err) a.err[s] = STS_ERR_SINGULAR;
    }
    return !singular;
}

// Breusch-Godfrey, one workgroup per series.  Window j (j = 0 the response, j = 1..L lag j) is rows
// W(j, i) = e[L + i - j], i < n = T - L.
template <int NT, bool LDS, bool OWN>
__global__ __launch_bounds__(NT) void bg_kernel(BgBpArgs a, int64_t s0) {
    extern __shared__ double dyn[];
    __shared__ double red[8 * 4];
    __shared__ double P[kMaxCols][kMaxFactors];   // P[j][c] = q_c . (centred window j)
    __shared__ double mu[kMaxCols];
    __shared__ double G[kMaxCols][kMaxCols + 1];
    const int64_t b = blockIdx.x, s = s0 + b;
    const double* __restrict__ g = a.in + s * a.ld;
    const int64_t T = a.T, n = a.f.n;
    const int tid = threadIdx.x, L = a.L, k = a.f.k;
    const double dn = (double)n;
    const double* Q;
    if (!series_basis<NT, OWN>(a, s, b, dyn + T, red, Q)) return;   // uniform
    if constexpr (LDS) {
        for (int64_t t = tid; t < T; t += NT) dyn[t] = g[t];
        __syncthreads();
    }
    auto X = [&](int64_t t) -> double {
        if constexpr (LDS) return dyn[t];
        else return g[t];
    };
    // window means, sums taken on x - x0
    const double x0 = X(L);
    for (int j = 0; j <= L; j++) {
        double acc = 0.0;
        for (int64_t i = tid; i < n; i += NT) acc += X(L + i - j) - x0;
        acc = bsum<NT>(acc, red) / dn;
        if (tid == 0) mu[j] = acc;
    }
    __syncthreads();
    auto CEN = [&](int j, int64_t i) -> double { return (X(L + i - j) - x0) - mu[j]; };
    // the centred total, and the factor components of every window
    double tss = 0.0;
    for (int64_t i = tid; i < n; i += NT) {
        const double v = CEN(0, i);
        tss += v * v;
    }
    tss = bsum<NT>(tss, red);
    if (tss == 0.0) {   // a bit-constant response: the reference's 0 / 0
        if (tid == 0) a.stat[s] = NAN;
        return;
    }
    for (int j = 0; j <= L; j++) {
        double acc[kMaxFactors];
#pragma unroll
        for (int c = 0; c < kMaxFactors; c++) acc[c] = 0.0;
        for (int64_t i = tid; i < n; i += NT) {
            const double v = CEN(j, i);
#pragma unroll
            for (int c = 0; c < kMaxFactors; c++)
                if (c < k) acc[c] += Q[(int64_t)c * n + i] * v;
        }
        bsum_many<NT>(acc, k, red);
        if (tid == 0) {
#pragma unroll
            for (int c = 0; c < kMaxFactors; c++)
                if (c < k) P[j][c] = acc[c];
        }
    }
    __syncthreads();
    double ess = 0.0;
    for (int c = 0; c < k; c++) ess += P[0][c] * P[0][c];
    bool singular = false;
    if (L > 0) {
        // Gram matrix of the residualised lags (index j - 1) with the residualised response as
        // row / column L, eight columns to a sweep
        auto col_of = [&](int c) -> int { return c < L ? c + 1 : 0; };
        for (int ca = 0; ca < L; ca++) {
            const int ja = col_of(ca);
            for (int cb0 = ca; cb0 <= L; cb0 += 8) {
                double acc[8];
#pragma unroll
                for (int u = 0; u < 8; u++) acc[u] = 0.0;
                for (int64_t i = tid; i < n; i += NT) {
                    double qv[kMaxFactors];
#pragma unroll
                    for (int c = 0; c < kMaxFactors; c++) qv[c] = c < k ? Q[(int64_t)c * n + i] : 0.0;
                    double za = CEN(ja, i);
#pragma unroll
                    for (int c = 0; c < kMaxFactors; c++)
                        if (c < k) za -= P[ja][c] * qv[c];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const int cb = cb0 + u;
                        if (cb <= L) {
                            const int jb = col_of(cb);
                            double zb = CEN(jb, i);
#pragma unroll
                            for (int c = 0; c < kMaxFactors; c++)
                                if (c < k) zb -= P[jb][c] * qv[c];
                            acc[u] += za * zb;
                        }
                    }
                }
                bsum_many<NT>(acc, L + 1 - cb0, red);
                if (tid == 0) {
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const int cb = cb0 + u;
                        if (cb <= L) {
                            G[ca][cb] = acc[u];
                            G[cb][ca] = acc[u];
                        }
                    }
                }
            }
        }
        __syncthreads();
        singular = lag_cholesky(G, L, L + 1, nullptr);   // row L becomes Lz^-1 Z'z_0
        if (!singular)
            for (int j = 0; j < L; j++) ess += G[L][j] * G[L][j];
    }
    if (tid == 0) {
        if (singular) {
            a.stat[s] = NAN;
            if (a.err) a.err[s] = STS_ERR_SINGULAR;
        } else {
            a.stat[s] = dn * (ess / tss);
        }
    }
}

// Breusch-Pagan alone: no lags, so no Gram matrix and no LDS beyond the series.  With shared
// factors this is the one-read kernel: the series comes from HBM once (into LDS in the one-wave
// form), the k basis rows come from the caches, and k + 1 dot products and a sum of squares remain.
template <int NT, bool LDS, bool OWN>
__global__ __launch_bounds__(NT) void bp_kernel(BgBpArgs a, int64_t s0) {
    extern __shared__ double dyn[];
    __shared__ double red[(kMaxFactors + 1) * 4];
    const int64_t b = blockIdx.x, s = s0 + b;
    const double* __restrict__ g = a.in + s * a.ld;
    const int64_t T = a.T;
    const int tid = threadIdx.x, k = a.f.k;
    const double dn = (double)T;
    const double* Q;
    if (!series_basis<NT, OWN>(a, s, b, dyn + T, red, Q)) return;   // uniform
    // sweep 1: the mean of e^2, sums taken on e^2 - e[0]^2
    const double e0 = g[0], x0 = e0 * e0;
    double m = 0.0;
    for (int64_t t = tid; t < T; t += NT) {
        const double e = g[t], d = e * e - x0;
        if constexpr (LDS) dyn[t] = d;
        m += d;
    }
    m = bsum<NT>(m, red) / dn;
    auto D = [&](int64_t t) -> double {
        if constexpr (LDS) return dyn[t];   // each thread reads back its own steps
        else {
            const double e = g[t];
            return e * e - x0;
        }
    };
    // sweep 2: the centred total and the factor components
    double acc[kMaxFactors + 1];
#pragma unroll
    for (int c = 0; c <= kMaxFactors; c++) acc[c] = 0.0;
    for (int64_t t = tid; t < T; t += NT) {
        const double v = D(t) - m;
        acc[0] += v * v;
#pragma unroll
        for (int c = 0; c < kMaxFactors; c++)
            if (c < k) acc[1 + c] += Q[(int64_t)c * T + t] * v;
    }
    bsum_many<NT>(acc, k + 1, red);
    if (tid == 0) {
        const double tss = acc[0];
        double ess = 0.0;
#pragma unroll
        for (int c = 0; c < kMaxFactors; c++)
            if (c < k) ess += acc[1 + c] * acc[1 + c];
        a.stat[s] = tss == 0.0 ? NAN : dn * (ess / tss);   // a bit-constant response: the reference's 0 / 0
    }
}

// 1 - chi2cdf(stat, dof), one lane per series (commons-math3 ChiSquaredDistribution, as lb_kernel)
__global__ void chi2_pvalue_kernel(const double* __restrict__ stat, double* __restrict__ pv, int64_t S, int dof) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    pv[s] = 1.0 - gamma_p(0.5 * (double)dof, 0.5 * stat[s]);
}

}  // namespace

hipError_t launch_factor_basis(const FactorBasisArgs& f, int64_t s0, int64_t nb, hipStream_t st) {
    const dim3 grid((unsigned)nb), block(kLongThreads);
    if (f.aux) hipLaunchKernelGGL((factor_basis_kernel<kLongThreads, true>), grid, block, 0, st, f, s0);
    else hipLaunchKernelGGL((factor_basis_kernel<kLongThreads, false>), grid, block, 0, st, f, s0);
    return hipGetLastError();
}

hipError_t launch_bgbp(const BgBpArgs& a, int64_t s0, int64_t ns, hipStream_t st) {
    const dim3 grid((unsigned)ns);
    const size_t series = (size_t)a.T * sizeof(double), own = (size_t)(a.T + a.f.k * a.f.n) * sizeof(double);
    if (a.squares) {
        if (own_basis(a)) hipLaunchKernelGGL((bp_kernel<64, true, true>), grid, dim3(64), own, st, a, s0);
        else if (a.T <= kStatOneWave) hipLaunchKernelGGL((bp_kernel<64, true, false>), grid, dim3(64), series, st, a, s0);
        else hipLaunchKernelGGL((bp_kernel<kLongThreads, false, false>), grid, dim3(kLongThreads), 0, st, a, s0);
    } else {
        if (own_basis(a)) hipLaunchKernelGGL((bg_kernel<64, true, true>), grid, dim3(64), own, st, a, s0);
        else if (a.T <= kStatOneWave) hipLaunchKernelGGL((bg_kernel<64, true, false>), grid, dim3(64), series, st, a, s0);
        else hipLaunchKernelGGL((bg_kernel<kLongThreads, false, false>), grid, dim3(kLongThreads), 0, st, a, s0);
    }
    return hipGetLastError();
}

hipError_t launch_chi2_pvalue(const double* stat, double* pv, int64_t S, int dof, hipStream_t st) {
    hipLaunchKernelGGL(chi2_pvalue_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, stat, pv, S, dof);
    return hipGetLastError();
}

hipError_t launch_dw(const StatArgs& a, hipStream_t st) {
    if (a.T <= kStatOneWave) hipLaunchKernelGGL(dw_kernel<64>, dim3((unsigned)a.S), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(dw_kernel<kLongThreads>, dim3((unsigned)a.S), dim3(kLongThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_kpss(const StatArgs& a, hipStream_t st) {
    if (a.T <= kStatOneWave)
        hipLaunchKernelGGL((kpss_kernel<64, true>), dim3((unsigned)a.S), dim3(64), (size_t)a.T * sizeof(double), st, a);
    else
        hipLaunchKernelGGL((kpss_kernel<kLongThreads, false>), dim3((unsigned)a.S), dim3(kLongThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_adf(const StatArgs& a, hipStream_t st) {
    if (a.T <= kStatOneWave)
        hipLaunchKernelGGL((adf_kernel<64, true>), dim3((unsigned)a.S), dim3(64),
                           (size_t)(2 * a.T) * sizeof(double), st, a);
    else
        hipLaunchKernelGGL((adf_kernel<kLongThreads, false>), dim3((unsigned)a.S), dim3(kLongThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_adf_pvalue(const double* stat, double* pv, int64_t S, int regression, hipStream_t st) {
    hipLaunchKernelGGL(adf_pvalue_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, stat, pv, S, regression);
    return hipGetLastError();
}

hipError_t launch_lb(const double* acf, int64_t S, int64_t T, int K, double* stat, double* pv, hipStream_t st) {
    hipLaunchKernelGGL(lb_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, acf, S, T, K, stat, pv);
    return hipGetLastError();
}

}  // namespace sts
