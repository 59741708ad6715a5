// sts_arima.hip -- ARIMA(p, d, q) with MA terms batched over a panel: the "css-cgd" fit, the
// CSS likelihood and gradient, the Hannan-Rissanen start, remove / add and forecast.
//
// Reference (S/ = src/main/scala/com/cloudera/sparkts/):
//   ARIMA.fitWithCSSCGD                      S/models/ARIMA.scala:166-192
//   ARIMA.HannanRissanenInit                 S/models/ARIMA.scala:207-233
//   ARIMAModel.logLikelihoodCSSARMA          S/models/ARIMA.scala:278-293
//   ARIMAModel.gradientlogLikelihoodCSSARMA  S/models/ARIMA.scala:312-381
//   ARIMAModel.iterateARMA / updateMAErrors  S/models/ARIMA.scala:390-463
//   ARIMAModel.remove / add                  S/models/ARIMA.scala:474-510
//   ARIMAModel.forecast                      S/models/ARIMA.scala:537-605
//
// Every kernel here works on ARMA level; the C-ABI layer differences the panel with the
// diff_kernel ping-pong of sts_arima_fit_ar and re-integrates with kArimaIntegrate launches.
//
// Fit / evaluation (arima_css_kernel): the shape of garch_fit_kernel.  One LANE per series runs
// commons-math3's optimizer as a resumable state machine (sts_arima_opt.hpp); a wave owns 64
// series and, each round, streams its block of rows through LDS once in kArimaChunk-step
// chunks while every lane with a pending request evaluates the likelihood -- and the gradient
// when the request wants it -- of its own series at its own point in one sequential pass
// (sts_arima_eval.hpp: the reference's operation order, -ffp-contract=off, fdlibm's log), so
// every evaluation is bit-exact and the optimizer takes the reference's path.
// Per-lane arrays: the point, direction, request, gradient, MA terms and AR history are
// indexed by constants in unrolled, guarded loops (registers); the q previous rows of
// dEdTheta are a ring in LDS, one column of 36 doubles per lane, because its head moves.
// There is no tail kernel for long-running series: a wave lasts as long as its slowest lane.
//
// Effects and forecast: the same LDS-staged row blocks, one lane per series running the
// recurrence in order and writing its row back through LDS.
#include "sts_arima_eval.hpp"
#include "sts_internal.hpp"
#include "sts_lane_rows.hpp"

#include <hip/hip_runtime.h>

namespace sts {
namespace {

constexpr int kSpw = 64;           // series per wave
constexpr int kCh = kArimaChunk;   // steps per LDS chunk
constexpr int kESpw = 32;          // series per wave of the effects / forecast kernels (half the prefetch registers)
constexpr int kRow = kCh + 1;      // arima_forecast_kernel's own copy of the loop
constexpr int kENld = kESpw * kCh / 64;

template <bool FIT>
__global__ __launch_bounds__(64) void arima_css_kernel(ArimaCssArgs a) {
    __shared__ double tile[LaneRows<kSpw, kCh>::kTile];
    __shared__ double ring[kArimaQ * kArimaDim * 64];
    const LaneBlock<kSpw> b(a.S);
    const int lane = b.lane;
    const int64_t sl = b.sl;
    const bool live = b.live;
    const int N = a.n_len;
    const int n = a.icpt + a.p + a.q;

    ArimaOpt o;
    o.n = n;
#pragma unroll
    for (int j = 0; j < kArimaDim; j++) {
        o.point[j] = (live && j < n) ? a.coef_in[sl * n + j] : 0.0;
        o.req[j] = o.point[j];
        o.dir[j] = 0.0;
    }
    arima_init(o);
    if (FIT) {
        if (live) arima_advance(o);
    } else {
        o.need_grad = a.grad != nullptr;
    }
    for (;;) {
        const bool pending = live && o.status < 0;
        const unsigned long long want = __ballot(pending);
        if (want == 0) break;
        ArimaEval g;
        g.start(o.req, a.p, a.q, a.icpt, N, pending && o.need_grad != 0, ring + lane, 64);
        stream_rows<kSpw, kCh>(tile, a.in + b.s0 * a.ld, a.ld, N, b.ns, want, pending,
                               [&](const double* myrow, int64_t tc, int len) { g.run(myrow, 0, len, tc); });
        if (pending) {
            o.res_f = g.loglik();
            if (o.need_grad) g.gradient(o.res_g);
            if (!FIT) {
                o.status = STS_OK;
            } else {
                arima_cache_insert(o);
                arima_advance(o);
            }
        }
    }
    if (!live) return;
    if (FIT) {
        const bool ok = o.status == STS_OK;
#pragma unroll
        for (int j = 0; j < kArimaDim; j++)
            if (j < n) a.coef_out[sl * n + j] = ok ? o.point[j] : __builtin_nan("");
        if (a.err) a.err[sl] = o.status;
        if (a.evals) a.evals[sl] = o.evals;
    } else {
        if (a.loglik) a.loglik[sl] = o.res_f;
        if (a.grad) {
#pragma unroll
            for (int j = 0; j < kArimaDim; j++)
                if (j < n) a.grad[sl * n + j] = o.res_g[j];
        }
    }
}

// per-series model in registers: intercept amount, AR and MA coefficients
struct ArimaCoef {
    double coef0, amt, phi[kArimaQ], theta[kArimaQ];
    __device__ __forceinline__ void load(const double* coef, int64_t s, int p, int q, int icpt, bool live) {
        const int n = icpt + p + q;
        const double* cs = coef + s * n;
        coef0 = live ? cs[0] : 0.0;
        amt = icpt ? coef0 : 0.0;
#pragma unroll
        for (int j = 0; j < kArimaQ; j++) {
            phi[j] = (live && j < p) ? cs[icpt + j] : 0.0;
            theta[j] = (live && j < q) ? cs[icpt + p + j] : 0.0;
        }
    }
};

// updateMAErrors over an array of `len` entries (:390-400): ascending copy, newest in front
__device__ __forceinline__ void update_ma(double (&ma)[kArimaQ], int len, double error) {
#pragma unroll
    for (int i = 0; i < kArimaQ - 1; i++)
        if (i < len - 1) ma[i + 1] = ma[i];
    if (len > 0) ma[0] = error;
}

__device__ __forceinline__ void push(double (&h)[kArimaQ], double v) {
#pragma unroll
    for (int j = kArimaQ - 1; j > 0; j--) h[j] = h[j - 1];
    h[0] = v;
}

// remove / add on the ARMA level, and one inverseDifferencesAtLag(x, x, 1, start) pass
template <int OP>
__global__ __launch_bounds__(64) void arima_effects_kernel(ArimaEffectsArgs a) {
    __shared__ double tile[LaneRows<kESpw, kCh>::kTile];
    const LaneBlock<kESpw> b(a.S);
    const bool live = b.live;
    const int p = a.p, q = a.q;
    ArimaCoef m;
    if (OP != kArimaIntegrate) m.load(a.coef, b.sl, p, q, a.icpt, live);
    // the maxLag assumed values before the series: the intercept amount (:480, :503)
    double hist[kArimaQ], ma[kArimaQ];
#pragma unroll
    for (int j = 0; j < kArimaQ; j++) {
        hist[j] = OP != kArimaIntegrate ? m.amt : 0.0;
        ma[j] = 0.0;
    }
    double prevY = 0.0;
    map_rows<kESpw, kCh>(tile, a.in, a.ld_in, a.out, a.ld_out, a.T, b.s0, b.ns, live,
                         [&](double* myrow, int64_t tc, int len) {
        for (int cc = 0; cc < len; cc++) {
            const double x = myrow[cc];
            double y;
            if (OP == kArimaIntegrate) {
                y = (tc + cc < a.start) ? x : x + prevY;
                prevY = y;
            } else if (OP == kArimaRemove) {
                // iterateARMA(diffedExtended, changes, _ - _, errors = changes)
                y = x - (double)a.icpt * m.coef0;
#pragma unroll
                for (int j = 0; j < kArimaQ; j++)
                    if (j < p) y = y - hist[j] * m.phi[j];
#pragma unroll
                for (int j = 0; j < kArimaQ; j++)
                    if (j < q) y = y - ma[j] * m.theta[j];
                update_ma(ma, q, y);
                push(hist, x);
            } else {
                // iterateARMA(changes, changes, _ + _, errors = errorsProvided)
                y = x + (double)a.icpt * m.coef0;
#pragma unroll
                for (int j = 0; j < kArimaQ; j++)
                    if (j < p) y = y + hist[j] * m.phi[j];
#pragma unroll
                for (int j = 0; j < kArimaQ; j++)
                    if (j < q) y = y + ma[j] * m.theta[j];
                update_ma(ma, q, x);
                push(hist, y);
            }
            myrow[cc] = y;
        }
    });
}

// forecast on the ARMA level (:538-569): out(t) = ts(t) for t < d, the fitted one-step value of
// the differenced series for d <= t < T, the forward curve for t >= T.  The chunk loop is map_rows
// (sts_lane_rows.hpp) written out, with T input and T + n_future output steps: over a shared loop
// with the two lengths the ARMA(1, 1) forecast ran 1.5 % slower (100 k x 250, 65 steps ahead).
__global__ __launch_bounds__(64) void arima_forecast_kernel(ArimaForecastArgs a) {
    __shared__ double tile[kESpw * kRow];
    const int lane = threadIdx.x;
    const int64_t s0 = (int64_t)blockIdx.x * kESpw;
    const int64_t sl = s0 + lane;
    const bool live = lane < kESpw && sl < a.S;
    const int ns = (a.S - s0 < kESpw) ? (int)(a.S - s0) : kESpw;
    const int64_t T = a.T, TO = a.T + a.n_future;
    const int p = a.p, q = a.q, d = a.d;
    const int maxLag = p > q ? p : q;
    ArimaCoef m;
    m.load(a.coef, sl, p, q, a.icpt, live);
    // ext = maxLag intercept amounts ++ diffed; hist = zeros, filled from index maxLag on
    double ext[kArimaQ], ma[kArimaQ], hh[kArimaQ], rr[kArimaQ];
#pragma unroll
    for (int j = 0; j < kArimaQ; j++) {
        ext[j] = m.amt;          // ext(i - 1 - j)
        ma[j] = 0.0;
        hh[j] = 0.0;             // hist(i - 1 - j)
        rr[j] = m.amt - 0.0;     // ext(i - 1 - j) - hist(i - 1 - j)
    }
    bool forward = false;
    double pre[kENld];
    auto fetch = [&](int64_t tc) {
#pragma unroll
        for (int i = 0; i < kENld; i++) {
            const int row = (i * 64 + lane) / kCh, col = (i * 64 + lane) % kCh;
            pre[i] = (row < ns && tc + col < T) ? a.diffed[(s0 + row) * a.ld_d + tc + col] : 0.0;
        }
    };
    fetch(0);
    for (int64_t tc = 0; tc < TO; tc += kCh) {
        const int len = (TO - tc < kCh) ? (int)(TO - tc) : kCh;
#pragma unroll
        for (int i = 0; i < kENld; i++) {
            const int row = (i * 64 + lane) / kCh, col = (i * 64 + lane) % kCh;
            tile[row * kRow + col] = pre[i];
        }
        if (tc + kCh < TO) fetch(tc + kCh);
        __syncthreads();
        if (live) {
            double* myrow = tile + lane * kRow;
            for (int cc = 0; cc < len; cc++) {
                const int64_t t = tc + cc;
                double y;
                if (t < d) {
                    y = a.ts[sl * a.ld_ts + t];
                } else if (t < T) {
                    // iterateARMA(diffedTsExtended, hist, _ + _, goldStandard = diffedTsExtended)
                    const double x = myrow[cc];
                    y = 0.0 + (double)a.icpt * m.coef0;
#pragma unroll
                    for (int j = 0; j < kArimaQ; j++)
                        if (j < p) y = y + ext[j] * m.phi[j];
#pragma unroll
                    for (int j = 0; j < kArimaQ; j++)
                        if (j < q) y = y + ma[j] * m.theta[j];
                    const double error = x - y;
                    update_ma(ma, q, error);
                    push(ext, x);
                    push(hh, y);
                    push(rr, error);
                } else {
                    if (!forward) {
                        forward = true;
                        // maTerms = ext - hist over the last maxLag indices, OLDEST first (:552-554);
                        // forward(0 until maxLag) = hist(-maxLag to -1): hh already is forward(i - 1 - j)
                        double fm[kArimaQ];
#pragma unroll
                        for (int i = 0; i < kArimaQ; i++) {
                            fm[i] = 0.0;
#pragma unroll
                            for (int k = 0; k < kArimaQ; k++)
                                if (k == maxLag - 1 - i) fm[i] = rr[k];
                        }
#pragma unroll
                        for (int i = 0; i < kArimaQ; i++) ma[i] = fm[i];
                    }
                    // iterateARMA(forward, forward, _ + _, goldStandard = forward, initMATerms = maTerms)
                    y = 0.0 + (double)a.icpt * m.coef0;
#pragma unroll
                    for (int j = 0; j < kArimaQ; j++)
                        if (j < p) y = y + hh[j] * m.phi[j];
#pragma unroll
                    for (int j = 0; j < kArimaQ; j++)
                        if (j < q) y = y + ma[j] * m.theta[j];
                    update_ma(ma, maxLag, y - y);   // the array has maxLag entries here
                    push(hh, y);
                }
                myrow[cc] = y;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kENld; i++) {
            const int row = (i * 64 + lane) / kCh, col = (i * 64 + lane) % kCh;
            if (row < ns && col < len) a.out[(s0 + row) * a.ld_out + tc + col] = tile[row * kRow + col];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void arima_level_sum_kernel(const double* __restrict__ level, int64_t ld,
                                                              double* __restrict__ sum, int64_t S, int64_t T,
                                                              int first) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= S * T) return;
    const int64_t s = g / T, t = g % T;
    sum[g] = (first ? 0.0 : sum[g]) + level[s * ld + t];
}

__global__ __launch_bounds__(256) void arima_diag_kernel(const double* __restrict__ level, int64_t ld, int64_t S,
                                                         int64_t col, double* __restrict__ diag, int d, int k) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < S) diag[s * d + k] = level[s * ld + col];
}

// results (:563-602) before the inverse differencing of the last d + n_future values
__global__ __launch_bounds__(256) void arima_forecast_merge_kernel(const double* __restrict__ ts, int64_t ld_ts,
                                                                   const double* __restrict__ sum,
                                                                   const double* __restrict__ raw,
                                                                   const double* __restrict__ diag,
                                                                   double* __restrict__ out, int64_t ld_out, int64_t S,
                                                                   int64_t T, int d, int n_future) {
    const int64_t TO = T + n_future;
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= S * TO) return;
    const int64_t s = g / TO, t = g % TO;
    double v;
    if (t >= T) v = raw[s * TO + t];
    else if (t >= T - d) v = diag[s * d + (t - (T - d))];
    else if (t < d) v = ts[s * ld_ts + t];
    else v = sum[s * T + t - 1] + raw[s * TO + d + t];   // (:591): hist(maxLag + i), as written
    out[s * ld_out + t] = v;
}

// ---- Hannan-Rissanen start (:207-233): stages two and three ------------------------------
//
// One thread per series.  The AR(m) one-step errors (:217-223) are recomputed on the fly in
// every sweep; the second regression (:225-231) is solved on centred columns (with an
// intercept) through a Cholesky factor of the Gram matrix plus one refinement step from the
// residuals of the data (corrected semi-normal equations), which brings the error from
// cond^2 eps to about cond eps.  Slopes in a fixed layout: 0-3 AR lags, 4-7 error lags.
constexpr int kHrK = 2 * kArimaQ;

template <class F>
__device__ __forceinline__ void hr_sweep(const double* y, int N, int p, int q, double c,
                                         const double (&ph)[kArimaQ + 1], F&& f) {
    const int maxLag = p > q ? p : q, m = maxLag + 1;
    double yw[kArimaQ + 1], ew[kArimaQ];
#pragma unroll
    for (int j = 0; j <= kArimaQ; j++) yw[j] = 0.0;
#pragma unroll
    for (int j = 0; j < kArimaQ; j++) ew[j] = 0.0;
    for (int i = 0; i < N; i++) {
        const double yi = y[i];
        if (i >= m) {
            double est = 0.0;
#pragma unroll
            for (int j = 0; j <= kArimaQ; j++)
                if (j < m) est = est + yw[j] * ph[j];
            est = est + c;
            const double e = yi - est;
            if (i - m >= maxLag) {
                double x[kHrK];
#pragma unroll
                for (int j = 0; j < kArimaQ; j++) {
                    x[j] = j < p ? yw[j] : 0.0;
                    x[kArimaQ + j] = j < q ? ew[j] : 0.0;
                }
                f(x, yi);
            }
#pragma unroll
            for (int j = kArimaQ - 1; j > 0; j--) ew[j] = ew[j - 1];
            ew[0] = e;
        }
#pragma unroll
        for (int j = kArimaQ; j > 0; j--) yw[j] = yw[j - 1];
        yw[0] = yi;
    }
}

// L L' = G in place (lower), false when a pivot is not above tol * the diagonal entry
__device__ __forceinline__ bool hr_cholesky(double (&G)[kHrK][kHrK], bool& nan) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kHrK; j++) {
        double dj = G[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) dj -= G[j][k] * G[j][k];
        nan = nan || dj != dj;
        ok = ok && dj > G[j][j] * 1e-14;
        const double l = __builtin_sqrt(dj);
        G[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < kHrK; i++) {
            double v = G[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= G[i][k] * G[j][k];
            G[i][j] = v / l;
        }
    }
    return ok;
}

__device__ __forceinline__ void hr_solve(const double (&L)[kHrK][kHrK], double (&b)[kHrK]) {
#pragma unroll
    for (int i = 0; i < kHrK; i++) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= L[i][k] * b[k];
        b[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = kHrK - 1; i >= 0; i--) {
        double v = b[i];
#pragma unroll
        for (int k = i + 1; k < kHrK; k++) v -= L[k][i] * b[k];
        b[i] = v / L[i][i];
    }
}

__global__ __launch_bounds__(64) void arima_hr_kernel(ArimaHrArgs a) {
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= a.S) return;
    const double* y = a.in + s * a.ld;
    const int N = a.n_len, p = a.p, q = a.q;
    const int maxLag = p > q ? p : q, m = maxLag + 1, n = a.icpt + p + q;
    const int rows = N - m - maxLag;
    const double c = a.c[s];
    double ph[kArimaQ + 1];
#pragma unroll
    for (int j = 0; j <= kArimaQ; j++) ph[j] = j < m ? a.phi[s * m + j] : 0.0;
    auto on = [&](int j) { return j < kArimaQ ? j < p : j - kArimaQ < q; };

    // column means (intercept) or no centring
    double mx[kHrK], my = 0.0;
#pragma unroll
    for (int j = 0; j < kHrK; j++) mx[j] = 0.0;
    if (a.icpt) {
        hr_sweep(y, N, p, q, c, ph, [&](const double (&x)[kHrK], double r) {
#pragma unroll
            for (int j = 0; j < kHrK; j++) mx[j] += x[j];
            my += r;
        });
#pragma unroll
        for (int j = 0; j < kHrK; j++) mx[j] /= (double)rows;
        my /= (double)rows;
    }
    double G[kHrK][kHrK], b[kHrK];
#pragma unroll
    for (int i = 0; i < kHrK; i++) {
        b[i] = 0.0;
#pragma unroll
        for (int j = 0; j < kHrK; j++) G[i][j] = 0.0;
    }
    hr_sweep(y, N, p, q, c, ph, [&](const double (&x)[kHrK], double r) {
#pragma unroll
        for (int i = 0; i < kHrK; i++) {
            const double xi = x[i] - mx[i];
#pragma unroll
            for (int j = 0; j <= i; j++) G[i][j] += xi * (x[j] - mx[j]);
            b[i] += xi * (r - my);
        }
    });
#pragma unroll
    for (int j = 0; j < kHrK; j++)
        if (!on(j)) G[j][j] = 1.0;   // absent columns: a unit block, slope 0
    bool nan = false;
    const bool ok = hr_cholesky(G, nan);
    hr_solve(G, b);
    // one refinement step from the residuals of the data
    double w[kHrK];
#pragma unroll
    for (int j = 0; j < kHrK; j++) w[j] = 0.0;
    hr_sweep(y, N, p, q, c, ph, [&](const double (&x)[kHrK], double r) {
        double res = r - my;
#pragma unroll
        for (int j = 0; j < kHrK; j++) res -= b[j] * (x[j] - mx[j]);
#pragma unroll
        for (int j = 0; j < kHrK; j++) w[j] += (x[j] - mx[j]) * res;
    });
    hr_solve(G, w);
    double b0 = my;
#pragma unroll
    for (int j = 0; j < kHrK; j++) {
        b[j] += w[j];
        b0 -= b[j] * mx[j];
    }
    const bool singular = !ok && !nan;
    double* out = a.init_out + s * n;
    const double bad = __builtin_nan("");
    if (a.icpt) out[0] = singular ? bad : b0;
#pragma unroll
    for (int j = 0; j < kArimaQ; j++) {
        if (j < p) out[a.icpt + j] = singular ? bad : b[j];
        if (j < q) out[a.icpt + p + j] = singular ? bad : b[kArimaQ + j];
    }
    if (a.err && singular && a.err[s] == 0) a.err[s] = STS_ERR_SINGULAR;
}

}  // namespace

hipError_t launch_arima_css(const ArimaCssArgs& a, bool fit, hipStream_t st) {
    if (fit) return launch_lane_rows(arima_css_kernel<true>, a.S, kSpw, st, a);
    return launch_lane_rows(arima_css_kernel<false>, a.S, kSpw, st, a);
}

hipError_t launch_arima_effects(int op, const ArimaEffectsArgs& a, hipStream_t st) {
    if (a.S <= 0 || a.T <= 0) return hipSuccess;
    switch (op) {
    case kArimaRemove: return launch_lane_rows(arima_effects_kernel<kArimaRemove>, a.S, kESpw, st, a);
    case kArimaAdd: return launch_lane_rows(arima_effects_kernel<kArimaAdd>, a.S, kESpw, st, a);
    case kArimaIntegrate: return launch_lane_rows(arima_effects_kernel<kArimaIntegrate>, a.S, kESpw, st, a);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_arima_forecast(const ArimaForecastArgs& a, hipStream_t st) {
    if (a.S <= 0 || a.T + a.n_future <= 0) return hipSuccess;
    return launch_lane_rows(arima_forecast_kernel, a.S, kESpw, st, a);
}

hipError_t launch_arima_level_sum(const double* level, int64_t ld, double* sum, int64_t S, int64_t T, int first,
                                  hipStream_t st) {
    if (S * T <= 0) return hipSuccess;
    hipLaunchKernelGGL(arima_level_sum_kernel, dim3((unsigned)((S * T + 255) / 256)), dim3(256), 0, st, level, ld, sum,
                       S, T, first);
    return hipGetLastError();
}

hipError_t launch_arima_diag(const double* level, int64_t ld, int64_t S, int64_t col, double* diag, int d, int k,
                             hipStream_t st) {
    if (S <= 0) return hipSuccess;
    hipLaunchKernelGGL(arima_diag_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, level, ld, S, col, diag,
                       d, k);
    return hipGetLastError();
}

hipError_t launch_arima_forecast_merge(const double* ts, int64_t ld_ts, const double* sum, const double* raw,
                                       const double* diag, double* out, int64_t ld_out, int64_t S, int64_t T, int d,
                                       int n_future, hipStream_t st) {
    const int64_t n = S * (T + n_future);
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(arima_forecast_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ts, ld_ts, sum,
                       raw, diag, out, ld_out, S, T, d, n_future);
    return hipGetLastError();
}

hipError_t launch_arima_hr(const ArimaHrArgs& a, hipStream_t st) {
    if (a.S <= 0) return hipSuccess;
    hipLaunchKernelGGL(arima_hr_kernel, dim3((unsigned)((a.S + 63) / 64)), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace sts
