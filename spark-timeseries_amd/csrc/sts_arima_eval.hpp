// sts_arima_eval.hpp -- ARIMAModel.logLikelihoodCSSARMA (S/models/ARIMA.scala:278-293, over
// iterateARMA :426-463) and gradientlogLikelihoodCSSARMA (:312-381) of one differenced series
// in one sequential pass, in the reference's statement order, with the state carried from one
// chunk of the series to the next.  Host + device: sts_arima.hip runs it one lane per series;
// tests/native/arima_sm_harness.cpp compiles the same code for the CPU.
//
// Columns are kept in a FIXED layout -- 0: intercept, 1 + j: AR lag j + 1, 5 + j: MA lag j + 1
// -- so every per-lane array is indexed by constants under guards (j < p, j < q) and stays in
// registers; the columns of dEdTheta never mix, so the layout changes no bit.  start() and
// gradient() translate from and to the reference's packed order (intercept, AR, MA).
// The q previous rows of dEdTheta live in a caller-provided ring (LDS on the device):
// element (slot, col) is ring[(slot * kArimaDim + col) * rs].
//
// Literal points of the reference that are kept:
//   - `(-n / 2)` is Int division; `css` sums left to right over drop(maxLag); the gradient's
//     sigma2 accumulates error * error / n per step; math.pow(x, 2) is x * x; math.log is
//     fdlibm's (sts_fdlibm.hpp); `intercept * coefficients(0)` is added with intercept = 0 too.
//   - updateMAErrors (:390-400) copies errs(i) to errs(i + 1) for ASCENDING i, so after the
//     first update every entry past the first holds the same (second newest) error.
//   - dEdTheta row 0 is built from the q previous rows and the rows then move back by one.
//     Parity note: `dEdTheta(1 to -1, ::) := dEdTheta(0 to -2, ::)` assigns overlapping Breeze
//     slices; this restates it as the shift its comment describes (the one that makes the
//     gradient the likelihood's derivative for q = 2).  No JVM is available to confirm that
//     Breeze copies the overlap for q >= 2.
#pragma once
#include "sts_arima_opt.hpp"
#include "sts_fdlibm.hpp"

namespace sts {

constexpr int kArimaQ = STS_ARIMA_MAX_ORDER;

STS_HD inline double arima_pick(const double (&a)[kArimaDim], int idx) {
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < kArimaDim; i++) v = (i == idx) ? a[i] : v;
    return v;
}

// fixed-layout index of packed column c
STS_HD inline int arima_fixed_index(int c, int icpt, int p) {
    return c < icpt ? 0 : (c - icpt < p ? 1 + c - icpt : 1 + kArimaQ + c - icpt - p);
}

struct ArimaEval {
    int p, q, icpt, n_len;   // orders, intercept (0 / 1), the differenced series' length
    bool grad;
    double coef0, phi[kArimaQ], theta[kArimaQ];
    double ma[kArimaQ];      // maTerms
    double hist[kArimaQ];    // y(i - 1) .. y(i - 4)
    double css, sigma2;
    double g[kArimaDim];     // gradient accumulators, fixed layout
    int head;                // ring slot that receives the next row
    double* ring;
    int rs;

    STS_HD inline void start(const double (&coef)[kArimaDim], int p_, int q_, int icpt_, int n_len_, bool grad_,
                             double* ring_, int rs_) {
        p = p_; q = q_; icpt = icpt_; n_len = n_len_; grad = grad_; ring = ring_; rs = rs_;
        coef0 = coef[0];
#pragma unroll
        for (int j = 0; j < kArimaQ; j++) {
            phi[j] = j < p ? arima_pick(coef, icpt + j) : 0.0;
            theta[j] = j < q ? arima_pick(coef, icpt + p + j) : 0.0;
            ma[j] = 0.0;
            hist[j] = 0.0;
        }
        css = 0.0;
        sigma2 = 0.0;
        head = 0;
#pragma unroll
        for (int k = 0; k < kArimaDim; k++) g[k] = 0.0;
        if (grad) {
            for (int s = 0; s < q; s++) {
#pragma unroll
                for (int k = 0; k < kArimaDim; k++) ring[(s * kArimaDim + k) * rs] = 0.0;
            }
        }
    }

    STS_HD inline bool active(int col) const {
        return col == 0 ? icpt != 0 : (col <= kArimaQ ? col - 1 < p : col - 1 - kArimaQ < q);
    }

    // one index i >= maxLag
    STS_HD inline void step(double y) {
        double yhat = 0.0;
        yhat = yhat + (double)icpt * coef0;
#pragma unroll
        for (int j = 0; j < kArimaQ; j++)
            if (j < p) yhat = yhat + hist[j] * phi[j];
#pragma unroll
        for (int j = 0; j < kArimaQ; j++)
            if (j < q) yhat = yhat + ma[j] * theta[j];
        double cur[kArimaDim];
        if (grad) {
#pragma unroll
            for (int col = 0; col < kArimaDim; col++) {
                cur[col] = 0.0;
                if (active(col)) {
#pragma unroll
                    for (int k = 0; k < kArimaQ; k++)
                        if (k < q) {
                            int slot = head - 1 - k;
                            if (slot < 0) slot += q;
                            cur[col] = cur[col] - theta[k] * ring[(slot * kArimaDim + col) * rs];
                        }
                }
            }
            if (icpt) cur[0] = cur[0] - 1.0;
#pragma unroll
            for (int j = 0; j < kArimaQ; j++)
                if (j < p) cur[1 + j] = cur[1 + j] - hist[j];
#pragma unroll
            for (int j = 0; j < kArimaQ; j++)
                if (j < q) cur[1 + kArimaQ + j] = cur[1 + kArimaQ + j] - ma[j];
        }
        const double error = y - yhat;
        css = css + error * error;
        if (grad) sigma2 = sigma2 + error * error / (double)n_len;
        // updateMAErrors: ascending copy, then the newest error in front
#pragma unroll
        for (int i = 0; i < kArimaQ - 1; i++)
            if (i < q - 1) ma[i + 1] = ma[i];
        if (q > 0) ma[0] = error;
        if (grad) {
#pragma unroll
            for (int col = 0; col < kArimaDim; col++)
                if (active(col)) {
                    g[col] = g[col] + cur[col] * error;
                    if (q > 0) ring[(head * kArimaDim + col) * rs] = cur[col];
                }
            if (q > 0) head = head + 1 == q ? 0 : head + 1;
        }
    }

    // indices t0 + c0 .. t0 + len - 1 of the series, row[c] = y(t0 + c)
    STS_HD inline void run(const double* row, int c0, int len, long long t0) {
        const int maxLag = p > q ? p : q;
        for (int cc = c0; cc < len; cc++) {
            const double y = row[cc];
            if (t0 + cc >= maxLag) step(y);
#pragma unroll
            for (int j = kArimaQ - 1; j > 0; j--) hist[j] = hist[j - 1];
            hist[0] = y;
        }
    }

    STS_HD inline double loglik() const {
        const double s2 = css / (double)n_len;
        return (double)(-n_len / 2) * fdlibm_log(6.283185307179586 * s2) - css / (2 * s2);
    }

    // the gradient in the reference's packed order
    STS_HD inline void gradient(double (&out)[kArimaDim]) const {
        const int n = icpt + p + q;
#pragma unroll
        for (int cidx = 0; cidx < kArimaDim; cidx++)
            out[cidx] = cidx < n ? arima_pick(g, arima_fixed_index(cidx, icpt, p)) / -sigma2 : 0.0;
    }
};

}  // namespace sts
