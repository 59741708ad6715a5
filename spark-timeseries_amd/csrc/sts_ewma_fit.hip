// sts_ewma_fit.hip -- EWMA.fitModel batched over a panel.
//
// Reference (S/ = src/main/scala/com/cloudera/sparkts/):
//   EWMA.fitModel            S/models/EWMA.scala:44-68
//   EWMAModel.sse            S/models/EWMA.scala:80-95
//   EWMAModel.gradient       S/models/EWMA.scala:102-123
//   addTimeDependentEffects  S/models/EWMA.scala:135-142 (the smoothed series both use)
// The optimizer is commons-math3 3.4.1 (pom.xml:396-400, not vendored):
//   NonLinearConjugateGradientOptimizer(FLETCHER_REEVES, SimpleValueChecker(1e-6, 1e-6)),
//   whose LineSearch is BracketFinder(growLimit 100, 500 evaluations) from [0, 1e-8]
//   followed by BrentOptimizer(1e-15, Double.MIN_VALUE, SimpleUnivariateValueChecker(1e-8,
//   1e-8)); InitialGuess 0.94, MaxIter / MaxEval 10000.  With one parameter the search
//   direction is reset to the steepest descent every iteration (iterations % n == 0).
//
// Device design: one LANE per series runs the optimizer as a resumable state machine
// (EwmaOpt below: every objective / gradient request is a yield point).  A wave owns SPW
// series; each round the wave streams its series block through LDS once (CH-step chunks,
// every load instruction = 64 consecutive steps of one series) and every lane with a
// pending request evaluates sse AND gradient of its own series at its own smoothing value
// in one sequential pass -- the reference's own operation order, so every evaluation is
// bit-exact and the optimizer takes the reference's path.  Rows of finished series are not
// loaded.  A small per-lane cache of evaluated points serves the optimizer's repeated
// requests (the objective at the point whose gradient was just computed, the line search's
// f(0)) without a pass; the evaluation COUNTERS still count them, as commons-math3 does.
// A series containing NaN (T >= 2) makes every sse NaN, so the reference's optimizer can
// only end in TooManyEvaluationsException: that is decided after the first pass.
#include "sts_ewma_opt.hpp"
#include "sts_internal.hpp"
#include "sts_lane_rows.hpp"

#include <hip/hip_runtime.h>

namespace sts {
namespace {

// One sequential pass of EWMAModel.sse (:80-95) and .gradient (:102-123) over chunk
// [c0, len) of a series row; state carried across chunks.  Statement order and operands
// are the reference's (no FMA: the library is built with -ffp-contract=off).
struct SseGrad {
    double sm, prevS, prevD, xprev, sq, dJ;
    bool bad;
    __device__ __forceinline__ void start(double x0) {
        sm = x0;       // smoothed(0) = ts(0)
        prevS = x0;    // prevSmoothed = ts(0)
        prevD = 0.0;
        xprev = x0;
        sq = 0.0;
        dJ = 0.0;
        bad = x0 != x0;
    }
    __device__ __forceinline__ void run(const double* row, int c0, int len, double s, double oms) {
#pragma unroll 8
        for (int c = c0; c < len; c++) {
            const double x = row[c];
            bad |= x != x;
            const double err = x - sm;               // ts(i + 1) - smoothed(i)
            sq += err * err;                         // sqrErrors += error * error
            const double dS = xprev - prevS + oms * prevD;   // ts(i) - prevSmoothed + (1 - s) * prevDSda
            dJ += err * dS;
            prevD = dS;
            prevS = sm;
            sm = s * x + oms * sm;                   // smoothed(i + 1)
            xprev = x;
        }
    }
};

// One wave = SPW series (lanes < SPW), CH-step chunks through LDS (stream_rows, sts_lane_rows.hpp).
// Each round every lane with a pending request evaluates sse and gradient at its own smoothing
// value; FIT = false is the plain sse / gradient operator (one round at smoothing[s]).
template <int SPW, int CH, bool FIT>
__global__ __launch_bounds__(64) void ewma_fit_kernel(EwmaFitArgs a) {
    __shared__ double tile[LaneRows<SPW, CH>::kTile];
    const LaneBlock<SPW> b(a.S);
    const int64_t sl = b.sl;
    const bool live = b.live;
    const int64_t T = a.T;

    EwmaOpt o;
    ewma_init(o);
    if (FIT) {
        if (live) ewma_advance(o);
    } else {
        o.req = live ? a.smoothing[sl] : 0.0;
    }
    bool first = true;
    for (;;) {
        const bool pending = live && o.status < 0;
        const unsigned long long want = __ballot(pending);   // rows to stream this round
        if (want == 0) break;
        const double s = o.req, oms = 1.0 - s;
        SseGrad g;
        g.start(0.0);
        stream_rows<SPW, CH>(tile, a.in + b.s0 * a.ld, a.ld, T, b.ns, want, pending, [&](const double* myrow, int64_t tc, int len) {
            if (tc == 0) g.start(myrow[0]);
            g.run(myrow, tc == 0 ? 1 : 0, len, s, oms);
        });
        if (pending) {
            o.res_f = g.sq;
            o.res_g = 2 * g.dJ;
            if (!FIT) {
                o.status = STS_OK;
            } else if (first && g.bad && T >= 2) {
                o.status = STS_ERR_TOO_MANY_EVALUATIONS;   // every sse is NaN (see header)
            } else {
                cache_insert(o);
                ewma_advance(o);
            }
        }
        first = false;
    }
    if (!live) return;
    if (FIT) {
        a.smoothing[sl] = (o.status == STS_OK) ? o.point : __builtin_nan("");
        if (a.err) a.err[sl] = o.status;
        if (a.evals) a.evals[sl] = o.evals;
    } else {
        if (a.sse) a.sse[sl] = o.res_f;
        if (a.grad) a.grad[sl] = o.res_g;
    }
}

#ifndef STS_EWMA_SPW
#define STS_EWMA_SPW 32   // series per wave (lanes that run the pass)
#endif
#ifndef STS_EWMA_CH
#define STS_EWMA_CH 64    // steps per LDS chunk
#endif
constexpr int kFitSpw = STS_EWMA_SPW;
constexpr int kFitCh = STS_EWMA_CH;

}  // namespace

hipError_t launch_ewma_fit(const EwmaFitArgs& a, bool fit, hipStream_t st) {
    if (fit) return launch_lane_rows(ewma_fit_kernel<kFitSpw, kFitCh, true>, a.S, kFitSpw, st, a);
    return launch_lane_rows(ewma_fit_kernel<kFitSpw, kFitCh, false>, a.S, kFitSpw, st, a);
}

}  // namespace sts
