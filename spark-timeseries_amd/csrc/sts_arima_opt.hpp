// sts_arima_opt.hpp -- commons-math3 3.4.1's optimizer for ARIMA.fitModel's "css-cgd" method
// (S/models/ARIMA.scala:166-192) as a resumable per-series state machine over an
// n-dimensional point, n = intercept + p + q <= kArimaDim.
//
//   NonLinearConjugateGradientOptimizer(FLETCHER_REEVES, SimpleValueChecker(1e-7, 1e-7))
//   optimize(ObjectiveFunction(logLikelihoodCSSARMA), ObjectiveFunctionGradient(gradient...),
//            GoalType.MAXIMIZE, InitialGuess(initParams), MaxIter(10000), MaxEval(10000))
//
// The outer loop is sts_garch_opt.hpp's at a run-time dimension.  GARCH passes no GoalType and
// ARIMA passes MAXIMIZE: both make every `goal == MINIMIZE` test false, so the gradient is used
// as is and the line search is sts_cm_line.hpp's machine with MIN = false.  What differs: the
// start point is the caller's, the outer checker is (1e-7, 1e-7), and the direction restarts
// when iterations % n == 0 (n is the point's length; GARCH's 3) or the Fletcher-Reeves beta < 0.
//
// Protocol: arima_advance(o) runs until the next evaluation that is not cached (o.status < 0,
// o.req holds the point, o.need_grad says whether the gradient is wanted) or the end
// (o.status >= 0).  The caller evaluates the objective -- and, when o.need_grad, the gradient
// -- at o.req into o.res_f / o.res_g, calls arima_cache_insert(o) and arima_advance(o) again.
// Only the two computeObjectiveGradient calls want the gradient; every line-search point
// wants the objective alone (the gradient pass costs about (q + 1) n times the objective's).
//
// Cache: an evaluation is a pure function of the point, so reusing a value changes no bit.
// Two reuses cover what the optimizer asks twice: the objective at the point whose gradient
// was just taken (the gradient pass yields it; `computeObjectiveValue(point)` and the
// bracket's f(0) ask again), and line-search abscissae asked again (Brent starts at the
// bracket's middle).  Within one line search the point is start + t * direction with start
// and direction fixed, so the key is t alone.  commons-math3 counts an evaluation whether or
// not it is reused here, so o.evals is the reference's count.
//
// Every per-lane array is indexed by unrolled loops with constant indices, guarded by i < n,
// so that the device keeps them in registers.  Host + device: the device kernel
// (sts_arima.hip) is the product; the host build serves tests/native/arima_sm_harness.cpp.
#pragma once
#include "sts_cm_line.hpp"

namespace sts {

constexpr int kArimaDim = 2 * STS_ARIMA_MAX_ORDER + 1;
constexpr int kArimaCache = 4;

struct ArimaOpt {
    double res_f, res_g[kArimaDim];   // result of the request being resumed
    double req[kArimaDim];            // requested point (intercept, AR, MA)
    int need_grad;                    // the request wants the gradient too
    int n;                            // the point's length
    int pc;                           // resume point (0 = start)
    int status;                       // -1 running, else the final sts_status
    // NonLinearConjugateGradientOptimizer
    double point[kArimaDim], dir[kArimaDim], delta, cur_v;
    int have_cur, iter, evals;
    // reuse: objective at `point` (valid while have_pt), and ls.t -> objective of this line search
    int have_pt;
    CmLine ls;                        // LineSearch
    double pt_f;
    double ct[kArimaCache], cf[kArimaCache];
    int cn;
};

// start: the caller has set o.n and o.point[0 .. n)
STS_HD inline void arima_init(ArimaOpt& o) {
    o.pc = 0;
    o.status = -1;
    o.iter = 0;
    o.evals = 0;
    o.have_cur = 0;
    o.have_pt = 0;
    o.cn = 0;
    o.need_grad = 0;
    o.res_f = 0.0;
#pragma unroll
    for (int i = 0; i < kArimaDim; i++) o.res_g[i] = 0.0;
}

// req = point + ls.t * dir; true when its value is known (then o.res_f holds it)
STS_HD inline bool arima_line_request(ArimaOpt& o) {
    const double t = o.ls.t;
    o.need_grad = 0;
    bool same = o.have_pt != 0;
#pragma unroll
    for (int i = 0; i < kArimaDim; i++)
        if (i < o.n) {
            o.req[i] = o.point[i] + t * o.dir[i];
            same = same && cm_bits(o.req[i]) == cm_bits(o.point[i]);
        }
    if (same) {
        o.res_f = o.pt_f;
        return true;
    }
    const unsigned long long k = cm_bits(t);
#pragma unroll
    for (int i = 0; i < kArimaCache; i++)
        if (i < o.cn && cm_bits(o.ct[i]) == k) {
            o.res_f = o.cf[i];
            return true;
        }
    return false;
}

STS_HD inline void arima_cache_insert(ArimaOpt& o) {
    if (o.need_grad) {   // a gradient request is at `point`: a new line search starts from it
        o.pt_f = o.res_f;
        o.have_pt = 1;
        o.cn = 0;
        return;
    }
    const int slot = o.cn < kArimaCache ? o.cn : (int)(cm_bits(o.ls.t) % kArimaCache);
#pragma unroll
    for (int i = 0; i < kArimaCache; i++)
        if (i == slot) {
            o.ct[i] = o.ls.t;
            o.cf[i] = o.res_f;
        }
    if (o.cn < kArimaCache) o.cn++;
}

// Yield points.  STS_AGRAD: computeObjectiveGradient(point), never cached.  STS_AAT(): the
// objective at point + ls.t * dir; a cached value falls straight through to the resume label.
#define STS_AGRAD()                                                                         \
    _Pragma("unroll") for (int i_ = 0; i_ < kArimaDim; i_++) if (i_ < o.n) o.req[i_] = o.point[i_]; \
    o.need_grad = 1;                                                                        \
    o.pc = __LINE__;                                                                        \
    return;                                                                                 \
    case __LINE__:
#define STS_AAT()                                                                           \
    o.pc = __LINE__;                                                                        \
    if (!arima_line_request(o)) return;                                                     \
    [[fallthrough]];                                                                        \
    case __LINE__:
#define STS_AFAIL(st)                                                                       \
    do {                                                                                    \
        o.status = (st);                                                                    \
        return;                                                                             \
    } while (0)
#define STS_ACOUNT()                                                                        \
    if (++o.evals > 10000) STS_AFAIL(STS_ERR_TOO_MANY_EVALUATIONS);

__attribute__((noinline)) STS_HD void arima_advance(ArimaOpt& o) {
    switch (o.pc) {
    case 0:
        STS_AGRAD()                                       // computeObjectiveGradient (not counted)
        // goal != MINIMIZE: r = gradient; identity preconditioner: steepest = r
        o.delta = 0;
#pragma unroll
        for (int i = 0; i < kArimaDim; i++)
            if (i < o.n) {
                o.dir[i] = o.res_g[i];
                o.delta += o.res_g[i] * o.dir[i];
            }
        for (;;) {
            if (++o.iter > 10000) STS_AFAIL(STS_ERR_TOO_MANY_ITERATIONS);
            STS_ACOUNT()
            o.res_f = o.pt_f;                             // objective at the current point: the
                                                          // gradient pass at it yielded it
            if (o.have_cur && cm_converged(o.cur_v, o.res_f, 1e-7, 1e-7)) {
                o.status = STS_OK;
                return;
            }
            o.have_cur = 1;
            o.cur_v = o.res_f;

            // ---- LineSearch.search(point, dir), MAXIMIZE ----
            cm_line_start(o.ls);
            for (;;) {
                {
                    const int st = cm_line_advance<false>(o.ls);
                    if (st == STS_OK) break;
                    if (st != kCmLineAsk) STS_AFAIL(st);
                }
                STS_ACOUNT()
                STS_AAT()
                o.ls.f = o.res_f;
            }
            // point[i] += step * searchDirection[i]; r = gradient(point)
            o.have_pt = 0;
#pragma unroll
            for (int i = 0; i < kArimaDim; i++)
                if (i < o.n) o.point[i] = o.point[i] + o.ls.alpha * o.dir[i];
            STS_AGRAD()                                   // computeObjectiveGradient(point)
            {
                const double deltaOld = o.delta;
                double dl = 0;
#pragma unroll
                for (int i = 0; i < kArimaDim; i++)
                    if (i < o.n) dl += o.res_g[i] * o.res_g[i];
                o.delta = dl;
                const double beta = o.delta / deltaOld;   // FLETCHER_REEVES
                const bool restart = o.iter % o.n == 0 || beta < 0;
#pragma unroll
                for (int i = 0; i < kArimaDim; i++)
                    if (i < o.n) o.dir[i] = restart ? o.res_g[i] : o.res_g[i] + beta * o.dir[i];
            }
        }
    default:
        STS_AFAIL(STS_ERR_HIP);   // unreachable
    }
}
#undef STS_AGRAD
#undef STS_AAT
#undef STS_AFAIL
#undef STS_ACOUNT

}  // namespace sts
