// sts_ewma_opt.hpp -- commons-math3 3.4.1's optimizer for EWMA.fitModel
// (S/models/EWMA.scala:44-68) as a resumable per-series state machine.
//
//   NonLinearConjugateGradientOptimizer(FLETCHER_REEVES, SimpleValueChecker(1e-6, 1e-6))
//   optimize(..., GoalType.MINIMIZE, InitialGuess 0.94, MaxIter 10000, MaxEval 10000)
//   LineSearch: sts_cm_line.hpp's machine with MIN = true
//
// ewma_advance(o) runs until the next sse / gradient request whose point is not in the
// small evaluation cache (o.req, o.status < 0) or until the optimizer ends (o.status >= 0).
// The caller evaluates EWMAModel.sse and .gradient at o.req, stores them in o.res_f /
// o.res_g, calls cache_insert(o) and ewma_advance(o) again.  Host + device: the device
// kernel (sts_ewma_fit.hip) is the product; the host build exists for the CPU test that
// checks the machine against the oracle's straight-line restatement.
#pragma once
#include "sts_cm_line.hpp"

namespace sts {

constexpr int kEwmaCache = 4;

struct EwmaOpt {
    double res_f, res_g;   // result of the request being resumed (sse, gradient)
    double req;            // requested smoothing value
    int pc;                // resume point (0 = start)
    int status;            // -1 running, else the final sts_status
    // NonLinearConjugateGradientOptimizer
    double point, dir, cur_v;
    int have_cur, iter, evals;
    int cn;                // entries of the cache below
    CmLine ls;             // LineSearch
    // evaluated points (bit patterns of s) -> (sse, gradient)
    unsigned long long cs[kEwmaCache];
    double cf[kEwmaCache], cg[kEwmaCache];
};

STS_HD inline void ewma_init(EwmaOpt& o) {
    o.pc = 0;
    o.status = -1;
    o.iter = 0;
    o.evals = 0;
    o.have_cur = 0;
    o.cn = 0;
    o.res_f = o.res_g = 0.0;
}

STS_HD inline bool ewma_cache_lookup(EwmaOpt& o) {
    const unsigned long long k = cm_bits(o.req);
#pragma unroll
    for (int i = 0; i < kEwmaCache; i++)
        if (i < o.cn && o.cs[i] == k) {
            o.res_f = o.cf[i];
            o.res_g = o.cg[i];
            return true;
        }
    return false;
}

STS_HD inline void cache_insert(EwmaOpt& o) {
    const int slot = o.cn < kEwmaCache ? o.cn : (int)(cm_bits(o.req) % kEwmaCache);
#pragma unroll
    for (int i = 0; i < kEwmaCache; i++)
        if (i == slot) {
            o.cs[i] = cm_bits(o.req);
            o.cf[i] = o.res_f;
            o.cg[i] = o.res_g;
        }
    if (o.cn < kEwmaCache) o.cn++;
}

// Yield points.  Each request stores the smoothing value and the resume label; a cache
// hit falls straight through to the label.  Counted requests (computeObjectiveValue, every
// line-search evaluation) bump the MaxEval counter first.
#define STS_YIELD(sv)                                                                       \
    o.req = (sv);                                                                           \
    o.pc = __LINE__;                                                                        \
    if (!ewma_cache_lookup(o)) return;                                                      \
    [[fallthrough]];                                                                        \
    case __LINE__:
#define STS_FAIL(st)                                                                        \
    do {                                                                                    \
        o.status = (st);                                                                    \
        return;                                                                             \
    } while (0)
#define STS_COUNT()                                                                         \
    if (++o.evals > 10000) STS_FAIL(STS_ERR_TOO_MANY_EVALUATIONS);

// Runs lane o's optimizer until its next uncached request (o.status stays -1) or the end.
__attribute__((noinline)) STS_HD void ewma_advance(EwmaOpt& o) {
    switch (o.pc) {
    case 0:
        o.point = 0.94;                                   // InitialGuess(Array(.94))
        STS_YIELD(o.point)                                // computeObjectiveGradient (not counted)
        o.dir = -o.res_g;                                 // MINIMIZE: r = -g; identity preconditioner
        for (;;) {
            if (++o.iter > 10000) STS_FAIL(STS_ERR_TOO_MANY_ITERATIONS);
            STS_COUNT()
            STS_YIELD(o.point)                            // objective at the current point
            if (o.have_cur && cm_converged(o.cur_v, o.res_f, 1e-6, 1e-6)) {
                o.status = STS_OK;
                return;
            }
            o.have_cur = 1;
            o.cur_v = o.res_f;

            // ---- LineSearch.search(point, dir), MINIMIZE ----
            cm_line_start(o.ls);
            for (;;) {
                {
                    const int st = cm_line_advance<true>(o.ls);
                    if (st == STS_OK) break;
                    if (st != kCmLineAsk) STS_FAIL(st);
                }
                STS_COUNT()
                STS_YIELD(o.point + o.ls.t * o.dir)
                o.ls.f = o.res_f;
            }
            o.point = o.point + o.ls.alpha * o.dir;          // point[i] += step * searchDirection[i]
            STS_YIELD(o.point)                            // computeObjectiveGradient(point)
            o.dir = -o.res_g;                             // iterations % 1 == 0: steepest descent
        }
    default:
        STS_FAIL(STS_ERR_HIP);   // unreachable
    }
}
#undef STS_YIELD
#undef STS_FAIL
#undef STS_COUNT

}  // namespace sts
