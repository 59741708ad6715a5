// sts_garch_opt.hpp -- commons-math3 3.4.1's optimizer for GARCH.fitModel
// (S/models/GARCH.scala:33-53) as a resumable per-series state machine over a 3-D point
// (omega, alpha, beta).
//
//   NonLinearConjugateGradientOptimizer(FLETCHER_REEVES, SimpleValueChecker(1e-6, 1e-6))
//   optimize(ObjectiveFunction(logLikelihood), ObjectiveFunctionGradient(gradient),
//            InitialGuess(.2, .2, .2), MaxIter(10000), MaxEval(10000))      -- no GoalType
//
// No GoalType is passed, so getGoalType() is null and every `goal == MINIMIZE` branch of
// the optimizer and its LineSearch is false: the gradient is used as is (ascent) and the
// line search is sts_cm_line.hpp's machine with MIN = false, which says why that is not
// "minimise -f".  The search direction restarts when iterations % 3 == 0 or the
// Fletcher-Reeves beta < 0.
//
// Same protocol as sts_ewma_opt.hpp: garch_advance(o) runs until the next evaluation whose
// point is not in the per-lane cache (o.status < 0, o.req holds the point) or the end
// (o.status >= 0).  The caller evaluates logLikelihood AND gradient at o.req into o.res_f /
// o.res_g, calls garch_cache_insert(o) and garch_advance(o) again.  Host + device: the
// device kernel (sts_garch.hip) is the product; the host build exists for the CPU test that
// checks the machine against the oracle's straight-line restatement.
#pragma once
#include "sts_cm_line.hpp"

namespace sts {

constexpr int kGarchCache = 4;

struct GarchOpt {
    double res_f, res_g[3];   // result of the request being resumed (logLikelihood, gradient)
    double req[3];            // requested point (omega, alpha, beta)
    int pc;                   // resume point (0 = start)
    int status;               // -1 running, else the final sts_status
    // NonLinearConjugateGradientOptimizer
    double point[3], dir[3], delta, cur_v;
    int have_cur, iter, evals;
    int cn;                   // entries of the cache below
    CmLine ls;                // LineSearch
    // evaluated points -> (logLikelihood, gradient)
    unsigned long long cs[kGarchCache][3];
    double cf[kGarchCache], cg[kGarchCache][3];
};

STS_HD inline void garch_init(GarchOpt& o) {
    o.pc = 0;
    o.status = -1;
    o.iter = 0;
    o.evals = 0;
    o.have_cur = 0;
    o.cn = 0;
    o.res_f = 0.0;
    o.res_g[0] = o.res_g[1] = o.res_g[2] = 0.0;
}

STS_HD inline bool garch_cache_lookup(GarchOpt& o) {
    const unsigned long long k0 = cm_bits(o.req[0]), k1 = cm_bits(o.req[1]), k2 = cm_bits(o.req[2]);
#pragma unroll
    for (int i = 0; i < kGarchCache; i++)
        if (i < o.cn && o.cs[i][0] == k0 && o.cs[i][1] == k1 && o.cs[i][2] == k2) {
            o.res_f = o.cf[i];
            o.res_g[0] = o.cg[i][0];
            o.res_g[1] = o.cg[i][1];
            o.res_g[2] = o.cg[i][2];
            return true;
        }
    return false;
}

STS_HD inline void garch_cache_insert(GarchOpt& o) {
    const int slot = o.cn < kGarchCache ? o.cn : (int)((cm_bits(o.req[0]) ^ cm_bits(o.req[1]) ^ cm_bits(o.req[2])) % kGarchCache);
#pragma unroll
    for (int i = 0; i < kGarchCache; i++)
        if (i == slot) {
            o.cs[i][0] = cm_bits(o.req[0]);
            o.cs[i][1] = cm_bits(o.req[1]);
            o.cs[i][2] = cm_bits(o.req[2]);
            o.cf[i] = o.res_f;
            o.cg[i][0] = o.res_g[0];
            o.cg[i][1] = o.res_g[1];
            o.cg[i][2] = o.res_g[2];
        }
    if (o.cn < kGarchCache) o.cn++;
}

// Yield points: the request is point + t * dir (or the point itself); a cache hit falls
// straight through to the resume label.
#define STS_GREQ(t)                                                                         \
    o.req[0] = o.point[0] + (t) * o.dir[0];                                                 \
    o.req[1] = o.point[1] + (t) * o.dir[1];                                                 \
    o.req[2] = o.point[2] + (t) * o.dir[2];
#define STS_GYIELD()                                                                        \
    o.pc = __LINE__;                                                                        \
    if (!garch_cache_lookup(o)) return;                                                     \
    [[fallthrough]];                                                                        \
    case __LINE__:
#define STS_GFAIL(st)                                                                       \
    do {                                                                                    \
        o.status = (st);                                                                    \
        return;                                                                             \
    } while (0)
#define STS_GCOUNT()                                                                        \
    if (++o.evals > 10000) STS_GFAIL(STS_ERR_TOO_MANY_EVALUATIONS);
#define STS_GAT(t)                                                                          \
    STS_GREQ(t)                                                                             \
    STS_GYIELD()

__attribute__((noinline)) STS_HD void garch_advance(GarchOpt& o) {
    switch (o.pc) {
    case 0:
        o.point[0] = .2;                                  // InitialGuess(Array(.2, .2, .2))
        o.point[1] = .2;
        o.point[2] = .2;
        o.req[0] = o.point[0];
        o.req[1] = o.point[1];
        o.req[2] = o.point[2];
        STS_GYIELD()                                      // computeObjectiveGradient (not counted)
        // goal != MINIMIZE: r = gradient; identity preconditioner: steepest = r
        o.dir[0] = o.res_g[0];
        o.dir[1] = o.res_g[1];
        o.dir[2] = o.res_g[2];
        o.delta = 0;
        o.delta += o.res_g[0] * o.dir[0];
        o.delta += o.res_g[1] * o.dir[1];
        o.delta += o.res_g[2] * o.dir[2];
        for (;;) {
            if (++o.iter > 10000) STS_GFAIL(STS_ERR_TOO_MANY_ITERATIONS);
            STS_GCOUNT()
            o.req[0] = o.point[0];                        // objective at the current point
            o.req[1] = o.point[1];
            o.req[2] = o.point[2];
            STS_GYIELD()
            if (o.have_cur && cm_converged(o.cur_v, o.res_f, 1e-6, 1e-6)) {
                o.status = STS_OK;
                return;
            }
            o.have_cur = 1;
            o.cur_v = o.res_f;

            // ---- LineSearch.search(point, dir), no GoalType ----
            cm_line_start(o.ls);
            for (;;) {
                {
                    const int st = cm_line_advance<false>(o.ls);
                    if (st == STS_OK) break;
                    if (st != kCmLineAsk) STS_GFAIL(st);
                }
                STS_GCOUNT()
                STS_GAT(o.ls.t)
                o.ls.f = o.res_f;
            }
            // point[i] += step * searchDirection[i]; r = gradient(point)
            o.point[0] = o.point[0] + o.ls.alpha * o.dir[0];
            o.point[1] = o.point[1] + o.ls.alpha * o.dir[1];
            o.point[2] = o.point[2] + o.ls.alpha * o.dir[2];
            o.req[0] = o.point[0];
            o.req[1] = o.point[1];
            o.req[2] = o.point[2];
            STS_GYIELD()                                  // computeObjectiveGradient(point)
            {
                const double deltaOld = o.delta;
                double dl = 0;
                dl += o.res_g[0] * o.res_g[0];
                dl += o.res_g[1] * o.res_g[1];
                dl += o.res_g[2] * o.res_g[2];
                o.delta = dl;
                const double beta = o.delta / deltaOld;   // FLETCHER_REEVES
                if (o.iter % 3 == 0 || beta < 0) {
                    o.dir[0] = o.res_g[0];
                    o.dir[1] = o.res_g[1];
                    o.dir[2] = o.res_g[2];
                } else {
                    o.dir[0] = o.res_g[0] + beta * o.dir[0];
                    o.dir[1] = o.res_g[1] + beta * o.dir[1];
                    o.dir[2] = o.res_g[2] + beta * o.dir[2];
                }
            }
        }
    default:
        STS_GFAIL(STS_ERR_HIP);   // unreachable
    }
}
#undef STS_GREQ
#undef STS_GYIELD
#undef STS_GFAIL
#undef STS_GCOUNT
#undef STS_GAT

}  // namespace sts
