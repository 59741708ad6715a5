// sts_arima_opt.hpp -- commons-math3 3.4.1's optimizer for ARIMA.fitModel's "css-cgd" method
// (S/models/ARIMA.scala:166-192) as a resumable per-series state machine over an
// n-dimensional point, n = intercept + p + q <= kArimaDim.
//
//   NonLinearConjugateGradientOptimizer(FLETCHER_REEVES, SimpleValueChecker(1e-7, 1e-7))
//   optimize(ObjectiveFunction(logLikelihoodCSSARMA), ObjectiveFunctionGradient(gradient...),
//            GoalType.MAXIMIZE, InitialGuess(initParams), MaxIter(10000), MaxEval(10000))
//
// This is sts_garch_opt.hpp's machine at a run-time dimension: the same BracketFinder(100, 500)
// search from (0, 1e-8), the same BrentOptimizer(1e-15, MIN_VALUE) with
// SimpleUnivariateValueChecker(1e-8, 1e-8), restated the same way.  GARCH passes no GoalType
// and ARIMA passes MAXIMIZE: both make every `goal == MINIMIZE` test false, so the branches
// are the ones that file restates (gradient used as is, BracketFinder comparing with `>`,
// Brent negating f).  What differs: the start point is the caller's, the outer checker is
// (1e-7, 1e-7), and the direction restarts when iterations % n == 0 (n is the point's length;
// GARCH's 3) or the Fletcher-Reeves beta < 0.
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
#include "sts.h"

#if defined(__HIPCC__)
#define STS_HD __host__ __device__
#else
#define STS_HD
#endif

namespace sts {

constexpr int kArimaDim = 2 * STS_ARIMA_MAX_ORDER + 1;
constexpr int kArimaCache = 4;

struct APv {
    double x, v;   // UnivariatePointValuePair
};

struct ArimaOpt {
    double res_f, res_g[kArimaDim];   // result of the request being resumed
    double req[kArimaDim];            // requested point (intercept, AR, MA)
    int need_grad;                    // the request wants the gradient too
    int n;                            // the point's length
    int pc;                           // resume point (0 = start)
    int status;                       // -1 running, else the final sts_status
    // NonLinearConjugateGradientOptimizer
    double point[kArimaDim], dir[kArimaDim], delta, cur_v, alpha;
    int have_cur, iter, evals;
    // BracketFinder
    int bev;
    double xA, xB, xC, fA, fB, fC, w, fW, wLim, tmp1, tmp2;
    // BrentOptimizer (f values negated internally, as isMinim == false does)
    double a, b, x, v, ww, d, e, fx, fv, fw, u, fu, m, tol1, tol2;
    APv prev, cur, best;
    int have_prev;
    // reuse: objective at `point` (valid while have_pt), and t -> objective of this line search
    double pt_f, t;
    int have_pt;
    double ct[kArimaCache], cf[kArimaCache];
    int cn;
};

STS_HD inline unsigned long long abits(double v) { return __builtin_bit_cast(unsigned long long, v); }

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
    o.t = 0.0;
#pragma unroll
    for (int i = 0; i < kArimaDim; i++) o.res_g[i] = 0.0;
}

// req = point + t * dir; true when its value is known (then o.res_f holds it)
STS_HD inline bool arima_line_request(ArimaOpt& o, double t) {
    o.t = t;
    o.need_grad = 0;
    bool same = o.have_pt != 0;
#pragma unroll
    for (int i = 0; i < kArimaDim; i++)
        if (i < o.n) {
            o.req[i] = o.point[i] + t * o.dir[i];
            same = same && abits(o.req[i]) == abits(o.point[i]);
        }
    if (same) {
        o.res_f = o.pt_f;
        return true;
    }
    const unsigned long long k = abits(t);
#pragma unroll
    for (int i = 0; i < kArimaCache; i++)
        if (i < o.cn && abits(o.ct[i]) == k) {
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
    const int slot = o.cn < kArimaCache ? o.cn : (int)(abits(o.t) % kArimaCache);
#pragma unroll
    for (int i = 0; i < kArimaCache; i++)
        if (i == slot) {
            o.ct[i] = o.t;
            o.cf[i] = o.res_f;
        }
    if (o.cn < kArimaCache) o.cn++;
}

// commons-math3 Precision.equals(x, y): within 1 ulp, NaN never equal
STS_HD inline bool a_equals(double x, double y) {
    const long long xi = (long long)abits(x), yi = (long long)abits(y);
    const unsigned long long sgn = 0x8000000000000000ull;
    bool eq;
    if ((((unsigned long long)(xi ^ yi)) & sgn) == 0) {
        const long long dd = xi - yi;
        eq = (dd < 0 ? -dd : dd) <= 1;
    } else {
        long long dp, dm;
        if (xi < yi) {
            dp = yi;
            dm = (long long)((unsigned long long)xi - sgn);
        } else {
            dp = xi;
            dm = (long long)((unsigned long long)yi - sgn);
        }
        eq = (dp > 1) ? false : (dm <= 1 - dp);
    }
    return eq && !__builtin_isnan(x) && !__builtin_isnan(y);
}

// SimpleValueChecker / SimpleUnivariateValueChecker (no iteration limit)
STS_HD inline bool a_converged(double p, double c, double rel, double abs_) {
    const double diff = __builtin_fabs(p - c);
    const double size = __builtin_fmax(__builtin_fabs(p), __builtin_fabs(c));
    return diff <= size * rel || diff <= abs_;
}

// BrentOptimizer.best(a, b, isMinim = false)
STS_HD inline APv a_best_max(const APv& a, const APv& b) { return (a.v >= b.v) ? a : b; }

constexpr double kAGold = 1.618034;
constexpr double kAEpsMin = 1e-21;
constexpr double kABrentRel = 1e-15;
constexpr double kABrentAbs = 4.9406564584124654e-324;

// Yield points.  STS_AGRAD: computeObjectiveGradient(point), never cached.  STS_AAT(t): the
// objective at point + t * dir; a cached value falls straight through to the resume label.
#define STS_AGRAD()                                                                         \
    _Pragma("unroll") for (int i_ = 0; i_ < kArimaDim; i_++) if (i_ < o.n) o.req[i_] = o.point[i_]; \
    o.need_grad = 1;                                                                        \
    o.pc = __LINE__;                                                                        \
    return;                                                                                 \
    case __LINE__:
#define STS_AAT(t_)                                                                         \
    o.pc = __LINE__;                                                                        \
    if (!arima_line_request(o, (t_))) return;                                               \
    [[fallthrough]];                                                                        \
    case __LINE__:
#define STS_AFAIL(st)                                                                       \
    do {                                                                                    \
        o.status = (st);                                                                    \
        return;                                                                             \
    } while (0)
#define STS_ACOUNT()                                                                        \
    if (++o.evals > 10000) STS_AFAIL(STS_ERR_TOO_MANY_EVALUATIONS);
#define STS_ABCOUNT()                                                                       \
    if (++o.bev > 500) STS_AFAIL(STS_ERR_TOO_MANY_EVALUATIONS);                             \
    STS_ACOUNT()

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
            if (o.have_cur && a_converged(o.cur_v, o.res_f, 1e-7, 1e-7)) {
                o.status = STS_OK;
                return;
            }
            o.have_cur = 1;
            o.cur_v = o.res_f;

            // ---- LineSearch: BracketFinder.search(f, MAXIMIZE, 0, 1e-8) ----
            o.bev = 0;
            o.xA = 0.0;
            o.xB = 1e-8;
            STS_ABCOUNT()
            STS_AAT(o.xA)
            o.fA = o.res_f;
            STS_ABCOUNT()
            STS_AAT(o.xB)
            o.fB = o.res_f;
            if (o.fA > o.fB) {
                o.tmp1 = o.xA; o.xA = o.xB; o.xB = o.tmp1;
                o.tmp1 = o.fA; o.fA = o.fB; o.fB = o.tmp1;
            }
            o.xC = o.xB + kAGold * (o.xB - o.xA);
            STS_ABCOUNT()
            STS_AAT(o.xC)
            o.fC = o.res_f;
            while (o.fC > o.fB) {
                o.tmp1 = (o.xB - o.xA) * (o.fB - o.fC);
                o.tmp2 = (o.xB - o.xC) * (o.fB - o.fA);
                o.w = o.tmp2 - o.tmp1;                                           // val
                o.w = __builtin_fabs(o.w) < kAEpsMin ? 2 * kAEpsMin : o.w;       // denom
                o.w = o.xB - ((o.xB - o.xC) * o.tmp2 - (o.xB - o.xA) * o.tmp1) / (2 * o.w);
                o.wLim = o.xB + 100 * (o.xC - o.xB);
                if ((o.w - o.xC) * (o.xB - o.w) > 0) {
                    STS_ABCOUNT()
                    STS_AAT(o.w)
                    o.fW = o.res_f;
                    if (o.fW > o.fC) {
                        o.xA = o.xB; o.xB = o.w; o.fA = o.fB; o.fB = o.fW;
                        break;
                    } else if (o.fW < o.fB) {
                        o.xC = o.w; o.fC = o.fW;
                        break;
                    }
                    o.w = o.xC + kAGold * (o.xC - o.xB);
                    STS_ABCOUNT()
                    STS_AAT(o.w)
                    o.fW = o.res_f;
                } else if ((o.w - o.wLim) * (o.wLim - o.xC) >= 0) {
                    o.w = o.wLim;
                    STS_ABCOUNT()
                    STS_AAT(o.w)
                    o.fW = o.res_f;
                } else if ((o.w - o.wLim) * (o.xC - o.w) > 0) {
                    STS_ABCOUNT()
                    STS_AAT(o.w)
                    o.fW = o.res_f;
                    if (o.fW > o.fC) {
                        o.xB = o.xC; o.xC = o.w; o.w = o.xC + kAGold * (o.xC - o.xB);
                        o.fB = o.fC; o.fC = o.fW;
                        STS_ABCOUNT()
                        STS_AAT(o.w)
                        o.fW = o.res_f;
                    }
                } else {
                    o.w = o.xC + kAGold * (o.xC - o.xB);
                    STS_ABCOUNT()
                    STS_AAT(o.w)
                    o.fW = o.res_f;
                }
                o.xA = o.xB; o.fA = o.fB;
                o.xB = o.xC; o.fB = o.fC;
                o.xC = o.w; o.fC = o.fW;
            }
            if (o.xA > o.xC) {
                o.tmp1 = o.xA; o.xA = o.xC; o.xC = o.tmp1;
            }
            if (!(o.xA < o.xC) || !(o.xB >= o.xA && o.xB <= o.xC)) STS_AFAIL(STS_ERR_BAD_ARG);

            // ---- BrentOptimizer.doOptimize over [lo, hi] from mid, isMinim = false ----
            o.a = o.xA;
            o.b = o.xC;
            o.x = o.xB;
            o.v = o.x;
            o.ww = o.x;
            o.d = 0.0;
            o.e = 0.0;
            STS_ACOUNT()
            STS_AAT(o.x)
            o.fx = -o.res_f;
            o.fv = o.fx;
            o.fw = o.fx;
            o.cur.x = o.x;
            o.cur.v = -o.fx;
            o.best = o.cur;
            o.have_prev = 0;
            for (;;) {
                o.m = 0.5 * (o.a + o.b);
                o.tol1 = kABrentRel * __builtin_fabs(o.x) + kABrentAbs;
                o.tol2 = 2 * o.tol1;
                if (__builtin_fabs(o.x - o.m) <= o.tol2 - 0.5 * (o.b - o.a)) {
                    o.prev = o.have_prev ? a_best_max(o.prev, o.cur) : o.cur;
                    o.alpha = a_best_max(o.best, o.prev).x;
                    break;
                }
                if (__builtin_fabs(o.e) > o.tol1) {   // fit parabola (p -> tmp1, q -> tmp2, r -> u)
                    o.u = (o.x - o.ww) * (o.fv - o.fx);
                    o.tmp2 = (o.x - o.v) * (o.fw - o.fx);
                    o.tmp1 = (o.x - o.v) * o.tmp2 - (o.x - o.ww) * o.u;
                    o.tmp2 = 2 * (o.tmp2 - o.u);
                    if (o.tmp2 > 0) o.tmp1 = -o.tmp1;
                    else o.tmp2 = -o.tmp2;
                    o.u = o.e;
                    o.e = o.d;
                    if (o.tmp1 > o.tmp2 * (o.a - o.x) && o.tmp1 < o.tmp2 * (o.b - o.x) &&
                        __builtin_fabs(o.tmp1) < __builtin_fabs(0.5 * o.tmp2 * o.u)) {
                        o.d = o.tmp1 / o.tmp2;
                        o.u = o.x + o.d;
                        if (o.u - o.a < o.tol2 || o.b - o.u < o.tol2) o.d = (o.x <= o.m) ? o.tol1 : -o.tol1;
                    } else {
                        o.e = (o.x < o.m) ? o.b - o.x : o.a - o.x;
                        o.d = (0.5 * (3 - __builtin_sqrt(5.0))) * o.e;
                    }
                } else {
                    o.e = (o.x < o.m) ? o.b - o.x : o.a - o.x;
                    o.d = (0.5 * (3 - __builtin_sqrt(5.0))) * o.e;
                }
                if (__builtin_fabs(o.d) < o.tol1) o.u = (o.d >= 0) ? o.x + o.tol1 : o.x - o.tol1;
                else o.u = o.x + o.d;
                STS_ACOUNT()
                STS_AAT(o.u)
                o.fu = -o.res_f;
                o.prev = o.cur;
                o.have_prev = 1;
                o.cur.x = o.u;
                o.cur.v = -o.fu;
                o.best = a_best_max(o.best, a_best_max(o.prev, o.cur));
                if (a_converged(o.prev.v, o.cur.v, 1e-8, 1e-8)) {
                    o.alpha = o.best.x;
                    break;
                }
                if (o.fu <= o.fx) {
                    if (o.u < o.x) o.b = o.x;
                    else o.a = o.x;
                    o.v = o.ww; o.fv = o.fw;
                    o.ww = o.x; o.fw = o.fx;
                    o.x = o.u; o.fx = o.fu;
                } else {
                    if (o.u < o.x) o.a = o.u;
                    else o.b = o.u;
                    if (o.fu <= o.fw || a_equals(o.ww, o.x)) {
                        o.v = o.ww; o.fv = o.fw;
                        o.ww = o.u; o.fw = o.fu;
                    } else if (o.fu <= o.fv || a_equals(o.v, o.x) || a_equals(o.v, o.ww)) {
                        o.v = o.u; o.fv = o.fu;
                    }
                }
            }
            // point[i] += step * searchDirection[i]; r = gradient(point)
            o.have_pt = 0;
#pragma unroll
            for (int i = 0; i < kArimaDim; i++)
                if (i < o.n) o.point[i] = o.point[i] + o.alpha * o.dir[i];
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
#undef STS_ABCOUNT

}  // namespace sts
