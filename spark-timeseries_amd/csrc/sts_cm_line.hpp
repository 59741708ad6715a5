// sts_cm_line.hpp -- commons-math3 3.4.1's LineSearch, as NonLinearConjugateGradientOptimizer
// builds it, as one resumable state machine shared by the EWMA, GARCH and ARIMA fits
// (sts_ewma_opt.hpp, sts_garch_opt.hpp, sts_arima_opt.hpp):
//
//   BracketFinder(growLimit 100, 500 evaluations).search(f, goal, 0, 1e-8), then
//   BrentOptimizer(1e-15, Double.MIN_VALUE, SimpleUnivariateValueChecker(1e-8, 1e-8)) over the
//   bracket from its middle point.
//
// f is the objective along the search direction, f(t) = objective(point + t * direction); the
// machine knows only t.  cm_line_advance<MIN>(s) runs until it needs f at s.t (it returns
// kCmLineAsk: the caller stores the value in s.f and calls again), until the step is found
// (STS_OK: s.alpha holds it) or until the search fails (the failure's sts_status).  How t becomes
// a request, what is cached and what MaxEval counts stay with the caller.
//
// MIN is `goal == MINIMIZE`.  EWMA passes MINIMIZE; GARCH passes no GoalType and ARIMA passes
// MAXIMIZE, which both make every such test false.  The two sets of branches are restated
// literally -- BracketFinder compares with `<` or `>`, BrentOptimizer works on f or on -f and
// best() keeps the smaller or the larger value -- not as "minimise -f": BracketFinder's EPS_MIN
// guard is not sign-symmetric, so the two differ.  Every comparison keeps the reference's
// operand order and so its NaN behaviour.
//
// Host + device: the device kernels are the product; the host build serves the CPU tests that
// check the machines against straight-line restatements (tests/native/*_sm_harness.cpp).
#pragma once
#include "sts.h"

#if defined(__HIPCC__)
#define STS_HD __host__ __device__
#else
#define STS_HD
#endif

namespace sts {

STS_HD inline unsigned long long cm_bits(double v) { return __builtin_bit_cast(unsigned long long, v); }

// commons-math3 Precision.equals(x, y): within 1 ulp, NaN never equal
STS_HD inline bool cm_equals(double x, double y) {
    const long long xi = (long long)cm_bits(x), yi = (long long)cm_bits(y);
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
STS_HD inline bool cm_converged(double p, double c, double rel, double abs_) {
    const double diff = __builtin_fabs(p - c);
    const double size = __builtin_fmax(__builtin_fabs(p), __builtin_fabs(c));
    return diff <= size * rel || diff <= abs_;
}

struct CmPv {
    double x, v;   // UnivariatePointValuePair
};

constexpr double kCmGold = 1.618034;       // BracketFinder.GOLD
constexpr double kCmEpsMin = 1e-21;        // BracketFinder.EPS_MIN
constexpr double kCmBrentRel = 1e-15;      // LineSearch.REL_TOL_UNUSED
constexpr double kCmBrentAbs = 4.9406564584124654e-324;   // LineSearch.ABS_TOL_UNUSED = Double.MIN_VALUE

constexpr int kCmLineAsk = -1;   // cm_line_advance: evaluate f at s.t into s.f and call again

struct CmLine {
    int pc;           // resume point (0 = start a search)
    int bev;          // BracketFinder's evaluation counter
    int have_prev;    // BrentOptimizer's `previous` is not null
    double t, f;      // the abscissa asked for; its value, supplied by the caller
    double alpha;     // the step found (valid after STS_OK)
    // BracketFinder
    double xA, xB, xC, fA, fB, fC, w, fW, wLim, tmp1, tmp2;
    // BrentOptimizer (fx, fv, fw, fu are -f when !MIN, as isMinim == false does)
    double a, b, x, v, ww, d, e, fx, fv, fw, u, fu, m, tol1, tol2;
    CmPv prev, cur, best;
};

// the next cm_line_advance(s) starts a new search
STS_HD inline void cm_line_start(CmLine& s) { s.pc = 0; }

// BracketFinder's `isMinim ? a < b : a > b`
template <bool MIN>
STS_HD inline bool cm_better(double a, double b) {
    return MIN ? a < b : a > b;
}

// BrentOptimizer.best(a, b, isMinim)
template <bool MIN>
STS_HD inline CmPv cm_best(const CmPv& a, const CmPv& b) {
    return (MIN ? a.v <= b.v : a.v >= b.v) ? a : b;
}

// Yield points: ask for f at t and resume at the label.  A bracket evaluation first bumps
// BracketFinder's own counter, whose limit trips before the request is issued.
#define STS_CM_ASK(tv)                                                                      \
    s.t = (tv);                                                                             \
    s.pc = __LINE__;                                                                        \
    return kCmLineAsk;                                                                      \
    case __LINE__:
#define STS_CM_BASK(tv)                                                                     \
    if (++s.bev > 500) return STS_ERR_TOO_MANY_EVALUATIONS;                                 \
    STS_CM_ASK(tv)

template <bool MIN>
STS_HD inline int cm_line_advance(CmLine& s) {
    switch (s.pc) {
    case 0:
        // ---- BracketFinder.search(f, goal, 0, 1e-8) ----
        s.bev = 0;
        s.xA = 0.0;
        s.xB = 1e-8;
        STS_CM_BASK(s.xA)
        s.fA = s.f;
        STS_CM_BASK(s.xB)
        s.fB = s.f;
        if (cm_better<MIN>(s.fA, s.fB)) {
            s.tmp1 = s.xA; s.xA = s.xB; s.xB = s.tmp1;
            s.tmp1 = s.fA; s.fA = s.fB; s.fB = s.tmp1;
        }
        s.xC = s.xB + kCmGold * (s.xB - s.xA);
        STS_CM_BASK(s.xC)
        s.fC = s.f;
        while (cm_better<MIN>(s.fC, s.fB)) {
            s.tmp1 = (s.xB - s.xA) * (s.fB - s.fC);
            s.tmp2 = (s.xB - s.xC) * (s.fB - s.fA);
            s.w = s.tmp2 - s.tmp1;                                            // val
            s.w = __builtin_fabs(s.w) < kCmEpsMin ? 2 * kCmEpsMin : s.w;      // denom
            s.w = s.xB - ((s.xB - s.xC) * s.tmp2 - (s.xB - s.xA) * s.tmp1) / (2 * s.w);
            s.wLim = s.xB + 100 * (s.xC - s.xB);
            if ((s.w - s.xC) * (s.xB - s.w) > 0) {
                STS_CM_BASK(s.w)
                s.fW = s.f;
                if (cm_better<MIN>(s.fW, s.fC)) {
                    s.xA = s.xB; s.xB = s.w; s.fA = s.fB; s.fB = s.fW;
                    break;
                } else if (cm_better<MIN>(s.fB, s.fW)) {
                    s.xC = s.w; s.fC = s.fW;
                    break;
                }
                s.w = s.xC + kCmGold * (s.xC - s.xB);
                STS_CM_BASK(s.w)
                s.fW = s.f;
            } else if ((s.w - s.wLim) * (s.wLim - s.xC) >= 0) {
                s.w = s.wLim;
                STS_CM_BASK(s.w)
                s.fW = s.f;
            } else if ((s.w - s.wLim) * (s.xC - s.w) > 0) {
                STS_CM_BASK(s.w)
                s.fW = s.f;
                if (cm_better<MIN>(s.fW, s.fC)) {
                    s.xB = s.xC; s.xC = s.w; s.w = s.xC + kCmGold * (s.xC - s.xB);
                    s.fB = s.fC; s.fC = s.fW;
                    STS_CM_BASK(s.w)
                    s.fW = s.f;
                }
            } else {
                s.w = s.xC + kCmGold * (s.xC - s.xB);
                STS_CM_BASK(s.w)
                s.fW = s.f;
            }
            s.xA = s.xB; s.fA = s.fB;
            s.xB = s.xC; s.fB = s.fC;
            s.xC = s.w; s.fC = s.fW;
        }
        // lo = xA, mid = xB, hi = xC (swapped when lo > hi); SearchInterval validation
        if (s.xA > s.xC) {
            s.tmp1 = s.xA; s.xA = s.xC; s.xC = s.tmp1;
        }
        if (!(s.xA < s.xC) || !(s.xB >= s.xA && s.xB <= s.xC)) return STS_ERR_BAD_ARG;

        // ---- BrentOptimizer.doOptimize over [lo, hi] from mid ----
        s.a = s.xA;
        s.b = s.xC;
        s.x = s.xB;
        s.v = s.x;
        s.ww = s.x;
        s.d = 0.0;
        s.e = 0.0;
        STS_CM_ASK(s.x)
        s.fx = MIN ? s.f : -s.f;
        s.fv = s.fx;
        s.fw = s.fx;
        s.cur.x = s.x;
        s.cur.v = s.f;                       // isMinim ? fx : -fx
        s.best = s.cur;
        s.have_prev = 0;
        for (;;) {
            s.m = 0.5 * (s.a + s.b);
            s.tol1 = kCmBrentRel * __builtin_fabs(s.x) + kCmBrentAbs;
            s.tol2 = 2 * s.tol1;
            if (__builtin_fabs(s.x - s.m) <= s.tol2 - 0.5 * (s.b - s.a)) {
                // best(best, best(previous, current))
                s.prev = s.have_prev ? cm_best<MIN>(s.prev, s.cur) : s.cur;
                s.alpha = cm_best<MIN>(s.best, s.prev).x;
                break;
            }
            if (__builtin_fabs(s.e) > s.tol1) {   // fit parabola (p -> tmp1, q -> tmp2, r -> u)
                s.u = (s.x - s.ww) * (s.fv - s.fx);
                s.tmp2 = (s.x - s.v) * (s.fw - s.fx);
                s.tmp1 = (s.x - s.v) * s.tmp2 - (s.x - s.ww) * s.u;
                s.tmp2 = 2 * (s.tmp2 - s.u);
                if (s.tmp2 > 0) s.tmp1 = -s.tmp1;
                else s.tmp2 = -s.tmp2;
                s.u = s.e;
                s.e = s.d;
                if (s.tmp1 > s.tmp2 * (s.a - s.x) && s.tmp1 < s.tmp2 * (s.b - s.x) &&
                    __builtin_fabs(s.tmp1) < __builtin_fabs(0.5 * s.tmp2 * s.u)) {
                    s.d = s.tmp1 / s.tmp2;
                    s.u = s.x + s.d;
                    if (s.u - s.a < s.tol2 || s.b - s.u < s.tol2) s.d = (s.x <= s.m) ? s.tol1 : -s.tol1;
                } else {
                    s.e = (s.x < s.m) ? s.b - s.x : s.a - s.x;
                    s.d = (0.5 * (3 - __builtin_sqrt(5.0))) * s.e;
                }
            } else {
                s.e = (s.x < s.m) ? s.b - s.x : s.a - s.x;
                s.d = (0.5 * (3 - __builtin_sqrt(5.0))) * s.e;
            }
            if (__builtin_fabs(s.d) < s.tol1) s.u = (s.d >= 0) ? s.x + s.tol1 : s.x - s.tol1;
            else s.u = s.x + s.d;
            STS_CM_ASK(s.u)
            s.fu = MIN ? s.f : -s.f;
            s.prev = s.cur;
            s.have_prev = 1;
            s.cur.x = s.u;
            s.cur.v = s.f;                   // isMinim ? fu : -fu
            s.best = cm_best<MIN>(s.best, cm_best<MIN>(s.prev, s.cur));
            if (cm_converged(s.prev.v, s.cur.v, 1e-8, 1e-8)) {
                s.alpha = s.best.x;
                break;
            }
            if (s.fu <= s.fx) {
                if (s.u < s.x) s.b = s.x;
                else s.a = s.x;
                s.v = s.ww; s.fv = s.fw;
                s.ww = s.x; s.fw = s.fx;
                s.x = s.u; s.fx = s.fu;
            } else {
                if (s.u < s.x) s.a = s.u;
                else s.b = s.u;
                if (s.fu <= s.fw || cm_equals(s.ww, s.x)) {
                    s.v = s.ww; s.fv = s.fw;
                    s.ww = s.u; s.fw = s.fu;
                } else if (s.fu <= s.fv || cm_equals(s.v, s.x) || cm_equals(s.v, s.ww)) {
                    s.v = s.u; s.fv = s.fu;
                }
            }
        }
        return STS_OK;
    default:
        return STS_ERR_HIP;   // unreachable
    }
}
#undef STS_CM_ASK
#undef STS_CM_BASK

}  // namespace sts
