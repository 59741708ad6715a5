// sts_roll.hip -- rolling-window statistics of a panel, alone and against a second panel or one
// shared factor (include/sts_roll.h r1 / r2).  DESIGN.md section 5.22.
//
// Every window is evaluated directly from LDS, in the header's order: no sum is slid, differenced or
// shared between windows.  That costs O(window) per output and is what makes an output a function of
// its own window alone (the header's purity contract): there is no state that a tile, a row or a
// launch could hand to the next.
//
// Tiling.  A workgroup of four waves owns kRollTile consecutive steps of one row, or -- when a whole
// row fits a tile -- as many whole rows as its buffer holds (roll_plan).  It loads each of its rows'
// segments once, coalesced, behind a halo of window - 1 steps re-read from HBM; the part of a halo
// that lies before the series start is NaN, so a truncated window is literally the full window whose
// missing part is missing values.  In the pair kernel a step that is NaN on either side is NaN in
// both buffers, so validity is `v == v` on x alone, with selects.
//
// Lanes and chains.  Consecutive lanes take consecutive outputs, so a wave's LDS read is 64
// consecutive doubles (rows of a multi-row workgroup are window - 1 apart at the seams).  Each output
// is one dependent FP64 chain; a thread carries kRollChains outputs, kThreads apart, through the
// window loop together, so the chains of a wave interleave on the DP pipe.
//
// One template over the op: SUM / MEAN / MIN / MAX read the window once; VAR / STD / ZSCORE and the
// pair ops read it twice, means (with the window's min and max, for the bit-constant rule) and then
// the centred pass.  -0.0 is the additive identity of IEEE addition, so "s = the first valid value,
// then s + x" is a select-only chain started from -0.0.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sts_internal.hpp"

namespace sts {
namespace {

constexpr int kThreads = 256;
constexpr int kNC = kRollChains;
static_assert(kRollTile >= 64 && kNC >= 1 && kNC <= 8, "tile and chains");
static_assert((size_t)2 * kRollCap * sizeof(double) <= (64u << 10), "static LDS of the pair kernel");

// what this workgroup owns: nr rows from row0, the steps t0 .. t0 + len of each; a row's segment
// sits behind its H halo steps, P doubles per row
struct Geo {
    int64_t row0, t0;
    int nr, len, H, P, nout;
};

__device__ __forceinline__ Geo geo(const RollArgs& a, const RollPlan& p, int64_t s0, int64_t n) {
    Geo g;
    g.H = a.window - 1;
    if (p.tiles == 1) {
        g.row0 = s0 + (int64_t)blockIdx.y * p.rows;
        const int64_t left = s0 + n - g.row0;
        g.nr = left < p.rows ? (int)left : p.rows;
        g.t0 = 0;
        g.len = (int)a.T;
    } else {
        g.row0 = s0 + blockIdx.y;
        g.nr = 1;
        g.t0 = (int64_t)blockIdx.x * kRollTile;
        g.len = a.T - g.t0 < kRollTile ? (int)(a.T - g.t0) : kRollTile;
    }
    g.P = g.len + g.H;
    g.nout = g.nr * g.len;
    return g;
}

// element h of row r's buffer is step t0 - H + h: below T by construction (h < len + H), NaN before
// the series start
template <bool PAIR>
__device__ __forceinline__ void load_rows(const RollArgs& a, const Geo& g, double* bx, double* by) {
    const int total = g.nr * g.P;
    for (int e = threadIdx.x; e < total; e += kThreads) {
        const int r = e / g.P, h = e - r * g.P;
        const int64_t t = g.t0 - g.H + h;
        double vx = NAN, vy = NAN;
        if (t >= 0) {
            vx = a.x[(g.row0 + r) * a.ld_x + t];
            if (PAIR) vy = a.y[(g.row0 + r) * a.ld_y + t];
        }
        if (PAIR) {
            const bool bad = vx != vx || vy != vy;
            bx[e] = bad ? NAN : vx;
            by[e] = bad ? NAN : vy;
        } else {
            bx[e] = vx;
        }
    }
    __syncthreads();
}

// the kNC outputs of this thread in the round from `base`: where each one's window starts in the
// buffer and where its result goes; an output past nout computes output 0 again and stores nothing
struct Round {
    int adr[kNC];
    int64_t dst[kNC];
    bool live[kNC];
};

__device__ __forceinline__ Round round_of(const Geo& g, int64_t ld_out, int base) {
    Round q;
#pragma unroll
    for (int m = 0; m < kNC; m++) {
        const int o = base + (int)threadIdx.x + kThreads * m;
        q.live[m] = o < g.nout;
        const int oo = q.live[m] ? o : 0;
        const int r = oo / g.len, i = oo - r * g.len;
        q.adr[m] = r * g.P + i;
        q.dst[m] = (g.row0 + r) * ld_out + g.t0 + i;
    }
    return q;
}

__device__ __forceinline__ bool neg_sign(double v) { return __double2hiint(v) < 0; }
__device__ __forceinline__ bool finite_range(double mn, double mx) { return mn > -INFINITY && mx < INFINITY; }
__device__ __forceinline__ double m2_of(double q, double r, double dn, bool constant) {
    double m2 = q - (r * r) / dn;
    if (constant) m2 = 0.0;
    return m2 < 0.0 ? 0.0 : m2;
}

template <int OP>
__global__ __launch_bounds__(kThreads) void roll_stat_kernel(RollArgs a, RollPlan p, int64_t s0, int64_t n_rows) {
    __shared__ double buf[kRollCap];
    const Geo g = geo(a, p, s0, n_rows);
    load_rows<false>(a, g, buf, nullptr);
    const int w = a.window;
    constexpr bool kTwoPass = OP == STS_ROLL_VAR || OP == STS_ROLL_STD || OP == STS_ROLL_ZSCORE;
    for (int base = 0; base < g.nout; base += kThreads * kNC) {
        const Round q = round_of(g, a.ld_out, base);
        double s[kNC], lo[kNC], hi[kNC];
        int n[kNC];
#pragma unroll
        for (int m = 0; m < kNC; m++) {
            s[m] = -0.0;
            lo[m] = INFINITY;
            hi[m] = -INFINITY;
            n[m] = 0;
        }
        for (int k = 0; k < w; k++) {
#pragma unroll
            for (int m = 0; m < kNC; m++) {
                const double v = buf[q.adr[m] + k];
                const bool ok = v == v;
                n[m] += ok ? 1 : 0;
                if (OP == STS_ROLL_MIN) {
                    if (v < lo[m] || (v == lo[m] && neg_sign(v))) lo[m] = v;
                } else if (OP == STS_ROLL_MAX) {
                    if (v > hi[m] || (v == hi[m] && !neg_sign(v))) hi[m] = v;
                } else {
                    const double sv = s[m] + v;
                    s[m] = ok ? sv : s[m];
                    if (kTwoPass) {
                        lo[m] = v < lo[m] ? v : lo[m];   // false for a NaN
                        hi[m] = v > hi[m] ? v : hi[m];
                    }
                }
            }
        }
        double res[kNC];
        if (!kTwoPass) {
#pragma unroll
            for (int m = 0; m < kNC; m++)
                res[m] = OP == STS_ROLL_SUM ? s[m] : OP == STS_ROLL_MEAN ? s[m] / (double)n[m] : OP == STS_ROLL_MIN ? lo[m] : hi[m];
        } else {
            double mu[kNC], r[kNC], qq[kNC];
#pragma unroll
            for (int m = 0; m < kNC; m++) {
                mu[m] = s[m] / (double)n[m];
                r[m] = 0.0;
                qq[m] = 0.0;
            }
            for (int k = 0; k < w; k++) {
#pragma unroll
                for (int m = 0; m < kNC; m++) {
                    const double v = buf[q.adr[m] + k];
                    const bool ok = v == v;
                    const double d = v - mu[m];
                    const double rr = r[m] + d, qn = qq[m] + d * d;
                    r[m] = ok ? rr : r[m];
                    qq[m] = ok ? qn : qq[m];
                }
            }
#pragma unroll
            for (int m = 0; m < kNC; m++) {
                const double dn = (double)n[m];
                const double m2 = m2_of(qq[m], r[m], dn, lo[m] == hi[m] && finite_range(lo[m], hi[m]));
                double v = m2 / (dn - 1.0);
                if (OP != STS_ROLL_VAR) v = sqrt(v);
                if (OP == STS_ROLL_ZSCORE) v = v == 0.0 ? NAN : (buf[q.adr[m] + g.H] - mu[m]) / v;
                res[m] = n[m] < 2 ? NAN : v;
            }
        }
#pragma unroll
        for (int m = 0; m < kNC; m++)
            if (q.live[m]) a.out[q.dst[m]] = n[m] < a.min_periods ? NAN : res[m];
    }
}

template <int OP>
__global__ __launch_bounds__(kThreads) void roll_pair_kernel(RollArgs a, RollPlan p, int64_t s0, int64_t n_rows) {
    __shared__ double bx[kRollCap], by[kRollCap];
    const Geo g = geo(a, p, s0, n_rows);
    load_rows<true>(a, g, bx, by);
    const int w = a.window;
    for (int base = 0; base < g.nout; base += kThreads * kNC) {
        const Round q = round_of(g, a.ld_out, base);
        double sx[kNC], sy[kNC], lox[kNC], hix[kNC], loy[kNC], hiy[kNC];
        int n[kNC];
#pragma unroll
        for (int m = 0; m < kNC; m++) {
            sx[m] = sy[m] = -0.0;
            lox[m] = loy[m] = INFINITY;
            hix[m] = hiy[m] = -INFINITY;
            n[m] = 0;
        }
        for (int k = 0; k < w; k++) {
#pragma unroll
            for (int m = 0; m < kNC; m++) {
                const double vx = bx[q.adr[m] + k], vy = by[q.adr[m] + k];
                const bool ok = vx == vx;   // a step is NaN in both buffers or in neither
                n[m] += ok ? 1 : 0;
                const double ax = sx[m] + vx, ay = sy[m] + vy;
                sx[m] = ok ? ax : sx[m];
                sy[m] = ok ? ay : sy[m];
                lox[m] = vx < lox[m] ? vx : lox[m];   // false for a NaN
                hix[m] = vx > hix[m] ? vx : hix[m];
                loy[m] = vy < loy[m] ? vy : loy[m];
                hiy[m] = vy > hiy[m] ? vy : hiy[m];
            }
        }
        double mx[kNC], my[kNC], rx[kNC], ry[kNC], qx[kNC], qy[kNC], c[kNC];
        bool cx[kNC], cy[kNC], zero[kNC];
#pragma unroll
        for (int m = 0; m < kNC; m++) {
            mx[m] = sx[m] / (double)n[m];
            my[m] = sy[m] / (double)n[m];
            rx[m] = ry[m] = qx[m] = qy[m] = c[m] = 0.0;
            const bool fx = finite_range(lox[m], hix[m]), fy = finite_range(loy[m], hiy[m]);
            cx[m] = lox[m] == hix[m] && fx;
            cy[m] = loy[m] == hiy[m] && fy;
            zero[m] = (cx[m] && fy) || (cy[m] && fx);
        }
        for (int k = 0; k < w; k++) {
#pragma unroll
            for (int m = 0; m < kNC; m++) {
                const double vx = bx[q.adr[m] + k], vy = by[q.adr[m] + k];
                const bool ok = vx == vx;
                const double dx = vx - mx[m], dy = vy - my[m];
                const double nrx = rx[m] + dx, nry = ry[m] + dy;
                const double nqx = qx[m] + dx * dx, nqy = qy[m] + dy * dy, nc = c[m] + dx * dy;
                rx[m] = ok ? nrx : rx[m];
                ry[m] = ok ? nry : ry[m];
                qx[m] = ok ? nqx : qx[m];
                qy[m] = ok ? nqy : qy[m];
                c[m] = ok ? nc : c[m];
            }
        }
#pragma unroll
        for (int m = 0; m < kNC; m++) {
            const double dn = (double)n[m];
            double cxy = c[m] - (rx[m] * ry[m]) / dn;
            if (zero[m]) cxy = 0.0;
            double v;
            if (OP == STS_ROLL_COV) {
                v = cxy / (dn - 1.0);
            } else if (OP == STS_ROLL_CORR) {
                v = cxy / (sqrt(m2_of(qx[m], rx[m], dn, cx[m])) * sqrt(m2_of(qy[m], ry[m], dn, cy[m])));
                v = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);
            } else {
                v = cxy / m2_of(qy[m], ry[m], dn, cy[m]);
            }
            if (q.live[m]) a.out[q.dst[m]] = (n[m] < 2 || n[m] < a.min_periods) ? NAN : v;
        }
    }
}

template <int OP>
hipError_t launch_stat(const RollArgs& a, const RollPlan& p, hipStream_t st) {
    return for_series_slices(a.S, 65535LL * p.rows, [&](int64_t s0, int64_t n) {
        const unsigned gy = (unsigned)((n + p.rows - 1) / p.rows);
        hipLaunchKernelGGL(roll_stat_kernel<OP>, dim3((unsigned)p.tiles, gy), dim3(kThreads), 0, st, a, p, s0, n);
    });
}

template <int OP>
hipError_t launch_pair(const RollArgs& a, const RollPlan& p, hipStream_t st) {
    return for_series_slices(a.S, 65535LL * p.rows, [&](int64_t s0, int64_t n) {
        const unsigned gy = (unsigned)((n + p.rows - 1) / p.rows);
        hipLaunchKernelGGL(roll_pair_kernel<OP>, dim3((unsigned)p.tiles, gy), dim3(kThreads), 0, st, a, p, s0, n);
    });
}

}  // namespace

RollPlan roll_plan(int64_t T, int window) {
    RollPlan p;
    p.tiles = (T + kRollTile - 1) / kRollTile;
    p.rows = p.tiles == 1 ? (int)(kRollCap / (T + window - 1)) : 1;
    return p;
}

hipError_t launch_roll(const RollArgs& a, hipStream_t st) {
    const RollPlan p = roll_plan(a.T, a.window);
    if (a.pair) {
        switch (a.op) {
            case STS_ROLL_COV: return launch_pair<STS_ROLL_COV>(a, p, st);
            case STS_ROLL_CORR: return launch_pair<STS_ROLL_CORR>(a, p, st);
            case STS_ROLL_BETA: return launch_pair<STS_ROLL_BETA>(a, p, st);
        }
        return hipErrorInvalidValue;
    }
    switch (a.op) {
        case STS_ROLL_SUM: return launch_stat<STS_ROLL_SUM>(a, p, st);
        case STS_ROLL_MEAN: return launch_stat<STS_ROLL_MEAN>(a, p, st);
        case STS_ROLL_VAR: return launch_stat<STS_ROLL_VAR>(a, p, st);
        case STS_ROLL_STD: return launch_stat<STS_ROLL_STD>(a, p, st);
        case STS_ROLL_MIN: return launch_stat<STS_ROLL_MIN>(a, p, st);
        case STS_ROLL_MAX: return launch_stat<STS_ROLL_MAX>(a, p, st);
        case STS_ROLL_ZSCORE: return launch_stat<STS_ROLL_ZSCORE>(a, p, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace sts
