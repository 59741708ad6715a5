// sts_cross.hip -- covariance and correlation matrices of a panel and of two panels
// (include/sts_cross.h c1): the one operator of this library that is bound by the FP64 MFMA pipe and
// not by HBM.  DESIGN.md section 5.21.
//
// Numerical form: the corrected two-pass algorithm.  cross_prep_kernel gives every series its mean
// mu, the rest r = sum (x - mu) that rounding leaves in the centred series, its own centred second
// moment C_ii and two flags (a non-finite value; max == min).  cross_gram_kernel forms
// G_ij = sum_t z_i[t] w_j[t] with z = x - mu centred as the values arrive, and the epilogue applies
// C_ij = G_ij - r_i q_j / T, the divide or the normalisation, the clamp, the NaN and constant rules and
// the unit diagonal, in that order.
//
// Gram kernel.  A workgroup of four waves owns one kCrossTile x kCrossTile output tile; wave (wr, wc)
// owns a 32 x 32 quarter as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64, kept in registers across
// the walk over T.  T is walked in stages of kCrossChunk steps: every thread owns one quarter of one
// row of each operand for the whole walk (so its mu is loaded once), loads the next stage's piece
// into registers before the current stage's MFMAs (16-byte loads where base and ld allow, the
// runtime test of sts_ar.hip), and afterwards centres it, zeroes it for t >= T and for rows >= S and
// lays it into the other LDS stage: one barrier per stage.  LDS rows are kCrossChunk + 2 doubles
// apart: lane l reads [row l & 15][k l >> 4], so one 32-lane half of a ds_read_b64 touches the
// doubles row * (kCrossChunk + 2) + k (mod 32), k in {0, 1}, and (kCrossChunk + 2) / 2 is odd -- each
// of the 32 bank pairs once, conflict-free for both operands, and the 16-byte stage writes stay aligned.
//
// Reproducibility (the header's contract).  A partial sum over T is closed every kCrossSplit steps, a
// boundary that depends on T alone, and the closed partials are added in ascending order: by the one
// workgroup that walks them all, or -- when the tiles alone cannot fill the chip (cross_plan) -- by
// cross_finalise_kernel over partials that one workgroup per (tile, segment) left in the scratch.
// Both do 0.0 + p_0 + p_1 + ..., so the two plans give the same bits.  In the symmetric form only
// tiles on or above the diagonal are computed; the mirror tile is written from the same values through
// LDS (both stores are row-contiguous), and on a diagonal tile the lower triangle is the mirror of
// the upper, so the output is symmetric by construction.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "sts_internal.hpp"
#include "sts_wgsum.hpp"

// A split plan is taken below this many tiles (two workgroups per CU on 256 CUs) and while its
// partials fit this many MiB of scratch
#ifndef STS_CROSS_SPLIT_TILES
#define STS_CROSS_SPLIT_TILES 512
#endif
#ifndef STS_CROSS_SPLIT_MB
#define STS_CROSS_SPLIT_MB 512
#endif

namespace sts {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kCT = kCrossTile;
constexpr int kKC = kCrossChunk;
constexpr int kStr = kKC + 2;                          // LDS row pitch of a stage, doubles
constexpr int kGramThreads = 256;
constexpr int kPer = kKC * kCT / kGramThreads;         // doubles of one operand a thread moves per stage
constexpr int kOpBuf = kCT * kStr;                     // one operand's stage
constexpr int kCtPitch = kCT + 1;
constexpr int kCtSize = kCT * kCtPitch;                // the output tile staged for the epilogue
constexpr int kTileElems = kCT * kCT;
constexpr int kGramLds = 4 * kOpBuf > kCtSize ? 4 * kOpBuf : kCtSize;
static_assert(kCT == 64, "the wave map (2 x 2 waves of 2 x 2 MFMA blocks, 4 threads per row) is written for a 64 x 64 tile");
static_assert(kKC % 8 == 0 && kKC >= 8, "a thread moves an even number of steps per operand and stage");
static_assert(kCrossSplit % kKC == 0 && kCrossSplit >= kKC, "a segment is whole stages");
static_assert((size_t)(kGramLds + 2 * kCT * kCrossStat) * sizeof(double) <= (64u << 10), "static LDS");

// ---- prep: one workgroup per series.  Thread j sums the steps j, j + 256, ... in four interleaved
// chains; the chains, then the lanes, then the four waves are combined in a fixed order: a function of
// the row and T alone.  The second sweep re-reads the row the workgroup has just streamed. ----
constexpr int kPrepThreads = 256;
static_assert(kPrepThreads == 256, "four waves: red[4], lo / hi and their combination below");

__global__ __launch_bounds__(kPrepThreads) void cross_prep_kernel(const double* __restrict__ x, int64_t T, int64_t ld,
                                                                 double* __restrict__ stat, double* __restrict__ mean) {
    __shared__ double red[4];
    __shared__ double lo[kPrepThreads / 64], hi[kPrepThreads / 64];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x;
    const double* __restrict__ row = x + s * ld;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    double mn = INFINITY, mx = -INFINITY;
    bool bad = false;
    for (int64_t t = tid; t < T; t += 4 * kPrepThreads) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t tt = t + kPrepThreads * u;
            if (tt < T) {
                const double v = row[tt];
                a[u] += v;
                bad |= !(fabs(v) <= DBL_MAX);
                mn = fmin(mn, v);
                mx = fmax(mx, v);
            }
        }
    }
    const double sum = bsum<kPrepThreads>((a[0] + a[1]) + (a[2] + a[3]), red);
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o, 64));
        mx = fmax(mx, __shfl_xor(mx, o, 64));
    }
    if ((tid & 63) == 0) {
        lo[tid >> 6] = mn;
        hi[tid >> 6] = mx;
    }
    const bool any_bad = __syncthreads_or(bad);   // uniform; also orders lo / hi
    double* st = stat + s * kCrossStat;
    if (any_bad) {
        if (tid == 0) {
            st[0] = NAN;
            st[1] = 0.0;
            st[2] = 0.0;
            st[3] = 2.0;
            if (mean) mean[s] = NAN;
        }
        return;
    }
    const double dT = (double)T;
    const double mu = sum / dT;
    double r[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t = tid; t < T; t += 4 * kPrepThreads) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t tt = t + kPrepThreads * u;
            if (tt < T) {
                const double z = row[tt] - mu;
                r[u] += z;
                q[u] += z * z;
            }
        }
    }
    const double rs = bsum<kPrepThreads>((r[0] + r[1]) + (r[2] + r[3]), red);
    const double qs = bsum<kPrepThreads>((q[0] + q[1]) + (q[2] + q[3]), red);
    if (tid == 0) {
        mn = fmin(fmin(lo[0], lo[1]), fmin(lo[2], lo[3]));
        mx = fmax(fmax(hi[0], hi[1]), fmax(hi[2], hi[3]));
        st[0] = mu;
        st[1] = rs;
        st[2] = qs - (rs * rs) / dT;
        st[3] = mx == mn ? 1.0 : 0.0;
        if (mean) mean[s] = mu;
    }
}

// ---- the tile of a workgroup and its series' statistics ----
struct TileCtx {
    int64_t tile, i0, j0, Sy;
    bool sym, diag;
};

__device__ __forceinline__ TileCtx tile_ctx(const CrossArgs& a, const CrossPlan& p) {
    TileCtx c;
    c.tile = blockIdx.x;
    c.sym = a.y == nullptr;
    c.Sy = c.sym ? a.Sx : a.Sy;
    int64_t I, J;
    if (c.sym) {   // upper triangle, column by column: tile = J (J + 1) / 2 + I, I <= J
        J = (int64_t)((sqrt(8.0 * (double)c.tile + 1.0) - 1.0) * 0.5);
        while ((J + 1) * (J + 2) / 2 <= c.tile) J++;
        while (J * (J + 1) / 2 > c.tile) J--;
        I = c.tile - J * (J + 1) / 2;
    } else {
        I = c.tile / p.tj;
        J = c.tile - I * p.tj;
    }
    c.i0 = I * kCT;
    c.j0 = J * kCT;
    c.diag = c.sym && I == J;
    return c;
}

// rows past the panel get zeros: flag 0, nothing of theirs is stored
__device__ __forceinline__ void load_stats(const CrossArgs& a, const TileCtx& c, const double* __restrict__ sx,
                                           const double* __restrict__ sy, double* st_i, double* st_j) {
    for (int k = threadIdx.x; k < kCT * kCrossStat; k += kGramThreads) {
        const int64_t gi = c.i0 + k / kCrossStat, gj = c.j0 + k / kCrossStat;
        st_i[k] = gi < a.Sx ? sx[gi * kCrossStat + k % kCrossStat] : 0.0;
        st_j[k] = gj < c.Sy ? sy[gj * kCrossStat + k % kCrossStat] : 0.0;
    }
}

// Ct holds G_ij of the tile; the results replace it and go out, with their mirror in the symmetric form
__device__ __forceinline__ void cross_epilogue(const CrossArgs& a, const TileCtx& c, double* Ct, const double* st_i,
                                               const double* st_j) {
    const double dT = (double)a.T, dn1 = (double)(a.T - 1);
    const bool corr = a.kind == STS_CROSS_CORR;
    for (int idx = threadIdx.x; idx < kTileElems; idx += kGramThreads) {
        const int r = idx / kCT, col = idx % kCT;
        const double* si = st_i + r * kCrossStat;
        const double* sj = st_j + col * kCrossStat;
        double v = Ct[r * kCtPitch + col] - (si[1] * sj[1]) / dT;
        if (corr) {
            v = v / (sqrt(si[2]) * sqrt(sj[2]));
            v = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);
        } else {
            v = v / dn1;
        }
        if (si[3] == 2.0 || sj[3] == 2.0) v = NAN;
        else if (si[3] == 1.0 || sj[3] == 1.0) v = corr ? NAN : 0.0;
        else if (corr && c.sym && c.i0 + r == c.j0 + col) v = 1.0;
        Ct[r * kCtPitch + col] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < kTileElems; idx += kGramThreads) {
        const int r = idx / kCT, col = idx % kCT;
        const int64_t gi = c.i0 + r, gj = c.j0 + col;
        if (gi < a.Sx && gj < c.Sy)
            a.out[gi * a.ld_o + gj] = (c.diag && r > col) ? Ct[col * kCtPitch + r] : Ct[r * kCtPitch + col];
    }
    if (c.sym && !c.diag)
        for (int idx = threadIdx.x; idx < kTileElems; idx += kGramThreads) {
            const int col = idx / kCT, r = idx % kCT;   // consecutive threads along the mirror's rows
            const int64_t gi = c.i0 + r, gj = c.j0 + col;
            if (gi < a.Sx && gj < c.Sy) a.out[gj * a.ld_o + gi] = Ct[r * kCtPitch + col];
        }
}

// kPer raw values of one row from step t on; what lies past T (or in a row that is not read) is
// never loaded
__device__ __forceinline__ void load_piece(const double* __restrict__ row, bool live, bool vec, int64_t t, int64_t T,
                                           double (&v)[kPer]) {
#pragma unroll
    for (int e = 0; e < kPer; e += 2) {
        const int64_t tt = t + e;
        if (live && vec && tt + 1 < T) {
            const double2 d = *reinterpret_cast<const double2*>(row + tt);
            v[e] = d.x;
            v[e + 1] = d.y;
        } else {
            v[e] = live && tt < T ? row[tt] : 0.0;
            v[e + 1] = live && tt + 1 < T ? row[tt + 1] : 0.0;
        }
    }
}

// centred, zero past T and in rows that are not read, into the thread's place of a stage
__device__ __forceinline__ void store_piece(double* dst, const double (&v)[kPer], double mu, bool live, int64_t t,
                                            int64_t T) {
#pragma unroll
    for (int e = 0; e < kPer; e += 2) {
        double2 z;
        z.x = live && t + e < T ? v[e] - mu : 0.0;
        z.y = live && t + e + 1 < T ? v[e + 1] - mu : 0.0;
        *reinterpret_cast<double2*>(dst + e) = z;
    }
}

__global__ __launch_bounds__(kGramThreads) void cross_gram_kernel(CrossArgs a, CrossPlan p, const double* __restrict__ sx,
                                                                 const double* __restrict__ sy, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double lds[kGramLds];
    __shared__ double st_i[kCT * kCrossStat], st_j[kCT * kCrossStat];
    const TileCtx c = tile_ctx(a, p);
    load_stats(a, c, sx, sy, st_i, st_j);
    __syncthreads();

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int64_t T = a.T;
    const double* Y = c.sym ? a.x : a.y;
    const int64_t ld_y = c.sym ? a.ld_x : a.ld_y;
    // this thread's quarter rows of the two operands, for the whole walk
    const int prow = tid >> 2, poff = (tid & 3) * kPer;
    const int64_t gi = c.i0 + prow, gj = c.j0 + prow;
    const bool live_a = gi < a.Sx && st_i[prow * kCrossStat + 3] != 2.0;
    const bool live_b = !c.diag && gj < c.Sy && st_j[prow * kCrossStat + 3] != 2.0;
    const double mu_a = st_i[prow * kCrossStat], mu_b = st_j[prow * kCrossStat];
    const double* row_a = a.x + (live_a ? gi * a.ld_x : 0);
    const double* row_b = Y + (live_b ? gj * ld_y : 0);
    const bool vec_a = ((reinterpret_cast<uintptr_t>(a.x) | (uintptr_t)(a.ld_x * 8)) & 15) == 0;
    const bool vec_b = ((reinterpret_cast<uintptr_t>(Y) | (uintptr_t)(ld_y * 8)) & 15) == 0;
    double* stage_a = lds + prow * kStr + poff;
    double* stage_b = lds + 2 * kOpBuf + prow * kStr + poff;
    // this lane's MFMA operand reads: A[row l & 15][k l >> 4], rows of B likewise
    const double* read_a = lds + (wr * 32 + (lane & 15)) * kStr + (lane >> 4);
    const double* read_b = lds + (c.diag ? 0 : 2 * kOpBuf) + (wc * 32 + (lane & 15)) * kStr + (lane >> 4);

    const int64_t seg_lo = p.split ? blockIdx.y : 0, seg_hi = p.split ? seg_lo + 1 : p.nseg;
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    d4 tot[2][2] = {{zero, zero}, {zero, zero}};
    for (int64_t seg = seg_lo; seg < seg_hi; seg++) {
        const int64_t t_lo = seg * kCrossSplit;
        const int64_t t_hi = t_lo + kCrossSplit < T ? t_lo + kCrossSplit : T;
        const int64_t nch = (t_hi - t_lo + kKC - 1) / kKC;
        d4 run[2][2] = {{zero, zero}, {zero, zero}};
        double va[kPer], vb[kPer];
        load_piece(row_a, live_a, vec_a, t_lo + poff, T, va);
        if (!c.diag) load_piece(row_b, live_b, vec_b, t_lo + poff, T, vb);
        store_piece(stage_a, va, mu_a, live_a, t_lo + poff, T);
        if (!c.diag) store_piece(stage_b, vb, mu_b, live_b, t_lo + poff, T);
        __syncthreads();
        for (int64_t ch = 0; ch < nch; ch++) {
            const int cur = (int)(ch & 1);
            const bool more = ch + 1 < nch;   // uniform
            const int64_t tn = t_lo + (ch + 1) * kKC + poff;
            if (more) {
                load_piece(row_a, live_a, vec_a, tn, T, va);
                if (!c.diag) load_piece(row_b, live_b, vec_b, tn, T, vb);
            }
            const double* ra = read_a + cur * kOpBuf;
            const double* rb = read_b + cur * kOpBuf;
#pragma unroll
            for (int kk = 0; kk < kKC; kk += 4) {
                const double a0 = ra[kk], a1 = ra[16 * kStr + kk];
                const double b0 = rb[kk], b1 = rb[16 * kStr + kk];
                run[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, run[0][0], 0, 0, 0);
                run[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, run[0][1], 0, 0, 0);
                run[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, run[1][0], 0, 0, 0);
                run[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, run[1][1], 0, 0, 0);
            }
            if (more) {
                store_piece(stage_a + (cur ^ 1) * kOpBuf, va, mu_a, live_a, tn, T);
                if (!c.diag) store_piece(stage_b + (cur ^ 1) * kOpBuf, vb, mu_b, live_b, tn, T);
            }
            __syncthreads();   // the other stage is written, this one is read: both free for the next turn
        }
#pragma unroll
        for (int bi = 0; bi < 2; bi++)
#pragma unroll
            for (int bj = 0; bj < 2; bj++) tot[bi][bj] += run[bi][bj];
    }

    // C/D map of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
    double* Ct = lds;   // every stage read is behind the last barrier
#pragma unroll
    for (int bi = 0; bi < 2; bi++)
#pragma unroll
        for (int bj = 0; bj < 2; bj++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++)
                Ct[(wr * 32 + bi * 16 + (lane >> 4) + 4 * reg) * kCtPitch + wc * 32 + bj * 16 + (lane & 15)] =
                    tot[bi][bj][reg];
    __syncthreads();
    if (p.split) {
        double* dst = part + ((int64_t)blockIdx.y * p.tiles + c.tile) * kTileElems;
        for (int idx = tid; idx < kTileElems; idx += kGramThreads) dst[idx] = Ct[(idx / kCT) * kCtPitch + idx % kCT];
        return;
    }
    cross_epilogue(a, c, Ct, st_i, st_j);
}

// split plan: the segments' partials of a tile in ascending order, then the epilogue
__global__ __launch_bounds__(kGramThreads) void cross_finalise_kernel(CrossArgs a, CrossPlan p,
                                                                     const double* __restrict__ sx,
                                                                     const double* __restrict__ sy,
                                                                     const double* __restrict__ part) {
    __shared__ double Ct[kCtSize];
    __shared__ double st_i[kCT * kCrossStat], st_j[kCT * kCrossStat];
    const TileCtx c = tile_ctx(a, p);
    load_stats(a, c, sx, sy, st_i, st_j);
    for (int idx = threadIdx.x; idx < kTileElems; idx += kGramThreads) {
        double tot = 0.0;
        for (int64_t seg = 0; seg < p.nseg; seg++) tot += part[(seg * p.tiles + c.tile) * kTileElems + idx];
        Ct[(idx / kCT) * kCtPitch + idx % kCT] = tot;
    }
    __syncthreads();
    cross_epilogue(a, c, Ct, st_i, st_j);
}

}  // namespace

CrossPlan cross_plan(int64_t Sx, int64_t Sy, int64_t T, bool symmetric) {
    CrossPlan p;
    p.ti = (Sx + kCT - 1) / kCT;
    p.tj = symmetric ? p.ti : (Sy + kCT - 1) / kCT;
    p.tiles = symmetric ? p.ti * (p.ti + 1) / 2 : p.ti * p.tj;
    p.nseg = (T + kCrossSplit - 1) / kCrossSplit;
    const int64_t room = ((int64_t)STS_CROSS_SPLIT_MB << 20) / (int64_t)(kTileElems * sizeof(double));
    p.split = p.nseg > 1 && p.tiles < STS_CROSS_SPLIT_TILES && p.tiles * p.nseg <= room;
    p.scratch_doubles = (size_t)(Sx + (symmetric ? 0 : Sy)) * kCrossStat +
                        (p.split ? (size_t)(p.tiles * p.nseg) * kTileElems : 0);
    return p;
}

hipError_t launch_cross(const CrossArgs& a, hipStream_t st) {
    const bool sym = a.y == nullptr;
    const int64_t Sy = sym ? a.Sx : a.Sy;
    const CrossPlan p = cross_plan(a.Sx, Sy, a.T, sym);
    double* sx = a.scratch;
    double* sy = sym ? sx : sx + a.Sx * kCrossStat;
    double* part = sy + Sy * kCrossStat;
    hipLaunchKernelGGL(cross_prep_kernel, dim3((unsigned)a.Sx), dim3(kPrepThreads), 0, st, a.x, a.T, a.ld_x, sx, a.mean_x);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (!sym) {
        hipLaunchKernelGGL(cross_prep_kernel, dim3((unsigned)Sy), dim3(kPrepThreads), 0, st, a.y, a.T, a.ld_y, sy, a.mean_y);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(cross_gram_kernel, dim3((unsigned)p.tiles, (unsigned)(p.split ? p.nseg : 1)), dim3(kGramThreads), 0, st,
                       a, p, sx, sy, part);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (p.split) {
        hipLaunchKernelGGL(cross_finalise_kernel, dim3((unsigned)p.tiles), dim3(kGramThreads), 0, st, a, p, sx, sy, part);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace sts
