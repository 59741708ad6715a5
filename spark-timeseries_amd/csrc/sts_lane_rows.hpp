// sts_lane_rows.hpp -- the chunk loop and the launcher of the lane-per-series kernels of
// sts_ewma_fit.hip, sts_garch.hip, sts_arima.hip, sts_recur.hip and sts_sample.hip.  A workgroup of
// one 64-lane wave owns SPW consecutive series.  It moves their SPW x CH block through an LDS tile
// chunk by chunk -- load instruction i of a lane covers element e = (i * 64 + lane) * EPL of the
// block, row e / CH, column e % CH, so an instruction reads 64 * EPL consecutive steps of a series --
// with the next chunk's loads in flight while the current chunk runs; then lane r < SPW walks row
// r of the tile in the reference's sequential order.  Two forms:
//   stream_rows   pass: load only, the rows chosen by a ballot mask (ewma_fit_kernel, arima_css_kernel);
//   map_rows      map: load, walk in place, store back (recur_kernel, garch_effects_kernel,
//                 arima_effects_kernel).
//
// The staging rule: a lane stores what it fetched into the tile UNCONDITIONALLY.  Every (row, column)
// of the element map lies inside the tile, so the store is in bounds; a slot of an unwanted row, of
// a row past the panel (row >= ns) or of a column past the chunk (col >= len) holds the 0.0 its
// fetch put in place of a load, and is never read: a walking lane reads only columns < len of its
// own row, which is live (and wanted), and the store half writes only rows < ns, columns < len.
// Guarding the staging store as well would be as correct and cost a compare per instruction.
//
// Three kernels of the family keep this loop written out, because over the shared one they ran
// slower than before: garch_fit_kernel (pass form, + 1.3 %), arima_forecast_kernel
// (map form with T + n_future output steps, + 1.5 %), garch_sample_kernel (the store half, + 0.9 %).
//
// Not built on this loop, on purpose: stats_fast_kernel (sts_stream.hip: line-aligned chunks with a
// per-row offset, clamped loads and reciprocal tables -- a loop of its own), garch_tail_kernel and
// recur_row_kernel (one wave per series, or several lanes per series), and everything in
// sts_tile.hip, sts_seg.hip, sts_short.hip and sts_ar*.hip (workgroups of several waves).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace sts {

// The block's geometry.  EPL: elements per lane per instruction (2: 16-byte accesses).  The row
// pitch CH + EPL skews consecutive rows across the LDS banks and, for EPL = 2, stays even, so the
// 16-byte LDS accesses are aligned.
template <int SPW, int CH, int EPL = 1>
struct LaneRows {
    static_assert(SPW >= 1 && SPW <= 64, "a lane per series");
    static_assert(EPL == 1 || EPL == 2, "8- or 16-byte accesses");
    static_assert(SPW * CH % (64 * EPL) == 0 && (EPL == 2 ? CH % 2 == 0 : (CH % 64 == 0 || 64 % CH == 0)),
                  "chunk shape: whole load instructions, whole rows or whole fractions of a row each");
    static constexpr int kRow = CH + EPL;               // row pitch of the tile
    static constexpr int kTile = SPW * kRow;            // doubles of LDS
    static constexpr int NLD = SPW * CH / (64 * EPL);   // load (and store) instructions per chunk per lane
    using Vec = std::conditional_t<EPL == 2, double2, double>;
    static __device__ __forceinline__ void at(int i, int lane, int& row, int& col) {
        const int e = (i * 64 + lane) * EPL;
        row = e / CH;
        col = e % CH;
    }
};

// A workgroup's place in the panel of S series: its first series s0, this lane's series sl (lanes
// < SPW), whether that series exists, and the number ns of the block's rows inside the panel.
template <int SPW>
struct LaneBlock {
    int lane, ns;
    int64_t s0, sl;
    bool live;
    __device__ __forceinline__ explicit LaneBlock(int64_t S) {
        lane = threadIdx.x;
        s0 = (int64_t)blockIdx.x * SPW;
        sl = s0 + lane;
        live = (SPW == 64 || lane < SPW) && sl < S;   // a wave has 64 lanes
        ns = (S - s0 < SPW) ? (int)(S - s0) : SPW;
    }
};

// Pass form.  base: the block's first row; the rows r < ns with bit r of `want` set stream through
// `tile` (LaneRows<SPW, CH>::kTile doubles) in chunks of CH steps, and every lane with `run` calls
// f(myrow, tc, len) per chunk: its row's steps [tc, tc + len) at myrow[0 .. len).  A running lane's
// row must be wanted.  f captures by reference: the walk carries per-lane state across chunks.
template <int SPW, int CH, class F>
__device__ __forceinline__ void stream_rows(double* tile, const double* base, int64_t ld, int64_t T, int ns,
                                            unsigned long long want, bool run, F&& f) {
    using G = LaneRows<SPW, CH>;
    const int lane = threadIdx.x;
    double pre[G::NLD];
    auto fetch = [&](int64_t tc) {
#pragma unroll
        for (int i = 0; i < G::NLD; i++) {
            int row, col;
            G::at(i, lane, row, col);
            const bool want_row = row < ns && ((want >> row) & 1ull);
            pre[i] = (want_row && tc + col < T) ? base[row * ld + tc + col] : 0.0;
        }
    };
    fetch(0);
    for (int64_t tc = 0; tc < T; tc += CH) {
        const int len = (T - tc < CH) ? (int)(T - tc) : CH;
#pragma unroll
        for (int i = 0; i < G::NLD; i++) {
            int row, col;
            G::at(i, lane, row, col);
            tile[row * G::kRow + col] = pre[i];
        }
        if (tc + CH < T) fetch(tc + CH);   // next chunk in flight during this one
        __syncthreads();
        if (run) f(tile + lane * G::kRow, tc, len);
        __syncthreads();
    }
}

// Map form.  in / out: the panels; s0: the block's first series.  Steps [0, T) of the rows r < ns
// are loaded, every lane with `run` calls f(myrow, tc, len) per chunk and leaves its outputs in
// myrow[0 .. len), and the tile's rows < ns, columns < len go to `out`.  in == out (with ld_in ==
// ld_out) is in place: chunks do not overlap and each is loaded before it is stored.  EPL = 2 needs
// 16-byte aligned rows on both sides (even ld, aligned bases) and a 16-byte aligned tile; a row's odd
// last step moves as a scalar.  An element's address is in + (s0 + row) * ld_in + ..., formed per
// instruction: with in + s0 * ld_in formed once the 8-byte AR recurrences lost their second wave.
template <int SPW, int CH, int EPL = 1, class F>
__device__ __forceinline__ void map_rows(double* tile, const double* in, int64_t ld_in, double* out, int64_t ld_out,
                                         int64_t T, int64_t s0, int ns, bool run, F&& f) {
    using G = LaneRows<SPW, CH, EPL>;
    const int lane = threadIdx.x;
    typename G::Vec pre[G::NLD];
    auto fetch = [&](int64_t tc) {
        const int len = (T - tc < CH) ? (int)(T - tc) : CH;
#pragma unroll
        for (int i = 0; i < G::NLD; i++) {
            int row, col;
            G::at(i, lane, row, col);
            const double* src = in + (s0 + row) * ld_in + tc + col;
            if constexpr (EPL == 2) {
                if (row < ns && col + 1 < len) {
                    pre[i] = *reinterpret_cast<const double2*>(src);
                } else {
                    pre[i].x = (row < ns && col < len) ? src[0] : 0.0;
                    pre[i].y = 0.0;
                }
            } else {
                pre[i] = (row < ns && col < len) ? src[0] : 0.0;
            }
        }
    };
    fetch(0);
    for (int64_t tc = 0; tc < T; tc += CH) {
        const int len = (T - tc < CH) ? (int)(T - tc) : CH;
#pragma unroll
        for (int i = 0; i < G::NLD; i++) {
            int row, col;
            G::at(i, lane, row, col);
            *reinterpret_cast<typename G::Vec*>(&tile[row * G::kRow + col]) = pre[i];
        }
        if (tc + CH < T) fetch(tc + CH);   // next chunk in flight during this one
        __syncthreads();
        if (run) f(tile + lane * G::kRow, tc, len);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < G::NLD; i++) {
            int row, col;
            G::at(i, lane, row, col);
            double* d = out + (s0 + row) * ld_out + tc + col;
            const double* t = &tile[row * G::kRow + col];
            if constexpr (EPL == 2) {
                if (row < ns && col + 1 < len) *reinterpret_cast<double2*>(d) = *reinterpret_cast<const double2*>(t);
                else if (row < ns && col < len) d[0] = t[0];
            } else {
                if (row < ns && col < len) d[0] = t[0];
            }
        }
        __syncthreads();
    }
}

// kernel<<<ceil(S / SPW), 64, 0, st>>>(args...): SPW is the constant the kernel is instantiated
// with; nothing to do for S <= 0
template <class K, class... A>
hipError_t launch_lane_rows(K kernel, int64_t S, int SPW, hipStream_t st, A... args) {
    if (S <= 0) return hipSuccess;
    const int64_t blocks = (S + SPW - 1) / SPW;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64), 0, st, args...);
    return hipGetLastError();
}

}  // namespace sts
