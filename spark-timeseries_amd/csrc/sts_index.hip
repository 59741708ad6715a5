// sts_index.hip -- the kernels of include/sts_index.h: date-time index lookups (the arithmetic is
// sts_index.hpp's, shared with the host) and the rebasing copies
//   toMillisArray / locAtDateTime         S/DateTimeIndex.scala:143-162, 212-222
//   rebase, uniform -> uniform            S/TimeSeriesUtils.scala:100-129
//   rebase by lookup                      S/TimeSeriesUtils.scala:131-203 (its documented meaning)
//   timeSeriesRDD(targetIndex, series)    S/TimeSeriesRDD.scala:446-482
// The copies are output-driven like sts_transforms.hip's: threads map to consecutive output steps,
// every output element (s, j < T_out) is written exactly once by a coalesced store, nothing else is
// written, and an input element is read only where the rule says it is copied.  No arithmetic touches
// a value: doubles travel as 64-bit words, so every payload survives.
#include "sts_elementwise.hpp"
#include "sts_internal.hpp"
#include "sts_index.hpp"

#include <hip/hip_runtime.h>

namespace sts {
namespace {

// rebase_map: a workgroup owns kMapCols map entries (one per thread) and kMapRows series
constexpr int kMapCols = kThreads;
constexpr int kMapRows = 64;
// rebase_map for rows of up to kMapFlat columns: the whole map in LDS (8 KB), kMapFlatPer elements per thread
constexpr int kMapFlat = 1024;
constexpr int kMapFlatPer = 16;

__global__ __launch_bounds__(kThreads) void instants_kernel(ix::Uniform u, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < u.periods) out[i] = ix::instant_at(u, i);
}

__global__ __launch_bounds__(kThreads) void locs_uniform_kernel(const int64_t* __restrict__ millis, int64_t n,
                                                                ix::Uniform u, int64_t* __restrict__ loc) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) loc[i] = ix::loc_at(u, millis[i]);
}

__global__ __launch_bounds__(kThreads) void locs_irregular_kernel(const int64_t* __restrict__ millis, int64_t n,
                                                                  const int64_t* __restrict__ instants,
                                                                  int64_t n_instants, int64_t* __restrict__ loc) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) loc[i] = ix::loc_irregular(instants, n_instants, millis[i]);
}

// out(s, j) = in(s, j + shift) where 0 <= j + shift < T_in, else dflt; one element per thread step
__global__ __launch_bounds__(kThreads) void shift_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                         int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                                                         int64_t ld_out, double rT, int64_t shift, uint64_t dflt) {
    for_each_out(S, T_out, rT, [=](int64_t s, int64_t j) {
        const int64_t m = j + shift;
        out[s * ld_out + j] = (m >= 0 && m < T_in) ? in[s * ld_in + m] : dflt;
    });
}

// (A 16-byte form for even pitches and even shifts was measured and dropped: 1.01-1.05 x the time of
// this one at 1 M x 390)

// out(s, j) = in(s, map[j]) where 0 <= map[j] < T_in, else dflt.  A workgroup owns kMapCols
// consecutive columns and kMapRows series: each thread loads the map entry of its column once and
// reuses it for every series of the tile, so the map's 8 bytes per column are paid once per kMapRows
// series (1/8 of a byte per element moved), and a row of the tile is one contiguous store of up to
// 2 KB.  An absent column is a predicated load, not a branch: lanes with and without a source run
// the same loop.
__global__ __launch_bounds__(kThreads) void map_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                       int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                                                       int64_t ld_out, int64_t col_tiles, double r_col_tiles,
                                                       const int64_t* __restrict__ map, uint64_t dflt) {
    int64_t row_tile, col_tile;   // blockIdx.x = row_tile * col_tiles + col_tile: one grid dimension, no series limit
    split((int64_t)blockIdx.x, col_tiles, r_col_tiles, row_tile, col_tile);
    const int64_t j = col_tile * kMapCols + threadIdx.x;
    if (j >= T_out) return;
    const int64_t m = map[j];
    const bool hit = m >= 0 && m < T_in;
    const int64_t s0 = row_tile * kMapRows;
    const int64_t s1 = s0 + kMapRows < S ? s0 + kMapRows : S;
    const uint64_t* x = in + (hit ? m : 0);
    uint64_t* y = out + j;
#pragma unroll 8
    for (int64_t s = s0; s < s1; s++) y[s * ld_out] = hit ? x[s * ld_in] : dflt;
}

// The same rule for short rows (T_out <= kMapFlat): a tile of 256 columns leaves lanes idle when a row
// is not a multiple of it (390 columns: 24 % of them), so here the workgroup keeps the WHOLE map in
// LDS, loaded once, and walks kMapFlatPer * 256 consecutive output elements as the other copies do:
// every lane is busy and the map is reused across the at least four series the stretch covers.
__global__ __launch_bounds__(kThreads) void map_flat_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                            int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                                                            int64_t ld_out, double rT, const int64_t* __restrict__ map,
                                                            uint64_t dflt) {
    __shared__ int64_t sh_map[kMapFlat];
    for (int64_t j = threadIdx.x; j < T_out; j += kThreads) {
        const int64_t m = map[j];
        sh_map[j] = (m >= 0 && m < T_in) ? m : -1;
    }
    __syncthreads();
    for_each_out<kMapFlatPer, 8>(S, T_out, rT, [=](int64_t s, int64_t j) {
        const int64_t m = sh_map[j];
        out[s * ld_out + j] = m >= 0 ? in[s * ld_in + m] : dflt;
    });
}

// out(s, j) = values[offsets[s] + j + start_loc[s]] where 0 <= j + start_loc[s] < offsets[s + 1] -
// offsets[s], else dflt.  The three int64 of a series are shared by the T_out threads of its row
// (one cache line per row).  start_loc is clamped so j + start_loc cannot wrap.
__global__ __launch_bounds__(kThreads) void align_kernel(const uint64_t* __restrict__ values,
                                                         const int64_t* __restrict__ offsets,
                                                         const int64_t* __restrict__ start_loc, int64_t S, int64_t T_out,
                                                         uint64_t* __restrict__ out, int64_t ld_out, double rT,
                                                         uint64_t dflt) {
    for_each_out(S, T_out, rT, [=](int64_t s, int64_t j) {
        const int64_t o = offsets[s], len = offsets[s + 1] - o;
        int64_t sl = start_loc[s];
        sl = sl > ix::kMaxInstant ? ix::kMaxInstant : (sl < -ix::kMaxInstant ? -ix::kMaxInstant : sl);
        const int64_t m = j + sl;
        out[s * ld_out + j] = (m >= 0 && m < len) ? values[o + m] : dflt;
    });
}

inline uint64_t bits_of(double v) {
    uint64_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}

}  // namespace

hipError_t launch_index_instants(const ix::Uniform& u, int64_t* out, hipStream_t st) {
    return launch_elementwise(instants_kernel, u.periods, kThreads, st, u, out);
}

hipError_t launch_index_locs(const int64_t* millis, int64_t n, const ix::Uniform* u, const int64_t* instants,
                             int64_t n_instants, int64_t* loc, hipStream_t st) {
    if (u) return launch_elementwise(locs_uniform_kernel, n, kThreads, st, millis, n, *u, loc);
    return launch_elementwise(locs_irregular_kernel, n, kThreads, st, millis, n, instants, n_instants, loc);
}

hipError_t launch_rebase_shift(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                               int64_t ld_out, int64_t shift, double dflt, hipStream_t st) {
    if (S <= 0 || T_out <= 0) return hipSuccess;
    // disjoint ranges: every shift at or past an end behaves like the nearest one, and j + shift cannot wrap
    if (shift > T_in) shift = T_in;
    if (shift < -T_out) shift = -T_out;
    return launch_elementwise(shift_kernel, S * T_out, kChunk, st, reinterpret_cast<const uint64_t*>(in),
                              reinterpret_cast<uint64_t*>(out), S, T_in, T_out, ld_in, ld_out, 1.0 / (double)T_out, shift,
                              bits_of(dflt));
}

hipError_t launch_rebase_map(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                             int64_t ld_out, const int64_t* map, double dflt, hipStream_t st) {
    if (S <= 0 || T_out <= 0) return hipSuccess;
    const uint64_t* x = reinterpret_cast<const uint64_t*>(in);
    uint64_t* y = reinterpret_cast<uint64_t*>(out);
    if (T_out <= kMapFlat)
        return launch_elementwise(map_flat_kernel, S * T_out, (int64_t)kMapFlatPer * kThreads, st, x, y, S, T_in, T_out,
                                  ld_in, ld_out, 1.0 / (double)T_out, map, bits_of(dflt));
    // one workgroup per tile
    const int64_t col_tiles = (T_out + kMapCols - 1) / kMapCols, row_tiles = (S + kMapRows - 1) / kMapRows;
    return launch_elementwise(map_kernel, col_tiles * row_tiles, 1, st, x, y, S, T_in, T_out, ld_in, ld_out, col_tiles,
                              1.0 / (double)col_tiles, map, bits_of(dflt));
}

hipError_t launch_align_uniform(const double* values, const int64_t* offsets, const int64_t* start_loc, int64_t S,
                                int64_t T_out, double* out, int64_t ld_out, double dflt, hipStream_t st) {
    if (S <= 0 || T_out <= 0) return hipSuccess;
    return launch_elementwise(align_kernel, S * T_out, kChunk, st, reinterpret_cast<const uint64_t*>(values), offsets,
                              start_loc, S, T_out, reinterpret_cast<uint64_t*>(out), ld_out, 1.0 / (double)T_out,
                              bits_of(dflt));
}

}  // namespace sts
