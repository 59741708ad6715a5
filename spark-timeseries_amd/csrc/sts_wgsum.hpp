// sts_wgsum.hpp -- workgroup-wide sums of the one-workgroup-per-series kernels (sts_stattests.hip,
// sts_regress.hip).  NT = 64 is one wave and uses shuffles only, so several such "workgroups" may
// share a real one (sts_regress.hip's hot kernel); NT > 64 goes through `red` with barriers.
#pragma once
#include <hip/hip_runtime.h>

namespace sts {

// Every thread gets the same bits (a butterfly of commutative additions), so branches on a
// reduced value are uniform.
template <int NT>
__device__ __forceinline__ double bsum(double v, double* red) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    if constexpr (NT > 64) {
        __syncthreads();   // red[] free again
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = red[0];
#pragma unroll
        for (int i = 1; i < NT / 64; i++) v += red[i];
    }
    return v;
}

// The first `live` (uniform) of N sums at once: their butterflies interleave, so a wave waits for
// one chain of shuffles, not `live` of them (red: N x 4 doubles when NT > 64)
template <int NT, int N>
__device__ __forceinline__ void bsum_many(double (&v)[N], int live, double* red) {
#pragma unroll
    for (int o = 32; o; o >>= 1)
#pragma unroll
        for (int c = 0; c < N; c++)
            if (c < live) v[c] += __shfl_xor(v[c], o, 64);
    if constexpr (NT > 64) {
        __syncthreads();   // red[] free again
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int c = 0; c < N; c++)
                if (c < live) red[c * 4 + (threadIdx.x >> 6)] = v[c];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < N; c++)
            if (c < live) {
                double t = red[c * 4];
#pragma unroll
                for (int i = 1; i < NT / 64; i++) t += red[c * 4 + i];
                v[c] = t;
            }
    }
}

}  // namespace sts
