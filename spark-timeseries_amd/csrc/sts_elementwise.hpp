// sts_elementwise.hpp -- the loop and the launcher of the element-parallel ("output-driven")
// kernels of sts_stream.hip, sts_transforms.hip and sts_index.hip.  A workgroup of kThreads threads
// owns PER * kThreads consecutive output elements of a panel of `rows` rows of `row_len` elements;
// thread i takes elements i, i + kThreads, ... of them, so every load and store of a wave is
// coalesced along the row, and each element's (row, column) comes from split().
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace sts {

constexpr int kThreads = 256;
constexpr int kPerThread = 8;
constexpr int64_t kChunk = (int64_t)kThreads * kPerThread;

// split a logical index g in [0, S*T) into (s, t) with a double reciprocal + fix-up
__device__ __forceinline__ void split(int64_t g, int64_t T, double rT, int64_t& s, int64_t& t) {
    s = (int64_t)((double)g * rT);
    int64_t b = s * T;
    if (b > g) { s--; b -= T; }
    else if (b + T <= g) { s++; b += T; }
    t = g - b;
}

// f(s, t) -- or f(s, t, g), g = s * row_len + t, for a packed output -- for this thread's PER
// elements of the rows x row_len panel, r_row_len = 1.0 / row_len; the launch is
// launch_elementwise(kernel, rows * row_len, PER * kThreads, ...).  f captures by value: the kernel's
// __restrict__ pointers then reach the loop as they are, and the code is the hand-written loop's
// instruction for instruction (by reference it carried a few more address instructions).
template <int PER = kPerThread, int UNROLL = PER, class F>
__device__ __forceinline__ void for_each_out(int64_t rows, int64_t row_len, double r_row_len, F&& f) {
    const int64_t n = rows * row_len;
    const int64_t g0 = (int64_t)blockIdx.x * (PER * kThreads) + threadIdx.x;
#pragma unroll UNROLL
    for (int j = 0; j < PER; j++) {
        const int64_t g = g0 + (int64_t)j * kThreads;
        if (g >= n) break;
        int64_t s, t;
        split(g, row_len, r_row_len, s, t);
        if constexpr (std::is_invocable_v<F&, int64_t, int64_t, int64_t>) f(s, t, g);
        else f(s, t);
    }
}

// kernel<<<ceil(n / per_block), kThreads, 0, st>>>(args...); nothing to do for n <= 0
template <class K, class... A>
hipError_t launch_elementwise(K kernel, int64_t n, int64_t per_block, hipStream_t st, A... args) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = (n + per_block - 1) / per_block;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, args...);
    return hipGetLastError();
}

}  // namespace sts
