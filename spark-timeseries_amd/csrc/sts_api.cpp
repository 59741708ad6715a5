// sts_api.cpp -- the C ABI (include/sts.h): argument validation with the reference's
// error semantics, stream/workspace handling, kernel dispatch, host-buffer staging.
//
// Reentrancy: no mutable global state after first use except the per-device
// memory-pool setup (guarded by std::call_once); every call runs on the caller's
// stream (NULL -> hipStreamPerThread) and allocates its scratch stream-ordered
// (hipMallocAsync / hipFreeAsync), so Spark's N executor threads can call
// concurrently.  Errors are reported through a thread-local message.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "sts_internal.hpp"
#include "sts_factor_basis.hpp"
#include "sts_index.hpp"

namespace {

thread_local std::string g_err;

int fail(int status, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return status;
}

int hip_fail(hipError_t e, const char* where) {
    return fail(STS_ERR_HIP, "%s: %s", where, hipGetErrorString(e));
}

#define HIP_TRY(call, where)                       \
    do {                                           \
        hipError_t e_ = (call);                    \
        if (e_ != hipSuccess) return hip_fail(e_, where); \
    } while (0)

hipStream_t as_stream(void* s) { return s ? reinterpret_cast<hipStream_t>(s) : hipStreamPerThread; }

std::once_flag g_pool_once[64];

// validate-only mode (sts::validate_call): every entry point validates its arguments
// before its first device action, ensure_device(), which then stops the call
thread_local bool g_validate_only = false;
constexpr int kValidated = -1000;

int ensure_device() {
    if (g_validate_only) return kValidated;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    int n = 0;
    e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail(STS_ERR_NO_DEVICE, "no HIP device visible");
    if (dev >= 0 && dev < 64) {
        std::call_once(g_pool_once[dev], [dev] {
            hipMemPool_t pool;
            if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) {
                uint64_t thr = UINT64_MAX;
                (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr);
            }
        });
    }
    return STS_OK;
}

// stream-ordered scratch
struct Scratch {
    void* p = nullptr;
    hipStream_t st;
    explicit Scratch(hipStream_t s) : st(s) {}
    hipError_t alloc(size_t bytes) { return hipMallocAsync(&p, bytes ? bytes : 16, st); }
    ~Scratch() {
        if (p) (void)hipFreeAsync(p, st);
    }
};

int check_panel(const void* in, int64_t S, int64_t T, int64_t ld, const char* name) {
    if (S < 0 || T < 0) return fail(STS_ERR_BAD_ARG, "%s: negative panel shape (S=%lld, T=%lld)", name,
                                    (long long)S, (long long)T);
    if (T > 0x7fffffffLL) return fail(STS_ERR_BAD_ARG, "%s: T=%lld exceeds the reference's Int index range",
                                      name, (long long)T);
    if (ld < T) return fail(STS_ERR_BAD_ARG, "%s: leading dimension %lld < T=%lld", name, (long long)ld,
                            (long long)T);
    if (S * T > 0 && !in) return fail(STS_ERR_BAD_ARG, "%s: null panel pointer", name);
    return STS_OK;
}

// The calling thread's host-mapped status array for calls without a caller err array (round 6):
// the kernels write it over PCIe and the call reads it after its stream synchronize, instead of a
// stream-ordered allocation + memset + D2H copy (a one-series fill: 35 -> ~15 us,
// tools/percall_parts.py).  Grown on demand up to kMappedErrMax entries, freed with the thread.
constexpr int64_t kMappedErrMax = 1 << 16;
struct MappedErr {
    int32_t* host = nullptr;
    int32_t* dev = nullptr;
    int64_t cap = 0;
    int32_t* get(int64_t n, int32_t** devp) {
        if (n > cap) {
            if (host) (void)hipHostFree(host);
            host = dev = nullptr;
            cap = 0;
            void* p = nullptr;
            if (hipHostMalloc(&p, (size_t)n * sizeof(int32_t), hipHostMallocMapped | hipHostMallocPortable) != hipSuccess)
                return nullptr;
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
                (void)hipHostFree(p);
                return nullptr;
            }
            host = static_cast<int32_t*>(p);
            dev = static_cast<int32_t*>(d);
            cap = n;
        }
        *devp = dev;
        return host;
    }
    ~MappedErr() {
        if (host) (void)hipHostFree(host);
    }
};
thread_local MappedErr t_mapped_err;

// err handling: caller array (async) or internal buffer checked synchronously
struct ErrSink {
    int32_t* dev = nullptr;
    int32_t* mapped = nullptr;   // host view of dev when dev is the thread's mapped array
    bool owned = false;
    Scratch scratch;
    int64_t S;
    ErrSink(int32_t* user, int64_t S_, hipStream_t st) : dev(user), scratch(st), S(S_) {}
    // zero = false: the caller guarantees that the kernel writes every entry, or zeroes it
    // itself (run_tile)
    int prepare(bool zero = true) {
        if (!dev) {
            owned = true;
            if (S > 0 && S <= kMappedErrMax) mapped = t_mapped_err.get(S, &dev);
            if (mapped) {
                std::memset(mapped, 0, (size_t)S * sizeof(int32_t));   // before any launch of this call
                return STS_OK;
            }
            hipError_t e = scratch.alloc((size_t)(S > 0 ? S : 1) * sizeof(int32_t));
            if (e != hipSuccess) return hip_fail(e, "hipMallocAsync(err)");
            dev = static_cast<int32_t*>(scratch.p);
        }
        if (S > 0 && zero) {
            hipError_t e = hipMemsetAsync(dev, 0, (size_t)S * sizeof(int32_t), scratch.st);
            if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(err)");
        }
        return STS_OK;
    }
    // a call that returns early (a failed launch) may still have kernels in flight that write
    // the thread's mapped array: wait for them before the next call on this thread reuses it
    ~ErrSink() {
        if (mapped && !finished) (void)hipStreamSynchronize(scratch.st);
    }
    bool finished = false;
    // for the internal buffer: wait and turn the first failing series into a status
    int finish(const char* what) {
        finished = true;
        if (!owned || S == 0) return STS_OK;
        if (mapped) {
            const hipError_t e = hipStreamSynchronize(scratch.st);
            if (e != hipSuccess) return hip_fail(e, what);
            return sts::series_status(mapped, S, what);
        }
        std::vector<int32_t> h((size_t)S);
        hipError_t e = hipMemcpyAsync(h.data(), dev, (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost, scratch.st);
        if (e == hipSuccess) e = hipStreamSynchronize(scratch.st);
        if (e != hipSuccess) return hip_fail(e, what);
        return sts::series_status(h.data(), S, what);
    }
};

int method_ok(int method, bool allow_none, const char* name) {
    if (method < (allow_none ? STS_FILL_NONE : STS_FILL_LINEAR) || method > STS_FILL_SPLINE)
        return fail(STS_ERR_UNSUPPORTED_METHOD, "%s: unsupported fill method %d", name, method);
    return STS_OK;
}

int tile_width(int64_t T) { return T <= 512 ? 512 : 4096; }
constexpr int64_t kTilesPerChunk = 16;  // tiles per workgroup (prefetch pipeline depth 1)
// without the ACF (fill only, fill + lag matrix: C5) one tile per workgroup: the denser sweep
// beats the prefetch pipeline (C5: 1.527-1.534 vs 1.647-1.659 ms same box, and 1.83 vs 2.03-2.07 on
// a box in its slow state, profiles/r04_v11_ab_c5_tpc.jsonl; fill only on the C3 shard 31.2-31.6 vs
// 33.3 ms, r04_v2_ab_tiles_per_chunk.jsonl)
constexpr int64_t kTilesPerChunkFill = 1;

// Measurement hook (bench.py): HIP events recorded on the launch stream around every
// tile-kernel launch of this thread while profiling is on.
struct ProfileState {
    bool on = false;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
};
thread_local ProfileState g_prof;

void prof_mark(hipStream_t st) {
    if (!g_prof.on) return;
    if (g_prof.used == g_prof.pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        g_prof.pool.push_back(e);
    }
    (void)hipEventRecord(g_prof.pool[g_prof.used++], st);
}

// a kernel launch bracketed by profiling events (bench.py's per-kernel timing)
template <typename F>
hipError_t timed(hipStream_t st, F&& launch) {
    prof_mark(st);
    const hipError_t e = launch();
    prof_mark(st);
    return e;
}

// bgtest / bptest / factor_ols: the factors' orthonormal bases (f.k x f.n doubles and aux_doubles more
// each, and a status) go to a stream-ordered scratch, then run(s0, ns) takes the series that read
// them.  One basis for shared factors; per-series factors in chunks of series whose bases fit
// kBasisChunkBytes, so the scratch stays bounded and warm in the caches; none where the kernels
// build each series' basis in LDS (own: one chunk, then).
constexpr size_t kBasisChunkBytes = (size_t)256 << 20;

template <class Run>
int over_factor_bases(sts::FactorBasisArgs& f, int64_t S, bool own, int aux_doubles, hipStream_t st,
                      const char* name, Run run) {
    const size_t nq = (size_t)f.k * (size_t)f.n;
    const size_t per_basis = (nq + (size_t)aux_doubles) * sizeof(double);
    int64_t chunk = 1;
    if (own) chunk = S;
    else if (f.fs != 0) chunk = std::max<int64_t>(1, std::min<int64_t>(S, (int64_t)(kBasisChunkBytes / per_basis)));
    const size_t nbasis = own ? 0 : (size_t)chunk;
    Scratch sc(st);
    HIP_TRY(sc.alloc((per_basis + sizeof(int32_t)) * nbasis), "hipMallocAsync(factor basis)");
    f.basis = static_cast<double*>(sc.p);
    double* end = f.basis + nq * nbasis;
    if (aux_doubles) f.aux = end;
    f.info = reinterpret_cast<int32_t*>(end + (size_t)aux_doubles * nbasis);
    if (f.fs != 0) {
        f.basis_stride = (int64_t)nq;
        f.aux_stride = aux_doubles;
        f.info_stride = 1;
    } else {
        chunk = S;   // the one basis serves every series
    }
    for (int64_t s0 = 0; s0 < S; s0 += chunk) {
        const int64_t ns = std::min<int64_t>(chunk, S - s0);
        if (!own) HIP_TRY(sts::launch_factor_basis(f, s0, f.fs != 0 ? ns : 1, st), name);
        HIP_TRY(timed(st, [&] { return run(s0, ns); }), name);
    }
    return STS_OK;
}

// fillts "spline" (sts_spline.hip): its own kernel, not a tile-kernel method.  err (device,
// S entries) is written for every series.
int run_spline(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int32_t* err,
               hipStream_t st) {
    if (S == 0) return STS_OK;
    if (T == 0) {
        if (err) HIP_TRY(hipMemsetAsync(err, 0, (size_t)S * sizeof(int32_t), st), "hipMemsetAsync(err)");
        return STS_OK;
    }
    const int64_t batch = sts::spline_batch(S, T);
    Scratch sc(st);
    hipError_t e = sc.alloc((size_t)batch * (size_t)T * 2 * sizeof(double));
    if (e != hipSuccess) return hip_fail(e, "hipMallocAsync(spline scratch)");
    e = timed(st, [&] {
        return sts::launch_spline(in, out, S, T, ld_in, ld_out, err, static_cast<double*>(sc.p), batch, st);
    });
    if (e != hipSuccess) return hip_fail(e, "fill (spline)");
    return STS_OK;
}

// fill (+ optional ACF partials / lag matrix) through the tile kernel
// err: zeroed here unless the chosen kernel writes every entry (the seg kernel with one
// segment per series); callers prepare their ErrSink with zero = false.
int run_tile(const double* in, double* out, double* lagmat, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
             int method, int K, double* acf, int max_lag, int inc, int32_t* err, hipStream_t st, const char* name) {
    if (method == STS_FILL_SPLINE) {
        // the spline is not fused: callers compose it (sts_fill_autocorr / _lag_matrix / _diff_ewma)
        if (K > 0 || lagmat) return fail(STS_ERR_BAD_ARG, "%s: spline fill is not fused", name);
        return run_spline(in, out, S, T, ld_in, ld_out, err, st);
    }
    if (S == 0) return STS_OK;
    if (T == 0) {
        if (err) HIP_TRY(hipMemsetAsync(err, 0, (size_t)S * sizeof(int32_t), st), "hipMemsetAsync(err)");
        return STS_OK;
    }
    // short series (T <= 16384: C1, the 10-year daily panels) go to the wave-private
    // segment kernel (2x faster there: one wave per series, no barriers), long ones to the
    // workgroup tile kernel (faster from T = 32768: C3, C5).  The segment kernel needs a
    // 16-B aligned panel, no lag matrix and K <= 60.  In the A/B build STS_TILE_KERNEL=tile|seg
    // forces one (tools/kbench.py, the knob tests).
    const char* force = sts::ab_knob("STS_TILE_KERNEL");
    const bool seg_ok = !lagmat && sts::seg_nt(K) >= 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0 &&
                        (ld_in % 2) == 0 &&
                        (!out || ((reinterpret_cast<uintptr_t>(out) & 15) == 0 && ld_out % 2 == 0)) &&
                        T < 0x7fff0000LL;
    const bool seg = seg_ok && (force ? !std::strcmp(force, "seg") : T <= 16384);
    // STS_TILE_W=2048: 2-wave workgroups on 2048-step tiles for K <= 60 (A/B build only)
    const char* tw_env = (!seg && K > 0 && K <= 60 && !lagmat) ? sts::ab_knob("STS_TILE_W") : nullptr;
    const int tw = seg ? sts::kSegW : (K > 0) ? (tw_env && std::atoi(tw_env) == 2048 ? 2048 : 4096) : tile_width(T);
    sts::TileArgs a{};
    a.in = in;
    a.out = out;
    a.lagmat = lagmat;
    a.err = err;
    a.S = S;
    a.T = T;
    a.ld_in = ld_in;
    a.ld_out = ld_out;
    a.tiles_per_series = (T + tw - 1) / tw;
    // STS_SEG_TILES: segment length (tiles) of the seg kernel, for A/B runs only
    const char* seg_env = seg ? sts::ab_knob("STS_SEG_TILES") : nullptr;
    // STS_TILES_PER_CHUNK: tiles per tile-kernel workgroup, for A/B runs only
    const char* tpc_env = seg ? nullptr : sts::ab_knob("STS_TILES_PER_CHUNK");
    const int seg_knob = seg_env ? std::atoi(seg_env) : 0, tpc_knob = tpc_env ? std::atoi(tpc_env) : 0;
    const int64_t per_chunk = seg ? (seg_knob > 0 ? seg_knob : sts::kSegTiles)
                                  : (tpc_knob > 0 ? tpc_knob : (K > 0 ? kTilesPerChunk : kTilesPerChunkFill));
    a.tiles_per_chunk = a.tiles_per_series < per_chunk ? a.tiles_per_series : per_chunk;
    a.chunks_per_series = (a.tiles_per_series + a.tiles_per_chunk - 1) / a.tiles_per_chunk;
    a.K = K;
    a.max_lag = max_lag;
    a.include_original = inc;
    if (S * a.chunks_per_series > 0x7fffffffLL) return fail(STS_ERR_BAD_ARG, "%s: panel too large for one launch", name);
    // one segment per series: the seg kernel writes err[s] for every series and, when the
    // finalize's general path applies (T > 2K) and the last tile holds >= 64 steps, the
    // final ACF itself (no partials, no second launch)
    const bool one_seg = seg && a.chunks_per_series == 1;
    const int64_t last_len = T - (a.tiles_per_series - 1) * tw;
    const bool fuse = one_seg && K > 0 && T > 2 * (int64_t)K && T >= 2 * sts::kAcfEdge && last_len >= 64 &&
                      !sts::ab_knob("STS_NO_FUSED_ACF");
    a.err_all = one_seg ? 1 : 0;
    a.acf_fused = fuse ? acf : nullptr;
    // any of the four fills + ACF with K <= 24 on T <= 2560 (C1): one wave holds the whole series
    // (sts_short.hip; its rule-3 fallback re-reads the filled series from out); STS_NO_SHORT keeps
    // the segment kernel (A/B build)
    const bool short_k = fuse && out && sts::short_ok(method, T, K) && !sts::ab_knob("STS_NO_SHORT");
    // two series per workgroup on one LDS block (sts_short.hip short_pair_kernel); STS_SHORT_PAIR=0/1
    // picks the form on the A/B build
    const char* pair_env = sts::ab_knob("STS_SHORT_PAIR");
    const bool short_pair = pair_env ? pair_env[0] == '1' : sts::kShortPairDefault;
    if (err && !one_seg) HIP_TRY(hipMemsetAsync(err, 0, (size_t)S * sizeof(int32_t), st), "hipMemsetAsync(err)");
    Scratch part(st);
    int32_t* exact = nullptr;
    if (K > 0 && !fuse) {
        // chunk partials, then (tile kernel) the per-series shifts, then rule 3's per-series flags
        const size_t np = (size_t)(S * a.chunks_per_series) * sts::kPartStride;
        const size_t nsh = seg ? 0 : (size_t)S;
        hipError_t e = part.alloc((np + nsh + ((size_t)S + 1) / 2) * sizeof(double));
        if (e != hipSuccess) return hip_fail(e, "hipMallocAsync(partials)");
        a.partials = static_cast<double*>(part.p);
        exact = reinterpret_cast<int32_t*>(a.partials + np + nsh);
        HIP_TRY(hipMemsetAsync(exact, 0, (size_t)S * sizeof(int32_t), st), "hipMemsetAsync(rule 3 flags)");
        if (!seg) {
            double* sh = a.partials + np;
            e = sts::launch_acf_shift(in, S, T, ld_in, method, sh, st);
            if (e != hipSuccess) return hip_fail(e, "acf shift");
            a.shift = sh;
        }
    }
    prof_mark(st);
    hipError_t e = short_k ? sts::launch_short(method, a, st, short_pair)
                   : seg   ? sts::launch_segment(method, a, st)
                           : sts::launch_tile(method, tw, a, st);
    prof_mark(st);
    if (e != hipSuccess) return hip_fail(e, name);
    if (K > 0 && !fuse) {
        sts::FinalizeArgs f{};
        f.F = out ? out : in;
        f.partials = a.partials;
        f.acf = acf;
        f.S = S;
        f.T = T;
        f.ldF = out ? ld_out : ld_in;
        f.parts_per_series = a.chunks_per_series;
        f.K = K;
        f.exact = exact;
        e = sts::launch_acf_finalize(f, st);
        if (e != hipSuccess) return hip_fail(e, "acf finalize");
        e = sts::launch_acf_exact(f.F, S, T, f.ldF, K, exact, acf, st);
        if (e != hipSuccess) return hip_fail(e, "acf exact (rule 3)");
    }
    return STS_OK;
}

}  // namespace

namespace sts {

// The first failing series of a host copy of err_per_series -> the reference's exception
// (status + thread-local message); STS_OK when none failed.
int series_status(const int32_t* h, int64_t S, const char* what) {
    for (int64_t s = 0; s < S; s++) {
        if (h[s] == STS_ERR_ALL_NAN) return fail(STS_ERR_ALL_NAN, "Input is all NaNs! (series %lld)", (long long)s);
        if (h[s] == STS_ERR_SINGULAR) return fail(STS_ERR_SINGULAR, "singular AR design matrix (series %lld)", (long long)s);
        if (h[s] == STS_ERR_TOO_FEW_POINTS)
            return fail(STS_ERR_TOO_FEW_POINTS,
                        "NumberIsTooSmallException: number of points: fewer than 3 non-NaN values for a spline (series %lld)",
                        (long long)s);
        if (h[s] == STS_ERR_TOO_MANY_EVALUATIONS)
            return fail(STS_ERR_TOO_MANY_EVALUATIONS,
                        "TooManyEvaluationsException: illegal state: maximal count (10000) exceeded: evaluations (series %lld)",
                        (long long)s);
        if (h[s] != 0) return fail(h[s], "%s failed for series %lld", what, (long long)s);
    }
    return STS_OK;
}

int set_error(int status, const char* msg) { return fail(status, "%s", msg); }

int validate_call(int (*fn)(void*), void* ctx, bool* has_work) {
    g_validate_only = true;
    const int r = fn(ctx);
    g_validate_only = false;
    *has_work = r == kValidated;   // stopped in ensure_device(); STS_OK: returned before it
    return *has_work ? STS_OK : r;
}

}  // namespace sts

extern "C" {

int sts_abi_version(void) { return STS_ABI_VERSION; }

int sts_init(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) return fail(STS_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(STS_ERR_BAD_ARG, "device %d out of range (%d devices)", device, n);
    HIP_TRY(hipSetDevice(device), "hipSetDevice");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(STS_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    return ensure_device();
}

const char* sts_last_error(void) { return g_err.c_str(); }

int sts_fill_method_from_name(const char* name) {
    if (!name) return -2;
    if (!std::strcmp(name, "linear")) return STS_FILL_LINEAR;
    if (!std::strcmp(name, "nearest")) return STS_FILL_NEAREST;
    if (!std::strcmp(name, "next")) return STS_FILL_NEXT;
    if (!std::strcmp(name, "previous")) return STS_FILL_PREVIOUS;
    if (!std::strcmp(name, "spline")) return STS_FILL_SPLINE;
    return -2;
}

int sts_profile_begin(void) {
    // create the event pool here, before the caller's timed region: a hipEventCreate inside
    // it costs CPU time per launch and can starve the queue of short kernels (C1: 0.13 ms)
    constexpr size_t kPrealloc = 512;
    while (g_prof.pool.size() < kPrealloc) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e), "hipEventCreate");
        g_prof.pool.push_back(e);
    }
    g_prof.on = true;
    g_prof.used = 0;
    return STS_OK;
}

int sts_profile_end(double* kernel_ms, int64_t* launches) {
    g_prof.on = false;
    double total = 0.0;
    int64_t n = 0;
    for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
        HIP_TRY(hipEventSynchronize(g_prof.pool[i + 1]), "hipEventSynchronize");
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, g_prof.pool[i], g_prof.pool[i + 1]), "hipEventElapsedTime");
        total += ms;
        n++;
    }
    g_prof.used = 0;
    for (hipEvent_t e : g_prof.pool) (void)hipEventDestroy(e);   // recreated by the next begin
    g_prof.pool.clear();
    if (kernel_ms) *kernel_ms = total;
    if (launches) *launches = n;
    return STS_OK;
}

int sts_stream_synchronize(void* stream) {
    HIP_TRY(hipStreamSynchronize(as_stream(stream)), "hipStreamSynchronize");
    return STS_OK;
}

int sts_fill(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int method,
             int32_t* err_per_series, void* stream) {
    int r;
    if ((r = method_ok(method, false, "fill"))) return r;
    if ((r = check_panel(in, S, T, ld_in, "fill"))) return r;
    if ((r = check_panel(out, S, T, ld_out, "fill"))) return r;
    if (S * T > 0 && in == out) return fail(STS_ERR_BAD_ARG, "fill: out must not alias in (fillts returns a new vector)");
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare(false))) return r;   // run_tile zeroes err unless its kernel writes all of it
    if ((r = run_tile(in, out, nullptr, S, T, ld_in, ld_out, method, 0, nullptr, 0, 0, es.dev, st, "fill"))) return r;
    return es.finish("fill");
}

int sts_fill_autocorr(const double* in, double* filled, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                      int method, int K, double* acf, int32_t* err_per_series, void* stream) {
    int r;
    if ((r = method_ok(method, true, "fill_autocorr"))) return r;
    if ((r = check_panel(in, S, T, ld_in, "fill_autocorr"))) return r;
    if (method != STS_FILL_NONE) {
        if ((r = check_panel(filled, S, T, ld_out, "fill_autocorr"))) return r;
        if (S * T > 0 && in == filled) return fail(STS_ERR_BAD_ARG, "fill_autocorr: filled must not alias in");
    } else if (filled) {
        return fail(STS_ERR_BAD_ARG, "fill_autocorr: filled must be NULL for STS_FILL_NONE");
    }
    if (K < 0) return fail(STS_ERR_BAD_ARG, "autocorr: negative numLags %d", K);
    if (S > 0 && K > 0 && !acf) return fail(STS_ERR_BAD_ARG, "autocorr: null output");
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare(false))) return r;   // zeroed by run_tile, or below when it does not run
    if (method == STS_FILL_SPLINE) {
        // fillSpline (not fused: sts_spline.hip), then autocorr of the filled panel; the ACF
        // pass reports into a scratch array so the spline's per-series status stands
        if ((r = run_spline(in, filled, S, T, ld_in, ld_out, es.dev, st))) return r;
        if (K > 0 && S > 0) {
            Scratch e2(st);
            HIP_TRY(e2.alloc((size_t)S * sizeof(int32_t)), "hipMallocAsync(err)");
            if ((r = sts_fill_autocorr(filled, nullptr, S, T, ld_out, ld_out, STS_FILL_NONE, K, acf,
                                       static_cast<int32_t*>(e2.p), st))) return r;
        }
        return es.finish("fill_autocorr");
    }
    if (S > 0 && (T == 0 || (K == 0 && method == STS_FILL_NONE)))
        HIP_TRY(hipMemsetAsync(es.dev, 0, (size_t)S * sizeof(int32_t), st), "hipMemsetAsync(err)");
    if (T == 0 && S > 0 && K > 0) {
        std::vector<double> nan((size_t)(S * K), NAN);
        HIP_TRY(hipMemcpyAsync(acf, nan.data(), nan.size() * sizeof(double), hipMemcpyHostToDevice, st), "acf");
        HIP_TRY(hipStreamSynchronize(st), "acf");
        return es.finish("fill_autocorr");
    }
    if (K == 0) {
        if (method != STS_FILL_NONE && (r = run_tile(in, filled, nullptr, S, T, ld_in, ld_out, method, 0, nullptr, 0, 0,
                                                    es.dev, st, "fill"))) return r;
        return es.finish("fill_autocorr");
    }
    if (K > sts::kFusedMaxLags) {
        // any numLags (sts_acf_wide.hip): fill first (no ACF), then lag blocks of 61 on MFMA
        const double* F = in;
        int64_t ldF = ld_in;
        if (method != STS_FILL_NONE) {
            if ((r = run_tile(in, filled, nullptr, S, T, ld_in, ld_out, method, 0, nullptr, 0, 0, es.dev, st, "fill")))
                return r;
            F = filled;
            ldF = ld_out;
        } else {
            HIP_TRY(hipMemsetAsync(es.dev, 0, (size_t)S * sizeof(int32_t), st), "hipMemsetAsync(err)");
        }
        Scratch sc(st);
        const size_t np = sts::acf_wide_partials(S, T, K);
        hipError_t e = sc.alloc(((size_t)S + np + ((size_t)S + 1) / 2) * sizeof(double));
        if (e != hipSuccess) return hip_fail(e, "hipMallocAsync(acf partials)");
        double* shift = static_cast<double*>(sc.p);
        int32_t* exact = reinterpret_cast<int32_t*>(shift + S + np);
        HIP_TRY(hipMemsetAsync(exact, 0, (size_t)S * sizeof(int32_t), st), "hipMemsetAsync(rule 3 flags)");
        HIP_TRY(sts::launch_acf_shift(F, S, T, ldF, STS_FILL_NONE, shift, st), "acf shift");
        HIP_TRY(timed(st, [&] { return sts::launch_acf_wide(F, S, T, ldF, shift, K, shift + S, acf, exact, st); }),
                "autocorr (wide)");
        return es.finish("fill_autocorr");
    }
    if ((r = run_tile(in, method == STS_FILL_NONE ? nullptr : filled, nullptr, S, T, ld_in, ld_out, method, K, acf, 0,
                      0, es.dev, st, "fill_autocorr"))) return r;
    return es.finish("fill_autocorr");
}

int sts_autocorr(const double* in, int64_t S, int64_t T, int64_t ld, int K, double* acf, void* stream) {
    return sts_fill_autocorr(in, nullptr, S, T, ld, ld, STS_FILL_NONE, K, acf, nullptr, stream);
}

int sts_diff_at_lag(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int lag,
                    int start, void* stream) {
    int r;
    if (!(start >= lag)) return fail(STS_ERR_REQUIREMENT, "requirement failed: starting index cannot be less than lag");
    if (lag < 0) return fail(STS_ERR_BAD_ARG, "differencesAtLag: negative lag %d", lag);
    if ((r = check_panel(in, S, T, ld_in, "differencesAtLag"))) return r;
    if ((r = check_panel(out, S, T, ld_out, "differencesAtLag"))) return r;
    if (lag == 0 || S * T == 0) return STS_OK;  // dest returned untouched (:363-364)
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    if (in == out) {
        if (ld_in != ld_out) return fail(STS_ERR_BAD_ARG, "differencesAtLag: in-place call with different ld");
        HIP_TRY(sts::launch_diff_inplace(out, S, T, ld_out, lag, start, st), "differencesAtLag(in place)");
    } else {
        HIP_TRY(sts::launch_diff(in, out, S, T, ld_in, ld_out, lag, start, st), "differencesAtLag");
    }
    return STS_OK;
}

int sts_lag_matrix(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int max_lag,
                   int include_original, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld_in, "lag"))) return r;
    if (max_lag < 0 || max_lag > T) return fail(STS_ERR_BAD_ARG, "lag: maxLag %d outside [0, T=%lld]", max_lag, (long long)T);
    const int64_t n = S * (T - max_lag) * (max_lag + (include_original ? 1 : 0));
    if (n > 0 && !out) return fail(STS_ERR_BAD_ARG, "lag: null output");
    if (n == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_lagmat(in, out, S, T, ld_in, max_lag, include_original, as_stream(stream)), "lag");
    return STS_OK;
}

int sts_fill_lag_matrix(const double* in, double* filled, double* lagmat, int64_t S, int64_t T, int64_t ld_in,
                        int64_t ld_out, int method, int max_lag, int include_original, int32_t* err_per_series,
                        void* stream) {
    int r;
    if ((r = method_ok(method, true, "fill_lag_matrix"))) return r;
    if ((r = check_panel(in, S, T, ld_in, "fill_lag_matrix"))) return r;
    if (filled && (r = check_panel(filled, S, T, ld_out, "fill_lag_matrix"))) return r;
    if (filled && S * T > 0 && filled == in) return fail(STS_ERR_BAD_ARG, "fill_lag_matrix: filled must not alias in");
    if (max_lag < 0 || max_lag > T) return fail(STS_ERR_BAD_ARG, "lag: maxLag %d outside [0, T=%lld]", max_lag, (long long)T);
    const int64_t n = S * (T - max_lag) * (max_lag + (include_original ? 1 : 0));
    if (n > 0 && !lagmat) return fail(STS_ERR_BAD_ARG, "lag: null output");
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare(false))) return r;   // run_tile zeroes err unless its kernel writes all of it
    if (method == STS_FILL_SPLINE) {
        // fillSpline (sts_spline.hip) into `filled` (or a scratch panel), then the lag matrix
        Scratch tmp(st);
        double* F = filled;
        int64_t ldF = ld_out;
        if (!F && S * T > 0) {
            HIP_TRY(tmp.alloc((size_t)(S * T) * sizeof(double)), "hipMallocAsync(filled)");
            F = static_cast<double*>(tmp.p);
            ldF = T;
        }
        if ((r = run_spline(in, F, S, T, ld_in, ldF, es.dev, st))) return r;
        if (n > 0) HIP_TRY(sts::launch_lagmat(F, lagmat, S, T, ldF, max_lag, include_original ? 1 : 0, st), "lag");
        return es.finish("fill_lag_matrix");
    }
    if ((r = run_tile(in, filled, n > 0 ? lagmat : nullptr, S, T, ld_in, ld_out, method, 0, nullptr, max_lag,
                      include_original ? 1 : 0, es.dev, st, "fill_lag_matrix"))) return r;
    return es.finish("fill_lag_matrix");
}

int sts_ewma_add(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                 const double* smoothing, void* stream) {
    int r;
    if (!out) return fail(STS_ERR_NULL_DEST, "EWMAModel.addTimeDependentEffects: dest is null (NullPointerException)");
    if ((r = check_panel(in, S, T, ld_in, "ewma_add"))) return r;
    if ((r = check_panel(out, S, T, ld_out, "ewma_add"))) return r;
    if (S > 0 && !smoothing) return fail(STS_ERR_BAD_ARG, "ewma_add: null smoothing");
    if (S * T == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    sts::RecurArgs a{};
    a.in = in; a.out = out; a.S = S; a.T = T; a.ld_in = ld_in; a.ld_out = ld_out; a.sm = smoothing;
    HIP_TRY(sts::launch_recur(sts::kEwmaAdd, a, as_stream(stream)), "ewma_add");
    return STS_OK;
}

int sts_ewma_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                    const double* smoothing, void* stream) {
    int r;
    if (!out) return fail(STS_ERR_NULL_DEST, "EWMAModel.removeTimeDependentEffects: dest is null (NullPointerException)");
    if ((r = check_panel(in, S, T, ld_in, "ewma_remove"))) return r;
    if ((r = check_panel(out, S, T, ld_out, "ewma_remove"))) return r;
    if (S > 0 && !smoothing) return fail(STS_ERR_BAD_ARG, "ewma_remove: null smoothing");
    if (S * T == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    if (in == out) {
        sts::RecurArgs a{};
        a.in = in; a.out = out; a.S = S; a.T = T; a.ld_in = ld_in; a.ld_out = ld_out; a.sm = smoothing;
        HIP_TRY(sts::launch_recur(sts::kEwmaRemoveInplace, a, st), "ewma_remove(in place)");
    } else {
        HIP_TRY(sts::launch_ewma_remove(in, out, S, T, ld_in, ld_out, smoothing, st), "ewma_remove");
    }
    return STS_OK;
}

int sts_ar_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                  const double* c, const double* coef, int p, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld_in, "ar_remove"))) return r;
    if ((r = check_panel(out, S, T, ld_out, "ar_remove"))) return r;
    if (p < 0) return fail(STS_ERR_BAD_ARG, "ar_remove: negative order");
    if (S > 0 && (!c || (p > 0 && !coef))) return fail(STS_ERR_BAD_ARG, "ar_remove: null model");
    if (S * T == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    if (in == out) {
        sts::RecurArgs a{};
        a.in = in; a.out = out; a.S = S; a.T = T; a.ld_in = ld_in; a.ld_out = ld_out; a.c = c; a.coef = coef; a.p = p;
        HIP_TRY(sts::launch_recur(sts::kArRemoveInplace, a, st), "ar_remove(in place)");
    } else {
        HIP_TRY(sts::launch_ar_remove(in, out, S, T, ld_in, ld_out, c, coef, p, st), "ar_remove");
    }
    return STS_OK;
}

int sts_ar_add(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, const double* c,
               const double* coef, int p, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld_in, "ar_add"))) return r;
    if ((r = check_panel(out, S, T, ld_out, "ar_add"))) return r;
    if (p < 0) return fail(STS_ERR_BAD_ARG, "ar_add: negative order");
    if (S > 0 && (!c || (p > 0 && !coef))) return fail(STS_ERR_BAD_ARG, "ar_add: null model");
    if (S * T == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    sts::RecurArgs a{};
    a.in = in; a.out = out; a.S = S; a.T = T; a.ld_in = ld_in; a.ld_out = ld_out; a.c = c; a.coef = coef; a.p = p;
    HIP_TRY(sts::launch_recur(sts::kArAdd, a, as_stream(stream)), "ar_add");
    return STS_OK;
}

static int ar_fit_common(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int p,
                         int no_intercept, double* c, double* coef, int32_t* err_per_series, void* stream,
                         const char* name) {
    int r;
    if ((r = check_panel(in, S, T, ld_in, name))) return r;
    if (out && (r = check_panel(out, S, T, ld_out, name))) return r;
    if (p < 1 || p > 31) return fail(STS_ERR_BAD_ARG, "%s: AR order %d outside [1, 31]", name, p);
    if (T - p < (int64_t)p + 1)
        return fail(STS_ERR_NOT_ENOUGH_DATA, "%s: not enough data (%lld rows) for the number of predictors (%d)", name,
                    (long long)(T - p), p);
    if (S > 0 && (!c || !coef)) return fail(STS_ERR_BAD_ARG, "%s: null model output", name);
    if (out && in == out) return fail(STS_ERR_BAD_ARG, "%s: out must not alias in", name);
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare())) return r;
    sts::ArArgs a{};
    a.in = in; a.out = out; a.c = c; a.coef = coef; a.err = es.dev;
    a.S = S; a.T = T; a.ld_in = ld_in; a.ld_out = ld_out; a.p = p; a.no_intercept = no_intercept ? 1 : 0;
    HIP_TRY(timed(st, [&] { return sts::launch_ar_fit(a, st); }), name);
    return es.finish(name);
}

int sts_ar_fit(const double* in, int64_t S, int64_t T, int64_t ld, int p, int no_intercept, double* c, double* coef,
               int32_t* err_per_series, void* stream) {
    return ar_fit_common(in, nullptr, S, T, ld, ld, p, no_intercept, c, coef, err_per_series, stream, "ar_fit");
}

int sts_ar_rule_count(const double* in, int64_t S, int64_t T, int64_t ld, int p, int no_intercept, int64_t* count,
                      void* stream) {
    int r;
    const char* name = "ar_rule_count";
    if ((r = check_panel(in, S, T, ld, name))) return r;
    if (!count) return fail(STS_ERR_BAD_ARG, "%s: null count", name);
    if (p < 1 || p > 31) return fail(STS_ERR_BAD_ARG, "%s: AR order %d outside [1, 31]", name, p);
    if (T - p < (int64_t)p + 1)
        return fail(STS_ERR_NOT_ENOUGH_DATA, "%s: not enough data (%lld rows) for the number of predictors (%d)", name,
                    (long long)(T - p), p);
    *count = 0;
    if (S == 0) return STS_OK;
    if (no_intercept) {
        *count = S;
        return STS_OK;
    }
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    Scratch sc(st);
    const size_t S8 = (size_t)S * sizeof(double);
    HIP_TRY(sc.alloc(S8 * (size_t)(p + 1) + S * sizeof(int32_t) + 64), "hipMallocAsync(ar_rule_count)");
    char* base = static_cast<char*>(sc.p);
    sts::ArArgs a{};
    a.in = in; a.out = nullptr; a.c = reinterpret_cast<double*>(base); a.coef = a.c + S;
    a.err = reinterpret_cast<int32_t*>(base + S8 * (size_t)(p + 1));
    a.S = S; a.T = T; a.ld_in = ld; a.ld_out = ld; a.p = p; a.no_intercept = 0;
    uint32_t* dcount = reinterpret_cast<uint32_t*>(base + S8 * (size_t)(p + 1) + S * sizeof(int32_t));
    HIP_TRY(sts::launch_ar_rule_count(a, dcount, st), name);
    uint32_t h = 0;
    HIP_TRY(hipMemcpyAsync(&h, dcount, sizeof(h), hipMemcpyDeviceToHost, st), name);
    HIP_TRY(hipStreamSynchronize(st), name);
    *count = (int64_t)h;
    return STS_OK;
}

int sts_ar_fit_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int p,
                      int no_intercept, double* c, double* coef, int32_t* err_per_series, void* stream) {
    if (!out) return fail(STS_ERR_BAD_ARG, "ar_fit_remove: null output");
    return ar_fit_common(in, out, S, T, ld_in, ld_out, p, no_intercept, c, coef, err_per_series, stream,
                         "ar_fit_remove");
}

int sts_ewma_fit(const double* in, int64_t S, int64_t T, int64_t ld, double* smoothing, int32_t* err_per_series,
                 void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld, "EWMA.fitModel"))) return r;
    if (S > 0 && T < 1) return fail(STS_ERR_BAD_ARG, "EWMA.fitModel: empty series (ts(0) does not exist)");
    if (S > 0 && !smoothing) return fail(STS_ERR_BAD_ARG, "EWMA.fitModel: null output");
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare())) return r;
    sts::EwmaFitArgs a{};
    a.in = in; a.S = S; a.T = T; a.ld = ld; a.smoothing = smoothing; a.err = es.dev;
    HIP_TRY(timed(st, [&] { return sts::launch_ewma_fit(a, true, st); }), "EWMA.fitModel");
    return es.finish("EWMA.fitModel");
}

int sts_ewma_sse_gradient(const double* in, int64_t S, int64_t T, int64_t ld, const double* smoothing, double* sse,
                          double* gradient, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld, "EWMAModel.sse"))) return r;
    if (S > 0 && T < 1) return fail(STS_ERR_BAD_ARG, "EWMAModel.sse: empty series (ts(0) does not exist)");
    if (S > 0 && !smoothing) return fail(STS_ERR_BAD_ARG, "EWMAModel.sse: null smoothing");
    if (S == 0 || (!sse && !gradient)) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    sts::EwmaFitArgs a{};
    a.in = in; a.S = S; a.T = T; a.ld = ld; a.smoothing = const_cast<double*>(smoothing);
    a.sse = sse; a.grad = gradient;
    HIP_TRY(timed(st, [&] { return sts::launch_ewma_fit(a, false, st); }), "EWMAModel.sse/gradient");
    return STS_OK;
}

// ---- GARCH(1,1) / AR(1)+GARCH(1,1): S/models/GARCH.scala ----

int sts_garch_fit(const double* in, int64_t S, int64_t T, int64_t ld, double* params, int32_t* err_per_series,
                  void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld, "GARCH.fitModel"))) return r;
    if (S > 0 && !params) return fail(STS_ERR_BAD_ARG, "GARCH.fitModel: null output");
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare())) return r;
    sts::GarchFitArgs a{};
    a.in = in; a.S = S; a.T = T; a.ld = ld; a.params = params; a.err = es.dev;
    HIP_TRY(timed(st, [&] { return sts::launch_garch_fit(a, true, st); }), "GARCH.fitModel");
    return es.finish("GARCH.fitModel");
}

int sts_garch_loglik_gradient(const double* in, int64_t S, int64_t T, int64_t ld, const double* params,
                              double* loglik, double* gradient, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld, "GARCHModel.logLikelihood"))) return r;
    if (S > 0 && !params) return fail(STS_ERR_BAD_ARG, "GARCHModel.logLikelihood: null params");
    if (S == 0 || (!loglik && !gradient)) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    sts::GarchFitArgs a{};
    a.in = in; a.S = S; a.T = T; a.ld = ld; a.params = const_cast<double*>(params);
    a.loglik = loglik; a.grad = gradient;
    HIP_TRY(timed(st, [&] { return sts::launch_garch_fit(a, false, st); }), "GARCHModel.logLikelihood/gradient");
    return STS_OK;
}

static int garch_effects(int op, const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                         const double* c, const double* phi, const double* omega, const double* alpha,
                         const double* beta, void* stream, const char* name) {
    int r;
    if ((r = check_panel(in, S, T, ld_in, name))) return r;
    if (!out) return fail(STS_ERR_NULL_DEST, "%s: dest is null (the reference writes into dest)", name);
    if ((r = check_panel(out, S, T, ld_out, name))) return r;
    if (S > 0 && (!omega || !alpha || !beta)) return fail(STS_ERR_BAD_ARG, "%s: null model parameters", name);
    const bool ar = op != sts::kGarchRemove && op != sts::kGarchAdd;
    if (S > 0 && ar && (!c || !phi)) return fail(STS_ERR_BAD_ARG, "%s: null model parameters", name);
    if (S * T == 0) return STS_OK;
    if (in == out && ld_in != ld_out) return fail(STS_ERR_BAD_ARG, "%s: in place needs ld_in == ld_out", name);
    if (op == sts::kArgarchRemove && in == out) op = sts::kArgarchRemoveInplace;   // dest eq ts
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    sts::GarchEffectsArgs a{};
    a.in = in; a.out = out; a.S = S; a.T = T; a.ld_in = ld_in; a.ld_out = ld_out;
    a.c = c; a.phi = phi; a.omega = omega; a.alpha = alpha; a.beta = beta;
    HIP_TRY(timed(st, [&] { return sts::launch_garch_effects(op, a, st); }), name);
    return STS_OK;
}

int sts_garch_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                     const double* omega, const double* alpha, const double* beta, void* stream) {
    return garch_effects(sts::kGarchRemove, in, out, S, T, ld_in, ld_out, nullptr, nullptr, omega, alpha, beta,
                         stream, "GARCHModel.removeTimeDependentEffects");
}

int sts_garch_add(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                  const double* omega, const double* alpha, const double* beta, void* stream) {
    return garch_effects(sts::kGarchAdd, in, out, S, T, ld_in, ld_out, nullptr, nullptr, omega, alpha, beta, stream,
                         "GARCHModel.addTimeDependentEffects");
}

int sts_argarch_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                       const double* c, const double* phi, const double* omega, const double* alpha,
                       const double* beta, void* stream) {
    return garch_effects(sts::kArgarchRemove, in, out, S, T, ld_in, ld_out, c, phi, omega, alpha, beta, stream,
                         "ARGARCHModel.removeTimeDependentEffects");
}

int sts_argarch_add(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                    const double* c, const double* phi, const double* omega, const double* alpha,
                    const double* beta, void* stream) {
    return garch_effects(sts::kArgarchAdd, in, out, S, T, ld_in, ld_out, c, phi, omega, alpha, beta, stream,
                         "ARGARCHModel.addTimeDependentEffects");
}

int sts_argarch_fit(const double* in, int64_t S, int64_t T, int64_t ld, double* c, double* phi, double* params,
                    int32_t* err_per_series, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld, "ARGARCH.fitModel"))) return r;
    if (S > 0 && (!c || !phi || !params)) return fail(STS_ERR_BAD_ARG, "ARGARCH.fitModel: null output");
    if (T - 1 < 2)
        return fail(STS_ERR_NOT_ENOUGH_DATA, "ARGARCH.fitModel: not enough data (%lld rows) for the number of predictors (1)",
                    (long long)(T - 1));
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare())) return r;
    // Autoregression.fitModel(ts) = AR(1) with intercept; residuals into dest = zeros(n)
    Scratch resid(st);
    HIP_TRY(resid.alloc((size_t)(S * T) * sizeof(double)), "hipMallocAsync(argarch)");
    double* rs = static_cast<double*>(resid.p);
    sts::ArArgs ar{};
    ar.in = in; ar.out = rs; ar.c = c; ar.coef = phi; ar.err = es.dev;
    ar.S = S; ar.T = T; ar.ld_in = ld; ar.ld_out = T; ar.p = 1; ar.no_intercept = 0;
    HIP_TRY(timed(st, [&] { return sts::launch_ar_fit(ar, st); }), "ARGARCH.fitModel (AR stage)");
    // GARCH.fitModel(residuals); an AR-stage failure keeps its status
    sts::GarchFitArgs g{};
    g.in = rs; g.S = S; g.T = T; g.ld = T; g.params = params; g.err = es.dev; g.keep_err = 1;
    HIP_TRY(timed(st, [&] { return sts::launch_garch_fit(g, true, st); }), "ARGARCH.fitModel (GARCH stage)");
    return es.finish("ARGARCH.fitModel");
}

int sts_series_stats(const double* in, int64_t S, int64_t T, int64_t ld, double* stats, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld, "seriesStats"))) return r;
    if (S > 0 && !stats) return fail(STS_ERR_BAD_ARG, "seriesStats: null output");
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    HIP_TRY(timed(st, [&] { return sts::launch_series_stats(in, stats, S, T, ld, st); }), "seriesStats");
    return STS_OK;
}

int sts_nan_instants(const double* in, int64_t S, int64_t T, int64_t ld, uint8_t* flags, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld, "removeInstantsWithNaNs"))) return r;
    if (T > 0 && !flags) return fail(STS_ERR_BAD_ARG, "removeInstantsWithNaNs: null flags");
    if (S * T == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    HIP_TRY(timed(st, [&] { return sts::launch_nan_instants(in, flags, S, T, ld, st); }), "nan_instants");
    return STS_OK;
}

int sts_active_instants(const uint8_t* flags, int64_t T, int64_t* active, int64_t* n_active, void* stream) {
    if (T < 0) return fail(STS_ERR_BAD_ARG, "active_instants: negative T");
    if (!n_active || (T > 0 && (!flags || !active))) return fail(STS_ERR_BAD_ARG, "active_instants: null pointer");
    int r;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    Scratch sc(st);
    HIP_TRY(sc.alloc((size_t)sts::active_scratch_elems(T) * sizeof(int64_t)), "hipMallocAsync(active scratch)");
    HIP_TRY(sts::launch_active_instants(flags, T, active, n_active, static_cast<int64_t*>(sc.p), st), "active_instants");
    return STS_OK;
}

int sts_gather_instants(const double* in, double* out, int64_t S, int64_t ld_in, int64_t ld_out, const int64_t* active,
                        int64_t n_active, void* stream) {
    if (S < 0 || n_active < 0 || ld_out < n_active) return fail(STS_ERR_BAD_ARG, "gather_instants: bad shape");
    if (S * n_active > 0 && (!in || !out || !active)) return fail(STS_ERR_BAD_ARG, "gather_instants: null pointer");
    if (S * n_active == 0) return STS_OK;
    int r;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    HIP_TRY(timed(st, [&] { return sts::launch_gather_instants(in, out, active, n_active, S, ld_in, ld_out, st); }),
            "gather_instants");
    return STS_OK;
}

int sts_to_instants(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld_in, "toInstants"))) return r;
    if (ld_out < S) return fail(STS_ERR_BAD_ARG, "toInstants: ld_out %lld < S=%lld", (long long)ld_out, (long long)S);
    if (S * T > 0 && !out) return fail(STS_ERR_BAD_ARG, "toInstants: null output");
    if (S * T == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    HIP_TRY(timed(st, [&] { return sts::launch_transpose(in, out, S, T, ld_in, ld_out, st); }), "toInstants");
    return STS_OK;
}

static inline int64_t be32(const uint8_t* p) {
    return (int64_t)(int32_t)(((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]);
}

int sts_wire_scan(const uint8_t* bytes, int64_t nbytes, int64_t max_records, int64_t* n_records, int64_t* T,
                  int64_t* key_off, int32_t* key_len, int64_t* val_off) {
    if (!n_records || !T || nbytes < 0 || (nbytes > 0 && !bytes)) return fail(STS_ERR_BAD_ARG, "wire_scan: bad arguments");
    int64_t pos = 0, n = 0, len = -1;
    while (pos < nbytes) {
        if (pos + 4 > nbytes) return fail(STS_ERR_BAD_ARG, "wire_scan: truncated key length at byte %lld", (long long)pos);
        const int64_t kl = be32(bytes + pos);
        if (kl < 0 || pos + 4 + kl + 4 > nbytes)
            return fail(STS_ERR_BAD_ARG, "wire_scan: bad key length %lld at byte %lld", (long long)kl, (long long)pos);
        const int64_t vn = be32(bytes + pos + 4 + kl);
        if (vn < 0 || pos + 8 + kl + 8 * vn > nbytes)
            return fail(STS_ERR_BAD_ARG, "wire_scan: bad series length %lld at byte %lld", (long long)vn, (long long)pos);
        if (len >= 0 && vn != len)
            return fail(STS_ERR_BAD_ARG, "wire_scan: record %lld holds %lld values, record 0 holds %lld (one shared index)",
                        (long long)n, (long long)vn, (long long)len);
        len = vn;
        if (n < max_records) {
            if (key_off) key_off[n] = pos + 4;
            if (key_len) key_len[n] = (int32_t)kl;
            if (val_off) val_off[n] = pos + 8 + kl;
        }
        n++;
        pos += 8 + kl + 8 * vn;
    }
    *n_records = n;
    *T = len < 0 ? 0 : len;
    return n > max_records ? fail(STS_ERR_BAD_ARG, "wire_scan: %lld records > capacity %lld", (long long)n,
                                  (long long)max_records)
                           : STS_OK;
}

int sts_wire_decode(const uint8_t* bytes, const int64_t* val_off, int64_t S, int64_t T, double* panel, int64_t ld,
                    void* stream) {
    int r;
    if ((r = check_panel(panel, S, T, ld, "wire_decode"))) return r;
    if (S * T > 0 && (!bytes || !val_off)) return fail(STS_ERR_BAD_ARG, "wire_decode: null pointer");
    if (S * T == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    HIP_TRY(timed(st, [&] { return sts::launch_wire_decode(bytes, val_off, panel, S, T, ld, st); }), "wire_decode");
    return STS_OK;
}

int sts_wire_encode(const double* panel, int64_t S, int64_t T, int64_t ld, const int64_t* val_off, uint8_t* bytes,
                    void* stream) {
    int r;
    if ((r = check_panel(panel, S, T, ld, "wire_encode"))) return r;
    if (S * T > 0 && (!bytes || !val_off)) return fail(STS_ERR_BAD_ARG, "wire_encode: null pointer");
    if (S * T == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    HIP_TRY(timed(st, [&] { return sts::launch_wire_encode(panel, S, T, ld, val_off, bytes, st); }), "wire_encode");
    return STS_OK;
}

int sts_observations_to_panel(const int32_t* series_id, const int64_t* loc, const double* value, int64_t n_obs,
                              double* panel, int64_t S, int64_t T, int64_t ld, void* stream) {
    int r;
    if ((r = check_panel(panel, S, T, ld, "timeSeriesRDDFromObservations"))) return r;
    if (n_obs < 0 || (n_obs > 0 && (!series_id || !loc || !value)))
        return fail(STS_ERR_BAD_ARG, "timeSeriesRDDFromObservations: bad observation arrays");
    if (S * T == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    Scratch win(st);
    HIP_TRY(win.alloc((size_t)(n_obs > 0 ? n_obs : 1)), "hipMallocAsync(obs flags)");
    HIP_TRY(timed(st, [&] {
                return sts::launch_observations(series_id, loc, value, n_obs, panel, S, T, ld,
                                                static_cast<unsigned char*>(win.p), st);
            }),
            "timeSeriesRDDFromObservations");
    return STS_OK;
}

// java.lang.Double.parseDouble for the tokens Double.toString writes (decimal, optional
// exponent, NaN, Infinity, -Infinity); surrounding whitespace is trimmed like Java's.
static bool parse_java_double(const char* b, const char* e, double* out) {
    while (b < e && (unsigned char)*b <= ' ') b++;
    while (e > b && (unsigned char)e[-1] <= ' ') e--;
    const size_t n = (size_t)(e - b);
    if (n == 0 || n > 400) return false;
    char buf[401];
    std::memcpy(buf, b, n);
    buf[n] = 0;
    const char* q = buf;
    const bool neg = (*q == '-'), sgn = (neg || *q == '+');
    if (sgn) q++;
    if (!std::strcmp(q, "NaN")) { *out = NAN; return true; }
    if (!std::strcmp(q, "Infinity")) { *out = neg ? -INFINITY : INFINITY; return true; }
    for (const char* c = q; *c; c++)   // decimal digits, '.', exponent (strtod would also take hex / "inf")
        if (!((*c >= '0' && *c <= '9') || *c == '.' || *c == 'e' || *c == 'E' || *c == '+' || *c == '-' ||
              *c == 'd' || *c == 'D' || *c == 'f' || *c == 'F'))
            return false;
    if (n > 0 && (buf[n - 1] == 'd' || buf[n - 1] == 'D' || buf[n - 1] == 'f' || buf[n - 1] == 'F')) buf[n - 1] = 0;
    char* end = nullptr;
    *out = std::strtod(buf, &end);   // correctly rounded (glibc), as parseDouble is
    return end && *end == 0 && end != q;
}

int sts_csv_parse(const char* text, int64_t len, int64_t max_records, int64_t* n_records, int64_t* T,
                  int64_t* key_off, int32_t* key_len, double* values, int64_t values_cap) {
    if (!n_records || !T || len < 0 || (len > 0 && !text)) return fail(STS_ERR_BAD_ARG, "csv_parse: bad arguments");
    int64_t pos = 0, n = 0, width = -1;
    while (pos < len) {
        int64_t eol = pos;
        while (eol < len && text[eol] != '\n') eol++;
        int64_t end = eol;
        if (end > pos && text[end - 1] == '\r') end--;
        if (end > pos) {   // sc.textFile skips nothing, but an empty trailing line is no record
            int64_t c = pos;
            while (c < end && text[c] != ',') c++;
            int64_t cnt = 0;
            int64_t f = c;
            while (f < end) {   // tokens.tail
                const int64_t g0 = f + 1;
                int64_t g = g0;
                while (g < end && text[g] != ',') g++;
                double v;
                if (!parse_java_double(text + g0, text + g, &v))
                    return fail(STS_ERR_BAD_ARG, "csv_parse: NumberFormatException at line %lld: \"%.*s\"", (long long)n,
                                (int)(g - g0 > 64 ? 64 : g - g0), text + g0);
                if (n < max_records && values && width >= 0 && n * width + cnt < values_cap) values[n * width + cnt] = v;
                else if (n < max_records && values && width < 0 && cnt < values_cap) values[cnt] = v;
                cnt++;
                f = g;
            }
            if (width >= 0 && cnt != width)
                return fail(STS_ERR_BAD_ARG, "csv_parse: line %lld holds %lld values, line 0 holds %lld", (long long)n,
                            (long long)cnt, (long long)width);
            width = cnt;
            if ((n + 1) * width > values_cap && values)
                return fail(STS_ERR_BAD_ARG, "csv_parse: values capacity %lld exceeded", (long long)values_cap);
            if (n < max_records) {
                if (key_off) key_off[n] = pos;
                if (key_len) key_len[n] = (int32_t)(c - pos);
            }
            n++;
        }
        pos = eol + 1;
    }
    *n_records = n;
    *T = width < 0 ? 0 : width;
    return n > max_records ? fail(STS_ERR_BAD_ARG, "csv_parse: %lld lines > capacity %lld", (long long)n,
                                  (long long)max_records)
                           : STS_OK;
}

namespace {

int arima_orders(const char* name, int64_t T, int p, int d, int q, int* n) {
    if (p < 0 || p > STS_ARIMA_MAX_ORDER || q < 0 || q > STS_ARIMA_MAX_ORDER)
        return fail(STS_ERR_BAD_ARG, "%s: orders p=%d, q=%d outside [0, %d]", name, p, q, STS_ARIMA_MAX_ORDER);
    if (d < 0 || d > T) return fail(STS_ERR_BAD_ARG, "%s: differencing order %d outside [0, T]", name, d);
    if (*n < 1) return fail(STS_ERR_BAD_ARG, "%s: a model without intercept, AR and MA terms has no coefficients", name);
    return STS_OK;
}

// differencesOfOrderD (S/UnivariateTimeSeries.scala:438-450): level i differences level i-1 at
// lag 1 from index i (ping-pong into packed scratch)
struct ArimaDiff {
    Scratch a, b;
    const double* cur = nullptr;
    int64_t ld = 0;
    explicit ArimaDiff(hipStream_t st) : a(st), b(st) {}
    int run(const double* in, int64_t S, int64_t T, int64_t ld_in, int d, hipStream_t st) {
        cur = in;
        ld = ld_in;
        if (d == 0 || S * T == 0) return STS_OK;
        HIP_TRY(a.alloc((size_t)(S * T) * sizeof(double)), "hipMallocAsync(arima)");
        if (d > 1) HIP_TRY(b.alloc((size_t)(S * T) * sizeof(double)), "hipMallocAsync(arima)");
        double* bufs[2] = {static_cast<double*>(a.p), static_cast<double*>(b.p)};
        for (int i = 1; i <= d; i++) {
            double* nxt = bufs[(i - 1) & 1];
            HIP_TRY(sts::launch_diff(cur, nxt, S, T, ld, T, 1, i, st), "differencesOfOrderD");
            cur = nxt;
            ld = T;
        }
        return STS_OK;
    }
};

}  // namespace

int sts_arima_fit_ar(const double* in, int64_t S, int64_t T, int64_t ld, int p, int d, int include_intercept,
                     double* c, double* coef, int32_t* err_per_series, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld, "ARIMA.fitModel"))) return r;
    if (d < 0 || d > T) return fail(STS_ERR_BAD_ARG, "ARIMA.fitModel: differencing order %d outside [0, T]", d);
    if (d == 0) return sts_ar_fit(in, S, T, ld, p, include_intercept ? 0 : 1, c, coef, err_per_series, stream);
    if (p < 1 || p > 31) return fail(STS_ERR_BAD_ARG, "ARIMA.fitModel: AR order %d outside [1, 31]", p);
    const int64_t Tn = T - d;
    if (Tn - p < (int64_t)p + 1)
        return fail(STS_ERR_NOT_ENOUGH_DATA, "ARIMA.fitModel: not enough data (%lld rows) for the number of predictors (%d)",
                    (long long)(Tn - p), p);
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ArimaDiff df(st);
    if ((r = df.run(in, S, T, ld, d, st))) return r;
    // .drop(d), then Autoregression.fitModel(diffed, p, !includeIntercept)
    return sts_ar_fit(df.cur + d, S, Tn, df.ld, p, include_intercept ? 0 : 1, c, coef, err_per_series, stream);
}

// ---- ARIMA(p, d, q) with MA terms: S/models/ARIMA.scala (sts_arima.hip) ----

int sts_arima_hr_init(const double* in, int64_t S, int64_t T, int64_t ld, int p, int d, int q, int include_intercept,
                      double* init_out, int32_t* err_per_series, void* stream) {
    const char* name = "ARIMA.HannanRissanenInit";
    int r, n = (include_intercept ? 1 : 0) + p + q;
    if ((r = check_panel(in, S, T, ld, name))) return r;
    if ((r = arima_orders(name, T, p, d, q, &n))) return r;
    if (S > 0 && !init_out) return fail(STS_ERR_BAD_ARG, "%s: null output", name);
    const int maxLag = p > q ? p : q, m = maxLag + 1;
    const int64_t N = T - d;
    if (N - m < (int64_t)m + 1)
        return fail(STS_ERR_NOT_ENOUGH_DATA, "%s: not enough data (%lld rows) for the number of predictors (%d)", name,
                    (long long)(N - m), m);
    if (N - m - maxLag < (int64_t)p + q + 1)
        return fail(STS_ERR_NOT_ENOUGH_DATA, "%s: not enough data (%lld rows) for the number of predictors (%d)", name,
                    (long long)(N - m - maxLag), p + q);
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare())) return r;
    ArimaDiff df(st);
    if ((r = df.run(in, S, T, ld, d, st))) return r;
    // stage one: Autoregression.fitModel(y, m) on the .drop(d) view
    Scratch arbuf(st);
    HIP_TRY(arbuf.alloc((size_t)S * (size_t)(m + 1) * sizeof(double)), "hipMallocAsync(arima)");
    double* c = static_cast<double*>(arbuf.p);
    double* phi = c + S;
    sts::ArArgs ar{};
    ar.in = df.cur + d; ar.c = c; ar.coef = phi; ar.err = es.dev;
    ar.S = S; ar.T = N; ar.ld_in = df.ld; ar.ld_out = N; ar.p = m; ar.no_intercept = 0;
    HIP_TRY(timed(st, [&] { return sts::launch_ar_fit(ar, st); }), "ARIMA.HannanRissanenInit (AR stage)");
    sts::ArimaHrArgs h{};
    h.in = df.cur + d; h.S = S; h.ld = df.ld; h.n_len = (int)N; h.p = p; h.q = q; h.icpt = include_intercept ? 1 : 0;
    h.c = c; h.phi = phi; h.init_out = init_out; h.err = es.dev;
    HIP_TRY(timed(st, [&] { return sts::launch_arima_hr(h, st); }), name);
    return es.finish(name);
}

int sts_arima_fit_css(const double* in, int64_t S, int64_t T, int64_t ld, int p, int d, int q, int include_intercept,
                      const double* init, double* coef_out, int32_t* err_per_series, int32_t* evals, void* stream) {
    const char* name = "ARIMA.fitModel(css-cgd)";
    int r, n = (include_intercept ? 1 : 0) + p + q;
    if ((r = check_panel(in, S, T, ld, name))) return r;
    if ((r = arima_orders(name, T, p, d, q, &n))) return r;
    if (S > 0 && (!init || !coef_out)) return fail(STS_ERR_BAD_ARG, "%s: null start or output", name);
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare())) return r;
    ArimaDiff df(st);
    if ((r = df.run(in, S, T, ld, d, st))) return r;
    sts::ArimaCssArgs a{};
    a.in = df.cur + d; a.S = S; a.ld = df.ld; a.n_len = (int)(T - d); a.p = p; a.q = q;
    a.icpt = include_intercept ? 1 : 0; a.coef_in = init; a.coef_out = coef_out; a.err = es.dev; a.evals = evals;
    HIP_TRY(timed(st, [&] { return sts::launch_arima_css(a, true, st); }), name);
    return es.finish(name);
}

int sts_arima_css_loglik_gradient(const double* in, int64_t S, int64_t T, int64_t ld, int p, int d, int q,
                                  int include_intercept, const double* coef, double* loglik, double* grad,
                                  void* stream) {
    const char* name = "ARIMAModel.logLikelihoodCSS";
    int r, n = (include_intercept ? 1 : 0) + p + q;
    if ((r = check_panel(in, S, T, ld, name))) return r;
    if ((r = arima_orders(name, T, p, d, q, &n))) return r;
    if (S > 0 && !coef) return fail(STS_ERR_BAD_ARG, "%s: null coefficients", name);
    if (S == 0 || (!loglik && !grad)) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ArimaDiff df(st);
    if ((r = df.run(in, S, T, ld, d, st))) return r;
    sts::ArimaCssArgs a{};
    a.in = df.cur + d; a.S = S; a.ld = df.ld; a.n_len = (int)(T - d); a.p = p; a.q = q;
    a.icpt = include_intercept ? 1 : 0; a.coef_in = coef; a.loglik = loglik; a.grad = grad;
    HIP_TRY(timed(st, [&] { return sts::launch_arima_css(a, false, st); }), name);
    return STS_OK;
}

static int arima_effects(bool add, const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                         int p, int d, int q, int include_intercept, const double* coef, void* stream) {
    const char* name = add ? "ARIMAModel.addTimeDependentEffects" : "ARIMAModel.removeTimeDependentEffects";
    int r, n = (include_intercept ? 1 : 0) + p + q;
    if ((r = check_panel(in, S, T, ld_in, name))) return r;
    if (!out) return fail(STS_ERR_NULL_DEST, "%s: dest is null (the reference writes into dest)", name);
    if ((r = check_panel(out, S, T, ld_out, name))) return r;
    if ((r = arima_orders(name, T, p, d, q, &n))) return r;
    if (S > 0 && !coef) return fail(STS_ERR_BAD_ARG, "%s: null coefficients", name);
    if (S * T == 0) return STS_OK;
    if (in == out && ld_in != ld_out) return fail(STS_ERR_BAD_ARG, "%s: in place needs ld_in == ld_out", name);
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    sts::ArimaEffectsArgs a{};
    a.out = out; a.S = S; a.T = T; a.ld_out = ld_out; a.p = p; a.q = q; a.icpt = include_intercept ? 1 : 0;
    a.coef = coef;
    if (!add) {
        ArimaDiff df(st);   // differencesOfOrderD(ts, d), all T values (:476)
        if ((r = df.run(in, S, T, ld_in, d, st))) return r;
        a.in = df.cur; a.ld_in = df.ld;
        HIP_TRY(timed(st, [&] { return sts::launch_arima_effects(sts::kArimaRemove, a, st); }), name);
        return STS_OK;
    }
    a.in = in; a.ld_in = ld_in;
    HIP_TRY(timed(st, [&] { return sts::launch_arima_effects(sts::kArimaAdd, a, st); }), name);
    // inverseDifferencesOfOrderD (:508): inverseDifferencesAtLag(x, x, 1, i) for i = d .. 1
    a.in = out; a.ld_in = ld_out;
    for (int i = d; i >= 1; i--) {
        a.start = i;
        HIP_TRY(sts::launch_arima_effects(sts::kArimaIntegrate, a, st), name);
    }
    return STS_OK;
}

int sts_arima_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int p, int d,
                     int q, int include_intercept, const double* coef, void* stream) {
    return arima_effects(false, in, out, S, T, ld_in, ld_out, p, d, q, include_intercept, coef, stream);
}

int sts_arima_add(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int p, int d,
                  int q, int include_intercept, const double* coef, void* stream) {
    return arima_effects(true, in, out, S, T, ld_in, ld_out, p, d, q, include_intercept, coef, stream);
}

int sts_arima_forecast(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int p, int d,
                       int q, int include_intercept, const double* coef, int n_future, void* stream) {
    const char* name = "ARIMAModel.forecast";
    int r, n = (include_intercept ? 1 : 0) + p + q;
    if (n_future < 0) return fail(STS_ERR_BAD_ARG, "%s: negative nFuture", name);
    const int64_t TO = T + n_future;
    if ((r = check_panel(in, S, T, ld_in, name))) return r;
    if (!out) return fail(STS_ERR_BAD_ARG, "%s: null output", name);
    if ((r = check_panel(out, S, TO, ld_out, name))) return r;
    if ((r = arima_orders(name, T, p, d, q, &n))) return r;
    if (S > 0 && !coef) return fail(STS_ERR_BAD_ARG, "%s: null coefficients", name);
    if (S * TO > 0 && static_cast<const void*>(in) == out) return fail(STS_ERR_BAD_ARG, "%s: out must not alias in", name);
    if (S * TO == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ArimaDiff df(st);
    if ((r = df.run(in, S, T, ld_in, d, st))) return r;
    sts::ArimaForecastArgs a{};
    a.ts = in; a.diffed = df.cur; a.S = S; a.T = T; a.ld_ts = ld_in; a.ld_d = df.ld; a.d = d; a.n_future = n_future;
    a.p = p; a.q = q; a.icpt = include_intercept ? 1 : 0; a.coef = coef;
    if (d == 0) {
        a.out = out; a.ld_out = ld_out;
        HIP_TRY(timed(st, [&] { return sts::launch_arima_forecast(a, st); }), name);
        return STS_OK;
    }
    // d > 0 (:571-603): the raw forecast, then the sums of the difference levels 0 .. d-1, the
    // diagonal of their last d columns, the merge and the inverse differencing of the tail
    Scratch raw(st), sum(st), diag(st), lv0(st), lv1(st);
    HIP_TRY(raw.alloc((size_t)(S * TO) * sizeof(double)), "hipMallocAsync(arima)");
    HIP_TRY(sum.alloc((size_t)(S * T) * sizeof(double)), "hipMallocAsync(arima)");
    HIP_TRY(diag.alloc((size_t)(S * d) * sizeof(double)), "hipMallocAsync(arima)");
    if (d > 1) HIP_TRY(lv0.alloc((size_t)(S * T) * sizeof(double)), "hipMallocAsync(arima)");
    if (d > 2) HIP_TRY(lv1.alloc((size_t)(S * T) * sizeof(double)), "hipMallocAsync(arima)");
    a.out = static_cast<double*>(raw.p); a.ld_out = TO;
    HIP_TRY(timed(st, [&] { return sts::launch_arima_forecast(a, st); }), name);
    const double* level = in;
    int64_t lld = ld_in;
    double* lbufs[2] = {static_cast<double*>(lv0.p), static_cast<double*>(lv1.p)};
    for (int k = 0; k < d; k++) {
        if (k > 0) {   // diffMatrix(k, k to -1) = differencesOfOrderD(diffMatrix(k - 1, k to -1), 1) (:582)
            double* nxt = lbufs[(k - 1) & 1];
            HIP_TRY(sts::launch_diff(level, nxt, S, T, lld, T, 1, k + 1, st), name);
            level = nxt;
            lld = T;
        }
        HIP_TRY(sts::launch_arima_level_sum(level, lld, static_cast<double*>(sum.p), S, T, k == 0, st), name);
        HIP_TRY(sts::launch_arima_diag(level, lld, S, T - d + k, static_cast<double*>(diag.p), d, k, st), name);
    }
    HIP_TRY(sts::launch_arima_forecast_merge(in, ld_in, static_cast<const double*>(sum.p),
                                             static_cast<const double*>(raw.p), static_cast<const double*>(diag.p),
                                             out, ld_out, S, T, d, n_future, st), name);
    sts::ArimaEffectsArgs e{};
    e.in = out + (T - d); e.out = out + (T - d); e.S = S; e.T = d + n_future; e.ld_in = ld_out; e.ld_out = ld_out;
    for (int i = d; i >= 1; i--) {
        e.start = i;
        HIP_TRY(sts::launch_arima_effects(sts::kArimaIntegrate, e, st), name);
    }
    return STS_OK;
}

int sts_fill_diff_ewma(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int method,
                       int lag, const double* smoothing, int32_t* err_per_series, void* stream) {
    int r;
    if ((r = method_ok(method, true, "fill_diff_ewma"))) return r;
    if ((r = check_panel(in, S, T, ld_in, "fill_diff_ewma"))) return r;
    if ((r = check_panel(out, S, T, ld_out, "fill_diff_ewma"))) return r;
    if (lag < 0) return fail(STS_ERR_BAD_ARG, "fill_diff_ewma: negative lag");
    if (S > 0 && !smoothing) return fail(STS_ERR_BAD_ARG, "fill_diff_ewma: null smoothing");
    if (S * T > 0 && in == out) return fail(STS_ERR_BAD_ARG, "fill_diff_ewma: out must not alias in");
    if (S * T == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare())) return r;
    if ((method == STS_FILL_PREVIOUS || method == STS_FILL_NONE) && lag >= 1 && lag <= 32 && method == STS_FILL_PREVIOUS) {
        sts::RecurArgs a{};
        a.in = in; a.out = out; a.S = S; a.T = T; a.ld_in = ld_in; a.ld_out = ld_out; a.sm = smoothing;
        a.lag = lag; a.start = lag; a.method = method;
        HIP_TRY(timed(st, [&] { return sts::launch_recur(sts::kFillDiffEwma, a, st); }), "fill_diff_ewma");
        return es.finish("fill_diff_ewma");
    }
    // general composition: fill (a fresh vector) -> differencesAtLag(filled, lag), which reads
    // the FILLED values (out of place: the reference's (ts, lag) form copies, :384-386) ->
    // EWMA add in place on `out` (dest eq ts is safe for add, S/models/EWMA.scala:135-142)
    const double* F = in;
    int64_t ldF = ld_in;
    Scratch tmp(st);
    if (method != STS_FILL_NONE) {
        double* f = out;
        if (lag > 0) {
            HIP_TRY(tmp.alloc((size_t)(S * T) * sizeof(double)), "hipMallocAsync(filled)");
            f = static_cast<double*>(tmp.p);
        }
        const int64_t ldf = lag > 0 ? T : ld_out;
        if ((r = run_tile(in, f, nullptr, S, T, ld_in, ldf, method, 0, nullptr, 0, 0, es.dev, st, "fill"))) return r;
        F = f;
        ldF = ldf;
    }
    if (lag > 0) {
        HIP_TRY(sts::launch_diff(F, out, S, T, ldF, ld_out, lag, lag, st), "differencesAtLag");
    } else if (F != out) {
        HIP_TRY(hipMemcpy2DAsync(out, ld_out * sizeof(double), F, ldF * sizeof(double), T * sizeof(double), S,
                                 hipMemcpyDeviceToDevice, st), "copy");
    }
    sts::RecurArgs a{};
    a.in = out; a.out = out; a.S = S; a.T = T; a.ld_in = ld_out; a.ld_out = ld_out; a.sm = smoothing;
    HIP_TRY(sts::launch_recur(sts::kEwmaAdd, a, st), "ewma_add");
    return es.finish("fill_diff_ewma");
}

// ---- panel transforms: include/sts_transforms.h (sts_transforms.hip, sts_recur.hip) ----

int sts_quotients(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int lag,
                  int minus_one, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld_in, "quotients"))) return r;
    if (lag < 0 || lag > T) return fail(STS_ERR_BAD_ARG, "quotients: lag %d outside [0, T=%lld]", lag, (long long)T);
    if ((r = check_panel(out, S, T - lag, ld_out, "quotients"))) return r;
    if (S * (T - lag) == 0) return STS_OK;   // lag == T: an empty vector
    if (in == out) return fail(STS_ERR_BAD_ARG, "quotients: out must not alias in");
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_quotients(in, out, S, T, ld_in, ld_out, lag, minus_one != 0, as_stream(stream)), "quotients");
    return STS_OK;
}

int sts_fill_quotients(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int method,
                       int lag, int minus_one, int32_t* err_per_series, void* stream) {
    int r;
    if ((r = method_ok(method, true, "fill_quotients"))) return r;
    if ((r = check_panel(in, S, T, ld_in, "fill_quotients"))) return r;
    if (lag < 0 || lag > T) return fail(STS_ERR_BAD_ARG, "fill_quotients: lag %d outside [0, T=%lld]", lag, (long long)T);
    if ((r = check_panel(out, S, T - lag, ld_out, "fill_quotients"))) return r;
    if (S * (T - lag) > 0 && in == out) return fail(STS_ERR_BAD_ARG, "fill_quotients: out must not alias in");
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    const bool m1 = minus_one != 0;
    if (method == STS_FILL_NONE) {   // r1 itself; no series can fail
        if ((r = es.prepare())) return r;
        HIP_TRY(sts::launch_quotients(in, out, S, T, ld_in, ld_out, lag, m1, st), "quotients");
        return es.finish("fill_quotients");
    }
    if (method == STS_FILL_PREVIOUS && lag >= 1 && lag <= sts::kFillQuotMaxLag) {
        // one pass: fillPrevious has no failing series, and its filled values never leave the wave
        if ((r = es.prepare())) return r;
        HIP_TRY(timed(st, [&] { return sts::launch_fill_prev_quotients(in, out, S, T, ld_in, ld_out, lag, m1, st); }),
                "fill_quotients");
        return es.finish("fill_quotients");
    }
    // composition: fill (a fresh vector) into scratch rows of even pitch, so the fill's 16-byte
    // store forms apply whatever T is, then r1 on it.  The fill runs for lag == T too: its
    // per-series statuses are part of the result.
    if ((r = es.prepare(false))) return r;   // run_tile zeroes err unless its kernel writes all of it
    const int64_t ldf = (T + 1) & ~(int64_t)1;
    Scratch tmp(st);
    HIP_TRY(tmp.alloc((size_t)(S * ldf) * sizeof(double)), "hipMallocAsync(filled)");
    double* f = static_cast<double*>(tmp.p);
    if ((r = run_tile(in, f, nullptr, S, T, ld_in, ldf, method, 0, nullptr, 0, 0, es.dev, st, "fill"))) return r;
    HIP_TRY(sts::launch_quotients(f, out, S, T, ldf, ld_out, lag, m1, st), "quotients");
    return es.finish("fill_quotients");
}

int sts_fill_with_default(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                          double filler, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld_in, "fillWithDefault"))) return r;
    if ((r = check_panel(out, S, T, ld_out, "fillWithDefault"))) return r;
    if (S * T == 0) return STS_OK;
    if (in == out && ld_in != ld_out) return fail(STS_ERR_BAD_ARG, "fillWithDefault: in-place call with different ld");
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_fill_default(in, out, S, T, ld_in, ld_out, filler, as_stream(stream)), "fillWithDefault");
    return STS_OK;
}

int sts_downsample(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int n, int phase,
                   void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld_in, "downsample"))) return r;
    if (n < 1) return fail(STS_ERR_BAD_ARG, "downsample: n = %d must be at least 1", n);
    if (phase < 0) return fail(STS_ERR_BAD_ARG, "downsample: negative phase %d", phase);
    const int64_t To = phase >= T ? 0 : (T - phase + n - 1) / n;   // ceil((T - phase) / n)
    if ((r = check_panel(out, S, To, ld_out, "downsample"))) return r;
    if (S * To == 0) return STS_OK;
    if (in == out) return fail(STS_ERR_BAD_ARG, "downsample: out must not alias in");
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_downsample(in, out, S, To, ld_in, ld_out, n, phase, as_stream(stream)), "downsample");
    return STS_OK;
}

int sts_upsample(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int n, int phase,
                 int use_zero, void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld_in, "upsample"))) return r;
    if (n < 1) return fail(STS_ERR_BAD_ARG, "upsample: n = %d must be at least 1", n);
    if (phase < 0 || phase >= n)
        return fail(STS_ERR_BAD_ARG, "upsample: phase %d outside [0, n=%d): the last value would land past the array",
                    phase, n);
    if ((r = check_panel(out, S, T * n, ld_out, "upsample"))) return r;   // T * n within the Int range too
    if (S * T == 0) return STS_OK;
    if (in == out) return fail(STS_ERR_BAD_ARG, "upsample: out must not alias in");
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_upsample(in, out, S, T * n, ld_in, ld_out, n, phase, use_zero ? 0.0 : (double)NAN,
                                 as_stream(stream)), "upsample");
    return STS_OK;
}

int sts_first_last_not_nan(const double* in, int64_t S, int64_t T, int64_t ld, int64_t* first, int64_t* last,
                           void* stream) {
    int r;
    if ((r = check_panel(in, S, T, ld, "firstNotNaN"))) return r;
    if (S == 0 || (!first && !last)) return STS_OK;
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_first_last(in, S, T, ld, first, last, as_stream(stream)), "firstNotNaN / lastNotNaN");
    return STS_OK;
}

int sts_inverse_diff_at_lag(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int lag,
                            int start, void* stream) {
    int r;
    if (!(start >= lag)) return fail(STS_ERR_REQUIREMENT, "requirement failed: starting index cannot be less than lag");
    if (lag < 0) return fail(STS_ERR_BAD_ARG, "inverseDifferencesAtLag: negative lag %d", lag);
    if ((r = check_panel(in, S, T, ld_in, "inverseDifferencesAtLag"))) return r;
    if ((r = check_panel(out, S, T, ld_out, "inverseDifferencesAtLag"))) return r;
    if (lag == 0 || S * T == 0) return STS_OK;  // dest returned untouched (:404-405)
    if (in == out && ld_in != ld_out)
        return fail(STS_ERR_BAD_ARG, "inverseDifferencesAtLag: in-place call with different ld");
    if ((r = ensure_device())) return r;
    sts::RecurArgs a{};
    a.in = in; a.out = out; a.S = S; a.T = T; a.ld_in = ld_in; a.ld_out = ld_out; a.lag = lag; a.start = start;
    HIP_TRY(sts::launch_recur(sts::kInvDiffAtLag, a, as_stream(stream)), "inverseDifferencesAtLag");
    return STS_OK;
}

// differencesOfOrderD / inverseDifferencesOfOrderD: d <= kOrderDOnePass in one pass (one register
// per level), larger d as the reference's d sweeps
static int order_d(bool inverse, const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                   int d, void* stream) {
    const char* name = inverse ? "inverseDifferencesOfOrderD" : "differencesOfOrderD";
    int r;
    if (d < 0) return fail(STS_ERR_BAD_ARG, "%s: negative order %d", name, d);
    if ((r = check_panel(in, S, T, ld_in, name))) return r;
    if ((r = check_panel(out, S, T, ld_out, name))) return r;
    if (S * T == 0) return STS_OK;
    if (in == out) return fail(STS_ERR_BAD_ARG, "%s: out must not alias in (the reference returns a copy)", name);
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    if (d > T) d = (int)T;   // a sweep whose start index is past the end copies every element
    if (d == 0) {
        HIP_TRY(hipMemcpy2DAsync(out, ld_out * sizeof(double), in, ld_in * sizeof(double), T * sizeof(double), S,
                                 hipMemcpyDeviceToDevice, st), name);
        return STS_OK;
    }
    sts::RecurArgs a{};
    a.in = in; a.out = out; a.S = S; a.T = T; a.ld_in = ld_in; a.ld_out = ld_out;
    if (d <= sts::kOrderDOnePass) {
        a.p = d;
        HIP_TRY(sts::launch_recur(inverse ? sts::kInvDiffOrderD : sts::kDiffOrderD, a, st), name);
        return STS_OK;
    }
    if (inverse) {   // addedTs = diffedTs.copy, then the sweeps i = d..1 in place
        HIP_TRY(hipMemcpy2DAsync(out, ld_out * sizeof(double), in, ld_in * sizeof(double), T * sizeof(double), S,
                                 hipMemcpyDeviceToDevice, st), name);
        a.in = out; a.ld_in = ld_out; a.lag = 1;
        for (int i = d; i >= 1; i--) {
            a.start = i;
            HIP_TRY(sts::launch_recur(sts::kInvDiffAtLag, a, st), name);
        }
        return STS_OK;
    }
    // the reference's ping-pong: sweep i reads the buffer sweep i - 1 wrote; the last one writes out
    const int64_t ldf = (T + 1) & ~(int64_t)1;
    Scratch tmp(st);
    HIP_TRY(tmp.alloc((size_t)(S * ldf) * sizeof(double)), "hipMallocAsync(order-d scratch)");
    double* f = static_cast<double*>(tmp.p);
    const double* src = in;
    int64_t ld_src = ld_in;
    for (int i = 1; i <= d; i++) {
        const bool to_out = (d - i) % 2 == 0;
        double* dst = to_out ? out : f;
        const int64_t ld_dst = to_out ? ld_out : ldf;
        HIP_TRY(sts::launch_diff(src, dst, S, T, ld_src, ld_dst, 1, i, st), name);
        src = dst;
        ld_src = ld_dst;
    }
    return STS_OK;
}

int sts_diff_order_d(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int d,
                     void* stream) {
    return order_d(false, in, out, S, T, ld_in, ld_out, d, stream);
}

int sts_inverse_diff_order_d(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int d,
                             void* stream) {
    return order_d(true, in, out, S, T, ld_in, ld_out, d, stream);
}

// ---- statistical tests: S/stats/TimeSeriesStatisticalTests.scala (sts_stattests.hip) ----

int sts_regression_from_name(const char* name) {
    if (!name) return -2;
    if (!std::strcmp(name, "nc")) return STS_REG_NC;
    if (!std::strcmp(name, "c")) return STS_REG_C;
    if (!std::strcmp(name, "ct")) return STS_REG_CT;
    if (!std::strcmp(name, "ctt")) return STS_REG_CTT;
    return -2;
}

static int stat_panel(const double* in, int64_t S, int64_t T, int64_t ld, const double* stat, const char* name) {
    int r;
    if ((r = check_panel(in, S, T, ld, name))) return r;
    if (S > 0 && !stat) return fail(STS_ERR_BAD_ARG, "%s: null output", name);
    if (S > 0x7fffffffLL) return fail(STS_ERR_BAD_ARG, "%s: panel too large for one launch", name);
    return STS_OK;
}

int sts_dw_test(const double* in, int64_t S, int64_t T, int64_t ld, double* stat, void* stream) {
    int r;
    if ((r = stat_panel(in, S, T, ld, stat, "dwtest"))) return r;
    if (T < 1) return fail(STS_ERR_BAD_ARG, "dwtest: empty series (residuals(0) does not exist)");
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    sts::StatArgs a{};
    a.in = in; a.S = S; a.T = T; a.ld = ld; a.stat = stat;
    HIP_TRY(timed(st, [&] { return sts::launch_dw(a, st); }), "dwtest");
    return STS_OK;
}

int sts_kpss_test(const double* in, int64_t S, int64_t T, int64_t ld, int regression, double* stat, void* stream) {
    int r;
    if (regression != STS_REG_C && regression != STS_REG_CT)
        return fail(STS_ERR_REQUIREMENT, "requirement failed: trend must be c or ct");
    if ((r = stat_panel(in, S, T, ld, stat, "kpsstest"))) return r;
    if (T <= regression)
        return fail(STS_ERR_NOT_ENOUGH_DATA, "kpsstest: not enough data (%lld rows) for the number of predictors (%d)",
                    (long long)T, regression);
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    sts::StatArgs a{};
    a.in = in; a.S = S; a.T = T; a.ld = ld; a.stat = stat; a.q = regression;
    a.L = (int)(3 * std::sqrt((double)T) / 13);   // :380, R tseries' default
    HIP_TRY(timed(st, [&] { return sts::launch_kpss(a, st); }), "kpsstest");
    return STS_OK;
}

int sts_adf_test(const double* in, int64_t S, int64_t T, int64_t ld, int max_lag, int regression, double* stat,
                 double* pvalue, int32_t* err_per_series, void* stream) {
    int r;
    if (regression < STS_REG_NC || regression > STS_REG_CTT)
        return fail(STS_ERR_BAD_ARG, "adftest: regression %d is not nc, c, ct or ctt", regression);
    if (max_lag < 0 || max_lag > 31) return fail(STS_ERR_BAD_ARG, "adftest: maxLag %d outside [0, 31]", max_lag);
    if ((r = stat_panel(in, S, T, ld, stat, "adftest"))) return r;
    const int64_t n_obs = T - 1 - max_lag, k = 1 + max_lag + regression;
    if (n_obs <= k)
        return fail(STS_ERR_NOT_ENOUGH_DATA, "adftest: not enough data (%lld rows) for the number of predictors (%lld)",
                    (long long)n_obs, (long long)k);
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare())) return r;
    sts::StatArgs a{};
    a.in = in; a.S = S; a.T = T; a.ld = ld; a.stat = stat; a.err = es.dev; a.p = max_lag; a.q = regression;
    HIP_TRY(timed(st, [&] { return sts::launch_adf(a, st); }), "adftest");
    if (pvalue) HIP_TRY(sts::launch_adf_pvalue(stat, pvalue, S, regression, st), "adftest (p-value)");
    return es.finish("adftest");
}

int sts_lb_test(const double* in, int64_t S, int64_t T, int64_t ld, int max_lag, double* stat, double* pvalue,
                void* stream) {
    int r;
    if (max_lag < 1) return fail(STS_ERR_BAD_ARG, "lbtest: maxLag %d < 1", max_lag);
    if ((r = stat_panel(in, S, T, ld, stat, "lbtest"))) return r;
    if (T < 1) return fail(STS_ERR_BAD_ARG, "lbtest: empty series");
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    // autocorr(residuals, maxLag) into a stream-ordered S x K scratch (a device status array keeps
    // the ACF call from synchronising), then the epilogue
    Scratch sc(st);
    const size_t nacf = (size_t)S * (size_t)max_lag;
    HIP_TRY(sc.alloc(nacf * sizeof(double) + (size_t)S * sizeof(int32_t)), "hipMallocAsync(lbtest)");
    double* acf = static_cast<double*>(sc.p);
    int32_t* err = reinterpret_cast<int32_t*>(acf + nacf);
    if ((r = sts_fill_autocorr(in, nullptr, S, T, ld, ld, STS_FILL_NONE, max_lag, acf, err, st))) return r;
    HIP_TRY(timed(st, [&] { return sts::launch_lb(acf, S, T, max_lag, stat, pvalue, st); }), "lbtest");
    return STS_OK;
}

// the factor panel of bgtest / bptest and of t5 / t6: k, ld_f, fs and the pointer
static int factor_panel(const double* factors, int64_t S, int64_t T, int k, int64_t ld_f, int64_t fs, const char* name) {
    if (k < 1 || k > sts::kMaxFactors)
        return fail(STS_ERR_BAD_ARG, "%s: %d factors outside [1, %d]", name, k, sts::kMaxFactors);
    if (ld_f < T)
        return fail(STS_ERR_BAD_ARG, "%s: factor leading dimension %lld < T=%lld", name, (long long)ld_f, (long long)T);
    if (fs != 0 && fs < (int64_t)(k - 1) * ld_f + T)
        return fail(STS_ERR_BAD_ARG, "%s: factor series stride %lld overlaps (needs 0 or >= %lld)", name, (long long)fs,
                    (long long)((int64_t)(k - 1) * ld_f + T));
    if (S * T > 0 && !factors) return fail(STS_ERR_BAD_ARG, "%s: null factor pointer", name);
    return STS_OK;
}

static int bgbp_test(bool bp, const double* resid, int64_t S, int64_t T, int64_t ld, const double* factors, int k,
                     int64_t ld_f, int64_t fs, int max_lag, double* stat, double* pvalue, int32_t* err_per_series,
                     void* stream) {
    const char* name = bp ? "bptest" : "bgtest";
    int r;
    if ((r = factor_panel(factors, S, T, k, ld_f, fs, name))) return r;
    if (!bp && (max_lag < 1 || max_lag > 31)) return fail(STS_ERR_BAD_ARG, "bgtest: maxLag %d outside [1, 31]", max_lag);
    if ((r = stat_panel(resid, S, T, ld, stat, name))) return r;
    const int L = bp ? 0 : max_lag;
    const int64_t n_obs = T - L, cols = 1 + (int64_t)k + L;
    if (n_obs <= cols)
        return fail(STS_ERR_NOT_ENOUGH_DATA, "%s: not enough data (%lld rows) for the number of predictors (%lld)", name,
                    (long long)n_obs, (long long)cols);
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare())) return r;
    sts::BgBpArgs a{};
    a.in = resid; a.S = S; a.T = T; a.ld = ld; a.L = L; a.squares = bp; a.stat = stat; a.err = es.dev;
    a.f.factors = factors; a.f.ld_f = ld_f; a.f.fs = fs; a.f.k = k; a.f.lo = L; a.f.n = n_obs;
    if ((r = over_factor_bases(a.f, S, sts::own_basis(a), 0, st, name,
                               [&](int64_t s0, int64_t ns) { return sts::launch_bgbp(a, s0, ns, st); })))
        return r;
    if (pvalue) HIP_TRY(sts::launch_chi2_pvalue(stat, pvalue, S, bp ? k : L, st), name);
    return es.finish(name);
}

int sts_bp_test(const double* resid, int64_t S, int64_t T, int64_t ld, const double* factors, int k, int64_t ld_f,
                int64_t fs, double* stat, double* pvalue, int32_t* err_per_series, void* stream) {
    return bgbp_test(true, resid, S, T, ld, factors, k, ld_f, fs, 0, stat, pvalue, err_per_series, stream);
}

int sts_bg_test(const double* resid, int64_t S, int64_t T, int64_t ld, const double* factors, int k, int64_t ld_f,
                int64_t fs, int max_lag, double* stat, double* pvalue, int32_t* err_per_series, void* stream) {
    return bgbp_test(false, resid, S, T, ld, factors, k, ld_f, fs, max_lag, stat, pvalue, err_per_series, stream);
}

// ---- include/sts_regress.h ----

// g1
int sts_factor_ols(const double* y, int64_t S, int64_t T, int64_t ld, const double* factors, int k, int64_t ld_f,
                   int64_t fs, double* beta, int64_t ld_b, double* stderr_out, double* stats, double* resid, int64_t ld_r,
                   int32_t* err_per_series, void* stream) {
    const char* name = "factor_ols";
    int r;
    if ((r = factor_panel(factors, S, T, k, ld_f, fs, name))) return r;
    if ((r = stat_panel(y, S, T, ld, beta, name))) return r;
    if (ld_b < (int64_t)k + 1)
        return fail(STS_ERR_BAD_ARG, "%s: coefficient leading dimension %lld < k + 1 = %d", name, (long long)ld_b, k + 1);
    if (resid && ld_r < T)
        return fail(STS_ERR_BAD_ARG, "%s: residual leading dimension %lld < T=%lld", name, (long long)ld_r, (long long)T);
    if (resid && resid == y && S > 0) return fail(STS_ERR_BAD_ARG, "%s: resid must not alias y", name);
    if (T <= (int64_t)k + 1)
        return fail(STS_ERR_NOT_ENOUGH_DATA, "%s: not enough data (%lld rows) for the number of predictors (%d)", name,
                    (long long)T, k + 1);
    if (S == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    ErrSink es(err_per_series, S, st);
    if ((r = es.prepare())) return r;
    sts::OlsArgs a{};
    a.y = y; a.S = S; a.T = T; a.ld = ld;
    a.f.factors = factors; a.f.ld_f = ld_f; a.f.fs = fs; a.f.k = k; a.f.n = T;
    a.beta = beta; a.se = stderr_out; a.ld_b = ld_b; a.stats = stats; a.resid = resid; a.ld_r = ld_r; a.err = es.dev;
    if ((r = over_factor_bases(a.f, S, sts::ols_regime(T, k, fs) == 2, sts::kOlsAux, st, name,
                               [&](int64_t s0, int64_t ns) { return sts::launch_ols(a, s0, ns, st); })))
        return r;
    return es.finish(name);
}

// g2
static int factor_effects(bool add, const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                          const double* factors, int k, int64_t ld_f, int64_t fs, const double* beta, int64_t ld_b,
                          void* stream) {
    const char* name = add ? "factor_add" : "factor_remove";
    int r;
    if ((r = factor_panel(factors, S, T, k, ld_f, fs, name))) return r;
    if ((r = check_panel(in, S, T, ld_in, name))) return r;
    if ((r = check_panel(out, S, T, ld_out, name))) return r;
    if (ld_b < (int64_t)k + 1)
        return fail(STS_ERR_BAD_ARG, "%s: coefficient leading dimension %lld < k + 1 = %d", name, (long long)ld_b, k + 1);
    if (S > 0 && !beta) return fail(STS_ERR_BAD_ARG, "%s: null coefficient pointer", name);
    if (S * T == 0) return STS_OK;
    if (in == out && ld_in != ld_out) return fail(STS_ERR_BAD_ARG, "%s: in-place call with different ld", name);
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_factor_effects(add, in, out, S, T, ld_in, ld_out, factors, k, ld_f, fs, beta, ld_b,
                                       as_stream(stream)), name);
    return STS_OK;
}

int sts_factor_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                      const double* factors, int k, int64_t ld_f, int64_t fs, const double* beta, int64_t ld_b,
                      void* stream) {
    return factor_effects(false, in, out, S, T, ld_in, ld_out, factors, k, ld_f, fs, beta, ld_b, stream);
}

int sts_factor_add(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                   const double* factors, int k, int64_t ld_f, int64_t fs, const double* beta, int64_t ld_b,
                   void* stream) {
    return factor_effects(true, in, out, S, T, ld_in, ld_out, factors, k, ld_f, fs, beta, ld_b, stream);
}

// ---- include/sts_cross.h ----

int sts_cross_kind_from_name(const char* name) {
    if (!name) return -2;
    if (!std::strcmp(name, "cov")) return STS_CROSS_COV;
    if (!std::strcmp(name, "corr")) return STS_CROSS_CORR;
    return -2;
}

// do the S x w block at a (rows ld apart) and the S_b x w_b block at b share a byte?  Extents only:
// a block is taken as the one range from its first to its last element.
static bool blocks_overlap(const double* a, int64_t S, int64_t ld, int64_t w, const double* b, int64_t S_b, int64_t ld_b,
                           int64_t w_b) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    const uintptr_t a1 = a0 + ((uintptr_t)(S - 1) * (uintptr_t)ld + (uintptr_t)w) * sizeof(double);
    const uintptr_t b1 = b0 + ((uintptr_t)(S_b - 1) * (uintptr_t)ld_b + (uintptr_t)w_b) * sizeof(double);
    return a0 < b1 && b0 < a1;
}

// c1.  Scratch: kCrossStat doubles per series of either panel, and in a split plan (cross_plan) the
// (tile, segment) partials.
int sts_cross_moments(const double* x, int64_t Sx, int64_t T, int64_t ld_x, const double* y, int64_t Sy, int64_t ld_y,
                      int kind, double* out, int64_t ld_o, double* mean_x, double* mean_y, void* stream) {
    const char* name = "cross_moments";
    if (!x || !out) return fail(STS_ERR_BAD_ARG, "%s: null %s pointer", name, !x ? "panel" : "output");
    if (Sx < 1) return fail(STS_ERR_BAD_ARG, "%s: Sx=%lld < 1", name, (long long)Sx);
    if (y && Sy < 1) return fail(STS_ERR_BAD_ARG, "%s: Sy=%lld < 1", name, (long long)Sy);
    if (T < 0 || T > 0x7fffffffLL)
        return fail(STS_ERR_BAD_ARG, "%s: T=%lld outside the reference's Int index range", name, (long long)T);
    if (ld_x < T) return fail(STS_ERR_BAD_ARG, "%s: leading dimension %lld < T=%lld", name, (long long)ld_x, (long long)T);
    if (y && ld_y < T)
        return fail(STS_ERR_BAD_ARG, "%s: leading dimension of y %lld < T=%lld", name, (long long)ld_y, (long long)T);
    const int64_t cols = y ? Sy : Sx;
    if (ld_o < cols)
        return fail(STS_ERR_BAD_ARG, "%s: output leading dimension %lld < %lld columns", name, (long long)ld_o,
                    (long long)cols);
    if (kind != STS_CROSS_COV && kind != STS_CROSS_CORR) return fail(STS_ERR_BAD_ARG, "%s: kind %d is not cov or corr", name, kind);
    if (mean_y && !y) return fail(STS_ERR_BAD_ARG, "%s: mean_y without y", name);
    const int64_t w = T > 0 ? T : 1;
    if (blocks_overlap(out, Sx, ld_o, cols, x, Sx, ld_x, w) || (y && blocks_overlap(out, Sx, ld_o, cols, y, Sy, ld_y, w)))
        return fail(STS_ERR_BAD_ARG, "%s: out overlaps an input panel", name);
    if (T < 2) return fail(STS_ERR_NOT_ENOUGH_DATA, "%s: %lld instants, a covariance needs 2", name, (long long)T);
    const sts::CrossPlan plan = sts::cross_plan(Sx, cols, T, y == nullptr);
    if (plan.tiles > 0x7fffffffLL)
        return fail(STS_ERR_BAD_ARG, "%s: %lld x %lld outputs exceed one launch", name, (long long)Sx, (long long)cols);
    int r;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    Scratch sc(st);
    HIP_TRY(sc.alloc(plan.scratch_doubles * sizeof(double)), "hipMallocAsync(cross scratch)");
    sts::CrossArgs a{};
    a.x = x; a.y = y; a.Sx = Sx; a.Sy = cols; a.T = T; a.ld_x = ld_x; a.ld_y = y ? ld_y : ld_x; a.kind = kind;
    a.out = out; a.ld_o = ld_o; a.mean_x = mean_x; a.mean_y = mean_y;
    a.scratch = static_cast<double*>(sc.p);
    HIP_TRY(timed(st, [&] { return sts::launch_cross(a, st); }), name);
    return STS_OK;
}

// ---- include/sts_roll.h ----

int sts_roll_op_from_name(const char* name) {
    static const char* const names[] = {"sum", "mean", "var", "std", "min", "max", "zscore"};
    if (!name) return -2;
    for (int i = 0; i < 7; i++)
        if (!std::strcmp(name, names[i])) return i;
    return -2;
}

int sts_roll_pair_op_from_name(const char* name) {
    static const char* const names[] = {"cov", "corr", "beta"};
    if (!name) return -2;
    for (int i = 0; i < 3; i++)
        if (!std::strcmp(name, names[i])) return i;
    return -2;
}

// r1 / r2: the guards both share, in the header's order; y == nullptr for r1.  No scratch: every
// launch reads the inputs and writes out.
static int roll_call(const char* name, const double* x, const double* y, int64_t Sy, int64_t ld_y, double* out, int64_t S,
                     int64_t T, int64_t ld_x, int64_t ld_out, int window, int min_periods, int op, bool pair, void* stream) {
    if (!x || !out || (pair && !y))
        return fail(STS_ERR_BAD_ARG, "%s: null %s pointer", name, !x ? "panel" : !out ? "output" : "y");
    if (S < 1 || T < 1) return fail(STS_ERR_BAD_ARG, "%s: empty panel (S=%lld, T=%lld)", name, (long long)S, (long long)T);
    if (T > 0x7fffffffLL)
        return fail(STS_ERR_BAD_ARG, "%s: T=%lld exceeds the reference's Int index range", name, (long long)T);
    if (ld_x < T || ld_out < T)
        return fail(STS_ERR_BAD_ARG, "%s: leading dimension %lld < T=%lld", name, (long long)(ld_x < T ? ld_x : ld_out),
                    (long long)T);
    if (window < 1 || window > STS_ROLL_MAX_WINDOW)
        return fail(STS_ERR_BAD_ARG, "%s: window %d outside [1, %d]", name, window, STS_ROLL_MAX_WINDOW);
    if (min_periods < 1 || min_periods > window)
        return fail(STS_ERR_BAD_ARG, "%s: min_periods %d outside [1, window=%d]", name, min_periods, window);
    if (op < 0 || op > (pair ? (int)STS_ROLL_BETA : (int)STS_ROLL_ZSCORE))
        return fail(STS_ERR_BAD_ARG, "%s: op %d is not one of the header's", name, op);
    if (pair) {
        if (Sy != 1 && Sy != S) return fail(STS_ERR_BAD_ARG, "%s: Sy=%lld is neither 1 nor S=%lld", name, (long long)Sy, (long long)S);
        if (Sy != 1 && ld_y < T)
            return fail(STS_ERR_BAD_ARG, "%s: leading dimension of y %lld < T=%lld", name, (long long)ld_y, (long long)T);
    }
    if (blocks_overlap(out, S, ld_out, T, x, S, ld_x, T) ||
        (pair && blocks_overlap(out, S, ld_out, T, y, Sy, Sy == 1 ? T : ld_y, T)))
        return fail(STS_ERR_BAD_ARG, "%s: out overlaps an input panel", name);
    int r;
    if ((r = ensure_device())) return r;
    sts::RollArgs a{};
    a.x = x; a.y = y; a.out = out; a.S = S; a.T = T; a.ld_x = ld_x; a.ld_y = pair && Sy != 1 ? ld_y : 0; a.ld_out = ld_out;
    a.window = window; a.min_periods = min_periods; a.op = op; a.pair = pair;
    HIP_TRY(sts::launch_roll(a, as_stream(stream)), name);
    return STS_OK;
}

int sts_roll_stat(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int window,
                  int min_periods, int op, void* stream) {
    return roll_call("roll_stat", in, nullptr, 0, 0, out, S, T, ld_in, ld_out, window, min_periods, op, false, stream);
}

int sts_roll_pair(const double* x, const double* y, int64_t Sy, int64_t ld_y, double* out, int64_t S, int64_t T,
                  int64_t ld_x, int64_t ld_out, int window, int min_periods, int op, void* stream) {
    return roll_call("roll_pair", x, y, Sy, ld_y, out, S, T, ld_x, ld_out, window, min_periods, op, true, stream);
}

int sts_gen_panel(double* out, int64_t s0, int64_t S, int64_t T, int64_t ld, uint64_t seed, double nan_p,
                  void* stream) {
    int r;
    if ((r = check_panel(out, S, T, ld, "gen_panel"))) return r;
    if ((r = ensure_device())) return r;
    uint32_t thr = 0;
    if (nan_p >= 1.0) thr = 0xFFFFFFFFu;
    else if (nan_p > 0.0) thr = (uint32_t)std::floor(nan_p * 4294967296.0);
    HIP_TRY(sts::launch_gen_panel(out, s0, S, T, ld, seed, thr, as_stream(stream)), "gen_panel");
    return STS_OK;
}

int sts_gen_ar_panel(double* out, double* c, double* phi, int64_t s0, int64_t S, int64_t T, int64_t ld, uint64_t seed,
                     int p, void* stream) {
    int r;
    if ((r = check_panel(out, S, T, ld, "gen_ar_panel"))) return r;
    if (p < 1 || p > 32) return fail(STS_ERR_BAD_ARG, "gen_ar_panel: order %d outside [1, 32]", p);
    if (S > 0 && (!c || !phi)) return fail(STS_ERR_BAD_ARG, "gen_ar_panel: null parameter outputs");
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_gen_ar(out, c, phi, s0, S, T, ld, seed, p, as_stream(stream)), "gen_ar_panel");
    return STS_OK;
}

// ---- samplers: include/sts_sample.h (sts_sample.hip) ----

// the arguments every sampler shares
static int sample_args(const double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, int64_t t0, const char* name) {
    int r;
    if ((r = check_panel(out, S, n, ld, name))) return r;
    if (s0 < 0 || t0 < 0)
        return fail(STS_ERR_BAD_ARG, "%s: negative first series (s0=%lld) or stream position (t0=%lld)", name,
                    (long long)s0, (long long)t0);
    return STS_OK;
}

static sts::SampleArgs sample_call(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, int64_t t0,
                                   uint64_t seed) {
    sts::SampleArgs a{};
    a.out = out; a.s0 = s0; a.S = S; a.n = n; a.ld = ld; a.t0 = t0; a.seed = seed;
    return a;
}

int sts_sample_normal(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, int64_t t0, uint64_t seed,
                      void* stream) {
    int r;
    if ((r = sample_args(out, s0, S, n, ld, t0, "sample_normal"))) return r;
    if (S * n == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    const sts::SampleArgs a = sample_call(out, s0, S, n, ld, t0, seed);
    HIP_TRY(timed(st, [&] { return sts::launch_sample_normal(a, st); }), "sample_normal");
    return STS_OK;
}

static int garch_sample(bool ar, double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, const double* c,
                        const double* phi, const double* omega, const double* alpha, const double* beta, int64_t t0,
                        uint64_t seed, void* stream, const char* name) {
    int r;
    if ((r = sample_args(out, s0, S, n, ld, t0, name))) return r;
    if (S > 0 && (!omega || !alpha || !beta || (ar && (!c || !phi))))
        return fail(STS_ERR_BAD_ARG, "%s: null model parameters", name);
    if (S * n == 0) return STS_OK;
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    sts::SampleArgs a = sample_call(out, s0, S, n, ld, t0, seed);
    a.c = c; a.phi = phi; a.omega = omega; a.alpha = alpha; a.beta = beta;
    HIP_TRY(timed(st, [&] { return sts::launch_garch_sample(ar, a, st); }), name);
    return STS_OK;
}

int sts_garch_sample(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, const double* omega,
                     const double* alpha, const double* beta, int64_t t0, uint64_t seed, void* stream) {
    return garch_sample(false, out, s0, S, n, ld, nullptr, nullptr, omega, alpha, beta, t0, seed, stream,
                        "GARCHModel.sample");
}

int sts_argarch_sample(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, const double* c, const double* phi,
                       const double* omega, const double* alpha, const double* beta, int64_t t0, uint64_t seed,
                       void* stream) {
    return garch_sample(true, out, s0, S, n, ld, c, phi, omega, alpha, beta, t0, seed, stream, "ARGARCHModel.sample");
}

// sample = addTimeDependentEffects(vec, vec) of the draws: the add entry point validates its own
// arguments first (validate-only, no device), then the draws and the in-place add share the stream
static int sample_then_add(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, int64_t t0, uint64_t seed,
                           void* stream, const char* name, const std::function<int()>& add) {
    int r;
    if ((r = sample_args(out, s0, S, n, ld, t0, name))) return r;
    if (!out) return STS_OK;   // an empty panel may come without a buffer (sts_arima_add insists on a dest)
    bool has_work = false;
    if ((r = sts::validate([&] { return add(); }, &has_work))) return r;
    if (!has_work) return STS_OK;
    if ((r = sts_sample_normal(out, s0, S, n, ld, t0, seed, stream))) return r;
    return add();
}

int sts_ar_sample(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, const double* c, const double* coef,
                  int p, int64_t t0, uint64_t seed, void* stream) {
    return sample_then_add(out, s0, S, n, ld, t0, seed, stream, "ARModel.sample",
                           [&] { return sts_ar_add(out, out, S, n, ld, ld, c, coef, p, stream); });
}

int sts_arima_sample(double* out, int64_t s0, int64_t S, int64_t n, int64_t ld, int p, int d, int q,
                     int include_intercept, const double* coef, int64_t t0, uint64_t seed, void* stream) {
    return sample_then_add(out, s0, S, n, ld, t0, seed, stream, "ARIMAModel.sample", [&] {
        return sts_arima_add(out, out, S, n, ld, ld, p, d, q, include_intercept, coef, stream);
    });
}

// ---- date-time indices and rebasing: include/sts_index.h (sts_index.hip, sts_index.hpp) ----

// the index every lookup shares: a validated uniform index in *u, or the irregular form's checks
static int index_args(int kind, int64_t start_ms, int64_t periods, int step, const int64_t* instants,
                      int64_t n_instants, sts::ix::Uniform* u, const char* name) {
    if (kind == STS_INDEX_IRREGULAR) {
        if (n_instants < 0) return fail(STS_ERR_BAD_ARG, "%s: negative index size %lld", name, (long long)n_instants);
        if (n_instants > 0 && !instants) return fail(STS_ERR_BAD_ARG, "%s: null instants", name);
        return STS_OK;
    }
    const char* why = sts::ix::make_uniform(kind, start_ms, periods, step, u);
    if (why)
        return fail(STS_ERR_BAD_ARG, "%s: %s (kind=%d, start=%lld, periods=%lld, step=%d)", name, why, kind,
                    (long long)start_ms, (long long)periods, step);
    return STS_OK;
}

int sts_index_instants(int kind, int64_t start_ms, int64_t periods, int step, const int64_t* instants,
                       int64_t n_instants, int64_t* out, void* stream) {
    int r;
    sts::ix::Uniform u{};
    if ((r = index_args(kind, start_ms, periods, step, instants, n_instants, &u, "toMillisArray"))) return r;
    const int64_t n = kind == STS_INDEX_IRREGULAR ? n_instants : periods;
    if (n == 0) return STS_OK;
    if (!out) return fail(STS_ERR_BAD_ARG, "toMillisArray: null output");
    if ((r = ensure_device())) return r;
    hipStream_t st = as_stream(stream);
    if (kind == STS_INDEX_IRREGULAR)
        HIP_TRY(hipMemcpyAsync(out, instants, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st), "toMillisArray");
    else
        HIP_TRY(sts::launch_index_instants(u, out, st), "toMillisArray");
    return STS_OK;
}

int sts_index_locs(const int64_t* millis, int64_t n, int kind, int64_t start_ms, int64_t periods, int step,
                   const int64_t* instants, int64_t n_instants, int64_t* loc, void* stream) {
    int r;
    sts::ix::Uniform u{};
    if (n < 0) return fail(STS_ERR_BAD_ARG, "locAtDateTime: negative count %lld", (long long)n);
    if ((r = index_args(kind, start_ms, periods, step, instants, n_instants, &u, "locAtDateTime"))) return r;
    if (n == 0) return STS_OK;
    if (!millis || !loc) return fail(STS_ERR_BAD_ARG, "locAtDateTime: null timestamps or output");
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_index_locs(millis, n, kind == STS_INDEX_IRREGULAR ? nullptr : &u, instants, n_instants, loc,
                                   as_stream(stream)), "locAtDateTime");
    return STS_OK;
}

int sts_rebase_shift(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                     int64_t ld_out, int64_t start_loc, double default_value, void* stream) {
    int r;
    if ((r = check_panel(in, S, T_in, ld_in, "rebase"))) return r;
    if ((r = check_panel(out, S, T_out, ld_out, "rebase"))) return r;
    if (S * T_out == 0) return STS_OK;
    if (in == out) return fail(STS_ERR_BAD_ARG, "rebase: out must not alias in");
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_rebase_shift(in, out, S, T_in, T_out, ld_in, ld_out, start_loc, default_value,
                                     as_stream(stream)), "rebase");
    return STS_OK;
}

int sts_rebase_map(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                   int64_t ld_out, const int64_t* map, double default_value, void* stream) {
    int r;
    if ((r = check_panel(in, S, T_in, ld_in, "rebase"))) return r;
    if ((r = check_panel(out, S, T_out, ld_out, "rebase"))) return r;
    if (S * T_out == 0) return STS_OK;
    if (!map) return fail(STS_ERR_BAD_ARG, "rebase: null map");
    if (in == out) return fail(STS_ERR_BAD_ARG, "rebase: out must not alias in");
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_rebase_map(in, out, S, T_in, T_out, ld_in, ld_out, map, default_value, as_stream(stream)),
            "rebase");
    return STS_OK;
}

int sts_align_uniform(const double* values, const int64_t* offsets, const int64_t* start_loc, int64_t S,
                      int64_t T_out, double* out, int64_t ld_out, double default_value, void* stream) {
    int r;
    if ((r = check_panel(out, S, T_out, ld_out, "timeSeriesRDD"))) return r;
    if (S * T_out == 0) return STS_OK;
    if (!offsets || !start_loc) return fail(STS_ERR_BAD_ARG, "timeSeriesRDD: null offsets or start locations");
    if ((r = ensure_device())) return r;
    HIP_TRY(sts::launch_align_uniform(values, offsets, start_loc, S, T_out, out, ld_out, default_value,
                                      as_stream(stream)), "timeSeriesRDD");
    return STS_OK;
}

}  // extern "C"
