// sts_host.cpp -- host-buffer entry points (the JNI path): a PINNED
// STAGING PIPELINE in front of the device entry points.
//
// A `_host` call is split by series into chunks of ~kChunkBytes of device traffic.  Each
// chunk runs H2D -> kernel(s) -> D2H on one of kSlots slots, each slot owning a HIP stream,
// a device buffer and pinned bounce buffers, all reused across calls.  While chunk i's
// kernel runs, later chunks upload and earlier ones download (one stream per slot), and the calling
// thread fills the next slot's bounce buffer: copy, compute and the CPU side overlap.
//
// Host memory that is already pinned (hipHostMalloc'd, e.g. by sts_host_alloc -- the JNI
// shim copies a Java array straight into such a buffer with GetDoubleArrayRegion) is moved
// by DMA directly, with no bounce copy; pageable memory goes through the slot's pinned
// buffer (one CPU copy, the same one hipMemcpy would make internally, but overlapped).
//
// One description per call.  A `_host` wrapper lists its per-series arrays (Arg) once and writes
// its device call once, against a Call; staged() runs that call first in validate-only mode
// (sts::validate) on the caller's host pointers, S and ld -- so every argument check, its order
// and its message are the device entry point's own, and a call the entry point answers before any
// device action (an empty panel, lag 0) stages nothing -- and then once per chunk on the chunk's
// device regions.  An output whose host pointer is an input's (an in-place call) shares that
// input's device region; an argument passed as NULL is NULL on the device too.
//
// Every device entry point runs on the slot's stream; per-series statuses always go to a
// device array and come back with the chunk, so a NULL err_per_series keeps the reference's
// exception semantics (the first failing series becomes the return status after all
// chunks) without a synchronisation per chunk.
//
// Reentrancy and memory (round 3).  A call BORROWS a whole slot set from a process-wide pool
// (sts_stage_pool.hpp) for its duration: at most sts_staging_set_limit() sets per device
// (default kDefaultSets = 4, i.e. at most 4 x 5 x 64 MB of HBM and as much pinned memory
// however many executor threads call), a call finding every set borrowed waits for one, and
// nothing is owned by a thread, so retired threads leak nothing.  A call never returns while
// a transfer of its own is in flight: every exit path (success, a HIP error in the middle of
// the pipeline, a failing kernel) drains the set's busy slots first, and a slot whose kernel
// or copy-out did not run is never copied to the caller.  sts_staging_release frees the idle
// sets.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "sts_internal.hpp"
#include "sts_stage_pool.hpp"

namespace {

// Pipeline shape (A/B on C2 from pinned host memory, profiles/r02_v6_ab_staging.jsonl): 2-D
// copies on 5 slots 78 ms per call, 3 slots 87 ms, 4 slots 94 ms; linear copies for
// contiguous rows were bimodal run to run (56-112 ms), so the 2-D form stays.
#ifndef STS_STAGE_SLOTS
#define STS_STAGE_SLOTS 5
#define STS_STAGE_MB 64
#endif
constexpr int kSlots = STS_STAGE_SLOTS;
constexpr size_t kChunkBytes = size_t(STS_STAGE_MB) << 20;   // device bytes (in + out) per chunk
constexpr size_t kAlign = 256;
constexpr int kDefaultSets = 4;                                // slot sets per device (sts_staging_set_limit)
constexpr size_t kMaxArgs = 16;                                // per-series arrays of one call (staged() checks)
// what a slot keeps between calls: one chunk plus the per-argument alignment; a call whose single
// series is larger than a chunk grows its slots for that call only (Borrow trims them again)
constexpr size_t kSlotKeep = kChunkBytes + kMaxArgs * kAlign;

size_t align_up(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

struct Slot {
    hipStream_t st = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // before H2D, after H2D, after kernel, after D2H
    void* dev = nullptr;
    size_t dev_cap = 0;
    void* pin = nullptr;
    size_t pin_cap = 0;
    bool busy = false;       // ev[3] recorded for a chunk not yet reaped
    bool copy_out = false;   // its kernel and D2H copies were enqueued: pageable outputs may be copied
    int64_t s0 = 0, ns = 0;
};

struct SlotSet {
    int device = -1;
    Slot slot[kSlots];
};

// statistics of this thread's last _host call (sts_staging_stats)
struct Stats {
    double h2d_ms = 0, kernel_ms = 0, d2h_ms = 0, wall_ms = 0;
    double bytes_h2d = 0, bytes_d2h = 0, chunks = 0, direct = 0;   // bytes moved by direct DMA
};
thread_local Stats g_stats;

int hip_status(hipError_t e, const char* where) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", where, hipGetErrorString(e));
    return sts::set_error(STS_ERR_HIP, buf);
}

void destroy_set(SlotSet* g) {
    int cur = -1;
    const bool switch_dev = hipGetDevice(&cur) == hipSuccess && cur != g->device;
    if (switch_dev) (void)hipSetDevice(g->device);
    for (Slot& s : g->slot) {
        if (s.st) (void)hipStreamSynchronize(s.st);
        if (s.dev) (void)hipFree(s.dev);
        if (s.pin) (void)hipHostFree(s.pin);
        for (hipEvent_t& e : s.ev)
            if (e) (void)hipEventDestroy(e);
        if (s.st) (void)hipStreamDestroy(s.st);
    }
    if (switch_dev) (void)hipSetDevice(cur);
    delete g;
}

int create_set(int dev, SlotSet** out) {
    SlotSet* g = new SlotSet;
    g->device = dev;
    hipError_t e = hipSuccess;
    for (Slot& s : g->slot) {
        if ((e = hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking)) != hipSuccess) break;
        for (hipEvent_t& ev : s.ev)
            if ((e = hipEventCreate(&ev)) != hipSuccess) break;
        if (e != hipSuccess) break;
    }
    if (e != hipSuccess) {
        const int r = hip_status(e, "staging: stream / event");
        destroy_set(g);
        return r;
    }
    *out = g;
    return STS_OK;
}

// never destroyed: at process exit the HIP runtime may already be gone, and the OS reclaims
sts::StagePool<SlotSet>& pool() {
    static sts::StagePool<SlotSet>* p = new sts::StagePool<SlotSet>(create_set, destroy_set, kDefaultSets);
    return *p;
}

// A borrowed set; on destruction (every exit path of staged()) all its busy slots are
// drained WITHOUT copying to the caller, then it goes back to the pool -- or, when a drain
// fails (device error), it is forgotten rather than reused or freed under a live DMA.
struct Borrow {
    SlotSet* set = nullptr;
    int dev = -1;
    ~Borrow() {
        if (!set) return;
        bool ok = true;
        for (Slot& sl : set->slot) {
            if (sl.busy && hipEventSynchronize(sl.ev[3]) != hipSuccess) ok = false;
            if (sl.st && hipStreamSynchronize(sl.st) != hipSuccess) ok = false;   // a partly enqueued chunk
            sl.busy = false;
            sl.copy_out = false;
        }
        // a set goes back to the pool at its bound (kSlots x kSlotKeep of HBM and of pinned
        // memory): buffers a one-series-larger-than-a-chunk call grew are freed here (drained above)
        if (ok)
            for (Slot& sl : set->slot) {
                if (sl.dev_cap > kSlotKeep) {
                    (void)hipFree(sl.dev);
                    sl.dev = nullptr;
                    sl.dev_cap = 0;
                }
                if (sl.pin_cap > kSlotKeep) {
                    (void)hipHostFree(sl.pin);
                    sl.pin = nullptr;
                    sl.pin_cap = 0;
                }
            }
        if (ok) pool().give_back(dev, set);
        else pool().forget(dev);
    }
};

bool is_pinned(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // pageable memory: clear the sticky lookup error
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// One per-series array of a _host call.  On the device, chunk rows are contiguous (`row`
// bytes per series); on the host, series s starts at s * hstride.
struct Arg {
    const void* src = nullptr;   // host input (copied in), or nullptr
    void* dst = nullptr;         // host output (copied out), or nullptr
    size_t row = 0;              // device bytes per series
    size_t hstride = 0;          // host bytes between series
    bool panel = false;          // row / hstride are the call's T / ld doubles: staged() sets them once validated
    int shares = -1;             // an output on an input's host memory (an in-place call): that input's index
    bool pinned_src = false, pinned_dst = false;
    size_t dev_off = 0, pin_off = 0;   // per-slot layout (set per chunk size)
    void* host() const { return src ? const_cast<void*>(src) : dst; }
};

Arg in_arg(const void* p, size_t row, size_t hstride) {
    Arg a;
    a.src = p;
    a.row = row;
    a.hstride = hstride;
    return a;
}
Arg out_arg(void* p, size_t row, size_t hstride) {
    Arg a;
    a.dst = p;
    a.row = row;
    a.hstride = hstride;
    return a;
}
// a panel of the call: T doubles per series, ld apart on the host
Arg in_panel(const double* p) {
    Arg a = in_arg(p, 0, 0);
    a.panel = true;
    return a;
}
Arg out_panel(double* p) {
    Arg a = out_arg(p, 0, 0);
    a.panel = true;
    return a;
}
// n doubles per series, packed
Arg in_vec(const double* p, int64_t n = 1) { return in_arg(p, (size_t)n * sizeof(double), (size_t)n * sizeof(double)); }
Arg out_vec(double* p, int64_t n = 1) { return out_arg(p, (size_t)n * sizeof(double), (size_t)n * sizeof(double)); }

// What a wrapper's one device call is handed.  For validation: the caller's host pointers, S and
// ld, and a null stream (the device entry point stops before it dereferences anything).  For a
// chunk: the chunk's device regions (row-contiguous), its series count and its row length T as
// ld, on the slot's stream.  An argument the caller passed as NULL is NULL in both.
struct Call {
    const std::vector<Arg>& args;
    char* dev;
    int64_t n, ld;
    hipStream_t st;
    void* at(size_t k) const {
        void* h = args[k].host();
        return st && h ? dev + args[k].dev_off : h;
    }
    const double* in(size_t k) const { return static_cast<const double*>(at(k)); }
    double* out(size_t k) const { return static_cast<double*>(at(k)); }
    int32_t* err(size_t k) const { return static_cast<int32_t*>(at(k)); }
};
using Kernel = std::function<int(const Call&)>;

void copy_rows(void* dst, size_t dstride, const void* src, size_t sstride, size_t row, int64_t n) {
    if (dstride == row && sstride == row) {
        std::memcpy(dst, src, row * (size_t)n);
        return;
    }
    for (int64_t i = 0; i < n; i++)
        std::memcpy(static_cast<char*>(dst) + (size_t)i * dstride, static_cast<const char*>(src) + (size_t)i * sstride,
                    row);
}

// Wait for a slot's chunk, account its time, copy its pageable outputs to the caller (only
// when its kernel and copy-out were enqueued).
int reap(Slot& sl, std::vector<Arg>& args) {
    if (!sl.busy) return STS_OK;
    hipError_t e = hipEventSynchronize(sl.ev[3]);
    if (e != hipSuccess) return hip_status(e, "staging: chunk");   // stays busy: Borrow drains it
    sl.busy = false;
    Stats& g = g_stats;
    float a = 0, b = 0, c = 0;
    if (hipEventElapsedTime(&a, sl.ev[0], sl.ev[1]) == hipSuccess) g.h2d_ms += a;
    if (hipEventElapsedTime(&b, sl.ev[1], sl.ev[2]) == hipSuccess) g.kernel_ms += b;
    if (hipEventElapsedTime(&c, sl.ev[2], sl.ev[3]) == hipSuccess) g.d2h_ms += c;
    if (!sl.copy_out) return STS_OK;
    sl.copy_out = false;
    for (Arg& x : args)
        if (x.dst && !x.pinned_dst)
            copy_rows(static_cast<char*>(x.dst) + (size_t)sl.s0 * x.hstride, x.hstride,
                      static_cast<char*>(sl.pin) + x.pin_off, x.row, x.row, sl.ns);
    return STS_OK;
}

// Run `kern` -- the wrapper's one device call -- over S series of T steps (ld apart on the host)
// in chunks through a borrowed slot set.
int staged(int64_t S, int64_t T, int64_t ld, std::vector<Arg> args, const Kernel& kern) {
    const auto t_start = std::chrono::steady_clock::now();
    Stats& g = g_stats;
    g = Stats();
    int r;
    if (args.size() > kMaxArgs) return sts::set_error(STS_ERR_BAD_ARG, "staging: too many per-series arguments");
    // the device entry point's own argument checks first, on the caller's shapes, ld and host
    // pointers (never dereferenced in validate-only mode): no staging on bad input, and none
    // where the entry point returns before its first device action (an empty panel, lag 0)
    bool work = false;
    if ((r = sts::validate([&] { return kern(Call{args, nullptr, S, ld, nullptr}); }, &work))) return r;
    // S = 0 on its own: sts_fill and sts_fill_autocorr reach the device with no series to launch
    if (!work || S <= 0) return STS_OK;
    Borrow bw;
    {
        hipError_t e = hipGetDevice(&bw.dev);
        if (e != hipSuccess) return hip_status(e, "hipGetDevice");
        if ((r = pool().acquire(bw.dev, &bw.set))) return r > 0 ? r : sts::set_error(STS_ERR_BAD_ARG, "staging: device id");
    }
    Slot* slots = bw.set->slot;
    size_t per_series = 0;
    for (size_t k = 0; k < args.size(); k++) {
        Arg& x = args[k];
        if (x.panel) x.row = (size_t)T * sizeof(double), x.hstride = (size_t)ld * sizeof(double);
        // in place: an output on an earlier input's host rows lives in that input's device (and
        // bounce) region and is copied out from there
        for (size_t j = 0; j < k && x.dst && x.shares < 0; j++)
            if (args[j].src == x.dst && args[j].row == x.row && args[j].hstride == x.hstride) x.shares = (int)j;
        if (x.shares >= 0) {
            x.pinned_dst = args[x.shares].pinned_src;
            continue;
        }
        x.pinned_src = is_pinned(x.src);
        x.pinned_dst = is_pinned(x.dst);
        per_series += x.row;
    }
    int64_t ns = per_series ? (int64_t)(kChunkBytes / per_series) : S;
    ns = std::max<int64_t>(1, std::min<int64_t>(ns, S));
    // per-slot layout: one device region per arg; one pinned region per pageable in / out
    size_t dev_bytes = 0, pin_bytes = 0;
    for (Arg& x : args) {
        if (x.shares >= 0) {
            x.dev_off = args[x.shares].dev_off;
            x.pin_off = args[x.shares].pin_off;
            continue;
        }
        x.dev_off = dev_bytes;
        dev_bytes += align_up(x.row * (size_t)ns);
        x.pin_off = pin_bytes;
        if ((x.src && !x.pinned_src) || (x.dst && !x.pinned_dst)) pin_bytes += align_up(x.row * (size_t)ns);
    }
    hipError_t e;
    for (int k = 0; k < kSlots; k++) {
        Slot& sl = slots[k];
        if (sl.dev_cap < dev_bytes) {
            if (sl.dev) (void)hipFree(sl.dev);
            sl.dev = nullptr;
            sl.dev_cap = 0;
            if ((e = hipMalloc(&sl.dev, dev_bytes)) != hipSuccess) return hip_status(e, "staging: hipMalloc");
            sl.dev_cap = dev_bytes;
        }
        if (sl.pin_cap < pin_bytes) {
            if (sl.pin) (void)hipHostFree(sl.pin);
            sl.pin = nullptr;
            sl.pin_cap = 0;
            if ((e = hipHostMalloc(&sl.pin, pin_bytes, hipHostMallocDefault)) != hipSuccess)
                return hip_status(e, "staging: hipHostMalloc");
            sl.pin_cap = pin_bytes;
        }
    }
    const int64_t nchunks = (S + ns - 1) / ns;
    int status = STS_OK;
    for (int64_t i = 0; i < nchunks && status == STS_OK; i++) {
        Slot& sl = slots[i % kSlots];
        if ((r = reap(sl, args))) return r;
        sl.s0 = i * ns;
        sl.ns = std::min<int64_t>(ns, S - sl.s0);
        char* dev = static_cast<char*>(sl.dev);
        char* pin = static_cast<char*>(sl.pin);
        // the calling thread stages pageable inputs while earlier chunks are on the device
        for (Arg& x : args)
            if (x.src && !x.pinned_src)
                copy_rows(pin + x.pin_off, x.row, static_cast<const char*>(x.src) + (size_t)sl.s0 * x.hstride,
                          x.hstride, x.row, sl.ns);
        if ((e = hipEventRecord(sl.ev[0], sl.st)) != hipSuccess) return hip_status(e, "staging: event");
        for (Arg& x : args) {
            if (!x.src) continue;
            const size_t n = x.row * (size_t)sl.ns;
            if (x.pinned_src)
                e = hipMemcpy2DAsync(dev + x.dev_off, x.row, static_cast<const char*>(x.src) + (size_t)sl.s0 * x.hstride,
                                     x.hstride, x.row, (size_t)sl.ns, hipMemcpyHostToDevice, sl.st);
            else
                e = hipMemcpyAsync(dev + x.dev_off, pin + x.pin_off, n, hipMemcpyHostToDevice, sl.st);
            if (e != hipSuccess) return hip_status(e, "staging: H2D");
            g.bytes_h2d += (double)n;
            if (x.pinned_src) g.direct += (double)n;
        }
        if ((e = hipEventRecord(sl.ev[1], sl.st)) != hipSuccess) return hip_status(e, "staging: event");
        status = kern(Call{args, dev, sl.ns, T, sl.st});
        if ((e = hipEventRecord(sl.ev[2], sl.st)) != hipSuccess) return hip_status(e, "staging: event");
        if (status == STS_OK) {
            for (Arg& x : args) {
                if (!x.dst) continue;
                const size_t n = x.row * (size_t)sl.ns;
                if (x.pinned_dst)
                    e = hipMemcpy2DAsync(static_cast<char*>(x.dst) + (size_t)sl.s0 * x.hstride, x.hstride,
                                         dev + x.dev_off, x.row, x.row, (size_t)sl.ns, hipMemcpyDeviceToHost, sl.st);
                else
                    e = hipMemcpyAsync(pin + x.pin_off, dev + x.dev_off, n, hipMemcpyDeviceToHost, sl.st);
                if (e != hipSuccess) return hip_status(e, "staging: D2H");
                g.bytes_d2h += (double)n;
                if (x.pinned_dst) g.direct += (double)n;
            }
        }
        if ((e = hipEventRecord(sl.ev[3], sl.st)) != hipSuccess) return hip_status(e, "staging: event");
        sl.busy = true;
        sl.copy_out = (status == STS_OK);
        g.chunks += 1;
    }
    for (int64_t i = 0; i < kSlots; i++) {   // drain in issue order
        Slot& sl = slots[(nchunks + i) % kSlots];
        if ((r = reap(sl, args))) return r;
    }
    g.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return status;
}

// Per-series statuses: the caller's host array, or an internal one whose first failure
// becomes the return status (the reference's exception) once every chunk is back.
struct ErrOut {
    std::vector<int32_t> own;
    int32_t* h;
    explicit ErrOut(int32_t* user, int64_t S) : h(user) {
        if (!h) {
            own.assign((size_t)(S > 0 ? S : 0), 0);
            h = own.data();
        }
    }
    int finish(int st, int64_t S, const char* what) {
        if (st != STS_OK || !own.size()) return st;
        return sts::series_status(h, S, what);
    }
};
Arg status(ErrOut& eo) { return out_arg(eo.h, sizeof(int32_t), sizeof(int32_t)); }

}  // namespace

extern "C" {

int sts_host_alloc(size_t bytes, void** out) {
    if (!out) return sts::set_error(STS_ERR_BAD_ARG, "sts_host_alloc: null output");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault);
    return e == hipSuccess ? STS_OK : hip_status(e, "hipHostMalloc");
}

int sts_host_free(void* p) {
    if (!p) return STS_OK;
    hipError_t e = hipHostFree(p);
    return e == hipSuccess ? STS_OK : hip_status(e, "hipHostFree");
}

int sts_staging_release(void) {
    (void)pool().trim();
    return STS_OK;
}

int sts_staging_set_limit(int max_sets) {
    if (max_sets < 1) return sts::set_error(STS_ERR_BAD_ARG, "sts_staging_set_limit: max_sets must be >= 1");
    (void)pool().set_cap(max_sets);
    return STS_OK;
}

int sts_staging_pool_info(int64_t* out8) {
    if (!out8) return sts::set_error(STS_ERR_BAD_ARG, "sts_staging_pool_info: null output");
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_status(e, "hipGetDevice");
    const auto in = pool().info(dev);
    const int64_t v[8] = {in.live, in.idle, in.borrowed, in.cap, in.high, in.lost, in.waits,
                          (int64_t)kSlots * (int64_t)kSlotKeep};
    std::memcpy(out8, v, sizeof v);
    return STS_OK;
}

int sts_staging_stats(double* out8) {
    if (!out8) return sts::set_error(STS_ERR_BAD_ARG, "sts_staging_stats: null output");
    const Stats& g = g_stats;
    const double tot = g.bytes_h2d + g.bytes_d2h;
    const double v[8] = {g.wall_ms, g.h2d_ms, g.kernel_ms, g.d2h_ms,
                         g.bytes_h2d, g.bytes_d2h, g.chunks, tot > 0 ? g.direct / tot : 0.0};
    std::memcpy(out8, v, sizeof v);
    return STS_OK;
}

// ---- the _host entry points.  Each lists its per-series arrays once and states its device call
// once; staged() runs that call for validation (the caller's pointers, S and ld) and per chunk.
// Every argument error, and every "nothing to do", is therefore the device entry point's own:
// a check written here is one no device entry point can make, and says why it stays. ----

int sts_fill_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int method, int32_t* err) {
    ErrOut eo(err, S);
    const int st = staged(S, T, ld, {in_panel(in), out_panel(out), status(eo)}, [&](const Call& c) {
        return sts_fill(c.in(0), c.out(1), c.n, T, c.ld, c.ld, method, c.err(2), c.st);
    });
    return eo.finish(st, S, "fill");
}

int sts_autocorr_host(const double* in, int64_t S, int64_t T, int64_t ld, int K, double* acf) {
    // a device err array per chunk (it stays all zero: raw autocorr has no failing series), so
    // the device entry point never synchronises inside the pipeline
    ErrOut eo(nullptr, S);
    const int st = staged(S, T, ld, {in_panel(in), out_vec(acf, K), status(eo)}, [&](const Call& c) {
        return sts_fill_autocorr(c.in(0), nullptr, c.n, T, c.ld, c.ld, STS_FILL_NONE, K, c.out(1), c.err(2), c.st);
    });
    return eo.finish(st, S, "autocorr");
}

int sts_fill_autocorr_host(const double* in, double* filled, int64_t S, int64_t T, int64_t ld, int method, int K,
                           double* acf, int32_t* err) {
    // picks the code path: raw autocorr has no filled panel to stage and leaves the caller's err alone
    if (method == STS_FILL_NONE && !filled) return sts_autocorr_host(in, S, T, ld, K, acf);
    ErrOut eo(err, S);
    const int st = staged(S, T, ld, {in_panel(in), out_panel(filled), out_vec(acf, K), status(eo)}, [&](const Call& c) {
        return sts_fill_autocorr(c.in(0), c.out(1), c.n, T, c.ld, c.ld, method, K, c.out(2), c.err(3), c.st);
    });
    return eo.finish(st, S, "fill_autocorr");
}

// in == out is the reference's in-place recurrence (dest eq ts), per series; out of place
// dest(i) = ts(i) for i < start (:363-369), so dest is fully written; lag 0 leaves dest untouched
int sts_diff_at_lag_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int lag, int start) {
    return staged(S, T, ld, {in_panel(in), out_panel(out)}, [&](const Call& c) {
        return sts_diff_at_lag(c.in(0), c.out(1), c.n, T, c.ld, c.ld, lag, start, c.st);
    });
}

int sts_lag_matrix_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int max_lag, int inc) {
    // a check of this wrapper's own, for the size alone: the matrix is sized only for a shape
    // sts_lag_matrix accepts (T in the reference's Int range, 0 <= maxLag <= T), so the product cannot
    // overflow; sts_lag_matrix rejects the rest with its own message
    const bool sized = max_lag >= 0 && max_lag <= T && T <= 0x7fffffffLL;
    const int64_t n = sized ? (T - max_lag) * ((int64_t)max_lag + (inc ? 1 : 0)) : 0;
    return staged(S, T, ld, {in_panel(in), out_vec(out, n)}, [&](const Call& c) {
        return sts_lag_matrix(c.in(0), c.out(1), c.n, T, c.ld, max_lag, inc, c.st);
    });
}

// in == out: add is safe; remove is the reference's read-after-overwrite, per series
static int ewma_host(decltype(&sts_ewma_add) fn, const double* in, double* out, int64_t S, int64_t T, int64_t ld,
                     const double* sm) {
    return staged(S, T, ld, {in_panel(in), out_panel(out), in_vec(sm)}, [&](const Call& c) {
        return fn(c.in(0), c.out(1), c.n, T, c.ld, c.ld, c.in(2), c.st);
    });
}

int sts_ewma_add_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, const double* sm) {
    return ewma_host(sts_ewma_add, in, out, S, T, ld, sm);
}

int sts_ewma_remove_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, const double* sm) {
    return ewma_host(sts_ewma_remove, in, out, S, T, ld, sm);
}

int sts_fill_diff_ewma_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int method, int lag,
                            const double* smoothing, int32_t* err) {
    ErrOut eo(err, S);
    const int st = staged(S, T, ld, {in_panel(in), out_panel(out), in_vec(smoothing), status(eo)}, [&](const Call& c) {
        return sts_fill_diff_ewma(c.in(0), c.out(1), c.n, T, c.ld, c.ld, method, lag, c.in(2), c.err(3), c.st);
    });
    return eo.finish(st, S, "fill_diff_ewma");
}

int sts_ewma_fit_host(const double* in, int64_t S, int64_t T, int64_t ld, double* smoothing, int32_t* err) {
    ErrOut eo(err, S);
    const int st = staged(S, T, ld, {in_panel(in), out_vec(smoothing), status(eo)}, [&](const Call& c) {
        return sts_ewma_fit(c.in(0), c.n, T, c.ld, c.out(1), c.err(2), c.st);
    });
    return eo.finish(st, S, "EWMA.fitModel");
}

int sts_ar_fit_host(const double* in, int64_t S, int64_t T, int64_t ld, int p, int no_intercept, double* c,
                    double* coef, int32_t* err) {
    ErrOut eo(err, S);
    const int st = staged(S, T, ld, {in_panel(in), out_vec(c), out_vec(coef, p), status(eo)}, [&](const Call& k) {
        return sts_ar_fit(k.in(0), k.n, T, k.ld, p, no_intercept, k.out(1), k.out(2), k.err(3), k.st);
    });
    return eo.finish(st, S, "ar_fit");
}

int sts_ar_fit_remove_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int p, int no_intercept,
                           double* c, double* coef, int32_t* err) {
    ErrOut eo(err, S);
    const int st = staged(S, T, ld, {in_panel(in), out_panel(out), out_vec(c), out_vec(coef, p), status(eo)},
                          [&](const Call& k) {
                              return sts_ar_fit_remove(k.in(0), k.out(1), k.n, T, k.ld, k.ld, p, no_intercept, k.out(2),
                                                       k.out(3), k.err(4), k.st);
                          });
    return eo.finish(st, S, "ar_fit_remove");
}

int sts_garch_fit_host(const double* in, int64_t S, int64_t T, int64_t ld, double* params, int32_t* err) {
    ErrOut eo(err, S);
    const int st = staged(S, T, ld, {in_panel(in), out_vec(params, 3), status(eo)}, [&](const Call& c) {
        return sts_garch_fit(c.in(0), c.n, T, c.ld, c.out(1), c.err(2), c.st);
    });
    return eo.finish(st, S, "GARCH.fitModel");
}

int sts_argarch_fit_host(const double* in, int64_t S, int64_t T, int64_t ld, double* c, double* phi, double* params,
                         int32_t* err) {
    ErrOut eo(err, S);
    const int st = staged(S, T, ld, {in_panel(in), out_vec(c), out_vec(phi), out_vec(params, 3), status(eo)},
                          [&](const Call& k) {
                              return sts_argarch_fit(k.in(0), k.n, T, k.ld, k.out(1), k.out(2), k.out(3), k.err(4),
                                                     k.st);
                          });
    return eo.finish(st, S, "ARGARCH.fitModel");
}

static int ar_host(decltype(&sts_ar_add) fn, const double* in, double* out, int64_t S, int64_t T, int64_t ld,
                   const double* c, const double* coef, int p) {
    // not an argument check: p = 0 has no coefficients (coef may be NULL) and no kernel loads one; one
    // zero stands in for every series' row (host stride 0) so that the call keeps its four per-series
    // arguments and the device call a non-NULL pointer, whatever the caller passed
    const double zero = 0.0;
    const Arg k = p > 0 ? in_vec(coef, p) : in_arg(&zero, sizeof(double), 0);
    return staged(S, T, ld, {in_panel(in), out_panel(out), in_vec(c), k}, [&](const Call& a) {
        return fn(a.in(0), a.out(1), a.n, T, a.ld, a.ld, a.in(2), a.in(3), p, a.st);
    });
}

int sts_ar_remove_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, const double* c,
                       const double* coef, int p) {
    return ar_host(sts_ar_remove, in, out, S, T, ld, c, coef, p);
}

int sts_ar_add_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, const double* c,
                    const double* coef, int p) {
    return ar_host(sts_ar_add, in, out, S, T, ld, c, coef, p);
}

// ---- statistical tests ----

int sts_dw_test_host(const double* in, int64_t S, int64_t T, int64_t ld, double* stat) {
    return staged(S, T, ld, {in_panel(in), out_vec(stat)}, [&](const Call& c) {
        return sts_dw_test(c.in(0), c.n, T, c.ld, c.out(1), c.st);
    });
}

int sts_kpss_test_host(const double* in, int64_t S, int64_t T, int64_t ld, int regression, double* stat) {
    return staged(S, T, ld, {in_panel(in), out_vec(stat)}, [&](const Call& c) {
        return sts_kpss_test(c.in(0), c.n, T, c.ld, regression, c.out(1), c.st);
    });
}

int sts_adf_test_host(const double* in, int64_t S, int64_t T, int64_t ld, int max_lag, int regression, double* stat,
                      double* pvalue, int32_t* err) {
    ErrOut eo(err, S);
    const int st = staged(S, T, ld, {in_panel(in), out_vec(stat), out_vec(pvalue), status(eo)}, [&](const Call& c) {
        return sts_adf_test(c.in(0), c.n, T, c.ld, max_lag, regression, c.out(1), c.out(2), c.err(3), c.st);
    });
    return eo.finish(st, S, "adftest");
}

int sts_lb_test_host(const double* in, int64_t S, int64_t T, int64_t ld, int max_lag, double* stat, double* pvalue) {
    return staged(S, T, ld, {in_panel(in), out_vec(stat), out_vec(pvalue)}, [&](const Call& c) {
        return sts_lb_test(c.in(0), c.n, T, c.ld, max_lag, c.out(1), c.out(2), c.st);
    });
}

// Calls with a factor panel (bgtest / bptest, include/sts_regress.h): a shared factor matrix
// (fs == 0) is copied to the device once, row by row (only the T elements of each factor row are
// read), and every chunk runs against it; per-series factors ride the staging pipeline as one block
// of (k - 1) * ld_f + T doubles per series (the padding between a series' own factor rows is moved
// with it and never used).  `call` is the wrapper's one device call, given the Call and the factor
// panel to pass: (factors, ld_f, fs).
using FactorCall = std::function<int(const Call&, const double*, int64_t, int64_t)>;
static int staged_with_factors(int64_t S, int64_t T, int64_t ld, const double* factors, int k, int64_t ld_f,
                               int64_t fs, std::vector<Arg> args, const FactorCall& call) {
    // a validation of this wrapper's own, ahead of staged()'s: the sizes below (k rows, the factor
    // span) must not overflow, and shared factors are uploaded before the pipeline runs -- nothing is
    // copied on bad input
    bool work = false;
    const int r = sts::validate([&] { return call(Call{args, nullptr, S, ld, nullptr}, factors, ld_f, fs); }, &work);
    if (r || !work) return r;
    const size_t row = (size_t)T * sizeof(double);
    const int64_t span = (int64_t)(k - 1) * ld_f + T;
    void* df = nullptr;
    if (fs == 0) {   // picks the code path: shared factors, once, outside the pipeline
        hipError_t e = hipMalloc(&df, (size_t)k * row);
        if (e != hipSuccess) return hip_status(e, "hipMalloc(factors)");
        e = hipMemcpy2D(df, row, factors, (size_t)ld_f * sizeof(double), row, (size_t)k, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(df);
            return hip_status(e, "hipMemcpy2D(factors)");
        }
    }
    // what the device call is given as factors: the uploaded copy (packed rows), or the chunk's own
    // blocks (during validation the caller's, at a stride the check above accepted)
    const size_t own = args.size();
    args.push_back(fs == 0 ? Arg() : in_arg(factors, (size_t)span * sizeof(double), (size_t)fs * sizeof(double)));
    const int st = staged(S, T, ld, args, [&](const Call& c) {
        const double* f = fs == 0 ? static_cast<const double*>(df) : c.in(own);
        return call(c, f, fs == 0 ? T : ld_f, fs == 0 ? 0 : span);
    });
    if (df) (void)hipFree(df);   // every chunk is back
    return st;
}

static int bgbp_host(bool bp, const double* resid, int64_t S, int64_t T, int64_t ld, const double* factors, int k,
                     int64_t ld_f, int64_t fs, int max_lag, double* stat, double* pvalue, int32_t* err) {
    ErrOut eo(err, S);
    const int st = staged_with_factors(
        S, T, ld, factors, k, ld_f, fs, {in_panel(resid), out_vec(stat), out_vec(pvalue), status(eo)},
        [&](const Call& c, const double* f, int64_t ldf, int64_t fsf) {
            return bp ? sts_bp_test(c.in(0), c.n, T, c.ld, f, k, ldf, fsf, c.out(1), c.out(2), c.err(3), c.st)
                      : sts_bg_test(c.in(0), c.n, T, c.ld, f, k, ldf, fsf, max_lag, c.out(1), c.out(2), c.err(3), c.st);
        });
    return eo.finish(st, S, bp ? "bptest" : "bgtest");
}

int sts_bp_test_host(const double* resid, int64_t S, int64_t T, int64_t ld, const double* factors, int k, int64_t ld_f,
                     int64_t fs, double* stat, double* pvalue, int32_t* err) {
    return bgbp_host(true, resid, S, T, ld, factors, k, ld_f, fs, 0, stat, pvalue, err);
}

int sts_bg_test_host(const double* resid, int64_t S, int64_t T, int64_t ld, const double* factors, int k, int64_t ld_f,
                     int64_t fs, int max_lag, double* stat, double* pvalue, int32_t* err) {
    return bgbp_host(false, resid, S, T, ld, factors, k, ld_f, fs, max_lag, stat, pvalue, err);
}

// ---- include/sts_regress.h: beta and stderr packed (k + 1 wide, 0 for a k the entry point rejects),
// the residual panel at the input's ld ----

int sts_factor_ols_host(const double* y, int64_t S, int64_t T, int64_t ld, const double* factors, int k, int64_t ld_f,
                        int64_t fs, double* beta, double* stderr_out, double* stats, double* resid, int32_t* err) {
    const int64_t w = (k >= 1 && k <= STS_MAX_FACTORS) ? k + 1 : 0;
    ErrOut eo(err, S);
    const int st = staged_with_factors(
        S, T, ld, factors, k, ld_f, fs,
        {in_panel(y), out_vec(beta, w), out_vec(stderr_out, w), out_vec(stats, 4), out_panel(resid), status(eo)},
        [&](const Call& c, const double* f, int64_t ldf, int64_t fsf) {
            return sts_factor_ols(c.in(0), c.n, T, c.ld, f, k, ldf, fsf, c.out(1), k + 1, c.out(2), c.out(3), c.out(4),
                                  c.ld, c.err(5), c.st);
        });
    return eo.finish(st, S, "factor_ols");
}

static int factor_effects_host(decltype(&sts_factor_add) fn, const double* in, double* out, int64_t S, int64_t T,
                               int64_t ld, const double* factors, int k, int64_t ld_f, int64_t fs, const double* beta) {
    const int64_t w = (k >= 1 && k <= STS_MAX_FACTORS) ? k + 1 : 0;
    return staged_with_factors(S, T, ld, factors, k, ld_f, fs, {in_panel(in), out_panel(out), in_vec(beta, w)},
                               [&](const Call& c, const double* f, int64_t ldf, int64_t fsf) {
                                   return fn(c.in(0), c.out(1), c.n, T, c.ld, c.ld, f, k, ldf, fsf, c.in(2), k + 1, c.st);
                               });
}

int sts_factor_remove_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, const double* factors, int k,
                           int64_t ld_f, int64_t fs, const double* beta) {
    return factor_effects_host(sts_factor_remove, in, out, S, T, ld, factors, k, ld_f, fs, beta);
}

int sts_factor_add_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, const double* factors, int k,
                        int64_t ld_f, int64_t fs, const double* beta) {
    return factor_effects_host(sts_factor_add, in, out, S, T, ld, factors, k, ld_f, fs, beta);
}

// ---- include/sts_cross.h.  Every output depends on two series that may lie anywhere in the two
// panels, so there are no chunks of series to pipeline: both panels are copied to the device whole
// (packed rows, only the T elements of a row are read), the one device call runs on the calling
// thread's stream, and the packed matrix and the means come back.  `call` is the wrapper's one device
// call: first in validate-only mode on the caller's pointers and ld, then on the device copies. ----

int sts_cross_moments_host(const double* x, int64_t Sx, int64_t T, int64_t ld_x, const double* y, int64_t Sy, int64_t ld_y,
                           int kind, double* out, double* mean_x, double* mean_y) {
    const int64_t cols = y ? Sy : Sx;
    const auto call = [&](const double* px, int64_t ldx, const double* py, int64_t ldy, double* po, double* mx, double* my) {
        return sts_cross_moments(px, Sx, T, ldx, py, Sy, ldy, kind, po, cols, mx, my, nullptr);
    };
    bool work = false;
    const int r = sts::validate([&] { return call(x, ld_x, y, ld_y, out, mean_x, mean_y); }, &work);
    if (r || !work) return r;
    const size_t row = (size_t)T * sizeof(double);
    const size_t nx = (size_t)Sx * (size_t)T, ny = y ? (size_t)Sy * (size_t)T : 0, no = (size_t)Sx * (size_t)cols;
    struct Dev {
        void* p = nullptr;
        ~Dev() {
            if (p) (void)hipFree(p);
        }
    } dev;
    hipError_t e = hipMalloc(&dev.p, (nx + ny + no + (size_t)Sx + (size_t)cols) * sizeof(double));
    if (e != hipSuccess) return hip_status(e, "hipMalloc(cross_moments)");
    double* dx = static_cast<double*>(dev.p);
    double* dy = y ? dx + nx : nullptr;
    double* dout = dx + nx + ny;
    double* dmx = mean_x ? dout + no : nullptr;
    double* dmy = mean_y ? dout + no + Sx : nullptr;
    e = hipMemcpy2D(dx, row, x, (size_t)ld_x * sizeof(double), row, (size_t)Sx, hipMemcpyHostToDevice);
    if (e == hipSuccess && y) e = hipMemcpy2D(dy, row, y, (size_t)ld_y * sizeof(double), row, (size_t)Sy, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_status(e, "hipMemcpy2D(cross_moments)");
    const int st = call(dx, T, dy, T, dout, dmx, dmy);
    e = hipStreamSynchronize(hipStreamPerThread);   // also on a failed call: nothing of it may outlive the buffer
    if (st != STS_OK) return st;
    if (e == hipSuccess) e = hipMemcpy(out, dout, no * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && mean_x) e = hipMemcpy(mean_x, dmx, (size_t)Sx * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && mean_y) e = hipMemcpy(mean_y, dmy, (size_t)cols * sizeof(double), hipMemcpyDeviceToHost);
    return e == hipSuccess ? STS_OK : hip_status(e, "cross_moments (host)");
}

// ---- include/sts_roll.h.  An output depends on its own row alone, so the panels ride the staging
// pipeline by chunks of series.  A per-series y is a third per-series array (T doubles per series,
// ld_y apart on the host); a shared factor is uploaded once, outside the pipeline, as bgbp_host's
// shared factors are. ----

int sts_roll_stat_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int window, int min_periods,
                       int op) {
    return staged(S, T, ld, {in_panel(in), out_panel(out)}, [&](const Call& c) {
        return sts_roll_stat(c.in(0), c.out(1), c.n, T, c.ld, c.ld, window, min_periods, op, c.st);
    });
}

int sts_roll_pair_host(const double* x, const double* y, int64_t Sy, int64_t ld_y, double* out, int64_t S, int64_t T,
                       int64_t ld, int window, int min_periods, int op) {
    const bool shared = Sy == 1;
    // the device call on the caller's pointers: the chunk's Sy is its own series count, or 1
    const auto call = [&](const double* px, const double* py, int64_t ldy, double* po, int64_t n, int64_t ldx, hipStream_t st,
                          bool whole) {
        return sts_roll_pair(px, py, whole ? Sy : (shared ? 1 : n), ldy, po, n, T, ldx, ldx, window, min_periods, op, st);
    };
    bool work = false;
    const int r = sts::validate([&] { return call(x, y, ld_y, out, S, ld, nullptr, true); }, &work);
    if (r || !work) return r;
    const size_t row = (size_t)T * sizeof(double);
    if (!shared) {
        return staged(S, T, ld, {in_panel(x), out_panel(out), in_arg(y, row, (size_t)ld_y * sizeof(double))},
                      [&](const Call& c) {
                          const bool val = c.st == nullptr;   // staged()'s own validation: the caller's pointers
                          return call(c.in(0), c.in(2), val ? ld_y : T, c.out(1), c.n, c.ld, c.st, val);
                      });
    }
    void* df = nullptr;
    hipError_t e = hipMalloc(&df, row);
    if (e != hipSuccess) return hip_status(e, "hipMalloc(roll factor)");
    e = hipMemcpy(df, y, row, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(df);
        return hip_status(e, "hipMemcpy(roll factor)");
    }
    const int st = staged(S, T, ld, {in_panel(x), out_panel(out)}, [&](const Call& c) {
        const bool val = c.st == nullptr;
        return call(c.in(0), val ? y : static_cast<const double*>(df), T, c.out(1), c.n, c.ld, c.st, val);
    });
    (void)hipFree(df);   // every chunk is back
    return st;
}

// ---- panel transforms (include/sts_transforms.h).  An output of another width than the input is
// packed (out_vec): the width is computed here, for the staging size alone and only for a shape the
// device entry point accepts (so it cannot overflow); every other shape gets width 0 and the entry
// point's own message. ----

int sts_quotients_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int lag, int minus_one) {
    const int64_t n = (lag >= 0 && lag <= T) ? T - lag : 0;
    return staged(S, T, ld, {in_panel(in), out_vec(out, n)}, [&](const Call& c) {
        return sts_quotients(c.in(0), c.out(1), c.n, T, c.ld, n, lag, minus_one, c.st);
    });
}

int sts_fill_quotients_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int method, int lag,
                            int minus_one, int32_t* err) {
    const int64_t n = (lag >= 0 && lag <= T) ? T - lag : 0;
    ErrOut eo(err, S);
    const int st = staged(S, T, ld, {in_panel(in), out_vec(out, n), status(eo)}, [&](const Call& c) {
        return sts_fill_quotients(c.in(0), c.out(1), c.n, T, c.ld, n, method, lag, minus_one, c.err(2), c.st);
    });
    return eo.finish(st, S, "fill_quotients");
}

// in == out: element-wise, safe
int sts_fill_with_default_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, double filler) {
    return staged(S, T, ld, {in_panel(in), out_panel(out)}, [&](const Call& c) {
        return sts_fill_with_default(c.in(0), c.out(1), c.n, T, c.ld, c.ld, filler, c.st);
    });
}

int sts_downsample_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int n, int phase) {
    const bool sized = n >= 1 && phase >= 0 && phase < T && T <= 0x7fffffffLL;
    const int64_t w = sized ? (T - phase + n - 1) / n : 0;
    return staged(S, T, ld, {in_panel(in), out_vec(out, w)}, [&](const Call& c) {
        return sts_downsample(c.in(0), c.out(1), c.n, T, c.ld, w, n, phase, c.st);
    });
}

int sts_upsample_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int n, int phase, int use_zero) {
    const bool sized = n >= 1 && T >= 0 && T <= 0x7fffffffLL && T * n <= 0x7fffffffLL;
    const int64_t w = sized ? T * n : 0;
    return staged(S, T, ld, {in_panel(in), out_vec(out, w)}, [&](const Call& c) {
        return sts_upsample(c.in(0), c.out(1), c.n, T, c.ld, sized ? w : T * (int64_t)n, n, phase, use_zero, c.st);
    });
}

int sts_first_last_not_nan_host(const double* in, int64_t S, int64_t T, int64_t ld, int64_t* first, int64_t* last) {
    return staged(S, T, ld, {in_panel(in), out_arg(first, sizeof(int64_t), sizeof(int64_t)),
                             out_arg(last, sizeof(int64_t), sizeof(int64_t))}, [&](const Call& c) {
        return sts_first_last_not_nan(c.in(0), c.n, T, c.ld, static_cast<int64_t*>(c.at(1)),
                                      static_cast<int64_t*>(c.at(2)), c.st);
    });
}

// in == out gives the same bits as out of place (history of outputs); lag 0 leaves dest untouched
int sts_inverse_diff_at_lag_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int lag, int start) {
    return staged(S, T, ld, {in_panel(in), out_panel(out)}, [&](const Call& c) {
        return sts_inverse_diff_at_lag(c.in(0), c.out(1), c.n, T, c.ld, c.ld, lag, start, c.st);
    });
}

int sts_diff_order_d_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int d) {
    return staged(S, T, ld, {in_panel(in), out_panel(out)}, [&](const Call& c) {
        return sts_diff_order_d(c.in(0), c.out(1), c.n, T, c.ld, c.ld, d, c.st);
    });
}

int sts_inverse_diff_order_d_host(const double* in, double* out, int64_t S, int64_t T, int64_t ld, int d) {
    return staged(S, T, ld, {in_panel(in), out_panel(out)}, [&](const Call& c) {
        return sts_inverse_diff_order_d(c.in(0), c.out(1), c.n, T, c.ld, c.ld, d, c.st);
    });
}

// ---- rebasing (include/sts_index.h i3, i4): the output is packed, T_out wide (0 for a shape the
// entry point rejects, as above) ----

int sts_rebase_shift_host(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld,
                          int64_t start_loc, double default_value) {
    const int64_t w = (T_out >= 0 && T_out <= 0x7fffffffLL) ? T_out : 0;
    return staged(S, T_in, ld, {in_panel(in), out_vec(out, w)}, [&](const Call& c) {
        return sts_rebase_shift(c.in(0), c.out(1), c.n, T_in, T_out, c.ld, T_out, start_loc, default_value, c.st);
    });
}

// the map is shared by every series: it is uploaded once, outside the pipeline (as bgbp_host's shared
// factors are), after the entry point has accepted the call on the caller's pointers
int sts_rebase_map_host(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld,
                        const int64_t* map, double default_value) {
    bool work = false;
    const int r = sts::validate(
        [&] { return sts_rebase_map(in, out, S, T_in, T_out, ld, T_out, map, default_value, nullptr); }, &work);
    if (r || !work) return r;
    void* dm = nullptr;
    hipError_t e = hipMalloc(&dm, (size_t)T_out * sizeof(int64_t));
    if (e != hipSuccess) return hip_status(e, "hipMalloc(map)");
    e = hipMemcpy(dm, map, (size_t)T_out * sizeof(int64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(dm);
        return hip_status(e, "hipMemcpy(map)");
    }
    const int st = staged(S, T_in, ld, {in_panel(in), out_vec(out, T_out)}, [&](const Call& c) {
        return sts_rebase_map(c.in(0), c.out(1), c.n, T_in, T_out, c.ld, T_out, c.st ? static_cast<const int64_t*>(dm) : map,
                              default_value, c.st);
    });
    (void)hipFree(dm);   // every chunk is back
    return st;
}

}  // extern "C"
