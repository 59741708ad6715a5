// Sanitizer driver for the C-ABI argument paths (TEST INFRASTRUCTURE ONLY;
// tests/test_sanitizers.py).  csrc/sts_api.cpp and csrc/sts_host.cpp are compiled for the
// host with -fsanitize=address,undefined (the device objects are linked as built) and every
// `_host` / device entry point is called with the invalid arguments the C ABI must reject
// (null panels, ld < T, bad method / order / lag, numLags < 0, aliasing) -- each must return
// its documented status without touching memory it does not own -- and then with valid
// arguments, which on a machine without a gfx950 device must fail cleanly with
// STS_ERR_NO_DEVICE or STS_ERR_HIP.  A host-against-device table (host_device_table) holds every
// `_host` entry point to its device entry point's status and message, fault kind by fault kind.
// Prints "ok" and exits 0 when every status matched.
//
// `host_args_san N` runs the whole sequence in N threads at once (the ThreadSanitizer build
// of tests/test_sanitizers.py: Spark's N executor threads calling the ABI concurrently,
// S/TimeSeriesRDD.scala:417-421), and checks that sts_last_error() stays per thread: each
// thread's own failing call leaves its own message, whatever the other threads do meanwhile.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "sts.h"

static std::atomic<int> failures{0};

static void expect(int got, int want, const char* what) {
    if (got != want) {
        std::printf("FAIL %s: status %d, expected %d (%s)\n", what, got, want, sts_last_error());
        failures++;
    }
}

static void expect_no_device(int got, const char* what) {
    if (got != STS_ERR_NO_DEVICE && got != STS_ERR_HIP) {
        std::printf("FAIL %s: status %d, expected no-device (%s)\n", what, got, sts_last_error());
        failures++;
    }
}

// ---- host against device: one argument contract ----
// A `_host` entry point validates through its device entry point (csrc/sts_host.cpp staged()), so on
// a faulty call both forms must return the same status and leave the same sts_last_error() text.
// Every FAULT row is a call the device entry point rejects before its first device action: the
// `_host` form goes first, and the device form is called with the same (host) pointers only once
// the `_host` form has answered with an argument status.  A NOWORK row is a valid call with nothing
// to do: STS_OK from both forms, no device visible.
static std::atomic<int> table_rows{0};

static bool argument_status(int st) { return st != STS_OK && st != STS_ERR_HIP && st != STS_ERR_NO_DEVICE; }

template <class H, class D>
static void same(bool fault, const char* what, H host, D dev) {
    table_rows++;
    const int a = host();
    const std::string ma = a ? sts_last_error() : "";
    if (fault ? !argument_status(a) : a != STS_OK) {
        std::printf("FAIL table %s: host status %d (%s), expected %s\n", what, a, ma.c_str(),
                    fault ? "an argument error" : "STS_OK");
        failures++;
        return;
    }
    const int b = dev();
    const std::string mb = b ? sts_last_error() : "";
    if (a != b || ma != mb) {
        std::printf("DIFF table %s: host %d \"%s\" / device %d \"%s\"\n", what, a, ma.c_str(), b, mb.c_str());
        failures++;
    }
}
// (the per-operator macros below expand to the pair "host call, device call" with the same arguments:
// ld_in = ld_out = ld, err_per_series NULL, stream NULL)
#define PAIR_(fault, what, host_call, dev_call) same(fault, what, [&] { return host_call; }, [&] { return dev_call; })
#define FAULT(what, ...) PAIR_(true, what, __VA_ARGS__)
#define NOWORK(what, ...) PAIR_(false, what, __VA_ARGS__)

static void host_device_table() {
    const int64_t S = 3, T = 50;
    std::vector<double> inv(S * T, 1.0), outv(S * T), acfv(S * 70), cv(S), cfv(S * 8), smv(S, 0.2), parv(S * 3), stv(S),
        pvv(S), fv(4 * S * T, 0.5);
    double *in = inv.data(), *out = outv.data(), *acf = acfv.data(), *c = cv.data(), *cf = cfv.data(), *sm = smv.data(),
           *par = parv.data(), *st = stv.data(), *pv = pvv.data(), *f = fv.data();
    double* const N = nullptr;
    const int L = STS_FILL_LINEAR;

    // fill(in, out, S, T, ld, method, err)
#define FILL(in_, out_, S_, T_, ld_, m_) \
    sts_fill_host(in_, out_, S_, T_, ld_, m_, nullptr), sts_fill(in_, out_, S_, T_, ld_, ld_, m_, nullptr, nullptr)
    FAULT("fill null in", FILL(N, out, S, T, T, L));
    FAULT("fill null out", FILL(in, N, S, T, T, L));
    FAULT("fill ld < T", FILL(in, out, S, T, T - 1, L));
    FAULT("fill S < 0", FILL(in, out, -1, T, T, L));
    FAULT("fill T < 0", FILL(in, out, S, -1, T, L));
    FAULT("fill alias", FILL(in, in, S, T, T, L));
    FAULT("fill method 99", FILL(in, out, S, T, T, 99));
    FAULT("fill method none", FILL(in, out, S, T, T, STS_FILL_NONE));
    // two faults at once: the device entry point's order of checks decides
    FAULT("fill null in + method 99", FILL(N, out, S, T, T, 99));
    FAULT("fill null in + ld < T", FILL(N, out, S, T, T - 1, L));
    // the `_host` form only: sts_fill itself has no early return for S = 0 (it reaches the device and
    // launches nothing), so without a device it cannot answer STS_OK
    NOWORK("fill S = 0 (host form)", sts_fill_host(in, out, 0, T, T, L, nullptr), (int)STS_OK);

    // autocorr(in, S, T, ld, K, acf)
#define ACF(in_, S_, T_, ld_, K_, acf_) \
    sts_autocorr_host(in_, S_, T_, ld_, K_, acf_), sts_autocorr(in_, S_, T_, ld_, K_, acf_, nullptr)
    FAULT("autocorr null in", ACF(N, S, T, T, 5, acf));
    FAULT("autocorr ld < T", ACF(in, S, T, T - 1, 5, acf));
    FAULT("autocorr S < 0", ACF(in, -2, T, T, 5, acf));
    FAULT("autocorr K < 0", ACF(in, S, T, T, -1, acf));
    FAULT("autocorr null acf", ACF(in, S, T, T, 5, N));

    // fill_autocorr(in, filled, S, T, ld, method, K, acf, err)
#define FACF(in_, fl_, S_, T_, ld_, m_, K_, acf_)                          \
    sts_fill_autocorr_host(in_, fl_, S_, T_, ld_, m_, K_, acf_, nullptr), \
        sts_fill_autocorr(in_, fl_, S_, T_, ld_, ld_, m_, K_, acf_, nullptr, nullptr)
    FAULT("fill_autocorr method 42", FACF(in, out, S, T, T, 42, 5, acf));
    FAULT("fill_autocorr null in", FACF(N, out, S, T, T, L, 5, acf));
    FAULT("fill_autocorr null filled", FACF(in, N, S, T, T, L, 5, acf));
    FAULT("fill_autocorr alias", FACF(in, in, S, T, T, L, 5, acf));
    FAULT("fill_autocorr ld < T", FACF(in, out, S, T, T - 1, L, 5, acf));
    FAULT("fill_autocorr T < 0", FACF(in, out, S, -3, T, L, 5, acf));
    FAULT("fill_autocorr K < 0", FACF(in, out, S, T, T, L, -1, acf));
    FAULT("fill_autocorr null acf", FACF(in, out, S, T, T, L, 5, N));
    FAULT("fill_autocorr none with filled", FACF(in, out, S, T, T, STS_FILL_NONE, 5, acf));
    FAULT("fill_autocorr none K < 0", FACF(in, N, S, T, T, STS_FILL_NONE, -1, acf));
    FAULT("fill_autocorr none with filled + null in", FACF(N, out, S, T, T, STS_FILL_NONE, 5, acf));

    // diff_at_lag(in, out, S, T, ld, lag, start)
#define DIFF(in_, out_, S_, T_, ld_, lag_, start_) \
    sts_diff_at_lag_host(in_, out_, S_, T_, ld_, lag_, start_), sts_diff_at_lag(in_, out_, S_, T_, ld_, ld_, lag_, start_, nullptr)
    FAULT("diff start < lag", DIFF(in, out, S, T, T, 3, 2));
    FAULT("diff lag < 0", DIFF(in, out, S, T, T, -1, 0));
    FAULT("diff null in", DIFF(N, out, S, T, T, 1, 1));
    FAULT("diff null out", DIFF(in, N, S, T, T, 1, 1));
    FAULT("diff ld < T", DIFF(in, out, S, T, T - 1, 1, 1));
    FAULT("diff S < 0", DIFF(in, out, -1, T, T, 1, 1));
    FAULT("diff null in + start < lag", DIFF(N, out, S, T, T, 3, 2));
    NOWORK("diff lag = 0", DIFF(in, out, S, T, T, 0, 0));
    NOWORK("diff lag = 0 in place", DIFF(in, in, S, T, T, 0, 7));
    NOWORK("diff T = 0", DIFF(in, out, S, 0, T, 1, 1));

    // lag_matrix(in, out, S, T, ld, maxLag, includeOriginal)
#define LAG(in_, out_, S_, T_, ld_, p_, inc_) \
    sts_lag_matrix_host(in_, out_, S_, T_, ld_, p_, inc_), sts_lag_matrix(in_, out_, S_, T_, ld_, p_, inc_, nullptr)
    FAULT("lag null in", LAG(N, out, S, T, T, 2, 1));
    FAULT("lag ld < T", LAG(in, out, S, T, T - 1, 2, 1));
    FAULT("lag T < 0", LAG(in, out, S, -1, T, 2, 1));
    FAULT("lag maxLag < 0", LAG(in, out, S, T, T, -1, 1));
    FAULT("lag maxLag > T", LAG(in, out, S, T, T, (int)T + 1, 1));
    FAULT("lag null out", LAG(in, N, S, T, T, 2, 1));
    NOWORK("lag maxLag = T", LAG(in, N, S, T, T, (int)T, 1));
    NOWORK("lag no columns", LAG(in, N, S, T, T, 0, 0));
    NOWORK("lag S = 0", LAG(in, out, 0, T, T, 2, 1));

    // ewma_add / ewma_remove(in, out, S, T, ld, smoothing)
#define EWMA(fn, in_, out_, S_, T_, ld_, sm_) \
    fn##_host(in_, out_, S_, T_, ld_, sm_), fn(in_, out_, S_, T_, ld_, ld_, sm_, nullptr)
    FAULT("ewma_add null dest", EWMA(sts_ewma_add, in, N, S, T, T, sm));
    FAULT("ewma_add null in", EWMA(sts_ewma_add, N, out, S, T, T, sm));
    FAULT("ewma_add ld < T", EWMA(sts_ewma_add, in, out, S, T, T - 1, sm));
    FAULT("ewma_add S < 0", EWMA(sts_ewma_add, in, out, -1, T, T, sm));
    FAULT("ewma_add null smoothing", EWMA(sts_ewma_add, in, out, S, T, T, N));
    FAULT("ewma_add in place null smoothing", EWMA(sts_ewma_add, in, in, S, T, T, N));
    NOWORK("ewma_add T = 0", EWMA(sts_ewma_add, in, out, S, 0, T, sm));
    FAULT("ewma_remove null dest", EWMA(sts_ewma_remove, in, N, S, T, T, sm));
    FAULT("ewma_remove null in", EWMA(sts_ewma_remove, N, out, S, T, T, sm));
    FAULT("ewma_remove ld < T", EWMA(sts_ewma_remove, in, out, S, T, T - 1, sm));
    FAULT("ewma_remove T < 0", EWMA(sts_ewma_remove, in, out, S, -1, T, sm));
    FAULT("ewma_remove null smoothing", EWMA(sts_ewma_remove, in, out, S, T, T, N));
    NOWORK("ewma_remove S = 0", EWMA(sts_ewma_remove, in, out, 0, T, T, N));

    // fill_diff_ewma(in, out, S, T, ld, method, lag, smoothing, err)
#define FDE(in_, out_, S_, T_, ld_, m_, lag_, sm_)                          \
    sts_fill_diff_ewma_host(in_, out_, S_, T_, ld_, m_, lag_, sm_, nullptr), \
        sts_fill_diff_ewma(in_, out_, S_, T_, ld_, ld_, m_, lag_, sm_, nullptr, nullptr)
    FAULT("fill_diff_ewma method 7", FDE(in, out, S, T, T, 7, 1, sm));
    FAULT("fill_diff_ewma method -2", FDE(in, out, S, T, T, -2, 1, sm));
    FAULT("fill_diff_ewma null in", FDE(N, out, S, T, T, L, 1, sm));
    FAULT("fill_diff_ewma null out", FDE(in, N, S, T, T, L, 1, sm));
    FAULT("fill_diff_ewma ld < T", FDE(in, out, S, T, T - 1, L, 1, sm));
    FAULT("fill_diff_ewma S < 0", FDE(in, out, -1, T, T, L, 1, sm));
    FAULT("fill_diff_ewma lag < 0", FDE(in, out, S, T, T, L, -1, sm));
    FAULT("fill_diff_ewma null smoothing", FDE(in, out, S, T, T, L, 1, N));
    FAULT("fill_diff_ewma alias", FDE(in, in, S, T, T, L, 1, sm));
    NOWORK("fill_diff_ewma T = 0", FDE(in, out, S, 0, T, L, 1, sm));

    // ewma_fit(in, S, T, ld, smoothing, err)
#define EFIT(in_, S_, T_, ld_, sm_) \
    sts_ewma_fit_host(in_, S_, T_, ld_, sm_, nullptr), sts_ewma_fit(in_, S_, T_, ld_, sm_, nullptr, nullptr)
    FAULT("ewma_fit null in", EFIT(N, S, T, T, sm));
    FAULT("ewma_fit ld < T", EFIT(in, S, T, T - 1, sm));
    FAULT("ewma_fit S < 0", EFIT(in, -1, T, T, sm));
    FAULT("ewma_fit empty series", EFIT(in, S, 0, T, sm));
    FAULT("ewma_fit null output", EFIT(in, S, T, T, N));
    NOWORK("ewma_fit S = 0", EFIT(in, 0, T, T, N));

    // ar_fit(in, S, T, ld, p, noIntercept, c, coef, err)
#define ARFIT(in_, S_, T_, ld_, p_, c_, cf_) \
    sts_ar_fit_host(in_, S_, T_, ld_, p_, 0, c_, cf_, nullptr), sts_ar_fit(in_, S_, T_, ld_, p_, 0, c_, cf_, nullptr, nullptr)
    FAULT("ar_fit null in", ARFIT(N, S, T, T, 2, c, cf));
    FAULT("ar_fit ld < T", ARFIT(in, S, T, T - 1, 2, c, cf));
    FAULT("ar_fit T < 0", ARFIT(in, S, -1, T, 2, c, cf));
    FAULT("ar_fit p = 0", ARFIT(in, S, T, T, 0, c, cf));
    FAULT("ar_fit p = 32", ARFIT(in, S, T, T, 32, c, cf));
    FAULT("ar_fit too short", ARFIT(in, S, 6, 6, 3, c, cf));
    FAULT("ar_fit null c", ARFIT(in, S, T, T, 2, N, cf));
    FAULT("ar_fit null coef", ARFIT(in, S, T, T, 2, c, N));
    NOWORK("ar_fit S = 0", ARFIT(in, 0, T, T, 2, N, N));

    // ar_fit_remove(in, out, S, T, ld, p, noIntercept, c, coef, err)
#define ARFR(in_, out_, S_, T_, ld_, p_, c_, cf_)                         \
    sts_ar_fit_remove_host(in_, out_, S_, T_, ld_, p_, 0, c_, cf_, nullptr), \
        sts_ar_fit_remove(in_, out_, S_, T_, ld_, ld_, p_, 0, c_, cf_, nullptr, nullptr)
    FAULT("ar_fit_remove null out", ARFR(in, N, S, T, T, 2, c, cf));
    FAULT("ar_fit_remove null in", ARFR(N, out, S, T, T, 2, c, cf));
    FAULT("ar_fit_remove alias", ARFR(in, in, S, T, T, 2, c, cf));
    FAULT("ar_fit_remove ld < T", ARFR(in, out, S, T, T - 1, 2, c, cf));
    FAULT("ar_fit_remove S < 0", ARFR(in, out, -1, T, T, 2, c, cf));
    FAULT("ar_fit_remove p = 0", ARFR(in, out, S, T, T, 0, c, cf));
    FAULT("ar_fit_remove p = 40", ARFR(in, out, S, T, T, 40, c, cf));
    FAULT("ar_fit_remove too short", ARFR(in, out, S, 4, 4, 2, c, cf));
    FAULT("ar_fit_remove null coef", ARFR(in, out, S, T, T, 2, c, N));
    NOWORK("ar_fit_remove S = 0", ARFR(in, out, 0, T, T, 2, c, cf));

    // garch_fit(in, S, T, ld, params, err); argarch_fit(in, S, T, ld, c, phi, params, err)
#define GFIT(in_, S_, T_, ld_, par_) \
    sts_garch_fit_host(in_, S_, T_, ld_, par_, nullptr), sts_garch_fit(in_, S_, T_, ld_, par_, nullptr, nullptr)
    FAULT("garch_fit null in", GFIT(N, S, T, T, par));
    FAULT("garch_fit ld < T", GFIT(in, S, T, T - 1, par));
    FAULT("garch_fit S < 0", GFIT(in, -1, T, T, par));
    FAULT("garch_fit null params", GFIT(in, S, T, T, N));
    NOWORK("garch_fit S = 0", GFIT(in, 0, T, T, N));
#define AGFIT(in_, S_, T_, ld_, c_, phi_, par_) \
    sts_argarch_fit_host(in_, S_, T_, ld_, c_, phi_, par_, nullptr), sts_argarch_fit(in_, S_, T_, ld_, c_, phi_, par_, nullptr, nullptr)
    FAULT("argarch_fit null in", AGFIT(N, S, T, T, c, cf, par));
    FAULT("argarch_fit ld < T", AGFIT(in, S, T, T - 1, c, cf, par));
    FAULT("argarch_fit T < 0", AGFIT(in, S, -1, T, c, cf, par));
    FAULT("argarch_fit null c", AGFIT(in, S, T, T, N, cf, par));
    FAULT("argarch_fit null phi", AGFIT(in, S, T, T, c, N, par));
    FAULT("argarch_fit null params", AGFIT(in, S, T, T, c, cf, N));
    FAULT("argarch_fit T < 3", AGFIT(in, S, 2, 2, c, cf, par));
    NOWORK("argarch_fit S = 0", AGFIT(in, 0, T, T, c, cf, par));

    // ar_remove / ar_add(in, out, S, T, ld, c, coef, p)
#define AR(fn, in_, out_, S_, T_, ld_, c_, cf_, p_) \
    fn##_host(in_, out_, S_, T_, ld_, c_, cf_, p_), fn(in_, out_, S_, T_, ld_, ld_, c_, cf_, p_, nullptr)
    FAULT("ar_remove null in", AR(sts_ar_remove, N, out, S, T, T, c, cf, 2));
    FAULT("ar_remove null out", AR(sts_ar_remove, in, N, S, T, T, c, cf, 2));
    FAULT("ar_remove ld < T", AR(sts_ar_remove, in, out, S, T, T - 1, c, cf, 2));
    FAULT("ar_remove S < 0", AR(sts_ar_remove, in, out, -1, T, T, c, cf, 2));
    FAULT("ar_remove p < 0", AR(sts_ar_remove, in, out, S, T, T, c, cf, -1));
    FAULT("ar_remove null c", AR(sts_ar_remove, in, out, S, T, T, N, cf, 2));
    FAULT("ar_remove null coef", AR(sts_ar_remove, in, out, S, T, T, c, N, 2));
    FAULT("ar_remove in place null c, p = 0", AR(sts_ar_remove, in, in, S, T, T, N, N, 0));
    NOWORK("ar_remove T = 0", AR(sts_ar_remove, in, out, S, 0, T, c, cf, 2));
    FAULT("ar_add null in", AR(sts_ar_add, N, out, S, T, T, c, cf, 2));
    FAULT("ar_add null out", AR(sts_ar_add, in, N, S, T, T, c, cf, 2));
    FAULT("ar_add ld < T", AR(sts_ar_add, in, out, S, T, T - 1, c, cf, 2));
    FAULT("ar_add T < 0", AR(sts_ar_add, in, out, S, -1, T, c, cf, 2));
    FAULT("ar_add p < 0", AR(sts_ar_add, in, out, S, T, T, c, cf, -3));
    FAULT("ar_add null c", AR(sts_ar_add, in, out, S, T, T, N, cf, 2));
    FAULT("ar_add null coef", AR(sts_ar_add, in, out, S, T, T, c, N, 2));
    NOWORK("ar_add S = 0, p = 0", AR(sts_ar_add, in, out, 0, T, T, N, N, 0));

    // dwtest(in, S, T, ld, stat); kpsstest(in, S, T, ld, regression, stat)
#define DW(in_, S_, T_, ld_, st_) sts_dw_test_host(in_, S_, T_, ld_, st_), sts_dw_test(in_, S_, T_, ld_, st_, nullptr)
    FAULT("dwtest null in", DW(N, S, T, T, st));
    FAULT("dwtest ld < T", DW(in, S, T, T - 1, st));
    FAULT("dwtest S < 0", DW(in, -1, T, T, st));
    FAULT("dwtest null stat", DW(in, S, T, T, N));
    FAULT("dwtest empty series", DW(in, S, 0, T, st));
    NOWORK("dwtest S = 0", DW(in, 0, T, T, N));
#define KPSS(in_, S_, T_, ld_, reg_, st_) \
    sts_kpss_test_host(in_, S_, T_, ld_, reg_, st_), sts_kpss_test(in_, S_, T_, ld_, reg_, st_, nullptr)
    FAULT("kpsstest regression nc", KPSS(in, S, T, T, STS_REG_NC, st));
    FAULT("kpsstest regression ctt", KPSS(in, S, T, T, STS_REG_CTT, st));
    FAULT("kpsstest null in", KPSS(N, S, T, T, STS_REG_C, st));
    FAULT("kpsstest ld < T", KPSS(in, S, T, T - 1, STS_REG_C, st));
    FAULT("kpsstest T < 0", KPSS(in, S, -1, T, STS_REG_C, st));
    FAULT("kpsstest null stat", KPSS(in, S, T, T, STS_REG_CT, N));
    FAULT("kpsstest too short", KPSS(in, S, 2, 2, STS_REG_CT, st));
    NOWORK("kpsstest S = 0", KPSS(in, 0, T, T, STS_REG_C, st));

    // adftest(in, S, T, ld, maxLag, regression, stat, pvalue, err); lbtest(in, S, T, ld, maxLag, stat, pvalue)
#define ADF(in_, S_, T_, ld_, p_, reg_, st_, pv_)                          \
    sts_adf_test_host(in_, S_, T_, ld_, p_, reg_, st_, pv_, nullptr), \
        sts_adf_test(in_, S_, T_, ld_, p_, reg_, st_, pv_, nullptr, nullptr)
    FAULT("adftest regression 4", ADF(in, S, T, T, 2, 4, st, pv));
    FAULT("adftest regression -1", ADF(in, S, T, T, 2, -1, st, pv));
    FAULT("adftest maxLag < 0", ADF(in, S, T, T, -1, STS_REG_C, st, pv));
    FAULT("adftest maxLag 32", ADF(in, S, T, T, 32, STS_REG_C, st, pv));
    FAULT("adftest null in", ADF(N, S, T, T, 2, STS_REG_C, st, pv));
    FAULT("adftest ld < T", ADF(in, S, T, T - 1, 2, STS_REG_C, st, N));
    FAULT("adftest S < 0", ADF(in, -1, T, T, 2, STS_REG_C, st, pv));
    FAULT("adftest null stat", ADF(in, S, T, T, 2, STS_REG_C, N, pv));
    FAULT("adftest too short", ADF(in, S, 8, 8, 3, STS_REG_CTT, st, N));
    NOWORK("adftest S = 0", ADF(in, 0, T, T, 2, STS_REG_C, N, N));
#define LB(in_, S_, T_, ld_, p_, st_, pv_) \
    sts_lb_test_host(in_, S_, T_, ld_, p_, st_, pv_), sts_lb_test(in_, S_, T_, ld_, p_, st_, pv_, nullptr)
    FAULT("lbtest maxLag 0", LB(in, S, T, T, 0, st, pv));
    FAULT("lbtest null in", LB(N, S, T, T, 5, st, pv));
    FAULT("lbtest ld < T", LB(in, S, T, T - 1, 5, st, N));
    FAULT("lbtest T < 0", LB(in, S, -1, T, 5, st, pv));
    FAULT("lbtest null stat", LB(in, S, T, T, 5, N, pv));
    FAULT("lbtest empty series", LB(in, S, 0, T, 5, st, pv));
    NOWORK("lbtest S = 0", LB(in, 0, T, T, 5, N, N));

    // bptest(resid, S, T, ld, factors, k, ld_f, fs, stat, pvalue, err); bgtest: + maxLag after fs
#define BP(e_, S_, T_, ld_, f_, k_, ldf_, fs_, st_, pv_)                          \
    sts_bp_test_host(e_, S_, T_, ld_, f_, k_, ldf_, fs_, st_, pv_, nullptr), \
        sts_bp_test(e_, S_, T_, ld_, f_, k_, ldf_, fs_, st_, pv_, nullptr, nullptr)
#define BG(e_, S_, T_, ld_, f_, k_, ldf_, fs_, p_, st_, pv_)                          \
    sts_bg_test_host(e_, S_, T_, ld_, f_, k_, ldf_, fs_, p_, st_, pv_, nullptr), \
        sts_bg_test(e_, S_, T_, ld_, f_, k_, ldf_, fs_, p_, st_, pv_, nullptr, nullptr)
    FAULT("bptest k = 0", BP(in, S, T, T, f, 0, T, 0, st, pv));
    FAULT("bptest k > max", BP(in, S, T, T, f, STS_MAX_FACTORS + 1, T, 0, st, pv));
    FAULT("bptest null resid", BP(N, S, T, T, f, 2, T, 0, st, pv));
    FAULT("bptest ld < T", BP(in, S, T, T - 1, f, 2, T, 0, st, N));
    FAULT("bptest S < 0", BP(in, -1, T, T, f, 2, T, 0, st, pv));
    FAULT("bptest null stat", BP(in, S, T, T, f, 2, T, 0, N, pv));
    FAULT("bptest ld_f < T", BP(in, S, T, T, f, 2, T - 1, 0, st, pv));
    FAULT("bptest fs overlaps", BP(in, S, T, T, f, 2, T, 2 * T - 1, st, pv));
    FAULT("bptest fs < 0", BP(in, S, T, T, f, 2, T, -1, st, pv));
    FAULT("bptest null factors", BP(in, S, T, T, N, 2, T, 0, st, pv));
    FAULT("bptest null per-series factors", BP(in, S, T, T, N, 2, T, 2 * T, st, pv));
    FAULT("bptest too short", BP(in, S, 3, 3, f, 2, 3, 0, st, pv));
    NOWORK("bptest S = 0", BP(in, 0, T, T, f, 2, T, 0, N, N));
    FAULT("bgtest k = 0", BG(in, S, T, T, f, 0, T, 0, 2, st, pv));
    FAULT("bgtest k > max", BG(in, S, T, T, f, STS_MAX_FACTORS + 1, T, 2 * T, 2, st, pv));
    FAULT("bgtest maxLag 0", BG(in, S, T, T, f, 2, T, 0, 0, st, pv));
    FAULT("bgtest maxLag 32", BG(in, S, T, T, f, 2, T, 0, 32, st, pv));
    FAULT("bgtest null resid", BG(N, S, T, T, f, 2, T, 0, 2, st, pv));
    FAULT("bgtest ld < T", BG(in, S, T, T - 1, f, 2, T, 2 * T, 2, st, N));
    FAULT("bgtest T < 0", BG(in, S, -1, T, f, 2, T, 0, 2, st, pv));
    FAULT("bgtest null stat", BG(in, S, T, T, f, 2, T, 0, 2, N, pv));
    FAULT("bgtest ld_f < T", BG(in, S, T, T, f, 2, T - 1, 2 * T, 2, st, pv));
    FAULT("bgtest fs overlaps", BG(in, S, T, T, f, 2, T + 1, 2 * T, 2, st, pv));
    FAULT("bgtest null factors", BG(in, S, T, T, N, 2, T, 0, 2, st, pv));
    FAULT("bgtest too short", BG(in, S, 6, 6, f, 2, 6, 0, 3, st, pv));
    NOWORK("bgtest S = 0", BG(in, 0, T, T, f, 2, T, 2 * T, 2, N, N));
}

static void run_checks(int tid) {
    const int64_t S = 3, T = 50;
    std::vector<double> in(S * T, 1.0), out(S * T), acf(S * 70), c(S), coef(S * 8), sm(S, 0.2), par(S * 3);
    std::vector<int32_t> err(S);
    for (int64_t i = 0; i < S * T; i++) in[i] = std::sin(0.1 * (double)i) + (i % 7 == 3 ? NAN : 0.0);

    // ---- argument validation (no device needed) ----
    expect(sts_fill_host(nullptr, out.data(), S, T, T, STS_FILL_LINEAR, nullptr), STS_ERR_BAD_ARG, "fill null in");
    expect(sts_fill_host(in.data(), in.data(), S, T, T, STS_FILL_LINEAR, nullptr), STS_ERR_BAD_ARG, "fill alias");
    expect(sts_fill_host(in.data(), out.data(), S, T, T, 99, nullptr), STS_ERR_UNSUPPORTED_METHOD, "fill method");
    expect(sts_fill_host(in.data(), out.data(), S, T, T - 1, STS_FILL_SPLINE, nullptr), STS_ERR_BAD_ARG,
           "fill spline ld < T");
    expect(sts_fill_host(in.data(), out.data(), S, T, T, STS_FILL_SPLINE + 1, nullptr), STS_ERR_UNSUPPORTED_METHOD,
           "fill method past spline");
    expect(sts_fill_host(in.data(), out.data(), S, T, T - 1, STS_FILL_LINEAR, nullptr), STS_ERR_BAD_ARG, "fill ld < T");
    expect(sts_fill_host(in.data(), out.data(), -1, T, T, STS_FILL_LINEAR, nullptr), STS_ERR_BAD_ARG, "fill S < 0");
    expect(sts_autocorr_host(in.data(), S, T, T, -1, acf.data()), STS_ERR_BAD_ARG, "autocorr K < 0");
    expect(sts_autocorr_host(in.data(), S, T, T, 5, nullptr), STS_ERR_BAD_ARG, "autocorr null out");
    expect(sts_fill_autocorr_host(in.data(), out.data(), S, T, T, 42, 5, acf.data(), nullptr),
           STS_ERR_UNSUPPORTED_METHOD, "fill_autocorr method");
    expect(sts_diff_at_lag_host(in.data(), out.data(), S, T, T, 3, 2), STS_ERR_REQUIREMENT, "diff start < lag");
    expect(sts_diff_at_lag_host(in.data(), out.data(), S, T, T, -1, 0), STS_ERR_BAD_ARG, "diff lag < 0");
    expect(sts_lag_matrix_host(in.data(), out.data(), S, T, T, T + 1, 1), STS_ERR_BAD_ARG, "lag maxLag > T");
    expect(sts_ewma_add_host(in.data(), out.data(), S, T, T, nullptr), STS_ERR_BAD_ARG, "ewma null smoothing");
    expect(sts_ewma_remove_host(in.data(), nullptr, S, T, T, sm.data()), STS_ERR_NULL_DEST, "ewma remove null dest");
    expect(sts_ar_fit_host(in.data(), S, T, T, 0, 0, c.data(), coef.data(), nullptr), STS_ERR_BAD_ARG, "ar p = 0");
    expect(sts_ar_fit_host(in.data(), S, T, T, 32, 0, c.data(), coef.data(), nullptr), STS_ERR_BAD_ARG, "ar p = 32");
    expect(sts_ar_fit_host(in.data(), S, 6, 6, 3, 0, c.data(), coef.data(), nullptr), STS_ERR_NOT_ENOUGH_DATA,
           "ar too short");
    expect(sts_ar_fit_remove_host(in.data(), in.data(), S, T, T, 2, 0, c.data(), coef.data(), nullptr),
           STS_ERR_BAD_ARG, "ar_fit_remove alias");
    expect(sts_ar_remove_host(in.data(), out.data(), S, T, T, nullptr, coef.data(), 2), STS_ERR_BAD_ARG,
           "ar remove null model");
    expect(sts_argarch_fit_host(in.data(), S, 2, 2, c.data(), coef.data(), par.data(), nullptr),
           STS_ERR_NOT_ENOUGH_DATA, "argarch T < 3");
    expect(sts_garch_fit_host(in.data(), S, T, T, nullptr, nullptr), STS_ERR_BAD_ARG, "garch null params");
    expect(sts_host_alloc(16, nullptr), STS_ERR_BAD_ARG, "host_alloc null out");
    expect(sts_staging_stats(nullptr), STS_ERR_BAD_ARG, "staging_stats null");
    double st8[8];
    expect(sts_staging_stats(st8), STS_OK, "staging_stats");
    expect(sts_staging_release(), STS_OK, "staging_release");
    // empty panels are no-ops
    expect(sts_fill_host(in.data(), out.data(), 0, T, T, STS_FILL_LINEAR, nullptr), STS_OK, "fill S = 0");
    expect(sts_fill_method_from_name("linear"), STS_FILL_LINEAR, "method name");
    expect(sts_fill_method_from_name("bogus"), -2, "method name bogus");
    expect(sts_fill_method_from_name(nullptr), -2, "method name null");

    host_device_table();

    // ---- valid calls: no gfx950 device here, so they must fail cleanly ----
    expect_no_device(sts_fill_host(in.data(), out.data(), S, T, T, STS_FILL_LINEAR, err.data()), "fill");
    expect_no_device(sts_fill_autocorr_host(in.data(), out.data(), S, T, T, STS_FILL_LINEAR, 20, acf.data(), nullptr),
                     "fill_autocorr");
    expect_no_device(sts_fill_diff_ewma_host(in.data(), out.data(), S, T, T, STS_FILL_PREVIOUS, 1, sm.data(), nullptr),
                     "fill_diff_ewma");
    expect_no_device(sts_ar_fit_remove_host(in.data(), out.data(), S, T, T, 5, 0, c.data(), coef.data(), nullptr),
                     "ar_fit_remove");
    expect_no_device(sts_init(0), "init");
    // staging pool controls
    expect(sts_staging_set_limit(0), STS_ERR_BAD_ARG, "staging limit 0");
    expect(sts_staging_set_limit(2 + tid % 3), STS_OK, "staging limit");
    expect(sts_staging_pool_info(nullptr), STS_ERR_BAD_ARG, "pool info null");
    // the thread-local error message: this thread's failing call, other threads' calls in
    // between, still this thread's message
    char want[64];
    std::snprintf(want, sizeof want, "S=%d,", -(tid + 1));
    expect(sts_fill_host(in.data(), out.data(), -(tid + 1), T, T, STS_FILL_LINEAR, nullptr), STS_ERR_BAD_ARG,
           "fill S < 0 (per thread)");
    for (int k = 0; k < 200; k++) std::this_thread::yield();
    const std::string msg = sts_last_error();
    if (msg.find(want) == std::string::npos) {
        std::printf("FAIL thread %d: last error \"%s\" is not its own (%s)\n", tid, msg.c_str(), want);
        failures++;
    }
    sts_staging_release();
}

int main(int argc, char** argv) {
    const int nthreads = argc > 1 ? std::atoi(argv[1]) : 0;
    if (nthreads <= 0) {
        run_checks(0);
    } else {
        for (int rep = 0; rep < 3; rep++) {
            std::vector<std::thread> th;
            for (int t = 0; t < nthreads; t++) th.emplace_back(run_checks, t);
            for (auto& t : th) t.join();
        }
    }
    std::printf("host-against-device table: %d rows\n", table_rows.load());
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
