// sts_internal.hpp -- shared declarations between the C-ABI layer (sts_api.cpp) and
// the HIP kernel translation units.  Host-side launchers only: no kernel bodies here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "sts.h"
#include "sts_transforms.h"
#include "sts_sample.h"
#include "sts_index.h"
#include "sts_regress.h"
#include "sts_cross.h"
#include "sts_roll.h"

namespace sts {

// Tile geometry of the imputation / autocorrelation tile kernel (sts_tile.hip).
// A tile is TW consecutive steps of ONE series plus HB steps of look-back and HA
// steps of look-ahead (ACF pairs reach 16*NT-1 <= 79 steps past the tile).
constexpr int kHB = 64;
constexpr int kHA = 128;
// per-chunk ACF partials: [0, 64) lag products, [64] sum y and [65] sum y^2 over the
// series' middle (sts_acf.hpp), [66] the shift c, [67] pad
constexpr int kPartStride = 68;
constexpr int kPartSum = 64, kPartSq = 65, kPartShift = 66;
// autocorr head / tail length handled per lag by the finalize (sts_acf.hpp); K <= kAcfEdge
// on the fused paths, and series shorter than 2 kAcfEdge take the direct two-pass finalize
constexpr int kAcfEdge = 64;
// short fused fill + ACF: the two-series-per-block form (sts_short.hip short_pair_kernel) by default
constexpr bool kShortPairDefault = false;

struct TileArgs {
    const double* in;
    double* out;          // filled output (may be null when not written)
    double* lagmat;       // lag-matrix output (may be null)
    double* partials;     // ACF partial sums [tiles][kPartStride] (may be null)
    int32_t* err;         // per-series error flags (may be null)
    int64_t S, T, ld_in, ld_out;
    int64_t tiles_per_series;
    int64_t tiles_per_chunk;    // tiles one workgroup walks (register-prefetched pipeline)
    int64_t chunks_per_series;  // = ceil(tiles_per_series / tiles_per_chunk)
    int K;                // ACF lags (0 = no ACF)
    int max_lag;          // lag matrix p
    int include_original; // lag matrix inc
    double* acf_fused;    // seg kernel, one segment per series: final ACF written directly (S x K)
    const double* shift;  // tile kernel with K > 0: per-series ACF shift (launch_acf_shift)
    int err_all;          // seg kernel, one segment per series: err[s] written for every series
};

struct FinalizeArgs {
    const double* F;      // filled series (or raw input when no fill), ld = ldF
    const double* partials;
    double* acf;          // S x K
    int64_t S, T, ldF, parts_per_series;   // ACF partials per series (one per chunk)
    int K;
    int32_t* exact;       // per series, zeroed by the caller: set where rule 3 (sts_acf.hpp) fires,
                          // for launch_acf_exact to recompute that series by the reference's loop
};

// A/B experiment knobs (environment variables) exist only in the -DSTS_AB build
// (build/libsts_hip_ab.so, tools/ and the knob tests); the product libsts_hip.so never reads
// its environment, so a Spark executor's environment cannot change which kernels run.
#ifdef STS_AB
inline const char* ab_knob(const char* name) { return std::getenv(name); }
#else
inline const char* ab_knob(const char*) { return nullptr; }
#endif

// status helpers of the C-ABI layer (sts_api.cpp): the first failing entry of a host copy of
// err_per_series as the reference's exception; a status with a thread-local message
int series_status(const int32_t* h, int64_t S, const char* what);
int set_error(int status, const char* msg);
// Run fn(ctx) -- a call of a device entry point -- in validate-only mode: the entry point
// checks its arguments and returns their status, stopping at its first device action.
// *has_work says whether it got that far: false with STS_OK means the entry point returned
// before any device action (an empty panel, lag 0), so the call has nothing to do.
// Every `_host` entry point validates this way -- its own device call, on the caller's pointers,
// shapes and ld -- before staging anything, and stages nothing without work (sts_host.cpp staged()).
int validate_call(int (*fn)(void*), void* ctx, bool* has_work);
template <class F>
int validate(F&& f, bool* has_work) {
    return validate_call([](void* c) { return (*static_cast<F*>(c))(); }, static_cast<void*>(&f), has_work);
}

// A series range that one launch cannot hold (a grid's y dimension ends at 65 535): launch(s0, n)
// enqueues series s0 .. s0 + n of consecutive slices of at most max_per_launch series; every
// slice's launch is checked, and the first error ends the loop.
template <class F>
hipError_t for_series_slices(int64_t S, int64_t max_per_launch, F&& launch) {
    for (int64_t s0 = 0; s0 < S; s0 += max_per_launch) {
        launch(s0, S - s0 < max_per_launch ? S - s0 : max_per_launch);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// launchers (return hipError_t of the launch)
hipError_t launch_tile(int method, int tw, const TileArgs& a, hipStream_t st);
hipError_t launch_acf_finalize(const FinalizeArgs& a, hipStream_t st);
// rule 3's fallback for the series flagged in exact[S] (acf_finalize / the wide finalize): every
// lag 1..K by the reference's two-pass loop, F streamed through LDS (sts_acf.hpp acf_exact_stream)
hipError_t launch_acf_exact(const double* F, int64_t S, int64_t T, int64_t ldF, int K, const int32_t* exact,
                            double* acf, hipStream_t st);
// per-series robust ACF shift (sts_acf.hpp) for the tile kernel
// method: the fill the series will take (STS_FILL_PREVIOUS reverses the shift's fallback)
hipError_t launch_acf_shift(const double* in, int64_t S, int64_t T, int64_t ld, int method, double* shift,
                            hipStream_t st);
// numLags above the fused kernels' 63 (sts_acf_wide.hip): partial count for S x T x K, and the
// lag-block MFMA pass + finalize on a filled panel F (shift: launch_acf_shift of F)
constexpr int kFusedMaxLags = 63;
size_t acf_wide_partials(int64_t S, int64_t T, int K);
hipError_t launch_acf_wide(const double* F, int64_t S, int64_t T, int64_t ld, const double* shift, int K, double* part,
                           double* acf, int32_t* exact, hipStream_t st);

// Wave-private segment kernel (sts_seg.hip): tiles of kSegW steps, kSegTiles tiles per
// wave.  TileArgs.tiles_per_series = ceil(T / kSegW), tiles_per_chunk = tiles per
// segment, chunks_per_series = segments per series.  seg_nt(K) < 0: K not supported.
constexpr int kSegW = 512;
constexpr int kSegTiles = 128;
int seg_nt(int K);
hipError_t launch_segment(int method, const TileArgs& a, hipStream_t st);
// fill('linear') + fused ACF with the whole series in one wave's registers (sts_short.hip):
// short_ok() says whether a one-segment, fused-ACF seg call may take it instead
bool short_ok(int method, int64_t T, int K);
hipError_t launch_short(int method, const TileArgs& a, hipStream_t st, bool pair);

// fillts "spline" (sts_spline.hip): series per launch for the (mu, z) scratch rows (16 B per
// step), and the batched launches over S series (scratch: spline_batch(S, T) x T double2)
int64_t spline_batch(int64_t S, int64_t T);
hipError_t launch_spline(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                         int32_t* err, double* scratch, int64_t batch, hipStream_t st);

hipError_t launch_diff(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                       int64_t ld_out, int lag, int start, hipStream_t st);
hipError_t launch_diff_inplace(double* x, int64_t S, int64_t T, int64_t ld, int lag, int start,
                               hipStream_t st);
hipError_t launch_lagmat(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                         int max_lag, int include_original, hipStream_t st);
hipError_t launch_ewma_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                              int64_t ld_out, const double* sm, hipStream_t st);
hipError_t launch_ar_remove(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                            int64_t ld_out, const double* c, const double* coef, int p,
                            hipStream_t st);

// series-per-lane recurrences (sts_recur.hip)
enum RecurOp { kEwmaAdd = 0, kEwmaRemoveInplace = 1, kArAdd = 2, kArRemoveInplace = 3,
               kFillDiffEwma = 4, kDiffInplace = 5,
               // sts_transforms.h r6 / r7: history of OUTPUTS at `lag`; one previous value per level (p = d <= 8)
               kInvDiffAtLag = 6, kDiffOrderD = 7, kInvDiffOrderD = 8 };
constexpr int kOrderDOnePass = 8;   // largest d the one-pass order-d lanes hold (one register per level)
struct RecurArgs {
    const double* in;
    double* out;
    int64_t S, T, ld_in, ld_out;
    const double* sm;     // EWMA smoothing per series
    const double* c;      // AR intercept per series
    const double* coef;   // AR coefficients [S][p]
    int p;                // AR order
    int lag, start;       // differencing
    int method;           // fill method for kFillDiffEwma
};
hipError_t launch_recur(RecurOp op, const RecurArgs& a, hipStream_t st);

// panel transforms (sts_transforms.hip; include/sts_transforms.h r1-r5)
hipError_t launch_quotients(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out, int lag,
                            bool minus_one, hipStream_t st);
// fillPrevious -> quotients in one pass, 1 <= lag <= kFillQuotMaxLag (one wave per series)
constexpr int kFillQuotMaxLag = 32;
hipError_t launch_fill_prev_quotients(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                                      int lag, bool minus_one, hipStream_t st);
hipError_t launch_fill_default(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                               double filler, hipStream_t st);
// out(s, j) = in(s, phase + j * n), j < T_out
hipError_t launch_downsample(const double* in, double* out, int64_t S, int64_t T_out, int64_t ld_in, int64_t ld_out, int n,
                             int phase, hipStream_t st);
// out(s, i), i < T_out = T * n: in(s, (i - phase) / n) on the grid, filler elsewhere
hipError_t launch_upsample(const double* in, double* out, int64_t S, int64_t T_out, int64_t ld_in, int64_t ld_out, int n,
                           int phase, double filler, hipStream_t st);
hipError_t launch_first_last(const double* in, int64_t S, int64_t T, int64_t ld, int64_t* first, int64_t* last,
                             hipStream_t st);

// AR fit (sts_ar.hip)
struct ArArgs {
    const double* in;
    double* out;          // remove output (null -> fit only)
    double* c;
    double* coef;
    int32_t* err;
    int64_t S, T, ld_in, ld_out;
    int p, no_intercept;
    // AR rule (sts_ar.hip / sts_ar_qr.hip): series the fast fit flags, appended by the fit
    // kernels (set by launch_ar_fit, not by callers)
    int64_t* qr_list;
    uint32_t* qr_count;
};
hipError_t launch_ar_fit(const ArArgs& a, hipStream_t st);
// the fast fit kernels only, flagged series counted into *count (device; AR rule diagnostic)
hipError_t launch_ar_rule_count(const ArArgs& a, uint32_t* count, hipStream_t st);
// the reference's Householder QR on the listed series (list == nullptr: series 0 .. n_direct-1;
// otherwise list[0 .. *count-1]); scratch = slots x ar_qr_wave_slot_elems doubles for p > 8
bool ar_qr_lane_ok(int p);
size_t ar_qr_wave_slot_elems(int64_t T, int p, int no_intercept);
hipError_t launch_ar_qr(const ArArgs& a, const int64_t* list, const uint32_t* count, int64_t n_direct,
                        double* scratch, int slots, bool force_wave, hipStream_t st);

// EWMA.fitModel and EWMAModel.sse / gradient (sts_ewma_fit.hip)
struct EwmaFitArgs {
    const double* in;
    int64_t S, T, ld;
    double* smoothing;    // fit: output; sse / gradient: input (per series)
    double* sse;          // sse / gradient outputs (may be null)
    double* grad;
    int32_t* err;         // fit: per-series status (may be null)
    int32_t* evals;       // fit: objective evaluations commons-math3 counted (may be null)
};
hipError_t launch_ewma_fit(const EwmaFitArgs& a, bool fit, hipStream_t st);

// GARCH.fitModel / GARCHModel.logLikelihood + gradient and the GARCH / ARGARCH
// time-dependent effects (sts_garch.hip)
struct GarchFitArgs {
    const double* in;
    int64_t S, T, ld;
    double* params;       // S x 3 (omega, alpha, beta): fit output / evaluation input
    int32_t* err;         // fit: per-series status (optional)
    int keep_err;         // fit: leave a nonzero err entry as it is (ARGARCH: the AR stage's)
    int32_t* evals;       // fit: commons-math3 evaluation count (optional)
    double* loglik;       // evaluation: S
    double* grad;         // evaluation: S x 3, the reference's (alpha, beta, omega) order
    // fit, MaxEval tail (set by launch_garch_fit): a lane still running after pass_budget
    // passes parks its optimizer state in park[slot] (slot from park_ctr[0], < park_cap)
    // and garch_tail_kernel finishes it, one wave per series (park_ctr[1]: its work queue)
    void* park;           // park_cap x GarchOpt
    int64_t* park_ids;    // series of each slot
    int32_t* park_ctr;
    int park_cap;
    int pass_budget;      // 0: no tail phase
};
hipError_t launch_garch_fit(const GarchFitArgs& a, bool fit, hipStream_t st);
enum GarchOp { kGarchRemove = 0, kGarchAdd = 1, kArgarchRemove = 2, kArgarchRemoveInplace = 3, kArgarchAdd = 4 };
struct GarchEffectsArgs {
    const double* in;
    double* out;
    int64_t S, T, ld_in, ld_out;
    const double *c, *phi, *omega, *alpha, *beta;   // per series (c, phi: ARGARCH only)
};
hipError_t launch_garch_effects(int op, const GarchEffectsArgs& a, hipStream_t st);

// ARIMA(p, d, q) with MA terms (sts_arima.hip).  Every launcher works on ARMA level: the
// C-ABI layer differences the panel (launch_diff ping-pong) and passes the view it needs.
struct ArimaCssArgs {
    const double* in;     // the differenced series, .drop(d) applied: S x n_len, ld
    int64_t S, ld;
    int n_len;
    int p, q, icpt;
    const double* coef_in;   // S x n: the start (fit) or the evaluation point
    double* coef_out;        // fit: S x n
    int32_t* err;            // fit: per-series status (optional)
    int32_t* evals;          // fit: commons-math3 evaluation count (optional)
    double* loglik;          // evaluation: S (optional)
    double* grad;            // evaluation: S x n (optional)
};
hipError_t launch_arima_css(const ArimaCssArgs& a, bool fit, hipStream_t st);
// steps of a series one LDS chunk of arima_css_kernel holds (the tests straddle it)
constexpr int kArimaChunk = 64;
enum ArimaOp { kArimaRemove = 0, kArimaAdd = 1, kArimaIntegrate = 2 };
struct ArimaEffectsArgs {
    const double* in;     // remove: differencesOfOrderD(ts, d), full length
    double* out;          // may be in
    int64_t S, T, ld_in, ld_out;
    int p, q, icpt;
    const double* coef;   // S x n
    int start;            // kArimaIntegrate: inverseDifferencesAtLag(x, x, 1, start)
};
hipError_t launch_arima_effects(int op, const ArimaEffectsArgs& a, hipStream_t st);
struct ArimaForecastArgs {
    const double* ts;       // the panel: S x T, ld_ts
    const double* diffed;   // differencesOfOrderD(ts, d), full length (ts itself for d = 0)
    double* out;            // S x (T + n_future): the fitted differences and the forward curve
    int64_t S, T, ld_ts, ld_d, ld_out;
    int d, n_future;
    int p, q, icpt;
    const double* coef;
};
hipError_t launch_arima_forecast(const ArimaForecastArgs& a, hipStream_t st);
// forecast with d > 0 (S/models/ARIMA.scala:571-603): sum += level (first: sum = 0.0 + level);
// diag[s * d + k] = level(s, col); and the merge of ts, sum, the raw forecast and diag into out
hipError_t launch_arima_level_sum(const double* level, int64_t ld, double* sum, int64_t S, int64_t T, int first,
                                  hipStream_t st);
hipError_t launch_arima_diag(const double* level, int64_t ld, int64_t S, int64_t col, double* diag, int d, int k,
                             hipStream_t st);
hipError_t launch_arima_forecast_merge(const double* ts, int64_t ld_ts, const double* sum, const double* raw,
                                       const double* diag, double* out, int64_t ld_out, int64_t S, int64_t T, int d,
                                       int n_future, hipStream_t st);
struct ArimaHrArgs {
    const double* in;     // the differenced series, .drop(d) applied
    int64_t S, ld;
    int n_len;
    int p, q, icpt;
    const double* c;      // the AR(m) stage, m = max(p, q) + 1: intercepts S, coefficients S x m
    const double* phi;
    double* init_out;     // S x n
    int32_t* err;         // optional; a nonzero entry (the AR stage's) is kept
};
hipError_t launch_arima_hr(const ArimaHrArgs& a, hipStream_t st);

// statistical tests (sts_stattests.hip): one workgroup per series; series of up to kStatOneWave
// steps live in one wave's LDS block, longer ones are swept from global memory by kLongThreads
constexpr int64_t kStatOneWave = 2560;
constexpr int kLongThreads = 256;
struct StatArgs {
    const double* in;
    int64_t S, T, ld;
    double* stat;         // S
    int32_t* err;         // ADF: per-series status, zeroed by the caller
    int p;                // ADF: maxLag
    int q;                // trend columns: sts_regression's value (KPSS: 1 or 2)
    int L;                // KPSS: Newey-West lag
};
hipError_t launch_dw(const StatArgs& a, hipStream_t st);
hipError_t launch_kpss(const StatArgs& a, hipStream_t st);
hipError_t launch_adf(const StatArgs& a, hipStream_t st);
hipError_t launch_adf_pvalue(const double* stat, double* pv, int64_t S, int regression, hipStream_t st);
// Ljung-Box statistic (and p-value unless pv is null) from an S x K ACF
hipError_t launch_lb(const double* acf, int64_t S, int64_t T, int K, double* stat, double* pv, hipStream_t st);
// Breusch-Godfrey / Breusch-Pagan.  kMaxFactors bounds k: the kernels keep one accumulator and one
// basis value per factor in registers (unrolled to this bound) and an LDS row of it per lag window.
constexpr int kMaxFactors = STS_MAX_FACTORS;
// A factor panel and the scratch its orthonormal bases go to (sts_factor_basis.hpp): what the tests
// and the factor OLS share.  One basis for shared factors (fs == 0, every stride 0), else one per
// series of a chunk, indexed from the chunk's first series.
struct FactorBasisArgs {
    const double* factors;   // factor j of series s at factors[s * fs + j * ld_f + t]; fs == 0: shared
    int64_t ld_f, fs;
    int k;                   // factors, 1..kMaxFactors
    int64_t lo, n;           // rows lo .. lo + n of the factors are used
    double* basis;           // k x n per basis, basis b at basis + b * basis_stride
    int64_t basis_stride;
    int32_t* info;           // per basis 0 or STS_ERR_SINGULAR (rank deficient), b * info_stride
    int64_t info_stride;
    double* aux;             // null, or kOlsAux doubles per basis (R^-1, factor means, ...), b * aux_stride
    int64_t aux_stride;
};
// per-series factors of a one-wave series whose basis fits the LDS budget behind the series: the
// series' kernel builds it there (the OLS aux block rides on top), and no scratch basis is needed
constexpr size_t kOwnBasisLds = 48 << 10;
inline bool own_basis_fits(int64_t T, int k, int64_t n, int64_t fs) {
    return fs != 0 && T <= kStatOneWave && (size_t)(T + k * n) * sizeof(double) <= kOwnBasisLds;
}
// bases of series s0 .. s0 + nb (nb = 1 and s0 = 0 for shared factors) into f.basis / f.info, and
// into f.aux where it is not null
hipError_t launch_factor_basis(const FactorBasisArgs& f, int64_t s0, int64_t nb, hipStream_t st);

struct BgBpArgs {
    const double* in;        // residual panel
    int64_t S, T, ld;
    FactorBasisArgs f;       // lo = L, n = T - L; no aux
    int L;                   // BG: maxLag; BP: 0
    bool squares;            // BP: the response is e^2
    double* stat;            // S
    int32_t* err;            // per-series status, zeroed by the caller
};
// true when launch_bgbp's kernels build each series' basis in LDS themselves: the scratch is not used
inline bool own_basis(const BgBpArgs& a) { return own_basis_fits(a.T, a.f.k, a.f.n, a.f.fs); }
// statistics of series s0 .. s0 + ns
hipError_t launch_bgbp(const BgBpArgs& a, int64_t s0, int64_t ns, hipStream_t st);
hipError_t launch_chi2_pvalue(const double* stat, double* pv, int64_t S, int dof, hipStream_t st);

// OLS of a panel on factors and the effects pair (sts_regress.hip, include/sts_regress.h)
struct OlsArgs {
    const double* y;
    int64_t S, T, ld;
    FactorBasisArgs f;       // lo = 0, n = T; with aux
    double* beta;            // S x (k + 1) at ld_b
    double* se;              // optional, as beta
    int64_t ld_b;
    double* stats;           // optional, S x 4: rss, tss, r2, sigma2
    double* resid;           // optional, S x T at ld_r
    int64_t ld_r;
    int32_t* err;            // per-series status, zeroed by the caller
};
// which of launch_ols's kernels a call takes (tests name the seams): 0 = shared factors, several
// waves per workgroup with the basis staged in LDS; 1 = one wave per series, basis in the scratch;
// 2 = one wave per series that builds its own factors' basis in LDS (no scratch); 3 = 256-thread
// sweeps over global memory
int ols_regime(int64_t T, int k, int64_t fs);
// fits of series s0 .. s0 + ns
hipError_t launch_ols(const OlsArgs& a, int64_t s0, int64_t ns, hipStream_t st);
hipError_t launch_factor_effects(bool add, const double* in, double* out, int64_t S, int64_t T, int64_t ld_in,
                                 int64_t ld_out, const double* factors, int k, int64_t ld_f, int64_t fs,
                                 const double* beta, int64_t ld_b, hipStream_t st);

// covariance / correlation matrices (sts_cross.hip, include/sts_cross.h)
constexpr int kCrossTile = STS_CROSS_TILE;     // output tile of one workgroup, square
constexpr int kCrossChunk = STS_CROSS_CHUNK;   // steps of T per LDS stage
constexpr int64_t kCrossSplit = STS_CROSS_SPLIT;   // steps after which a partial sum over T is closed
constexpr int kCrossStat = 4;                  // per series in the scratch: mu, r, C_ii, flag (0 / 1 constant / 2 non-finite)
struct CrossArgs {
    const double* x;
    const double* y;         // null: the symmetric form
    int64_t Sx, Sy, T, ld_x, ld_y;
    int kind;
    double* out;
    int64_t ld_o;
    double* mean_x;          // optional
    double* mean_y;
    double* scratch;         // cross_plan().scratch_doubles doubles
};
// what a call launches: the tile grid, the segments of T (closed every kCrossSplit steps) and whether
// each segment gets a workgroup of its own (few tiles, long T) with a finalise kernel behind them
struct CrossPlan {
    int64_t ti, tj, tiles, nseg;
    bool split;
    size_t scratch_doubles;
};
CrossPlan cross_plan(int64_t Sx, int64_t Sy, int64_t T, bool symmetric);
// the prep kernel(s), the Gram kernel and, in a split plan, the finalise kernel
hipError_t launch_cross(const CrossArgs& a, hipStream_t st);

// rolling-window statistics (sts_roll.hip, include/sts_roll.h)
constexpr int kRollTile = STS_ROLL_TILE;       // steps of one row a workgroup owns
constexpr int kRollChains = STS_ROLL_CHAINS;   // outputs a thread carries at a time
constexpr int kRollCap = kRollTile + STS_ROLL_MAX_WINDOW - 1;   // doubles of one LDS buffer: a tile and its halo
struct RollArgs {
    const double* x;
    const double* y;         // pair ops only; ld_y == 0: one shared factor
    double* out;
    int64_t S, T, ld_x, ld_y, ld_out;
    int window, min_periods, op;
    bool pair;               // op is an sts_roll_pair_op
};
// a workgroup owns rows whole rows when T <= kRollTile (rows * (T + window - 1) <= kRollCap), else one
// tile of one row; tiles = tiles per row
struct RollPlan {
    int64_t tiles;
    int rows;
};
RollPlan roll_plan(int64_t T, int window);
hipError_t launch_roll(const RollArgs& a, hipStream_t st);

// seriesStats / removeInstantsWithNaNs / toInstants (sts_instants.hip)
hipError_t launch_series_stats(const double* in, double* out, int64_t S, int64_t T, int64_t ld, hipStream_t st);
hipError_t launch_nan_instants(const double* in, uint8_t* flags, int64_t S, int64_t T, int64_t ld, hipStream_t st);
int64_t active_scratch_elems(int64_t T);
hipError_t launch_active_instants(const uint8_t* flags, int64_t T, int64_t* active, int64_t* n_active,
                                  int64_t* scratch, hipStream_t st);
hipError_t launch_gather_instants(const double* in, double* out, const int64_t* active, int64_t n_active, int64_t S,
                                  int64_t ld_in, int64_t ld_out, hipStream_t st);
hipError_t launch_transpose(const double* in, double* out, int64_t S, int64_t T, int64_t ld_in, int64_t ld_out,
                            hipStream_t st);

// ingest formats (sts_ingest.hip)
hipError_t launch_wire_decode(const unsigned char* bytes, const int64_t* val_off, double* panel, int64_t S, int64_t T,
                              int64_t ld, hipStream_t st);
hipError_t launch_wire_encode(const double* panel, int64_t S, int64_t T, int64_t ld, const int64_t* val_off,
                              unsigned char* bytes, hipStream_t st);
hipError_t launch_observations(const int32_t* sid, const int64_t* loc, const double* val, int64_t n, double* panel,
                               int64_t S, int64_t T, int64_t ld, unsigned char* win, hipStream_t st);

// generators (sts_gen.hip)
hipError_t launch_gen_panel(double* out, int64_t s0, int64_t S, int64_t T, int64_t ld,
                            uint64_t seed, uint32_t nan_thr, hipStream_t st);
hipError_t launch_gen_ar(double* out, double* c, double* phi, int64_t s0, int64_t S, int64_t T,
                         int64_t ld, uint64_t seed, int p, hipStream_t st);

// samplers (sts_sample.hip; include/sts_sample.h): series s of the call draws
// z(seed, s0 + s, t0 + i), i < n (sts_normal.hpp)
struct SampleArgs {
    double* out;          // S x n, ld
    int64_t s0, S, n, ld, t0;
    uint64_t seed;
    const double *c, *phi, *omega, *alpha, *beta;   // per series (GARCH: omega, alpha, beta; ARGARCH: all)
};
hipError_t launch_sample_normal(const SampleArgs& a, hipStream_t st);
hipError_t launch_garch_sample(bool ar, const SampleArgs& a, hipStream_t st);

// date-time indices and rebasing (sts_index.hip; include/sts_index.h i1-i5).  A uniform index
// arrives validated (sts_index.hpp make_uniform); u == nullptr in launch_index_locs: irregular
namespace ix { struct Uniform; }
hipError_t launch_index_instants(const ix::Uniform& u, int64_t* out, hipStream_t st);
hipError_t launch_index_locs(const int64_t* millis, int64_t n, const ix::Uniform* u, const int64_t* instants,
                             int64_t n_instants, int64_t* loc, hipStream_t st);
hipError_t launch_rebase_shift(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                               int64_t ld_out, int64_t shift, double dflt, hipStream_t st);
hipError_t launch_rebase_map(const double* in, double* out, int64_t S, int64_t T_in, int64_t T_out, int64_t ld_in,
                             int64_t ld_out, const int64_t* map, double dflt, hipStream_t st);
hipError_t launch_align_uniform(const double* values, const int64_t* offsets, const int64_t* start_loc, int64_t S,
                                int64_t T_out, double* out, int64_t ld_out, double dflt, hipStream_t st);

}  // namespace sts
