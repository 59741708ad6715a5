"""The chunk plan of the `_host` staging pipeline (spark-timeseries_amd/csrc/sts_host.cpp, staged()),
restated in plain Python, and one row per chunked `_host` entry point.

The plan.  staged() sums the DEVICE row bytes of every per-series array of the call:

    per_series = sum(width * itemsize)    over the call's per-series arrays, where
                   - an output on an input's host rows (an in-place call) counts once,
                   - the internal int32 status array counts whenever the wrapper has one, also
                     when the caller passes err = NULL,
                   - an optional output passed as NULL still counts,
                   - shared factors, the shared roll factor and the rebase map count for nothing
                     (they are uploaded once, outside the pipeline);
    ns      = max(1, min(S, CHUNK // per_series))     series per chunk
    nchunks = ceil(S / ns)                            chunk i runs on slot i % SLOTS

Every width below is taken from the wrapper's description in the headers (include/sts*.h), not from
the library.  Nothing here needs a GPU, the library or the oracle: tests/test_staging_plan_cpu.py
proves the table complete and every shape's seam conditions, tests/test_staging_seams_gpu.py runs
the shapes.
"""
from collections import namedtuple

CHUNK = 64 << 20          # STS_STAGE_MB: device bytes (in + out) per chunk
SLOTS = 5                 # STS_STAGE_SLOTS
ALIGN = 256
MAX_ARGS = 16
# what sts_staging_pool_info()[7] reports for these constants: the GPU module asserts it, so a library
# built with another chunk size or slot count fails loudly instead of no longer crossing a seam
POOL_KEEP = SLOTS * (CHUNK + MAX_ARGS * ALIGN)

ITEMSIZE = {"f8": 8, "i8": 8, "i4": 4}

# The `_host` names of sparkts/_native.py's signature tables that have no chunks, and why.
EXCLUDED = {
    "sts_host_alloc": "allocates pinned memory: no panel",
    "sts_host_free": "frees pinned memory: no panel",
    "sts_cross_moments_host": "every output depends on two series anywhere in the two panels, so both panels are "
                              "copied whole: no chunks (tests/test_cross_gpu.py covers it)",
}

# One per-series array.  width: device elements per series, a function of the call's parameters.
# kind: where series s starts on the host --
#   panel   s * ld        (T doubles per series, the call's ld)
#   vec     s * width     (packed)
#   ypanel  s * ld_y      (sts_roll_pair_host's per-series y)
#   fblock  s * fs        (per-series factors: one block of (k - 1) * ld_f + T doubles)
#   zero    0             (the one zero that stands in for every series' coef row at p = 0)
Arr = namedtuple("Arr", "name dir dtype width kind")


def _T(p):
    return p["T"]


def panel_in(name="in"):
    return Arr(name, "in", "f8", _T, "panel")


def panel_out(name="out"):
    return Arr(name, "out", "f8", _T, "panel")


def vec_in(name, width=lambda p: 1):
    return Arr(name, "in", "f8", width, "vec")


def vec_out(name, width=lambda p: 1, dtype="f8"):
    return Arr(name, "out", dtype, width, "vec")


def fblock(p):
    """the per-series factor block, or nothing for a shared factor matrix"""
    if p["fs"] == "shared":
        return []
    return [Arr("factors", "in", "f8", lambda q: (q["k"] - 1) * q["ld_f"] + q["T"], "fblock")]


# A variant of a row: its id, the parameters it overrides, and
#   inplace  the output named `out` is the input named `in`
#   null     names of optional outputs passed as NULL ("err" among them)
#   chunks   3 (S = 2 ns + 37) or 6 (S = 5 ns + 37: chunk 5 reuses slot 0)
#   mixed    also run with the inputs pinned and the outputs pageable
class Variant(object):
    def __init__(self, id, T=390, chunks=3, inplace=False, null=(), mixed=False, **params):
        self.id, self.T, self.chunks, self.inplace, self.null, self.mixed = id, T, chunks, inplace, tuple(null), mixed
        self.params = params


V = Variant


# A row: the wrapper, its free parameters, its per-series arrays in the wrapper's order (a function of
# the parameters: a shared factor matrix is no per-series array), whether it has a status array,
# what its input panel holds ("nan": about 5 % NaN), and the variants to run.
class Row(object):
    def __init__(self, name, arrays, variants, status=False, data="noise", **params):
        self.name, self._arrays, self.variants, self.status, self.data, self.params = (
            name, arrays, variants, status, data, params)

    def p(self, v):
        """the call's parameters for variant v (T among them; a rebase row's T is T_in)"""
        p = dict(self.params)
        p.update(v.params)
        p["T"] = v.T
        p["ld"] = v.T + 3
        if "k" in p:
            p["ld_f"] = v.T + 3
        return p

    def arrays(self, v):
        p = self.p(v)
        return self._arrays(p) if callable(self._arrays) else list(self._arrays)

    def plan(self, v):
        return plan(self, v)


Plan = namedtuple("Plan", "T per_series ns S nchunks h2d d2h")


def per_series_bytes(arrays, p, status, inplace):
    b = 0
    for a in arrays:
        if inplace and a.dir == "out" and a.name == "out":
            continue                      # shares the input's device region
        b += a.width(p) * ITEMSIZE[a.dtype]
    return b + (4 if status else 0)


def chunking(S, per_series):
    ns = max(1, min(S, CHUNK // per_series)) if per_series else S
    return ns, -(-S // ns)


def plan(row, v):
    """the shape variant v of `row` runs at and what staged() must decide for it; h2d / d2h are the
    bytes the pipeline moves (a NULL output is not copied; shared uploads are in neither)"""
    p = row.p(v)
    arrays = row.arrays(v)
    per = per_series_bytes(arrays, p, row.status, v.inplace)
    ns = CHUNK // per
    S = (v.chunks - 1) * ns + 37
    ns2, nchunks = chunking(S, per)
    assert ns2 == ns
    h2d = S * sum(a.width(p) * ITEMSIZE[a.dtype] for a in arrays if a.dir == "in")
    d2h = S * sum(a.width(p) * ITEMSIZE[a.dtype] for a in arrays if a.dir == "out" and a.name not in v.null)
    if row.status:
        d2h += 4 * S                      # the caller's err array or the internal one
    return Plan(v.T, per, ns, S, nchunks, h2d, d2h)


def seam_series(pl):
    """the series a case checks against the CPU reference: both sides of every chunk seam and the ends"""
    s = {0, pl.S - 1}
    for c in range(1, pl.nchunks):
        s.update((c * pl.ns - 1, c * pl.ns, c * pl.ns + 1))
    return sorted(x for x in s if 0 <= x < pl.S)


# ---- the table ----

FILLS = ("linear", "nearest", "next", "previous", "spline")
IO = [panel_in(), panel_out()]
FACTOR_VARIANTS = lambda T1, T3: [V("shared", T=T1, k=3, fs="shared"), V("per_series", T=T3, k=3, fs="own")]


def _lagmat(p):
    return (p["T"] - p["max_lag"]) * (p["max_lag"] + (1 if p["inc"] else 0))


def _down(p):
    return (p["T"] - p["phase"] + p["n"] - 1) // p["n"]


def _ar(p):
    return IO + [vec_in("c"), vec_in("coef", lambda q: q["p"]) if p["p"] > 0 else Arr("coef", "in", "f8", lambda q: 1, "zero")]


TABLE = [
    # ---- include/sts.h ----
    Row("sts_fill_host", IO, [V(m, T=390, method=m, chunks=6 if m == "previous" else 3, mixed=(m == "linear"))
                              for m in FILLS], status=True, data="nan"),
    Row("sts_autocorr_host", [panel_in(), vec_out("acf", lambda p: p["K"])], [V("K20", T=391, K=20)],
        status=True),          # its own route (method NONE, filled NULL); the status array is internal
    Row("sts_fill_autocorr_host", [panel_in(), panel_out("filled"), vec_out("acf", lambda p: p["K"])],
        [V("K20-short-pair", T=389, K=20, method="linear"), V("K64-wide", T=391, K=64, method="linear")],
        status=True, data="nan"),
    Row("sts_diff_at_lag_host", IO, [V("out_of_place", T=391, lag=3, start=5), V("in_place", T=393, lag=3, start=5, inplace=True)]),
    Row("sts_lag_matrix_host", [panel_in(), vec_out("out", _lagmat)], [V("p10-inc", T=390, max_lag=10, inc=1)]),
    Row("sts_ewma_add_host", IO + [vec_in("smoothing")], [V("out_of_place", T=391), V("in_place", T=389, inplace=True)]),
    Row("sts_ewma_remove_host", IO + [vec_in("smoothing")], [V("out_of_place", T=391), V("in_place", T=389, inplace=True)]),
    Row("sts_fill_diff_ewma_host", IO + [vec_in("smoothing")], [V("previous", T=386, method="previous", lag=1)],
        status=True, data="nan"),
    Row("sts_ewma_fit_host", [panel_in(), vec_out("smoothing")], [V("fit", T=389, chunks=6)], status=True),
    Row("sts_ar_fit_host", [panel_in(), vec_out("c"), vec_out("coef", lambda p: p["p"])], [V("p3", T=390, p=3, no_intercept=0)],
        status=True, data="ar"),
    Row("sts_ar_fit_remove_host", IO + [vec_out("c"), vec_out("coef", lambda p: p["p"])],
        [V("p3", T=391, p=3, no_intercept=0)], status=True, data="ar"),
    Row("sts_garch_fit_host", [panel_in(), vec_out("params", lambda p: 3)], [V("fit", T=390)], status=True, data="garch"),
    Row("sts_argarch_fit_host", [panel_in(), vec_out("c"), vec_out("phi"), vec_out("params", lambda p: 3)],
        [V("fit", T=389)], status=True, data="garch"),
    Row("sts_ar_remove_host", _ar, [V("p3", T=390, p=3), V("p3-in_place", T=389, p=3, inplace=True), V("p0-null-coef", T=390, p=0)]),
    Row("sts_ar_add_host", _ar, [V("p3", T=390, p=3), V("p3-in_place", T=389, p=3, inplace=True), V("p0-null-coef", T=390, p=0)]),
    Row("sts_dw_test_host", [panel_in(), vec_out("stat")], [V("dw", T=389)]),
    Row("sts_kpss_test_host", [panel_in(), vec_out("stat")], [V("ct", T=389, regression="ct")]),
    Row("sts_adf_test_host", [panel_in(), vec_out("stat"), vec_out("pvalue")],
        [V("lag2-c", T=391, max_lag=2, regression="c"), V("null-pvalue", T=391, max_lag=2, regression="c", null=("pvalue",))],
        status=True),
    Row("sts_lb_test_host", [panel_in(), vec_out("stat"), vec_out("pvalue")],
        [V("lag5", T=390, max_lag=5), V("null-pvalue", T=390, max_lag=5, null=("pvalue",))], data="ar"),
    Row("sts_bp_test_host", lambda p: [panel_in("resid"), vec_out("stat"), vec_out("pvalue")] + fblock(p),
        FACTOR_VARIANTS(391, 389) + [V("null-pvalue", T=391, k=3, fs="shared", null=("pvalue",))], status=True),
    Row("sts_bg_test_host", lambda p: [panel_in("resid"), vec_out("stat"), vec_out("pvalue")] + fblock(p),
        FACTOR_VARIANTS(391, 389) + [V("null-pvalue", T=391, k=3, fs="shared", null=("pvalue",))], status=True,
        max_lag=5, data="ar"),
    # ---- include/sts_regress.h ----
    Row("sts_factor_ols_host",
        lambda p: [panel_in("y"), vec_out("beta", lambda q: q["k"] + 1), vec_out("stderr", lambda q: q["k"] + 1),
                   vec_out("stats", lambda q: 4), panel_out("resid")] + fblock(p),
        [V("shared", T=389, k=3, fs="shared"), V("per_series", T=390, k=3, fs="own", chunks=6),
         V("null-stderr-resid-err", T=389, k=3, fs="shared", null=("stderr", "resid", "err"))], status=True),
    Row("sts_factor_remove_host", lambda p: IO + [vec_in("beta", lambda q: q["k"] + 1)] + fblock(p),
        FACTOR_VARIANTS(390, 390) + [V("in_place", T=389, k=3, fs="shared", inplace=True)]),
    Row("sts_factor_add_host", lambda p: IO + [vec_in("beta", lambda q: q["k"] + 1)] + fblock(p),
        FACTOR_VARIANTS(390, 390) + [V("in_place", T=390, k=3, fs="own", inplace=True)]),
    # ---- include/sts_roll.h ----
    Row("sts_roll_stat_host", IO, [V("mean-w20", T=391, window=20, min_periods=5, op="mean")], data="nan"),
    Row("sts_roll_pair_host", lambda p: IO + ([] if p["Sy"] == "shared" else [Arr("y", "in", "f8", _T, "ypanel")]),
        [V("shared", T=391, Sy="shared", mixed=True), V("per_series", T=391, Sy="own", chunks=6)],
        window=20, min_periods=5, op="cov", data="nan"),
    # ---- include/sts_transforms.h ----
    Row("sts_quotients_host", [panel_in(), vec_out("out", lambda p: p["T"] - p["lag"])], [V("lag2", T=392, lag=2, minus_one=1)],
        data="price"),
    Row("sts_fill_quotients_host", [panel_in(), vec_out("out", lambda p: p["T"] - p["lag"])],
        [V("previous-lag1", T=390, method="previous", lag=1, minus_one=1)], status=True, data="price-nan"),
    Row("sts_fill_with_default_host", IO, [V("out_of_place", T=391, filler=-7.5), V("in_place", T=393, filler=-7.5, inplace=True)],
        data="nan"),
    Row("sts_downsample_host", [panel_in(), vec_out("out", _down)], [V("n3-phase1", T=390, n=3, phase=1)], data="nan"),
    Row("sts_upsample_host", [panel_in(), vec_out("out", lambda p: p["T"] * p["n"])], [V("n3", T=389, n=3, phase=1, use_zero=0)],
        data="nan"),
    Row("sts_first_last_not_nan_host", [panel_in(), vec_out("first", dtype="i8"), vec_out("last", dtype="i8")],
        [V("both", T=390), V("null-last", T=390, null=("last",))], data="edges"),
    Row("sts_inverse_diff_at_lag_host", IO, [V("out_of_place", T=391, lag=3, start=5), V("in_place", T=393, lag=3, start=5, inplace=True)]),
    Row("sts_diff_order_d_host", IO, [V("d2", T=391, d=2, chunks=6, mixed=True)]),
    Row("sts_inverse_diff_order_d_host", IO, [V("d2", T=391, d=2)]),
    # ---- include/sts_index.h (T is T_in) ----
    Row("sts_rebase_shift_host", [panel_in(), vec_out("out", lambda p: p["T_out"])],
        [V("longer", T=390, T_out=401, start_loc=-4, default=47.0), V("shorter-negative-start", T=394, T_out=380, start_loc=-6, default=47.0)],
        data="nan"),
    Row("sts_rebase_map_host", [panel_in(), vec_out("out", lambda p: p["T_out"])], [V("map-absent-repeats", T=391, T_out=397, default=47.0)],
        data="nan"),
]

NAMES = [r.name for r in TABLE]
CASES = [(r, v) for r in TABLE for v in r.variants]


def case_id(r, v):
    return "%s-%s" % (r.name[4:-5], v.id)


# ---- statuses across chunks: every wrapper with a status array that has a failing series to report
# (sts_autocorr_host's is internal and raw autocorr has none), at the shape of one of its variants, with
# the series the operation documents as failing:
#   all_nan_but_first   fill "nearest": an all-NaN row with one leading value ("Input is all NaNs!")
#   nan                 the EWMA / GARCH fits: every objective value is NaN
#   constant            a dyadic constant: an exactly singular AR / ADF design
#   duplicate_factor    per-series factors with factor 1 = factor 0: a rank-deficient design
def _status_case(name, vid, kind, **override):
    row = next(r for r in TABLE if r.name == name)
    v = next(x for x in row.variants if x.id == vid)
    params = dict(v.params)
    chunks = override.pop("chunks", v.chunks)
    params.update(override)
    return row, Variant("status-" + kind, T=v.T, chunks=chunks, inplace=v.inplace, **params), kind


STATUS_CASES_KIND = [
    _status_case("sts_fill_host", "nearest", "all_nan_but_first"),
    _status_case("sts_fill_autocorr_host", "K20-short-pair", "all_nan_but_first", method="nearest"),
    _status_case("sts_fill_diff_ewma_host", "previous", "all_nan_but_first", method="nearest"),
    _status_case("sts_fill_quotients_host", "previous-lag1", "all_nan_but_first", method="nearest"),
    _status_case("sts_ewma_fit_host", "fit", "nan", chunks=3),
    _status_case("sts_garch_fit_host", "fit", "nan"),
    _status_case("sts_ar_fit_host", "p3", "constant"),
    _status_case("sts_ar_fit_remove_host", "p3", "constant"),
    _status_case("sts_argarch_fit_host", "fit", "constant"),
    _status_case("sts_adf_test_host", "lag2-c", "constant"),
    _status_case("sts_bp_test_host", "per_series", "duplicate_factor"),
    _status_case("sts_bg_test_host", "per_series", "duplicate_factor"),
    _status_case("sts_factor_ols_host", "per_series", "duplicate_factor", chunks=3),
]
STATUS_CASES = [(r, v) for r, v, _ in STATUS_CASES_KIND]

# ---- the shared form against the per-series form fed copies, at the shared variant's T and S (every row
# with a "shared" and a "per_series" variant).  "bits": the two forms run the same arithmetic.  "bar": by the
# design of the kernels they do not at these lengths -- shared factors get their orthonormal basis from
# factor_basis_kernel with 256 threads, per-series factors of a series that fits one wave build their own in
# LDS with 64 (series_basis<NT, OWN> of sts_stattests.hip, regimes 0 and 2 of sts_regress.hip; include/
# sts_regress.h: "bit for bit within one kernel regime, within the bar across regimes"), so the sums behind
# the basis are taken in another order and the row is held to the operation's own bar, 1e-10.
SHARED_AGAINST_COPIES = {
    "sts_bp_test_host": "bar",
    "sts_bg_test_host": "bar",
    "sts_factor_ols_host": "bar",
    "sts_factor_remove_host": "bits",
    "sts_factor_add_host": "bits",
    "sts_roll_pair_host": "bits",
}
