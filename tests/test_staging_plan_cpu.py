"""tests/staging_plan.py without a GPU: its table has a row for every chunked `_host` entry point the
bindings know, and every shape tests/test_staging_seams_gpu.py runs really has chunk seams of the kind
that can go wrong -- at least three chunks, a partial last one, an odd series count per chunk (the
two-series workgroups of the short fill+ACF kernel pair up differently after the seam) that is not at a
wave boundary either."""
import pytest

import staging_plan as sp
from sparkts import _native

CASES = sp.CASES
IDS = [sp.case_id(r, v) for r, v in CASES]
ALL = CASES + sp.STATUS_CASES


def host_names():
    names = set()
    for table in (_native.SIGNATURES, _native.TRANSFORM_SIGNATURES, _native.SAMPLE_SIGNATURES, _native.INDEX_SIGNATURES,
                  _native.REGRESS_SIGNATURES, _native.CROSS_SIGNATURES, _native.ROLL_SIGNATURES):
        names.update(n for n in table if n.endswith("_host"))
    return names


def test_every_chunked_host_entry_point_has_a_row():
    declared = host_names()
    assert "sts_host_alloc" not in declared and "sts_host_free" not in declared     # they end in _alloc / _free
    chunked = declared - set(sp.EXCLUDED)
    assert len(chunked) == 37, sorted(chunked)
    assert set(sp.EXCLUDED) == {"sts_host_alloc", "sts_host_free", "sts_cross_moments_host"}
    assert "sts_cross_moments_host" in declared and "no chunks" in sp.EXCLUDED["sts_cross_moments_host"]
    missing = sorted(chunked - set(sp.NAMES))
    assert not missing, "no row in staging_plan.TABLE for %s" % missing
    stale = sorted(set(sp.NAMES) - chunked)
    assert not stale, "rows for names the bindings no longer have: %s" % stale
    assert len(set(sp.NAMES)) == len(sp.NAMES) == 37
    assert len(set(IDS)) == len(IDS)


def test_constants():
    assert sp.CHUNK == 64 * 1024 * 1024 and sp.SLOTS == 5
    assert sp.POOL_KEEP == 5 * (64 * 1024 * 1024 + 16 * 256)


def test_plan_formula_on_the_issue_example():
    # fill at T = 390: in + out rows and the int32 status
    row = next(r for r in sp.TABLE if r.name == "sts_fill_host")
    v = next(v for v in row.variants if v.id == "linear")
    pl = row.plan(v)
    assert (pl.T, pl.per_series, pl.ns, pl.S, pl.nchunks) == (390, 6244, 10747, 21531, 3)
    assert pl.h2d == 21531 * 390 * 8 and pl.d2h == 21531 * (390 * 8 + 4)
    # one series larger than a chunk: ns = 1
    assert sp.chunking(7, 2 * 4500000 * 8 + 4) == (1, 7)
    assert sp.chunking(10, 6244) == (10, 1)


@pytest.mark.parametrize("row,v", ALL, ids=[sp.case_id(r, v) for r, v in ALL])
def test_shape_crosses_seams(row, v):
    pl = row.plan(v)
    assert 385 <= pl.T <= 395
    assert pl.nchunks == v.chunks and pl.nchunks >= 3
    last = pl.S - (pl.nchunks - 1) * pl.ns
    assert 1 <= last < pl.ns, (pl, last)
    assert pl.ns % 2 == 1, "ns = %d is even (per_series %d): pick another T" % (pl.ns, pl.per_series)
    assert pl.ns % 64 not in (0, 63, 1), pl
    assert len(row.arrays(v)) + (1 if row.status else 0) <= sp.MAX_ARGS
    # the host input of a three-chunk case stays near 134 MB, a six-chunk one near 330 MB
    assert pl.h2d <= (v.chunks - 1) * sp.CHUNK + 37 * pl.per_series
    seams = sp.seam_series(pl)
    assert {0, pl.ns - 1, pl.ns, pl.ns + 1, 2 * pl.ns - 1, 2 * pl.ns, pl.S - 1} <= set(seams)
    assert len(seams) <= 3 * pl.nchunks


def test_variants_the_seams_need():
    by = {r.name: r for r in sp.TABLE}
    ids = lambda n: {v.id: v for v in by[n].variants}
    # in place wherever the header allows it
    for n in ("diff_at_lag", "inverse_diff_at_lag", "ewma_add", "ewma_remove", "ar_add", "ar_remove", "factor_add",
              "factor_remove", "fill_with_default"):
        assert any(v.inplace for v in by["sts_%s_host" % n].variants), n
    # optional outputs NULL
    for n, names in (("adf_test", {"pvalue"}), ("lb_test", {"pvalue"}), ("bg_test", {"pvalue"}), ("bp_test", {"pvalue"}),
                     ("first_last_not_nan", {"last"}), ("factor_ols", {"stderr", "resid", "err"})):
        assert any(set(v.null) == names for v in by["sts_%s_host" % n].variants), n
    # shared against per-series factors, k = 3; shared against per-series y
    for n in ("bg_test", "bp_test", "factor_ols", "factor_add", "factor_remove"):
        fs = {v.params["fs"] for v in by["sts_%s_host" % n].variants}
        assert fs == {"shared", "own"} and all(v.params["k"] == 3 for v in by["sts_%s_host" % n].variants), n
    assert {v.params["Sy"] for v in by["sts_roll_pair_host"].variants} == {"shared", "own"}
    # p = 0 with coef = NULL: the stride-0 zero row is a per-series array of the plan
    for n in ("sts_ar_add_host", "sts_ar_remove_host"):
        v = ids(n)["p0-null-coef"]
        assert [a.kind for a in by[n].arrays(v)][-1] == "zero" and by[n].plan(v).per_series == 2 * v.T * 8 + 16
    assert {v.params["method"] for v in by["sts_fill_host"].variants} == set(sp.FILLS)
    assert {v.params["K"] for v in by["sts_fill_autocorr_host"].variants} == {20, 64}
    # widths other than T
    assert by["sts_lag_matrix_host"].variants[0].params == {"max_lag": 10, "inc": 1}
    assert by["sts_downsample_host"].variants[0].params == {"n": 3, "phase": 1}
    assert by["sts_upsample_host"].variants[0].params["n"] == 3
    sh = by["sts_rebase_shift_host"].variants
    assert any(v.params["T_out"] > v.T for v in sh) and any(v.params["T_out"] < v.T and v.params["start_loc"] < 0 for v in sh)
    # in-place shares the device region: counted once
    v = ids("sts_diff_at_lag_host")["in_place"]
    assert by["sts_diff_at_lag_host"].plan(v).per_series == v.T * 8
    # a NULL optional output still counts in the chunk size but is not copied out
    a, b = ids("sts_adf_test_host")["lag2-c"], ids("sts_adf_test_host")["null-pvalue"]
    pa, pb = by["sts_adf_test_host"].plan(a), by["sts_adf_test_host"].plan(b)
    assert pa.per_series == pb.per_series and pa.d2h - pb.d2h == 8 * pa.S
    # shared factors count for nothing, per-series blocks for (k - 1) ld_f + T doubles
    a, b = ids("sts_bg_test_host")["shared"], ids("sts_bg_test_host")["per_series"]
    pa, pb = by["sts_bg_test_host"].plan(a), by["sts_bg_test_host"].plan(b)
    assert pb.per_series - (b.T - a.T) * 8 - pa.per_series == (2 * (b.T + 3) + b.T) * 8
    assert sum(1 for r, v in CASES if v.mixed) == 3


def test_slot_reuse_rows():
    six = [(r, v) for r, v in CASES if v.chunks == 6]
    assert len(six) >= 4 and all(r.plan(v).nchunks == 6 > sp.SLOTS for r, v in six)
    kinds = [[a.kind for a in r.arrays(v)] for r, v in six]
    assert any(r.arrays(v) == sp.IO and not r.status for r, v in six), "a plain panel -> panel row"
    assert any(sum(1 for a in r.arrays(v) if a.kind == "panel") == 1 and
               all(a.dir == "out" for a in r.arrays(v)[1:]) for r, v in six), "a fit: the input panel only"
    assert any("fblock" in k for k in kinds), "per-series factors"
    assert any(r.name == "sts_roll_pair_host" and "ypanel" in k for (r, v), k in zip(six, kinds))


def test_shared_against_copies_rows():
    both = {r.name for r in sp.TABLE if {"shared", "per_series"} <= {v.id for v in r.variants}}
    assert both == set(sp.SHARED_AGAINST_COPIES) and len(both) == 6
    assert set(sp.SHARED_AGAINST_COPIES.values()) == {"bits", "bar"}
    for name in both:
        row = next(r for r in sp.TABLE if r.name == name)
        vs = next(v for v in row.variants if v.id == "shared")
        vo = next(v for v in row.variants if v.id == "per_series")
        # the per-series form at the shared variant's T and S has more, smaller chunks
        S = row.plan(vs).S
        per = sp.per_series_bytes(row.arrays(sp.Variant("copies", T=vs.T, **vo.params)), row.p(sp.Variant("c", T=vs.T, **vo.params)),
                                  row.status, False)
        assert sp.chunking(S, per)[1] >= 3 and row.plan(vs).nchunks >= 3


def test_every_status_wrapper_has_a_status_case():
    with_status = {r.name for r in sp.TABLE if r.status}
    assert len(with_status) == 14
    # raw autocorr has no failing series: its status array is internal and stays zero
    assert {r.name for r, v in sp.STATUS_CASES} == with_status - {"sts_autocorr_host"}
    assert len(set(sp.case_id(r, v) for r, v in ALL)) == len(ALL)
