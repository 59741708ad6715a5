"""The table of tests/test_stream_order_gpu.py covers the header (no GPU): every function that
include/sts.h declares with `void* stream` as its last parameter has a row there, so a new entry
point cannot join the ABI without its stream-ordering test; and the ASYNC / SYNC split of the rows
is what the module says it is."""
import test_stream_order_gpu as so


def test_every_stream_entry_point_has_a_row():
    declared = so.stream_entry_points()
    assert len(declared) >= 45 and "sts_fill" in declared and "sts_bg_test" in declared, declared
    assert not [n for n in declared if n.endswith("_host")], "a _host entry point takes no stream"
    missing = sorted(set(declared) - so.COVERED)
    assert not missing, "no row in test_stream_order_gpu.TABLE for %s" % missing
    stale = sorted(so.COVERED - set(declared))
    assert not stale, "rows for functions sts.h no longer declares with a stream: %s" % stale
    assert len(set(so.IDS)) == len(so.IDS)


def test_async_list_and_reasons_to_block():
    # the entry points that must be held to "returns before the gate opens", each with a row of its own
    for must in ("sts_fill", "sts_fill_diff_ewma", "sts_fill_lag_matrix", "sts_ar_fit_remove", "sts_series_stats"):
        assert must in so.ASYNC, must
    # a row leaves the ASYNC list only with the line of sts_api.cpp that makes it wait
    assert set(so.SYNC) == {"fill_autocorr-T0", "autocorr-T390-K64", "ar_rule_count"}, sorted(so.SYNC)
    for ident, why in so.SYNC.items():
        assert "hipStreamSynchronize" in why or "ErrSink::finish()" in why, (ident, why)
    # every entry point but the three that wait by design (and sts_stream_synchronize) is on the list
    waits = {"sts_autocorr", "sts_ar_rule_count", "sts_stream_synchronize"}
    assert set(so.ASYNC) == set(so.stream_entry_points()) - waits
