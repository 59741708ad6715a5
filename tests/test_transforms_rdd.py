"""The TimeSeriesRDD methods built on include/sts_transforms.h (S/TimeSeriesRDD.scala:80-126) and
the pipelines.fill_returns closure, on a device-resident partition.  Needs an MI355X."""
import numpy as np
import pytest

import transforms_ref as tr
from transforms_ref import assert_bits

pytestmark = pytest.mark.gpu

S, T = 13, 65


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


@pytest.fixture(scope="module")
def rdd(torch):
    from sparkts.timeseriesrdd import TimeSeriesRDD
    x = tr.hard_panel(S, T, 77)
    index = np.datetime64("2015-04-09") + np.arange(T)
    keys = ["k%d" % s for s in range(S)]
    parts = [s % 3 for s in range(S)]
    return x, TimeSeriesRDD(index, keys, torch.as_tensor(x, device="cuda:0"), parts)


def same_records(a, b, index):
    assert a.keys == b.keys and a.partitions == b.partitions
    assert np.array_equal(np.asarray(a.index), index)
    assert a.data.shape[-1] == len(index)


@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_differences_and_quotients(rdd, n):
    x, r = rdd
    d = r.differences(n)
    same_records(d, r, r.index[n:])
    assert_bits(d.data.cpu().numpy(), tr.breeze_diff(x, n), "differences(%d)" % n)
    q = r.quotients(n)
    same_records(q, r, r.index[n:])
    assert_bits(q.data.cpu().numpy(), tr.quotients(x, n), "quotients(%d)" % n)


def test_return_rates(rdd):
    from sparkts import UnivariateTimeSeries as uts
    x, r = rdd
    rr = r.returnRates()
    same_records(rr, r, r.index[1:])
    assert_bits(rr.data.cpu().numpy(), tr.quotients(x, 1, True), "returnRates")
    assert_bits(rr.data.cpu().numpy(), uts.price2ret(r.data, 1).cpu().numpy(), "returnRates == price2ret(., 1)")


@pytest.mark.parametrize("method", ["previous", "linear", "next"])
def test_fill_and_return_rates(rdd, method):
    x, r = rdd
    fused = r.fillAndReturnRates(method)
    two = r.fill(method).returnRates()
    same_records(fused, r, r.index[1:])
    assert_bits(fused.data.cpu().numpy(), two.data.cpu().numpy(), "fillAndReturnRates(%s)" % method)
    if method == "previous":
        assert_bits(fused.data.cpu().numpy(), tr.quotients(tr.fill_previous(x), 1, True), "against the restatement")


def test_fill_and_return_rates_raises_like_fill(rdd):
    from sparkts.errors import IllegalArgumentException
    _, r = rdd
    with pytest.raises(IllegalArgumentException, match="Input is all NaNs!"):
        r.fill("nearest")
    with pytest.raises(IllegalArgumentException, match="Input is all NaNs!"):
        r.fillAndReturnRates("nearest")


def test_find_series_and_filters(rdd):
    x, r = rdd
    assert_bits(r.findSeries("k3").cpu().numpy(), x[3], "findSeries")
    first, last = tr.first_not_nan(x), tr.last_not_nan(x)
    for loc in (0, 5, T // 3, T - 1):
        for got, keep in ((r.filterStartingBefore(loc), first <= loc), (r.filterEndingAfter(loc), last >= loc)):
            idx = np.flatnonzero(keep)
            assert 0 < idx.size < S
            assert got.keys == [r.keys[s] for s in idx] and got.partitions == [r.partitions[s] for s in idx]
            assert np.array_equal(np.asarray(got.index), r.index)
            assert_bits(got.data.cpu().numpy(), x[idx], "filter at %d" % loc)


def test_fill_returns_closure_runs_once_per_panel(rdd, monkeypatch):
    from sparkts import _native, pipelines
    x, r = rdd
    calls = []
    real = _native.lib().sts_fill_quotients

    class Counting:
        def __getattr__(self, name):
            if name == "sts_fill_quotients":
                return lambda *a: calls.append(a[2]) or real(*a)
            return getattr(_native._lib, name)
    proxy = Counting()
    monkeypatch.setattr(_native, "lib", lambda: proxy)
    op = pipelines.fill_returns("previous", 2)
    assert pipelines.is_batched(op)
    out = r.mapSeries(op, r.index[2:])
    assert calls == [S], "one call for the whole panel: %s" % calls
    same_records(out, r, r.index[2:])
    assert_bits(out.data.cpu().numpy(), tr.quotients(tr.fill_previous(x), 2, True), "mapSeries(fill_returns)")
