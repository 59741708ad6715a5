"""TimeSeriesRDD with a DateTimeIndex on the device: date slices, withIndex, the date forms of the
filters, timeSeriesRDD(targetIndex, series), timeSeriesRDDFromObservations with a DateTimeIndex, and
the index through removeInstantsWithNaNs and the CSV round trip.  Expected values come from
tests/index_ref.py (and the oracle's fill).  Needs an MI355X.
"""
import numpy as np
import pytest

import index_ref as ir
import oracle

pytestmark = pytest.mark.gpu

NAN = float("nan")
D = ir.D


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


@pytest.fixture(scope="module")
def m():
    from sparkts import datetimeindex
    return datetimeindex


def rdd_of(torch, index, x, keys=None):
    from sparkts.timeseriesrdd import TimeSeriesRDD
    keys = keys or ["k%d" % i for i in range(x.shape[0])]
    return TimeSeriesRDD(index, keys, torch.as_tensor(np.ascontiguousarray(x), device="cuda:0"))


def ref_index(index):
    """a mirror index as index_ref takes it, through its string"""
    return ir.from_string(str(index))


def host(rdd):
    return rdd.data.cpu().numpy()


def price_panel(S, T, seed):
    x = np.random.default_rng(seed).standard_normal((S, T)).cumsum(axis=1) + 100.0
    x[0, 3] = x[1, 0] = x[2, T - 1] = NAN
    x[3, 2:6] = NAN
    return x


def test_readme_line(torch, m):
    """rdd['2015-04-10':'2015-04-14'].fill('linear')"""
    index = m.uniform("2015-04-06", periods=12, freq=m.DayFrequency(1))
    x = price_panel(5, 12, 1)
    rdd = rdd_of(torch, index, x)
    got = rdd['2015-04-10':'2015-04-14'].fill('linear')
    ref = ref_index(index)
    tgt = ir.u_slice(ref, ir.millis("2015-04-10"), ir.millis("2015-04-14"))
    cut = ir.gather_panel(x, ir.rebase_map(ref, tgt), NAN)
    assert cut.shape == (5, 5) and ref_index(got.index) == tgt
    ir.assert_bits(host(got), oracle.panel_fill(cut, "linear")[0], "slice + fill('linear')")
    assert got.keys == rdd.keys


def test_in_range_uniform_slice_is_a_view(torch, m):
    index = m.uniform("2015-04-06", periods=40, freq=m.BusinessDayFrequency(1))
    rdd = rdd_of(torch, index, price_panel(6, 40, 2))
    inner = rdd.slice("2015-04-13", "2015-04-24")
    assert len(inner.index) == 10 and inner.index == index[5:15]
    assert inner.data.data_ptr() == rdd.data.data_ptr() + 8 * 5 and inner.data.stride(0) == rdd.data.stride(0)
    ir.assert_bits(host(inner), host(rdd)[:, 5:15])
    # a view is a panel like any other: the fill reads it at its own pitch
    ir.assert_bits(host(inner.fill("previous")), oracle.panel_fill(np.ascontiguousarray(host(rdd)[:, 5:15]), "previous")[0])


def earlier(freq, t, k):
    """the latest instant from which k advances reach t (walking back hour by hour, weekends skipped)"""
    for back in range(1, 24 * 40):
        try:
            if ir.advance(freq, t - back * ir.H, k) == t:
                return t - back * ir.H
        except ir.IllegalArgument:
            pass
    raise AssertionError("no instant %d steps before %d" % (k, t))


@pytest.mark.parametrize("freq", ["days", "businessDays", "hours"])
def test_slice_reaching_past_both_ends(torch, m, freq):
    f = {"days": m.DayFrequency(2), "businessDays": m.BusinessDayFrequency(1), "hours": m.HourFrequency(6)}[freq]
    index = m.uniform("2015-04-06", periods=9, freq=f)
    x = ir.hard_panel(4, 9, 3)
    rdd = rdd_of(torch, index, x)
    ref = ref_index(index)
    for lo, hi in ((-3, 12), (-4, 2), (5, 11), (-6, -2), (10, 14)):
        start = ir.advance(ref[2], ref[0], lo) if lo >= 0 else earlier(ref[2], ref[0], -lo)
        end = ir.advance(ref[2], start, hi - lo)
        got = rdd.slice(start, end)
        tgt = ir.u_slice(ref, start, end)
        assert ref_index(got.index) == tgt and tgt[1] == hi - lo + 1
        ir.assert_bits(host(got), ir.gather_panel(x, ir.rebase_map(ref, tgt), NAN), "slice %d..%d" % (lo, hi))


def test_with_index_all_kind_pairs(torch, m):
    x = ir.hard_panel(67, 30, 4)
    uni = m.uniform("2015-04-06", periods=30, freq=m.BusinessDayFrequency(1))
    picks = np.sort(np.random.default_rng(5).choice(45, size=30, replace=False))
    irr = m.irregular(ir.millis("2015-04-01") + picks * D)
    targets = [m.uniform("2015-03-30", periods=50, freq=m.BusinessDayFrequency(1)),          # uniform -> uniform: shift
               m.uniform("2015-04-20", periods=7, freq=m.BusinessDayFrequency(1)),
               m.uniform("2015-04-01", periods=50, freq=m.DayFrequency(1)),                  # irregular -> uniform
               m.irregular(ir.millis("2015-04-01") + np.array([0, 3, 3, 7, 8, 20, 44, 60]) * D),   # duplicates in the target
               m.irregular([])]
    for src in (uni, irr):
        rdd = rdd_of(torch, src, x)
        for tgt in targets:
            if isinstance(src, m.UniformDateTimeIndex) and isinstance(tgt, m.UniformDateTimeIndex) \
                    and src.frequency != tgt.frequency:
                with pytest.raises(ValueError, match="frequencies"):
                    rdd.withIndex(tgt)
                continue
            for default in (NAN, 47.0):
                got = rdd.withIndex(tgt, default)
                assert got.index is tgt and got.keys == rdd.keys
                ir.assert_bits(host(got), ir.gather_panel(x, ir.rebase_map(ref_index(src), ref_index(tgt)), default),
                               "%s -> %s" % (str(src)[:40], str(tgt)[:40]))
    # a host panel takes the _host twins
    from sparkts.timeseriesrdd import TimeSeriesRDD
    for src, tgt in ((uni, targets[0]), (irr, targets[2])):
        got = TimeSeriesRDD(src, None, x).withIndex(tgt, 47.0)
        ir.assert_bits(got.data, ir.gather_panel(x, ir.rebase_map(ref_index(src), ref_index(tgt)), 47.0), "host twin")


def test_date_filters_agree_with_location_filters(torch, m):
    index = m.uniform("2015-04-06", periods=12, freq=m.BusinessDayFrequency(1))
    x = np.arange(60, dtype=np.float64).reshape(5, 12)
    x[1, :4] = NAN
    x[2, :7] = NAN
    x[3, 9:] = NAN
    x[4, 5:] = NAN
    rdd = rdd_of(torch, index, x)
    for loc in (0, 3, 4, 6, 7, 11):
        dt = ir.iso(ir.u_at(ref_index(index), loc))
        for by_date, by_loc in ((rdd.filterStartingBefore(dt), rdd.filterStartingBefore(loc)),
                                (rdd.filterEndingAfter(dt), rdd.filterEndingAfter(loc))):
            assert by_date.keys == by_loc.keys
            ir.assert_bits(host(by_date), host(by_loc))
    assert rdd.filterStartingBefore("2015-04-09").keys == ["k0", "k3", "k4"]
    assert rdd.filterEndingAfter("2015-04-16").keys == ["k0", "k1", "k2", "k3"]


def test_time_series_rdd_from_series(torch, m):
    from sparkts.timeseriesrdd import timeSeriesRDD
    f = m.BusinessDayFrequency(1)
    target = m.uniform("2015-04-06", periods=20, freq=f)
    rng = np.random.default_rng(6)
    series = []
    for i, (start, n) in enumerate([("2015-04-06", 20), ("2015-03-02", 10), ("2015-04-10", 0), ("2015-04-13", 50),
                                    ("2015-03-30", 9), ("2015-05-01", 1), ("2015-06-01", 5), ("2015-04-08", 3)]):
        series.append(("s%d" % i, m.uniform(start, periods=n, freq=f), ir.hard_panel(1, n, 60 + i)[0] if n else np.empty(0)))
    rdd = timeSeriesRDD(target, series, defaultValue=47.0)
    assert rdd.keys == [s[0] for s in series] and rdd.index is target and tuple(rdd.data.shape) == (8, 20)
    got = host(rdd)
    for s, (key, index, values) in enumerate(series):
        ir.assert_bits(got[s], ir.rebase(ref_index(index), ref_index(target), values, 47.0), key)
    with pytest.raises(ValueError, match="frequencies"):
        timeSeriesRDD(target, [("a", m.uniform("2015-04-06", periods=2, freq=m.DayFrequency(1)), [1.0, 2.0])])
    with pytest.raises(ValueError, match="common"):
        timeSeriesRDD(target, [("a", m.uniform("2015-04-06T01:00:00.000Z", periods=2, freq=f), [1.0, 2.0])])


@pytest.mark.parametrize("kind", ["uniform", "irregular"])
def test_observations_with_a_datetime_index(torch, m, kind):
    from sparkts import io
    if kind == "uniform":
        index = m.uniform("2015-04-06", periods=15, freq=m.BusinessDayFrequency(1))
    else:
        index = m.irregular(ir.millis("2015-04-06") + np.array([0, 1, 2, 5, 9, 10, 30]) * D)
    inst = np.asarray(index)
    rng = np.random.default_rng(8)
    n = 400
    keys = ["key%d" % k for k in rng.integers(0, 9, size=n)]
    ts = np.concatenate([rng.choice(inst, size=n - 60), rng.choice(inst, size=30) + 1,
                         ir.millis("2015-04-04") + rng.integers(-3, 40, size=30) * D])
    rng.shuffle(ts)
    vals = rng.standard_normal(n)
    a = io.timeSeriesRDDFromObservations(index, keys, ts, vals, numPartitions=3)
    b = io.timeSeriesRDDFromObservations(inst, keys, ts, vals, numPartitions=3)
    assert a.keys == b.keys and a.partitions == b.partitions and a.index is index
    ir.assert_bits(host(a), host(b), "DateTimeIndex against its millis array")
    assert np.isfinite(host(a)).sum() > 50


def test_remove_instants_with_nans_gives_an_irregular_index(torch, m):
    index = m.uniform("2015-04-06", periods=10, freq=m.BusinessDayFrequency(2))
    x = np.arange(30, dtype=np.float64).reshape(3, 10)
    x[0, 2] = x[2, 7] = x[1, 9] = NAN
    got = rdd_of(torch, index, x).removeInstantsWithNaNs()
    keep = [0, 1, 3, 4, 5, 6, 8]
    assert isinstance(got.index, m.IrregularDateTimeIndex)
    assert got.index.toMillisArray().tolist() == [ir.u_at(ref_index(index), i) for i in keep]
    ir.assert_bits(host(got), x[:, keep])


@pytest.mark.parametrize("kind", ["days", "hours", "businessDays", "irregular"])
def test_csv_round_trips_the_index(torch, m, tmp_path, kind):
    from sparkts import io
    index = {"days": m.uniform("2015-04-06", periods=6, freq=m.DayFrequency(3)),
             "hours": m.uniform("1969-12-31T22:00:00.000Z", periods=6, freq=m.HourFrequency(1)),
             "businessDays": m.uniform("2015-04-10", periods=6, freq=m.BusinessDayFrequency(2)),
             "irregular": m.irregular(["2015-04-06", "2015-04-07", "2015-04-07", "2015-05-01", "2015-05-02", "2016-01-01"])}[kind]
    x = np.random.default_rng(9).standard_normal((3, 6))
    rdd = rdd_of(torch, index, x, ["a", "b", "c"])
    io.saveAsCsv(rdd, str(tmp_path / "out"))
    assert open(str(tmp_path / "out" / "timeIndex")).read().strip() == ir.to_string(ref_index(index))
    back = io.timeSeriesRDDFromCsv(str(tmp_path / "out"), parseIndex=True)
    assert back.index == index and type(back.index) is type(index) and back.keys == rdd.keys
    ir.assert_bits(host(back), x)
    assert io.timeSeriesRDDFromCsv(str(tmp_path / "out")).index == str(index)
