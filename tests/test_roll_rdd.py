"""The Python mirror of include/sts_roll.h on a device-resident partition: sparkts.rolling.roll, the
seven UnivariateTimeSeries.roll* functions and the TimeSeriesRDD methods keep the index and keys,
give the C ABI's bits after fill("previous").returnRates(), take `other` as an RDD and as a (T,)
factor, take 1-D series and host arrays, and raise the mapped error classes."""
import ctypes

import numpy as np
import pytest

import roll_ref as rr

pytestmark = pytest.mark.gpu

S, T = 11, 130
NAMES = {"sum": "rollSum", "mean": "rollMean", "var": "rollVar", "std": "rollStd", "min": "rollMin", "max": "rollMax",
         "zscore": "rollZScore"}
PAIR_NAMES = {"cov": "rollCov", "corr": "rollCorr", "beta": "rollBeta"}


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


def prices(seed, s=S, t=T):
    rng = np.random.default_rng([93, seed])
    x = 100.0 * np.exp(np.cumsum(0.01 * rng.standard_normal((s, t)), axis=1))
    x[rng.random((s, t)) < 0.05] = np.nan
    x[:, 0] = 100.0
    return x


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def abi(torch, x, op, w, mp, y=None):
    """the C ABI on device tensors -> numpy"""
    from sparkts import _native
    L = _native.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.empty_like(x)
    n, t = x.shape
    if y is None:
        st = L.sts_roll_stat(vp(x), vp(out), n, t, t, t, w, mp, rr.OPS.index(op), None)
    else:
        st = L.sts_roll_pair(vp(x), vp(y), 1 if y.dim() == 1 else n, t, vp(out), n, t, t, t, w, mp, rr.PAIR_OPS.index(op), None)
    assert st == 0, L.sts_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def rdd(torch):
    from sparkts.datetimeindex import uniform, DayFrequency
    from sparkts.timeseriesrdd import TimeSeriesRDD
    x = prices(1)
    index = uniform("2020-01-01T00:00Z", periods=T, freq=DayFrequency(1))
    return x, TimeSeriesRDD(index, ["k%d" % s for s in range(S)], torch.as_tensor(x, device="cuda:0"))


def test_methods_keep_the_index_and_keys_and_give_the_abi_bits(torch, rdd):
    x, r = rdd
    for op, name in NAMES.items():
        got = getattr(r, name)(20, 5)
        assert got.keys == r.keys and got.index is r.index and got.partitions == r.partitions
        assert got.data.is_cuda and tuple(got.data.shape) == (S, T)
        assert same(got.data.cpu().numpy(), abi(torch, r.data, op, 20, 5)), op
        assert same(getattr(r, name)(7).data.cpu().numpy(), abi(torch, r.data, op, 7, 7)), op      # minPeriods = n
    want = rr.stat(x, "mean", 20, 5)
    assert rr.same_bits(r.rollMean(20, 5).data.cpu().numpy(), want)


def test_the_pipeline_of_the_issue_stays_on_the_device(torch, rdd):
    from sparkts.timeseriesrdd import TimeSeriesRDD
    x, r = rdd
    ret = r.fill("previous").returnRates()
    vol = ret.rollStd(20)
    assert vol.data.is_cuda and vol.keys == r.keys and tuple(vol.data.shape) == (S, T - 1)
    assert same(vol.data.cpu().numpy(), abi(torch, ret.data.contiguous(), "std", 20, 20))
    assert rr.ulp_diff(vol.data.cpu().numpy(), rr.stat(ret.data.cpu().numpy(), "std", 20)) <= 4
    factor = ret.data.mean(dim=0)                                 # a market factor, (T - 1,)
    beta = ret.rollBeta(factor, 20)
    assert beta.keys == r.keys and same(beta.data.cpu().numpy(), abi(torch, ret.data.contiguous(), "beta", 20, 20, factor))
    assert rr.same_bits(beta.data.cpu().numpy(), rr.pair(ret.data.cpu().numpy(), factor.cpu().numpy(), "beta", 20))
    other = TimeSeriesRDD(ret.index, ret.keys, torch.as_tensor(prices(2)[:, 1:], device="cuda:0")).fill("previous")
    for op, name in PAIR_NAMES.items():
        got = getattr(ret, name)(other, 20, 10)
        assert got.keys == r.keys and got.data.is_cuda
        assert same(got.data.cpu().numpy(), abi(torch, ret.data.contiguous(), op, 20, 10, other.data.contiguous())), op


def test_series_and_host_arrays(torch, rdd):
    from sparkts import UnivariateTimeSeries as uts
    from sparkts.rolling import roll
    x, r = rdd
    dev_all = r.rollVar(10, 3).data.cpu().numpy()
    one = uts.rollVar(r.data[3], 10, 3)                           # a device series
    assert one.is_cuda and tuple(one.shape) == (T,) and same(one.cpu().numpy(), dev_all[3])
    h = uts.rollVar(x, 10, 3)                                     # a host panel: the _host twin
    assert isinstance(h, np.ndarray) and same(h, dev_all)
    h1 = uts.rollZScore(x[5], 10, 3)                              # a host series
    assert h1.shape == (T,) and same(h1, r.rollZScore(10, 3).data.cpu().numpy()[5])
    f = np.nanmean(x, axis=0)
    hb = roll(x, "corr", 10, 3, other=f)
    db = roll(r.data, "corr", 10, 3, other=torch.as_tensor(f, device="cuda:0"))
    assert same(hb, db.cpu().numpy())
    hp = roll(x[2], "cov", 10, 3, other=x[4])                     # two host series
    assert hp.shape == (T,) and same(hp, roll(r.data[2], "cov", 10, 3, other=r.data[4]).cpu().numpy())
    for op, name in NAMES.items():
        assert same(getattr(uts, name)(x, 4, 2), roll(x, op, 4, 2)), op


def test_errors_raise_the_mapped_classes(torch, rdd):
    from sparkts.errors import IllegalArgumentException
    from sparkts.rolling import roll
    from sparkts.timeseriesrdd import TimeSeriesRDD
    x, r = rdd
    for bad in (lambda: r.rollMean(0), lambda: r.rollMean(1025), lambda: r.rollMean(5, 6), lambda: r.rollMean(5, 0),
                lambda: roll(x, "mean", 0), lambda: roll(r.data, "nope", 3), lambda: roll(r.data, "beta", 3),
                lambda: roll(r.data, "beta", 3, other=x),                                   # host with device
                lambda: r.rollBeta(torch.zeros(T - 1, dtype=torch.float64, device="cuda:0"), 3),
                lambda: r.rollCov(TimeSeriesRDD(None, ["a"], r.data[:1]), 3)):
        with pytest.raises(IllegalArgumentException):
            bad()
    assert r.rollMean(T + 50, 1).data.shape == r.data.shape                               # window > T is legal
