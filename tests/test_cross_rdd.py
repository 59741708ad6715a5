"""TimeSeriesRDD.covariance / .correlation (include/sts_cross.h through sparkts.stats.cross) on a
device-resident partition: rows and columns in `keys` order, the two pipelines the issue names staying
on the device, `other` as an RDD and as a (T, k) factor matrix, and the index check.  The GPU tests
need an MI355X; the index check raises before any native call and runs anywhere."""
import numpy as np
import pytest

import cross_ref as cr

S, T, K = 19, 130, 3


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    from sparkts import _native
    _native.ensure_device(0)
    return _t


def prices(seed, s=S, t=T):
    rng = np.random.default_rng([91, seed])
    return 100.0 * np.exp(np.cumsum(0.01 * rng.standard_normal((s, t)), axis=1))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def rdd(torch):
    from sparkts.timeseriesrdd import TimeSeriesRDD
    x = prices(1)
    return x, TimeSeriesRDD(None, ["k%d" % s for s in range(S)], torch.as_tensor(x, device="cuda:0"))


@pytest.mark.gpu
def test_rows_and_columns_follow_the_keys(torch, rdd):
    from sparkts import stats
    from sparkts.timeseriesrdd import TimeSeriesRDD
    x, r = rdd
    ref = cr.restated(x)
    cov, corr = r.covariance(), r.correlation()
    assert cov.is_cuda and corr.is_cuda and tuple(cov.shape) == tuple(corr.shape) == (S, S)
    assert cr.errors(cov.cpu().numpy(), ref, "cov") <= cr.BAR and cr.errors(corr.cpu().numpy(), ref, "corr") <= cr.BAR
    assert same(cov.cpu().numpy(), stats.cov(r.data).cpu().numpy())
    # the same records in another order: entry (a, b) is still the pair of keys (a, b)
    perm = np.random.default_rng(2).permutation(S)
    p = TimeSeriesRDD(None, [r.keys[i] for i in perm], r.data[torch.as_tensor(perm, device="cuda:0")])
    pc = p.correlation().cpu().numpy()
    c = corr.cpu().numpy()
    for a in (0, 5, S - 1):
        for b in (1, 7):
            assert pc[p.keys.index("k%d" % a), p.keys.index("k%d" % b)] == c[a, b]
    assert same(pc, c[np.ix_(perm, perm)])
    # a numpy partition takes the host path: the same bits
    h = TimeSeriesRDD(None, r.keys, x).covariance()
    assert isinstance(h, np.ndarray) and same(h, cov.cpu().numpy())


@pytest.mark.gpu
def test_return_rates_then_correlation_stays_on_the_device(torch, rdd):
    x, r = rdd
    rr = r.returnRates()
    c = rr.correlation()
    assert c.is_cuda and tuple(c.shape) == (S, S)
    ret = rr.data.cpu().numpy()
    assert cr.errors(c.cpu().numpy(), cr.restated(ret), "corr") <= cr.BAR
    assert cr.errors(rr.covariance().cpu().numpy(), cr.restated(ret), "cov") <= cr.BAR


@pytest.mark.gpu
def test_residual_covariance_of_a_factor_model(torch, rdd):
    x, r = rdd
    rng = np.random.default_rng(3)
    F = rng.standard_normal((T - 1, K))
    Fd = torch.as_tensor(F, device="cuda:0")
    rr = r.returnRates()
    res = rr.regress(Fd).residuals
    cov = res.covariance()
    assert cov.is_cuda and tuple(cov.shape) == (S, S)
    e = res.data.cpu().numpy()
    assert cr.errors(cov.cpu().numpy(), cr.restated(e), "cov") <= cr.BAR
    # residuals against the factors they were fitted on: uncorrelated
    rf = res.correlation(Fd)
    assert rf.is_cuda and tuple(rf.shape) == (S, K)
    assert np.abs(rf.cpu().numpy()).max() <= cr.BAR


@pytest.mark.gpu
def test_other_as_an_rdd_and_as_a_factor_matrix(torch, rdd):
    from sparkts import stats
    from sparkts.timeseriesrdd import TimeSeriesRDD
    x, r = rdd
    y = prices(4, 5)
    other = TimeSeriesRDD(None, ["o%d" % i for i in range(5)], torch.as_tensor(y, device="cuda:0"))
    ref = cr.restated(x, y)
    for kind, fn in (("cov", r.covariance), ("corr", r.correlation)):
        got = fn(other)
        assert got.is_cuda and tuple(got.shape) == (S, 5)
        assert cr.errors(got.cpu().numpy(), ref, kind) <= cr.BAR
        # (T, k): as regress takes it -- C order (copied once into series) and Breeze's column-major data (a view)
        F_c = torch.as_tensor(np.ascontiguousarray(y.T), device="cuda:0")
        F_breeze = other.data.transpose(0, 1)
        assert tuple(F_c.shape) == tuple(F_breeze.shape) == (T, 5)
        assert same(fn(F_c).cpu().numpy(), got.cpu().numpy()) and same(fn(F_breeze).cpu().numpy(), got.cpu().numpy())
    assert same(r.covariance(other).cpu().numpy(), stats.cov(r.data, other.data).cpu().numpy())
    # numpy with numpy
    hc = TimeSeriesRDD(None, r.keys, x).correlation(y.T)
    assert isinstance(hc, np.ndarray) and same(hc, r.correlation(other).cpu().numpy())


def test_a_mismatched_index_raises():
    from sparkts import datetimeindex as dti
    from sparkts.errors import IllegalArgumentException
    from sparkts.timeseriesrdd import TimeSeriesRDD
    a = TimeSeriesRDD(dti.uniform("2015-04-09", periods=8, freq=dti.DayFrequency(1)), ["a", "b"], np.zeros((2, 8)))
    b = TimeSeriesRDD(dti.uniform("2015-04-10", periods=8, freq=dti.DayFrequency(1)), ["c"], np.zeros((1, 8)))
    short = TimeSeriesRDD(dti.uniform("2015-04-09", periods=7, freq=dti.DayFrequency(1)), ["d"], np.zeros((1, 7)))
    for fn in (a.covariance, a.correlation):
        with pytest.raises(IllegalArgumentException, match="different date-time indices"):
            fn(b)
        with pytest.raises(IllegalArgumentException, match="instants"):
            fn(short)
        with pytest.raises(IllegalArgumentException):
            fn(np.zeros((7, 2)))
