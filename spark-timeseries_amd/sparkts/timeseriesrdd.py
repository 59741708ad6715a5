"""Host mirror of com.cloudera.sparkts.TimeSeriesRDD's hot path (S/TimeSeriesRDD.scala:53-588).

A TimeSeriesRDD here is one PARTITION of keyed series resident in HBM: the (S, T)
panel of this rank's records (series-contiguous, exactly each record's
DenseVector.data), their keys, and the shared time index.  The hot path is position
based and takes any index as metadata; with a DateTimeIndex
(sparkts.datetimeindex) the panel can also be sliced by date, rebased onto another index
(withIndex) and built from series with indices of their own (timeSeriesRDD), on the
device (include/sts_index.h).  Partitioning follows Spark's
`parallelize` slicing (contiguous key ranges per partition, `shard_range`); one
process per GPU owns one partition.  fill / mapSeries are narrow maps: no data
crosses ranks.  The only collective is `all_gather_results`, an all-gather (RCCL
over xGMI on ROCm) of small per-series results such as autocorrelations.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

from . import UnivariateTimeSeries as uts
from . import _native
from ._panel import Panel, check, ptr


def shard_range(n_series: int, rank: int, world: int):
    """[start, end) of partition `rank` under ParallelCollectionRDD slicing:
    start = i*n/world, end = (i+1)*n/world (integer arithmetic)."""
    return (rank * n_series) // world, ((rank + 1) * n_series) // world


class TimeSeriesRDD:
    """A partition's panel: `data` (S, T), its `keys` (record order) and the shared `index`.
    `partitions` (optional, one int per record) is the Spark partition each record lives in --
    timeSeriesRDDFromObservations sets it (the reference's shuffle by key hash); every
    transformation below keeps keys, order and partitions."""

    def __init__(self, index, keys: Optional[Sequence[str]], data, partitions: Optional[Sequence[int]] = None):
        self.index = index
        self.data = data
        self.keys = list(keys) if keys is not None else None
        self.partitions = list(partitions) if partitions is not None else None

    def _derive(self, data, index=None) -> "TimeSeriesRDD":
        """A transformed panel with the same keys, record order and partitions."""
        return TimeSeriesRDD(self.index if index is None else index, self.keys, data, self.partitions)

    # --- S/TimeSeriesRDD.scala:180-182 ---
    def fill(self, method: str) -> "TimeSeriesRDD":
        """fill(method) == mapSeries(UnivariateTimeSeries.fillts(_, method))."""
        return self._derive(uts.fillts(self.data, method))

    def _islice(self, n: int):
        """index.islice(n, index.size); an index that cannot be sliced is dropped"""
        if self.index is None:
            return None
        try:
            return self.index[n:]
        except (TypeError, IndexError, KeyError):
            return None

    def _sliced(self, data, n: int) -> "TimeSeriesRDD":
        return TimeSeriesRDD(self._islice(n), self.keys, data, self.partitions)

    def _select(self, keep) -> "TimeSeriesRDD":
        """filter: the records with keep[s], their keys and partitions, in order"""
        idx = [s for s, k in enumerate(keep) if k]
        data = self.data[idx] if len(idx) != len(keep) else self.data
        keys = [self.keys[s] for s in idx] if self.keys is not None else None
        parts = [self.partitions[s] for s in idx] if self.partitions is not None else None
        return TimeSeriesRDD(self.index, keys, data, parts)

    # --- S/TimeSeriesRDD.scala:80-82 ---
    def findSeries(self, key: str):
        """filter(_._1 == key).first()._2: the first series recorded under `key`."""
        if self.keys is None or key not in self.keys:
            raise KeyError(key)
        return self.data[self.keys.index(key)]

    # --- S/TimeSeriesRDD.scala:88-90 ---
    def differences(self, n: int) -> "TimeSeriesRDD":
        """Breeze's recursive diff(vec, n): the order-n differences without their first n
        instants, index.islice(n, size).  Bit-identical: diff(v, n) subtracts neighbours n times,
        the subtractions differencesOfOrderD makes from position n on."""
        if n < 0 or n > int(self.data.shape[-1]):
            from .errors import IllegalArgumentException
            raise IllegalArgumentException("differences: order %d outside [0, %d]" % (n, int(self.data.shape[-1])))
        return self._sliced(uts.differencesOfOrderD(self.data, n)[..., n:], n)

    # --- S/TimeSeriesRDD.scala:96-98 ---
    def quotients(self, n: int) -> "TimeSeriesRDD":
        return self._sliced(uts.quotients(self.data, n), n)

    # --- S/TimeSeriesRDD.scala:104-106 ---
    def returnRates(self) -> "TimeSeriesRDD":
        """mapSeries(price2ret(_, 1), index.islice(1, size))."""
        return self._sliced(uts.price2ret(self.data, 1), 1)

    def fillAndReturnRates(self, method: str) -> "TimeSeriesRDD":
        """fill(method).returnRates() in one call (sts_fill_quotients; fill("previous") is one
        pass over HBM)."""
        from .pipelines import fill_quotients
        return self._sliced(fill_quotients(self.data, method, 1, True), 1)

    # --- S/TimeSeriesRDD.scala:115-126 ---
    def _loc(self, dt):
        """an int is a location as it is; a date-time goes through index.locAtDateTime"""
        import numbers
        if isinstance(dt, numbers.Integral) and not isinstance(dt, bool):
            return int(dt)
        if not _is_datetime_index(self.index):
            raise TypeError("a date-time argument needs a DateTimeIndex (sparkts.datetimeindex), not %s"
                            % type(self.index).__name__)
        return self.index.locAtDateTime(dt)

    def filterStartingBefore(self, loc) -> "TimeSeriesRDD":
        """Keep the series whose first observation is at or before location `loc`
        (firstNotNaN <= loc); keys and partitions of the survivors are kept.  A date-time `loc` is
        index.locAtDateTime(loc), as in the reference."""
        loc = self._loc(loc)
        first = uts.firstNotNaN(self.data)
        first = [first] if isinstance(first, int) else first.tolist()
        return self._select([f <= loc for f in first])

    def filterEndingAfter(self, loc) -> "TimeSeriesRDD":
        """Keep the series whose last observation is at or after location `loc` (lastNotNaN >= loc);
        a date-time `loc` is index.locAtDateTime(loc)."""
        loc = self._loc(loc)
        last = uts.lastNotNaN(self.data)
        last = [last] if isinstance(last, int) else last.tolist()
        return self._select([l >= loc for l in last])

    # --- S/TimeSeriesRDD.scala:159-172, S/TimeSeriesUtils.scala:65-203 ---
    def withIndex(self, newIndex, defaultValue: float = float("nan")) -> "TimeSeriesRDD":
        """Rebase every series onto `newIndex`: out(s, j) is the value at the first location of
        newIndex's instant j in this index, `defaultValue` where it is absent (include/sts_index.h,
        "Rebase").  Two uniform indices are a shift (sts_rebase_shift); every other pair is a lookup
        made on the device (sts_index_locs) and a gather (sts_rebase_map)."""
        from . import datetimeindex as dti
        if not _is_datetime_index(self.index) or not _is_datetime_index(newIndex):
            raise TypeError("withIndex needs DateTimeIndex objects (sparkts.datetimeindex) on both sides")
        p = Panel(self.data)
        lib = _native.lib()
        n = len(newIndex)
        out = p.empty(T=n)
        dflt = float(defaultValue)
        if isinstance(self.index, dti.UniformDateTimeIndex) and isinstance(newIndex, dti.UniformDateTimeIndex):
            start = dti.uniform_start_loc(self.index, newIndex)
            if p.device:
                check(lib.sts_rebase_shift(ptr(p.t), ptr(out), p.S, p.T, n, p.ld, n, start, dflt, p.stream), "rebase")
            else:
                check(lib.sts_rebase_shift_host(ptr(p.t), ptr(out), p.S, p.T, n, p.ld, start, dflt), "rebase")
        elif p.device:
            m = self.index.locsAtDateTimes(_device_instants(newIndex, p.t.device, p.stream))
            check(lib.sts_rebase_map(ptr(p.t), ptr(out), p.S, p.T, n, p.ld, n, ptr(m), dflt, p.stream), "rebase")
        else:
            import numpy as np
            m = np.ascontiguousarray(self.index.locsAtDateTimes(newIndex.toMillisArray()), dtype=np.int64)
            check(lib.sts_rebase_map_host(ptr(p.t), ptr(out), p.S, p.T, n, p.ld, ptr(m), dflt), "rebase")
        return TimeSeriesRDD(newIndex, self.keys, p.out(out), self.partitions)

    def slice(self, start, end) -> "TimeSeriesRDD":
        """The instants in [start, end], both inclusive (date-times) -- rdd['2015-04-10':'2015-04-14'].
        A slice that lies inside the index is a VIEW of the panel (no kernel, same row pitch), as the
        reference's is (S/TimeSeriesUtils.scala:123-124); a uniform slice that reaches past an end
        is rebased with NaN there (withIndex)."""
        from . import datetimeindex as dti
        if not _is_datetime_index(self.index):
            raise TypeError("slice by date-time needs a DateTimeIndex (sparkts.datetimeindex)")
        if isinstance(self.index, dti.IrregularDateTimeIndex):
            lo, hi = self.index._slice_locs(start, end)
            return TimeSeriesRDD(self.index.islice(lo, hi), self.keys, self.data[..., lo:hi], self.partitions)
        target = self.index.slice(start, end)
        if target.periods < 0:
            target = dti.UniformDateTimeIndex(target.start, 0, target.frequency)
        lo = dti.uniform_start_loc(self.index, target)
        if lo >= 0 and lo + target.periods <= len(self.index):
            return TimeSeriesRDD(target, self.keys, self.data[..., lo:lo + target.periods], self.partitions)
        return self.withIndex(target)

    def __getitem__(self, key):
        """rdd['2015-04-10':'2015-04-14'] is slice(...); rdd['key'] is findSeries('key')."""
        if isinstance(key, slice):
            if key.step is not None or key.start is None or key.stop is None:
                from .errors import IllegalArgumentException
                raise IllegalArgumentException("a date slice needs both bounds and no step")
            return self.slice(key.start, key.stop)
        return self.findSeries(key)

    # --- S/TimeSeriesRDD.scala:188-199 ---
    def mapSeries(self, f: Callable, index=None) -> "TimeSeriesRDD":
        """Apply f to every series; keys (and their order) are unchanged.  A closure marked
        `sparkts.pipelines.batched` (e.g. pipelines.ar_remove(p), the README.md:61 closure)
        runs ONCE on the whole (S, T) partition panel -- one kernel launch; any other
        closure runs per series as in the reference (correct for arbitrary code, one call
        per series)."""
        from .pipelines import apply_per_series, is_batched
        out = f(self.data) if is_batched(f) else apply_per_series(f, self.data)
        return self._derive(out, index)

    def autocorr(self, numLags: int):
        """rdd.mapValues(autocorr(_, numLags)) over the partition: (S, numLags)."""
        return uts.autocorr(self.data, numLags)

    # --- S/stats/TimeSeriesStatisticalTests.scala over the partition panel: (S,) per result ---
    def adftest(self, maxLag: int, regression: str = "c"):
        """rdd.mapValues(adftest(_, maxLag, regression)): (statistics, p-values)."""
        from .stats import TimeSeriesStatisticalTests as tst
        return tst.adftest(self.data, maxLag, regression)

    def kpsstest(self, method: str):
        """rdd.mapValues(kpsstest(_, method)): (statistics, critical values)."""
        from .stats import TimeSeriesStatisticalTests as tst
        return tst.kpsstest(self.data, method)

    def dwtest(self):
        """rdd.mapValues(dwtest(_)): Durbin-Watson statistics."""
        from .stats import TimeSeriesStatisticalTests as tst
        return tst.dwtest(self.data)

    def lbtest(self, maxLag: int):
        """rdd.mapValues(lbtest(_, maxLag)): (statistics, p-values)."""
        from .stats import TimeSeriesStatisticalTests as tst
        return tst.lbtest(self.data, maxLag)

    def bgtest(self, factors, maxLag: int):
        """rdd.mapValues(bgtest(_, factors, maxLag)): (statistics, p-values); factors (T, k) shared or
        (S, T, k) per series."""
        from .stats import factor_tests
        return factor_tests.bgtest(self.data, factors, maxLag)

    def bptest(self, factors):
        """rdd.mapValues(bptest(_, factors)): (statistics, p-values)."""
        from .stats import factor_tests
        return factor_tests.bptest(self.data, factors)

    def regress(self, factors, residuals: bool = True):
        """rdd.mapValues(OLS with intercept on the factors) in one batched call: the OLSResult of
        stats.ols, its residuals a TimeSeriesRDD with this one's keys and index, so
        rdd.regress(F).residuals.bgtest(F, 5) never leaves the device."""
        from .stats import regression
        r = regression.ols(self.data, factors, residuals)
        if r.residuals is not None:
            r.residuals = self._derive(r.residuals)
        return r

    def _cross_other(self, other, name):
        """`other` of covariance / correlation as a panel with this one's instants: another
        TimeSeriesRDD's panel, or the columns of a (T, k) factor matrix as regress takes it (a view:
        a Breeze DenseMatrix(T, k)'s data is a k-series panel with ld = T)."""
        from .errors import IllegalArgumentException
        if other is None:
            return None
        T = int(self.data.shape[-1])
        if isinstance(other, TimeSeriesRDD):
            if int(other.data.shape[-1]) != T:
                raise IllegalArgumentException("%s: the other RDD has %d instants, this one %d"
                                               % (name, int(other.data.shape[-1]), T))
            if _is_datetime_index(self.index) and _is_datetime_index(other.index) and self.index != other.index:
                raise IllegalArgumentException("%s: the two RDDs have different date-time indices" % name)
            return other.data
        shape = tuple(int(v) for v in getattr(other, "shape", ()))
        if len(shape) != 2 or shape[0] != T or shape[1] < 1:
            raise IllegalArgumentException("%s: other must be a TimeSeriesRDD or a (T, k) factor matrix with T=%d, got "
                                           "shape %s" % (name, T, shape))
        return other.transpose(0, 1) if hasattr(other, "stride") else other.T

    def covariance(self, other=None):
        """toRowMatrix().computeCovariance() of the reference's users, on the series-major panel in
        one call: the (S, S) sample covariance matrix of this RDD's series, rows and columns in
        `keys` order; with `other` (a TimeSeriesRDD on the same instants, or a (T, k) factor matrix)
        the (S, S') / (S, k) matrix of this RDD's series against the other's."""
        from .stats import cross
        return cross.cov(self.data, self._cross_other(other, "covariance"))

    def correlation(self, other=None):
        """Statistics.corr on the instants: Pearson correlations, as covariance()."""
        from .stats import cross
        return cross.corr(self.data, self._cross_other(other, "correlation"))

    # --- rolling-window statistics (include/sts_roll.h): the same index and keys ---
    def _roll(self, op, n, minPeriods=None, other=None):
        from .rolling import roll
        return self._derive(roll(self.data, op, n, minPeriods, other))

    def rollSum(self, n: int, minPeriods=None) -> "TimeSeriesRDD":
        """mapSeries(UnivariateTimeSeries.rollSum(_, n)): out[t] over the n steps ending at t."""
        return self._roll("sum", n, minPeriods)

    def rollMean(self, n: int, minPeriods=None) -> "TimeSeriesRDD":
        return self._roll("mean", n, minPeriods)

    def rollVar(self, n: int, minPeriods=None) -> "TimeSeriesRDD":
        return self._roll("var", n, minPeriods)

    def rollStd(self, n: int, minPeriods=None) -> "TimeSeriesRDD":
        return self._roll("std", n, minPeriods)

    def rollMin(self, n: int, minPeriods=None) -> "TimeSeriesRDD":
        return self._roll("min", n, minPeriods)

    def rollMax(self, n: int, minPeriods=None) -> "TimeSeriesRDD":
        return self._roll("max", n, minPeriods)

    def rollZScore(self, n: int, minPeriods=None) -> "TimeSeriesRDD":
        return self._roll("zscore", n, minPeriods)

    def _roll_other(self, other, name):
        """`other` of rollCov / rollCorr / rollBeta: another TimeSeriesRDD with this one's index and
        count, or one (T,) factor that every series shares."""
        from .errors import IllegalArgumentException
        T = int(self.data.shape[-1])
        if isinstance(other, TimeSeriesRDD):
            if tuple(int(v) for v in other.data.shape) != tuple(int(v) for v in self.data.shape):
                raise IllegalArgumentException("%s: the other RDD is %s, this one %s"
                                               % (name, tuple(other.data.shape), tuple(self.data.shape)))
            if _is_datetime_index(self.index) and _is_datetime_index(other.index) and self.index != other.index:
                raise IllegalArgumentException("%s: the two RDDs have different date-time indices" % name)
            return other.data
        shape = tuple(int(v) for v in getattr(other, "shape", ()))
        if shape != (T,):
            raise IllegalArgumentException("%s: other must be a TimeSeriesRDD or a (T,) factor with T=%d, got shape %s"
                                           % (name, T, shape))
        return other

    def rollCov(self, other, n: int, minPeriods=None) -> "TimeSeriesRDD":
        """The rolling sample covariance of every series with the same series of `other`, or with
        the one factor `other`."""
        return self._roll("cov", n, minPeriods, self._roll_other(other, "rollCov"))

    def rollCorr(self, other, n: int, minPeriods=None) -> "TimeSeriesRDD":
        return self._roll("corr", n, minPeriods, self._roll_other(other, "rollCorr"))

    def rollBeta(self, other, n: int, minPeriods=None) -> "TimeSeriesRDD":
        """The rolling slope of every series on `other`: beta against a market factor."""
        return self._roll("beta", n, minPeriods, self._roll_other(other, "rollBeta"))

    def fillAndAutocorr(self, method: str, numLags: int):
        """fill(method) followed by autocorr of every filled series, fused into one pass
        over HBM.  Returns (filled TimeSeriesRDD, acf (S, K))."""
        p = Panel(self.data)
        code = uts.fill_method_code(method)
        lib = _native.lib()
        filled = p.empty()
        acf = p.empty(T=numLags)
        if not p.device:
            raise TypeError("fillAndAutocorr runs on device-resident partitions (torch GPU tensors)")
        check(lib.sts_fill_autocorr(ptr(p.t), ptr(filled), p.S, p.T, p.ld, p.T, code, numLags, ptr(acf), None,
                                    p.stream), "fill_autocorr")
        return self._derive(filled), acf

    # --- S/TimeSeriesRDD.scala:204-206 ---
    def seriesStats(self) -> "StatCounters":
        """map(kt => new StatCounter(kt._2.valuesIterator)) over the partition: one lane-per-
        series Welford pass on the device, in StatCounter.merge's order (bit-exact)."""
        p = Panel(self.data)
        if not p.device:
            raise TypeError("seriesStats runs on device-resident partitions (torch GPU tensors)")
        import torch
        st = torch.empty((p.S, 4), dtype=torch.float64, device=p.t.device)
        check(_native.lib().sts_series_stats(ptr(p.t), p.S, p.T, p.ld, ptr(st), p.stream), "seriesStats")
        return StatCounters(p.T, st)

    # --- S/TimeSeriesRDD.scala:131-152 ---
    def removeInstantsWithNaNs(self, group=None) -> "TimeSeriesRDD":
        """Drop every instant at which ANY series of the whole RDD is NaN.  The reference
        aggregates per-partition Boolean arrays with OR on the driver; here every rank
        flags its own partition on the device and the flags are combined with an
        all-reduce (MAX on uint8 = OR; RCCL over xGMI on the GPU box), then each partition
        is compacted locally.  Returns the new RDD; its index is self.index[active] when the
        index is indexable, else the kept positions."""
        import torch
        p = Panel(self.data)
        if not p.device:
            raise TypeError("removeInstantsWithNaNs runs on device-resident partitions (torch GPU tensors)")
        lib = _native.lib()
        flags = torch.zeros((p.T,), dtype=torch.uint8, device=p.t.device)
        check(lib.sts_nan_instants(ptr(p.t), p.S, p.T, p.ld, ptr(flags), p.stream), "removeInstantsWithNaNs")
        flags = all_reduce_nan_flags(flags, group)
        active = torch.empty((max(p.T, 1),), dtype=torch.int64, device=p.t.device)
        n_dev = torch.zeros((1,), dtype=torch.int64, device=p.t.device)
        check(lib.sts_active_instants(ptr(flags), p.T, ptr(active), ptr(n_dev), p.stream), "active_instants")
        n = int(n_dev.item())
        out = torch.empty((p.S, n), dtype=torch.float64, device=p.t.device)
        check(lib.sts_gather_instants(ptr(p.t), ptr(out), p.S, p.ld, n, ptr(active), n, p.stream), "gather_instants")
        kept = active[:n]
        index = self.index
        if index is not None:
            try:
                index = index[kept.cpu().numpy()]
            except (TypeError, IndexError, KeyError):
                index = kept.cpu().numpy()
        else:
            index = kept.cpu().numpy()
        return self._derive(p.out(out), index)

    # --- S/TimeSeriesRDD.scala:215-324 ---
    def toInstants(self, group=None):
        """One record per instant with every series' value, series in key (partition)
        order, instants in time order.  Locally a transpose kernel; across ranks the
        instants are re-partitioned by time with an all-to-all (RCCL over xGMI), so rank r
        returns instants [t0_r, t1_r) (shard_range over T) of ALL series -- Spark's
        toInstants shuffle.  Returns (index slice, (T_r, S_total) tensor)."""
        index, got, _ = self._instants(group)
        return index, got

    def _instants(self, group=None):
        import torch
        p = Panel(self.data)
        if not p.device:
            raise TypeError("toInstants runs on device-resident partitions (torch GPU tensors)")
        inst = torch.empty((p.T, p.S), dtype=torch.float64, device=p.t.device)
        check(_native.lib().sts_to_instants(ptr(p.t), ptr(inst), p.S, p.T, p.ld, p.S, p.stream), "toInstants")
        got, (t0, t1) = exchange_instants(inst, group)
        index = self.index
        if index is not None:
            try:
                index = index[t0:t1]
            except (TypeError, IndexError, KeyError):
                index = None
        return index, got, t0

    def toRowMatrix(self, group=None):
        """S/TimeSeriesRDD.scala:410-414: the toInstants rows without their instants (a
        RowMatrix's row order carries no meaning).  Returns this rank's (T_r, S_total) rows."""
        return self.toInstants(group)[1]

    def toIndexedRowMatrix(self, group=None):
        """S/TimeSeriesRDD.scala:385-400: toInstants rows indexed by frequency.difference(
        first, instant), i.e. the instant's position in a uniform index.  Non-uniform indices
        raise UnsupportedOperationException("only supported for uniform indices") as the
        reference does.  Returns (row indices int64 (T_r,), (T_r, S_total) rows)."""
        from .errors import UnsupportedOperationException
        if not _is_uniform(self.index):
            raise UnsupportedOperationException("only supported for uniform indices")
        import torch
        _, rows, t0 = self._instants(group)
        return torch.arange(t0, t0 + rows.shape[0], dtype=torch.int64, device=rows.device), rows

    def collectAsTimeSeries(self):
        """(index, keys, (T, S) column-major matrix) like S/TimeSeriesRDD.scala:62-74."""
        d = self.data.cpu().numpy() if hasattr(self.data, "cpu") else self.data
        return self.index, self.keys, d.T

    def count(self) -> int:
        return int(self.data.shape[0])


class StatCounters:
    """Per-series org.apache.spark.util.StatCounter values of a partition: count n (= T),
    mean, m2 from the device pass; the derived statistics follow StatCounter's own formulas."""

    def __init__(self, n: int, stats):
        self.n = n
        self.stats = stats   # (S, 4): mean, m2, max, min

    def count(self):
        return self.n

    def mean(self):
        return self.stats[:, 0]

    def sum(self):
        return self.n * self.stats[:, 0]

    def max(self):
        return self.stats[:, 2]

    def min(self):
        return self.stats[:, 3]

    def variance(self):
        return self.stats[:, 1] / self.n if self.n else self.stats[:, 1] * float("nan")

    def sampleVariance(self):
        return self.stats[:, 1] / (self.n - 1) if self.n > 1 else self.stats[:, 1] * float("nan")

    def stdev(self):
        return self.variance() ** 0.5

    def sampleStdev(self):
        return self.sampleVariance() ** 0.5


def all_reduce_nan_flags(flags, group=None):
    """OR the per-instant NaN flags (uint8) of every partition: all-reduce MAX (RCCL has
    no bitwise OR; MAX on 0/1 bytes is the same).  The reference's
    aggregate(zero)(merge, comb) (S/TimeSeriesRDD.scala:132-144)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(flags, op=dist.ReduceOp.MAX, group=group)
    return flags


def exchange_instants(local, group=None):
    """Re-partition instant-major data by time: `local` is this rank's (T, S_r) block
    (every instant, this partition's series).  Returns ((T_r, S_total) for instants
    [t0, t1) = shard_range(T, rank, world), (t0, t1)); one all-to-all."""
    import torch
    import torch.distributed as dist
    T, S_r = int(local.shape[0]), int(local.shape[1])
    if not (dist.is_available() and dist.is_initialized()):
        return local, (0, T)
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    n = torch.tensor([S_r], device=local.device, dtype=torch.int64)
    sizes = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(sizes, n, group=group)
    s_all = [int(x.item()) for x in sizes]
    bounds = [shard_range(T, q, world) for q in range(world)]
    send = local.contiguous().reshape(-1)            # rows [t0_q, t1_q) are contiguous
    in_split = [(b - a) * S_r for a, b in bounds]
    t0, t1 = bounds[rank]
    out_split = [(t1 - t0) * s for s in s_all]
    recv = local.new_empty((sum(out_split),))
    dist.all_to_all_single(recv, send, out_split, in_split, group=group)
    blocks, off = [], 0
    for s, m in zip(s_all, out_split):
        blocks.append(recv[off: off + m].reshape(t1 - t0, s))
        off += m
    return torch.cat(blocks, dim=1), (t0, t1)


class ResultGather:
    """All-gather of per-series results (S_r, ...) of every partition into one (S, ...)
    tensor in partition order -- the build's only collective (RCCL over xGMI on ROCm).

    The partition sizes are static for a job, so they are exchanged ONCE here (one tiny
    all-gather + host sync at construction); every later call is a single
    all_gather_into_tensor into a buffer allocated once, with no size exchange and no
    host synchronisation.  Equal partitions return that buffer itself (valid until the
    next call; clone it to keep it); ragged ones are compacted with one precomputed
    index_select into a fresh tensor."""

    def __init__(self, n_local: int, row_shape=(), dtype=None, device=None, group=None):
        import torch
        import torch.distributed as dist
        self.group = group
        self.world = dist.get_world_size(group)
        n = torch.tensor([int(n_local)], device=device, dtype=torch.int64)
        sizes = [torch.zeros_like(n) for _ in range(self.world)]
        dist.all_gather(sizes, n, group=group)
        self.sizes = [int(x.item()) for x in sizes]
        self.n_local = int(n_local)
        self.m = max(self.sizes) if self.sizes else 0
        self.row_shape = tuple(row_shape)
        self.pad = torch.zeros((self.m,) + self.row_shape, dtype=dtype, device=device)
        self.buf = torch.empty((self.world * self.m,) + self.row_shape, dtype=dtype, device=device)
        self.uniform = all(s == self.m for s in self.sizes)
        self.keep = None
        if not self.uniform:
            idx = [q * self.m + i for q, s in enumerate(self.sizes) for i in range(s)]
            self.keep = torch.tensor(idx, dtype=torch.int64, device=device)

    def __call__(self, local):
        import torch.distributed as dist
        if int(local.shape[0]) != self.n_local or tuple(local.shape[1:]) != self.row_shape:
            raise ValueError("ResultGather: expected (%d,)+%s rows, got %s" % (self.n_local, self.row_shape,
                                                                              tuple(local.shape)))
        src = local
        if self.n_local != self.m or not local.is_contiguous():
            self.pad[: self.n_local] = local
            src = self.pad
        dist.all_gather_into_tensor(self.buf, src, group=self.group)
        return self.buf if self.uniform else self.buf.index_select(0, self.keep)


def all_gather_results(local, group=None, gather: Optional[ResultGather] = None):
    """All-gather per-series results of every partition (ragged S per rank allowed) into
    one tensor in partition order.  Pass a ResultGather built once per job to keep the
    size exchange out of a loop; without one, a one-shot gather is built for this call."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return local
    if gather is None:
        gather = ResultGather(local.shape[0], local.shape[1:], local.dtype, local.device, group)
    return gather(local)


def _is_datetime_index(index) -> bool:
    from .datetimeindex import DateTimeIndex
    return isinstance(index, DateTimeIndex)


def _device_instants(index, device, stream):
    """index.toMillisArray() as an int64 tensor on `device`: computed there for a uniform index
    (sts_index_instants), the cached upload for an irregular one"""
    import torch
    inst = index._device_instants(device)
    if inst is not None:
        return inst
    out = torch.empty((len(index),), dtype=torch.int64, device=device)
    check(_native.lib().sts_index_instants(*index._c_args(), ptr(out), stream), "toMillisArray")
    return out


def timeSeriesRDD(targetIndex, series, device=None, defaultValue: float = float("nan")) -> TimeSeriesRDD:
    """S/TimeSeriesRDD.scala:446-482 for series that each come with their own uniform index:
    `series` is an iterable of (key, UniformDateTimeIndex, values).  The values are concatenated and
    uploaded once, each series' location in `targetIndex` is computed on the host, and
    sts_align_uniform builds the (S, len(targetIndex)) panel: every series rebased onto targetIndex,
    `defaultValue` elsewhere.  Unequal frequencies or firsts off the target's grid raise
    IllegalArgumentException (datetimeindex.uniform_start_loc)."""
    import ctypes

    import numpy as np
    import torch

    from . import datetimeindex as dti
    if not isinstance(targetIndex, dti.UniformDateTimeIndex):
        raise TypeError("timeSeriesRDD: targetIndex must be a UniformDateTimeIndex")
    keys, rows, start = [], [], []
    for key, index, values in series:
        if not isinstance(index, dti.UniformDateTimeIndex):
            raise TypeError("timeSeriesRDD: series %r needs a UniformDateTimeIndex" % (key,))
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        if v.size != len(index):
            from .errors import IllegalArgumentException
            raise IllegalArgumentException("timeSeriesRDD: series %r has %d values for %d instants" % (key, v.size, len(index)))
        keys.append(key)
        rows.append(v)
        start.append(dti.uniform_start_loc(index, targetIndex))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    _native.ensure_device(dev.index if dev.index is not None else torch.cuda.current_device())
    S, T = len(keys), len(targetIndex)
    offsets = np.zeros(S + 1, dtype=np.int64)
    np.cumsum([r.size for r in rows], out=offsets[1:])
    flat = np.concatenate(rows) if rows else np.empty(0, dtype=np.float64)
    vals_d = torch.as_tensor(flat, device=dev)
    off_d = torch.as_tensor(offsets, device=dev)
    start_d = torch.as_tensor(np.asarray(start, dtype=np.int64), device=dev)
    panel = torch.empty((S, T), dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    check(_native.lib().sts_align_uniform(ptr(vals_d), ptr(off_d), ptr(start_d), S, T, ptr(panel), T,
                                          float(defaultValue), st), "timeSeriesRDD")
    return TimeSeriesRDD(targetIndex, keys, panel)


def _is_uniform(index) -> bool:
    """A UniformDateTimeIndex (any frequency: a business-day index is uniform in locations, not
    in milliseconds) or an analogue: None (positions), a range, or instants with one constant
    spacing (numpy datetime64 / numbers / ISO date strings)."""
    import numpy as np
    if index is None or isinstance(index, range):
        return True
    if _is_datetime_index(index):
        from .datetimeindex import UniformDateTimeIndex
        return isinstance(index, UniformDateTimeIndex)
    try:
        a = np.asarray(index)
        if a.dtype.kind in "US":
            a = a.astype("datetime64[ns]")
        if a.size < 3:
            return True
        d = np.diff(a)
        return bool((d == d[0]).all())
    except (TypeError, ValueError):
        return False
