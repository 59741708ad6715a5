"""com.cloudera.sparkts.stats: batched statistical tests over series and panels."""
from . import TimeSeriesStatisticalTests
from .TimeSeriesStatisticalTests import adftest, dwtest, kpsstest, lbtest

__all__ = ["TimeSeriesStatisticalTests", "adftest", "dwtest", "kpsstest", "lbtest"]
