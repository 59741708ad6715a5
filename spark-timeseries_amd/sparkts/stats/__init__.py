"""com.cloudera.sparkts.stats: batched statistical tests over series and panels."""
from . import TimeSeriesStatisticalTests, factor_tests
from .TimeSeriesStatisticalTests import adftest, dwtest, kpsstest, lbtest
from .factor_tests import bgtest, bptest

__all__ = ["TimeSeriesStatisticalTests", "factor_tests", "adftest", "bgtest", "bptest", "dwtest", "kpsstest", "lbtest"]
