"""com.cloudera.sparkts.stats: batched statistical tests over series and panels."""
from . import TimeSeriesStatisticalTests, factor_tests, regression
from .TimeSeriesStatisticalTests import adftest, dwtest, kpsstest, lbtest
from .factor_tests import bgtest, bptest
from .regression import OLSResult, ols

__all__ = ["TimeSeriesStatisticalTests", "factor_tests", "regression", "adftest", "bgtest", "bptest", "dwtest", "kpsstest",
           "lbtest", "ols", "OLSResult"]
