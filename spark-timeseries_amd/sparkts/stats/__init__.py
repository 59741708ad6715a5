"""com.cloudera.sparkts.stats: batched statistical tests over series and panels."""
from . import TimeSeriesStatisticalTests, cross, factor_tests, regression
from .TimeSeriesStatisticalTests import adftest, dwtest, kpsstest, lbtest
from .cross import corr, cov
from .factor_tests import bgtest, bptest
from .regression import OLSResult, ols

__all__ = ["TimeSeriesStatisticalTests", "cross", "factor_tests", "regression", "adftest", "bgtest", "bptest", "corr", "cov",
           "dwtest", "kpsstest", "lbtest", "ols", "OLSResult"]
