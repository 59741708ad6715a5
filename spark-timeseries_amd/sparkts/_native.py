"""Loader and ctypes bindings for libsts_hip.so (the C ABI in include/sts.h, include/sts_transforms.h,
include/sts_sample.h, include/sts_index.h, include/sts_regress.h, include/sts_cross.h and include/sts_roll.h).

This is the Python analogue of the JNI shim: plain pointers and
sizes cross the boundary, no torch types.  There is deliberately NO fallback:
if the HIP library is missing or no gfx950 device is visible, every operator
raises -- the product path never computes on the CPU.
"""
from __future__ import annotations

import ctypes
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.dirname(HERE)
# The product library is the in-tree build; the package reads no environment variable (an
# executor's environment must not be able to swap the library).  Measurement tools select
# another build explicitly with use_library() before the first call.
LIB_PATH = os.path.join(PKG_ROOT, "build", "libsts_hip.so")

_c_i64 = ctypes.c_int64
_c_int = ctypes.c_int
_c_vp = ctypes.c_void_p
_c_dbl = ctypes.c_double

# name -> (restype, argtypes); mirrors include/sts.h exactly (tests/test_abi.py checks
# that every symbol declared there is exported and bound here).
SIGNATURES = {
    "sts_abi_version": (_c_int, []),
    "sts_init": (_c_int, [_c_int]),
    "sts_last_error": (ctypes.c_char_p, []),
    "sts_fill_method_from_name": (_c_int, [ctypes.c_char_p]),
    "sts_stream_synchronize": (_c_int, [_c_vp]),
    "sts_profile_begin": (_c_int, []),
    "sts_profile_end": (_c_int, [_c_vp, _c_vp]),
    "sts_fill": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_vp, _c_vp]),
    "sts_diff_at_lag": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp]),
    "sts_lag_matrix": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp]),
    "sts_autocorr": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_vp, _c_vp]),
    "sts_ewma_add": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp]),
    "sts_ewma_remove": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp]),
    "sts_ar_fit": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_ar_rule_count": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp]),
    "sts_ar_remove": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_int, _c_vp]),
    "sts_ar_add": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_int, _c_vp]),
    "sts_fill_autocorr": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    "sts_fill_diff_ewma": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    "sts_fill_lag_matrix": (_c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int,
                                     _c_vp, _c_vp]),
    "sts_ar_fit_remove": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp,
                                   _c_vp, _c_vp]),
    "sts_ewma_fit": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp]),
    "sts_ewma_sse_gradient": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_garch_fit": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp]),
    "sts_garch_loglik_gradient": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_garch_remove": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_garch_add": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_argarch_remove": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64] + [_c_vp] * 6),
    "sts_argarch_add": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64] + [_c_vp] * 6),
    "sts_argarch_fit": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_series_stats": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp]),
    "sts_nan_instants": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp]),
    "sts_active_instants": (_c_int, [_c_vp, _c_i64, _c_vp, _c_vp, _c_vp]),
    "sts_gather_instants": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64, _c_vp]),
    "sts_to_instants": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_vp]),
    "sts_wire_scan": (_c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_wire_decode": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_i64, _c_vp]),
    "sts_wire_encode": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp]),
    "sts_observations_to_panel": (_c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp, _c_i64, _c_i64, _c_i64, _c_vp]),
    "sts_csv_parse": (_c_int, [_c_vp, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i64]),
    "sts_arima_fit_ar": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_arima_hr_init": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    "sts_arima_fit_css": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp,
                                   _c_vp, _c_vp]),
    "sts_arima_css_loglik_gradient": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_vp,
                                               _c_vp, _c_vp, _c_vp]),
    "sts_arima_remove": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_vp,
                                  _c_vp]),
    "sts_arima_add": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_vp,
                               _c_vp]),
    "sts_arima_forecast": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_vp,
                                    _c_int, _c_vp]),
    "sts_gen_panel": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_i64, ctypes.c_uint64, _c_dbl, _c_vp]),
    "sts_gen_ar_panel": (_c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, ctypes.c_uint64, _c_int, _c_vp]),
    "sts_fill_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_vp]),
    "sts_autocorr_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_vp]),
    "sts_diff_at_lag_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int]),
    "sts_lag_matrix_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int]),
    "sts_ewma_add_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_vp]),
    "sts_ewma_remove_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_vp]),
    "sts_ewma_fit_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp]),
    "sts_garch_fit_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp]),
    "sts_argarch_fit_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_ar_fit_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    "sts_ar_remove_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_int]),
    "sts_ar_add_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_int]),
    "sts_host_alloc": (_c_int, [ctypes.c_size_t, _c_vp]),
    "sts_host_free": (_c_int, [_c_vp]),
    "sts_staging_release": (_c_int, []),
    "sts_staging_stats": (_c_int, [_c_vp]),
    "sts_staging_set_limit": (_c_int, [_c_int]),
    "sts_staging_pool_info": (_c_int, [_c_vp]),
    "sts_fill_autocorr_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp]),
    "sts_fill_diff_ewma_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp]),
    "sts_ar_fit_remove_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    "sts_regression_from_name": (_c_int, [ctypes.c_char_p]),
    "sts_adf_test": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_kpss_test": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_vp, _c_vp]),
    "sts_dw_test": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp]),
    "sts_lb_test": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_vp, _c_vp, _c_vp]),
    "sts_bp_test": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_int, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp, _c_vp]),
    "sts_bg_test": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_int, _c_i64, _c_i64, _c_int, _c_vp, _c_vp, _c_vp,
                             _c_vp]),
    "sts_adf_test_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_vp, _c_vp, _c_vp]),
    "sts_kpss_test_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_vp]),
    "sts_dw_test_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp]),
    "sts_lb_test_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_vp, _c_vp]),
    "sts_bp_test_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_int, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp]),
    "sts_bg_test_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_int, _c_i64, _c_i64, _c_int, _c_vp, _c_vp,
                                  _c_vp]),
}

# The panel transforms of include/sts_transforms.h, a sibling header with the same contracts:
# a table of its own, bound by load_library / load_variant together with SIGNATURES
# (tests/test_transforms_cpu.py holds it to its header as tests/test_abi.py holds SIGNATURES to sts.h).
_PANELS = [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64]     # in, out, S, T, ld_in, ld_out
_PANELS_HOST = [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64]        # in, out, S, T, ld
TRANSFORM_SIGNATURES = {
    "sts_quotients": (_c_int, _PANELS + [_c_int, _c_int, _c_vp]),
    "sts_fill_quotients": (_c_int, _PANELS + [_c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "sts_fill_with_default": (_c_int, _PANELS + [_c_dbl, _c_vp]),
    "sts_downsample": (_c_int, _PANELS + [_c_int, _c_int, _c_vp]),
    "sts_upsample": (_c_int, _PANELS + [_c_int, _c_int, _c_int, _c_vp]),
    "sts_first_last_not_nan": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp, _c_vp]),
    "sts_inverse_diff_at_lag": (_c_int, _PANELS + [_c_int, _c_int, _c_vp]),
    "sts_diff_order_d": (_c_int, _PANELS + [_c_int, _c_vp]),
    "sts_inverse_diff_order_d": (_c_int, _PANELS + [_c_int, _c_vp]),
    "sts_quotients_host": (_c_int, _PANELS_HOST + [_c_int, _c_int]),
    "sts_fill_quotients_host": (_c_int, _PANELS_HOST + [_c_int, _c_int, _c_int, _c_vp]),
    "sts_fill_with_default_host": (_c_int, _PANELS_HOST + [_c_dbl]),
    "sts_downsample_host": (_c_int, _PANELS_HOST + [_c_int, _c_int]),
    "sts_upsample_host": (_c_int, _PANELS_HOST + [_c_int, _c_int, _c_int]),
    "sts_first_last_not_nan_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_vp]),
    "sts_inverse_diff_at_lag_host": (_c_int, _PANELS_HOST + [_c_int, _c_int]),
    "sts_diff_order_d_host": (_c_int, _PANELS_HOST + [_c_int]),
    "sts_inverse_diff_order_d_host": (_c_int, _PANELS_HOST + [_c_int]),
}

# The samplers of include/sts_sample.h, the third sibling header (tests/test_sample_cpu.py holds this
# table to it): out, s0, S, n, ld, then the model, then t0, seed, stream.
_c_u64 = ctypes.c_uint64
_DRAWS = [_c_vp, _c_i64, _c_i64, _c_i64, _c_i64]             # out, s0, S, n, ld
_STREAM_POS = [_c_i64, _c_u64, _c_vp]                        # t0, seed, stream
SAMPLE_SIGNATURES = {
    "sts_sample_normal": (_c_int, _DRAWS + _STREAM_POS),
    "sts_garch_sample": (_c_int, _DRAWS + [_c_vp] * 3 + _STREAM_POS),
    "sts_argarch_sample": (_c_int, _DRAWS + [_c_vp] * 5 + _STREAM_POS),
    "sts_ar_sample": (_c_int, _DRAWS + [_c_vp, _c_vp, _c_int] + _STREAM_POS),
    "sts_arima_sample": (_c_int, _DRAWS + [_c_int, _c_int, _c_int, _c_int, _c_vp] + _STREAM_POS),
}

# Date-time indices and rebasing, include/sts_index.h, the fourth sibling header (tests/test_index_cpu.py
# holds this table to it).  An index travels as kind, start_ms, periods, step, instants, n_instants.
_INDEX = [_c_int, _c_i64, _c_i64, _c_int, _c_vp, _c_i64]
_REBASE = [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64]     # in, out, S, T_in, T_out, ld_in, ld_out
_REBASE_HOST = [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64]        # in, out, S, T_in, T_out, ld
INDEX_SIGNATURES = {
    "sts_index_instants": (_c_int, _INDEX + [_c_vp, _c_vp]),
    "sts_index_locs": (_c_int, [_c_vp, _c_i64] + _INDEX + [_c_vp, _c_vp]),
    "sts_rebase_shift": (_c_int, _REBASE + [_c_i64, _c_dbl, _c_vp]),
    "sts_rebase_map": (_c_int, _REBASE + [_c_vp, _c_dbl, _c_vp]),
    "sts_align_uniform": (_c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_i64, _c_vp, _c_i64, _c_dbl, _c_vp]),
    "sts_rebase_shift_host": (_c_int, _REBASE_HOST + [_c_i64, _c_dbl]),
    "sts_rebase_map_host": (_c_int, _REBASE_HOST + [_c_vp, _c_dbl]),
}
INDEX_DAYS, INDEX_HOURS, INDEX_BUSINESS_DAYS, INDEX_IRREGULAR = 0, 1, 2, 3

# OLS of a panel on factors and the effects pair, include/sts_regress.h, the fifth sibling header
# (tests/test_factor_ols_cpu.py holds this table to it).  A factor panel travels as factors, k, ld_f, fs.
_FACTORS = [_c_vp, _c_int, _c_i64, _c_i64]
REGRESS_SIGNATURES = {
    "sts_factor_ols": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64] + _FACTORS + [_c_vp, _c_i64, _c_vp, _c_vp, _c_vp, _c_i64,
                                                                              _c_vp, _c_vp]),
    "sts_factor_remove": (_c_int, _PANELS + _FACTORS + [_c_vp, _c_i64, _c_vp]),
    "sts_factor_add": (_c_int, _PANELS + _FACTORS + [_c_vp, _c_i64, _c_vp]),
    "sts_factor_ols_host": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64] + _FACTORS + [_c_vp] * 5),
    "sts_factor_remove_host": (_c_int, _PANELS_HOST + _FACTORS + [_c_vp]),
    "sts_factor_add_host": (_c_int, _PANELS_HOST + _FACTORS + [_c_vp]),
}

# Covariance and correlation matrices, include/sts_cross.h, the sixth sibling header
# (tests/test_cross_cpu.py holds this table to it): x, Sx, T, ld_x, then y, Sy, ld_y, then kind.
_TWO_PANELS = [_c_vp, _c_i64, _c_i64, _c_i64, _c_vp, _c_i64, _c_i64, _c_int]
CROSS_SIGNATURES = {
    "sts_cross_kind_from_name": (_c_int, [ctypes.c_char_p]),
    "sts_cross_moments": (_c_int, _TWO_PANELS + [_c_vp, _c_i64, _c_vp, _c_vp, _c_vp]),
    "sts_cross_moments_host": (_c_int, _TWO_PANELS + [_c_vp, _c_vp, _c_vp]),
}
CROSS_COV, CROSS_CORR = 0, 1

# Rolling-window statistics, include/sts_roll.h, the seventh sibling header
# (tests/test_roll_cpu.py holds this table to it).
_ROLL_TAIL = [_c_int, _c_int, _c_int]            # window, min_periods, op
_ROLL_Y = [_c_vp, _c_vp, _c_i64, _c_i64, _c_vp]  # x, y, Sy, ld_y, out
ROLL_SIGNATURES = {
    "sts_roll_op_from_name": (_c_int, [ctypes.c_char_p]),
    "sts_roll_pair_op_from_name": (_c_int, [ctypes.c_char_p]),
    "sts_roll_stat": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64, _c_i64] + _ROLL_TAIL + [_c_vp]),
    "sts_roll_pair": (_c_int, _ROLL_Y + [_c_i64, _c_i64, _c_i64, _c_i64] + _ROLL_TAIL + [_c_vp]),
    "sts_roll_stat_host": (_c_int, [_c_vp, _c_vp, _c_i64, _c_i64, _c_i64] + _ROLL_TAIL),
    "sts_roll_pair_host": (_c_int, _ROLL_Y + [_c_i64, _c_i64, _c_i64] + _ROLL_TAIL),
}
ROLL_OPS = ("sum", "mean", "var", "std", "min", "max", "zscore")
ROLL_PAIR_OPS = ("cov", "corr", "beta")
ROLL_MAX_WINDOW = 1024


def _bind(handle):
    for table in (SIGNATURES, TRANSFORM_SIGNATURES, SAMPLE_SIGNATURES, INDEX_SIGNATURES, REGRESS_SIGNATURES,
                  CROSS_SIGNATURES, ROLL_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
    return handle


_lib = None
_lock = threading.Lock()
_inited = set()


class NativeLibraryError(RuntimeError):
    """libsts_hip.so is missing or unusable: there is no CPU fallback."""


def load_library(path: str = LIB_PATH):
    """Load and bind libsts_hip.so (no device needed, used by the CPU ABI tests)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(path):
                raise NativeLibraryError(
                    "libsts_hip.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                    " (there is no CPU fallback)" % path)
            _lib = _bind(ctypes.CDLL(path))
    return _lib


def lib():
    return load_library()


def use_library(path: str) -> None:
    """Bind the process to ANOTHER build of the library (same C ABI) before its first use:
    bench.py / tools/ pass their STS_HIP_LIB here for same-box A/B runs of tools/variant.sh
    builds.  Not called by the product path."""
    global _lib
    with _lock:
        if _lib is not None:
            raise NativeLibraryError("use_library(%s): a library is already loaded" % path)
    v = load_variant(path)
    with _lock:
        _lib = v


_variants = {}


def load_variant(path: str):
    """Bind ANOTHER build of the library (same C ABI) without touching the product handle:
    build/libsts_hip_ab.so (A/B experiment knobs, -DSTS_AB) for the knob parity tests and
    tools/.  The product library never reads its environment."""
    with _lock:
        if path not in _variants:
            if not os.path.exists(path):
                raise NativeLibraryError("library variant not found at %s" % path)
            _variants[path] = _bind(ctypes.CDLL(path))
    return _variants[path]


AB_LIB_PATH = os.path.join(PKG_ROOT, "build", "libsts_hip_ab.so")


def ensure_device(device: int) -> None:
    """sts_init(device) once per (thread, device): selects the HIP device and checks gfx950."""
    key = (threading.get_ident(), device)
    if key in _inited:
        return
    from .errors import raise_for_status
    raise_for_status(lib().sts_init(device), "sts_init")
    _inited.add(key)
