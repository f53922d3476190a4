"""ctypes binding of ``libbisip_hip.so`` (C ABI in ``include/bisip_hip.h``).

This is the only compute backend of the package.  There is no CPU fallback: if the
shared library is missing or no MI355X is visible, calls raise ``RuntimeError``.
"""

import ctypes
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libbisip_hip.so')

MODEL_POLYDECOMP, MODEL_COLECOLE, MODEL_DIAS2000, MODEL_SHIN2015 = 0, 1, 2, 3
VARIANT_AUTO, VARIANT_FAITHFUL, VARIANT_COLLAPSED, VARIANT_REDUCED, VARIANT_WAVE, VARIANT_REDUCED_COMP = 0, 1, 2, 3, 4, 5
VARIANTS = {'auto': VARIANT_AUTO, 'faithful': VARIANT_FAITHFUL, 'collapsed': VARIANT_COLLAPSED,
            'reduced': VARIANT_REDUCED, 'wave': VARIANT_WAVE, 'reduced_comp': VARIANT_REDUCED_COMP}

_dp = ctypes.POINTER(ctypes.c_double)


class ModelDesc(ctypes.Structure):
    """``bisip_model_desc`` of include/bisip_hip.h."""
    _fields_ = [('n_modes', ctypes.c_int), ('poly_deg', ctypes.c_int), ('n_taus', ctypes.c_int),
                ('c_exp', ctypes.c_double), ('taus', _dp), ('log_taus', _dp)]


class StretchArgs(ctypes.Structure):
    """``bisip_stretch_args`` of include/bisip_hip.h (device pointers as integers)."""
    _fields_ = [('coords', ctypes.c_void_p), ('logp', ctypes.c_void_p),
                ('active', ctypes.c_void_p), ('partner', ctypes.c_void_p),
                ('zz', ctypes.c_void_p), ('factor', ctypes.c_void_p), ('logu', ctypes.c_void_p),
                ('n_slots', ctypes.c_int64), ('slot_lo', ctypes.c_int64), ('slot_hi', ctypes.c_int64),
                ('block', ctypes.c_void_p), ('chain_row', ctypes.c_void_p),
                ('logp_row', ctypes.c_void_p), ('naccept', ctypes.c_void_p),
                ('status', ctypes.c_void_p), ('pad', ctypes.c_int64), ('world', ctypes.c_int32),
                ('walkers_per_spectrum', ctypes.c_int64)]


class MoveArgs(ctypes.Structure):
    """``bisip_move_args`` of include/bisip_hip.h."""
    _fields_ = [('stretch', StretchArgs), ('active', ctypes.c_void_p), ('p0', ctypes.c_void_p), ('p1', ctypes.c_void_p),
                ('p2', ctypes.c_void_p), ('gamma', ctypes.c_void_p), ('logu', ctypes.c_void_p),
                ('snooker_gamma', ctypes.c_double)]


class PersistArgs(ctypes.Structure):
    """``bisip_persist_args`` of include/bisip_hip.h."""
    _fields_ = [('coords', ctypes.c_void_p), ('logp', ctypes.c_void_p), ('n_walkers', ctypes.c_int64),
                ('walkers_per_ensemble', ctypes.c_int64), ('n_steps', ctypes.c_int64),
                ('thin_by', ctypes.c_int64), ('active', ctypes.c_void_p), ('partner', ctypes.c_void_p),
                ('zz', ctypes.c_void_p), ('factor', ctypes.c_void_p), ('logu', ctypes.c_void_p),
                ('chain', ctypes.c_void_p), ('logp_chain', ctypes.c_void_p),
                ('naccept', ctypes.c_void_p), ('status', ctypes.c_void_p)]


# name -> (restype, argtypes); every symbol include/bisip_hip.h declares
SYMBOLS = {
    'bisip_ctx_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, _dp, _dp, _dp, ctypes.c_int, _dp, _dp,
                                        ctypes.POINTER(ModelDesc)]),
    'bisip_batch_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, _dp, _dp, _dp, ctypes.c_int, _dp, _dp,
                                          ctypes.POINTER(ModelDesc)]),
    'bisip_ctx_nspectra': (ctypes.c_int, [ctypes.c_void_p]),
    'bisip_ctx_destroy': (None, [ctypes.c_void_p]),
    'bisip_ctx_set_bounds': (ctypes.c_int, [ctypes.c_void_p, _dp, _dp]),
    'bisip_ctx_set_spectrum_offset': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    'bisip_ctx_set_variant': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'bisip_ctx_get_variant': (ctypes.c_int, [ctypes.c_void_p]),
    'bisip_logprob': (ctypes.c_int, [ctypes.c_void_p, _dp, ctypes.c_int64, _dp]),
    'bisip_logprob_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_forward': (ctypes.c_int, [ctypes.c_void_p, _dp, ctypes.c_int64, _dp]),
    'bisip_forward_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_loglike_z': (ctypes.c_int, [ctypes.c_void_p, _dp, ctypes.c_int64, _dp]),
    'bisip_loglike_z_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_stretch_half_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StretchArgs), ctypes.c_void_p]),
    'bisip_stretch_eval_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StretchArgs), ctypes.c_void_p]),
    'bisip_stretch_apply_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StretchArgs), ctypes.c_void_p]),
    'bisip_stretch_run_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StretchArgs), ctypes.c_int64,
                                             ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_stretch_run_sharded_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(StretchArgs),
                                                     ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_stretch_run_sharded_sim_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(StretchArgs),
                                                         ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_rccl_unique_id': (ctypes.c_int, [ctypes.c_void_p]),
    'bisip_rccl_comm_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_int]),
    'bisip_rccl_comm_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'bisip_stretch_draw_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_double,
                                              ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64] +
                               [ctypes.c_void_p] * 7),
    'bisip_stretch_philox_inline': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    'bisip_stretch_run_philox_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(StretchArgs), ctypes.c_int64, ctypes.c_int64,
                                                    ctypes.c_int64, ctypes.c_double, ctypes.c_uint64, ctypes.c_int64,
                                                    ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_stretch_persistent_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(PersistArgs), ctypes.c_void_p]),
    'bisip_move_draw_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_void_p, ctypes.c_double, ctypes.c_double] + [ctypes.c_void_p] * 7),
    'bisip_move_half_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(MoveArgs), ctypes.c_int, ctypes.c_int64,
                                           ctypes.c_void_p]),
    'bisip_move_run_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(MoveArgs), ctypes.POINTER(ctypes.c_int32),
                                          ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_chain_moments_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    'bisip_chain_moments_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 4),
    'bisip_chain_percentiles_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                                           ctypes.c_int]),
    'bisip_chain_percentiles_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                   ctypes.c_int64, ctypes.c_int, _dp, ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_chain_autocorr_time_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    'bisip_chain_autocorr_time_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                     ctypes.c_int64, ctypes.c_int, ctypes.c_double] + [ctypes.c_void_p] * 4),
    'bisip_rtd_integrals_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 4),
    'bisip_rtd_columns_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_rtd_descriptors_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                 ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_rtd_descriptors_host': (ctypes.c_int, [_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                  ctypes.c_int, _dp, ctypes.c_int, _dp, ctypes.c_int, _dp]),
    'bisip_mode_order_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4),
    'bisip_mode_order_host': (ctypes.c_int, [_dp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_int, _dp, _dp, ctypes.POINTER(ctypes.c_ubyte)]),
    'bisip_chain_range_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 3),
    'bisip_chain_histograms_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                  ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_chain_pair_histograms_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                       ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                       ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_chain_trace_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    'bisip_chain_trace_lds_walkers': (ctypes.c_int, [ctypes.c_int]),
    'bisip_chain_trace_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_int, _dp, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_void_p]),
    'bisip_chain_rhat_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    'bisip_chain_rhat_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_chain_cov_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    'bisip_chain_cov_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p]),
    'bisip_chain_best_sample_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    'bisip_chain_best_sample_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                                   ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_int64, ctypes.c_void_p]),
    'bisip_chain_hdi_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                   ctypes.POINTER(ctypes.c_int64)]),
    'bisip_chain_hdi_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_chain_ess_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int]),
    'bisip_chain_ess_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_chain_rank_normalize_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    'bisip_chain_rank_normalize_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                      ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_int64, ctypes.c_void_p]),
    'bisip_chain_rank_normalize_folded_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                             ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                             ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_chain_ess_squares_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                   ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_chain_central_moments_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    'bisip_chain_central_moments_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                       ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 5),
    'bisip_column_percentiles_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    'bisip_column_percentiles_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, _dp, ctypes.c_int,
                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_grouped_percentiles_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    'bisip_grouped_percentiles_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, _dp, ctypes.c_int,
                                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_forward_percentiles': (ctypes.c_int, [ctypes.c_void_p, _dp, ctypes.c_int64, _dp, ctypes.c_int, _dp]),
    'bisip_numpy_stretch_stream': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64,
                                                  ctypes.c_double, ctypes.c_int64] + [ctypes.c_void_p] * 4),
    'bisip_forward_spectrum_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_forward_spectra_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_forward_columns_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_forward_columns_kind_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                                      ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    'bisip_forward_percentiles_kind': (ctypes.c_int, [ctypes.c_void_p, _dp, ctypes.c_int64, _dp, ctypes.c_int, ctypes.c_int, _dp]),
    'bisip_response_moments_workspace': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    'bisip_response_moments_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_fit_quality_workspace': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    'bisip_fit_quality_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                             ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_predictive_check_workspace': (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    'bisip_predictive_check_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
    'bisip_gauss_newton_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64] +
                               [ctypes.c_void_p] * 4),
    'bisip_map_fit_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_int64, ctypes.c_double] + [ctypes.c_void_p] * 8),
    'bisip_lm_step_host': (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, _dp, _dp, ctypes.c_double, _dp, _dp, _dp,
                                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]),
    'bisip_columns_percentiles_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, _dp, ctypes.c_int,
                                                     ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_q_columns_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_void_p]),
    'bisip_loo_columns_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]),
    'bisip_loo_columns_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_void_p]),
    'bisip_bridge_logg_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 5),
    'bisip_bridge_draw_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_bridge_scale_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_int64] + [ctypes.c_void_p] * 5),
    'bisip_bridge_iterate_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_double, ctypes.c_int64] + [ctypes.c_void_p] * 5),
    'bisip_ctx_reduced_check': (ctypes.c_int, [ctypes.c_void_p, _dp, ctypes.c_int64, _dp, _dp]),
    'bisip_read_tables': (ctypes.c_int, [ctypes.POINTER(ctypes.c_char_p), ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    'bisip_philox4x32': (None, [ctypes.POINTER(ctypes.c_uint32)] * 3),
    'bisip_ctx_ndim': (ctypes.c_int, [ctypes.c_void_p]),
    'bisip_ctx_nfreq': (ctypes.c_int, [ctypes.c_void_p]),
    'bisip_ctx_device': (ctypes.c_int, [ctypes.c_void_p]),
    'bisip_ctx_loop_flags': (ctypes.c_int, [ctypes.c_void_p]),
    'bisip_ctx_reduced_tiers': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    'bisip_frequency_grid_step': (ctypes.c_int, [ctypes.c_int, _dp, _dp]),
    'bisip_ctx_loglike_const': (ctypes.c_double, [ctypes.c_void_p]),
    'bisip_ctx_kernel_name': (ctypes.c_char_p, [ctypes.c_void_p]),
    'bisip_ctx_reduced_error': (ctypes.c_double, [ctypes.c_void_p]),
    'bisip_polydecomp_operands': (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, ctypes.POINTER(ModelDesc),
                                                 _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    'bisip_polydecomp_reduced_estimates': (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, ctypes.POINTER(ModelDesc),
                                                          _dp, _dp, _dp]),
    'bisip_ctx_reduced_guard': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                               _dp, ctypes.POINTER(ctypes.c_int)]),
    'bisip_clock_probe_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p]),
    'bisip_fp64_stream_probe_lanes': (ctypes.c_int64, []),
    'bisip_fp64_stream_probe_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    'bisip_ctx_reduced_guard_rows': (ctypes.c_int, [ctypes.c_void_p, _dp, ctypes.c_int64, _dp, _dp, ctypes.POINTER(ctypes.c_int)]),
    'bisip_chain_shell_rows_workspace': (ctypes.c_int64, [ctypes.c_int64]),
    'bisip_ensemble_gram_workspace': (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int]),
    'bisip_ensemble_gram_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    'bisip_chain_shell_rows_dev': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p]),
    'bisip_polydecomp_reduced_reference': (ctypes.c_int, [ctypes.c_int, _dp, _dp, _dp, ctypes.POINTER(ModelDesc),
                                                          _dp, ctypes.c_int64, _dp]),
    'bisip_reduced_emulate': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _dp, ctypes.POINTER(ctypes.c_float), _dp, _dp, _dp,
                                             ctypes.c_double, ctypes.c_double, _dp, _dp, _dp, ctypes.c_int64, _dp]),
    'bisip_ctx_reduced_operands': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, _dp,
                                                  ctypes.POINTER(ctypes.c_float), _dp, _dp, _dp, _dp, _dp,
                                                  ctypes.POINTER(ctypes.c_int)]),
    'bisip_abi_version': (ctypes.c_int, []),
    'bisip_device_count': (ctypes.c_int, []),
    'bisip_last_error': (ctypes.c_char_p, []),
}

_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own ``libamdhip64.so.7``; the system ROCm has one
    with the same soname.  Only one HIP runtime may own the GPU in a process, so when
    torch is installed (it supplies device memory, streams and RCCL around this library)
    its runtime is mapped first and ``libbisip_hip.so`` binds to it by soname."""
    if 'torch' in sys.modules:
        return
    try:
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if os.path.exists(cand):
        ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)


def load_library():
    """Load the HIP library; raise loudly when it has not been built."""
    global _lib
    if _lib is None:
        _share_hip_runtime_with_torch()
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: build it with `make -C bisip_amd/csrc` '
                '(or __graft_entry__.build()).  bisip_amd has no CPU fallback.')
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the ABI and the header drift apart
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _check(rc):
    if rc != 0:
        msg = load_library().bisip_last_error().decode('utf-8', 'replace')
        if rc == -1:
            raise ValueError(f'bisip_hip: {msg}')
        raise RuntimeError(f'bisip_hip (status {rc}): {msg}')


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


RESPONSE_KINDS = {'ri': 0, 'pa': 1}      # BISIP_RESPONSE_RI, BISIP_RESPONSE_PA


def response_kind(kind):
    """BISIP_RESPONSE_* of 'ri' / 'pa'; an integer goes through as it is (the library refuses the ones it does not know)."""
    if isinstance(kind, str):
        try:
            return RESPONSE_KINDS[kind]
        except KeyError:
            raise ValueError(f"kind must be 'ri' or 'pa', got {kind!r}") from None
    return int(kind)


def _p(a):
    return a.ctypes.data_as(_dp)


def polydecomp_operands(w, zn, zn_err, taus, log_taus, c_exp):
    """Host-side precompute of the PolynomialDecomposition operands (no GPU needed)."""
    lib = load_library()
    w, zn, zn_err = _c(w).ravel(), _c(zn).reshape(2, -1), _c(zn_err).reshape(2, -1)
    taus = _c(taus).ravel()
    log_taus = _c(log_taus).reshape(-1, taus.size)
    N, D = w.size, log_taus.shape[0]
    n = D + 1
    desc = ModelDesc(0, D - 1, taus.size, float(c_exp), _p(taus), _p(log_taus))
    out = dict(G_re=np.empty((N, D)), G_im=np.empty((N, D)), R=np.empty((n, n)),
               bhat=np.empty(n), e=np.empty(n), rest=np.empty(1), lconst=np.empty(1))
    _check(lib.bisip_polydecomp_operands(N, _p(w), _p(zn), _p(zn_err), ctypes.byref(desc),
                                         *[_p(out[k]) for k in
                                           ('G_re', 'G_im', 'R', 'bhat', 'e', 'rest', 'lconst')]))
    out['rest'] = float(out['rest'][0])
    out['lconst'] = float(out['lconst'][0])
    return out


def polydecomp_reduced_estimates(w, zn, zn_err, taus, log_taus, c_exp, bounds):
    """Host-side error estimates (plain, compensated) of the QR-reduced kernels for one spectrum
    and prior box -- what BISIP_VARIANT_AUTO decides on.  No GPU needed."""
    lib = load_library()
    w, zn, zn_err = _c(w).ravel(), _c(zn).reshape(2, -1), _c(zn_err).reshape(2, -1)
    taus = _c(taus).ravel()
    log_taus = _c(log_taus).reshape(-1, taus.size)
    b = _c(bounds).reshape(2, -1)
    lo, hi = _c(b[0]), _c(b[1])
    if lo.size != log_taus.shape[0] + 1:
        raise ValueError('bounds must have shape (2, poly_deg + 2)')
    desc = ModelDesc(0, log_taus.shape[0] - 1, taus.size, float(c_exp), _p(taus), _p(log_taus))
    est = np.empty(2)
    _check(lib.bisip_polydecomp_reduced_estimates(w.size, _p(w), _p(zn), _p(zn_err), ctypes.byref(desc), _p(lo), _p(hi), _p(est)))
    return float(est[0]), float(est[1])


def frequency_grid_step(w):
    """Host only: the common step of ln w if ``w`` is a geometric grid in the sense of
    bisip_frequency_grid_step (include/bisip_hip.h), else None."""
    lib = load_library()
    w = _c(w).ravel()
    step = ctypes.c_double(0.0)
    rc = lib.bisip_frequency_grid_step(int(w.size), w.ctypes.data_as(_dp), ctypes.cast(ctypes.byref(step), _dp))
    if rc < 0:
        _check(rc)
    return float(step.value) if rc == 1 else None


def polydecomp_reduced_reference(w, zn, zn_err, taus, log_taus, c_exp, theta):
    """Host-only, no GPU: the PolynomialDecomposition log-likelihood of the rows of ``theta`` with nothing
    rounded to double on the way (bisip_polydecomp_reduced_reference): the yardstick of the reduced
    kernels' estimates, checks and guard."""
    w, zn, zn_err, taus = _c(w), _c(zn), _c(zn_err), _c(taus).ravel()
    log_taus = _c(log_taus).reshape(-1, taus.size)
    theta = _c(theta).reshape(-1, log_taus.shape[0] + 1)
    desc = ModelDesc()
    desc.poly_deg = log_taus.shape[0] - 1
    desc.c_exp = float(c_exp)
    desc.n_taus = taus.size
    desc.taus = _p(taus)
    desc.log_taus = _p(log_taus)
    out = np.empty(theta.shape[0])
    _check(load_library().bisip_polydecomp_reduced_reference(w.size, _p(w), _p(zn), _p(zn_err), ctypes.byref(desc),
                                                            _p(theta), theta.shape[0], _p(out)))
    return out


def reduced_emulate(ops, bounds, theta):
    """Host-only, no GPU: what the QR-reduced kernels store for the rows of ``theta``, bit for bit
    (bisip_reduced_emulate: the host emulation of their arithmetic, then the open-box prior).  ``ops``: the operands
    as a kernel holds them -- ``comp`` (bool), ``R`` the packed upper triangle (row-major), ``Rlo`` (float32, compensated
    only), ``bhat``, ``e``, ``elo`` (compensated only), ``rest``, ``lconst`` -- e.g. what ``HipContext.reduced_operands``
    returns; ``bounds`` (2, n)."""
    comp = bool(ops['comp'])
    bhat = _c(ops['bhat']).ravel()
    n = bhat.size
    R, e = _c(ops['R']).ravel(), _c(ops['e']).ravel()
    Rlo = None if ops.get('Rlo') is None else np.ascontiguousarray(ops['Rlo'], dtype=np.float32).ravel()
    elo = None if ops.get('elo') is None else _c(ops['elo']).ravel()
    tri = n * (n + 1) // 2
    if R.size != tri or e.size != n or (Rlo is not None and Rlo.size != tri) or (elo is not None and elo.size != n):
        raise ValueError(f'operands of n = {n}: R and Rlo hold {tri} entries, bhat, e and elo {n}')
    b = _c(bounds).reshape(2, -1)
    lo, hi = _c(b[0]), _c(b[1])
    if lo.size != n:
        raise ValueError(f'bounds must have shape (2, {n})')
    theta = _c(theta).reshape(-1, n)
    out = np.empty(theta.shape[0])
    _check(load_library().bisip_reduced_emulate(n, int(comp), _p(R), None if Rlo is None else Rlo.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                _p(bhat), _p(e), None if elo is None else _p(elo), float(ops['rest']),
                                                float(ops['lconst']), _p(lo), _p(hi), _p(theta), theta.shape[0], _p(out)))
    return out


def device_count():
    return int(load_library().bisip_device_count())


class HipContext:
    """One inversion problem resident on one GPU (``bisip_ctx``)."""

    def __init__(self, model_id, w, zn, zn_err, bounds, device=0, n_modes=0, poly_deg=0,
                 c_exp=1.0, taus=None, log_taus=None, variant='auto'):
        lib = load_library()
        if lib.bisip_device_count() < 1:
            raise RuntimeError('bisip_amd needs a visible AMD GPU (hipGetDeviceCount() == 0); '
                               'there is no CPU fallback')
        w = _c(w)
        batch = w.ndim == 2          # (E, N): batch of spectra
        E = w.shape[0] if batch else 1
        N = w.shape[-1]
        w = w.reshape(E, N)
        zn = _c(zn).reshape(E, 2, -1)
        zn_err = _c(zn_err).reshape(E, 2, -1)
        b = _c(bounds).reshape(2, -1)
        lo, hi = _c(b[0]), _c(b[1])
        if zn.shape[2] != N or zn_err.shape[2] != N:
            raise ValueError('zn and zn_err must have shape (2, N) [or (E, 2, N)] with N = len(w)')
        desc = ModelDesc()
        desc.n_modes = int(n_modes)
        desc.poly_deg = int(poly_deg)
        desc.c_exp = float(c_exp)
        keep = []
        if taus is not None:
            taus = _c(taus).ravel()
            log_taus = _c(log_taus).reshape(int(poly_deg) + 1, taus.size)
            desc.n_taus = taus.size
            desc.taus = _p(taus)
            desc.log_taus = _p(log_taus)
            keep = [taus, log_taus]
        handle = ctypes.c_void_p()
        if batch:
            _check(lib.bisip_batch_create(ctypes.byref(handle), int(device), int(model_id), E, N,
                                          _p(w), _p(zn), _p(zn_err), lo.size, _p(lo), _p(hi),
                                          ctypes.byref(desc)))
        else:
            _check(lib.bisip_ctx_create(ctypes.byref(handle), int(device), int(model_id), N,
                                        _p(w), _p(zn), _p(zn_err), lo.size, _p(lo), _p(hi),
                                        ctypes.byref(desc)))
        del keep
        self._lib = lib
        self._h = handle
        self.ndim = lo.size
        self.N = N
        self.n_spectra = E
        self.device = int(device)
        self.model_id = int(model_id)
        self.n_modes = int(n_modes)
        self.poly_deg = int(poly_deg)
        # bisip_logprob's guard of the QR-reduced kernels (see logprob)
        self._guarded = self.model_id == MODEL_POLYDECOMP
        self._calls, self._escalations_seen, self._guard_warned, self._forced = 0, 0, False, False
        self._guard_enabled = True
        if variant != 'auto':
            self.set_variant(variant)

    # -- lifetime ---------------------------------------------------------------------
    def close(self):
        if getattr(self, '_h', None):
            self._lib.bisip_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration ----------------------------------------------------------------
    def set_spectrum_offset(self, first_spectrum):
        """This batch context holds spectra [first_spectrum, first_spectrum + E) of a survey: the
        Philox stream of each is keyed by its survey index."""
        _check(self._lib.bisip_ctx_set_spectrum_offset(self._h, int(first_spectrum)))

    def set_bounds(self, bounds):
        b = _c(bounds).reshape(2, -1)
        if b.shape[1] != self.ndim:
            raise ValueError(f'bounds must have shape (2, {self.ndim})')
        lo, hi = _c(b[0]), _c(b[1])
        _check(self._lib.bisip_ctx_set_bounds(self._h, _p(lo), _p(hi)))

    def set_variant(self, variant):
        v = VARIANTS[variant] if isinstance(variant, str) else int(variant)
        _check(self._lib.bisip_ctx_set_variant(self._h, v))
        self._forced = v != VARIANTS['auto']

    @property
    def variant(self):
        v = self._lib.bisip_ctx_get_variant(self._h)
        return {num: name for name, num in VARIANTS.items()}[v]

    @property
    def kernel_name(self):
        return self._lib.bisip_ctx_kernel_name(self._h).decode()

    @property
    def reduced_tiers(self):
        """PolynomialDecomposition: (spectra on the plain, spectra on the compensated QR-reduced kernel); a
        batch on 'auto' decides per spectrum, inside one launch."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self._lib.bisip_ctx_reduced_tiers(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def reduced_operands(self, spectrum=0, tier=0):
        """PolynomialDecomposition: the host copies of what the device holds for ``spectrum`` on QR-reduced tier
        ``tier`` (0 plain, 1 compensated) under the current prior box (bisip_ctx_reduced_operands; launches and
        estimates nothing), as ``reduced_emulate`` takes them, plus ``runs``: does the present variant send this
        spectrum through this tier?  ValueError for a tier that holds no operands of that spectrum."""
        n = self.poly_deg + 2
        tri = n * (n + 1) // 2
        R, Rlo = np.empty(tri), np.zeros(tri, dtype=np.float32)
        bhat, e, elo, rest, lconst = np.empty(n), np.empty(n), np.empty(n), np.empty(1), np.empty(1)
        runs = ctypes.c_int(0)
        _check(self._lib.bisip_ctx_reduced_operands(self._h, int(spectrum), int(tier), _p(R),
                                                    Rlo.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), _p(bhat), _p(e), _p(elo),
                                                    _p(rest), _p(lconst), ctypes.byref(runs)))
        return dict(comp=int(tier) == 1, R=R, Rlo=Rlo if int(tier) == 1 else None, bhat=bhat, e=e, elo=elo,
                    rest=float(rest[0]), lconst=float(lconst[0]), runs=bool(runs.value))

    @property
    def loop_flags(self):
        """ColeCole / Shin: 1 = shared reciprocals (the prior box keeps the products normal), 3 = that and
        exponentials stepped along a geometric frequency grid; 0 = safe loop or another model."""
        return int(self._lib.bisip_ctx_loop_flags(self._h))

    @property
    def persistent_walkers(self):
        """Largest single ensemble for which the persistent sampler kernel (one workgroup holds the
        ensemble) beats one launch per half-step with this context's log-probability kernel --
        measured crossovers, benchmarks/micro/persistent_crossover.py: the cheaper the kernel per
        walker, the longer one CU keeps up with launches that spread over the chip."""
        name = self.kernel_name
        if 'reduced_comp' in name:
            # the compensated tier with its triangle in scalar registers and its low words in LDS wins in the
            # persistent kernel at every degree up to 512 walkers (1.6-2.3x the launch path at 32 walkers,
            # degrees 5-10; profiles/r03_micro_persistent_comp_by_degree.txt), up to 1024 at degree <= 5
            return 1024 if self.poly_deg <= 5 else 512
        if 'reduced' in name:
            return 1024
        if 'Dias' in name:
            return 768
        if 'ColeCole' in name:
            return {1: 768, 2: 512}.get(self.n_modes, 256)
        return 512          # Shin, per-frequency PolynomialDecomposition

    @property
    def group_walkers(self):
        """Largest single ensemble, beyond one workgroup, for which the multi-workgroup persistent kernel
        (k_stretch_group: a barrier among the ensemble's workgroups per half-step instead of a launch) beats one
        launch per half-step -- benchmarks/micro/group_sampler.py: 2.5-5.2 us against 4.3-6.3 per half-step at
        2,048 and 4,096 walkers for the reduced PolynomialDecomposition kernels (one lane per slot: one WAVE per
        workgroup, 1.45-1.75x), Cole-Cole, Dias and Shin (1.15-1.4x);
        at 8,192 the two tie or the launches win (fewer lanes per walker), and the per-frequency
        PolynomialDecomposition form, one lane per walker, loses everywhere.  0: never.  A walker's row must fit 64
        bytes (ndim <= 7)."""
        if self.ndim > 7 or self.n_spectra != 1:
            return 0
        name = self.kernel_name
        if 'PDCollapsed' in name or 'faithful' in name or 'wave' in name:
            return 0
        # the reduced PolynomialDecomposition kernels (one lane per slot, one wave per workgroup) up to 32,768 walkers:
        # up to 256 workgroups on all XCDs, meeting at a two-level barrier
        return 32768 if 'k_logprob_pd_reduced' in name else 4096

    @property
    def persistent_in_big_batches(self):
        """A batch that fills the chip (>= 65,536 walkers in all) runs its launches in the bulk regime; the
        persistent kernel -- one workgroup per ensemble, waiting on dependency chains -- still wins with every
        kernel except the compensated triangle from degree 9, where the two tie (512 x 256, whole fits: 5.9
        against 10.7 us per half-step at degree 5, 11.3 against 15.2 at degree 6, 10.4 against 13.5 at degree
        7, 15.0 against 16.4 at degree 8, 24.2 against 23.8 at degree 9; benchmarks/micro/batch_comp_by_degree.py)."""
        return not ('reduced_comp' in self.kernel_name and self.poly_deg > 8)

    @property
    def reduced_error(self):
        """Estimated worst relative log-prob error of the QR-reduced kernel for the current box."""
        return float(self._lib.bisip_ctx_reduced_error(self._h))

    def reduced_check(self, theta, logp):
        """Worst |logp - reference| / max(1, |reference|) of log-probabilities a QR-reduced kernel
        gave for the rows of ``theta``, against the reduced form in long double from the unrounded
        operands (host; bisip_ctx_reduced_check).  PolynomialDecomposition contexts only."""
        theta = self._theta2d(theta)
        logp = _c(logp).ravel()
        if logp.size != theta.shape[0]:
            raise ValueError('one log-probability per row of theta')
        out = np.empty(1)
        _check(self._lib.bisip_ctx_reduced_check(self._h, _p(theta), theta.shape[0], _p(logp), _p(out)))
        return float(out[0])

    def reduced_guard_rows(self, theta, logp):
        """The guard for rows that came from the DEVICE (bisip_ctx_reduced_guard_rows): measure the
        log-probabilities the context's QR-reduced kernel gave ``theta`` as ``reduced_check`` does and, past
        2e-11 on a context that chose its formulation itself ('auto'), move the context to the next
        formulation.  Returns ``(worst relative error, escalated)``; after an escalation every
        log-probability the caller holds is stale (the device sampler re-runs its chunk).  Rows with a NaN
        (unfilled slots of chain_shell_rows_dev) and rows outside the prior are skipped."""
        theta = self._theta2d(theta)
        logp = _c(logp).ravel()
        if logp.size != theta.shape[0]:
            raise ValueError('one log-probability per row of theta')
        worst, esc = np.empty(1), ctypes.c_int(0)
        _check(self._lib.bisip_ctx_reduced_guard_rows(self._h, _p(theta), theta.shape[0], _p(logp), _p(worst),
                                                      ctypes.byref(esc)))
        return float(worst[0]), bool(esc.value)

    @property
    def guards_itself(self):
        """True for a PolynomialDecomposition context that CHOSE a QR-reduced kernel from its estimate
        ('auto'): the formulation the device sampler measures on its own rows and may move."""
        return (self.model_id == MODEL_POLYDECOMP and not self._forced and self.variant in ('reduced', 'reduced_comp')
                and self._guard_enabled)

    @property
    def loglike_const(self):
        return float(self._lib.bisip_ctx_loglike_const(self._h))

    # -- compute ----------------------------------------------------------------------
    def _theta2d(self, theta):
        theta = np.asarray(theta)
        if theta.ndim != 2 or theta.shape[1] != self.ndim:
            raise ValueError(f'theta must have shape (W, {self.ndim}), got {theta.shape}')
        return _c(theta)

    def logprob(self, theta):
        """theta (W, ndim) host -> logp (W,) host.

        PolynomialDecomposition: the library measures the QR-reduced kernel on rows of this very
        batch on the first call and every 2^n-th after it (bisip_ctx_reduced_guard); a context on
        'auto' that fails moves to the next formulation and re-evaluates the batch -- reported here
        as a RuntimeWarning -- and a caller-forced reduced variant past the tolerance is named."""
        theta = self._theta2d(theta)
        out = np.empty(theta.shape[0], dtype=np.float64)
        _check(self._lib.bisip_logprob(self._h, _p(theta), theta.shape[0], _p(out)))
        if self._guarded and theta.shape[0]:
            self._calls += 1
            if self._calls & (self._calls - 1) == 0:
                self._report_guard()
        return out

    def reduced_guard(self, enable=None):
        """(checks made, worst relative error seen, formulation changes) of the guard bisip_logprob runs
        on the QR-reduced kernels; ``enable`` True / False switches it on / off."""
        n, w, e = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_int(0)
        if enable is not None:
            self._guard_enabled = bool(enable)
        _check(self._lib.bisip_ctx_reduced_guard(self._h, -1 if enable is None else int(bool(enable)),
                                                 ctypes.byref(n), ctypes.cast(ctypes.byref(w), _dp), ctypes.byref(e)))
        return int(n.value), float(w.value), int(e.value)

    def _report_guard(self):
        import warnings
        _, worst, esc = self.reduced_guard()
        if esc > self._escalations_seen:
            self._escalations_seen = esc
            warnings.warn(f'the QR-reduced kernel was {worst:.1e} (relative) away from the exact log-probability on '
                          f'rows of this batch; the context now runs {self.kernel_name} and the batch was '
                          're-evaluated with it', RuntimeWarning, stacklevel=3)
        elif worst > 1e-10 and self._forced and not self._guard_warned and self.variant in ('reduced', 'reduced_comp'):
            self._guard_warned = True
            warnings.warn(f'the {self.variant!r} kernel is {worst:.1e} (relative) away from the exact log-probability '
                          "on rows of this batch (tolerance 1e-10); use variant='auto' or 'reduced_comp'",
                          RuntimeWarning, stacklevel=3)

    def forward(self, theta):
        """theta (W, ndim) host -> Z (W, 2, N) host."""
        theta = self._theta2d(theta)
        out = np.empty((theta.shape[0], 2, self.N), dtype=np.float64)
        _check(self._lib.bisip_forward(self._h, _p(theta), theta.shape[0], _p(out)))
        return out

    def forward_percentiles(self, theta, p):
        """``np.percentile(forward(theta), p, axis=0)`` computed on the device: theta (W, ndim)
        host -> (len(p), 2, N) host (single-spectrum contexts; a batch context raises NotImplementedError)."""
        theta = self._theta2d(theta)
        p = _c(np.atleast_1d(p)).ravel()
        out = np.empty((p.size, 2, self.N), dtype=np.float64)
        rc = self._lib.bisip_forward_percentiles(self._h, _p(theta), theta.shape[0], _p(p), p.size, _p(out))
        if rc == -4:
            raise NotImplementedError(self._lib.bisip_last_error().decode('utf-8', 'replace'))
        _check(rc)
        return out

    def forward_percentiles_kind(self, theta, p, kind='ri'):
        """``forward_percentiles`` in the representation ``kind``: 'ri' the same bits, 'pa' ``np.percentile`` of the
        amplitude and of minus the phase of every sample's response (bisip_amd.response.response_pa)."""
        theta = self._theta2d(theta)
        p = _c(np.atleast_1d(p)).ravel()
        out = np.empty((p.size, 2, self.N), dtype=np.float64)
        rc = self._lib.bisip_forward_percentiles_kind(self._h, _p(theta), theta.shape[0], _p(p), p.size, response_kind(kind),
                                                      _p(out))
        if rc == -4:
            raise NotImplementedError(self._lib.bisip_last_error().decode('utf-8', 'replace'))
        _check(rc)
        return out

    def loglike_z(self, Z):
        """Gaussian log-likelihood of caller-computed responses: Z (W, 2, N) host -> (W,) host."""
        Z = _c(Z)
        if Z.ndim != 3 or Z.shape[1:] != (2, self.N):
            raise ValueError(f'Z must have shape (W, 2, {self.N}), got {Z.shape}')
        out = np.empty(Z.shape[0], dtype=np.float64)
        _check(self._lib.bisip_loglike_z(self._h, _p(Z), Z.shape[0], _p(out)))
        return out

    def logprob_dev(self, d_theta_ptr, W, d_out_ptr, stream=0):
        """Device pointers (ints), asynchronous on ``stream`` (a hipStream_t as int)."""
        _check(self._lib.bisip_logprob_dev(self._h, ctypes.c_void_p(d_theta_ptr), int(W),
                                           ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(stream)))

    def forward_dev(self, d_theta_ptr, W, d_Z_ptr, stream=0):
        _check(self._lib.bisip_forward_dev(self._h, ctypes.c_void_p(d_theta_ptr), int(W),
                                           ctypes.c_void_p(d_Z_ptr), ctypes.c_void_p(stream)))

    def forward_spectrum_dev(self, spectrum, d_theta_ptr, W, d_Z_ptr, stream=0):
        """Batch context: forward of W rows that all belong to one spectrum (device pointers)."""
        _check(self._lib.bisip_forward_spectrum_dev(self._h, int(spectrum), ctypes.c_void_p(d_theta_ptr), int(W),
                                                    ctypes.c_void_p(d_Z_ptr), ctypes.c_void_p(stream)))

    def forward_columns_dev(self, first_spectrum, n_spectra, d_theta_ptr, W, d_cols_ptr, stream=0):
        """Batch (or single) context: the responses of W rows over n_spectra consecutive spectra, written
        column-major (n_spectra, 2N, W / n_spectra) -- what columns_percentiles_dev reads (device pointers)."""
        _check(self._lib.bisip_forward_columns_dev(self._h, int(first_spectrum), int(n_spectra), ctypes.c_void_p(d_theta_ptr),
                                                   int(W), ctypes.c_void_p(d_cols_ptr), ctypes.c_void_p(stream)))

    def forward_columns_kind_dev(self, first_spectrum, n_spectra, d_theta_ptr, W, d_cols_ptr, kind='ri', stream=0):
        """``forward_columns_dev`` in the representation ``kind``: 'pa' writes the amplitude into column j and minus the
        phase into column N + j of every spectrum."""
        _check(self._lib.bisip_forward_columns_kind_dev(self._h, int(first_spectrum), int(n_spectra), ctypes.c_void_p(d_theta_ptr),
                                                        int(W), ctypes.c_void_p(d_cols_ptr), response_kind(kind),
                                                        ctypes.c_void_p(stream)))

    def response_moments_workspace(self, n_samples, n_spectra, walkers_per_ensemble):
        """Bytes of device scratch response_moments_dev needs (0: none; negative: shape not supported)."""
        return int(self._lib.bisip_response_moments_workspace(self._h, int(n_samples), int(n_spectra), int(walkers_per_ensemble)))

    def response_moments_dev(self, first_spectrum, n_spectra, d_chain_ptr, n_samples, sample_stride, walkers_per_ensemble,
                             kind, d_mean_ptr, d_std_ptr, d_work_ptr=0, work_bytes=0, stream=0):
        """Mean and std (ddof = 0) of the model response over the used samples of ``n_spectra`` spectra: d_mean, d_std
        (n_spectra, 2, N), either 0 / None.  ``d_chain_ptr``: walker 0 of ``first_spectrum`` in the first used sample.
        Device pointers (ints), asynchronous on ``stream``."""
        _check(self._lib.bisip_response_moments_dev(self._h, int(first_spectrum), int(n_spectra), d_chain_ptr or None,
                                                    int(n_samples), int(sample_stride), int(walkers_per_ensemble),
                                                    response_kind(kind), d_mean_ptr or None, d_std_ptr or None,
                                                    d_work_ptr or None, int(work_bytes), ctypes.c_void_p(stream)))

    def fit_quality_workspace(self, n_samples, n_spectra, walkers_per_ensemble):
        """Bytes of device scratch fit_quality_dev needs (0: none; negative: shape not supported)."""
        return int(self._lib.bisip_fit_quality_workspace(self._h, int(n_samples), int(n_spectra), int(walkers_per_ensemble)))

    def fit_quality_dev(self, first_spectrum, n_spectra, d_chain_ptr, n_samples, sample_stride, walkers_per_ensemble,
                        d_mean_q_ptr, d_var_q_ptr, d_lmeh_ptr, d_work_ptr=0, work_bytes=0, stream=0):
        """Per data point over the used samples of ``n_spectra`` spectra, with ``q = (y - forward)^2 / sigma^2``: the mean
        of q, its variance (ddof = 1) and ``log(mean(exp(-q / 2)))``: d_mean_q, d_var_q, d_lmeh (n_spectra, 2, N), any
        0 / None but not all.  ``d_chain_ptr``: walker 0 of ``first_spectrum`` in the first used sample.  Device pointers
        (ints), asynchronous on ``stream``."""
        _check(self._lib.bisip_fit_quality_dev(self._h, int(first_spectrum), int(n_spectra), d_chain_ptr or None,
                                               int(n_samples), int(sample_stride), int(walkers_per_ensemble),
                                               d_mean_q_ptr or None, d_var_q_ptr or None, d_lmeh_ptr or None,
                                               d_work_ptr or None, int(work_bytes), ctypes.c_void_p(stream)))

    def predictive_check_workspace(self, n_samples, n_spectra, walkers_per_ensemble):
        """Bytes of device scratch predictive_check_dev needs (always positive; negative: shape not supported)."""
        return int(self._lib.bisip_predictive_check_workspace(self._h, int(n_samples), int(n_spectra), int(walkers_per_ensemble)))

    def predictive_check_dev(self, first_spectrum, n_spectra, d_chain_ptr, n_samples, sample_stride, walkers_per_ensemble,
                             d_pit_ptr, d_row_ptr, d_sign_changes_ptr, d_work_ptr=0, work_bytes=0, stream=0):
        """Posterior predictive checks over the used samples of ``n_spectra`` spectra (bisip_amd.predictive): d_pit
        (n_spectra, 2, N), the mean of ``Phi((y - forward) / sigma)``; d_row (n_spectra, 3), the means of the chi-square
        ``T``, of ``P(chi2_2N >= T)`` and of ``P(max of 2N |eps| >= the largest standardised residual)``; d_sign_changes
        (n_spectra, 2N - 1) int64, the histogram of the residual's sign changes along the frequency axis; any 0 / None but
        not all.  ``d_chain_ptr``: walker 0 of ``first_spectrum`` in the first used sample.  Device pointers (ints),
        asynchronous on ``stream``."""
        _check(self._lib.bisip_predictive_check_dev(self._h, int(first_spectrum), int(n_spectra), d_chain_ptr or None,
                                                    int(n_samples), int(sample_stride), int(walkers_per_ensemble),
                                                    d_pit_ptr or None, d_row_ptr or None, d_sign_changes_ptr or None,
                                                    d_work_ptr or None, int(work_bytes), ctypes.c_void_p(stream)))

    def gauss_newton_dev(self, first_spectrum, n_spectra, d_theta_ptr, S, d_chi2_ptr, d_g_ptr, d_A_ptr, stream=0):
        """The normal equations of the misfit (bisip_amd.mapfit.normal_equations) at ``S`` points for each of ``n_spectra``
        spectra, d_theta (n_spectra, S, ndim): d_chi2 (n_spectra, S), d_g (n_spectra, S, ndim), d_A (n_spectra, S, ndim,
        ndim), any 0 / None.  Device pointers (ints), asynchronous on ``stream``."""
        _check(self._lib.bisip_gauss_newton_dev(self._h, int(first_spectrum), int(n_spectra), d_theta_ptr or None, int(S),
                                                d_chi2_ptr or None, d_g_ptr or None, d_A_ptr or None, ctypes.c_void_p(stream)))

    def map_fit_dev(self, first_spectrum, n_spectra, d_starts_ptr, S, max_iter, pred_tol, d_theta_ptr, d_chi2_ptr, d_logp_ptr,
                    d_pred_ptr, d_A_ptr, d_iterations_ptr, d_status_ptr, stream=0):
        """The Levenberg-Marquardt loop of bisip_amd.mapfit.lm_fit from ``S`` starts for each of ``n_spectra`` spectra,
        d_starts (n_spectra, S, ndim), in one launch: per (spectrum, start) d_theta (ndim), d_chi2, d_logp, d_pred, d_A
        (ndim, ndim), d_iterations and d_status (int64), any 0 / None.  Device pointers (ints), asynchronous on ``stream``."""
        _check(self._lib.bisip_map_fit_dev(self._h, int(first_spectrum), int(n_spectra), d_starts_ptr or None, int(S),
                                           int(max_iter), float(pred_tol), d_theta_ptr or None, d_chi2_ptr or None,
                                           d_logp_ptr or None, d_pred_ptr or None, d_A_ptr or None, d_iterations_ptr or None,
                                           d_status_ptr or None, ctypes.c_void_p(stream)))

    def q_columns_dev(self, first_spectrum, n_spectra, d_cols_ptr, rows_per_spectrum, stream=0):
        """The Re / Im columns ``(n_spectra, 2N, rows_per_spectrum)`` that forward_columns_dev wrote become, in place, the
        squared standardised residuals ``q = (y - Z)^2 * iv`` of their data points (the bits of fitquality.pointwise_q).
        Device pointer (int), asynchronous on ``stream``."""
        _check(self._lib.bisip_q_columns_dev(self._h, int(first_spectrum), int(n_spectra), d_cols_ptr or None,
                                             int(rows_per_spectrum), ctypes.c_void_p(stream)))

    def forward_spectra_dev(self, first_spectrum, n_spectra, d_theta_ptr, W, d_Z_ptr, stream=0):
        """Batch context: forward of W rows over n_spectra consecutive spectra, W / n_spectra rows each
        (a multiple of 64 when n_spectra > 1), one launch (device pointers)."""
        _check(self._lib.bisip_forward_spectra_dev(self._h, int(first_spectrum), int(n_spectra), ctypes.c_void_p(d_theta_ptr),
                                                   int(W), ctypes.c_void_p(d_Z_ptr), ctypes.c_void_p(stream)))

    # -- device-resident stretch move ---------------------------------------------------
    def stretch_half_dev(self, args, stream=0):
        _check(self._lib.bisip_stretch_half_dev(self._h, ctypes.byref(args), ctypes.c_void_p(stream)))

    def stretch_eval_dev(self, args, stream=0):
        _check(self._lib.bisip_stretch_eval_dev(self._h, ctypes.byref(args), ctypes.c_void_p(stream)))

    def stretch_apply_dev(self, args, stream=0):
        _check(self._lib.bisip_stretch_apply_dev(self._h, ctypes.byref(args), ctypes.c_void_p(stream)))

    def stretch_run_dev(self, first_args, W, n_steps, thin_by=1, stream=0):
        _check(self._lib.bisip_stretch_run_dev(self._h, ctypes.byref(first_args), int(W),
                                               int(n_steps), int(thin_by), ctypes.c_void_p(stream)))

    def stretch_run_sharded_dev(self, comm, first_args, W, n_steps, thin_by=1, stream=0):
        """``comm``: an ncclComm_t as an integer (rccl_comm_create() or torch's _comm_ptr())."""
        _check(self._lib.bisip_stretch_run_sharded_dev(self._h, ctypes.c_void_p(comm), ctypes.byref(first_args),
                                                       int(W), int(n_steps), int(thin_by), ctypes.c_void_p(stream)))

    def stretch_run_sharded_sim_dev(self, world, first_args, W, n_steps, thin_by=1, stream=0):
        """The sharded half-step loop with every rank of a ``world``-rank group evaluated on this device in
        turn and no collective (test aid: bisip_stretch_run_sharded_sim_dev)."""
        _check(self._lib.bisip_stretch_run_sharded_sim_dev(self._h, int(world), ctypes.byref(first_args),
                                                           int(W), int(n_steps), int(thin_by), ctypes.c_void_p(stream)))

    def stretch_persistent_dev(self, args, stream=0):
        """Returns False when the ensemble does not fit one workgroup (status -4)."""
        rc = self._lib.bisip_stretch_persistent_dev(self._h, ctypes.byref(args), ctypes.c_void_p(stream))
        if rc == -4:
            return False
        _check(rc)
        return True

    def stretch_philox_inline(self, W):
        """True where :meth:`stretch_run_philox_dev` serves this context's ensemble of ``W`` walkers (a single
        ensemble big enough for the packed-state half-step)."""
        return bool(self._lib.bisip_stretch_philox_inline(self._h, int(W)))

    def stretch_run_philox_dev(self, first_args, W, n_steps, thin_by, a, seed, step0, perm, stream=0):
        """:meth:`stretch_run_dev` with the Philox stream drawn in place by every half-step launch: no stream arrays
        (``first_args``' five stream pointers are ignored); ``perm``: device pointer of this chunk's (n_steps, 3)
        affine splits.  Same chain as :meth:`stretch_draw_dev` + :meth:`stretch_run_dev`."""
        _check(self._lib.bisip_stretch_run_philox_dev(self._h, ctypes.byref(first_args), int(W), int(n_steps), int(thin_by),
                                                      float(a), int(seed), int(step0), ctypes.c_void_p(perm),
                                                      ctypes.c_void_p(stream)))

    def stretch_draw_dev(self, W, a, seed, step0, n_steps, perm, active, partner, zz, factor, logu,
                         stream=0):
        _check(self._lib.bisip_stretch_draw_dev(self._h, int(W), float(a), int(seed), int(step0),
                                                int(n_steps), *[ctypes.c_void_p(p) for p in
                                                                (perm, active, partner, zz, factor, logu)],
                                                ctypes.c_void_p(stream)))

    # -- differential-evolution and snooker moves (bisip_amd/moves.py) --------------------
    def move_draw_dev(self, W, seed, step0, n_steps, perm, g0, sigma, active, p0, p1, p2, gamma, logu, stream=0):
        """The moves' stream arrays (purposes 4, 5 and 1 of the Philox contract) for ``n_steps`` iterations; every
        array argument is a device pointer."""
        _check(self._lib.bisip_move_draw_dev(self._h, int(W), int(seed), int(step0), int(n_steps), ctypes.c_void_p(perm),
                                             float(g0), float(sigma),
                                             *[ctypes.c_void_p(p) for p in (active, p0, p1, p2, gamma, logu)],
                                             ctypes.c_void_p(stream)))

    def move_half_dev(self, args, kind, W, stream=0):
        """One half-step of move ``kind`` (moves.MOVE_*) over a :class:`MoveArgs`; ``W``: walkers per ensemble."""
        _check(self._lib.bisip_move_half_dev(self._h, ctypes.byref(args), int(kind), int(W), ctypes.c_void_p(stream)))

    def move_run_dev(self, first_args, kinds, W, n_steps, thin_by=1, stream=0):
        """``n_steps`` iterations back to back, iteration k running move ``kinds[k]`` (a host array of moves.MOVE_*)."""
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        if kinds.shape != (int(n_steps),):
            raise ValueError(f'kinds has shape {kinds.shape}, expected ({int(n_steps)},)')
        _check(self._lib.bisip_move_run_dev(self._h, ctypes.byref(first_args), kinds.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                            int(W), int(n_steps), int(thin_by), ctypes.c_void_p(stream)))


RCCL_ID_BYTES = 128


def clock_probe_dev(d_out_ptr, window_us, stream=0):
    """One wavefront that brackets ``window_us`` with (shader clock, 100 MHz clock) reads into the
    four int64 at ``d_out_ptr``: enqueue it on a side stream next to a kernel under measurement;
    engine clock in GHz = (out[1] - out[0]) / (out[3] - out[2]) * 0.1."""
    _check(load_library().bisip_clock_probe_dev(ctypes.c_void_p(d_out_ptr), float(window_us), ctypes.c_void_p(stream)))


def fp64_stream_probe_lanes():
    """Doubles the output buffer of :func:`fp64_stream_probe_dev` must hold."""
    return int(load_library().bisip_fp64_stream_probe_lanes())


def fp64_stream_probe_dev(d_out_ptr, rounds, stream=0):
    """One launch of a stream of independent fp64 FMAs (8 waves per SIMD on every compute unit, 32 * ``rounds``
    per wave, operands with full mantissas): the ceiling a compute-bound kernel is held to.  Returns the launch's
    number of wave-instructions; the caller times it."""
    n = ctypes.c_int64(0)
    _check(load_library().bisip_fp64_stream_probe_dev(ctypes.c_void_p(d_out_ptr), int(rounds), ctypes.byref(n), ctypes.c_void_p(stream)))
    return int(n.value)


def rccl_unique_id():
    """ncclGetUniqueId as bytes (rank 0 makes it, every rank passes it to rccl_comm_create)."""
    buf = ctypes.create_string_buffer(RCCL_ID_BYTES)
    _check(load_library().bisip_rccl_unique_id(buf))
    return buf.raw


def rccl_comm_create(world, rank, unique_id, device):
    """ncclCommInitRank on ``device`` (collective over the ranks); returns the ncclComm_t as int."""
    if len(unique_id) != RCCL_ID_BYTES:
        raise ValueError(f'unique_id must be {RCCL_ID_BYTES} bytes')
    comm = ctypes.c_void_p()
    buf = ctypes.create_string_buffer(bytes(unique_id), RCCL_ID_BYTES)
    _check(load_library().bisip_rccl_comm_create(ctypes.byref(comm), int(world), int(rank), buf, int(device)))
    return comm.value


def rccl_comm_destroy(comm):
    _check(load_library().bisip_rccl_comm_destroy(ctypes.c_void_p(comm)))


def chain_moments_workspace(n_samples, n_ensembles, ndim):
    return int(load_library().bisip_chain_moments_workspace(n_samples, n_ensembles, ndim))


def chain_moments_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim,
                      d_mean_ptr, d_std_ptr, d_work_ptr, stream=0):
    """Device pointers (ints); asynchronous on ``stream``."""
    _check(load_library().bisip_chain_moments_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles,
                                                  walkers_per_ensemble, ndim, d_mean_ptr, d_std_ptr,
                                                  d_work_ptr, stream))


def chain_autocorr_time_workspace(n_samples, n_ensembles, walkers_per_ensemble, ndim):
    """Bytes of device scratch chain_autocorr_time_dev needs (0: shape not supported)."""
    return int(load_library().bisip_chain_autocorr_time_workspace(int(n_samples), int(n_ensembles),
                                                                  int(walkers_per_ensemble), int(ndim)))


def chain_autocorr_time_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, c,
                            d_tau_ptr, d_window_ptr, d_work_ptr, stream=0):
    """emcee's integrated autocorrelation time per (ensemble, parameter) into d_tau (n_ensembles, ndim), the
    windows into d_window (int64, or 0 / None); device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_autocorr_time_dev(d_chain_ptr, int(n_samples), int(sample_stride),
                                                        int(n_ensembles), int(walkers_per_ensemble), int(ndim),
                                                        float(c), d_tau_ptr, d_window_ptr or None, d_work_ptr,
                                                        stream))


def rtd_integrals_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim,
                      d_power_sums_ptr, d_norm_factor_ptr, d_out_ptr, stream=0):
    """PolynomialDecomposition's (m_total, log_tau_mean, m_norm) of every used sample into d_out (n_samples,
    n_ensembles * walkers_per_ensemble, 3); device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_rtd_integrals_dev(d_chain_ptr, int(n_samples), int(sample_stride), int(n_ensembles),
                                                  int(walkers_per_ensemble), int(ndim), d_power_sums_ptr,
                                                  d_norm_factor_ptr, d_out_ptr, stream))


def rtd_columns_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, first_ensemble,
                    count, d_log_tau_ptr, n_tau, d_cols_ptr, stream=0):
    """The RTD m_l of every used sample of ensembles [first_ensemble, first_ensemble + count) into d_cols
    (count * n_tau, n_samples * walkers_per_ensemble); device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_rtd_columns_dev(d_chain_ptr, int(n_samples), int(sample_stride), int(n_ensembles),
                                                int(walkers_per_ensemble), int(ndim), int(first_ensemble), int(count),
                                                d_log_tau_ptr, int(n_tau), d_cols_ptr, stream))


def rtd_descriptors_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, d_log_tau_ptr,
                        n_tau, d_q_ptr, n_q, d_out_ptr, stream=0):
    """The relaxation descriptors (log_tau_peak, m_peak, log_tau_q1, ..., log_tau_qJ) of every used sample into d_out
    (n_samples, n_ensembles * walkers_per_ensemble, 2 + n_q); device pointers (ints), asynchronous on ``stream``.  The
    caller has checked ``q`` and the grid (bisip_amd.decomposition.checked_fractions, checked_grid)."""
    _check(load_library().bisip_rtd_descriptors_dev(d_chain_ptr, int(n_samples), int(sample_stride), int(n_ensembles),
                                                    int(walkers_per_ensemble), int(ndim), d_log_tau_ptr, int(n_tau),
                                                    d_q_ptr, int(n_q), d_out_ptr, stream))


def rtd_descriptors_host(chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, log_tau, q, offset=0):
    """Host-only, no GPU: the rows of bisip_rtd_descriptors_dev by the same row function on the CPU
    (bisip_rtd_descriptors_host).  ``chain``: a float64 array whose samples start ``offset`` doubles in and lie
    ``sample_stride`` doubles apart; returns ``(n_samples, n_ensembles * walkers_per_ensemble, 2 + len(q))``."""
    chain, log_tau, q = _c(chain).ravel(), _c(log_tau).ravel(), _c(q).ravel()
    n, stride, rows, ndim, offset = int(n_samples), int(sample_stride), int(n_ensembles) * int(walkers_per_ensemble), int(ndim), int(offset)
    if n < 1 or rows < 1 or offset < 0 or stride < rows * ndim or offset + (n - 1) * stride + rows * ndim > chain.size:
        raise ValueError('the samples asked for lie outside the chain array')
    out = np.empty((n, rows, 2 + q.size))
    _check(load_library().bisip_rtd_descriptors_host(_p(chain[offset:]), n, stride, int(n_ensembles),
                                                     int(walkers_per_ensemble), ndim, _p(log_tau), log_tau.size,
                                                     _p(q), q.size, _p(out)))
    return out


def mode_order_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, n_modes, key_group,
                   d_ordered_ptr, d_desc_ptr, d_moved_ptr, stream=0):
    """The modes of every used sample of a PeltonColeCole chain in the order of ``key_group`` (0: m, 1: log_tau, 2: c) into
    d_ordered (n_samples, n_ensembles * walkers_per_ensemble, 1 + 3 n_modes), their descriptors (m_total, log_tau_cc...,
    log_tau_peak...) into d_desc (..., 1 + 2 n_modes) and whether the order differs from the stored one into d_moved (...)
    uint8; each 0 / None when not asked for, one at least; device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_mode_order_dev(d_chain_ptr, int(n_samples), int(sample_stride), int(n_ensembles),
                                               int(walkers_per_ensemble), int(n_modes), int(key_group), d_ordered_ptr or None,
                                               d_desc_ptr or None, d_moved_ptr or None, stream))


def mode_order_host(chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, n_modes, key_group, ordered=True,
                    desc=True, moved=True, offset=0):
    """Host-only, no GPU: the rows of bisip_mode_order_dev by the same row function on the CPU (bisip_mode_order_host).
    ``chain``: a float64 array whose samples start ``offset`` doubles in and lie ``sample_stride`` doubles apart; returns
    ``(ordered (n_samples, rows, 1 + 3 n_modes), desc (n_samples, rows, 1 + 2 n_modes), moved (n_samples, rows) bool)``,
    None for an output that is not asked for."""
    chain = _c(chain).ravel()
    n, stride, rows, K, offset = int(n_samples), int(sample_stride), int(n_ensembles) * int(walkers_per_ensemble), int(n_modes), int(offset)
    ndim = 1 + 3 * K
    if n < 1 or rows < 1 or K < 1 or offset < 0 or stride < rows * ndim or offset + (n - 1) * stride + rows * ndim > chain.size:
        raise ValueError('the samples asked for lie outside the chain array')
    o = np.empty((n, rows, ndim)) if ordered else None
    d = np.empty((n, rows, 1 + 2 * K)) if desc else None
    mv = np.empty((n, rows), dtype=np.uint8) if moved else None
    _check(load_library().bisip_mode_order_host(_p(chain[offset:]), n, stride, int(n_ensembles), int(walkers_per_ensemble), K,
                                                int(key_group), None if o is None else _p(o), None if d is None else _p(d),
                                                None if mv is None else mv.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))))
    return o, d, None if mv is None else mv.astype(bool)


def lm_step_host(A, g, theta, bounds, lam):
    """Host-only, no GPU: the dense step of one Levenberg-Marquardt iteration by the functions the kernel calls
    (bisip_lm_step_host, csrc/lm_step.h).  A (ndim, ndim), g, theta (ndim), bounds (2, ndim) the PRIOR box.  Returns a dict:
    fixed (ndim,) bool, pred, ok, and delta, trial (ndim) of the candidate with this lambda (NaN when not ok)."""
    A, g, theta = _c(A), _c(g).ravel(), _c(theta).ravel()
    b = _c(bounds).reshape(2, -1)
    lo, hi = _c(b[0]), _c(b[1])
    n = theta.size
    if A.shape != (n, n) or g.size != n or lo.size != n:
        raise ValueError(f'A ({n}, {n}), g, theta ({n},) and bounds (2, {n}) expected')
    delta, trial, pred = np.empty(n), np.empty(n), np.empty(1)
    fixed, ok = ctypes.c_int64(0), ctypes.c_int(0)
    _check(load_library().bisip_lm_step_host(n, _p(A), _p(g), _p(theta), _p(lo), _p(hi), float(lam), _p(delta), _p(trial),
                                             _p(pred), ctypes.byref(fixed), ctypes.byref(ok)))
    return dict(fixed=np.array([(fixed.value >> j) & 1 for j in range(n)], dtype=bool), pred=float(pred[0]), ok=bool(ok.value),
                delta=delta, trial=trial)


def chain_range_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, d_out_ptr,
                    d_nonfinite_ptr, stream=0):
    """Min and max of the finite values per (ensemble, parameter) into d_out (n_ensembles, ndim, 2), the number of
    non-finite values into d_nonfinite (n_ensembles, ndim) int64; device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_range_dev(d_chain_ptr, int(n_samples), int(sample_stride), int(n_ensembles),
                                                int(walkers_per_ensemble), int(ndim), d_out_ptr, d_nonfinite_ptr,
                                                stream))


def chain_histograms_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, d_edges_ptr,
                         bins, d_counts_ptr, stream=0):
    """np.histogram's counts of every (ensemble, parameter) within d_edges (n_ensembles, ndim, bins + 1) into d_counts
    (n_ensembles, ndim, bins) int64; device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_histograms_dev(d_chain_ptr, int(n_samples), int(sample_stride), int(n_ensembles),
                                                     int(walkers_per_ensemble), int(ndim), d_edges_ptr, int(bins),
                                                     d_counts_ptr, stream))


def chain_pair_histograms_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim,
                              d_edges_ptr, bins, d_counts_ptr, stream=0):
    """np.histogram2d's counts of every pair of parameters (np.triu_indices(ndim, 1) order) within d_edges into
    d_counts (n_ensembles, ndim (ndim - 1) / 2, bins, bins) int64; device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_pair_histograms_dev(d_chain_ptr, int(n_samples), int(sample_stride),
                                                          int(n_ensembles), int(walkers_per_ensemble), int(ndim),
                                                          d_edges_ptr, int(bins), d_counts_ptr, stream))


def chain_trace_workspace(n_samples, n_ensembles, walkers_per_ensemble, ndim, n_percentiles):
    """Bytes of device scratch chain_trace_dev needs (0: none; negative: shape not supported)."""
    return int(load_library().bisip_chain_trace_workspace(int(n_samples), int(n_ensembles), int(walkers_per_ensemble),
                                                          int(ndim), int(n_percentiles)))


def chain_trace_lds_walkers(ndim):
    """The largest walkers_per_ensemble that chain_trace_dev sorts in LDS at this ndim (bigger ensembles are gathered
    into columns first and need the workspace)."""
    return int(load_library().bisip_chain_trace_lds_walkers(int(ndim)))


def chain_trace_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, percentiles,
                    d_pct_ptr, d_mean_ptr, d_work_ptr=0, work_bytes=0, stream=0):
    """np.percentile and the mean over the walkers of every (sample, ensemble, parameter): d_pct (len(p), n_samples,
    n_ensembles, ndim), d_mean (n_samples, n_ensembles, ndim) or 0 / None; ``percentiles``: host array in [0, 100], up
    to 8, or None / empty for the mean alone.  Device pointers (ints), asynchronous on ``stream``."""
    p = _c([] if percentiles is None else percentiles).ravel()
    _check(load_library().bisip_chain_trace_dev(d_chain_ptr or None, int(n_samples), int(sample_stride), int(n_ensembles),
                                                int(walkers_per_ensemble), int(ndim), _p(p) if p.size else None, p.size,
                                                d_pct_ptr or None, d_mean_ptr or None, d_work_ptr or None,
                                                int(work_bytes), stream))


def chain_rhat_workspace(n_samples, n_ensembles, walkers_per_ensemble, ndim, splits):
    """Bytes of device scratch chain_rhat_dev needs (0: none; negative: shape not supported)."""
    return int(load_library().bisip_chain_rhat_workspace(int(n_samples), int(n_ensembles), int(walkers_per_ensemble),
                                                         int(ndim), int(splits)))


def chain_rhat_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, splits, d_mean_ptr,
                   d_var_ptr, d_rhat_ptr, d_work_ptr=0, work_bytes=0, stream=0):
    """Mean and variance (ddof = 1) along the step axis of every walker's series, or of its two halves (``splits`` = 1 /
    2): d_mean, d_var (splits, n_ensembles, walkers_per_ensemble, ndim); and the Gelman-Rubin R-hat over those chains:
    d_rhat (n_ensembles, ndim).  Each may be 0 / None, not all.  Device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_rhat_dev(d_chain_ptr or None, int(n_samples), int(sample_stride), int(n_ensembles),
                                               int(walkers_per_ensemble), int(ndim), int(splits), d_mean_ptr or None,
                                               d_var_ptr or None, d_rhat_ptr or None, d_work_ptr or None,
                                               int(work_bytes), stream))


def chain_cov_workspace(n_samples, n_ensembles, walkers_per_ensemble, ndim):
    """Bytes of device scratch chain_cov_dev needs (0: none; negative: shape not supported)."""
    return int(load_library().bisip_chain_cov_workspace(int(n_samples), int(n_ensembles), int(walkers_per_ensemble), int(ndim)))


def chain_cov_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, d_mean_ptr, d_cov_ptr,
                  d_work_ptr=0, work_bytes=0, stream=0):
    """``np.cov(rows.T, ddof=1)`` of every ensemble's used samples: d_cov (n_ensembles, ndim, ndim), d_mean (n_ensembles,
    ndim) or 0 / None.  Device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_cov_dev(d_chain_ptr or None, int(n_samples), int(sample_stride), int(n_ensembles),
                                              int(walkers_per_ensemble), int(ndim), d_mean_ptr or None, d_cov_ptr or None,
                                              d_work_ptr or None, int(work_bytes), stream))


def chain_best_sample_workspace(n_samples, n_ensembles, walkers_per_ensemble):
    """Bytes of device scratch chain_best_sample_dev needs (0: none; negative: shape not supported)."""
    return int(load_library().bisip_chain_best_sample_workspace(int(n_samples), int(n_ensembles), int(walkers_per_ensemble)))


def chain_best_sample_dev(d_chain_ptr, chain_stride, d_logp_ptr, logp_stride, n_samples, n_ensembles, walkers_per_ensemble,
                          ndim, d_theta_ptr, d_best_logp_ptr, d_index_ptr, d_work_ptr=0, work_bytes=0, stream=0):
    """The stored sample of largest log-probability of every ensemble: d_theta (n_ensembles, ndim), d_best_logp
    (n_ensembles,), d_index (n_ensembles,) int64.  Each may be 0 / None, not all; the chain too when theta is.  Device
    pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_best_sample_dev(d_chain_ptr or None, int(chain_stride), d_logp_ptr or None,
                                                      int(logp_stride), int(n_samples), int(n_ensembles),
                                                      int(walkers_per_ensemble), int(ndim), d_theta_ptr or None,
                                                      d_best_logp_ptr or None, d_index_ptr or None, d_work_ptr or None,
                                                      int(work_bytes), stream))


def _windows_array(windows):
    w = [int(k) for k in np.atleast_1d(windows)]
    return (ctypes.c_int64 * max(1, len(w)))(*w), len(w)


def chain_hdi_workspace(n_samples, n_ensembles, walkers_per_ensemble, ndim, windows):
    """Bytes of device scratch chain_hdi_dev needs for the windows ``K`` (negative: shape or windows refused)."""
    w, nw = _windows_array(windows)
    return int(load_library().bisip_chain_hdi_workspace(int(n_samples), int(n_ensembles), int(walkers_per_ensemble), int(ndim),
                                                        nw, w))


def chain_hdi_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, windows, d_out_ptr,
                  d_index_ptr=0, d_work_ptr=0, work_bytes=0, stream=0):
    """Highest-density intervals of every ensemble's used samples for the windows ``K = floor(mass * N)``: d_out
    (len(windows), 2, n_ensembles, ndim), d_index (len(windows), n_ensembles, ndim) int64 or 0 / None.  Device pointers
    (ints), asynchronous on ``stream``."""
    w, nw = _windows_array(windows)
    _check(load_library().bisip_chain_hdi_dev(d_chain_ptr or None, int(n_samples), int(sample_stride), int(n_ensembles),
                                              int(walkers_per_ensemble), int(ndim), w, nw, d_out_ptr or None,
                                              d_index_ptr or None, d_work_ptr or None, int(work_bytes), stream))


def chain_ess_workspace(n_samples, n_ensembles, walkers_per_ensemble, ndim, splits, n_threshold=0):
    """Bytes of device scratch chain_ess_dev needs (0: shape not supported)."""
    return int(load_library().bisip_chain_ess_workspace(int(n_samples), int(n_ensembles), int(walkers_per_ensemble), int(ndim),
                                                        int(splits), int(n_threshold)))


def chain_ess_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, splits, d_threshold_ptr,
                  n_threshold, d_ess_ptr, d_work_ptr=0, work_bytes=0, stream=0):
    """The effective sample size of every (ensemble, parameter) over its walkers' series, or their two halves (``splits``
    = 1 / 2), into d_ess (n_ensembles, ndim); with d_threshold (n_threshold, n_ensembles, ndim) of the indicators ``x <=
    threshold`` instead, into d_ess (n_threshold, n_ensembles, ndim).  Device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_ess_dev(d_chain_ptr or None, int(n_samples), int(sample_stride), int(n_ensembles),
                                              int(walkers_per_ensemble), int(ndim), int(splits), d_threshold_ptr or None,
                                              int(n_threshold), d_ess_ptr or None, d_work_ptr or None, int(work_bytes),
                                              stream))


def chain_rank_normalize_workspace(n_samples, n_ensembles, walkers_per_ensemble, ndim):
    """Bytes of device scratch chain_rank_normalize_dev needs (0: shape not supported, more than 2^31 values)."""
    return int(load_library().bisip_chain_rank_normalize_workspace(int(n_samples), int(n_ensembles),
                                                                   int(walkers_per_ensemble), int(ndim)))


def chain_rank_normalize_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, d_z_ptr,
                             d_work_ptr=0, work_bytes=0, stream=0):
    """The rank-normalised chain (bisip_amd.ess.z_scale per ensemble) into d_z (n_samples, n_ensembles *
    walkers_per_ensemble, ndim), contiguous.  Device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_rank_normalize_dev(d_chain_ptr or None, int(n_samples), int(sample_stride),
                                                         int(n_ensembles), int(walkers_per_ensemble), int(ndim),
                                                         d_z_ptr or None, d_work_ptr or None, int(work_bytes), stream))


def chain_rank_normalize_folded_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim,
                                    d_center_ptr, d_z_ptr, d_work_ptr=0, work_bytes=0, stream=0):
    """The rank-normalised folded chain, ``z_scale(abs(x - center))`` per ensemble with d_center (n_ensembles, ndim), into
    d_z as chain_rank_normalize_dev; its workspace.  Device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_rank_normalize_folded_dev(d_chain_ptr or None, int(n_samples), int(sample_stride),
                                                                int(n_ensembles), int(walkers_per_ensemble), int(ndim),
                                                                d_center_ptr or None, d_z_ptr or None, d_work_ptr or None,
                                                                int(work_bytes), stream))


def chain_ess_squares_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, splits, d_center_ptr,
                          d_ess_ptr, d_work_ptr=0, work_bytes=0, stream=0):
    """chain_ess_dev of the series ``(x - center) * (x - center)`` with d_center (n_ensembles, ndim), into d_ess
    (n_ensembles, ndim); workspace: chain_ess_workspace without thresholds.  Device pointers (ints), asynchronous on
    ``stream``."""
    _check(load_library().bisip_chain_ess_squares_dev(d_chain_ptr or None, int(n_samples), int(sample_stride),
                                                      int(n_ensembles), int(walkers_per_ensemble), int(ndim), int(splits),
                                                      d_center_ptr or None, d_ess_ptr or None, d_work_ptr or None,
                                                      int(work_bytes), stream))


def chain_central_moments_workspace(n_samples, n_ensembles, ndim):
    """DOUBLES of device scratch chain_central_moments_dev needs: twice chain_moments_workspace."""
    return int(load_library().bisip_chain_central_moments_workspace(int(n_samples), int(n_ensembles), int(ndim)))


def chain_central_moments_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, d_center_ptr,
                              d_m2_ptr, d_m4_ptr, d_work_ptr, stream=0):
    """The means of ``(x - center)**2`` and ``(x - center)**4`` of every (ensemble, parameter) into d_m2 and d_m4
    (n_ensembles, ndim), d_center (n_ensembles, ndim).  Device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_chain_central_moments_dev(d_chain_ptr or None, int(n_samples), int(sample_stride),
                                                          int(n_ensembles), int(walkers_per_ensemble), int(ndim),
                                                          d_center_ptr or None, d_m2_ptr or None, d_m4_ptr or None,
                                                          d_work_ptr or None, stream))


def ensemble_gram_workspace(W, ndim):
    """Doubles of device scratch ensemble_gram_dev needs (0: ndim beyond 8)."""
    return int(load_library().bisip_ensemble_gram_workspace(int(W), int(ndim)))


def ensemble_gram_dev(d_coords_ptr, W, ndim, d_out_ptr, d_work_ptr, stream=0):
    """Shifted sums and second moments of a device-resident (W, ndim) ensemble into d_out
    (ndim + ndim (ndim + 1) / 2 doubles); device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_ensemble_gram_dev(d_coords_ptr, int(W), int(ndim), d_out_ptr, d_work_ptr, stream))


def chain_shell_rows_workspace(n_ensembles):
    """Bytes of device scratch chain_shell_rows_dev needs."""
    return int(load_library().bisip_chain_shell_rows_workspace(int(n_ensembles)))


def chain_shell_rows_dev(d_chain_ptr, d_logp_ptr, n_samples, n_ensembles, walkers_per_ensemble, ndim, k, n_stride,
                         d_out_ptr, d_work_ptr, stream=0, ties=True):
    """Per ensemble the k stored samples of smallest |logp| (+ n_stride walkers of the first sample) into
    d_out (n_ensembles, k + n_stride, ndim + 1); device pointers (ints), asynchronous on ``stream``.
    ``ties=False`` leaves out the samples that tie with the k-th (a reproducible set)."""
    _check(load_library().bisip_chain_shell_rows_dev(d_chain_ptr, d_logp_ptr, int(n_samples), int(n_ensembles),
                                                     int(walkers_per_ensemble), int(ndim), int(k), int(n_stride),
                                                     int(bool(ties)), d_out_ptr, d_work_ptr, stream))


def chain_percentiles_workspace(n_samples, n_ensembles, walkers_per_ensemble, ndim, n_percentiles):
    """Bytes of device scratch bisip_chain_percentiles_dev needs (0: shape not supported)."""
    return int(load_library().bisip_chain_percentiles_workspace(n_samples, n_ensembles, walkers_per_ensemble,
                                                                ndim, n_percentiles))


def chain_percentiles_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim,
                          percentiles, d_out_ptr, d_work_ptr, work_bytes, stream=0):
    """Device pointers (ints); ``percentiles`` is a host array in [0, 100]."""
    p = _c(percentiles).ravel()
    _check(load_library().bisip_chain_percentiles_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles,
                                                      walkers_per_ensemble, ndim, _p(p), p.size, d_out_ptr,
                                                      d_work_ptr, work_bytes, stream))


def column_percentiles_workspace(n_rows, n_cols, n_percentiles):
    """BYTES of device workspace for column_percentiles_dev (0: more than 2^31 values)."""
    return int(load_library().bisip_column_percentiles_workspace(int(n_rows), int(n_cols), int(n_percentiles)))


def column_percentiles_dev(d_rows_ptr, n_rows, n_cols, percentiles, d_out_ptr, d_work_ptr, work_bytes, stream=0):
    """np.percentile(rows, p, axis=0) of a device-resident (n_rows, n_cols) array; device pointers (ints)."""
    p = _c(percentiles).ravel()
    _check(load_library().bisip_column_percentiles_dev(d_rows_ptr, int(n_rows), int(n_cols), _p(p), p.size,
                                                       d_out_ptr, d_work_ptr, int(work_bytes), stream))


def columns_percentiles_dev(d_cols_ptr, n_columns, n, percentiles, d_out_ptr, stream=0):
    """np.percentile of n_columns contiguous device columns of n values: d_out (len(p), n_columns).  Device
    pointers (ints); no workspace."""
    p = _c(percentiles).ravel()
    _check(load_library().bisip_columns_percentiles_dev(d_cols_ptr, int(n_columns), int(n), _p(p), p.size, d_out_ptr, stream))


def loo_columns_workspace(n, columns, tail_len):
    """BYTES of device workspace for loo_columns_dev (negative: shape refused)."""
    return int(load_library().bisip_loo_columns_workspace(int(n), int(columns), int(tail_len)))


def loo_columns_dev(d_q_ptr, n, columns, tail_len, d_elpd_rel_ptr, d_khat_ptr, d_sigma_ptr, d_ntail_ptr, d_work_ptr,
                    work_bytes, stream=0):
    """PSIS-LOO of ``columns`` contiguous device columns of ``n`` values ``q`` (bisip_amd.loo.psis_loo_columns): d_elpd_rel,
    d_khat, d_sigma (float64) and d_ntail (int64), ``(columns,)`` each, any 0 / None but not all.  Device pointers (ints),
    asynchronous on ``stream``."""
    _check(load_library().bisip_loo_columns_dev(d_q_ptr or None, int(n), int(columns), int(tail_len), d_elpd_rel_ptr or None,
                                                d_khat_ptr or None, d_sigma_ptr or None, d_ntail_ptr or None,
                                                d_work_ptr or None, int(work_bytes), stream))


def bridge_logg_dev(d_chain_ptr, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim, d_logp_ptr, logp_stride,
                    d_mean_ptr, d_chol_ptr, d_const_ptr, d_l_ptr, stream=0):
    """Bridge sampling, step 1: ``l = logp - log_g`` of every stored row into d_l ``(n_ensembles, n_samples *
    walkers_per_ensemble)``; the proposal is d_mean ``(n_ensembles, ndim)``, d_chol ``(n_ensembles, ndim, ndim)`` lower and
    d_const ``(n_ensembles,)`` (bisip_amd.evidence).  Device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_bridge_logg_dev(d_chain_ptr or None, int(n_samples), int(sample_stride), int(n_ensembles),
                                                int(walkers_per_ensemble), int(ndim), d_logp_ptr or None, int(logp_stride),
                                                d_mean_ptr or None, d_chol_ptr or None, d_const_ptr or None, d_l_ptr or None,
                                                stream))


def bridge_draw_dev(d_mean_ptr, d_chol_ptr, d_const_ptr, n_ensembles, ndim, n_draws, seed, first_draw, first_ensemble,
                    d_theta_ptr, d_logg_ptr, stream=0):
    """Bridge sampling, step 2: draws ``first_draw ... first_draw + n_draws - 1`` of every ensemble's proposal into d_theta
    ``(n_ensembles * n_draws, ndim)`` and their ``log_g`` into d_logg ``(n_ensembles * n_draws,)``; ensemble ``e`` draws from
    the Philox stream of ``first_ensemble + e``.  Device pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_bridge_draw_dev(d_mean_ptr or None, d_chol_ptr or None, d_const_ptr or None, int(n_ensembles),
                                                int(ndim), int(n_draws), int(seed) & 0xffffffffffffffff, int(first_draw),
                                                int(first_ensemble), d_theta_ptr or None, d_logg_ptr or None, stream))


def bridge_scale_dev(d_l1_ptr, n1, d_logp2_ptr, d_logg2_ptr, n2, n_ensembles, d_lstar_ptr, d_l2_ptr, d_a1_ptr, d_a2_ptr,
                     stream=0):
    """Bridge sampling, step 3: ``a1 = exp(-(l2 - lstar))`` ``(n_ensembles, n2)`` with ``l2 = logp2 - logg2`` (into d_l2, 0 /
    None or one of its two inputs) and ``a2 = exp(l1 - lstar)`` ``(n_ensembles, n1)``.  Device pointers (ints)."""
    _check(load_library().bisip_bridge_scale_dev(d_l1_ptr or None, int(n1), d_logp2_ptr or None, d_logg2_ptr or None, int(n2),
                                                 int(n_ensembles), d_lstar_ptr or None, d_l2_ptr or None, d_a1_ptr or None,
                                                 d_a2_ptr or None, stream))


def bridge_iterate_dev(d_a1_ptr, n2, d_a2_ptr, n1, n_ensembles, d_s1_ptr, tol, maxiter, d_r_ptr, d_iterations_ptr,
                       d_moments_ptr, d_f2_ptr=0, stream=0):
    """Bridge sampling, step 4: the iteration of every ensemble on the device: d_r ``(n_ensembles,)`` the final ``r``,
    d_iterations ``(n_ensembles,)`` int64, d_moments ``(n_ensembles, 4)``, d_f2 ``(n_ensembles, n1)`` or 0 / None.  Device
    pointers (ints), asynchronous on ``stream``."""
    _check(load_library().bisip_bridge_iterate_dev(d_a1_ptr or None, int(n2), d_a2_ptr or None, int(n1), int(n_ensembles),
                                                   d_s1_ptr or None, float(tol), int(maxiter), d_r_ptr or None,
                                                   d_iterations_ptr or None, d_moments_ptr or None, d_f2_ptr or None, stream))


def grouped_percentiles_workspace(n_groups, n_rows, n_cols, n_percentiles):
    """BYTES of device workspace for grouped_percentiles_dev (0: more than 2^31 values in one sort)."""
    return int(load_library().bisip_grouped_percentiles_workspace(int(n_groups), int(n_rows), int(n_cols), int(n_percentiles)))


def grouped_percentiles_dev(d_rows_ptr, n_groups, n_rows, n_cols, percentiles, d_out_ptr, d_work_ptr, work_bytes, stream=0):
    """np.percentile(rows[g], p, axis=0) for every g of a device-resident (n_groups, n_rows, n_cols) array in
    one segmented sort; d_out (len(p), n_groups, n_cols).  Device pointers (ints)."""
    p = _c(percentiles).ravel()
    _check(load_library().bisip_grouped_percentiles_dev(d_rows_ptr, int(n_groups), int(n_rows), int(n_cols), _p(p), p.size,
                                                        d_out_ptr, d_work_ptr, int(work_bytes), stream))


def numpy_stretch_stream(rng, W, a, n_steps, out=None):
    """n_steps iterations of the stretch move's RandomState stream, generated in C; ``rng``
    (a numpy.random.RandomState) is advanced exactly as draw_step would advance it.
    Returns active, partner (int32) and zz, u (float64), each (n_steps, 2, (W+1)//2);
    ``out`` = four preallocated C-contiguous arrays of those shapes to fill instead."""
    lib = load_library()
    name, key, pos, has_gauss, cached = rng.get_state()
    if name != 'MT19937':
        raise ValueError('expected an MT19937 RandomState')
    key = np.ascontiguousarray(key, dtype=np.uint32).copy()
    cpos = ctypes.c_int32(int(pos))
    nh = (int(W) + 1) // 2
    shape = (int(n_steps), 2, nh)
    if out is None:
        out = (np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape), np.empty(shape))
    active, partner, zz, u = out
    for arr, dt in ((active, np.int32), (partner, np.int32), (zz, np.float64), (u, np.float64)):
        if arr.shape != shape or arr.dtype != dt or not arr.flags.c_contiguous:
            raise ValueError(f'out arrays must be C-contiguous {shape}: int32, int32, float64, float64')
    _check(lib.bisip_numpy_stretch_stream(key.ctypes.data, ctypes.byref(cpos), int(W), float(a),
                                          int(n_steps), active.ctypes.data, partner.ctypes.data,
                                          zz.ctypes.data, u.ctypes.data))
    rng.set_state((name, key, int(cpos.value), has_gauss, cached))
    return active, partner, zz, u


def read_tables(paths, headers, n_rows, threads=1):
    """Parse many 5-column spectrum files on `threads` host threads (bisip_read_tables).
    Returns ``tables (n_files, n_rows, 5)`` and ``status (n_files,)``: 0 = filled with what
    np.loadtxt yields, 1 = read this file with np.loadtxt instead (see include/bisip_hip.h)."""
    import os
    lib = load_library()
    enc = [os.fsencode(p) for p in paths]
    arr = (ctypes.c_char_p * len(enc))(*enc)
    tables = np.empty((len(enc), int(n_rows), 5), dtype=np.float64)
    status = np.ones(len(enc), dtype=np.int32)
    _check(lib.bisip_read_tables(arr, len(enc), int(headers), int(n_rows), tables.ctypes.data,
                                 status.ctypes.data, int(threads)))
    return tables, status


def philox4x32(counter, key):
    """One Philox4x32-10 block on the host (same inline code as the device stream)."""
    lib = load_library()
    c = (ctypes.c_uint32 * 4)(*[int(x) & 0xffffffff for x in counter])
    k = (ctypes.c_uint32 * 2)(*[int(x) & 0xffffffff for x in key])
    out = (ctypes.c_uint32 * 4)()
    lib.bisip_philox4x32(c, k, out)
    return [int(x) for x in out]
