"""ctypes binding of libmi355rec.so (C ABI declared in include/mi355rec.h).

There is NO CPU fallback: if the shared library is missing, or no gfx950 device is visible when a handle is
created, the call raises.  The library is only dlopen()ed on first use and the HIP context is only created
by the first *_create call, so importing this package before a fork (the reference's hyper-parameter search
forks one worker per configuration, ParameterTuning/run_parameter_search.py:498) is safe.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MI355REC_LIB: another build of the same library, for measurements of compile-time variants)
LIB_PATH = os.environ.get("MI355REC_LIB") or os.path.join(_HERE, "libmi355rec.so")

E_INVALID, E_HIP, E_NO_DEVICE, E_UNSUPPORTED, E_NUMERIC = -1, -2, -3, -4, -5

SIMILARITY_CODES = {"cosine": 0, "adjusted": 1, "asymmetric": 2, "pearson": 3, "jaccard": 4, "tanimoto": 4,
                    "dice": 5, "tversky": 6, "euclidean": 7}
EUCLIDEAN_MODE_CODES = {"lin": 0, "log": 1, "exp": 2}
FEATURE_WEIGHTING_CODES = {"none": 0, "BM25": 1, "TF-IDF": 2}
SGD_MODE_CODES = {"sgd": 0, "adagrad": 1, "rmsprop": 2, "adam": 3}
ALGORITHM_CODES = {"MF_BPR": 0, "FUNK_SVD": 1, "ASY_SVD": 2}
PRECISION_CODES = {"fp32": 0, "fp64": 1}


class NativeLibraryError(RuntimeError):
    """libmi355rec.so is missing, or the HIP runtime / device failed."""


class Stats(C.Structure):
    _fields_ = [("call_ms", C.c_double), ("kernel_ms", C.c_double), ("n_launches", C.c_int64), ("n_timed", C.c_int64),
                ("n_units", C.c_int64), ("algorithmic_bytes", C.c_double), ("algorithmic_flops", C.c_double),
                ("loss", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class SimConfig(C.Structure):
    _fields_ = [("topK", C.c_int32), ("shrink", C.c_int32), ("normalize", C.c_int32), ("similarity", C.c_int32),
                ("asymmetric_alpha", C.c_float), ("tversky_alpha", C.c_float), ("tversky_beta", C.c_float),
                ("unit_column_side", C.c_int32), ("normalize_avg_row", C.c_int32), ("euclidean_mode", C.c_int32),
                ("feature_weighting", C.c_int32), ("weighting_documents", C.c_int32), ("bm25_k1", C.c_float), ("bm25_b", C.c_float),
                ("norm_sum_order", C.c_int32), ("reserved", C.c_int32)]


class MFConfig(C.Structure):
    _fields_ = [("algorithm", C.c_int32), ("n_factors", C.c_int32), ("batch_size", C.c_int32),
                ("use_bias", C.c_int32), ("sgd_mode", C.c_int32), ("learning_rate", C.c_double),
                ("user_reg", C.c_double), ("item_reg", C.c_double), ("bias_reg", C.c_double),
                ("positive_reg", C.c_double), ("negative_reg", C.c_double),
                ("negative_interactions_quota", C.c_double),
                ("gamma", C.c_double), ("beta_1", C.c_double), ("beta_2", C.c_double),
                ("random_seed", C.c_uint64), ("precision", C.c_int32), ("reserved", C.c_int32)]


class SlimConfig(C.Structure):
    _fields_ = [("symmetric", C.c_int32), ("sgd_mode", C.c_int32), ("learning_rate", C.c_double),
                ("li_reg", C.c_double), ("lj_reg", C.c_double),
                ("gamma", C.c_double), ("beta_1", C.c_double), ("beta_2", C.c_double), ("random_seed", C.c_uint64),
                ("precision", C.c_int32), ("train_with_sparse_weights", C.c_int32), ("topK", C.c_int32), ("reserved", C.c_int32)]


class CsrBlock(C.Structure):
    """mi355rec_csr_block: one resident CSR matrix of a stack and the factor its values are multiplied by."""
    _fields_ = [("n_rows", C.c_int32), ("nnz", C.c_int32), ("d_indptr", C.c_void_p), ("d_indices", C.c_void_p), ("d_data", C.c_void_p),
                ("scale", C.c_float)]


STACK_MAX_BLOCKS = 16

_vp = C.c_void_p
_i32, _i64, _f32, _f64 = C.c_int32, C.c_int64, C.c_float, C.c_double

# name -> (restype, argtypes); must list every symbol declared in include/mi355rec.h
SIGNATURES = {
    "mi355rec_last_error": (C.c_char_p, []),
    "mi355rec_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mi355rec_set_device": (C.c_int, [C.c_int]),
    "mi355rec_device_name": (C.c_int, [C.c_char_p, C.c_int]),
    "mi355rec_device_malloc": (C.c_int, [C.POINTER(_vp), C.c_uint64]),
    "mi355rec_device_free": (C.c_int, [_vp]),
    "mi355rec_device_memcpy": (C.c_int, [_vp, _vp, C.c_uint64, C.c_int]),
    "mi355rec_device_synchronize": (C.c_int, []),
    "mi355rec_device_trim": (C.c_int, [C.POINTER(C.c_uint64)]),
    "mi355rec_sim_create": (C.c_int, [C.POINTER(_vp), C.POINTER(SimConfig), _i32, _i32, _vp, _vp, _vp, _vp]),
    "mi355rec_sim_create_resident": (C.c_int, [C.POINTER(_vp), C.POINTER(SimConfig), _i32, _i32, _vp, _vp, _vp, _vp]),
    "mi355rec_sim_get_weighted_values": (C.c_int, [_vp, _vp]),
    "mi355rec_sim_compute_part_device": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "mi355rec_sim_compute_part_chunk_device": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "mi355rec_sim_pack_slab_device": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "mi355rec_sim_unpack_slab_device": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "mi355rec_sim_part_columns": (C.c_int, [_vp, _i32, _i32, _vp, C.POINTER(_i32)]),
    "mi355rec_sim_compute": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "mi355rec_sim_compute_device": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "mi355rec_sim_compute_dense": (C.c_int, [_vp, _i32, _i32, _vp, _i64]),
    "mi355rec_sim_compute_dense_device": (C.c_int, [_vp, _i32, _i32, _vp, _i64]),
    "mi355rec_sim_compute_csr": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "mi355rec_sim_column_costs": (C.c_int, [_vp, _vp]),
    "mi355rec_sim_schedule_info": (C.c_int, [_vp, _vp, _vp, _vp]),
    "mi355rec_sim_accumulator_info": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_f64)]),
    "mi355rec_sim_selection_info": (C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "mi355rec_lds_atomic_rate": (C.c_int, [C.POINTER(_f64)]),
    "mi355rec_sim_sync": (C.c_int, [_vp]),
    "mi355rec_sim_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_sim_destroy": (None, [_vp]),
    "mi355rec_csr_stack_device": (C.c_int, [_i32, C.POINTER(CsrBlock), _i32, _vp, _vp, _vp]),
    "mi355rec_mf_create": (C.c_int, [C.POINTER(_vp), C.POINTER(MFConfig), _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "mi355rec_mf_run_epochs": (C.c_int, [_vp, _i32]),
    "mi355rec_mf_run_samples": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64]),
    "mi355rec_mf_shard_begin_epoch": (C.c_int, [_vp, _i32, _i32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_uint64), C.POINTER(_i32)]),
    "mi355rec_mf_shard_batch": (C.c_int, [_vp, _i32]),
    "mi355rec_mf_shard_merge": (C.c_int, [_vp, _i32]),
    "mi355rec_mf_shard_end_epoch": (C.c_int, [_vp]),
    "mi355rec_mf_get_factors": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mi355rec_mf_get_factors_f64": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "mi355rec_mf_asy_user_factors": (C.c_int, [_vp, _vp, _vp]),
    "mi355rec_asy_user_factors": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi355rec_mf_get_last_samples": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(_i64)]),
    "mi355rec_mf_set_profiling": (C.c_int, [_vp, _i32]),
    "mi355rec_mf_get_phase_ticks": (C.c_int, [_vp, _vp, _i64, C.POINTER(_i64)]),
    "mi355rec_mf_get_schedule_ticks": (C.c_int, [_vp, _vp, _i64, C.POINTER(_i64)]),
    "mi355rec_mf_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_mf_destroy": (None, [_vp]),
    "mi355rec_mf_group_create": (C.c_int, [C.POINTER(_vp), C.POINTER(_vp), _i32]),
    "mi355rec_mf_group_run_epochs": (C.c_int, [_vp, _i32]),
    "mi355rec_mf_group_set_profiling": (C.c_int, [_vp, _i32]),
    "mi355rec_mf_group_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_mf_group_destroy": (None, [_vp]),
    "mi355rec_slim_create": (C.c_int, [C.POINTER(_vp), C.POINTER(SlimConfig), _i32, _i32, _vp, _vp]),
    "mi355rec_slim_run_epochs": (C.c_int, [_vp, _i32]),
    "mi355rec_slim_run_samples": (C.c_int, [_vp, _vp, _vp, _vp, _i64]),
    "mi355rec_slim_get_last_samples": (C.c_int, [_vp, _vp, _vp, _vp, _i64, C.POINTER(_i64)]),
    "mi355rec_slim_get_S_topk": (C.c_int, [_vp, _i32, _vp, _vp]),
    "mi355rec_slim_get_W_csr": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int64)]),
    "mi355rec_slim_get_S_sparse": (C.c_int, [_vp, _vp, _vp]),
    "mi355rec_slim_get_S_dense": (C.c_int, [_vp, _vp]),
    "mi355rec_slim_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_slim_schedule_info": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "mi355rec_slim_destroy": (None, [_vp]),
    "mi355rec_ials_create": (C.c_int, [C.POINTER(_vp), _i32, _i32, _i32, _f64, _vp, _vp, _vp, _vp, _vp]),
    "mi355rec_ials_run_epochs": (C.c_int, [_vp, _i32]),
    "mi355rec_ials_user_half": (C.c_int, [_vp, _i32, _i32]),
    "mi355rec_ials_item_half": (C.c_int, [_vp, _i32, _i32]),
    "mi355rec_ials_device_factors": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "mi355rec_ials_sync": (C.c_int, [_vp]),
    "mi355rec_ials_get_factors": (C.c_int, [_vp, _vp, _vp]),
    "mi355rec_ials_schedule_info": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "mi355rec_ials_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_ials_destroy": (None, [_vp]),
    "mi355rec_slimen_create": (C.c_int, [C.POINTER(_vp), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi355rec_slimen_fit": (C.c_int, [_vp, _i32, _i32, _vp, _f64, _f64, _i32, _i32, _i32, _f64]),
    "mi355rec_slimen_get": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "mi355rec_slimen_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_slimen_fit_info": (C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i32),
                                           C.POINTER(_i32), C.POINTER(_f64)]),
    "mi355rec_slimen_get_gram": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "mi355rec_slimen_destroy": (None, [_vp]),
    "mi355rec_svd_create": (C.c_int, [C.POINTER(_vp), _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi355rec_svd_set_block": (C.c_int, [_vp, _i32, _vp]),
    "mi355rec_svd_get_block": (C.c_int, [_vp, _i32, _vp]),
    "mi355rec_svd_product": (C.c_int, [_vp, _i32]),
    "mi355rec_svd_gram": (C.c_int, [_vp, _i32, _vp]),
    "mi355rec_svd_apply": (C.c_int, [_vp, _i32, _vp]),
    "mi355rec_svd_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_svd_fit_info": (C.c_int, [_vp, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_i64), C.POINTER(_i64),
                                        C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i32)]),
    "mi355rec_svd_destroy": (None, [_vp]),
    "mi355rec_nmf_create": (C.c_int, [C.POINTER(_vp), _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mi355rec_nmf_set_block": (C.c_int, [_vp, _i32, _vp]),
    "mi355rec_nmf_get_block": (C.c_int, [_vp, _i32, _vp]),
    "mi355rec_nmf_fill_block": (C.c_int, [_vp, _i32, _f32]),
    "mi355rec_nmf_cd_sweep": (C.c_int, [_vp, _i32, _vp, _i32, C.POINTER(_f64)]),
    "mi355rec_nmf_mu_step": (C.c_int, [_vp, _i32, _i32, _i32]),
    "mi355rec_nmf_divergence": (C.c_int, [_vp, _i32, C.POINTER(_f64)]),
    "mi355rec_nmf_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_nmf_fit_info": (C.c_int, [_vp, C.POINTER(_f64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64),
                                        C.POINTER(_i64), C.POINTER(_i32)]),
    "mi355rec_nmf_destroy": (None, [_vp]),
    "mi355rec_ease_create": (C.c_int, [C.POINTER(_vp), _i32]),
    "mi355rec_ease_set_gram_from_sim": (C.c_int, [_vp, _vp]),
    "mi355rec_ease_set_matrix": (C.c_int, [_vp, _vp, _i64]),
    "mi355rec_ease_get_matrix": (C.c_int, [_vp, _vp, _i64]),
    "mi355rec_ease_set_diagonal": (C.c_int, [_vp, _vp]),
    "mi355rec_ease_invert": (C.c_int, [_vp]),
    "mi355rec_ease_invert_pivoted": (C.c_int, [_vp]),
    "mi355rec_ease_pivot_info": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64)]),
    "mi355rec_ease_get_dense": (C.c_int, [_vp, _vp, _i64]),
    "mi355rec_ease_get_topk": (C.c_int, [_vp, _i32, _vp, _vp]),
    "mi355rec_ease_fit_info": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_f64), C.POINTER(_f64),
                                         C.POINTER(_f64), C.POINTER(_i64)]),
    "mi355rec_ease_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_ease_destroy": (None, [_vp]),
    "mi355rec_scorer_create": (C.c_int, [C.POINTER(_vp), _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _f32, _vp, _vp]),
    "mi355rec_scorer_update": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _f32]),
    "mi355rec_scorer_update_from_mf": (C.c_int, [_vp, _vp]),
    "mi355rec_scorer_update_from_ials": (C.c_int, [_vp, _vp]),
    "mi355rec_scorer_recommend": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mi355rec_scorer_recommend_candidates": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "mi355rec_scorer_score_capacity": (C.c_int, [_vp, C.POINTER(_i64)]),
    "mi355rec_scorer_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_scorer_destroy": (None, [_vp]),
    "mi355rec_spscorer_create": (C.c_int, [C.POINTER(_vp), _i32, _i32, _i32] + [_vp] * 8),
    "mi355rec_spscorer_recommend": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mi355rec_spscorer_recommend_candidates": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "mi355rec_spscorer_set_exact": (C.c_int, [_vp, _i32]),
    "mi355rec_spscorer_update_b": (C.c_int, [_vp, _vp, _vp, _vp]),
    "mi355rec_spscorer_get_b": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(_i64)]),
    "mi355rec_spscorer_update_from_slim": (C.c_int, [_vp, _vp, _i32]),
    "mi355rec_spscorer_get_stats":(C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_spscorer_destroy": (None, [_vp]),
    "mi355rec_dscorer_create": (C.c_int, [C.POINTER(_vp), _i32, _i32, _i32] + [_vp] * 6),
    "mi355rec_dscorer_update": (C.c_int, [_vp, _vp]),
    "mi355rec_dscorer_set_from_ease": (C.c_int, [_vp, _vp]),
    "mi355rec_dscorer_recommend": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mi355rec_dscorer_recommend_candidates": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "mi355rec_dscorer_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_dscorer_destroy": (None, [_vp]),
    "mi355rec_itemscorer_create": (C.c_int, [C.POINTER(_vp), _i32, _i32, _vp, _vp, _vp]),
    "mi355rec_itemscorer_create_resident": (C.c_int, [C.POINTER(_vp), _i32, _i32, _vp, _vp, _vp, _i64]),
    "mi355rec_itemscorer_update": (C.c_int, [_vp, _vp]),
    "mi355rec_itemscorer_recommend": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "mi355rec_itemscorer_recommend_candidates": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "mi355rec_itemscorer_window_bits": (C.c_int, [_vp, C.POINTER(_i32)]),
    "mi355rec_itemscorer_set_window_bits": (C.c_int, [_vp, _i32]),
    "mi355rec_itemscorer_get_stats": (C.c_int, [_vp, C.POINTER(Stats)]),
    "mi355rec_itemscorer_destroy": (None, [_vp]),
    "mi355rec_urm_item_counts": (C.c_int, [_i32, _i32, _vp, _vp, _vp]),
    "mi355rec_urm_item_counts_resident": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp]),
    "mi355rec_urm_global_effects": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _f64, _f64, C.POINTER(_f32), _vp, _vp]),
    "mi355rec_urm_global_effects_resident": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _f64, _f64, C.POINTER(_f32), _vp, _vp]),
    "mi355rec_eval_create": (C.c_int, [C.POINTER(_vp), _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i32]),
    "mi355rec_eval_begin": (C.c_int, [_vp, _vp, _vp, _vp, _i32]),
    "mi355rec_eval_add_lists": (C.c_int, [_vp, _i32, _i32, _vp]),
    "mi355rec_eval_add_scorer": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "mi355rec_eval_add_spscorer": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "mi355rec_eval_add_itemscorer": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "mi355rec_eval_add_dscorer": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "mi355rec_eval_add_dscorer_candidates": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "mi355rec_eval_set_candidates": (C.c_int, [_vp, _vp, _vp]),
    "mi355rec_eval_add_scorer_candidates": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "mi355rec_eval_add_spscorer_candidates": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "mi355rec_eval_add_itemscorer_candidates": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "mi355rec_eval_finish": (C.c_int, [_vp, _vp, _vp]),
    "mi355rec_eval_get_per_user": (C.c_int, [_vp, _vp]),
    "mi355rec_eval_set_diversity": (C.c_int, [_vp, _vp, _i32]),
    "mi355rec_eval_get_diversity": (C.c_int, [_vp, _vp, _vp]),
    "mi355rec_eval_diversity_info": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_f64), C.POINTER(_f64)]),
    "mi355rec_eval_destroy": (None, [_vp]),
}

_lib = None


def load():
    """dlopen libmi355rec.so (built by __graft_entry__.build() / `make -C csrc`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise NativeLibraryError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as exc:
        raise NativeLibraryError("cannot load %s: %s" % (LIB_PATH, exc)) from exc
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError here = header and library out of sync
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc):
    """Map a C-ABI return code to the exception the reference would raise at the same point."""
    if rc == 0:
        return
    msg = load().mi355rec_last_error().decode("utf-8", "replace")
    if rc == E_INVALID:
        raise ValueError(msg)
    if rc == E_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == E_NUMERIC:
        raise FloatingPointError(msg)
    raise NativeLibraryError(msg)


class Handle:
    """Base of every wrapper of a native handle type: `_PREFIX` names its entry points ("mi355rec_ials" -> mi355rec_ials_create,
    mi355rec_ials_<name>, mi355rec_ials_get_stats, mi355rec_ials_destroy).  `_h` is the handle (a c_void_p) while the object is
    open and None before a successful _create and after close()."""
    _PREFIX = None
    _h = None

    def _create(self, *args, entry="create"):
        self._lib = load()
        h = C.c_void_p()
        check(getattr(self._lib, "%s_%s" % (self._PREFIX, entry))(C.byref(h), *args))
        self._h = h

    def _call(self, name, *args):
        if not self._h:
            raise ValueError("%s is closed" % type(self).__name__)
        check(getattr(self._lib, "%s_%s" % (self._PREFIX, name))(self._h, *args))

    def stats(self):
        """The library's figures of the last call on this handle, as a dict."""
        st = Stats()
        self._call("get_stats", C.byref(st))
        return st.as_dict()

    def close(self):
        h, self._h = self._h, None
        if h:
            getattr(self._lib, self._PREFIX + "_destroy")(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ptr(array):
    """Host pointer of a C-contiguous ndarray (or None)."""
    if array is None:
        return None
    assert array.flags["C_CONTIGUOUS"]
    return array.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int(0)
    check(load().mi355rec_device_count(C.byref(n)))
    return n.value


def set_device(index):
    check(load().mi355rec_set_device(int(index)))


def device_name():
    buf = C.create_string_buffer(256)
    check(load().mi355rec_device_name(buf, 256))
    return buf.value.decode()


def as_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def as_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def both_layouts(matrix):
    """(X, arrays): X is `matrix` as float32 CSR with sorted indices; arrays are its indptr, indices and data followed by those of its
    sorted CSC, six contiguous arrays as the create calls of the handles that keep both layouts take them."""
    import scipy.sparse as sps
    X = sps.csr_matrix(matrix, dtype=np.float32)
    X.sort_indices()
    Xc = sps.csc_matrix(X)
    Xc.sort_indices()
    return X, (as_i32(X.indptr), as_i32(X.indices), as_f32(X.data), as_i32(Xc.indptr), as_i32(Xc.indices), as_f32(Xc.data))


def lds_atomic_rate():
    """ds_add_u32 lane-adds per second of the whole device on uniformly random LDS cells (the similarity build's roofline peak)."""
    rate = C.c_double(0.0)
    check(load().mi355rec_lds_atomic_rate(C.byref(rate)))
    return float(rate.value)


def trim_device_cache():
    """Give the library's cache of released device blocks back to the driver (a process that shares the GPU with PyTorch / RCCL calls
    this between phases of fits); returns the bytes freed."""
    freed = C.c_uint64(0)
    check(load().mi355rec_device_trim(C.byref(freed)))
    return int(freed.value)


class DeviceArray:
    """A raw device allocation of the calling process's GPU (int32 words), released with the object."""

    def __init__(self, n_words):
        self.n_words = int(n_words)
        self.ptr = C.c_void_p()
        check(load().mi355rec_device_malloc(C.byref(self.ptr), 4 * self.n_words))

    def address(self, word_offset=0):
        return (self.ptr.value or 0) + 4 * int(word_offset)

    def to_host(self, out=None):
        out = np.empty(self.n_words, np.int32) if out is None else out
        check(load().mi355rec_device_memcpy(ptr(out), self.ptr, 4 * self.n_words, 0))
        return out

    def copy_from_device(self, other, n_words, word_offset=0):
        """Blocking device-to-device copy of other[0:n_words] into self[word_offset:...]."""
        check(load().mi355rec_device_memcpy(C.c_void_p(self.address(word_offset)), other.ptr, 4 * int(n_words), 2))

    def close(self):
        if getattr(self, "ptr", None) is not None and self.ptr.value:
            load().mi355rec_device_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _HostIdentity:
    """Which host CSR matrix is this?  Remembers one (its arrays are shared, not copied: the addresses of its three buffers are
    part of its identity) and recognises it, or an equal copy, when it is presented again: `matches`."""

    def __init__(self, csr):
        self.nnz = int(csr.nnz)
        self._fingerprint = self.fingerprint_of(csr)
        self._buffers = self._buffers_of(csr)
        self._host = csr                         # (keeps the buffers alive: their addresses identify the matrix)
        self._full = None
        self._verified = {}
        self._calls = 0

    @staticmethod
    def fingerprint_of(csr):
        """Shape, nnz and a checksum of a sample of the row pointers (every 64th: each one counts ALL the entries before it), indices and values (every nnz / 8192-th entry:
        a strided sample is one cache miss per entry, 65 536 of them per array cost 0.5 ms of every constructor)."""
        import zlib
        return (csr.shape, int(csr.nnz), zlib.crc32(np.ascontiguousarray(csr.indptr, np.int32)[::64].tobytes()),
                zlib.crc32(np.ascontiguousarray(csr.data, np.float32)[:: max(1, csr.nnz // 8192)].tobytes()),
                zlib.crc32(np.ascontiguousarray(csr.indices, np.int32)[:: max(1, csr.nnz // 8192)].tobytes()))

    @staticmethod
    def _buffers_of(csr):
        return tuple(a.__array_interface__["data"][0] for a in (csr.indptr, csr.indices, csr.data))

    @staticmethod
    def _full_checksum(csr):
        """Digest of EVERY index and value.  xxh3 where the module is there (7 ms per 80 MB array; zlib.crc32 over a copy of the bytes took 150):
        a search that hands every fit its own copy of URM_train pays this once per fit, so it has to stay near the 3 ms upload it saves."""
        arrays = (np.ascontiguousarray(csr.indices, np.int32), np.ascontiguousarray(csr.data, np.float32))
        try:
            import xxhash
            return tuple(xxhash.xxh3_128_digest(memoryview(a)) for a in arrays)
        except ImportError:
            import zlib
            return tuple(zlib.crc32(memoryview(a)) for a in arrays)

    def _rotating_sample_equal(self, csr):
        """A strided sample of indices and values of `csr` against the same positions of the uploaded matrix; the offset moves on
        with every call, so that repeated fits look at different entries (8192 per array and call)."""
        stride = max(1, self.nnz // 8192)
        self._calls += 1
        at = (self._calls * 2654435761) % stride
        mine = self._host
        return (np.array_equal(np.asarray(csr.indices)[at::stride], mine.indices[at::stride]) and
                np.array_equal(np.asarray(csr.data, dtype=np.float32)[at::stride], mine.data[at::stride]))

    def matches(self, csr, thorough=None):
        """Is `csr` the uploaded matrix?  Always compared: shape, nnz, every 64th row pointer, a fixed sample of indices and values and
        a second sample whose offset changes from call to call -- a fraction of a millisecond.  The FIRST time a matrix (identified
        by the addresses of its three buffers) is presented, a checksum of EVERY index and value is compared as well (~15 ms at
        ML-20M size) and the verdict is remembered for those buffers: the hundreds of fits of a search on the same URM_train copy
        (the recommenders copy it in their constructor, BaseRecommender.py:29, so it is never the uploaded object itself) pay it
        once.  thorough=True (or MI355REC_RESIDENT_VERIFY=full) compares the checksum on every call; thorough=False (or
        MI355REC_RESIDENT_VERIFY=sample) never does (the caller vouches for the copy)."""
        import os
        if self.fingerprint_of(csr) != self._fingerprint or not self._rotating_sample_equal(csr):
            return False
        key = self._buffers_of(csr)
        if key == self._buffers:
            return True
        if thorough is None:
            mode = os.environ.get("MI355REC_RESIDENT_VERIFY", "")
            thorough = True if mode == "full" else (False if mode == "sample" else None)
        if thorough is False:
            return True
        seen = self._verified
        if thorough is None and key in seen:
            return seen[key]
        if self._full is None:
            self._full = self._full_checksum(self._host)
        verdict = self._full_checksum(csr) == self._full
        if len(seen) >= 64:
            seen.clear()
        seen[key] = verdict
        return verdict


class ResidentURM:
    """A CSR matrix (int32 structure, float32 values, sorted indices) uploaded ONCE to the calling process's GPU.  Similarity
    builds started from it (`Compute_Similarity_MI355X(..., resident=...)`, `ItemKNNCFRecommender.fit(..., resident_urm=...)`)
    copy the arrays at HBM speed instead of paying the PCIe upload in every fit -- the reference's hyper-parameter search runs
    hundreds of fits on the same URM_train (ParameterTuning/SearchAbstractClass.py:253-262)."""

    def __init__(self, matrix):
        import scipy.sparse as sps
        csr = sps.csr_matrix(matrix, dtype=np.float32)
        if not csr.has_sorted_indices:
            csr = csr.sorted_indices()
        self.shape = csr.shape
        self.nnz = int(csr.nnz)
        self._host = csr
        self._identity = _HostIdentity(csr)
        # A CSC input is the transpose of a CSR matrix its owner keeps (`ICM_train.T`, `URM_train.T`: same three buffers): that
        # matrix is remembered too, so that `matches_transposed` recognises it without a transposition per fit -- one more sampled
        # fingerprint here, no copy.  (Like `_host` for a sorted float32 CSR input it shares the owner's arrays: a matrix edited in
        # place after the upload is not the uploaded matrix any more, whichever of the two is asked.)
        self._transposed = _HostIdentity(sps.csr_matrix(matrix.T, dtype=np.float32)) if sps.isspmatrix_csc(matrix) else None
        self.indptr, self.indices, self.data = DeviceArray(len(csr.indptr)), DeviceArray(max(1, self.nnz)), DeviceArray(max(1, self.nnz))
        lib = load()
        for dev, host in ((self.indptr, as_i32(csr.indptr)), (self.indices, as_i32(csr.indices)), (self.data, as_f32(csr.data))):
            if len(host):
                check(lib.mi355rec_device_memcpy(dev.ptr, ptr(host), 4 * len(host), 1))

    # ---- which host matrix this is: `_HostIdentity` above; the names below are this class's long-standing surface
    fingerprint_of = staticmethod(_HostIdentity.fingerprint_of)
    _buffers_of = staticmethod(_HostIdentity._buffers_of)

    @property
    def _verified(self):
        return self._identity._verified

    def matches(self, csr, thorough=None):
        """Is `csr` the uploaded matrix?  See `_HostIdentity.matches`."""
        return self._identity.matches(csr, thorough)

    def matches_transposed(self, csr, thorough=None):
        """Is the uploaded matrix the transpose of `csr`?  Answered for an object made from a CSC matrix (`ResidentURM(M.T)` of a CSR
        M): `csr` is compared with that M exactly as `matches` compares with the uploaded matrix -- no transposition."""
        return self._transposed is not None and self._transposed.matches(csr, thorough)

    # ---- what a ResidentStack asks of its blocks
    def value_range(self):
        """(smallest, largest) stored value, (0, 0) for an empty matrix; one pass over the host copy, remembered."""
        if getattr(self, "_range", None) is None:
            d = self._host.data
            self._range = (float(d.min()), float(d.max())) if len(d) else (0.0, 0.0)
        return self._range

    def count_non_finite(self):
        return int(np.sum(np.logical_not(np.isfinite(self._host.data))))

    def close(self):
        for a in (self.indptr, self.indices, self.data):
            a.close()


class ResidentStack:
    """`ResidentURM` blocks stacked row-wise into one CSR matrix IN device memory, block b's values multiplied by scales[b]
    (mi355rec_csr_stack_device): bit for bit the arrays of `scipy.sparse.vstack([b * s ...], format="csr")`.  The dataMatrix of the CF+CBF
    hybrid KNN recommenders -- feature rows times ICM_weight on top of the user rows -- made at HBM speed for every fit of a search,
    from blocks that were uploaded once.  `indptr`, `indices`, `data` are DeviceArrays; `download()` returns the host CSR."""

    def __init__(self, blocks, scales):
        blocks, scales = list(blocks), [float(s) for s in scales]
        if not blocks or len(blocks) != len(scales):
            raise ValueError("ResidentStack: %d blocks and %d scales" % (len(blocks), len(scales)))
        n_cols = blocks[0].shape[1]
        if any(b.shape[1] != n_cols for b in blocks):
            raise ValueError("ResidentStack: the blocks have different numbers of columns: {}".format([b.shape for b in blocks]))
        n_rows, nnz = sum(b.shape[0] for b in blocks), sum(b.nnz for b in blocks)
        if n_rows >= 2 ** 31 - 1 or nnz > 2 ** 31 - 1:
            raise ValueError("ResidentStack: %d rows and %d cells do not fit int32 row pointers" % (n_rows, nnz))
        self.blocks, self.scales = blocks, scales
        self.shape, self.nnz = (n_rows, n_cols), nnz
        self.indptr, self.indices, self.data = DeviceArray(n_rows + 1), DeviceArray(max(1, nnz)), DeviceArray(max(1, nnz))
        table = (CsrBlock * len(blocks))(*[CsrBlock(b.shape[0], b.nnz, b.indptr.ptr, b.indices.ptr, b.data.ptr, s)
                                           for b, s in zip(blocks, scales)])
        check(load().mi355rec_csr_stack_device(len(blocks), table, n_cols, self.indptr.ptr, self.indices.ptr, self.data.ptr))

    def structure(self):
        """(indptr, indices) as host arrays, read back from the device copy."""
        indptr = self.indptr.to_host()
        return indptr, (self.indices.to_host()[:self.nnz] if self.nnz else np.empty(0, np.int32))

    def download(self):
        """The stacked matrix as a host CSR (float32, the blocks' sorted indices)."""
        import scipy.sparse as sps
        indptr, indices = self.structure()
        data = self.data.to_host()[:self.nnz].view(np.float32) if self.nnz else np.empty(0, np.float32)
        return sps.csr_matrix((data, indices, indptr), shape=self.shape)

    def values_nonnegative(self):
        """No stored value of the stack is negative -- from the blocks' value ranges and the signs of the scales, nothing is read back."""
        for b, s in zip(self.blocks, self.scales):
            lo, hi = b.value_range()
            if (s > 0 and lo < 0) or (s < 0 and hi > 0):
                return False
        return True

    def count_non_finite(self):
        """For the message of the reference's assertion (a block under a non-finite scale counts whole)."""
        return sum(b.count_non_finite() if np.isfinite(s) else b.nnz for b, s in zip(self.blocks, self.scales))

    def close(self):
        for a in (self.indptr, self.indices, self.data):
            a.close()
