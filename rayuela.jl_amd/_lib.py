"""ctypes binding of librayuela_hip.so -- the ONLY compute backend of this package.

There is no CPU fallback: if the library is missing or cannot be loaded this module raises,
and every wrapper raises RayuelaHipError on a non-zero status (message from rq_last_error()).
The binding mirrors include/rayuela_hip.h one to one.
"""
import ctypes as C

import numpy as np
import os

_HERE = os.path.dirname(os.path.abspath(__file__))


class RayuelaHipError(RuntimeError):
    pass


def lib_path():
    return os.environ.get("RAYUELA_HIP_LIB", os.path.join(_HERE, "librayuela_hip.so"))


_vp, _i32, _i64, _u32, _u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64

# name -> (restype, argtypes); kept in sync with include/rayuela_hip.h: tests/test_cabi.py parses the header's prototypes and
# compares names, arity and the size, signedness and kind of every argument and return type
SIGNATURES = {
    "rq_version": (C.c_char_p, []),
    "rq_last_scan_kernel": (C.c_char_p, []),
    "rq_last_error": (C.c_char_p, []),
    "rq_device_count": (_i32, []),
    "rq_set_device": (_i32, [_i32]),
    "linscan_aqd_query": (None, [_vp, _vp, _vp, _vp, _vp, _i32, C.c_uint, _i32, _i32, _i32, _i32, _i32]),
    "linscan_aqd_query_extra_byte": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32]),
    "linscan_aqd_cq_query_extra_byte": (None, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32]),
    "rq_linscan_lsq": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32]),
    "rq_linscan_cq": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32]),
    "rq_lsq_prepare": (_vp, [_vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_lsq_search": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32]),
    "rq_lsq_release": (None, [_vp]),
    "rq_lsq_prepare_cbnorms": (_vp, [_vp, _vp, _vp, _i32, _i64, _i32, _i32, _i32]),
    "rq_aq_norms": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_dev_aq_norms": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_quantize_norms": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32]),
    "rq_dev_quantize_norms": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "rq_get_norms_codebook": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _u64]),
    "rq_dev_linscan_aq": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _u32, _i32, _vp]),
    "rq_linscan_pq": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32]),
    "rq_linscan_opq": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32]),
    "rq_encode_pq": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_encode_opq": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_encode_pq_i16": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_encode_opq_i16": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_encode_pq_bytes": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_encode_opq_bytes": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_encode_pq_bytes_i16": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_encode_opq_bytes_i16": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_encode_pq_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32]),
    "rq_encode_opq_wide": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32]),
    "rq_encode_rvq_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "rq_dev_encode_pq_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_encode_opq_wide": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_encode_rvq_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "rq_encode_rvq": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "rq_encode_rvq_i16": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "rq_train_rvq": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, C.c_uint64]),
    "rq_dev_encode_rvq": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "rq_encode_rvq_beam": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "rq_encode_rvq_beam_i16": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "rq_dev_encode_rvq_beam": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "rq_encode_rvq_beam_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "rq_dev_encode_rvq_beam_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "rq_last_beam_timing": (_i32, [_vp, _i32]),
    "rq_ervq_update_codebook_wide": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32]),
    "rq_train_ervq_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _u64, _i32]),
    "rq_ervq_update_codebook": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32]),
    "rq_train_ervq": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _u64]),
    "rq_last_ervq_timing": (_i32, [_vp, _i32]),
    "rq_encode_icm": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _u64, _i64, _i32]),
    "rq_dev_encode_icm": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _u64, _i64,
                                 _i32, _vp]),
    "rq_last_icm_timing": (_i32, [_vp, _vp]),
    "rq_encode_icm_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _u64, _i64, _i32,
                                  _i32]),
    "rq_icm_wide_plan": (_i32, [_i64, _i32, _i32, _i32, _i32, _vp, _i32]),
    "rq_update_codebooks_lsq": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_double]),
    "rq_dev_update_codebooks_lsq": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_double, _vp]),
    "rq_dev_lsq_normal_eq": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_double, _vp]),
    "rq_train_lsq": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _u64, _i32]),
    "rq_last_lsq_timing": (_i32, [_vp, _i32]),
    "rq_update_codebooks_lsq_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_double, _i32]),
    "rq_lsq_normal_eq_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_double, _i32]),
    "rq_lsq_wide_plan": (_i32, [_i64, _i32, _i32, _i32, _vp, _i32]),
    "rq_train_lsq_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _u64, _i32,
                                 _i32]),
    "rq_sr_std": (_i32, [_vp, _vp, _i64, _i32]),
    "rq_sr_perturb": (_i32, [_vp, _vp, _vp, C.c_double, _i64, _i32, _i32, _u64, _i64, _i64]),
    "rq_sr_schedule": (_i32, [_vp, _i32, _i64, _i64, C.c_double]),
    "rq_train_sr": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                           C.c_double, _i32, _u64, _i32]),
    "rq_last_sr_timing": (_i32, [_vp, _i32]),
    "rq_train_sr_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                C.c_double, _i32, _u64, _i32, _i32, _i32]),
    "rq_last_sr_stats": (_i32, [_vp, _i32]),
    "rq_quantize_chainq": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32]),
    "rq_dev_quantize_chainq": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "rq_chain_dims": (_i32, [_i32, _i32, _vp, _vp]),
    "rq_update_codebooks_chain": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_double]),
    "rq_dev_update_codebooks_chain": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_double, _vp]),
    "rq_dev_reconstruct_aq": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_train_chainq": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32]),
    "rq_last_chainq_timing": (_i32, [_vp, _i32]),
    "rq_quantize_chainq_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32]),
    "rq_update_codebooks_chain_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, C.c_double, _i32]),
    "rq_train_chainq_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32]),
    "rq_chain_wide_plan": (_i32, [_i64, _i32, _i32, _i32, _i32, _vp, _i32]),
    "rq_dataset_upload": (_vp, [_vp, _i64, _i32]),
    "rq_dataset_upload_bytes": (_vp, [_vp, _i64, _i32]),
    "rq_dataset_encode": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32]),
    "rq_dataset_free": (None, [_vp]),
    "rq_encode_pq_bytes_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32]),
    "rq_encode_opq_bytes_wide": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32]),
    "rq_dataset_encode_wide": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32]),
    "rq_rotate_T": (_i32, [_vp, _vp, _vp, _i32, _i64]),
    "rq_dev_encode_pq": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_encode_pq_filter_w": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_last_encode_kernel": (C.c_char_p, []),
    "rq_last_encode_stats": (C.c_int, [C.c_void_p]),
    "rq_dev_rotate_T": (_i32, [_vp, _vp, _vp, _i32, _i64, _vp]),
    "rq_dev_encode_opq": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_encode_pq_bytes": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_encode_opq_bytes": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_rotate_T_bytes": (_i32, [_vp, _vp, _vp, _i32, _i64, _vp]),
    "rq_dev_adc_lut": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "rq_dev_linscan": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _u32, _i32, _vp]),
    "rq_linscan_pq_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32]),
    "rq_linscan_opq_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32]),
    "rq_dev_linscan_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _u32, _i32, _vp]),
    "rq_dev_adc_lut_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_linscan_lsq_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32]),
    "rq_linscan_cq_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32]),
    "rq_linscan_lsq_cbnorms_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32,
                                           _i32]),
    "rq_dev_linscan_aq_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _u32, _i32,
                                      _vp]),
    "rq_dev_aq_lut_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "rq_aq_norms_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32]),
    "rq_dev_aq_norms_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_quantize_norms_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32]),
    "rq_dev_quantize_norms_wide": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "rq_get_norms_codebook_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _u64, _i32]),
    "rq_scan_wide_plan": (_i32, [_i32, _i32, _vp, _i32]),
    "rq_scan_wide_slices": (_i32, [_i64, _i64, _i32, _i32, _i32, _vp, _i32]),
    "rq_scan_row_width": (_i32, [_i32]),
    "rq_order_bytes": (_i64, [_i64, _i32]),
    "rq_order_plan": (_i32, [_i64, _i32, _vp, _i32]),
    "rq_dev_order_rows": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "rq_dev_linscan_ordered": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _u32, _i32, _vp]),
    "rq_dev_merge_topk": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_synth_codes": (_i32, [_vp, _i64, _i32, _u64, _i64, _vp]),
    "rq_dev_update_centers": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_reconstruct": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_qerror": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "rq_dev_gram": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "rq_dev_gram_codes": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_qerror_codes": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_kmpp_seeds": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _u64]),
    "rq_train_pq": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _u64]),
    "rq_train_opq": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _u64, _vp, _vp]),
    "rq_train_pq_wide": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _u64, _i32]),
    "rq_train_opq_wide": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _u64, _vp, _vp, _i32]),
    "rq_train_rvq_wide": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _u64, _i32]),
    "rq_dev_update_centers_wide": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_dev_reconstruct_wide": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "rq_train_profile": (_i32, [_vp, _i32]),
    "rq_dev_polar_factor": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "rq_index_create": (_vp, [_i32, _i32, _vp]),
    "rq_index_create_sharded": (_vp, [_i32, _i32, _vp, _vp, _i32]),
    "rq_index_set_codes": (_i32, [_vp, _vp, _i64, _u32]),
    "rq_index_set_codes_synth": (_i32, [_vp, _i64, _u64, _u32]),
    "rq_index_create_wide": (_vp, [_i32, _i32, _i32, _vp]),
    "rq_index_create_sharded_wide": (_vp, [_i32, _i32, _i32, _vp, _vp, _i32]),
    "rq_index_set_codes_wide": (_i32, [_vp, _vp, _i64, _i32, _u32]),
    "rq_index_create_aq": (_vp, [_i32, _i32, _vp, _i32, _vp, _i32]),
    "rq_index_create_aq_wide": (_vp, [_i32, _i32, _i32, _vp, _i32, _vp, _i32]),
    "rq_index_set_codes_aq": (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _u32]),
    "rq_index_set_codes_aq_wide": (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _u32]),
    "rq_index_aq_info": (_i32, [_vp, _vp, _i32]),
    "rq_ivf_create": (_vp, [_i32, _i32, _vp, _i32, _vp, _i32]),
    "rq_ivf_build": (_i32, [_vp, _vp, _i64, _u32]),
    "rq_ivf_set_codes": (_i32, [_vp, _vp, _vp, _i64, _u32]),
    "rq_ivf_build_bytes": (_i32, [_vp, _vp, _i64, _u32]),
    "rq_ivf_add": (_i32, [_vp, _vp, _i64, _u32]),
    "rq_ivf_add_bytes": (_i32, [_vp, _vp, _i64, _u32]),
    "rq_ivf_add_codes": (_i32, [_vp, _vp, _vp, _i64, _u32]),
    "rq_ivf_search": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32]),
    "rq_ivf_search_refine": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _u32, _i32]),
    "rq_ivf_get_lists": (_i32, [_vp, _vp, _vp, _vp]),
    "rq_ivf_info": (_i32, [_vp, _vp, _i32]),
    "rq_ivf_last_timing": (_i32, [_vp, _vp, _i32]),
    "rq_ivf_destroy": (None, [_vp]),
    "rq_index_search_opq": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32]),
    "rq_index_info": (_i32, [_vp, _vp, _i32]),
    "rq_release_workspaces": (_i32, []),
    "rq_host_alloc": (_vp, [C.c_size_t]),
    "rq_host_free": (None, [_vp]),
    "rq_index_search": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32]),
    "rq_index_destroy": (None, [_vp]),
    "rq_set_tuning": (_i32, [C.c_char_p, _i32]),
    "rq_reset_tuning": (_i32, [C.c_char_p]),
    "rq_scan_stats": (_i32, [_vp]),
    "rq_scan_orders_in_call": (_i32, [_i64, _i64, _i32]),
    "rq_scan_finish_stats": (_i32, [_vp]),
    "rq_order_cache_stats": (_i32, [_vp]),
    "rq_scan_plan": (_i32, [_i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "rq_last_timing": (_i32, [_vp, _vp, _vp, _vp]),
    "rq_test_fill_scratch": (_i32, [_i32, _vp]),
    "rq_test_scratch_report": (_i32, [_vp, _vp, _vp, _i32]),
    "rq_centers_plan": (_i32, [_i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32]),
    "rq_knn_f32": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32]),
    "rq_knn": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32]),
    "rq_knn_bytes": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32]),
    "rq_dataset_knn": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32]),
    "rq_last_knn_stats": (_i32, [_vp]),
    "rq_last_knn_timing": (_i32, [_vp, _i32]),
    "rq_knn_plan": (_i32, [_i64, _i64, _i32, _i32, _vp, _i32]),
    "rq_test_knn_chunk_rows": (_i64, [_i64]),
    "rq_dataset_rerank": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _u32, _i32]),
    "rq_last_rerank_timing": (_i32, [_vp, _i32]),
    "rq_last_rerank_stats": (_i32, [_vp]),
    "rq_rerank_plan": (_i32, [_i64, _i64, _i32, _i64, _i32, _vp, _i32]),
    "rq_test_rerank_limits": (_i64, [_i64, _i64]),
    "rq_test_scan_wide_slice_rows": (_i64, [_i64]),
}

_LIB = None


def lib():
    """Load the shared library (once).  Raises RayuelaHipError if it is not there."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.isfile(path):
            raise RayuelaHipError(
                "librayuela_hip.so not found at %s -- build it with `make -C rayuela.jl_amd/csrc` "
                "(or __graft_entry__.build()); there is no CPU fallback" % path)
        try:
            # torch (when used for device memory / RCCL) bundles its own libamdhip64.so.7: importing it
            # first makes both sides share ONE HIP runtime, so device pointers are interchangeable.
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the pure host-pointer API
            pass
        handle = C.CDLL(path)
        lenient = os.environ.get("RAYUELA_HIP_LENIENT") == "1"     # tools/ab_shard.py against an OLDER build: newer symbols may be absent
        for name, (res, args) in SIGNATURES.items():
            if lenient and not hasattr(handle, name):
                continue
            fn = getattr(handle, name)  # AttributeError here == ABI mismatch; let it surface
            fn.restype = res
            fn.argtypes = args
        _LIB = handle
    return _LIB


def check(status):
    if status != 0:
        msg = lib().rq_last_error().decode("utf-8", "replace")
        raise RayuelaHipError("librayuela_hip status %d: %s" % (status, msg))


def set_tuning(key, value):
    check(lib().rq_set_tuning(key.encode(), int(value)))


def reset_tuning(key=None):
    """Forget what set_tuning stored for `key` (None: every key): the knob reads RQ_<KEY> from the environment again, else
    the library's default."""
    check(lib().rq_reset_tuning(None if key is None else key.encode()))


def scan_plan(n, nq, m, d, k, num_cu=256):
    """The planner's decision (host code only): dict of qg, groups, whole, slices, rows_per_slice, grid, cap, bigk, xcd, bulk.
    bulk = 1: k > RQ_MAX_K takes the bulk top-k path (grid: its distance kernel, cap: queries per batch)."""
    out = (C.c_int64 * 8)()
    check(lib().rq_scan_plan(n, nq, m, d, k, num_cu, C.cast(out, C.c_void_p)))
    keys = ("qg", "groups", "whole", "slices", "rows_per_slice", "grid", "cap", "flags")
    p = dict(zip(keys, [int(x) for x in out]))
    p["bigk"], p["xcd"], p["bulk"] = p["flags"] & 1, (p["flags"] >> 1) & 1, (p["flags"] >> 2) & 1
    return p


def scan_wide_plan(m, h):
    """Where the scan over 16-bit codes keeps its table of m * h entries (host code only, rq_scan_wide_plan): dict of qpg (queries
    per gather: 4, 2 or 1), in_lds (1: the table of a query group is in LDS, 0: gathered from global memory), qg (queries per
    group) and lds_bytes."""
    out = (C.c_int * 4)()
    check(lib().rq_scan_wide_plan(m, h, C.cast(out, C.c_void_p), 4))
    return dict(zip(("qpg", "in_lds", "qg", "lds_bytes"), [int(x) for x in out]))


def scan_wide_slices(n, nq, m, h, k):
    """How the scan over 16-bit codes takes n rows and nq queries through its scratch budget (host code only,
    rq_scan_wide_slices): dict of rows (per slice), slices, batch (queries), bytes (scratch of a batch) and forced (1: the test
    hook rq_test_scan_wide_slice_rows set rows)."""
    out = (C.c_int64 * 5)()
    check(lib().rq_scan_wide_slices(n, nq, m, h, k, C.cast(out, C.c_void_p), 5))
    return dict(zip(("rows", "slices", "batch", "bytes", "forced"), [int(x) for x in out]))


def order_cache_stats():
    """The kept in-call row order of raw-pointer scans on the current device since the last release (rq_order_cache_stats)."""
    out = (C.c_uint64 * 8)()
    check(lib().rq_order_cache_stats(C.cast(out, C.c_void_p)))
    return dict(zip(["consulted", "hits", "plain_builds", "balanced_builds", "uncached", "upgrades"], [int(x) for x in out[:6]]))


WS_SLOTS = 20          # csrc/rq_internal.h (tests/test_gpu_scratch.py reads the names from there)


def fill_scratch(value):
    """Test hook, not for callers (rq_test_fill_scratch): every byte of library scratch on the current device becomes `value`."""
    out = (C.c_uint64 * 7)()
    check(lib().rq_test_fill_scratch(int(value), C.cast(out, C.c_void_p)))
    return dict(zip(["slot_bytes", "pool_bytes", "pinned_bytes", "slots", "ws_gen", "pool_buffers", "pinned_blocks"],
                    [int(x) for x in out]))


def scratch_report(stream=0):
    """Test hook, not for callers (rq_test_scratch_report): (bytes, differs) per scratch slot of `stream` (a handle; 0: null)."""
    nbytes, differs = (C.c_int64 * WS_SLOTS)(), (C.c_int * WS_SLOTS)()
    check(lib().rq_test_scratch_report(C.c_void_p(stream or None), C.cast(nbytes, C.c_void_p), C.cast(differs, C.c_void_p), WS_SLOTS))
    return [int(x) for x in nbytes], [bool(x) for x in differs]


def scan_stats():
    out = (C.c_uint64 * 16)()
    check(lib().rq_scan_stats(C.cast(out, C.c_void_p)))
    names = ["lut", "sample", "stream", "cuts", "final_cut", "sort_write", "n_cuts", "n_fallbacks", "sample_rows", "sort_load", "sort_stages", "sort_out", "n_items", "n_items_filtered", "first_block_pushed", "first_block_rows"]
    st = dict(zip(names, [int(x) for x in out]))
    fin = (C.c_uint64 * 8)()
    check(lib().rq_scan_finish_stats(C.cast(fin, C.c_void_p)))
    st.update(zip(["bf_items", "bf_look_skips", "bf_select_sort"], [int(x) for x in fin[:3]]))
    return st


class _PinnedBlock:
    """A page-locked buffer of the library's pool, exposed through the array interface; returned to the pool when the
    last numpy view of it is collected."""

    def __init__(self, ptr, shape, dtype):
        self._ptr = ptr
        self.__array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(dtype).str, "data": (ptr, False), "version": 3}

    def __del__(self):
        try:
            lib().rq_host_free(self._ptr)
        except Exception:     # noqa: BLE001 -- interpreter shutdown
            pass


# Results below this size are not worth a pool round trip (and small pinned allocations fragment the pool)
_PIN_MIN_BYTES = 4 << 20


def result_empty(shape, dtype):
    """An uninitialised result array: page-locked memory from the library's pool (rq_host_alloc) when the array is large,
    else numpy's own.  Page-locked results skip the first-touch page faults that otherwise bound the copy back
    (include/rayuela_hip.h); they are ordinary numpy arrays to the caller."""
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dtype.itemsize
    if nbytes >= _PIN_MIN_BYTES:
        ptr = lib().rq_host_alloc(nbytes)
        if ptr:
            return np.asarray(_PinnedBlock(ptr, shape, dtype))
    return np.empty(shape, dtype=dtype)


TRAIN_PHASES = ["h2d_ms", "init_ms", "qerror_ms", "gram_ms", "svd_ms", "rotate_ms", "update_centers_ms", "encode_ms",
                "reconstruct_ms", "converge_ms", "d2h_ms", "loop_ms", "iterations", "jacobi_sweeps", "ns_steps", "host_polar"]


def train_profile():
    """Phase clock of this thread's last train_pq / train_opq call (rq_train_profile)."""
    out = (C.c_double * 16)()
    check(lib().rq_train_profile(C.cast(out, C.c_void_p), 16))
    return dict(zip(TRAIN_PHASES, [float(x) for x in out]))


def last_timing():
    t = (C.c_double * 4)()
    p = [C.cast(C.byref(t, 8 * i), C.c_void_p) for i in range(4)]
    lib().rq_last_timing(*p)
    return dict(total_ms=t[0], h2d_ms=t[1], kernel_ms=t[2], d2h_ms=t[3])
