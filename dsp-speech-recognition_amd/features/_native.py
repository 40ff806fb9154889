"""ctypes binding of libdsp_frontend.so (include/dsp_frontend.h) -- the only way this package
computes anything.  There is deliberately NO CPU fallback: if the library or a GPU is missing,
every compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
LIB_PATH = os.environ.get('DSP_FRONTEND_LIB', os.path.join(_PKG, 'lib', 'libdsp_frontend.so'))

OK, EINVAL, EHIP, ENODEV = 0, -1, -2, -3
WAVE_F32, WAVE_I16 = 0, 1
OUT_FRAMES, OUT_MAGSPEC, OUT_POWSPEC, OUT_FBANK, OUT_MFCC = 0, 1, 2, 3, 4
PLAN_ANY_NFFT = 1
ROUTE_PASSES, ROUTE_MIXED, ROUTE_CHIRP = 0, 1, 2
VAD_PER_FRAME, VAD_SCAN, VAD_SUM, VAD_TILE_ABS, VAD_TILE_SQ = 0, 1, 2, 3, 4     # dsp_debug_vad_route

c_i32, c_i64, c_f32, c_f64, c_vp = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p


class PlanDesc(C.Structure):
    _fields_ = [
        ('frame_len', c_i32), ('frame_step', c_i32), ('nfft', c_i32), ('nfilt', c_i32),
        ('numcep', c_i32), ('append_energy', c_i32), ('preemph', c_f32),
        ('h_window', c_vp), ('h_mel_start', c_vp), ('h_mel_count', c_vp), ('h_mel_weights', c_vp),
        ('h_dct', c_vp), ('h_window64', c_vp), ('preemph64', c_f64),
    ]


class HmlstmDesc(C.Structure):
    _fields_ = [
        ('input_size', c_i32), ('hidden1', c_i32), ('hidden2', c_i32), ('reserved', c_i32),
        ('d_c1_U11', c_vp), ('d_c1_U21', c_vp), ('d_c1_W01', c_vp), ('d_c1_bias', c_vp),
        ('d_c2_U11', c_vp), ('d_c2_W01', c_vp), ('d_c2_bias', c_vp),
    ]


class BigruDesc(C.Structure):
    _fields_ = [
        ('input_size', c_i32), ('hidden', c_i32), ('n_layers', c_i32), ('reserved', c_i32),
        ('d_params', c_vp * 32),
    ]


class SvmDesc(C.Structure):
    _fields_ = [
        ('n_features', c_i32), ('n_sv', c_i32), ('class0', c_i32), ('class1', c_i32),
        ('gamma', c_f64), ('intercept', c_f64),
        ('h_center', c_vp), ('h_scale', c_vp), ('h_sv', c_vp), ('h_dual', c_vp),
    ]


class AttnDesc(C.Structure):
    _fields_ = [
        ('d_model', c_i32), ('d_inner', c_i32), ('n_head', c_i32), ('d_k', c_i32), ('d_v', c_i32), ('eps', c_f32),
        ('d_params', c_vp * 16),
    ]


class RowsOperand(C.Structure):
    _fields_ = [('d_ptr', c_vp), ('stride_t', c_i64), ('stride_b', c_i64), ('cols', c_i32), ('reserved', c_i32)]


class GraphCensus(C.Structure):
    _fields_ = [('n_nodes', c_i32), ('n_kernel', c_i32), ('n_memset', c_i32), ('n_memcpy', c_i32), ('n_other', c_i32),
                ('n_wide_memset', c_i32), ('n_roots', c_i32), ('max_fanout', c_i32), ('widest_memset_bytes', c_i64),
                ('names_bytes', c_i64)]


class EnsembleRule(C.Structure):
    _fields_ = [('label_a', c_i32), ('label_b', c_i32), ('threshold', c_f64), ('svm', c_vp)]


# name -> (restype, argtypes); mirrors include/dsp_frontend.h one to one.
SIGNATURES = {
    'dsp_abi_version': (C.c_int, []),
    'dsp_last_error': (C.c_char_p, []),
    'dsp_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'dsp_set_device': (C.c_int, [C.c_int]),
    'dsp_get_device': (C.c_int, [c_vp]),
    'dsp_malloc': (C.c_int, [C.POINTER(c_vp), C.c_size_t]),
    'dsp_free': (C.c_int, [c_vp]),
    'dsp_memcpy_h2d': (C.c_int, [c_vp, c_vp, C.c_size_t, c_vp]),
    'dsp_memcpy_d2h': (C.c_int, [c_vp, c_vp, C.c_size_t, c_vp]),
    'dsp_memset': (C.c_int, [c_vp, C.c_int, C.c_size_t, c_vp]),
    'dsp_stream_synchronize': (C.c_int, [c_vp]),
    'dsp_frame_count': (C.c_int, [c_i64, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_frame_offsets': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp]),
    'dsp_frames_bound': (C.c_int, [c_i64, c_i32, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_batch_offsets_batch': (C.c_int, [c_vp, c_i32, c_i64, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_layout_create_capacity': (C.c_int, [c_i32, c_i64, c_i32, c_i32, C.POINTER(c_vp)]),
    'dsp_layout_refresh': (C.c_int, [c_vp, c_vp, c_vp]),
    'dsp_plan_create': (C.c_int, [C.POINTER(PlanDesc), C.POINTER(c_vp)]),
    'dsp_plan_create_ex': (C.c_int, [C.POINTER(PlanDesc), C.c_uint32, C.POINTER(c_vp)]),
    'dsp_plan_transform': (C.c_int, [c_vp, C.POINTER(c_i32), C.POINTER(c_i32)]),
    'dsp_debug_plan_transform_tables': (C.c_int, [c_vp, c_vp, c_i32, C.POINTER(c_i32), c_vp, c_vp]),
    'dsp_plan_destroy': (C.c_int, [c_vp]),
    'dsp_plan_has_fast_path': (C.c_int, [c_vp]),
    'dsp_debug_force_generic': (C.c_int, [C.c_int]),
    'dsp_debug_pool_stats': (C.c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    'dsp_debug_use_mfma512': (C.c_int, [C.c_int]),
    'dsp_debug_host_dry_run': (C.c_int, [C.c_int]),
    'dsp_debug_vad_route': (C.c_int, [c_i32, c_i32, C.c_int, c_i32, C.POINTER(c_i32)]),
    'dsp_plan_has_mfma512': (C.c_int, [c_vp]),
    'dsp_preemphasis_batch': (C.c_int, [c_vp, C.c_int, c_vp, c_i32, c_i64, c_f32, c_vp, c_vp]),
    'dsp_features_batch': (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp, c_i32, c_i64, c_i64, C.c_int,
                                     c_vp, c_i64, c_vp, c_vp]),
    'dsp_delta_batch': (C.c_int, [c_vp, c_i64, c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp, c_i64,
                                  c_vp, c_i64, c_vp]),
    'dsp_mfcc_delta_batch': (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp, c_i32, c_i64, c_i64, c_i32,
                                       c_vp, c_vp]),
    'dsp_scale_columns': (C.c_int, [c_vp, c_i64, c_i32, c_vp, c_vp]),
    'dsp_vad_features_batch': (C.c_int, [c_vp, C.c_int, c_vp, c_vp, c_i32, c_i64, c_i64, c_i32, c_i32,
                                         c_i32, c_vp, c_vp, c_vp]),
    'dsp_segments_workspace_bytes': (C.c_int, [c_vp, c_i32, c_i64, C.POINTER(C.c_size_t)]),
    'dsp_mfcc_delta_segments_batch': (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_i32,
                                                c_vp, C.c_size_t, c_vp, c_vp]),
    'dsp_endpoint_layout_segments_batch': (C.c_int, [c_vp, c_vp, c_i32, c_f64, c_f64, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                     c_i64, c_vp, C.c_size_t, c_vp]),
    'dsp_layout_create': (C.c_int, [c_vp, c_i32, c_i64, c_i32, c_i32, c_vp, C.POINTER(c_vp)]),
    'dsp_layout_destroy': (C.c_int, [c_vp]),
    'dsp_vad_features_layout_batch': (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    'dsp_trim_scale_batch': (C.c_int, [c_vp, C.c_int, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    'dsp_endpoint_rule_batch': (C.c_int, [c_vp, c_vp, c_vp, c_i32, c_i32, c_f64, c_f64, c_vp, c_vp]),
    'dsp_acr_gate_batch': (C.c_int, [c_vp, C.c_int, c_vp, c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_i32, c_i32, c_f64, c_vp, c_vp]),
    'dsp_endpoint_rule_acr_batch': (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_f64, c_f64, c_vp, c_vp]),
    'dsp_endpoint_layout_batch': (C.c_int, [c_vp, c_vp, c_i32, c_f64, c_f64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_model_timefeat_batch': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'dsp_pitch_scores_batch': (C.c_int, [c_vp, c_vp, c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp, c_i32,
                                         c_i32, c_i32, c_vp, c_vp]),
    'dsp_pitch_track_batch': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'dsp_pitch_rows_batch': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'dsp_pitch_cepstrum_batch': (C.c_int, [c_vp, c_vp, c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp, c_i32, c_vp, c_vp, c_vp]),
    'dsp_pitch_cepstrum_track_batch': (C.c_int, [c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    'dsp_pitch_feature_batch': (C.c_int, [c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_vp]),
    'dsp_pitch_smooth_subseq_batch': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_f64, c_vp, c_vp, c_vp]),
    'dsp_resample_layout_batch': (C.c_int, [c_vp, c_i32, c_i64, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
    'dsp_decimate_batch': (C.c_int, [c_vp, c_vp, c_vp, c_i32, c_i64, c_i64, c_i64, c_vp, c_vp]),
    'dsp_model_pitchfeat_batch': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    'dsp_model_finalize_batch': (C.c_int, [c_vp, c_i64, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    'dsp_model_finalize_segments_batch': (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    'dsp_hmlstm_create': (C.c_int, [C.POINTER(HmlstmDesc), C.POINTER(c_vp)]),
    'dsp_hmlstm_destroy': (C.c_int, [c_vp]),
    'dsp_hmlstm_forward': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_hmlstm_tape_bytes': (C.c_int, [c_vp, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_hmlstm_forward_train': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                           c_i64, c_vp]),
    'dsp_hmlstm_backward': (C.c_int, [c_vp, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                      c_vp, c_vp]),
    'dsp_hmlstm_forward_train_rows': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                c_vp, c_vp, c_i64, c_vp]),
    'dsp_hmlstm_backward_rows': (C.c_int, [c_vp, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                           c_vp, c_vp, c_vp, c_vp]),
    'dsp_bigru_create': (C.c_int, [C.POINTER(BigruDesc), C.POINTER(c_vp)]),
    'dsp_bigru_destroy': (C.c_int, [c_vp]),
    'dsp_bigru_workspace_bytes': (C.c_int, [c_vp, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_bigru_forward': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'dsp_bigru_tape_bytes': (C.c_int, [c_vp, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_bigru_tape_rows': (C.c_int, [c_vp, c_i32, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_bigru_forward_train': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'dsp_bigru_backward': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp]),
    'dsp_svm_create': (C.c_int, [C.POINTER(SvmDesc), C.POINTER(c_vp)]),
    'dsp_svm_destroy': (C.c_int, [c_vp]),
    'dsp_svm_decision_batch': (C.c_int, [c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_vp]),
    'dsp_ensemble_decide_batch': (C.c_int, [c_vp, c_i64, c_i32, c_i32, C.POINTER(EnsembleRule), c_i32, c_vp, c_i64, c_vp, c_i64,
                                            c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_trim_preemph_batch': (C.c_int, [c_vp, C.c_int, c_vp, c_vp, c_vp, c_i32, c_f64, c_vp, c_vp]),
    'dsp_model_finalize_placed_batch': (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp,
                                                  c_vp, c_i32, c_i32, c_i32, c_vp]),
    'dsp_model_timefeat_placed_batch': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    'dsp_model_pitchfeat_placed_batch': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp]),
    'dsp_gather_clips_batch': (C.c_int, [c_vp, C.c_int, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp]),
    'dsp_rate_groups_batch': (C.c_int, [c_vp, c_vp, c_vp, c_i32, c_i64, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_gather_groups_batch': (C.c_int, [c_vp, C.c_int, c_vp, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp]),
    'dsp_scatter_segments_batch': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    'dsp_scatter_group_rows_batch': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'dsp_attn_create': (C.c_int, [C.POINTER(AttnDesc), C.POINTER(c_vp)]),
    'dsp_attn_destroy': (C.c_int, [c_vp]),
    'dsp_attn_workspace_bytes': (C.c_int, [c_vp, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_attn_forward': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp]),
    'dsp_selfattn_pool_batch': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_selfattn_pool_rows_batch': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_head_lengths_batch': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp]),
    'dsp_head_pool_batch': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp]),
    'dsp_attn_tape_bytes': (C.c_int, [c_vp, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_attn_forward_train': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp]),
    'dsp_attn_backward_bytes': (C.c_int, [c_vp, c_i32, c_i32, C.POINTER(c_i64), C.POINTER(c_i64)]),
    'dsp_attn_backward': (C.c_int, [c_vp, c_i32, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp]),
    'dsp_selfattn_pool_train_batch': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_selfattn_pool_backward_batch': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_head_pool_train_batch': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_vp, c_vp]),
    'dsp_head_pool_backward_batch': (C.c_int, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp]),
    'dsp_selfattn_pool_rows_train_batch': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_selfattn_pool_rows_backward_batch': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp,
                                                        c_vp, c_vp]),
    'dsp_bigru_refresh': (C.c_int, [c_vp, C.POINTER(BigruDesc), c_vp]),
    'dsp_hmlstm_refresh': (C.c_int, [c_vp, C.POINTER(HmlstmDesc), c_vp]),
    'dsp_attn_refresh': (C.c_int, [c_vp, C.POINTER(AttnDesc), c_vp]),
    'dsp_adam_chunk_elems': (C.c_int, []),
    'dsp_adam_chunk_table': (C.c_int, [c_i32, c_vp, c_i64, c_vp, c_vp, C.POINTER(c_i64)]),
    'dsp_adam_create': (C.c_int, [c_i32, c_vp, c_vp, c_vp, c_vp, c_f64, c_f64, c_f64, c_f64, C.POINTER(c_vp)]),
    'dsp_adam_destroy': (C.c_int, [c_vp]),
    'dsp_adam_bind_grads': (C.c_int, [c_vp, c_vp, c_vp]),
    'dsp_adam_set_hyper': (C.c_int, [c_vp, c_f64, c_f64, c_f64, c_f64, c_vp]),
    'dsp_adam_set_step': (C.c_int, [c_vp, c_i64, c_vp]),
    'dsp_adam_get_state': (C.c_int, [c_vp, C.POINTER(c_i64), c_vp, c_vp]),
    'dsp_adam_step': (C.c_int, [c_vp, c_i32, c_vp]),
    'dsp_rows_wgrad_scratch_bytes': (C.c_int, [c_i32, c_i32, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_rows_wgrad': (C.c_int, [C.POINTER(RowsOperand), C.POINTER(RowsOperand), c_i32, c_vp, c_i64, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp,
                                 c_vp, c_i64, c_vp]),
    'dsp_rows_product': (C.c_int, [C.POINTER(RowsOperand), c_vp, C.POINTER(RowsOperand), c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    'dsp_robust_scale_fit_batch': (C.c_int, [c_vp, c_i64, c_i32, c_i32, c_vp, c_i64, c_f64, c_f64, c_i32, c_vp, c_vp, c_vp, c_vp]),
    'dsp_var_all': (C.c_int, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'dsp_svm_fit_workspace_bytes': (C.c_int, [c_i32, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_svm_fit_batch': (C.c_int, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp, c_vp, c_f64, c_i32, c_vp, c_i64,
                                    c_vp, c_vp, c_vp, c_i64, c_vp]),
    'dsp_rng_advance': (C.c_int, [c_vp, c_vp]),
    'dsp_dropout_apply': (C.c_int, [c_vp, c_vp, c_i64, c_f64, c_i32, c_vp, c_vp, c_vp]),
    'dsp_dropout_apply_key': (C.c_int, [c_vp, c_vp, c_i64, c_f64, c_i32, c_vp, c_vp]),
    'dsp_dropout_multipliers': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_f64, c_i32, c_vp, c_vp, c_vp]),
    'dsp_metrics_bytes': (C.c_int, [c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_metrics_reset': (C.c_int, [c_vp, c_i32, c_i32, c_vp]),
    'dsp_xent_metrics_batch': (C.c_int, [c_vp, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_i32,
                                         c_vp]),
    'dsp_adv_disc_work_bytes': (C.c_int, [c_i32, c_i32, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_adv_disc_forward': (C.c_int, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'dsp_adv_disc_train': (C.c_int, [c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_f64, c_vp, c_vp, c_vp,
                                     c_i64, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_vp]),
    'dsp_rows_colsum_scratch_bytes': (C.c_int, [c_i32, c_i32, c_i32, C.POINTER(c_i64)]),
    'dsp_rows_colsum': (C.c_int, [C.POINTER(RowsOperand), C.POINTER(RowsOperand), c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp]),
    'dsp_graph_census': (C.c_int, [c_vp, C.POINTER(GraphCensus), c_vp, C.c_size_t]),
}

_lib = None
_lock = threading.Lock()


class DspError(RuntimeError):
    pass


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.

    PyTorch-ROCm wheels bundle their own ``libamdhip64.so`` (SONAME ``libamdhip64.so.7``) but link
    to it under the unversioned name, so the loader does not recognise a system runtime that is
    already mapped: a process that loads this library first and imports torch later would end up
    with two HIP runtimes, and the second one finds no GPU ("No HIP GPUs are available").  When
    torch is installed but not imported yet, map ITS runtime first (without importing torch); our
    library's ``libamdhip64.so.7`` dependency then binds to it by SONAME, which is also what
    happens when torch is imported first.  ``DSP_HIP_RUNTIME=system`` keeps the system runtime.
    """
    if 'torch' in sys.modules or os.environ.get('DSP_HIP_RUNTIME', 'auto') == 'system':
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), 'lib', 'libamdhip64.so')
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError:
            pass            # fall back to whatever the dynamic loader finds


def load():
    """Load the shared library (no GPU needed for this step) and declare every signature."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise DspError(
                f'{LIB_PATH} not found: build it with `python __graft_entry__.py` (or make -C '
                f'dsp-speech-recognition_amd/csrc). There is no CPU fallback.')
        _share_hip_runtime_with_torch()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.dsp_abi_version() != 2:
            raise DspError(f'ABI version mismatch: {lib.dsp_abi_version()}')
        _lib = lib
    return _lib


def current_device():
    """HIP device current on this thread (plans and scratch buffers are per device)."""
    dev = C.c_int(-1)
    check(load().dsp_get_device(C.byref(dev)))
    return dev.value


def check(rc):
    if rc != OK:
        msg = load().dsp_last_error()
        raise DspError(f'dsp_frontend error {rc}: {msg.decode() if msg else "?"}')


def check_value(rc, what):
    """``check`` where EINVAL is the caller's value at fault: ValueError with the library's message (else ``what``)."""
    if rc == EINVAL:
        msg = load().dsp_last_error()
        raise ValueError(msg.decode() if msg else what)
    check(rc)


_device_ready = False


def require_device():
    """Fail loudly when no GPU is usable (product path has no CPU route)."""
    global _device_ready
    if _device_ready:
        return
    lib = load()
    n = C.c_int(0)
    rc = lib.dsp_device_count(C.byref(n))
    if rc != OK or n.value < 1:
        msg = lib.dsp_last_error()
        raise DspError('no MI355X/HIP device available; this package has no CPU fallback '
                       f'({msg.decode() if msg else "device count 0"})')
    _device_ready = True


def frame_count(n, L, S):
    out = c_i64(0)
    check(load().dsp_frame_count(int(n), int(L), int(S), C.byref(out)))
    return out.value


def frame_offsets(sample_offsets, L, S):
    so = np.ascontiguousarray(sample_offsets, dtype=np.int64)
    fo = np.empty_like(so)
    check(load().dsp_frame_offsets(so.ctypes.data, len(so) - 1, int(L), int(S), fo.ctypes.data))
    return fo


def frames_bound(sample_capacity, n_utt, L, S):
    """dsp_frames_bound: an upper bound on the frame count of any ``n_utt`` clips whose lengths sum to ``sample_capacity``."""
    out = c_i64(0)
    check_value(load().dsp_frames_bound(int(sample_capacity), int(n_utt), int(L), int(S), C.byref(out)), 'invalid argument')
    return out.value


class DeviceBuffer:
    """Owning handle of hipMalloc'ed memory."""

    def __init__(self, nbytes):
        require_device()
        self.nbytes = int(nbytes)
        self.wave = None            # set by VadMfccPipeline.run on a result buffer: the wave buffer it was computed from
        p = c_vp(0)
        check(load().dsp_malloc(C.byref(p), max(self.nbytes, 1)))
        self.ptr = p.value

    def upload(self, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(load().dsp_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes, stream))
        check(load().dsp_stream_synchronize(stream))  # `arr` may be a temporary
        return self

    def download(self, shape, dtype, stream=None):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes, (out.nbytes, self.nbytes)
        check(load().dsp_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, stream))
        return out

    def free(self):
        if getattr(self, 'ptr', None):
            try:
                load().dsp_free(self.ptr)
            except Exception:
                pass
            self.ptr = None

    def __del__(self):
        self.free()


class Scratch:
    """Grow-only named device buffers so single-utterance calls do not hipMalloc every time.

    Slots are PER THREAD (and per device): every drop-in call uploads, launches and downloads on its
    own thread's buffers, so concurrent callers never share a slot (ctypes releases the GIL during
    the C calls).  A slot is only ever replaced by the thread that owns it, between its own calls;
    the old buffer's hipFree waits for work still queued on it.  Results that outlive the call
    (``download=False`` paths) are never scratch slots: they are owned DeviceBuffers.
    """

    def __init__(self, alloc=None):
        self._tls = threading.local()
        self._alloc = alloc or DeviceBuffer

    def _bufs(self):
        d = getattr(self._tls, 'bufs', None)
        if d is None:
            d = self._tls.bufs = {}
        return d

    def get(self, name, nbytes, device=None):
        key = (current_device() if device is None else device, name)   # hipMalloc'ed memory belongs to one device
        bufs = self._bufs()
        b = bufs.get(key)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = self._alloc(max(int(nbytes * 1.5), 4096))
            bufs[key] = b
        return b


SCRATCH = Scratch()


def device_array(name, arr, stream=None):
    """Upload a host array into this thread's named scratch slot; returns the DeviceBuffer."""
    arr = np.ascontiguousarray(arr)
    return SCRATCH.get(name, arr.nbytes).upload(arr, stream)


def as_wave(sig):
    """Map a host signal to (contiguous array, dtype code): int16 stays int16 (reader.py:80), every
    other numeric type is rounded to fp32 (the arithmetic type of the kernels)."""
    a = np.asarray(sig)
    if a.dtype == np.int16:
        return np.ascontiguousarray(a), WAVE_I16
    return np.ascontiguousarray(a, dtype=np.float32), WAVE_F32
