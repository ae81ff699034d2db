"""ctypes binding of libnlt_hip.so (include/nlt_hip.h) + thin torch-tensor adapters.

PyTorch is plumbing here (device memory + streams): every function takes torch CUDA tensors,
checks dtype/contiguity, and hands raw device pointers and the current HIP stream to the
C ABI.  There is NO CPU or torch fallback: if the library is missing or a call returns a
non-zero status this raises.
"""
import ctypes
import struct as _struct
import threading
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NLT_HIP_LIB') or os.path.join(_HERE, 'libnlt_hip.so')   # NLT_HIP_LIB: A/B of two builds (tools/ab_front.py)

CONV1X1, CONV_K2S2, CONV_K2S1, DECONV_K2S2, DECONV_K2S1 = range(5)
CONV_K3S1, CONV_K3S2, DECONV_K3S1, DECONV_K3S2 = range(5, 9)       # kernel = 3: the nlt_conv_k3_* entry points only
ALGO_AUTO, ALGO_DIRECT, ALGO_MFMA = range(3)

_c_int, _c_long, _c_float, _vp = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p
_c_double = ctypes.c_double
MAP_F64, MAP_F32, MAP_F16 = range(3)

# name -> (restype, argtypes); must list every symbol include/nlt_hip.h declares
SIGNATURES = {
    'nlt_version': (ctypes.c_char_p, []),
    'nlt_status_string': (ctypes.c_char_p, [_c_int]),
    'nlt_packed_weight_floats': (_c_long, [_c_int] * 4),
    'nlt_pack_conv_weights': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_conv_forward': (_c_int, [_c_int, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _c_int, _c_int,
                                  _c_int, _c_int, _c_int, _vp, _vp, _vp, _c_int, _vp, _c_int,
                                  _c_int, _c_float, _vp, _c_int, _c_int, _vp]),
    'nlt_stem_forward': (_c_int, [_vp] * 6 + [_c_int] * 5 + [_vp] * 4 + [_vp, _vp, _vp]),
    'nlt_obs_mean_forward': (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _vp]),
    'nlt_head_forward': (_c_int, [_vp, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _vp, _vp,
                                  _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_warp_forward': (_c_int, [_vp, _vp, _vp] + [_c_int] * 5 + [_vp] * 5),
    'nlt_warp_forward_store': (_c_int, [_vp] * 4 + [_c_int] * 5 + [_vp] * 5),
    'nlt_resample_forward': (_c_int, [_vp, _vp] + [_c_int] * 6 + [_vp, _vp]),
    'nlt_resize_bilinear_forward': (_c_int, [_vp] + [_c_int] * 6 + [_vp, _vp]),
    'nlt_mul_forward': (_c_int, [_vp, _vp, _c_long, _vp, _vp]),
    'nlt_conv_backward_weights': (_c_int, [_c_int, _c_int, _vp, _c_int, _c_int, _vp, _c_int, _c_int,
                                           _c_int, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _vp, _vp]),
    'nlt_wgrad_workspace_floats': (_c_long, [_c_int] * 7),
    'nlt_conv_backward_weights_tiled': (_c_int, [_c_int, _vp, _c_int, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                                                 _vp, _c_int, _c_int, _vp, _vp, _vp, _c_long, _vp]),
    'nlt_repack_weights': (_c_int, [_vp, _c_int, _c_long, _vp]),
    'nlt_tape_play': (_c_int, [_vp, _c_int, _vp]),
    'nlt_event_create': (_c_int, [_c_int, _vp]),
    'nlt_event_destroy': (_c_int, [_vp]),
    'nlt_event_record': (_c_int, [_vp, _vp]),
    'nlt_stream_wait_event': (_c_int, [_vp, _vp]),
    'nlt_wgrad_narrow_workspace_floats': (_c_long, [_c_int] * 7),
    'nlt_conv_backward_weights_narrow': (_c_int, [_c_int, _vp, _c_int, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int,
                                                 _vp, _c_int, _c_int, _vp, _vp, _vp, _c_long, _vp]),
    'nlt_lrelu_backward': (_c_int, [_vp, _c_int, _vp, _c_int, _c_int, _c_long, _c_float, _vp, _c_int, _vp]),
    'nlt_obs_mean_backward': (_c_int, [_vp, _c_int, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _vp, _vp]),
    'nlt_resize_cv_linear': (_c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_l2_train_loss': (_c_int, [_vp, _vp, _vp, _c_int, _c_long, _c_float, _vp, _vp, _vp, _vp]),
    'nlt_level_split_backward': (_c_int, [_vp, _vp, _c_int, _vp, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _c_float, _vp, _vp]),
    'nlt_stem_backward': (_c_int, [_vp] * 6 + [_c_int] * 5 + [_vp] * 6 + [_vp]),
    'nlt_head_backward': (_c_int, [_vp, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _vp, _c_int, _c_int, _c_int,
                                   _vp, _c_int, _vp, _c_int, _vp, _vp, _vp]),
    'nlt_warp_backward': (_c_int, [_vp, _vp] + [_c_int] * 5 + [_vp, _vp]),
    'nlt_resize_bilinear_backward': (_c_int, [_vp] + [_c_int] * 6 + [_vp, _vp]),
    'nlt_l2_loss_forward': (_c_int, [_vp, _vp, _c_int, _c_long, _vp, _vp]),
    'nlt_l2_loss_backward': (_c_int, [_vp, _vp, _vp, _c_int, _c_long, _vp, _vp]),
    'nlt_l2_loss_weighted_forward': (_c_int, [_vp, _vp, _vp, _c_int, _c_long, _c_int, _vp, _vp]),
    'nlt_l2_loss_weighted_backward': (_c_int, [_vp, _vp, _vp, _vp, _c_int, _c_long, _c_int, _vp, _vp]),
    'nlt_barron_workspace_floats': (_c_long, [_c_int] * 3),
    'nlt_barron_loss': (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp]),
    'nlt_scale_rows': (_c_int, [_vp, _vp, _c_int, _c_long, _vp, _vp]),
    'nlt_ssim_workspace_floats': (_c_long, [_c_int] * 5),
    'nlt_ssim_loss': (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _vp, _c_long, _vp, _vp, _vp]),
    'nlt_ssim_values': (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _vp, _c_long, _vp, _vp]),
    'nlt_lpips_conv1_forward': (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp]),
    'nlt_lpips_conv1_backward_data': (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp]),
    'nlt_lpips_conv2_forward': (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp]),
    'nlt_lpips_conv2_backward_data': (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _vp, _vp]),
    'nlt_lpips_pool_forward': (_c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_lpips_pool_backward': (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_lpips_head_workspace_floats': (_c_long, [_c_int, _c_long]),
    'nlt_lpips_head_forward': (_c_int, [_vp, _vp, _c_int, _c_long, _c_int, _vp, _vp, _c_long, _vp, _vp]),
    'nlt_lpips_head_backward': (_c_int, [_vp, _vp, _c_int, _c_long, _c_int, _vp, _vp, _vp, _vp]),
    'nlt_lpips_weights_floats': (_c_long, []),
    'nlt_lpips_workspace_floats': (_c_long, [_c_int] * 4),
    'nlt_lpips_loss': (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _vp, _vp, _c_long, _vp, _vp, _vp]),
    'nlt_sub_forward': (_c_int, [_vp, _vp, _c_long, _vp, _vp]),
    'nlt_finish_pred': (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_act_forward': (_c_int, [_vp, _c_long, _c_int, _c_float, _vp, _vp]),
    'nlt_act_backward': (_c_int, [_vp, _vp, _c_long, _c_int, _c_float, _vp, _vp]),
    'nlt_pixelnorm_forward': (_c_int, [_vp, _c_long, _c_int, _c_float, _vp, _vp]),
    'nlt_pixelnorm_backward': (_c_int, [_vp, _vp, _c_long, _c_int, _c_float, _vp, _vp]),
    'nlt_pool2x2_forward': (_c_int, [_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_pool2x2_backward': (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_norm_workspace_floats': (_c_long, [_c_long, _c_int]),
    'nlt_norm_forward': (_c_int, [_c_int, _vp, _c_long, _c_int, _vp, _vp, _vp, _vp, _c_float, _vp, _vp]),
    'nlt_norm_backward': (_c_int, [_c_int, _vp, _vp, _c_long, _c_int, _vp, _vp, _vp, _c_float, _vp, _vp, _vp, _vp, _vp]),
    'nlt_clip_by_norm_slots': (_c_int, [_vp, _vp, _c_int, _c_float, _vp]),
    'nlt_adam_amsgrad_step': (_c_int, [_vp] * 5 + [_c_long] + [_c_float] * 4 + [_vp]),
    'nlt_front_packed_floats': (_c_long, []),
    'nlt_front_pack_weights': (_c_int, [_vp] * 15 + [_vp]),
    'nlt_front_forward': (_c_int, [_vp] * 5 + [_c_int] * 4 + [_vp, _c_int, _c_float, _vp, _vp, _vp, _vp]),
    'nlt_front_l2_packed_floats': (_c_long, []),
    'nlt_front_pack_l2_weights': (_c_int, [_vp] * 5 + [_vp]),
    'nlt_front2_forward': (_c_int, [_vp] * 5 + [_c_int] * 4 + [_vp, _vp, _c_int, _c_float, _vp, _vp, _vp, _vp, _vp]),
    'nlt_front4_forward': (_c_int, [_vp] * 5 + [_c_int] * 4 + [_vp, _vp, _c_int, _c_float, _vp, _vp, _vp, _vp, _c_int, _vp]),
    'nlt_front4_forward_u8': (_c_int, [_vp] * 6 + [_c_int] * 4 + [_vp, _vp, _c_int, _c_float, _vp, _vp, _vp, _vp, _c_int, _vp]),
    'nlt_front4_forward_train': (_c_int, [_vp] * 5 + [_c_int] * 4 + [_vp, _vp, _c_int, _c_float] + [_vp] * 7 + [_vp]),
    'nlt_dec_block_forward': (_c_int, [_vp, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_int, _c_float, _vp, _vp]),
    'nlt_back_forward': (_c_int, [_vp] * 3 + [_c_int] * 3 + [_vp] * 5 + [_c_float, _vp, _vp]),
    'nlt_front_forward_train': (_c_int, [_vp] * 5 + [_c_int] * 4 + [_vp, _c_int, _c_float] + [_vp] * 6),
    'nlt_back_forward_train': (_c_int, [_vp] * 3 + [_c_int] * 3 + [_vp] * 5 + [_c_float] + [_vp] * 4),
    'nlt_front_backward_workspace_floats': (_c_long, [_c_int] * 3),
    'nlt_front_backward': (_c_int, [_vp] * 5 + [_c_int] * 4 + [_vp] * 21),
    'nlt_back_backward_workspace_floats': (_c_long, [_c_int] * 3),
    'nlt_back_backward': (_c_int, [_vp] * 5 + [_c_int] * 3 + [_vp] * 3 + [_c_float] + [_vp] * 10),
    'nlt_conv_splitk_workspace_floats': (_c_long, [_c_int] * 6),
    'nlt_conv_forward_splitk': (_c_int, [_c_int, _c_int, _c_int, _vp, _vp, _c_int, _c_int, _vp, _c_int, _c_int,
                                         _c_int, _c_int, _c_int, _vp, _vp, _c_int, _vp, _c_int, _c_int, _c_float,
                                         _vp, _c_int, _c_int, _vp]),
    'nlt_conv_forward_map': (_c_int, [_c_int, _c_int, _c_int, _vp, _vp, _c_int, _c_int, _vp, _c_int, _c_int,
                                      _c_int, _c_int, _c_int, _vp, _vp, _c_int, _vp, _c_int, _c_int, _c_float,
                                      _vp, _c_int, _vp]),
    'nlt_dec_block_forward_map': (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _vp, _c_int, _c_float, _vp, _vp, _vp]),
    'nlt_back_forward_map': (_c_int, [_vp, _vp, _c_int, _vp, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_float, _vp, _vp, _vp]),
    'nlt_front_ovr_forward': (_c_int, [_vp] * 3 + [_c_int] * 3 + [_vp] * 5 + [_c_int, _c_float, _vp, _c_int, _vp, _vp, _vp]),
    'nlt_front_ovr_forward_u8': (_c_int, [_vp] * 4 + [_c_int] * 3 + [_vp] * 5 + [_c_int, _c_float, _vp, _c_int, _vp, _vp, _vp]),
    # extract_feat (csrc/front_obs.hip): the observation-only front launch, the frame sums and their finishing launches
    'nlt_front_obs_forward': (_c_int, [_vp, _vp] + [_c_int] * 3 + [_vp, _vp, _c_float, _c_int] + [_vp] * 3 + [_vp]),
    'nlt_front_obs_forward_u8': (_c_int, [_vp] * 3 + [_c_int] * 3 + [_vp, _vp, _c_float, _c_int] + [_vp] * 3 + [_vp]),
    'nlt_frame_sum_accumulate': (_c_int, [_vp, _c_int, _c_long, _vp, _c_int, _vp]),
    'nlt_frame_mean_finish': (_c_int, [_vp, _c_long, _c_long, _vp, _vp]),
    'nlt_frame_mean_finish_l0': (_c_int, [_vp, _c_long, _c_long, _vp, _vp, _vp, _vp]),
    'nlt_conv_backward_data': (_c_int, [_c_int, _c_int, _c_int, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_int,
                                        _vp, _c_int, _vp, _c_int, _c_float, _c_int, _c_int, _vp, _vp, _c_float, _c_int, _vp]),
    'nlt_conv_tile_packed_floats': (_c_long, [_c_int] * 4),
    'nlt_pack_conv_tile_weights': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_conv_tile_forward': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_int, _c_int,
                                       _vp, _c_int, _vp, _c_int, _c_int, _c_float, _vp]),
    'nlt_pack_conv_tile_weights_adjoint': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_conv_c32_supported': (_c_int, [_c_int] * 3),
    'nlt_conv_c32_forward': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_int,
                                      _vp, _c_int, _vp, _c_int, _c_int, _c_float, _vp]),
    'nlt_conv_wino_packed_floats': (_c_long, [_c_int] * 4),
    'nlt_pack_conv_wino_weights': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_conv_wino_forward': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_int, _c_int,
                                       _vp, _c_int, _vp, _c_int, _c_int, _c_float, _vp]),
    'nlt_pack_conv_wino_weights_adjoint': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_conv_wino_backward_data': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _c_int,
                                             _vp, _c_int, _c_float, _c_int, _vp]),
    'nlt_conv_tile_backward_data': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _c_int,
                                             _vp, _c_int, _c_float, _c_int, _c_int, _vp, _vp, _c_float, _c_int, _vp]),
    'nlt_conv_tile3_packed_elems': (_c_long, [_c_int] * 4),
    'nlt_pack_conv_tile3_weights': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_conv_tile3_forward': (_c_int, [_c_int, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_int, _c_int,
                                        _vp, _c_int, _vp, _c_int, _c_int, _c_float, _vp]),
    'nlt_conv_tile3r_forward': (_c_int, [_c_int, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_int, _c_int,
                                         _vp, _c_int, _vp, _c_int, _c_int, _c_float, _c_int, _vp]),
    'nlt_conv_tile3d_forward': (_c_int, [_c_int, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_int, _c_int,
                                         _vp, _c_int, _vp, _c_int, _c_int, _c_float, _vp]),
    'nlt_conv_tile3w_s2_packed_elems': (_c_long, [_c_int] * 2),
    'nlt_pack_conv_tile3w_s2_weights': (_c_int, [_vp, _c_int, _c_int, _vp, _vp]),
    'nlt_conv_tile3w_s2_lds_bytes': (_c_long, [_c_int] * 3),
    'nlt_conv_tile3w_s2_forward': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_int, _vp, _c_int,
                                            _vp, _c_int, _c_int, _c_float, _vp, _vp, _c_int, _vp, _c_int, _c_int, _c_float, _c_int, _vp]),
    'nlt_conv_bf16_packed_elems': (_c_long, [_c_int] * 4),
    'nlt_conv_bf16_pack': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_conv_bf16_forward': (_c_int, [_c_int, _c_int, _vp, _c_int, _c_int, _c_int, _vp, _c_int, _c_int, _c_int,
                                       _c_int, _c_int, _c_int, _vp, _vp, _c_int, _vp, _c_int, _c_int, _c_int, _c_float, _vp]),
    'nlt_conv_bf16_forward_map': (_c_int, [_c_int, _c_int, _vp, _c_int, _c_int, _c_int, _vp, _c_int, _c_int, _c_int,
                                           _c_int, _c_int, _c_int, _vp, _vp, _c_int, _vp, _c_int, _c_int, _c_int, _c_float,
                                           _vp, _c_int, _vp]),
    'nlt_obs_mean_bf16': (_c_int, [_vp, _c_int, _c_int, _c_long, _c_int, _vp, _c_int, _vp]),
    'nlt_chmix_bf16_packed_elems': (_c_long, [_c_int, _c_int]),
    'nlt_chmix_bf16_pack': (_c_int, [_vp, _c_int, _c_int, _vp, _vp]),
    'nlt_chmix_bf16_forward': (_c_int, [_vp, _c_long, _c_int, _vp, _vp, _c_int, _c_int, _c_float, _vp, _vp]),
    'nlt_cosine_map': (_c_int, [_vp] * 4 + [_c_double] * 3 + [_c_long, _vp, _vp, _vp]),
    'nlt_albedo': (_c_int, [_vp, _c_int, _c_long, _vp, _vp, _vp]),
    'nlt_diffuse_base': (_c_int, [_vp, _vp, _c_int, _c_long, _vp, _vp]),
    'nlt_remap_bilinear_u8': (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_remap_bilinear_f32': (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_capture_camspc': (_c_int, [_vp] * 4 + [_c_double] * 6 + [_vp, _vp, _c_int, _c_int] + [_vp] * 5),
    'nlt_capture_uvspc': (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _vp, _vp, _c_int, _c_int, _c_int] + [_vp] * 6),
    'nlt_diffuse_bases': (_c_int, [_vp, _vp, _vp] + [_c_int] * 5 + [_vp, _vp, _vp]),
    'nlt_uv_index_map_workspace_bytes': (_c_long, [_c_int, _c_int, _c_long]),
    'nlt_uv_index_map': (_c_int, [_vp, _vp, _c_long, _c_int, _c_int, _c_int, _c_int, _c_double, _vp, _vp, _vp, _vp]),
    'nlt_knn_indices': (_c_int, [_vp, _c_int, _vp, _c_int, _c_int, _vp, _vp]),
    'nlt_psnr_sums': (_c_int, [_vp, _vp, _vp, _c_long, _c_int, _vp, _vp, _vp]),
    'nlt_gather_frames_u8': (_c_int, [_vp, _vp, _c_int, _c_long, _vp, _vp]),
    'nlt_assemble_batch': (_c_int, [_vp] * 6 + [_c_int, _c_int, _c_long, _c_int] + [_vp] * 6 + [_vp]),
    # deterministic mode (csrc/deterministic.hip and the owning files): atomic-free siblings, caller-supplied workspaces
    'nlt_warp_backward_det_workspace_bytes': (_c_long, [_c_int] * 5),
    'nlt_warp_backward_det': (_c_int, [_vp, _vp] + [_c_int] * 5 + [_vp, _vp, _c_long, _vp]),
    'nlt_resize_bilinear_backward_gather': (_c_int, [_vp] + [_c_int] * 6 + [_vp, _vp]),
    'nlt_loss_det_workspace_floats': (_c_long, [_c_int]),
    'nlt_l2_loss_forward_det': (_c_int, [_vp, _vp, _c_int, _c_long, _vp, _vp, _c_long, _vp]),
    'nlt_l2_loss_weighted_forward_det': (_c_int, [_vp, _vp, _vp, _c_int, _c_long, _c_int, _vp, _vp, _c_long, _vp]),
    'nlt_l2_train_loss_det': (_c_int, [_vp, _vp, _vp, _c_int, _c_long, _c_float, _vp, _vp, _vp, _vp, _c_long, _vp]),
    'nlt_barron_det_slots_floats': (_c_long, [_c_int] * 3),
    'nlt_barron_loss_det': (_c_int, [_vp, _vp, _c_int, _c_int, _c_int, _vp, _vp, _vp, _vp, _c_long, _vp]),
    'nlt_stem_backward_det_workspace_floats': (_c_long, [_c_int] * 4),
    'nlt_stem_backward_det': (_c_int, [_vp] * 6 + [_c_int] * 5 + [_vp] * 6 + [_vp, _c_long, _vp]),
    'nlt_head_backward_det_workspace_floats': (_c_long, [_c_int] * 5),
    'nlt_head_backward_det': (_c_int, [_vp, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _vp, _c_int, _c_int, _c_int,
                                       _vp, _c_int, _vp, _c_int, _vp, _vp, _vp, _c_long, _vp]),
    'nlt_conv_backward_weights_det_workspace_floats': (_c_long, [_c_int] * 7),
    'nlt_conv_backward_weights_det': (_c_int, [_c_int, _c_int, _vp, _c_int, _c_int, _vp, _c_int, _c_int,
                                               _c_int, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _vp, _vp, _c_long, _vp]),
    # kernel = 3 (csrc/conv_k3.hip)
    'nlt_conv_k3_forward': (_c_int, [_c_int, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _vp, _vp, _c_int, _vp, _c_int, _c_float, _vp]),
    'nlt_conv_k3_backward_data': (_c_int, [_c_int, _c_int, _vp, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _vp, _vp]),
    'nlt_conv_k3_wgrad_workspace_floats': (_c_long, [_c_int] * 6),
    'nlt_conv_k3_backward_weights': (_c_int, [_c_int, _vp, _c_int, _c_int, _c_int, _c_int, _vp, _c_int, _vp, _vp, _vp, _c_long, _vp]),
    # relighting under an environment map (csrc/relight.hip)
    'nlt_envmap_light_weights_workspace_floats': (_c_long, [_c_int] * 4),
    'nlt_envmap_light_weights': (_c_int, [_vp, _c_int, _c_int, _vp, _c_int, _vp, _c_int, _vp, _c_long, _vp, _vp]),
    'nlt_relight_accumulate': (_c_int, [_vp, _c_int, _c_long, _vp, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    'nlt_relight_finish': (_c_int, [_vp, _c_int, _c_long, _c_float, _c_int, _vp, _vp]),
    # mesh ray casting (csrc/raycast.hip)
    'nlt_bvh_tris_doubles': (_c_long, [_c_long]),
    'nlt_bvh_nodes_doubles': (_c_long, [_c_long]),
    'nlt_bvh_morton': (_c_int, [_vp, _c_long] + [_c_double] * 6 + [_vp, _vp]),
    'nlt_bvh_build': (_c_int, [_vp, _vp, _c_long, _vp, _c_long, _vp, _c_long, _vp]),
    'nlt_raycast': (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp, _c_long, _vp, _vp, _vp, _vp]),
    'nlt_raycast_camera': (_c_int, [_vp, _vp, _c_long, _vp, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp]),
    'nlt_raycast_shadow': (_c_int, [_vp, _vp, _c_long, _vp, _vp, _c_long] + [_c_double] * 3 + [_vp, _vp]),
    'nlt_render_direct': (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp, _c_int, _c_int, _c_int] + [_c_double] * 9 + [_vp, _vp, _vp]),
    'nlt_render_global': (_c_int, [_vp, _vp, _c_long, _vp, _vp, _vp, _c_int, _c_int, _c_int] + [_c_double] * 10 +
                          [_vp, _c_int, _c_int, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp]),
    # UV unwrap (csrc/unwrap.hip)
    'nlt_unwrap_workspace_bytes': (_c_long, [_c_long]),
    'nlt_unwrap_frames': (_c_int, [_vp, _c_long, _vp, _c_long, _vp, _c_long, _vp, _vp, _vp, _vp, _vp]),
    'nlt_unwrap_seed': (_c_int, [_vp, _vp, _c_long, _vp, _vp, _c_long, _vp, _vp]),
    'nlt_unwrap_gather': (_c_int, [_vp, _vp, _vp, _c_long, _c_long] + [_c_double] * 3 + [_vp, _c_long, _vp, _vp]),
    'nlt_unwrap_farthest': (_c_int, [_vp, _vp, _vp, _vp, _c_long, _vp, _c_int, _vp, _c_long, _vp, _vp]),
    'nlt_unwrap_assign': (_c_int, [_vp, _vp, _c_long, _vp, _c_int, _vp, _vp]),
    'nlt_unwrap_edge_keys': (_c_int, [_vp, _c_long, _vp, _c_long, _c_long, _vp, _vp, _vp]),
    'nlt_unwrap_islands_init': (_c_int, [_vp, _c_long, _vp, _vp]),
    'nlt_unwrap_islands_round': (_c_int, [_vp, _vp, _vp, _c_long, _vp, _c_long, _vp, _vp, _vp]),
    'nlt_unwrap_boxes': (_c_int, [_vp, _vp, _vp, _c_long, _vp, _vp, _c_long, _vp, _c_int, _vp, _vp, _c_long, _vp]),
    'nlt_unwrap_uv': (_c_int, [_vp, _c_long, _vp, _vp, _c_long, _vp, _vp, _vp, _c_long, _c_double, _c_int, _vp, _vp]),
}

_real = None


def _load():
    """Loads libnlt_hip.so once; raises (loudly) when it has not been built."""
    global _real
    if _real is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libnlt_hip.so not found at %s -- build it with `python __graft_entry__.py` or "
                "`make -C neural-light-transport_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _real = L
    return _real


# ---------------------------------------------------------------- launch tape
# A plan (engine.RenderPlan) issues the same ~40 (forward) / ~130 (backward) C calls with the same arguments every
# step: same buffers, same weights, same streams.  Deriving those arguments again in Python (tensor -> pointer, layout
# checks, fragment-cache lookups, .detach() views) costs ~15-20 us per launch -- as much wall time as the GPU needs for
# the whole step at the training shape.  While a tape is open every launching C call is ALSO appended to it as
# (function, resolved arguments); a later step with the same inputs replays the list with nothing but the ctypes
# calls.  (hipGraph replay of the same sequence measured slower than eager launches on ROCm 7.0; see DESIGN.md.)
# The open tape belongs to the THREAD that opened it (pipeline.RenderPipeline drives one lane per host thread: a lane that
# records must not collect another lane's launches).
_tls = threading.local()
_alloc_epoch = [0]          # bumped whenever a cached device buffer the C calls point into is re-allocated

# int-returning entry points that answer a question instead of launching: a 0 from them is "no", not "launched"
_NOT_LAUNCHES = frozenset(('nlt_conv_c32_supported',))


class _TapeLib:
    """Stand-in for the CDLL while a tape is open: launching entry points (int status) are recorded after they ran."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if SIGNATURES[name][0] is not _c_int or name in _NOT_LAUNCHES:
            return fn                                   # size / capability queries: pure, not part of the step

        def recorded(*args):
            rc = fn(*args)
            t = getattr(_tls, 'tape', None)
            if t is not None and rc == 0:
                t.append((fn, args))
            return rc
        setattr(self, name, recorded)
        return recorded


_tape_lib = None


def lib():
    global _tape_lib
    if getattr(_tls, 'tape', None) is None:
        return _real if _real is not None else _load()
    if _tape_lib is None:
        _tape_lib = _TapeLib(_load())
    return _tape_lib


def tape_begin():
    if getattr(_tls, 'tape', None) is not None:
        raise NLTError("a launch tape is already open")
    _tls.tape = []
    _tls.epoch = _alloc_epoch[0]


def tape_end(tag=None, extra=None):
    """Closes the tape and returns [launch list, allocation epoch it is valid for, caller's validity tag, native form, extra]
    (`extra`: whatever the recorder wants back at replay time -- engine.py keeps the packed-buffer keys the tape reads)."""
    t, _tls.tape = _tls.tape, None
    if _tls.epoch != _alloc_epoch[0]:
        return None                                     # a cached buffer was re-allocated while recording: pointers are stale
    return (t, _alloc_epoch[0], tag, [None], extra)


def tape_abort():
    _tls.tape = None


def tape_pause():
    """Takes the open tape (if any) away for a launch that must NOT be recorded (its arguments change from step to step);
    hand the return value back to `tape_resume`."""
    t = getattr(_tls, 'tape', None)
    _tls.tape = None
    return t


def tape_resume(t):
    _tls.tape = t


def tape_valid(tape, tag=None):
    return tape is not None and tape[1] == _alloc_epoch[0] and tape[2] == tag


# Native replay (csrc/tape.hip: nlt_tape_play): the recorded calls of a tape, compiled once into arrays of nlt_tape_call and walked
# by ONE C call per run of consecutive native entries; what cannot be expressed (a Python hook, an entry with double arguments)
# stays a Python step between two runs.  OPT-IN (NLT_NATIVE_REPLAY=1): measured on MI355X boxes it changes nothing -- host enqueue
# 1.55 -> 1.52 ms per train step at config 4, 1.51 -> 1.48 at the 512^2 shape (r03): the ~9 us per launch are the HIP runtime's own
# (launch + the second-stream event traffic), not ctypes', and the steps are not host-bound to begin with.
NATIVE_REPLAY = os.environ.get('NLT_NATIVE_REPLAY', '0') != '0'


class _TapeCall(ctypes.Structure):
    _fields_ = [('fn', ctypes.c_void_p), ('n_float', ctypes.c_int), ('reserved', ctypes.c_int), ('iargs', ctypes.c_long * 32),
                ('fargs', ctypes.c_float * 4)]


def _describe(fn, args):
    """(address, integer-class args, float args) of one recorded step, or None when it has to stay a Python call."""
    owner = getattr(fn, '__self__', None)
    if owner is not None:                               # bound methods recorded by record_event / wait_event
        name = getattr(fn, '__name__', '')
        if isinstance(owner, torch.cuda.Event) and name == 'record' and len(args) == 1:
            return (ctypes.cast(_real.nlt_event_record, ctypes.c_void_p).value, [owner.cuda_event, args[0].cuda_stream], [])
        if isinstance(owner, torch.cuda.Stream) and name == 'wait_event' and len(args) == 1:
            return (ctypes.cast(_real.nlt_stream_wait_event, ctypes.c_void_p).value, [owner.cuda_stream, args[0].cuda_event], [])
        return None
    at = getattr(fn, 'argtypes', None)
    if at is None or len(at) != len(args):
        return None
    ia, fa = [], []
    for t, a in zip(at, args):
        if t is _c_float:
            fa.append(float(a))
        elif t in (_c_int, _c_long, _vp):
            ia.append(0 if a is None else int(a))
        else:
            return None                                 # doubles, char pointers: not a launching entry of a plan
    if len(ia) > 32 or len(fa) > 4:
        return None
    return (ctypes.cast(fn, ctypes.c_void_p).value, ia, fa)


def _compile(calls):
    """[('native', array, count) | ('py', fn, args)] in order."""
    segs, run = [], []

    def flush():
        if run:
            arr = (_TapeCall * len(run))()
            for i, (addr, ia, fa) in enumerate(run):
                arr[i].fn, arr[i].n_float = addr, len(fa)
                for j, v in enumerate(ia):
                    arr[i].iargs[j] = v
                for j, v in enumerate(fa):
                    arr[i].fargs[j] = v
            segs.append(('native', arr, len(run)))
            del run[:]
    for fn, args in calls:
        d = _describe(fn, args)
        if d is None or not d[0]:
            flush()
            segs.append(('py', fn, args))
        else:
            run.append(d)
    flush()
    return segs


def replay(tape):
    if (NATIVE_REPLAY or getattr(_tls, 'native_replay', False)) and len(tape) > 3 and _real is not None:
        box = tape[3]
        if box[0] is None:
            box[0] = _compile(tape[0])
        failed = ctypes.c_int(-1)
        for seg in box[0]:
            if seg[0] == 'native':
                rc = _real.nlt_tape_play(seg[1], seg[2], ctypes.byref(failed))
                if rc:
                    raise NLTError("replayed launch %d failed: %s" % (failed.value, _real.nlt_status_string(rc).decode()))
            else:
                rc = seg[1](*seg[2])
                if rc:
                    raise NLTError("replayed launch failed: %s" % lib().nlt_status_string(rc).decode())
        return
    for fn, args in tape[0]:
        rc = fn(*args)
        if rc:                                          # event helpers return None
            raise NLTError("replayed launch failed: %s" % lib().nlt_status_string(rc).decode())


def tape_call(fn, *args):
    """A host-side step that belongs to the plan (a hook): run it now and, while a tape is open, on every replay."""
    fn(*args)
    t = getattr(_tls, 'tape', None)
    if t is not None:
        t.append((fn, args))


class LightEvent:
    """A HIP event for ordering two streams of one device: no timing, no system-scope fence at the record (csrc/tape.hip).  Record
    and wait go through the C ABI, so an open launch tape picks them up like any launch (and replays them natively)."""

    def __init__(self):
        h = ctypes.c_void_p()
        _check(_load().nlt_event_create(1, ctypes.byref(h)), 'nlt_event_create')     # (no stream: an event belongs to the device)
        self.handle = h.value

    def __del__(self):
        try:
            if self.handle and _real is not None:
                _real.nlt_event_destroy(self.handle)
        except Exception:
            pass


LIGHT_EVENTS = None         # None: decide per event (below); True / False: forced (tests, the bench's A/B leg)


def light_events_enabled():
    """Events WITHOUT a system-scope fence at the record (csrc/tape.hip) order the plan's device-to-device hand-overs; the
    kernels' own agent-scope release / acquire orders the data.  In a multi-rank process group one of those hand-overs feeds the
    side-stream RCCL all-reduce of a gradient range, whose peers read the bucket over xGMI: until that has been A/B-tested
    on real multi-GPU hardware (bench.py's `light_events_ab` leg does it, bitwise) the default at world > 1 is the FENCED event
    (advisor r04 / review r05).  NLT_LIGHT_EVENTS=0 / 1 forces either."""
    if LIGHT_EVENTS is not None:
        return bool(LIGHT_EVENTS)
    e = os.environ.get('NLT_LIGHT_EVENTS')
    if e is not None:
        return e != '0'
    try:
        import torch.distributed as dist
        return not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
    except Exception:
        return True


def new_event():
    """Event for the plan's cross-stream hand-overs (`light_events_enabled`; otherwise an ordinary torch.cuda.Event)."""
    return LightEvent() if light_events_enabled() else torch.cuda.Event()


def record_event(ev, stream):
    if isinstance(ev, LightEvent):
        _check(lib().nlt_event_record(ev.handle, stream.cuda_stream), 'nlt_event_record')     # (the caller's stream, not the current one)
        return
    ev.record(stream)
    t = getattr(_tls, 'tape', None)
    if t is not None:
        t.append((ev.record, (stream,)))


def wait_event(stream, ev):
    if isinstance(ev, LightEvent):
        _check(lib().nlt_stream_wait_event(stream.cuda_stream, ev.handle), 'nlt_stream_wait_event')     # (the stream comes first)
        return
    stream.wait_event(ev)
    t = getattr(_tls, 'tape', None)
    if t is not None:
        t.append((stream.wait_event, (ev,)))


_WS_SCOPE = os.environ.get('NLT_WS_SCOPE', '1') != '0'      # (A/B switch)


def set_workspace_scope(token):
    """Scratch that is cached per stream (the split-K partial sums) is additionally keyed by this token; a plan sets it to its
    own identity on entry.  Two plans whose launches are CAPTURED on the same capture stream (pipeline.RenderPipeline lanes
    replaying hipGraphs) would otherwise bake one workspace into both graphs and race on it when the graphs replay side by side."""
    _tls.scope = token if _WS_SCOPE else 0


def drop_workspace_scope(token):
    """Forgets the scratch cached for a plan that is gone (RenderPlan.__del__: the lanes of a closed pipeline)."""
    for key in [k for k in _ws_cache if len(k) > 2 and k[2] == token]:      # (device, stream, token): the split-K keys of `_workspace`
        del _ws_cache[key]


def set_thread_native_replay(on):
    """This host thread replays its launch tapes through nlt_tape_play (one C call per run of launches, the interpreter lock
    released for all of it): what lets the lanes of pipeline.RenderPipeline enqueue in parallel."""
    _tls.native_replay = bool(on)


class NLTError(RuntimeError):
    pass


def _check(status, what):
    if status != 0:
        raise NLTError("%s failed: %s (%d)" % (what, lib().nlt_status_string(status).decode(), status))


def _ptr(t):
    if t is None:
        return None
    if not (t.is_cuda and t.dtype in (torch.float32, torch.int32)):
        raise NLTError("expected a float32/int32 CUDA tensor, got %s on %s" % (t.dtype, t.device))
    return t.data_ptr()


def _tptr(t, dtype, what):
    """Device pointer of a contiguous CUDA tensor of exactly `dtype` (None passes through)."""
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise NLTError("%s: expected a contiguous %s CUDA tensor, got %s on %s" % (what, dtype, t.dtype, t.device))
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dense(t, what):
    if not t.is_contiguous():
        raise NLTError("%s must be contiguous" % what)
    return t


def dense_obs_weights(obs_weights, n, k, device):
    """The `obs_weights` argument of Model.call / _call / RenderPlan.forward / backward / generic.forward as the kernels read it:
    a dense float32 [n, k] array on `device`, element (frame, observation) at f * k + i.  The reference takes whatever
    `tf.reshape(obs_weights, (N, 1, 1, 1, -1))` takes and broadcasts against the [N, H, W, C, k] stack (nlt.py:143-145,162-163):
    shape[0] == N and N * k elements.  None passes through; a strided view (a slice of a wider tensor, a transposed storage) is
    copied dense; anything else raises ValueError before any launch -- the kernels would read it at the wrong places or past
    its end."""
    if obs_weights is None:
        return None
    t = obs_weights
    ok = (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == torch.device(device) and t.dim() >= 1
          and t.shape[0] == n and t.numel() == n * k)
    if not ok:
        got = ("a %s of shape %s, dtype %s on %s" % (type(t).__name__, tuple(t.shape), t.dtype, t.device) if torch.is_tensor(t)
               else "a %s" % type(t).__name__)
        raise ValueError("obs_weights must be a float32 tensor on %s with shape[0] == %d frames and %d x %d elements "
                         "(one factor per frame and observation), got %s" % (torch.device(device), n, n, k, got))
    return t.detach().reshape(n, k).contiguous()


def _call(name, *args):
    """Launches entry point `name` with `args` + the current stream; a non-zero status raises NLTError under that name.  (Looked up
    on `lib()`, so an open tape records the call.)"""
    _check(getattr(lib(), name)(*args, _stream()), name)


def _size(name, *args, what=None):
    """Answer of a `*_workspace_floats` / `*_workspace_bytes` / `*_packed_floats` / `*_packed_elems` query; <= 0 ("these shapes are
    not implemented") raises NLTError with the query and its arguments."""
    n = getattr(lib(), name)(*args)                     # (a query: no stream, never taped)
    if n <= 0:
        raise NLTError("%s%r: unsupported%s" % (name, args, ' (%s)' % what if what else ''))
    return n


_ws_cache = {}
_splitk_ws = _ws_cache      # (the split-K entries are this cache's 3-tuples; the host bookkeeping test reaches them under this name)


def _workspace(key, device, need, zero=False):
    """Scratch floats cached under (device, *key), grown on demand; the address is stable until then (launch tapes and captured
    graphs point at it).  A string names a family with one buffer per device ('front_bwd'; `_per_stream` adds the stream); the
    one tuple key is split-K's (stream, plan token), which `drop_workspace_scope` recognises by its length."""
    key = (str(device),) + key if isinstance(key, tuple) else (str(device), key)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = (torch.zeros if zero else torch.empty)(need, device=device, dtype=torch.float32)
        _ws_cache[key] = ws
        _alloc_epoch[0] += 1                            # recorded launch tapes point into the old buffer
    return ws


def _per_stream(family):
    """Key of a family whose launches may run on two streams at once (the plan deals weight gradients to two streams)."""
    return '%s.%d' % (family, _stream())


def _pack(size_name, size_args, pack_name, pack_args, dtype, device):
    """Packed weights: asks `size_name` for the length, allocates it, launches `pack_name`(*pack_args, out) and returns out."""
    out = torch.empty(_size(size_name, *size_args), device=device, dtype=dtype)
    _call(pack_name, *pack_args, out.data_ptr())
    return out


def packed_weight_floats(mode, c0, c1, cout):
    return lib().nlt_packed_weight_floats(mode, c0, c1, cout)       # (a query: no stream; -1 = unsupported, for the caller to read)


def pack_conv_weights(mode, w_keras, c0, c1, cout):
    return _pack('nlt_packed_weight_floats', (mode, c0, c1, cout),
                 'nlt_pack_conv_weights', (mode, _ptr(_dense(w_keras, 'w_keras')), c0, c1, cout), torch.float32, w_keras.device)


def conv_forward(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, w_keras, w_packed, bias, cout, out, ldo,
                 act=True, alpha=0.3, algo=ALGO_AUTO, tile_hint=0, mask_src=None, ldm=0, accumulate=False):
    """src*/out/mask_src may be views INTO wider tensors: pass the (already offset) tensor whose
    data_ptr() is the first element of the channel slice, and the per-texel stride ld*."""
    _call('nlt_conv_forward', mode, algo, tile_hint, _ptr(src0), ld0, c0, _ptr(src1), ld1, c1, n, h, w, _ptr(w_keras),
          _ptr(w_packed), _ptr(bias), cout, _ptr(out), ldo, 1 if act else 0, float(alpha), _ptr(mask_src), ldm,
          1 if accumulate else 0)


def stem_forward(base, cvis, lvis, nn_rgb, nn_base, obs_weights, n, k, h, w, c, wq, bq, wo, bo, fm0, obs0):
    for t, nm in ((base, 'base'), (cvis, 'cvis'), (lvis, 'lvis'), (nn_rgb, 'nn_rgb'), (nn_base, 'nn_base')):
        _dense(t, nm)
    _call('nlt_stem_forward', _ptr(base), _ptr(cvis), _ptr(lvis), _ptr(nn_rgb), _ptr(nn_base), _ptr(obs_weights), n, k, h, w, c,
          _ptr(wq), _ptr(bq), _ptr(wo), _ptr(bo), _ptr(fm0), _ptr(obs0))


def obs_mean_forward(obs, obs_weights, n, k, hw, c, out, ldo):
    _call('nlt_obs_mean_forward', _ptr(_dense(obs, 'obs')), _ptr(obs_weights), n, k, hw, c, _ptr(out), ldo)


def head_forward(dec, ldd, cd, skip, lds, cs, w_keras, bias, base, n, h, w, pred):
    _call('nlt_head_forward', _ptr(dec), ldd, cd, _ptr(skip), lds, cs, _ptr(w_keras), _ptr(bias), _ptr(base), n, h, w, _ptr(pred))


def warp_forward(pred, base, warp, n, uvh, uvw, hc, wc, pred_cam, base_cam, fg_cam, idx_out=None):
    _call('nlt_warp_forward', _ptr(pred), _ptr(base), _ptr(_dense(warp, 'warp')), n, uvh, uvw, hc, wc, _ptr(pred_cam),
          _ptr(base_cam), _ptr(fg_cam), _ptr(idx_out))


def warp_forward_store(pred, diffuse_store, uv2cam_store, ids, n, uvh, uvw, hc, wc, pred_cam, base_cam, fg_cam, idx_out=None):
    """warp_forward for a store-resident batch: base / map read from the uint8 diffuse and fp16 uv2cam stores (frame ids)."""
    if tuple(diffuse_store.shape[1:]) != (uvh, uvw, 3) or tuple(uv2cam_store.shape[1:]) != (hc, wc, 2):
        raise NLTError("stores %s / %s do not match uv %dx%d, camera %dx%d"
                       % (tuple(diffuse_store.shape), tuple(uv2cam_store.shape), uvh, uvw, hc, wc))
    _call('nlt_warp_forward_store', _ptr(pred), _tptr(diffuse_store, torch.uint8, 'diffuse store'),
          _tptr(uv2cam_store, torch.float16, 'uv2cam store'), _tptr(ids, torch.int32, 'ids'), n, uvh, uvw, hc, wc, _ptr(pred_cam),
          _ptr(base_cam), _ptr(fg_cam), _ptr(idx_out))


def resample_forward(data, warp_px):
    """tfa.image.resampler(data [n,h,w,c], warp_px [n,hc,wc,2] in pixel units) for c % 4 == 0 (the 64-channel stress point)."""
    n, h, w, c = data.shape
    hc, wc = warp_px.shape[1:3]
    out = torch.empty((n, hc, wc, c), device=data.device, dtype=torch.float32)
    _call('nlt_resample_forward', _ptr(_dense(data, 'data')), _ptr(_dense(warp_px, 'warp_px')), n, h, w, c, hc, wc, _ptr(out))
    return out


def resize_bilinear_forward(x, oh, ow):
    n, h, w, c = x.shape
    out = torch.empty((n, oh, ow, c), device=x.device, dtype=torch.float32)
    _call('nlt_resize_bilinear_forward', _ptr(_dense(x, 'x')), n, h, w, c, oh, ow, _ptr(out))
    return out


def _same_shape(a, b, what):
    if tuple(a.shape) != tuple(b.shape):
        raise NLTError("%s: shapes differ, %s vs %s" % (what, tuple(a.shape), tuple(b.shape)))


def mul_forward(a, b):
    _same_shape(a, b, 'mul_forward')
    out = torch.empty_like(a)
    _call('nlt_mul_forward', _ptr(_dense(a, 'a')), _ptr(_dense(b, 'b')), a.numel(), _ptr(out))
    return out


# ---------------------------------------------------------------- train step
# Deterministic mode (`deterministic = true`, models/nlt.py): while it is on for this thread, the adapters below whose kernels end
# in float atomics hand their arguments to the atomic-free `_det` / `_gather` siblings instead (`_call_det`).
# A case with no sibling raises NotImplementedError and names the kernel: nothing falls back to atomics silently.
class deterministic_scope:
    """`with deterministic_scope(on):` -- the mode of this thread's calls inside the block (nesting restores the outer value)."""

    def __init__(self, on):
        self.on = bool(on)

    def __enter__(self):
        self.prev = getattr(_tls, 'det', False)
        _tls.det = self.on
        return self

    def __exit__(self, *exc):
        _tls.det = self.prev
        return False


def deterministic():
    return getattr(_tls, 'det', False)


def _call_det(name, args, family, device, size, kernel=None, in_bytes=False):
    """`name`(*args), or in deterministic mode `name`_det(*args, workspace, its size): the C ABI gives every `_det` entry its plain
    twin's parameters + those two.  The workspace is cached per (family, stream, device) and sized by the query `size` = (entry
    name, *arguments), in floats or (in_bytes) in bytes.  `kernel`: the float-atomic kernel to name in the NotImplementedError
    when the query knows no atomic-free form for these shapes; without one, every shape has a form and a refusal is an NLTError."""
    if not deterministic():
        return _call(name, *args)
    if kernel is None:
        need = _size(*size)
    else:
        need = getattr(lib(), size[0])(*size[1:])       # (a query: no stream, never taped)
        if need <= 0:
            raise NotImplementedError("deterministic mode: %s (%s) has no atomic-free form: %s%r is not implemented"
                                      % (kernel, name, size[0], tuple(size[1:])))
    unit = 4 if in_bytes else 1
    ws = _workspace(_per_stream('det.' + family), device, (need + unit - 1) // unit)
    _call(name + '_det', *args, _ptr(ws), unit * ws.numel())


def conv_backward_weights(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, dpre, ldp, cout, dw, db, algo=ALGO_AUTO):
    _call_det('nlt_conv_backward_weights', (mode, algo, _ptr(src0), ld0, c0, _ptr(src1), ld1, c1, n, h, w, _ptr(dpre), ldp, cout,
                                            _ptr(dw), _ptr(db)),
              'wgrad', dpre.device, ('nlt_conv_backward_weights_det_workspace_floats', mode, c0, c1, n, h, w, cout),
              kernel='wgrad_mfma_kernel / wgrad_direct_kernel')


def conv_backward_weights_tiled(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, dpre, ldp, cout, dw, db):
    """Second-generation weight gradient (deterministic two-pass); the slice workspace is cached per device and stream."""
    ws = _workspace(_per_stream('wgrad_tiled'), src0.device, _size('nlt_wgrad_workspace_floats', mode, c0, c1, n, h, w, cout))
    _call('nlt_conv_backward_weights_tiled', mode, _ptr(src0), ld0, c0, _ptr(src1), ld1, c1, n, h, w, _ptr(dpre), ldp, cout,
          _ptr(dw), _ptr(db), _ptr(ws), ws.numel())


def wgrad_narrow_supported(mode, c0, c1, n, h, w, cout):
    return lib().nlt_wgrad_narrow_workspace_floats(mode, c0, c1, n, h, w, cout) > 0      # (a query: no stream)


def conv_backward_weights_narrow(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, dpre, ldp, cout, dw, db):
    """Weight gradient of a narrow layer (<= 32 output columns, K <= 128): MFMA tile matched to the layer."""
    ws = _workspace(_per_stream('wgrad_narrow'), src0.device, _size('nlt_wgrad_narrow_workspace_floats', mode, c0, c1, n, h, w, cout))
    _call('nlt_conv_backward_weights_narrow', mode, _ptr(src0), ld0, c0, _ptr(src1), ld1, c1, n, h, w, _ptr(dpre), ldp, cout,
          _ptr(dw), _ptr(db), _ptr(ws), ws.numel())


def conv_k3_forward(mode, x, w_keras, bias, cout, out, act=False, alpha=0.3, algo=ALGO_AUTO):
    """3x3 Conv2D / Conv2DTranspose (+ fused LeakyReLU / ReLU) on a dense [n,h,w,cin] tensor; reads the Keras array."""
    n, h, w, cin = _dense(x, 'x').shape
    _call('nlt_conv_k3_forward', mode, algo, _ptr(x), n, h, w, cin, _ptr(_dense(w_keras, 'w_keras')), _ptr(bias), cout,
          _ptr(_dense(out, 'out')), 1 if act else 0, float(alpha))


def conv_k3_backward_data(mode, dpre, w_keras, n, h, w, cin, cout, dx, algo=ALGO_AUTO):
    """dx [n,h,w,cin] of the layer `mode` from dpre [n,oh,ow,cout]: the opposite family's forward on the layer's own array."""
    _call('nlt_conv_k3_backward_data', mode, algo, _ptr(_dense(dpre, 'dpre')), n, h, w, cin, _ptr(_dense(w_keras, 'w_keras')), cout,
          _ptr(_dense(dx, 'dx')))


def conv_k3_backward_weights(mode, x, dpre, cout, dw, db):
    """dw += weight gradient, db += bias gradient of a 3x3 layer: two passes through a cached workspace, no float atomics, so the
    plain entry IS the deterministic one (`_call`, not `_call_det`)."""
    n, h, w, cin = _dense(x, 'x').shape
    ws = _workspace(_per_stream('wgrad_k3'), x.device, _size('nlt_conv_k3_wgrad_workspace_floats', mode, n, h, w, cin, cout))
    _call('nlt_conv_k3_backward_weights', mode, _ptr(x), n, h, w, cin, _ptr(_dense(dpre, 'dpre')), cout, _ptr(dw), _ptr(db),
          _ptr(ws), ws.numel())


def lrelu_backward(g, ldg, y, ldy, c, texels, alpha, out, ldo):
    _call('nlt_lrelu_backward', _ptr(g), ldg, _ptr(y), ldy, c, texels, float(alpha), _ptr(out), ldo)


def obs_mean_backward(dmean, ldm, obs_y, obs_weights, dobs_partial, n, k, hw, c, alpha, dpre_obs):
    _call('nlt_obs_mean_backward', _ptr(dmean), ldm, _ptr(obs_y), _ptr(obs_weights), _ptr(dobs_partial), n, k, hw, c, float(alpha),
          _ptr(dpre_obs))


def resize_cv_linear(src, oh, ow, out=None):
    """cv2.resize(normalised src, (ow, oh)) (INTER_LINEAR) -> float32.  src [n,h,w,c] uint8, int32 (16-bit samples) or
    float32 (already normalised)."""
    kind = {torch.uint8: 0, torch.int32: 1, torch.float32: 2}.get(src.dtype)
    if kind is None or src.dim() != 4:
        raise NLTError("resize_cv_linear: [n,h,w,c] uint8 / int32 / float32 expected, got %s %s" % (src.dtype, tuple(src.shape)))
    src = _dense(src, 'src')
    n, h, w, c = src.shape
    if out is None:
        out = torch.empty((n, oh, ow, c), device=src.device, dtype=torch.float32)
    _call('nlt_resize_cv_linear', _tptr(src, src.dtype, 'src'), kind, n, h, w, c, oh, ow, _ptr(out))
    return out


def level_split_backward(dfm, fm_y, ld, obs_y, obs_weights, dobs_partial, n, k, hw, c, alpha_q, alpha_o, dpre_obs):
    """lrelu_backward on the query half (in place) + obs_mean_backward on the observation half of dfm [n,hw,ld], one launch."""
    _call('nlt_level_split_backward', _ptr(dfm), _ptr(fm_y), ld, _ptr(obs_y), _ptr(obs_weights), _ptr(dobs_partial), n, k, hw, c,
          float(alpha_q), float(alpha_o), _ptr(dpre_obs))


def stem_backward(base, cvis, lvis, nn_rgb, nn_base, obs_weights, n, k, h, w, c, dfm0, dobs0, dwq, dbq, dwo, dbo):
    _call_det('nlt_stem_backward', (_ptr(base), _ptr(cvis), _ptr(lvis), _ptr(nn_rgb), _ptr(nn_base), _ptr(obs_weights), n, k, h, w, c,
                                    _ptr(dfm0), _ptr(dobs0), _ptr(dwq), _ptr(dbq), _ptr(dwo), _ptr(dbo)),
              'stem', dfm0.device, ('nlt_stem_backward_det_workspace_floats', n, h, w, c), kernel='stem_bwd_kernel')


def head_backward(dec, ldd, cd, skip, lds, cs, w_keras, dpred, n, h, w, d_dec, ldgd, d_skip, ldgs, dw, db):
    _call_det('nlt_head_backward', (_ptr(dec), ldd, cd, _ptr(skip), lds, cs, _ptr(w_keras), _ptr(_dense(dpred, 'dpred')), n, h, w,
                                    _ptr(d_dec), ldgd, _ptr(d_skip), ldgs, _ptr(dw), _ptr(db)),
              'head', dpred.device, ('nlt_head_backward_det_workspace_floats', n, h, w, cd, cs), kernel='head_bwd_kernel')


def warp_backward(dpred_cam, warp, n, uvh, uvw, hc, wc, dpred):
    # (irregular: the `_det` form sizes its workspace in BYTES, and refuses >= 2^29 camera pixels)
    _call_det('nlt_warp_backward', (_ptr(_dense(dpred_cam, 'dpred_cam')), _ptr(_dense(warp, 'warp')), n, uvh, uvw, hc, wc, _ptr(dpred)),
              'warp', dpred.device, ('nlt_warp_backward_det_workspace_bytes', n, uvh, uvw, hc, wc), kernel='warp_bwd_kernel',
              in_bytes=True)


def warp_backward_det(dpred_cam, warp, n, uvh, uvw, hc, wc, dpred):
    """nlt_warp_backward with each texel's contributions added in ascending (camera pixel, corner) order: bit-repeatable."""
    with deterministic_scope(True):
        warp_backward(dpred_cam, warp, n, uvh, uvw, hc, wc, dpred)


def resize_bilinear_backward(dout, h, w):
    n, oh, ow, c = dout.shape
    dx = torch.empty((n, h, w, c), device=dout.device, dtype=torch.float32)
    # (irregular: the atomic-free sibling is a gather -- its own suffix, no workspace)
    _call('nlt_resize_bilinear_backward' + ('_gather' if deterministic() else ''), _ptr(_dense(dout, 'dout')), n, h, w, c, oh, ow,
          _ptr(dx))
    return dx


def _loss_det_size(n):
    return ('nlt_loss_det_workspace_floats', n)         # the three L2 losses share the family 'loss' and this query


def l2_loss_forward(pred, gt):
    _same_shape(pred, gt, 'l2_loss_forward')
    n = pred.shape[0]
    loss = torch.empty(n, device=pred.device, dtype=torch.float32)
    _call_det('nlt_l2_loss_forward', (_ptr(_dense(pred, 'pred')), _ptr(_dense(gt, 'gt')), n, pred[0].numel(), _ptr(loss)),
              'loss', pred.device, _loss_det_size(n))
    return loss


def l2_train_loss(pred, rgb, fg, global_bs):
    """gt = rgb * fg, loss = sum_f mean((pred_f - gt_f)^2) / global_bs (0-dim tensor), dpred: one launch."""
    _same_shape(pred, rgb, 'l2_train_loss'); _same_shape(pred, fg, 'l2_train_loss')
    gt, dpred = torch.empty_like(pred), torch.empty_like(pred)
    loss = torch.empty((), device=pred.device, dtype=torch.float32)
    _call_det('nlt_l2_train_loss', (_ptr(_dense(pred, 'pred')), _ptr(_dense(rgb, 'rgb')), _ptr(_dense(fg, 'fg')), pred.shape[0],
                                    pred[0].numel(), 1.0 / float(global_bs), _ptr(gt), _ptr(dpred), _ptr(loss)),
              'loss', pred.device, _loss_det_size(pred.shape[0]))
    return loss, gt, dpred


def l2_loss_backward(pred, gt, gloss):
    _same_shape(pred, gt, 'l2_loss_backward')
    if gloss.numel() != pred.shape[0]:
        raise NLTError("l2_loss_backward: %d loss gradients for %d examples" % (gloss.numel(), pred.shape[0]))
    dpred = torch.empty_like(pred)
    _call('nlt_l2_loss_backward', _ptr(pred), _ptr(gt), _ptr(_dense(gloss, 'gloss')), pred.shape[0], pred[0].numel(), _ptr(dpred))
    return dpred


def l2_loss_weighted_forward(pred, gt, weights):
    """weights [N,H,W] (already broadcast): loss[f] = mean_hw(weights * mean_c (gt - pred)^2)."""
    _same_shape(pred, gt, 'l2_loss_weighted_forward')
    n, c = pred.shape[0], pred.shape[-1]
    hw = pred[0].numel() // c
    if weights.numel() != n * hw:
        raise NLTError("l2_loss_weighted_forward: %d weights for %d texels" % (weights.numel(), n * hw))
    loss = torch.empty(n, device=pred.device, dtype=torch.float32)
    _call_det('nlt_l2_loss_weighted_forward', (_ptr(_dense(pred, 'pred')), _ptr(_dense(gt, 'gt')), _ptr(_dense(weights, 'weights')),
                                               n, hw, c, _ptr(loss)),
              'loss', pred.device, _loss_det_size(n))
    return loss


def l2_loss_weighted_backward(pred, gt, weights, gloss):
    _same_shape(pred, gt, 'l2_loss_weighted_backward')
    n, c = pred.shape[0], pred.shape[-1]
    hw = pred[0].numel() // c
    if gloss.numel() != n or weights.numel() != n * hw:
        raise NLTError("l2_loss_weighted_backward: %d loss gradients, %d weights for %d examples of %d texels"
                       % (gloss.numel(), weights.numel(), n, hw))
    dpred = torch.empty_like(pred)
    _call('nlt_l2_loss_weighted_backward', _ptr(_dense(pred, 'pred')), _ptr(_dense(gt, 'gt')), _ptr(_dense(weights, 'weights')),
          _ptr(_dense(gloss, 'gloss')), n, hw, c, _ptr(dpred))
    return dpred


def barron_loss(pred, gt, want_grad):
    _same_shape(pred, gt, 'barron_loss')
    n, h, w, c = pred.shape
    assert c == 3
    ws = torch.empty(_size('nlt_barron_workspace_floats', n, h, w), device=pred.device, dtype=torch.float32)
    loss = torch.empty(n, device=pred.device, dtype=torch.float32)
    dunit = torch.empty_like(pred) if want_grad else None
    # (irregular: `ws` is the ordinary per-call scratch of both forms; what the `_det` form appends is its `slots`, sized by a query
    # named after them)
    _call_det('nlt_barron_loss', (_ptr(_dense(pred, 'pred')), _ptr(_dense(gt, 'gt')), n, h, w, _ptr(ws), _ptr(loss), _ptr(dunit)),
              'barron', pred.device, ('nlt_barron_det_slots_floats', n, h, w))
    return loss, dunit


def ssim_loss(pred, gt, max_val, want_grad):
    """pred, gt [n,h,w,c] (c = 1 or 3, h, w >= 11) -> (loss [n] = (1 - ssim(gt, pred)) / 2, d loss[f] / d pred or None).  One
    form for both modes: its sums are ordered (csrc/ssim.hip), so `deterministic` has nothing to switch."""
    _same_shape(pred, gt, 'ssim_loss')
    if pred.dim() != 4:
        raise NLTError("ssim_loss: [n,h,w,c] expected, got %s" % (tuple(pred.shape),))
    n, h, w, c = pred.shape
    ws = torch.empty(_size('nlt_ssim_workspace_floats', n, h, w, c, 1 if want_grad else 0, what='h, w >= 11 and 1 or 3 channels'),
                     device=pred.device, dtype=torch.float32)
    loss = torch.empty(n, device=pred.device, dtype=torch.float32)
    dunit = torch.empty_like(pred) if want_grad else None
    _call('nlt_ssim_loss', _ptr(_dense(pred, 'pred')), _ptr(_dense(gt, 'gt')), n, h, w, c, float(max_val), _ptr(ws), ws.numel(),
          _ptr(loss), _ptr(dunit))
    return loss, dunit


def ssim_values(im1, im2, max_val):
    """im1, im2 [n,h,w,c] float32 (c = 1, or 3: luma first) -> SSIM of every pair as a float64 CUDA tensor [n], one launch."""
    _same_shape(im1, im2, 'ssim_values')
    if im1.dim() != 4:
        raise NLTError("ssim_values: [n,h,w,c] expected, got %s" % (tuple(im1.shape),))
    n, h, w, c = im1.shape
    ws = torch.empty(_size('nlt_ssim_workspace_floats', n, h, w, c, 0, what='h, w >= 11 and 1 or 3 channels'),
                     device=im1.device, dtype=torch.float32)
    out = torch.empty(n, device=im1.device, dtype=torch.float64)
    _call('nlt_ssim_values', _ptr(_dense(im1, 'im1')), _ptr(_dense(im2, 'im2')), n, h, w, c, float(max_val), _ptr(ws), ws.numel(),
          out.data_ptr())
    return out


# ---------------------------------------------------------------- LPIPS v0.1, alex / lin (csrc/lpips.hip)
def _lpips_out(n, h, w, c, like):
    return torch.empty((n, h, w, c), device=like.device, dtype=torch.float32)


def lpips_conv1_forward(x, affine, w_keras, bias):
    """x [n,h,w,3] in [0,1], affine = shift[3] + scale[3], w_keras (11,11,3,64) -> relu(conv1(((2x - 1) - shift) / scale)) [n,h1,w1,64]."""
    n, h, w, _ = _dense(x, 'x').shape
    y = _lpips_out(n, (h - 7) // 4 + 1, (w - 7) // 4 + 1, 64, x)
    _call('nlt_lpips_conv1_forward', _ptr(x), n, h, w, _ptr(_dense(affine, 'affine')), _ptr(_dense(w_keras, 'w_keras')), _ptr(bias), _ptr(y))
    return y


def lpips_conv1_backward_data(dpre, h, w, affine, w_keras):
    """dpre [n,h1,w1,64] (w.r.t. conv1's pre-activation) -> d / d x [n,h,w,3], the 2 / scale of the input affine included."""
    n = _dense(dpre, 'dpre').shape[0]
    dx = _lpips_out(n, h, w, 3, dpre)
    _call('nlt_lpips_conv1_backward_data', _ptr(dpre), n, h, w, _ptr(_dense(affine, 'affine')), _ptr(_dense(w_keras, 'w_keras')), _ptr(dx))
    return dx


def lpips_conv2_forward(x, w_keras, bias):
    """x [n,h,w,64], w_keras (5,5,64,192) -> relu(conv2(x)) [n,h,w,192]."""
    n, h, w, _ = _dense(x, 'x').shape
    y = _lpips_out(n, h, w, 192, x)
    _call('nlt_lpips_conv2_forward', _ptr(x), n, h, w, _ptr(_dense(w_keras, 'w_keras')), _ptr(bias), _ptr(y))
    return y


def lpips_conv2_backward_data(dpre, w_keras):
    """dpre [n,h,w,192] -> d / d (conv2's input) [n,h,w,64]."""
    n, h, w, _ = _dense(dpre, 'dpre').shape
    dx = _lpips_out(n, h, w, 64, dpre)
    _call('nlt_lpips_conv2_backward_data', _ptr(dpre), n, h, w, _ptr(_dense(w_keras, 'w_keras')), _ptr(dx))
    return dx


def lpips_pool_forward(x):
    """Max-pool 3x3 stride 2, no padding, floor."""
    n, h, w, c = _dense(x, 'x').shape
    y = _lpips_out(n, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c, x)
    _call('nlt_lpips_pool_forward', _ptr(x), n, h, w, c, _ptr(y))
    return y


def lpips_pool_backward(dy, x):
    """d / d x of lpips_pool_forward(x) from dy: each window's gradient to its first maximum in window order."""
    n, h, w, c = _dense(x, 'x').shape
    dx = torch.empty_like(x)
    _call('nlt_lpips_pool_backward', _ptr(_dense(dy, 'dy')), _ptr(x), n, h, w, c, _ptr(dx))
    return dx


def lpips_head_forward(fp, fg, lin):
    """fp, fg [n,h,w,c] feature maps of one level -> d [n] = mean over texels of sum_c lin[c] (fp / |fp| - fg / |fg|)^2."""
    _same_shape(fp, fg, 'lpips_head_forward')
    n, h, w, c = _dense(fp, 'fp').shape
    ws = torch.empty(_size('nlt_lpips_head_workspace_floats', n, h * w), device=fp.device, dtype=torch.float32)
    d = torch.empty(n, device=fp.device, dtype=torch.float32)
    _call('nlt_lpips_head_forward', _ptr(fp), _ptr(_dense(fg, 'fg')), n, h * w, c, _ptr(_dense(lin, 'lin')), _ptr(ws), ws.numel(), _ptr(d))
    return d


def lpips_head_backward(fp, fg, lin, dup=None):
    """(dup + d d[f] / d fp) * (fp > 0): the gradient w.r.t. the pre-activation of the conv that made fp."""
    _same_shape(fp, fg, 'lpips_head_backward')
    n, h, w, c = _dense(fp, 'fp').shape
    dpre = torch.empty_like(fp)
    _call('nlt_lpips_head_backward', _ptr(fp), _ptr(_dense(fg, 'fg')), n, h * w, c, _ptr(_dense(lin, 'lin')),
          _ptr(None if dup is None else _dense(dup, 'dup')), _ptr(dpre))
    return dpre


def lpips_loss(pred, gt, weights, want_grad):
    """pred, gt [n,h,w,3] in [0,1] (h, w >= 31), weights: the blob of lpips_weights.blob() on the device -> (loss [n], d loss[f] /
    d pred or None).  One form for both modes: its sums are ordered (csrc/lpips.hip), so `deterministic` has nothing to switch."""
    _same_shape(pred, gt, 'lpips_loss')
    if pred.dim() != 4 or pred.shape[3] != 3:
        raise NLTError("lpips_loss: [n,h,w,3] expected, got %s" % (tuple(pred.shape),))
    if weights.numel() != lib().nlt_lpips_weights_floats():
        raise NLTError("lpips_loss: a weights blob of %d floats expected, got %d" % (lib().nlt_lpips_weights_floats(), weights.numel()))
    n, h, w, _ = pred.shape
    ws = torch.empty(_size('nlt_lpips_workspace_floats', n, h, w, 1 if want_grad else 0, what='h, w >= 31'),
                     device=pred.device, dtype=torch.float32)
    loss = torch.empty(n, device=pred.device, dtype=torch.float32)
    dunit = torch.empty_like(pred) if want_grad else None
    _call('nlt_lpips_loss', _ptr(_dense(pred, 'pred')), _ptr(_dense(gt, 'gt')), n, h, w, _ptr(_dense(weights, 'weights')), _ptr(ws),
          ws.numel(), _ptr(loss), _ptr(dunit))
    return loss, dunit


# ---------------------------------------------------------------- relighting under an environment map (csrc/relight.hip)
def envmap_light_weights(envmap, dirs, rot):
    """envmap [he,we,3] (linear radiance, lat-long, z-up: include/nlt_hip.h), dirs [L,3] unit vectors, rot [R,3,3] -> [R,L,3]:
    per rotation and light the probe's solid-angle integral over the pixels nearest that light.  Ordered float64 sums."""
    if envmap.dim() != 3 or envmap.shape[2] != 3 or dirs.dim() != 2 or dirs.shape[1] != 3 or rot.dim() != 3 or tuple(rot.shape[1:]) != (3, 3):
        raise NLTError("envmap_light_weights: envmap [he,we,3], dirs [L,3], rot [R,3,3] expected, got %s, %s, %s"
                       % (tuple(envmap.shape), tuple(dirs.shape), tuple(rot.shape)))
    he, we, n_lights, n_rot = envmap.shape[0], envmap.shape[1], dirs.shape[0], rot.shape[0]
    need = _size('nlt_envmap_light_weights_workspace_floats', he, we, n_lights, n_rot, what='at most 1024 lights')
    ws = _workspace(_per_stream('envmap_weights'), envmap.device, need)
    out = torch.empty((n_rot, n_lights, 3), device=envmap.device, dtype=torch.float32)
    _call('nlt_envmap_light_weights', _ptr(_dense(envmap, 'envmap')), he, we, _ptr(_dense(dirs, 'dirs')), n_lights,
          _ptr(_dense(rot, 'rot')), n_rot, _ptr(ws), ws.numel(), _ptr(out))
    return out


def relight_accumulate(pred, weights, l0, acc, is_linear):
    """acc [R,texels,3] += sum_l weights[:, l0 + l] * lin(clip01(pred[l])) over the chunk pred [Lc,...,3] (any texel shape), one
    fmaf per light in light order; weights [R,L,3].  In place; returns acc."""
    if pred.dim() < 2 or pred.shape[-1] != 3 or weights.dim() != 3 or weights.shape[2] != 3 or acc.dim() < 2 or acc.shape[-1] != 3:
        raise NLTError("relight_accumulate: pred [Lc,...,3], weights [R,L,3], acc [R,...,3] expected, got %s, %s, %s"
                       % (tuple(pred.shape), tuple(weights.shape), tuple(acc.shape)))
    n_chunk, n_rot, n_lights = pred.shape[0], weights.shape[0], weights.shape[1]
    texels = pred[0].numel() // 3
    if acc.shape[0] != n_rot or acc[0].numel() != texels * 3:
        raise NLTError("relight_accumulate: acc %s does not match %d rotations of %d texels" % (tuple(acc.shape), n_rot, texels))
    _call('nlt_relight_accumulate', _ptr(_dense(pred, 'pred')), n_chunk, texels, _ptr(_dense(weights, 'weights')), n_rot, n_lights,
          int(l0), 1 if is_linear else 0, _ptr(_dense(acc, 'acc')))
    return acc


def relight_finish(acc, exposure, to_srgb):
    """enc(clip01(exposure * acc)) as a new tensor of acc's shape [R,...,3]; enc: sRGB encode (to_srgb) or the identity."""
    if acc.dim() < 2 or acc.shape[-1] != 3:
        raise NLTError("relight_finish: acc [R,...,3] expected, got %s" % (tuple(acc.shape),))
    out = torch.empty_like(acc)
    _call('nlt_relight_finish', _ptr(_dense(acc, 'acc')), acc.shape[0], acc[0].numel() // 3, float(exposure), 1 if to_srgb else 0,
          _ptr(out))
    return out


def scale_rows(x, scale):
    if scale.numel() != x.shape[0]:
        raise NLTError("scale_rows: %d scales for %d rows" % (scale.numel(), x.shape[0]))
    out = torch.empty_like(x)
    _call('nlt_scale_rows', _ptr(_dense(x, 'x')), _ptr(_dense(scale, 'scale')), x.shape[0], x[0].numel(), _ptr(out))
    return out


# ---------------------------------------------------------------- layers of the non-default config branches
ACT_LRELU, ACT_ELU = 0, 1
POOL_MAX, POOL_AVG = 0, 1


def sub_forward(a, b):
    _same_shape(a, b, 'sub_forward')
    out = torch.empty_like(a)
    _call('nlt_sub_forward', _ptr(_dense(a, 'a')), _ptr(_dense(b, 'b')), a.numel(), _ptr(out))
    return out


def finish_pred(y, base, pred):
    n, h, w, c = y.shape
    if c != 3 or (base is not None and tuple(base.shape) != tuple(y.shape)) or tuple(pred.shape) != tuple(y.shape):
        raise NLTError("finish_pred: y / base / pred must be [n,h,w,3] of one shape")
    _call('nlt_finish_pred', _ptr(_dense(y, 'y')), _ptr(base), n, h, w, _ptr(pred))


def act_forward(x, kind, alpha):
    y = torch.empty_like(x)
    _call('nlt_act_forward', _ptr(_dense(x, 'x')), x.numel(), kind, float(alpha), _ptr(y))
    return y


def act_backward(g, y, kind, alpha):
    _same_shape(g, y, 'act_backward')
    dx = torch.empty_like(y)
    _call('nlt_act_backward', _ptr(_dense(g, 'g')), _ptr(_dense(y, 'y')), y.numel(), kind, float(alpha), _ptr(dx))
    return dx


def pixelnorm_forward(x, eps=1e-8):
    y = torch.empty_like(x)
    c = x.shape[-1]
    _call('nlt_pixelnorm_forward', _ptr(_dense(x, 'x')), x.numel() // c, c, float(eps), _ptr(y))
    return y


def pixelnorm_backward(g, x, eps=1e-8):
    _same_shape(g, x, 'pixelnorm_backward')
    dx = torch.empty_like(x)
    c = x.shape[-1]
    _call('nlt_pixelnorm_backward', _ptr(_dense(g, 'g')), _ptr(_dense(x, 'x')), x.numel() // c, c, float(eps), _ptr(dx))
    return dx


NORM_LAYER, NORM_BATCH = 0, 1


def norm_forward(kind, x, gamma, beta, mean, var, eps):
    """LayerNormalization (kind 0) / inference-mode BatchNormalization (kind 1) over the channel axis of x [..., c]."""
    c = x.shape[-1]
    y = torch.empty_like(x)
    _call('nlt_norm_forward', kind, _ptr(_dense(x, 'x')), x.numel() // c, c, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(var),
          float(eps), _ptr(y))
    return y


def norm_backward(kind, g, x, gamma, mean, var, eps, dgamma, dbeta):
    """dx; dgamma / dbeta are ACCUMULATED into the given views (of the flat gradient bucket)."""
    _same_shape(g, x, 'norm_backward')
    c = x.shape[-1]
    texels = x.numel() // c
    ws = _workspace('norm', x.device, _size('nlt_norm_workspace_floats', texels, c, what='the kernel takes c <= 1024'))
    dx = torch.empty_like(x)
    _call('nlt_norm_backward', kind, _ptr(_dense(g, 'g')), _ptr(_dense(x, 'x')), texels, c, _ptr(gamma), _ptr(mean), _ptr(var),
          float(eps), _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(ws))
    return dx


def pool2x2_forward(x, kind):
    n, h, w, c = x.shape
    y = torch.empty((n, h // 2, w // 2, c), device=x.device, dtype=torch.float32)
    _call('nlt_pool2x2_forward', _ptr(_dense(x, 'x')), n, h, w, c, kind, _ptr(y))
    return y


def pool2x2_backward(g, x, kind):
    n, h, w, c = x.shape
    if tuple(g.shape) != (n, h // 2, w // 2, c):
        raise NLTError("pool2x2_backward: gradient %s for input %s" % (tuple(g.shape), tuple(x.shape)))
    dx = torch.empty_like(x)
    _call('nlt_pool2x2_backward', _ptr(_dense(g, 'g')), _ptr(_dense(x, 'x')), n, h, w, c, kind, _ptr(dx))
    return dx


def clip_by_norm_slots(grad, slots, clipnorm):
    """grad: flat fp32 bucket; slots: int64 [n,2] (offset, count) on the same device; in place."""
    _call('nlt_clip_by_norm_slots', _ptr(grad), _tptr(slots, torch.int64, 'slots'), slots.shape[0], float(clipnorm))


def adam_amsgrad_step(param, grad, m, v, vhat, lr_t, beta1, beta2, eps):
    _call('nlt_adam_amsgrad_step', _ptr(param), _ptr(grad), _ptr(m), _ptr(v), _ptr(vhat), param.numel(), float(lr_t), float(beta1),
          float(beta2), float(eps))


def _splitk_workspace(mode, n, h, w, cout, ksplit, device, always=False):
    """The split-K scratch of the current (device, stream, plan) for |ksplit| > 1 (`always`: for any ksplit), else None: cached,
    grown on demand, ZEROED when allocated -- its first words are the tiles' ticket counters, which every launch leaves at zero
    (include/nlt_hip.h: nlt_conv_splitk_workspace_floats).  Per stream: the query and observation paths run concurrently; per
    plan: see set_workspace_scope."""
    if abs(ksplit) <= 1 and not always:
        return None
    need = _size('nlt_conv_splitk_workspace_floats', mode, n, h, w, cout, ksplit)
    return _workspace((_stream(), getattr(_tls, 'scope', 0)), device, need, zero=True)


def conv_forward_splitk(mode, ksplit, src0, c0, ld0, src1, c1, ld1, n, h, w, w_packed, bias, cout, out, ldo,
                        act=True, alpha=0.3, tile_hint=0, mask_src=None, ldm=0, accumulate=False):
    """nlt_conv_forward (MFMA path) with the K loop split over |ksplit| wave slices (ksplit > 0: one launch, the last workgroup
    to arrive at a tile adds the groups' partial tiles; ksplit < 0: the two-launch form of rounds 2-5); the partial-sum
    workspace is cached per device and grown on demand."""
    ws = _splitk_workspace(mode, n, h, w, cout, ksplit, src0.device, always=True)
    _call('nlt_conv_forward_splitk', mode, tile_hint, ksplit, _ptr(ws), _ptr(src0), ld0, c0, _ptr(src1), ld1, c1, n, h, w,
          _ptr(w_packed), _ptr(bias), cout, _ptr(out), ldo, 1 if act else 0, float(alpha), _ptr(mask_src), ldm,
          1 if accumulate else 0)


def conv_forward_map(mode, ksplit, src0, c0, ld0, src1, c1, ld1, n, h, w, w_packed, bias, cout, out, ldo, bias_map,
                     act=True, alpha=0.3, tile_hint=0, w_keras=None):
    """out = act(conv(src0 | src1) + bias + bias_map): the per-frame half of a conv over concat(q, given observation map)
    (include/nlt_hip.h: nlt_conv_forward_map).  bias_map [1 or n, oh, ow, cout] dense.  (w_keras is not read here; the host
    tests' CPU emulation of this adapter computes from it.)"""
    ws = _splitk_workspace(mode, n, h, w, cout, ksplit, src0.device)
    _call('nlt_conv_forward_map', mode, tile_hint, ksplit, _ptr(ws), _ptr(src0), ld0, c0, _ptr(src1), ld1, c1, n, h, w,
          _ptr(w_packed), _ptr(bias), cout, _ptr(out), ldo, 1 if act else 0, float(alpha), _ptr(_dense(bias_map, 'bias_map')),
          bias_map.shape[0])


def conv_backward_data(adj_mode, dpre, cpre, ldp, n, h, w, w_packed, zero_bias, cout, out, ldo, mask_src=None, ldm=0,
                       mask_alpha=0.3, accumulate=False, tile_hint=0, ksplit=1, split=None, w_keras=None):
    """Gradient w.r.t. a conv's input channels (include/nlt_hip.h: nlt_conv_backward_data).  split = (c, obs_y, dobs,
    alpha_o, has_partial): the target is dfm[l] with one observation per frame; its observation half goes, finished, to dobs.
    (w_keras -- the Keras-layout slice the fragments were packed from -- is not read here; the host tests' CPU emulation of
    this adapter computes from it.)"""
    ws = _splitk_workspace(adj_mode, n, h, w, cout, ksplit, dpre.device)
    sc, sy, sd, sa, sp = split if split is not None else (0, None, None, 0.0, False)
    _call('nlt_conv_backward_data', adj_mode, tile_hint, ksplit, _ptr(ws), _ptr(dpre), ldp, cpre, n, h, w, _ptr(w_packed),
          _ptr(zero_bias), cout, _ptr(out), ldo, _ptr(mask_src), ldm, float(mask_alpha), 1 if accumulate else 0, sc, _ptr(sy),
          _ptr(sd), float(sa), 1 if sp else 0)


# ---------------------------------------------------------------- one-launch refresh of all packed weights
REPACK_MFMA, REPACK_TILE, REPACK_WINO, REPACK_TILE3S2 = 0, 1, 2, 3
REPACK_FIELDS = [('src', 'u8'), ('dst', 'u8'), ('total', 'i8'), ('first_block', 'i8'), ('kind', 'i4'), ('mode', 'i4'),
                 ('c0', 'i4'), ('c1', 'i4'), ('cout', 'i4'), ('tn', 'i4'), ('lo', 'i4'), ('full', 'i4')]   # = nlt_repack_desc


def repack_table(entries, device):
    """entries: dicts with the nlt_repack_desc fields except first_block (src / dst as tensors).  Returns the device
    table (uint8 tensor), the number of descriptors and the grid size for nlt_repack_weights."""
    import numpy as np
    tab = np.zeros(len(entries), dtype=np.dtype(REPACK_FIELDS))
    blocks = 0
    for i, e in enumerate(entries):
        nbytes = e['dst'].numel() * e['dst'].element_size()           # (bf16 term buffers count in 4-byte words like the rest)
        if nbytes % 16 or e['dst'].data_ptr() % 16:                    # (the refresh launch stores quads)
            raise NLTError("repack_table: a packed buffer must be 16-byte aligned and a multiple of 4 floats long")
        tab[i] = (e['src'].data_ptr(), e['dst'].data_ptr(), nbytes // 4, blocks, e['kind'], e['mode'], e['c0'], e['c1'],
                  e['cout'], e['tn'], e['lo'], e['full'])
        blocks += (nbytes // 4 + 255) // 256
    return torch.from_numpy(tab.view(np.uint8)).to(device), len(entries), blocks


def repack_weights(table, n_desc, total_blocks):
    _call('nlt_repack_weights', _tptr(table, torch.uint8, 'repack table'), n_desc, total_blocks)


# ---------------------------------------------------------------- LDS-tiled encoder convs
def conv_tile_supported(mode, cin, cout, tn):
    return lib().nlt_conv_tile_packed_floats(mode, cin, cout, tn) > 0       # (a query: no stream)


def pack_conv_tile_weights(mode, w_keras, cin, cout, tn):
    return _pack('nlt_conv_tile_packed_floats', (mode, cin, cout, tn),
                 'nlt_pack_conv_tile_weights', (mode, _ptr(_dense(w_keras, 'w_keras')), cin, cout, tn), torch.float32, w_keras.device)


def conv_tile_forward(mode, src, ld, cin, frames, kobs, h, w, packed, bias, cout, tn, out, ldo, mean_out, ldm,
                      act=True, alpha=0.3):
    _call('nlt_conv_tile_forward', mode, _ptr(src), ld, cin, frames, kobs, h, w, _ptr(packed), _ptr(bias), cout, tn, _ptr(out), ldo,
          _ptr(mean_out), ldm, 1 if act else 0, float(alpha))


def pack_conv_tile_weights_adjoint(adj_mode, w_keras, cpre, cout, tn, full, lo):
    """Tile fragments of the ADJOINT conv family read from the layer's own (contiguous) Keras array: output columns = the layer's
    input channels [lo, lo + cout) of `full`."""
    return _pack('nlt_conv_tile_packed_floats', (adj_mode, cpre, cout, tn), 'nlt_pack_conv_tile_weights_adjoint',
                 (adj_mode, _ptr(_dense(w_keras, 'w_keras')), cpre, cout, tn, full, lo), torch.float32, w_keras.device)


def conv_tile_backward_data(adj_mode, dpre, cpre, ldp, n, h, w, packed, cout, tn, out, ldo, mask_src=None, ldm=0, mask_alpha=0.3,
                            accumulate=False, split=None, w_keras=None):
    """Backward-data on the LDS-tiled kernel (include/nlt_hip.h: nlt_conv_tile_backward_data); split as conv_backward_data's
    (transposed k2s2 mode only)."""
    sc, sy, sd, sa, sp = split if split is not None else (0, None, None, 0.0, False)
    _call('nlt_conv_tile_backward_data', adj_mode, _ptr(dpre), ldp, cpre, n, h, w, _ptr(packed), cout, tn, _ptr(out), ldo,
          _ptr(mask_src), ldm, float(mask_alpha), 1 if accumulate else 0, sc, _ptr(sy), _ptr(sd), float(sa), 1 if sp else 0)


def conv_c32_supported(mode, cin, cout):
    return lib().nlt_conv_c32_supported(mode, cin, cout) > 0        # (a query: no stream)


def conv_c32_forward(mode, src, ld, cin, frames, kobs, h, w, packed, bias, cout, out, ldo, mean_out, ldm, act=True, alpha=0.3):
    """Narrow stride-1 conv (cin 16 | 32 -> 32) with LDS-resident weights; packed = pack_conv_tile_weights(mode, w, cin, 32, 32)."""
    _call('nlt_conv_c32_forward', mode, _ptr(src), ld, cin, frames, kobs, h, w, _ptr(packed), _ptr(bias), cout, _ptr(out), ldo,
          _ptr(mean_out), ldm, 1 if act else 0, float(alpha))


# ---------------------------------------------------------------- Winograd stride-1 k2 convs (csrc/conv_wino.hip)
def conv_wino_supported(mode, cin, cout, tn):
    return lib().nlt_conv_wino_packed_floats(mode, cin, cout, tn) > 0       # (a query: no stream)


def pack_conv_wino_weights(mode, w_keras, cin, cout, tn, full=None, lo=0):
    """G g G^T fragments of a stride-1 k2 kernel; full / lo: the ADJOINT family read from a layer's own array (columns = that
    layer's input channels [lo, lo + cout) of `full`)."""
    src = (mode, _ptr(_dense(w_keras, 'w_keras')), cin, cout, tn)
    if full is None:
        name, args = 'nlt_pack_conv_wino_weights', src
    else:
        name, args = 'nlt_pack_conv_wino_weights_adjoint', src + (full, lo)
    return _pack('nlt_conv_wino_packed_floats', (mode, cin, cout, tn), name, args, torch.float32, w_keras.device)


def conv_wino_forward(mode, src, ld, cin, frames, kobs, h, w, packed, bias, cout, tn, out, ldo, mean_out, ldm, act=True, alpha=0.3):
    _call('nlt_conv_wino_forward', mode, _ptr(src), ld, cin, frames, kobs, h, w, _ptr(packed), _ptr(bias), cout, tn, _ptr(out), ldo,
          _ptr(mean_out), ldm, 1 if act else 0, float(alpha))


def conv_wino_backward_data(adj_mode, dpre, cpre, ldp, n, h, w, packed, cout, tn, out, ldo, mask_src=None, ldm=0, mask_alpha=0.3,
                            accumulate=False):
    _call('nlt_conv_wino_backward_data', adj_mode, _ptr(dpre), ldp, cpre, n, h, w, _ptr(packed), cout, tn, _ptr(out), ldo,
          _ptr(mask_src), ldm, float(mask_alpha), 1 if accumulate else 0)


# ---------------------------------------------------------------- bf16 middle of the network
def pack_conv_tile3_weights(mode, w_keras, cin, cout, tn):
    return _pack('nlt_conv_tile3_packed_elems', (mode, cin, cout, tn),
                 'nlt_pack_conv_tile3_weights', (mode, _ptr(_dense(w_keras, 'w_keras')), cin, cout, tn), torch.int16, w_keras.device)


def conv_tile3_forward(mode, src, ld, cin, frames, kobs, h, w, packed, bias, cout, tn, out, ldo, mean_out, ldm,
                       act=True, alpha=0.3, nprod=6):
    """conv_tile_forward with fp32 operands split into three bf16 terms (precision = f32x3; nprod = 6 or 9 term products)."""
    _call('nlt_conv_tile3_forward', mode, nprod, _ptr(src), ld, cin, frames, kobs, h, w, packed.data_ptr(), _ptr(bias), cout, tn,
          _ptr(out), ldo, _ptr(mean_out), ldm, 1 if act else 0, float(alpha))


def conv_tile3r_plan(mode, cin, tn):
    """The resident form's launch shape as csrc/conv_tile3.hip's launcher works it out: (LDS bytes of a workgroup, waves per
    workgroup, workgroups per CU, output rows of a tile), or None where it refuses (the group's weights + the texel staging exceed
    the CU's 160 KB).  Stride 1 at 32 channels per group: 8 waves with a 4 x 16 (else 2 x 16) tile and a staging region each;
    otherwise the 8 x 16 tile of a workgroup and two shared texel stages."""
    if mode not in (CONV_K2S1, CONV_K2S2) or cin % 16 or tn not in (32, 64):
        return None
    if mode == CONV_K2S1 and tn == 32:
        for rows in (4, 2):
            lds = cin * 768 + 8 * 6 * (((rows + 1) * 17 + 15) // 16 * 16) * 16
            if lds <= 160 * 1024:
                return (lds, 8, 1, rows)
    lds = cin * (tn // 16) * 384 + 2 * 6 * (160 if mode == CONV_K2S1 else 272) * 16
    if lds > 160 * 1024:
        return None
    return (lds, 8, 1, 8) if 2 * lds > 160 * 1024 else (lds, 4, 2, 8)


def conv_tile3r_forward(mode, src, ld, cin, frames, kobs, h, w, packed, bias, cout, tn, out, ldo, mean_out, ldm,
                        act=True, alpha=0.3, nprod=6, max_workgroups=0):
    """conv_tile3_forward by persistent workgroups with the group's split weights resident in LDS: the same bits."""
    _call('nlt_conv_tile3r_forward', mode, nprod, _ptr(src), ld, cin, frames, kobs, h, w, packed.data_ptr(), _ptr(bias), cout, tn,
          _ptr(out), ldo, _ptr(mean_out), ldm, 1 if act else 0, float(alpha), max_workgroups)


def conv_tile3d_forward(mode, src, ld, cin, frames, kobs, h, w, packed, bias, cout, tn, out, ldo, mean_out, ldm,
                        act=True, alpha=0.3, nprod=6):
    """conv_tile3_forward's stride-2 conv with the texels loaded straight into MFMA operands (no LDS texel stage): the same bits.
    mean_out must be None."""
    _call('nlt_conv_tile3d_forward', mode, nprod, _ptr(src), ld, cin, frames, kobs, h, w, packed.data_ptr(), _ptr(bias), cout, tn,
          _ptr(out), ldo, _ptr(mean_out), ldm, 1 if act else 0, float(alpha))


def pack_conv_tile3w_s2_weights(w_keras, cin2, cout2):
    """Three-term bf16 fragments of a stride-2 k2 kernel in the channel order the stride-1 stage of conv_tile3w_s2_forward hands
    its results over in (csrc/pack_common.h: nlt_tile3s2_fragment)."""
    return _pack('nlt_conv_tile3w_s2_packed_elems', (cin2, cout2),
                 'nlt_pack_conv_tile3w_s2_weights', (_ptr(_dense(w_keras, 'w_keras')), cin2, cout2), torch.int16, w_keras.device)


def conv_tile3w_s2_plan(cin, cout, cout2):
    """LDS bytes of a workgroup of conv_tile3w_s2_forward (both weight sets + 8 wave regions), or None where it refuses."""
    n = lib().nlt_conv_tile3w_s2_lds_bytes(cin, cout, cout2)          # (a query: no stream)
    return n if n > 0 else None


def conv_tile3w_s2_forward(src, ld, cin, frames, kobs, h, w, packed, bias, cout, mean_out, ldm, packed2, bias2, cout2, out2, ldo2,
                           act=True, alpha=0.3, act2=True, alpha2=0.3, nprod=6, max_workgroups=0, out=None, ldo=0):
    """The wave-private stride-1 conv (32 -> 32) and the next level's stride-2 conv (32 -> 64) per observation in one launch:
    mean_out as conv_tile3r_forward's (the same bits), out2 [frames * kobs, h / 2, w / 2, ldo2]; the stride-1 map itself is not
    stored (`out` must stay None: the entry point refuses it)."""
    _call('nlt_conv_tile3w_s2_forward', nprod, _ptr(src), ld, cin, frames, kobs, h, w, packed.data_ptr(), _ptr(bias), cout,
          _ptr(out), ldo, _ptr(mean_out), ldm, 1 if act else 0, float(alpha), packed2.data_ptr(), _ptr(bias2), cout2,
          _ptr(out2), ldo2, 1 if act2 else 0, float(alpha2), max_workgroups)


def conv_bf16_pack(mode, w_keras, c0, c1, cout):
    return _pack('nlt_conv_bf16_packed_elems', (mode, c0, c1, cout),
                 'nlt_conv_bf16_pack', (mode, _ptr(_dense(w_keras, 'w_keras')), c0, c1, cout), torch.bfloat16, w_keras.device)


def _any_ptr(t, what):
    """(device pointer, is_fp32) of a float32 or bfloat16 CUDA tensor (or an already offset view of one)."""
    if t is None:
        return None, 0
    if not (t.is_cuda and t.dtype in (torch.float32, torch.bfloat16)):
        raise NLTError("%s: expected a float32 / bfloat16 CUDA tensor, got %s on %s" % (what, t.dtype, t.device))
    return t.data_ptr(), 1 if t.dtype == torch.float32 else 0


def conv_bf16_forward(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, w_packed, bias, cout, out, ldo, act=True, alpha=0.3, tile_hint=0):
    """src* / out: float32 or bfloat16 tensors (views into wider NHWC tensors allowed: pass the per-texel stride ld*)."""
    p0, f0 = _any_ptr(src0, 'src0')
    p1, f1 = _any_ptr(src1, 'src1')
    po, fo = _any_ptr(out, 'out')
    _call('nlt_conv_bf16_forward', mode, tile_hint, p0, ld0, c0, f0, p1, ld1, c1, f1, n, h, w,
          _tptr(w_packed, torch.bfloat16, 'w_packed'), _ptr(bias), cout, po, ldo, fo, 1 if act else 0, float(alpha))


def conv_bf16_forward_map(mode, src0, c0, ld0, src1, c1, ld1, n, h, w, w_packed, bias, cout, out, ldo, bias_map,
                          act=True, alpha=0.3, tile_hint=0):
    """out = act((conv(src0 | src1) + bias) + bias_map) on the bf16 matrix cores: conv_bf16_forward with the per-output-texel
    fp32 map [1 or n, oh, ow, cout] (dense) of the override plan (include/nlt_hip.h: nlt_conv_bf16_forward_map)."""
    p0, f0 = _any_ptr(src0, 'src0')
    p1, f1 = _any_ptr(src1, 'src1')
    po, fo = _any_ptr(out, 'out')
    _call('nlt_conv_bf16_forward_map', mode, tile_hint, p0, ld0, c0, f0, p1, ld1, c1, f1, n, h, w,
          _tptr(w_packed, torch.bfloat16, 'w_packed'), _ptr(bias), cout, po, ldo, fo, 1 if act else 0, float(alpha),
          _tptr(bias_map, torch.float32, 'bias_map'), bias_map.shape[0])


def obs_mean_bf16(obs, n, k, hw, c, out, ldo):
    if obs.dtype != torch.bfloat16 or out.dtype != torch.bfloat16:
        raise NLTError("obs_mean_bf16: bfloat16 tensors expected")
    _call('nlt_obs_mean_bf16', obs.data_ptr(), n, k, hw, c, out.data_ptr(), ldo)


# ---------------------------------------------------------------- bf16 channel mix
def chmix_bf16_pack(w_keras):
    """Keras (1,1,cin,cout) fp32 kernel -> bf16 MFMA fragments."""
    cin, cout = w_keras.shape[2], w_keras.shape[3]
    return _pack('nlt_chmix_bf16_packed_elems', (cin, cout),
                 'nlt_chmix_bf16_pack', (_ptr(_dense(w_keras, 'w_keras')), cin, cout), torch.bfloat16, w_keras.device)


def chmix_bf16_forward(x, packed, bias, cout, act=True, alpha=0.3):
    """x [..., cin] bf16 (dense NHWC) -> [..., cout] bf16."""
    cin = x.shape[-1]
    out = torch.empty(tuple(x.shape[:-1]) + (cout,), device=x.device, dtype=torch.bfloat16)
    _call('nlt_chmix_bf16_forward', _tptr(x, torch.bfloat16, 'x'), x.numel() // cin, cin, _tptr(packed, torch.bfloat16, 'packed'),
          _ptr(bias), cout, 1 if act else 0, float(alpha), out.data_ptr())
    return out


# ---------------------------------------------------------------- fused inference ends
def front_pack_weights(wq0, bq0, wo0, bo0, wqa, bqa, wqb, bqb, woa, boa, wob, bob, wh, bh, out=None):
    """out: a blob from an earlier call to refill in place (keeps its address: launch tapes, hipGraphs)."""
    if out is None:
        out = torch.empty(_size('nlt_front_packed_floats'), device=wq0.device, dtype=torch.float32)
    args = [_ptr(_dense(t, 'weight')) for t in (wq0, bq0, wo0, bo0, wqa, bqa, wqb, bqb, woa, boa, wob, bob, wh, bh)]
    _call('nlt_front_pack_weights', *args, _ptr(out))
    return out


def front_forward(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, packed, add_base, alpha, fm1, obs1, skip3):
    for t, nm in ((base, 'base'), (cvis, 'cvis'), (lvis, 'lvis'), (nn_rgb, 'nn_rgb'), (nn_base, 'nn_base')):
        _dense(t, nm)
    _call('nlt_front_forward', _ptr(base), _ptr(cvis), _ptr(lvis), _ptr(nn_rgb), _ptr(nn_base), n, k, h, w, _ptr(packed),
          1 if add_base else 0, float(alpha), _ptr(fm1), _ptr(obs1), _ptr(skip3))


def front_pack_l2_weights(wq, bq, wo, bo, out=None):
    if out is None:
        out = torch.empty(_size('nlt_front_l2_packed_floats'), device=wq.device, dtype=torch.float32)
    _call('nlt_front_pack_l2_weights', _ptr(_dense(wq, 'wq')), _ptr(bq), _ptr(_dense(wo, 'wo')), _ptr(bo), _ptr(out))
    return out


def front2_forward(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, packed, packed_l2, add_base, alpha, fm1, skip3, qtmp2, otmp2):
    for t, nm in ((base, 'base'), (cvis, 'cvis'), (lvis, 'lvis'), (nn_rgb, 'nn_rgb'), (nn_base, 'nn_base')):
        _dense(t, nm)
    _call('nlt_front2_forward', _ptr(base), _ptr(cvis), _ptr(lvis), _ptr(nn_rgb), _ptr(nn_base), n, k, h, w, _ptr(packed),
          _ptr(packed_l2), 1 if add_base else 0, float(alpha), _ptr(fm1), _ptr(skip3), _ptr(qtmp2), _ptr(otmp2))


def front4_supported(*tensors):
    """The LDS-staged front kernel loads 16-byte row pieces: every input buffer must start on a 16-byte boundary."""
    return all(t.data_ptr() % 16 == 0 for t in tensors)


def front4_forward(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, packed, packed_l2, add_base, alpha, fm1, skip3, qtmp2, otmp2,
                   waves_per_simd=0):
    for t, nm in ((base, 'base'), (cvis, 'cvis'), (lvis, 'lvis'), (nn_rgb, 'nn_rgb'), (nn_base, 'nn_base')):
        _dense(t, nm)
    _call('nlt_front4_forward', _ptr(base), _ptr(cvis), _ptr(lvis), _ptr(nn_rgb), _ptr(nn_base), n, k, h, w, _ptr(packed),
          _ptr(packed_l2), 1 if add_base else 0, float(alpha), _ptr(fm1), _ptr(skip3), _ptr(qtmp2), _ptr(otmp2),
          int(waves_per_simd))


def front4_forward_u8(diffuse_store, rgb_store, cvis_store, lvis_store, ids, nn_ids, n, k, h, w, packed, packed_l2, add_base,
                      alpha, fm1, skip3, qtmp2, otmp2, waves_per_simd=0):
    u8 = torch.uint8
    _call('nlt_front4_forward_u8', _tptr(diffuse_store, u8, 'diffuse_store'), _tptr(rgb_store, u8, 'rgb_store'),
          _tptr(cvis_store, u8, 'cvis_store'), _tptr(lvis_store, u8, 'lvis_store'), _tptr(ids, torch.int32, 'ids'),
          _tptr(nn_ids, torch.int32, 'nn_ids'), n, k, h, w, _ptr(packed), _ptr(packed_l2), 1 if add_base else 0, float(alpha),
          _ptr(fm1), _ptr(skip3), _ptr(qtmp2), _ptr(otmp2), int(waves_per_simd))


def front4_forward_train(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, packed, packed_l2, add_base, alpha, fm1, skip3, qtmp2, otmp2,
                         obs1, qtmp1, otmp1):
    """front4_forward that also keeps the level-1 maps the backward pass reads (train mode)."""
    _call('nlt_front4_forward_train', _ptr(base), _ptr(cvis), _ptr(lvis), _ptr(nn_rgb), _ptr(nn_base), n, k, h, w, _ptr(packed),
          _ptr(packed_l2), 1 if add_base else 0, float(alpha), _ptr(fm1), _ptr(skip3), _ptr(qtmp2), _ptr(otmp2), _ptr(obs1),
          _ptr(qtmp1), _ptr(otmp1))


def front_ovr_forward(base, cvis, lvis, n, h, w, packed, packed_l2, p1, s0, p2, add_base, alpha, q1, ldq, skip3, qtmp2):
    """The query-only front launch of the reference's inference mode (include/nlt_hip.h: nlt_front_ovr_forward)."""
    for t, nm in ((base, 'base'), (cvis, 'cvis'), (lvis, 'lvis'), (p1, 'p1'), (s0, 's0'), (p2, 'p2')):
        _dense(t, nm)
    _call('nlt_front_ovr_forward', _ptr(base), _ptr(cvis), _ptr(lvis), n, h, w, _ptr(packed), _ptr(packed_l2), _ptr(p1), _ptr(s0),
          _ptr(p2), 1 if add_base else 0, float(alpha), _ptr(q1), ldq, _ptr(skip3), _ptr(qtmp2))


def front_ovr_forward_u8(diffuse_store, cvis_store, lvis_store, ids, n, h, w, packed, packed_l2, p1, s0, p2, add_base, alpha, q1, ldq,
                         skip3, qtmp2):
    """front_ovr_forward on a store-resident batch: frame ids of the uint8 capture store (nlt_front_ovr_forward_u8)."""
    u8 = torch.uint8
    for t, nm in ((p1, 'p1'), (s0, 's0'), (p2, 'p2')):
        _dense(t, nm)
    _call('nlt_front_ovr_forward_u8', _tptr(diffuse_store, u8, 'diffuse_store'), _tptr(cvis_store, u8, 'cvis_store'),
          _tptr(lvis_store, u8, 'lvis_store'), _tptr(ids, torch.int32, 'ids'), n, h, w, _ptr(packed), _ptr(packed_l2), _ptr(p1),
          _ptr(s0), _ptr(p2), 1 if add_base else 0, float(alpha), _ptr(q1), ldq, _ptr(skip3), _ptr(qtmp2))


def _front_obs_sizes(frames, h, w, otmp2, sum1, sum_raw, inputs_ok):
    """The buffers of a front_obs launch hold exactly what the kernel reads and writes for (frames, h, w)."""
    if not (inputs_ok and otmp2.numel() == frames * (h // 4) * (w // 4) * 32 and sum1.numel() == (h // 2) * (w // 2) * 16
            and sum_raw.numel() == h * w * 3):
        raise NLTError("front_obs_forward: buffers do not match %d frames of %d x %d (otmp2 %s, sum1 %s, sum_raw %s)"
                       % (frames, h, w, tuple(otmp2.shape), tuple(sum1.shape), tuple(sum_raw.shape)))


def front_obs_forward(rgb, base, frames, h, w, packed, packed_l2, alpha, accumulate, otmp2, sum1, sum_raw):
    """The observation-only front launch of extract_feat (include/nlt_hip.h: nlt_front_obs_forward): otmp2 [F,h/4,w/4,32] written,
    the float64 accumulators sum1 [h/2,w/2,16] and sum_raw [h,w,3] overwritten (accumulate false) or added to."""
    f64 = torch.float64
    _front_obs_sizes(frames, h, w, otmp2, sum1, sum_raw, rgb.numel() == base.numel() == frames * h * w * 3)
    _call('nlt_front_obs_forward', _ptr(_dense(rgb, 'rgb')), _ptr(_dense(base, 'base')), frames, h, w, _ptr(packed), _ptr(packed_l2),
          float(alpha), 1 if accumulate else 0, _ptr(_dense(otmp2, 'otmp2')), _tptr(sum1, f64, 'sum1'), _tptr(sum_raw, f64, 'sum_raw'))


def front_obs_forward_u8(rgb_store, diffuse_store, ids, frames, h, w, packed, packed_l2, alpha, accumulate, otmp2, sum1, sum_raw):
    """front_obs_forward on frames ids [F] (int32; -1: zeros) of the resident uint8 capture store (nlt_front_obs_forward_u8)."""
    u8, f64 = torch.uint8, torch.float64
    _front_obs_sizes(frames, h, w, otmp2, sum1, sum_raw, tuple(rgb_store.shape[1:]) == tuple(diffuse_store.shape[1:]) == (h, w, 3)
                     and rgb_store.shape[0] == diffuse_store.shape[0] and ids.numel() == frames)
    _call('nlt_front_obs_forward_u8', _tptr(rgb_store, u8, 'rgb_store'), _tptr(diffuse_store, u8, 'diffuse_store'),
          _tptr(ids, torch.int32, 'ids'), frames, h, w, _ptr(packed), _ptr(packed_l2), float(alpha), 1 if accumulate else 0,
          _ptr(_dense(otmp2, 'otmp2')), _tptr(sum1, f64, 'sum1'), _tptr(sum_raw, f64, 'sum_raw'))


def frame_sum_accumulate(x, acc, accumulate):
    """acc [count] float64 (+)= sum over the frames of x [F, ...] float32 (count = elements of one frame), in frame order."""
    frames, count = x.shape[0], acc.numel()
    if x.numel() != frames * count:
        raise NLTError("frame_sum_accumulate: x %s does not hold frames of %d elements" % (tuple(x.shape), count))
    _call('nlt_frame_sum_accumulate', _ptr(_dense(x, 'x')), frames, count, _tptr(acc, torch.float64, 'acc'), 1 if accumulate else 0)


def frame_mean_finish(acc, total_frames, out):
    """out float32 = float32(acc / total_frames), element for element (the division in float64)."""
    if out.numel() != acc.numel():
        raise NLTError("frame_mean_finish: out has %d elements, acc %d" % (out.numel(), acc.numel()))
    _call('nlt_frame_mean_finish', _tptr(acc, torch.float64, 'acc'), acc.numel(), int(total_frames), _ptr(_dense(out, 'out')))


def frame_mean_finish_l0(sum_raw, total_frames, wo0, bo0, out):
    """out [1,h,w,16] = wo0 . (sum_raw / total_frames) + bo0: the level-0 mean of extract_feat from the raw sum [h,w,3] float64."""
    texels = sum_raw.numel() // 3
    if sum_raw.numel() != 3 * texels or out.numel() != 16 * texels or wo0.numel() != 48 or bo0.numel() != 16:
        raise NLTError("frame_mean_finish_l0: sum_raw %s, wo0 %s, bo0 %s, out %s do not fit" %
                       (tuple(sum_raw.shape), tuple(wo0.shape), tuple(bo0.shape), tuple(out.shape)))
    _call('nlt_frame_mean_finish_l0', _tptr(sum_raw, torch.float64, 'sum_raw'), texels, int(total_frames),
          _ptr(_dense(wo0, 'wo0')), _ptr(_dense(bo0, 'bo0')), _ptr(_dense(out, 'out')))


def dec_block_forward_map(x, skip, lds, n, h, w, w_s2q, w_s1, b_s1, c, alpha, bias_map, out):
    """One expanding block of the inference mode: [x 2c | query half 4c of `skip`] + bias map (include/nlt_hip.h)."""
    _call('nlt_dec_block_forward_map', _ptr(_dense(x, 'x')), _ptr(skip), lds, n, h, w, _ptr(_dense(w_s2q, 'w_s2q')),
          _ptr(_dense(w_s1, 'w_s1')), _ptr(b_s1), c, float(alpha), _ptr(_dense(bias_map, 'bias_map')), _ptr(_dense(out, 'out')))


def back_forward_map(x, q1, ldq, skip3, n, h2, w2, w_s2q, w_s1, b_s1, w_head, alpha, bias_map, pred):
    """Last expanding block + head of the inference mode: [x 8 | 16 query channels of the level-1 map] + bias map."""
    _call('nlt_back_forward_map', _ptr(_dense(x, 'x')), _ptr(q1), ldq, _ptr(_dense(skip3, 'skip3')), n, h2, w2,
          _ptr(_dense(w_s2q, 'w_s2q')), _ptr(_dense(w_s1, 'w_s1')), _ptr(b_s1), _ptr(_dense(w_head, 'w_head')), float(alpha),
          _ptr(_dense(bias_map, 'bias_map')), _ptr(_dense(pred, 'pred')))


def dec_block_forward(x, cx, skip, cs, n, h, w, w_s2, b_s2, w_s1, b_s1, c, alpha, out):
    """One expanding block (deconv k2s2 + LeakyReLU + deconv k2s1 + LeakyReLU), c = 8 or 16, intermediate in LDS."""
    _call('nlt_dec_block_forward', _ptr(_dense(x, 'x')), cx, _ptr(_dense(skip, 'skip')), cs, n, h, w, _ptr(w_s2), _ptr(b_s2),
          _ptr(w_s1), _ptr(b_s1), c, float(alpha), _ptr(out))


def back_forward(x, fm1, skip3, n, h2, w2, w_s2, b_s2, w_s1, b_s1, w_head, alpha, pred):
    _call('nlt_back_forward', _ptr(_dense(x, 'x')), _ptr(_dense(fm1, 'fm1')), _ptr(_dense(skip3, 'skip3')), n, h2, w2, _ptr(w_s2),
          _ptr(b_s2), _ptr(w_s1), _ptr(b_s1), _ptr(w_head), float(alpha), _ptr(pred))


def front_forward_train(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, packed, add_base, alpha, fm1, obs1, skip3, qtmp1, otmp1):
    for t, nm in ((base, 'base'), (cvis, 'cvis'), (lvis, 'lvis'), (nn_rgb, 'nn_rgb'), (nn_base, 'nn_base')):
        _dense(t, nm)
    _call('nlt_front_forward_train', _ptr(base), _ptr(cvis), _ptr(lvis), _ptr(nn_rgb), _ptr(nn_base), n, k, h, w, _ptr(packed),
          1 if add_base else 0, float(alpha), _ptr(fm1), _ptr(obs1), _ptr(skip3), _ptr(_dense(qtmp1, 'qtmp1')),
          _ptr(_dense(otmp1, 'otmp1')))


def back_forward_train(x, fm1, skip3, n, h2, w2, w_s2, b_s2, w_s1, b_s1, w_head, alpha, pred, u, v):
    _call('nlt_back_forward_train', _ptr(_dense(x, 'x')), _ptr(_dense(fm1, 'fm1')), _ptr(_dense(skip3, 'skip3')), n, h2, w2,
          _ptr(w_s2), _ptr(b_s2), _ptr(w_s1), _ptr(b_s1), _ptr(w_head), float(alpha), _ptr(pred), _ptr(_dense(u, 'u')),
          _ptr(_dense(v, 'v')))


def front_backward(base, cvis, lvis, nn_rgb, nn_base, n, k, h, w, dy1q, dy1o, dpred, weights, grads):
    """weights = (wq0, bq0, wo0, bo0, wqa, woa, wh); grads = (dwq0, dbq0, dwo0, dbo0, dwqa, dbqa, dwoa, dboa, dwh),
    accumulated in place (views of the flat gradient bucket)."""
    ws = _workspace('front_bwd', base.device, _size('nlt_front_backward_workspace_floats', n, h, w))
    for t, nm in ((base, 'base'), (cvis, 'cvis'), (lvis, 'lvis'), (nn_rgb, 'nn_rgb'), (nn_base, 'nn_base'),
                  (dy1q, 'dy1q'), (dy1o, 'dy1o'), (dpred, 'dpred')):
        _dense(t, nm)
    args = [_ptr(t) for t in (base, cvis, lvis, nn_rgb, nn_base)] + [n, k, h, w, _ptr(dy1q), _ptr(dy1o), _ptr(dpred)]
    args += [_ptr(_dense(t, 'weight')) for t in weights] + [_ptr(_dense(t, 'grad')) for t in grads]
    _call('nlt_front_backward', *args, _ptr(ws))


def back_backward(x, fm1, u, v, dpred, n, h2, w2, w_s2, w_s1, w_head, alpha, dx, dfm1, dw_s2, db_s2, dw_s1, db_s1, dw_head, db_head):
    """Gradients of the last expanding block + head; dx / dfm1 written, weight gradients accumulated in place."""
    ws = _workspace('back_bwd', x.device, _size('nlt_back_backward_workspace_floats', n, h2, w2))
    ins = [_ptr(_dense(t, nm)) for t, nm in ((x, 'x'), (fm1, 'fm1'), (u, 'u'), (v, 'v'), (dpred, 'dpred'))]
    wts = [_ptr(_dense(t, 'weight')) for t in (w_s2, w_s1, w_head)]
    outs = [_ptr(_dense(t, 'grad')) for t in (dx, dfm1, dw_s2, db_s2, dw_s1, db_s1, dw_head, db_head)]
    _call('nlt_back_backward', *ins, n, h2, w2, *wts, float(alpha), *outs, _ptr(ws))


# ---------------------------------------------------------------- mesh ray casting (csrc/raycast.hip)
def bvh_build(tri_verts, lo, hi):
    """tri_verts [T,3,3] float64, lo / hi the mesh's box (3 numbers each) -> (tris, nodes): the two float64 hierarchy buffers
    of include/nlt_hip.h, exactly the queried sizes.  Morton codes on the device, a stable torch.sort, then the build."""
    if tri_verts.dim() != 3 or tuple(tri_verts.shape[1:]) != (3, 3):
        raise NLTError("bvh_build: tri_verts [T,3,3] expected, got %s" % (tuple(tri_verts.shape),))
    n, dev = tri_verts.shape[0], tri_verts.device
    n_tris_d = _size('nlt_bvh_tris_doubles', n, what='1 .. 2^31 - 1 triangles')
    n_nodes_d = _size('nlt_bvh_nodes_doubles', n)
    tv = _tptr(tri_verts, torch.float64, 'tri_verts')
    codes = torch.empty(n, device=dev, dtype=torch.int32)
    _call('nlt_bvh_morton', tv, n, *(float(x) for x in lo), *(float(x) for x in hi), codes.data_ptr())
    order = torch.sort(codes, stable=True).indices.to(torch.int32)
    tris = torch.empty(n_tris_d, device=dev, dtype=torch.float64)
    nodes = torch.empty(n_nodes_d, device=dev, dtype=torch.float64)
    _call('nlt_bvh_build', tv, _tptr(order, torch.int32, 'order'), n, tris.data_ptr(), tris.numel(), nodes.data_ptr(), nodes.numel())
    return tris, nodes


def _bvh_args(tris, nodes, n_tris, tri2face):
    if tri2face is not None and tri2face.numel() != n_tris:
        raise NLTError("tri2face has %d entries for %d triangles" % (tri2face.numel(), n_tris))
    if tris.numel() != _size('nlt_bvh_tris_doubles', n_tris) or nodes.numel() != _size('nlt_bvh_nodes_doubles', n_tris):
        raise NLTError("the hierarchy buffers were not built for %d triangles" % n_tris)
    return _tptr(tris, torch.float64, 'tris'), _tptr(nodes, torch.float64, 'nodes'), n_tris


def raycast(tris, nodes, n_tris, tri2face, origins, dirs):
    """origins, dirs [R,3] float64 (directions as given) -> (t float64 [R], +inf = miss; tri int32 [R]; face int32 [R])."""
    if origins.dim() != 2 or origins.shape[1] != 3 or origins.shape != dirs.shape:
        raise NLTError("raycast: origins and dirs [R,3] expected, got %s, %s" % (tuple(origins.shape), tuple(dirs.shape)))
    r, dev = origins.shape[0], origins.device
    t = torch.empty(r, device=dev, dtype=torch.float64)
    tri = torch.empty(r, device=dev, dtype=torch.int32)
    face = torch.empty(r, device=dev, dtype=torch.int32)
    _call('nlt_raycast', *_bvh_args(tris, nodes, n_tris, tri2face), _tptr(tri2face, torch.int32, 'tri2face'),
          _tptr(origins, torch.float64, 'origins'), _tptr(dirs, torch.float64, 'dirs'), r, t.data_ptr(), tri.data_ptr(), face.data_ptr())
    return t, tri, face


def raycast_camera(tris, nodes, n_tris, tri2face, cam_mat_inv, cam_loc, imh, imw):
    """cam_mat_inv: the 16 numbers of the inverse world -> pixel matrix, row-major; cam_loc: 3 numbers ->
    (locs, normals float64 [imh*imw,3], valid uint8 [imh*imw], face_i int32 [imh*imw]), row-major pixels."""
    vals = [float(x) for x in cam_mat_inv] + [float(x) for x in cam_loc]
    if len(vals) != 19:
        raise NLTError("raycast_camera: 16 matrix entries and 3 coordinates expected")
    if getattr(_tls, 'tape', None) is not None:
        raise NLTError("raycast_camera reads its camera from host memory during the call: it cannot be recorded on a launch tape")
    host = (_c_double * 19)(*vals)
    dev, p = tris.device, int(imh) * int(imw)
    locs = torch.empty((p, 3), device=dev, dtype=torch.float64)
    normals = torch.empty((p, 3), device=dev, dtype=torch.float64)
    valid = torch.empty(p, device=dev, dtype=torch.uint8)
    face_i = torch.empty(p, device=dev, dtype=torch.int32)
    _call('nlt_raycast_camera', *_bvh_args(tris, nodes, n_tris, tri2face), _tptr(tri2face, torch.int32, 'tri2face'),
          ctypes.addressof(host), int(imh), int(imw), locs.data_ptr(), normals.data_ptr(), valid.data_ptr(), face_i.data_ptr())
    return locs, normals, valid, face_i


def raycast_shadow(tris, nodes, n_tris, locs, valid, light_loc):
    """locs [P,3] float64, valid [P] uint8, light_loc 3 numbers -> occluded uint8 [P] (data_gen/render.py:238-254)."""
    p = valid.numel()
    if locs.numel() != 3 * p:
        raise NLTError("raycast_shadow: locs %s does not match %d pixels" % (tuple(locs.shape), p))
    occluded = torch.empty(p, device=valid.device, dtype=torch.uint8)
    _call('nlt_raycast_shadow', *_bvh_args(tris, nodes, n_tris, None), _tptr(locs, torch.float64, 'locs'),
          _tptr(valid, torch.uint8, 'valid'), p, *(float(x) for x in light_loc), occluded.data_ptr())
    return occluded


def render_direct(tris, nodes, n_tris, tri_normals, tri_rgb, cam_mat_inv, cam_loc, imh, imw, spp_side, light_loc, intensity, kd, ks,
                  alpha):
    """One point light's direct lighting of the mesh (include/nlt_hip.h: nlt_render_direct).  tri_normals, tri_rgb: float64
    [n_tris,3,3] or None; camera as `raycast_camera`; light_loc, kd: 3 numbers -> (rgb_linear float32 [imh*imw,3], coverage
    float32 [imh*imw]), row-major pixels."""
    vals = [float(x) for x in cam_mat_inv] + [float(x) for x in cam_loc]
    if len(vals) != 19:
        raise NLTError("render_direct: 16 matrix entries and 3 coordinates expected")
    if getattr(_tls, 'tape', None) is not None:
        raise NLTError("render_direct reads its camera from host memory during the call: it cannot be recorded on a launch tape")
    for name, t in (('tri_normals', tri_normals), ('tri_rgb', tri_rgb)):
        if t is not None and t.numel() != 9 * n_tris:
            raise NLTError("render_direct: %s %s does not match %d triangles" % (name, tuple(t.shape), n_tris))
    host = (_c_double * 19)(*vals)
    dev, p = tris.device, int(imh) * int(imw)
    rgb = torch.empty((max(p, 0), 3), device=dev, dtype=torch.float32)
    coverage = torch.empty(max(p, 0), device=dev, dtype=torch.float32)
    _call('nlt_render_direct', *_bvh_args(tris, nodes, n_tris, None), _tptr(tri_normals, torch.float64, 'tri_normals'),
          _tptr(tri_rgb, torch.float64, 'tri_rgb'), ctypes.addressof(host), int(imh), int(imw), int(spp_side),
          *(float(x) for x in light_loc), float(intensity), *(float(x) for x in kd), float(ks), float(alpha), rgb.data_ptr(),
          coverage.data_ptr())
    return rgb, coverage


def render_global(tris, nodes, n_tris, tri_normals, tri_rgb, cam_mat_inv, cam_loc, imh, imw, spp_side, light_loc, intensity, kd, ks,
                  alpha, light_radius, light_pts, bounce_pts=None, want_indirect=True):
    """`render_direct` with a spherical light and one diffuse bounce (include/nlt_hip.h: nlt_render_global).  light_pts: float64
    [n_lsets, n_l, 3] unit vectors; bounce_pts: float64 [n_bsets, n_b, 2] points of the unit disc, or None (no bounce: n_b = 0 and
    a NULL table) -> (rgb_linear float32 [imh*imw,3], coverage float32 [imh*imw], rgb_indirect float32 [imh*imw,3] or None)."""
    vals = [float(x) for x in cam_mat_inv] + [float(x) for x in cam_loc]
    if len(vals) != 19:
        raise NLTError("render_global: 16 matrix entries and 3 coordinates expected")
    if getattr(_tls, 'tape', None) is not None:
        raise NLTError("render_global reads its camera from host memory during the call: it cannot be recorded on a launch tape")
    for name, t in (('tri_normals', tri_normals), ('tri_rgb', tri_rgb)):
        if t is not None and t.numel() != 9 * n_tris:
            raise NLTError("render_global: %s %s does not match %d triangles" % (name, tuple(t.shape), n_tris))
    if light_pts.dim() != 3 or light_pts.shape[2] != 3:
        raise NLTError("render_global: light_pts [n_lsets, n_l, 3] expected, got %s" % (tuple(light_pts.shape),))
    if bounce_pts is not None and (bounce_pts.dim() != 3 or bounce_pts.shape[2] != 2):
        raise NLTError("render_global: bounce_pts [n_bsets, n_b, 2] expected, got %s" % (tuple(bounce_pts.shape),))
    n_lsets, n_l = int(light_pts.shape[0]), int(light_pts.shape[1])
    n_bsets, n_b = (1, 0) if bounce_pts is None else (int(bounce_pts.shape[0]), int(bounce_pts.shape[1]))
    host = (_c_double * 19)(*vals)
    dev, p = tris.device, int(imh) * int(imw)
    rgb = torch.empty((max(p, 0), 3), device=dev, dtype=torch.float32)
    coverage = torch.empty(max(p, 0), device=dev, dtype=torch.float32)
    indirect = torch.empty((max(p, 0), 3), device=dev, dtype=torch.float32) if want_indirect else None
    _call('nlt_render_global', *_bvh_args(tris, nodes, n_tris, None), _tptr(tri_normals, torch.float64, 'tri_normals'),
          _tptr(tri_rgb, torch.float64, 'tri_rgb'), ctypes.addressof(host), int(imh), int(imw), int(spp_side),
          *(float(x) for x in light_loc), float(intensity), *(float(x) for x in kd), float(ks), float(alpha), float(light_radius),
          _tptr(light_pts, torch.float64, 'light_pts'), n_l, n_lsets, _tptr(bounce_pts if n_b > 0 else None, torch.float64, 'bounce_pts'),
          n_b, n_bsets, rgb.data_ptr(), coverage.data_ptr(), None if indirect is None else indirect.data_ptr())
    return rgb, coverage, indirect


# ---------------------------------------------------------------- UV unwrap (csrc/unwrap.hip)
UNWRAP_MAX_ISLAND_ROUNDS = 256


def _unwrap_mesh_args(loop_verts, face_off):
    return _tptr(loop_verts, torch.int32, 'loop_verts'), loop_verts.numel(), _tptr(face_off, torch.int32, 'face_off'), face_off.numel() - 1


def _no_tape(what):
    if getattr(_tls, 'tape', None) is not None:
        raise NLTError("%s reads a device value between its launches: it cannot be recorded on a launch tape" % what)


def unwrap_frames(verts, loop_verts, face_off):
    """verts [V,3] float64, loop_verts [L] int32, face_off [F+1] int32 (include/nlt_hip.h: nlt_unwrap_frames) ->
    (n, unit float64 [3,F], by component; area float64 [F]; ok uint8 [F])."""
    if verts.dim() != 2 or verts.shape[1] != 3 or loop_verts.dim() != 1 or face_off.dim() != 1:
        raise NLTError("unwrap_frames: verts [V,3], loop_verts [L], face_off [F+1] expected")
    lv, n_loops, fo, f = _unwrap_mesh_args(loop_verts, face_off)
    dev = verts.device
    n = torch.empty((3, max(f, 0)), device=dev, dtype=torch.float64)
    unit = torch.empty((3, max(f, 0)), device=dev, dtype=torch.float64)
    area = torch.empty(max(f, 0), device=dev, dtype=torch.float64)
    ok = torch.empty(max(f, 0), device=dev, dtype=torch.uint8)
    _call('nlt_unwrap_frames', _tptr(verts, torch.float64, 'verts'), verts.shape[0], lv, n_loops, fo, f, n.data_ptr(), unit.data_ptr(),
          area.data_ptr(), ok.data_ptr())
    return n, unit, area, ok


def _unwrap_pair(pair):
    idx, bits = (int(x) for x in pair.cpu())                        # (one read per round: the host decides whether to go on)
    return idx, _struct.unpack('<d', _struct.pack('<q', bits))[0]


def unwrap_vectors(unit, area, ok, cos_half, cos_full, aw, omw, max_groups=256):
    """The greedy projection vectors of include/nlt_hip.h (nlt_unwrap_seed, then nlt_unwrap_gather + nlt_unwrap_farthest per
    round) -> (vectors float64 [K,3], a view of a [max_groups,3] buffer; the seeds, K face indices).  ValueError: no face has
    an area, or more than max_groups vectors would be needed."""
    _no_tape('unwrap_vectors')
    f, dev = area.numel(), area.device
    need = _size('nlt_unwrap_workspace_bytes', f, what='1 .. 2^31 - 1 faces')
    ws = _workspace(_per_stream('unwrap'), dev, (need + 3) // 4)
    ws_bytes = ws.numel() * 4
    remaining = torch.empty(f, device=dev, dtype=torch.uint8)
    best = torch.empty(f, device=dev, dtype=torch.float64)
    vectors = torch.empty((int(max_groups), 3), device=dev, dtype=torch.float64)
    pair = torch.empty(2, device=dev, dtype=torch.int64)
    up, ap, okp = _tptr(unit, torch.float64, 'unit'), _tptr(area, torch.float64, 'area'), _tptr(ok, torch.uint8, 'ok')
    if unit.numel() != 3 * f or ok.numel() != f:
        raise NLTError("unwrap_vectors: unit %s, ok %s do not match %d faces" % (tuple(unit.shape), tuple(ok.shape), f))
    _call('nlt_unwrap_seed', ap, okp, f, remaining.data_ptr(), ws.data_ptr(), ws_bytes, pair.data_ptr())
    seed, _ = _unwrap_pair(pair)
    if seed < 0:
        raise ValueError("the mesh has no face with a finite, non-zero area: nothing to unwrap")
    seeds = []
    while True:
        k = len(seeds)
        if k >= max_groups:
            raise ValueError("more than max_groups = %d projection vectors are needed at this angle limit" % max_groups)
        vec = vectors.data_ptr() + 24 * k
        _call('nlt_unwrap_gather', up, ap, remaining.data_ptr(), f, seed, float(cos_half), float(aw), float(omw), ws.data_ptr(), ws_bytes, vec)
        _call('nlt_unwrap_farthest', up, okp, remaining.data_ptr(), best.data_ptr(), f, vec, 1 if k == 0 else 0, ws.data_ptr(), ws_bytes,
              pair.data_ptr())
        seeds.append(seed)
        seed, value = _unwrap_pair(pair)
        if seed < 0 or value >= cos_full:
            return vectors[:len(seeds)], seeds


def unwrap_assign(unit, ok, vectors):
    """unit [3,F], ok [F], vectors [K,3] -> group int32 [F] (nlt_unwrap_assign)."""
    f = ok.numel()
    group = torch.empty(f, device=ok.device, dtype=torch.int32)
    _call('nlt_unwrap_assign', _tptr(unit, torch.float64, 'unit'), _tptr(ok, torch.uint8, 'ok'), f,
          _tptr(vectors, torch.float64, 'vectors'), vectors.shape[0], group.data_ptr())
    return group


def unwrap_islands(loop_verts, face_off, n_verts, group, max_rounds=UNWRAP_MAX_ISLAND_ROUNDS):
    """Edge keys, a stable torch.sort (plumbing, as in `bvh_build`), then hooking rounds until the device flag reports no change
    -> (label int32 [F]: the smallest face index of the face's island, -1 degenerate; loop_face int32 [L]; the rounds run).
    More than max_rounds rounds raise NLTError."""
    _no_tape('unwrap_islands')
    lv, n_loops, fo, f = _unwrap_mesh_args(loop_verts, face_off)
    dev = loop_verts.device
    keys = torch.empty(max(n_loops, 0), device=dev, dtype=torch.int64)
    loop_face = torch.empty(max(n_loops, 0), device=dev, dtype=torch.int32)
    label = torch.empty(max(f, 0), device=dev, dtype=torch.int32)
    changed = torch.empty(1, device=dev, dtype=torch.int32)
    gp = _tptr(group, torch.int32, 'group')
    _call('nlt_unwrap_edge_keys', lv, n_loops, fo, f, int(n_verts), keys.data_ptr(), loop_face.data_ptr())
    keys_sorted, order = torch.sort(keys, stable=True)
    _call('nlt_unwrap_islands_init', gp, f, label.data_ptr())
    for rounds in range(1, int(max_rounds) + 1):
        _call('nlt_unwrap_islands_round', _tptr(keys_sorted, torch.int64, 'keys_sorted'), _tptr(order, torch.int64, 'order'),
              loop_face.data_ptr(), n_loops, gp, f, label.data_ptr(), changed.data_ptr())
        if int(changed.cpu()[0]) == 0:
            return label, loop_face, rounds
    raise NLTError("unwrap_islands: the labels still changed after %d rounds" % max_rounds)


def unwrap_boxes(verts, loop_verts, loop_face, group, island, frames, n_islands):
    """frames [K,2,3] float64, island int32 [F] -> (puv float64 [L,2], boxes float64 [n_islands,4]) (nlt_unwrap_boxes)."""
    n_loops, f, dev = loop_verts.numel(), group.numel(), verts.device
    if frames.dim() != 3 or tuple(frames.shape[1:]) != (2, 3) or island.numel() != f or loop_face.numel() != n_loops:
        raise NLTError("unwrap_boxes: frames [K,2,3], island [F], loop_face [L] expected")
    puv = torch.empty((n_loops, 2), device=dev, dtype=torch.float64)
    boxes = torch.empty((max(int(n_islands), 0), 4), device=dev, dtype=torch.float64)
    _call('nlt_unwrap_boxes', _tptr(verts, torch.float64, 'verts'), _tptr(loop_verts, torch.int32, 'loop_verts'),
          _tptr(loop_face, torch.int32, 'loop_face'), n_loops, _tptr(group, torch.int32, 'group'), _tptr(island, torch.int32, 'island'), f,
          _tptr(frames, torch.float64, 'frames'), frames.shape[0], puv.data_ptr(), boxes.data_ptr(), int(n_islands))
    return puv, boxes


def unwrap_uv(puv, face_off, island, boxes, rot, offsets, scale, vmax):
    """puv [L,2], boxes [I,4], rot uint8 [I], offsets [I,2] -> the dense uv float64 [F,vmax,2] (nlt_unwrap_uv)."""
    f, n_islands = face_off.numel() - 1, boxes.shape[0]
    if rot.numel() != n_islands or offsets.numel() != 2 * n_islands or island.numel() != f:
        raise NLTError("unwrap_uv: rot [I], offsets [I,2] and island [F] must match boxes [I,4] and face_off [F+1]")
    uv = torch.empty((max(f, 0), int(vmax), 2), device=puv.device, dtype=torch.float64)
    _call('nlt_unwrap_uv', _tptr(puv, torch.float64, 'puv'), puv.shape[0], _tptr(face_off, torch.int32, 'face_off'),
          _tptr(island, torch.int32, 'island'), f, _tptr(boxes, torch.float64, 'boxes'), _tptr(rot, torch.uint8, 'rot'),
          _tptr(offsets, torch.float64, 'offsets'), n_islands, float(scale), int(vmax), uv.data_ptr())
    return uv


# ---------------------------------------------------------------- texel-buffer assembly
_MAP_DTYPES = {torch.float64: MAP_F64, torch.float32: MAP_F32, torch.float16: MAP_F16}


def cosine_map(locs, normals, valid, occluded, src_loc, want_float=True, want_u8=True):
    """locs/normals [...,3] float64, valid/occluded [...] uint8 -> (cos float64, quantised uint8)."""
    shape = valid.shape
    pixels = valid.numel()
    cos = torch.empty(shape, device=valid.device, dtype=torch.float64) if want_float else None
    q = torch.empty(shape, device=valid.device, dtype=torch.uint8) if want_u8 else None
    sx, sy, sz = (float(x) for x in src_loc)
    _call('nlt_cosine_map', _tptr(locs, torch.float64, 'locs'), _tptr(normals, torch.float64, 'normals'),
          _tptr(valid, torch.uint8, 'valid'), _tptr(occluded, torch.uint8, 'occluded'), sx, sy, sz, pixels,
          _tptr(cos, torch.float64, 'cos'), _tptr(q, torch.uint8, 'q'))
    return cos, q


def albedo(rgb_frames):
    """rgb_frames [F,H,W,3] uint8 -> albedo [H,W,3] float64."""
    f = rgb_frames.shape[0]
    elems = rgb_frames[0].numel()
    out = torch.empty(rgb_frames.shape[1:], device=rgb_frames.device, dtype=torch.float64)
    ws = torch.empty(1, device=rgb_frames.device, dtype=torch.int64)
    _call('nlt_albedo', _tptr(rgb_frames, torch.uint8, 'rgb_frames'), f, elems, out.data_ptr(), ws.data_ptr())
    return out


def diffuse_base(albedo_, lvis):
    """albedo [H,W,3] float64, lvis [F,H,W] uint8 -> diffuse [F,H,W,3] uint8."""
    f = lvis.shape[0]
    texels = lvis[0].numel()
    out = torch.empty(tuple(lvis.shape) + (3,), device=lvis.device, dtype=torch.uint8)
    _call('nlt_diffuse_base', _tptr(albedo_, torch.float64, 'albedo'), _tptr(lvis, torch.uint8, 'lvis'), f, texels, out.data_ptr())
    return out


def remap_bilinear(src, mapping, force_kbg=True):
    """src [h,w] or [h,w,c] uint8 / float32; mapping [oh,ow,>=2] float64/32/16 in [0,1] -> [oh,ow(,c)]."""
    if mapping.dtype not in _MAP_DTYPES:
        raise NLTError("mapping dtype %s" % mapping.dtype)
    squeeze = src.dim() == 2
    h, w = src.shape[:2]
    c = 1 if squeeze else src.shape[2]
    oh, ow, ldm = mapping.shape
    out = torch.empty((oh, ow) if squeeze else (oh, ow, c), device=src.device, dtype=src.dtype)
    name = {torch.uint8: 'nlt_remap_bilinear_u8', torch.float32: 'nlt_remap_bilinear_f32'}.get(src.dtype)
    if name is None:
        raise NLTError("remap source dtype %s" % src.dtype)
    _call(name, _tptr(src, src.dtype, 'src'), h, w, c, _tptr(mapping, mapping.dtype, 'mapping'), _MAP_DTYPES[mapping.dtype],
          ldm, oh, ow, 1 if force_kbg else 0, out.data_ptr())
    return out


def capture_camspc(locs, normals, valid, occluded, cam_loc, light_loc, alpha, uv2cam):
    """One launch over the camera pixels (data_gen/render.py:155-171).  locs/normals [imh*imw,3] float64, valid / occluded
    (or None) [imh*imw] uint8, alpha [imh,imw] uint8 (or None: nothing masked), uv2cam [imh,imw,2] float64 ->
    (cvis_camspc, lvis_camspc uint8 [imh,imw], masked uv2cam float16 [imh,imw,2], uv2cam.png uint8 [imh,imw,3])."""
    if uv2cam.dim() != 3 or uv2cam.shape[2] != 2 or valid.numel() != uv2cam.shape[0] * uv2cam.shape[1]:
        raise NLTError("capture_camspc: uv2cam %s does not cover the %d pixels of `valid`" % (tuple(uv2cam.shape), valid.numel()))
    imh, imw = uv2cam.shape[:2]
    if alpha is not None and tuple(alpha.shape) != (imh, imw):
        raise NLTError("capture_camspc: alpha %s is not [%d,%d]" % (tuple(alpha.shape), imh, imw))
    dev, u8 = valid.device, torch.uint8
    cvis = torch.empty((imh, imw), device=dev, dtype=u8)
    lvis = torch.empty((imh, imw), device=dev, dtype=u8)
    f16 = torch.empty((imh, imw, 2), device=dev, dtype=torch.float16)
    png = torch.empty((imh, imw, 3), device=dev, dtype=u8)
    _call('nlt_capture_camspc', _tptr(locs, torch.float64, 'locs'), _tptr(normals, torch.float64, 'normals'),
          _tptr(valid, u8, 'valid'), _tptr(occluded, u8, 'occluded'), *(float(x) for x in cam_loc), *(float(x) for x in light_loc),
          _tptr(alpha, u8, 'alpha'), _tptr(uv2cam, torch.float64, 'uv2cam'), imh, imw, cvis.data_ptr(), lvis.data_ptr(),
          f16.data_ptr(), png.data_ptr())
    return cvis, lvis, f16, png


def capture_uvspc(cam2uv, cvis_camspc, lvis_camspc, rgb_camspc=None):
    """One launch over the UV texels (data_gen/render.py:157,159,173-179).  cam2uv [uvh,uvw,>=2] float64; cvis_camspc,
    lvis_camspc [imh,imw] uint8; rgb_camspc [imh,imw,3|4] uint8 or None -> (cvis, lvis uint8 [uvh,uvw], rgb uint8 [uvh,uvw,3]
    or None, cam2uv float16 [uvh,uvw,2], cam2uv.png uint8 [uvh,uvw,3])."""
    if cam2uv.dim() != 3 or cvis_camspc.dim() != 2 or lvis_camspc.shape != cvis_camspc.shape:
        raise NLTError("capture_uvspc: cam2uv %s, cvis_camspc %s, lvis_camspc %s" % tuple(tuple(t.shape) for t in (cam2uv, cvis_camspc, lvis_camspc)))
    uvh, uvw, ldm = cam2uv.shape
    imh, imw = cvis_camspc.shape
    if rgb_camspc is not None and (rgb_camspc.dim() != 3 or tuple(rgb_camspc.shape[:2]) != (imh, imw)):
        raise NLTError("capture_uvspc: rgb_camspc %s is not [%d,%d,3|4]" % (tuple(rgb_camspc.shape), imh, imw))
    dev, u8 = cam2uv.device, torch.uint8
    cvis = torch.empty((uvh, uvw), device=dev, dtype=u8)
    lvis = torch.empty((uvh, uvw), device=dev, dtype=u8)
    rgb = torch.empty((uvh, uvw, 3), device=dev, dtype=u8) if rgb_camspc is not None else None
    f16 = torch.empty((uvh, uvw, 2), device=dev, dtype=torch.float16)
    png = torch.empty((uvh, uvw, 3), device=dev, dtype=u8)
    _call('nlt_capture_uvspc', _tptr(cam2uv, torch.float64, 'cam2uv'), ldm, uvh, uvw, _tptr(cvis_camspc, u8, 'cvis_camspc'),
          _tptr(lvis_camspc, u8, 'lvis_camspc'), _tptr(rgb_camspc, u8, 'rgb_camspc'), 0 if rgb_camspc is None else rgb_camspc.shape[2],
          imh, imw, cvis.data_ptr(), lvis.data_ptr(), _tptr(rgb, u8, 'rgb'), f16.data_ptr(), png.data_ptr())
    return cvis, lvis, rgb, f16, png


def diffuse_bases(albedo_, lvis, uv2cam):
    """One launch for all frames (data_gen/postproc.py:66-82).  albedo [H,W,3] float64, lvis [F,H,W] uint8, uv2cam
    [F,imh,imw,2] float16 (as stored) -> (diffuse uint8 [F,H,W,3], diffuse_camspc uint8 [F,imh,imw,3])."""
    if lvis.dim() != 3 or uv2cam.dim() != 4 or uv2cam.shape[0] != lvis.shape[0] or uv2cam.shape[3] != 2 \
            or tuple(albedo_.shape) != tuple(lvis.shape[1:]) + (3,):
        raise NLTError("diffuse_bases: albedo %s, lvis %s, uv2cam %s" % tuple(tuple(t.shape) for t in (albedo_, lvis, uv2cam)))
    f, h, w = lvis.shape
    imh, imw = uv2cam.shape[1:3]
    diffuse = torch.empty((f, h, w, 3), device=lvis.device, dtype=torch.uint8)
    cam = torch.empty((f, imh, imw, 3), device=lvis.device, dtype=torch.uint8)
    _call('nlt_diffuse_bases', _tptr(albedo_, torch.float64, 'albedo'), _tptr(lvis, torch.uint8, 'lvis'),
          _tptr(uv2cam, torch.float16, 'uv2cam'), f, h, w, imh, imw, diffuse.data_ptr(), cam.data_ptr())
    return diffuse, cam


def uv_index_map(uvs, values, h, w, max_l1=4, fill=0.0, want_index=False):
    """uvs [P,2], values [P,M] float64 -> grid [h,w,M] float64 (+ int32 sample-index map)."""
    p, m = values.shape
    ws = torch.empty((_size('nlt_uv_index_map_workspace_bytes', h, w, p) + 3) // 4, device=uvs.device, dtype=torch.int32)
    out = torch.empty((h, w, m), device=uvs.device, dtype=torch.float64)
    idx = torch.empty((h, w), device=uvs.device, dtype=torch.int32) if want_index else None
    _call('nlt_uv_index_map', _tptr(uvs, torch.float64, 'uvs'), _tptr(values, torch.float64, 'values'), p, m, h, w, int(max_l1),
          float(fill), ws.data_ptr(), out.data_ptr(), _tptr(idx, torch.int32, 'index_out'))
    return (out, idx) if want_index else out


def knn_indices(ref_pos, cand_pos, k=1):
    """ref_pos [P,3], cand_pos [Q,3] float64 -> int32 [P,k]."""
    p, q = ref_pos.shape[0], cand_pos.shape[0]
    out = torch.empty((p, k), device=ref_pos.device, dtype=torch.int32)
    _call('nlt_knn_indices', _tptr(ref_pos, torch.float64, 'ref_pos'), p, _tptr(cand_pos, torch.float64, 'cand_pos'), q, k,
          out.data_ptr())
    return out


def psnr_sums(im1, im2, mask=None):
    """im1 / im2 [H,W] or [H,W,C] float32 (C = 1 or 3), mask [H,W] uint8 or None -> (sum of squared luma differences,
    number of pixels counted) as a float64 CUDA tensor [2]."""
    _same_shape(im1, im2, 'psnr_sums')
    c = 1 if im1.dim() == 2 else im1.shape[2]
    pixels = im1.numel() // c
    if mask is not None and mask.numel() != pixels:
        raise NLTError("psnr_sums: mask has %d pixels, the images %d" % (mask.numel(), pixels))
    ws = torch.empty(512, device=im1.device, dtype=torch.float64)
    out = torch.empty(2, device=im1.device, dtype=torch.float64)
    _call('nlt_psnr_sums', _ptr(_dense(im1, 'im1')), _ptr(_dense(im2, 'im2')), _tptr(mask, torch.uint8, 'mask'), pixels, c,
          ws.data_ptr(), out.data_ptr())
    return out


def gather_frames_u8(store, ids, out=None):
    """store [F,...] uint8, ids [n] int32 (-1 -> zeros) -> float32 [n,...] = float32(float64(u8) / 255).
    out: a persistent destination of that shape (a loader's staging ring) instead of a fresh tensor."""
    n = ids.numel()
    shape = (n,) + tuple(store.shape[1:])
    if out is None:
        out = torch.empty(shape, device=store.device, dtype=torch.float32)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise NLTError("gather_frames_u8: out must be a contiguous float32 tensor of shape %s" % (shape,))
    _call('nlt_gather_frames_u8', _tptr(store, torch.uint8, 'store'), _tptr(ids, torch.int32, 'ids'), n, store[0].numel(),
          _ptr(out))
    return out


def assemble_batch(diffuse_store, rgb_store, cvis_store, lvis_store, ids, nn_ids, test_mode=False, out=None):
    """uint8 stores [F,H,W,3] / [F,H,W]; ids [N] int32; nn_ids [N,k] int32 -> dict of float32 buffers.
    out: the dict of an earlier call with the same shapes, refilled in place (a loader's staging ring)."""
    n = ids.numel()
    k = 0 if nn_ids is None else nn_ids.shape[1]
    _, h, w = cvis_store.shape
    dev = cvis_store.device
    E = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
    if out is None:
        out = {'base': E(n, h, w, 3), 'cvis': E(n, h, w, 1), 'lvis': E(n, h, w, 1), 'rgb': E(n, h, w, 3),
               'nn_base': E(n, k, h, w, 3) if k else None, 'nn_rgb': E(n, k, h, w, 3) if k else None}
    elif tuple(out['base'].shape) != (n, h, w, 3) or (k and tuple(out['nn_rgb'].shape) != (n, k, h, w, 3)):
        raise NLTError("assemble_batch: `out` was made for another batch shape")
    u8 = torch.uint8
    _call('nlt_assemble_batch', _tptr(diffuse_store, u8, 'diffuse_store'), _tptr(rgb_store, u8, 'rgb_store'),
          _tptr(cvis_store, u8, 'cvis_store'), _tptr(lvis_store, u8, 'lvis_store'), _tptr(ids, torch.int32, 'ids'),
          _tptr(nn_ids, torch.int32, 'nn_ids'), n, k, h * w, 1 if test_mode else 0,
          *[_ptr(out[x]) for x in ('base', 'cvis', 'lvis', 'rgb', 'nn_base', 'nn_rgb')])
    return out
