"""ctypes binding of ``lib/libseam_hip.so`` (the C ABI declared in ``include/seam_hip.h``).

There is NO fallback: if the shared library is missing or a symbol cannot be
resolved, importing/using the product path raises.  Build it with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C seam-match-rcnn_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

# torch bundles its own HIP runtime (soname libamdhip64.so.7).  It MUST be in the process before
# libseam_hip.so is dlopen'ed, so that the library binds to the same runtime instance torch uses
# (loading /opt/rocm's copy first gives two runtimes and "no ROCm-capable device" at launch).
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SEAM_LIB_PATH") or os.path.join(_HERE, "lib", "libseam_hip.so")   # env: kernel experiments only

_p = C.c_void_p
_i = C.c_int
_f = C.c_float
_i64 = C.c_int64

class TrunkLayer(C.Structure):
    """seam_trunk_layer_t of include/seam_hip.h."""
    _fields_ = [("w", C.c_void_p), ("u", C.c_void_p), ("u24", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p)]


SGD_MAX_SLOTS = 32      # SEAM_SGD_MAX_SLOTS
SGD_FP_SLOTS = 64       # SEAM_SGD_FP_SLOTS


class SgdTensor(C.Structure):
    """seam_sgd_tensor_t of include/seam_hip.h."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("buf", C.c_void_p), ("numel", C.c_int64), ("group", C.c_int), ("slot", C.c_int)]


class SgdChunk(C.Structure):
    """seam_sgd_chunk_t of include/seam_hip.h."""
    _fields_ = [("tensor", C.c_int), ("count", C.c_int), ("offset", C.c_int64)]


class SgdGroup(C.Structure):
    """seam_sgd_group_t of include/seam_hip.h."""
    _fields_ = [("lr", C.c_float), ("momentum", C.c_float), ("one_minus_dampening", C.c_float), ("weight_decay", C.c_float),
                ("nesterov", C.c_int), ("maximize", C.c_int), ("first", C.c_int), ("reserved", C.c_int)]


class SgdGroups(C.Structure):
    """seam_sgd_groups_t of include/seam_hip.h."""
    _fields_ = [("n", C.c_int), ("reserved", C.c_int * 3), ("g", SgdGroup * SGD_MAX_SLOTS)]


class ClipRecord(C.Structure):
    """seam_clip_record_t of include/seam_hip.h (six int32 words on the device: norm, coefficient, finite, pad, 64-bit count)."""
    _fields_ = [("total_norm", C.c_float), ("clip_coef", C.c_float), ("finite", C.c_int), ("reserved", C.c_int),
                ("nonfinite_steps", C.c_uint64)]


REPACK_IGEMM, REPACK_WINO, REPACK_WINO24, REPACK_PC, REPACK_SW, REPACK_SPLIT3, REPACK_NARROW, REPACK_SXPC, REPACK_SXPC64, REPACK_W24SX = range(10)     # SEAM_REPACK_*


class RepackJob(C.Structure):
    """seam_repack_job_t of include/seam_hip.h."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("scale", C.c_void_p), ("items", C.c_int64),
                ("form", C.c_int), ("K", C.c_int), ("Cin", C.c_int), ("R", C.c_int), ("S", C.c_int), ("Cstore", C.c_int), ("mode", C.c_int),
                ("kred", C.c_int), ("rows", C.c_int), ("first_block", C.c_int), ("n_blocks", C.c_int), ("reserved", C.c_int)]


# name -> (restype, argtypes); mirrors include/seam_hip.h one to one
SIGNATURES = {
    "seam_version": (_i, []),
    "seam_fastdiv_exact": (_i, [C.c_uint, C.c_ulonglong]),
    "seam_error_string": (C.c_char_p, [_i]),
    "seam_option_count": (_i, []),
    "seam_option_name": (C.c_char_p, [_i]),
    "seam_set_option": (_i, [C.c_char_p, _i]),
    "seam_get_option": (_i, [C.c_char_p, C.POINTER(_i)]),
    "seam_conv_kred": (_i, [_i, _i, _i]),
    "seam_conv_rows_padded": (_i, [_i]),
    "seam_conv_tile": (_i, [_i, _i]),
    "seam_conv_tile_prec": (_i, [_i, _i, _i]),
    "seam_conv_tile_taps": (_i, [_i, _i, _i, _i]),
    "seam_pack_conv_weight_f32": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv2d_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_linear_narrow_supported": (_i, [_i, _i]),
    "seam_pack_linear_narrow_f32": (_i, [_p, _p, _i, _i, _p]),
    "seam_linear_narrow_f32": (_i, [_p, _p, _p, _p, C.c_longlong, _i, _i, _i, _p]),
    "seam_conv2d_crop_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv2d_crop_f16": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_preprocess_s2d_batch_f32": (_i, [_p, C.c_size_t, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_preprocess_s2d_batch_f16": (_i, [_p, C.c_size_t, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_preprocess_s2d_pad_batch_f16": (_i, [_p, C.c_size_t, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_preprocess_s2d_pad_batch_f32": (_i, [_p, C.c_size_t, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv2d_dual_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv1x1_pc_supported": (_i, [C.c_longlong, _i, _i]),
    "seam_conv1x1_pc_weight_floats": (C.c_longlong, [_i, _i]),
    "seam_pack_conv1x1_pc_f32": (_i, [_p, _p, _i, _i, _p]),
    "seam_conv1x1_pc_f32": (_i, [_p, _p, _p, _p, _p, _p, C.c_longlong, _i, _i, _i, _p]),
    "seam_conv1x1_sw_config": (_i, [_i, _i, _i, _i]),
    "seam_conv1x1_sw_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv1x1_swh_config": (_i, [C.c_longlong, _i, _i, _i]),
    "seam_conv1x1_f16pc_supported": (_i, [C.c_longlong, _i, _i]),
    "seam_conv1x1_f16pc_weight_halves": (C.c_longlong, [_i, _i]),
    "seam_pack_conv1x1_weight_f16pc": (_i, [_p, _p, _i, _i, _p]),
    "seam_conv1x1_f16pc": (_i, [_p, _p, _p, _p, _p, _p, C.c_longlong, _i, _i, _i, _p]),
    "seam_conv1x1_sxpc_supported": (_i, [C.c_longlong, _i, _i]),
    "seam_conv1x1_sxpc_weight_bytes": (C.c_longlong, [_i, _i]),
    "seam_pack_conv1x1_weight_sxpc": (_i, [_p, _p, _i, _i, _p]),
    "seam_conv1x1_sxpc": (_i, [_p, _p, _p, _p, _p, _p, C.c_longlong, _i, _i, _i, _p]),
    "seam_conv1x1_sxpc_dual_supported": (_i, [C.c_longlong, _i, _i, _i]),
    "seam_conv1x1_sxpc_dual": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv1x1_sxpc_up_supported": (_i, [C.c_longlong, _i, _i, _i, _i, _i, _i, _i]),
    "seam_conv1x1_sxpc_up": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv1x1_sxpc64_supported": (_i, [C.c_longlong, _i, _i]),
    "seam_pack_conv1x1_weight_sxpc64": (_i, [_p, _p, _i, _i, _p]),
    "seam_conv1x1_sxpc64": (_i, [_p, _p, _p, _p, _p, _p, C.c_longlong, _i, _i, _i, _p]),
    "seam_conv1x1_sxpc_short_supported": (_i, [C.c_longlong, _i, _i]),
    "seam_pack_conv1x1_weight_sxpc_short": (_i, [_p, _p, _i, _i, _p]),
    "seam_conv1x1_sxpc_short": (_i, [_p, _p, _p, _p, _p, _p, C.c_longlong, _i, _i, _i, _p]),
    "seam_conv1x1_sxpc_dual_short_supported": (_i, [C.c_longlong, _i, _i, _i]),
    "seam_conv1x1_sxpc_dual_short": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_stem_sxpc_supported": (_i, [_i, _i, _i]),
    "seam_stem_sxpc": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "seam_conv1x1_swh_f16": (_i, [_p, _p, _p, _p, _p, _p, _p, C.c_longlong, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_stem_s2d_swh_f16": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p]),
    "seam_conv2d_dual_f16": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv2d_upres_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_pack_conv_weight_bx3": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv2d_bx3": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_pack_conv_weight_sx": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv2d_sx": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_wino_supported": (_i, [_i, _i, _i, _i, _i]),
    "seam_wino_weight_floats": (C.c_longlong, [_i, _i]),
    "seam_wino_slot_fill_pct": (_i, [_i, _i, _i, _i, _i, _i]),
    "seam_wino_tile_variant": (_i, [_i, _i, _i, _i, _i, _i]),
    "seam_pack_conv_weight_wino_f32": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "seam_wino_issue_slots": (C.c_longlong, [_i, _i, _i, _i, _i, _i]),
    "seam_wino24_issue_slots": (C.c_longlong, [_i, _i, _i, _i, _i, _i]),
    "seam_wino24_variant": (_i, [_i, _i, _i, _i, _i, _i]),
    "seam_wino24_form": (_i, [_i, _i, _i, _i, _i, _i]),
    "seam_wino24_weight_floats": (C.c_longlong, [_i, _i]),
    "seam_pack_conv_weight_wino24_f32": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "seam_conv3x3_wino24_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_wino24sx_weight_bytes": (C.c_longlong, [_i, _i]),
    "seam_pack_conv_weight_wino24_sx": (_i, [_p, _p, _i, _i, _i, _i, _p]),
    "seam_conv3x3_wino24sx_supported": (_i, [_i, _i, _i, _i, _i, _i, _i]),
    "seam_conv3x3_wino24sx_blocks": (C.c_longlong, [_i, _i, _i, _i, _i, _i]),
    "seam_conv3x3_wino24sx_set_nsplit": (_i, [_i]),
    "seam_conv3x3_wino24sx_get_nsplit": (_i, []),
    "seam_wino24_layout": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_i)]),
    "seam_conv3x3_wino24sx_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv3x3_wino_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv3x3_f16pc_supported": (_i, [_i, _i, _i, _i, _i, _i]),
    "seam_conv3x3_f16pc_pays": (_i, [_i, _i, _i, _i, _i, _i]),
    "seam_f16pc_weight_halves": (C.c_longlong, [_i, _i]),
    "seam_pack_conv_weight_f16pc": (_i, [_p, _p, _i, _i, _i, _p]),
    "seam_conv3x3_f16pc": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv_kred_f16": (_i, [_i, _i, _i]),
    "seam_pack_conv_weight_f16": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "seam_conv2d_f16": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_preprocess_f32": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "seam_preprocess_batch_f32": (_i, [_p, C.c_size_t, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_preprocess_batch_f16": (_i, [_p, C.c_size_t, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_preprocess_u8": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_preprocess_f16": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "seam_maxpool2d_f16": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_upsample_add_f16": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "seam_roi_align_f16": (_i, [_p, _p, _p, _p, C.POINTER(_i), _i, _f, _f, _f, _f, _i, _p, _p, _p, _i, _i, _i, _p]),
    "seam_roi_align_set_lds": (None, [_i]),
    "seam_nchw_f32_to_nhwc_f16": (_i, [_p, _p, _i, _i, _i, _p]),
    "seam_nhwc_f16_to_nchw_f32": (_i, [_p, _p, _i, _i, _i, _p]),
    "seam_avgpool_f16": (_i, [_p, _p, _i, _i, _i, _p]),
    "seam_mask_select_f16": (_i, [_p, _p, _p, _i, _i, _p]),
    "seam_maxpool2d_f32": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    "seam_maxpool2d_fast": (_i, [_i, _i, _i, _i, _i, _i, _i, _i]),
    "seam_upsample_add_f32": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "seam_roi_align_f32": (_i, [_p, _p, _p, _p, C.POINTER(_i), _i, _f, _f, _f, _f, _i, _p, _p, _p, _i, _i, _i, _p]),
    "seam_nchw_to_nhwc_f32": (_i, [_p, _p, _i, _i, _i, _p]),
    "seam_nhwc_to_nchw_f32": (_i, [_p, _p, _i, _i, _i, _p]),
    "seam_avgpool_f32": (_i, [_p, _p, _i, _i, _i, _p]),
    "seam_nlb_workspace_floats": (_i64, [_i, _i]),
    "seam_nlb_attnpool_f32": (_i, [_p, _i64, _i64, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p]),
    "seam_nlb_mfma_max_len": (_i, []),
    "seam_nlb_attnpool_mfma_f32": (_i, [_p, _i64, _i64, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _p]),
    "seam_pair_logits_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "seam_rank_topk_max_k": (_i, []),
    "seam_rank_topk_f32": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "seam_match_scores_f32": (_i, [_p, _p, _i64, _p]),
    "seam_host_build_tracklets": (_i, [_p, _p, _p, _p, _i, C.c_double, _p, _p, _p]),
    "seam_build_tracklets_max_rows": (_i, []),
    "seam_build_tracklets_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, C.c_double, _p, _p, _p, _p, _p]),
    "seam_pair_scores_blockdiag_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "seam_rank_of_f32": (_i, [_p, _p, _p, _i, _i, _p]),
    "seam_score_reduce_f32": (_i, [_p, _p, _i, _i, _i, _p]),
    "seam_score_reduce_seg_f32": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "seam_rank_of_scores_f32": (_i, [_p, _p, _p, _i, _i, _p]),
    "seam_box_iou_f32": (_i, [_p, _p, _p, _i, _i, _p]),
    "seam_gt_select_f32": (_i, [_p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _i, _p]),
    "seam_pair_topk_workspace_floats": (_i64, [_i, _i, _i]),
    "seam_pair_topk_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p]),
    "seam_match_trunk_workspace_floats": (_i64, [_i]),
    "seam_match_trunk_f32": (_i, [_p, C.POINTER(TrunkLayer), C.POINTER(TrunkLayer), _p, _i, _p, C.POINTER(_i), _p]),
    "seam_pair_topk_mfma_min_gallery": (_i, []),
    "seam_pair_topk_mfma_max_k": (_i, []),
    "seam_pair_topk_mfma_workspace_floats": (_i64, [_i, _i, _i]),
    "seam_pair_topk_mfma_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _i, _p, _p]),
    "seam_decode_boxes_f32": (_i, [_p, _p, _p, _i, _i, _f, _f, _f, _f, _f, _f, _p]),
    "seam_nms_sorted_f32": (_i, [_p, _p, _i, _i, _f, _p, _p]),
    "seam_nms_sorted_topn_f32": (_i, [_p, _p, _i, _i, _f, _i, _p, _p]),
    "seam_rpn_topk_max": (_i, []),
    "seam_rpn_topk_decode_f32": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i64, _i, _i64, _i, _i64, _i, _p]),
    "seam_paste_masks_f32": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "seam_mask_inter_f32": (_i, [_p, _p, _i, _p, _i, _i, _i, _p, _p, _p]),
    "seam_mask_select_f32": (_i, [_p, _p, _p, _i, _i, _p]),
    "seam_conv_wgrad_workspace_floats": (_i64, [_i, _i, _i, _i, _i]),
    "seam_conv_wgrad_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p]),
    "seam_conv_wgrad_crop_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p]),
    "seam_colsum_workspace_floats": (_i64, [_i, _i]),
    "seam_colsum_f32": (_i, [_p, _p, _i, _i, _p, _p]),
    "seam_avgpool_relu_bwd_f32": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "seam_bn1d_train_fwd_f32": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _f, _f, _p]),
    "seam_bn1d_bwd_f32": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "seam_frame_noise_u8": (_i, [_p, _p, _p, _i, _i, C.c_double, C.c_uint64, _p]),
    "seam_noise_u8_batch": (_i, [_p, _i64, _p, _p, _p, _p, _p, _p, _i, _p]),
    "seam_frames_prepare_batch_u8": (_i, [_p, _i64, _p, _p, _p, _p, _p, _p, _i64, _p, _i64, _p, _i, _i, _i, _p]),
    "seam_resize_workspace_bytes": (_i64, [_i, _i, _i, _i]),
    "seam_resize_bicubic_u8": (_i, [_p, _p, _i, _i, _i, _i, _p, _p]),
    "seam_ce2_fwd_bwd_f32": (_i, [_p, _p, _p, _p, _p, _i64, _p]),
    "seam_pair_logits_bwd_f32": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "seam_nlb_bwd_workspace_floats": (_i64, [_i, _i]),
    "seam_nlb_attnpool_bwd_f32": (_i, [_p, _i64, _i64, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p, _p, _p, C.POINTER(_p), _p, _i, _p]),
    "seam_nlb_block_bwd_f32": (_i, [_p, _i64, _i64, _p, _i, _i, _p, _p, _p, _p, _p, _p, _i64, _i64, _p, C.POINTER(_p), _p, _i, _p]),
    "seam_roi_sample_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _f, _f, _f, _p, _p, _p, _p, _p, _p, _p]),
    "seam_fastrcnn_loss_fwd_bwd_f32": (_i, [_p, _p, _p, _p, _i, _i, _p, _p, _p, _p]),
    "seam_mask_loss_fwd_bwd_f32": (_i, [_p, _p, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p]),
    "seam_rpn_max_gt": (_i, []),
    "seam_rpn_match_workspace_floats": (_i64, [_i, _i, _i]),
    "seam_rpn_match_f32": (_i, [_p, _p, _p, _i, _i, _i, _f, _f, _p, _p, _p, _p]),
    "seam_rpn_sample_workspace_bytes": (_i64, [_i, _i]),
    "seam_rpn_sample_f32": (_i, [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "seam_rpn_gather_patches_f32": (_i, [C.POINTER(_p), C.POINTER(_i), _p, _i, _i, _i, _i, _p, _p]),
    "seam_rpn_loss_fwd_bwd_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p]),
    "seam_roi_align_bwd_workspace_bytes": (_i64, [_i, _i]),
    "seam_roi_align_bwd_f32": (_i, [_p, _p, _p, C.POINTER(_i), _i, _f, _f, _f, _f, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p]),
    "seam_rpn_scatter_patches_f32": (_i, [_p, _p, _i, _i, _i, _i, C.POINTER(_p), C.POINTER(_i), _p]),
    "seam_upsample_add_bwd_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "seam_subsample_add_bwd_f32": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "seam_pack_conv3x3s2_dgrad_f32": (_i, [_p, _p, _p, _i, _i, _p]),
    "seam_conv3x3s2_dgrad_f32": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "seam_relu_mask_add_f32": (_i, [_p, _p, _p, _p, _i64, _i, _p]),
    "seam_maxpool3s2_relu_bwd_f32": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "seam_poly_masks_ws_bytes": (_i64, [_i, _i]),
    "seam_poly_masks_u8": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i, _i, _i, _i, _p]),
    "seam_rle_masks_u8": (_i, [_p, _p, _p, _p, _p, _i, _p]),
    "seam_preprocess_u8_batch_f32": (_i, [_p, _i64, _p, _p, _p, _i, _i, _i, _i, _p]),
    "seam_poly_masks_resized_u8": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _i64, _i, _i, _i, _i, _p]),
    "seam_rle_masks_resized_u8": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i, _p]),
    "seam_rle_encode_ws_bytes": (_i64, [_i, _i]),
    "seam_rle_encode_masks_u8": (_i, [_p, _i64, _p, _p, _p, _p, _p, _i64, _p, _i, _p]),
    "seam_rle_encode_paste_f32": (_i, [_p, _p, _i, _i, _i, _p, _i64, _p, _p]),
    "seam_rle_positions_masks": (_i, [_p, _p, _p, _p, _i64, _p, _p, _i64, _i, _p]),
    "seam_rle_positions_paste": (_i, [_i, _i, _i, _p, _i64, _p, _p, _i64, _p]),
    "seam_rle_bits_from_runs": (_i, [_p, _p, _i, _p, _p, _p, _p, _i64, _i, _p]),
    "seam_rle_bits_combine": (_i, [_p, _p, _i, _p, _p, _p, _i64, _i, _p, _p, _p, _p, _i64, _i, _i, _p]),
    "seam_rle_count_bits": (_i, [_p, _p, _p, _p, _i64, _p, _i, _p]),
    "seam_rle_bits_inter": (_i, [_p, _i, _p, _p, _p, _p, _i64, _i, _p, _p]),
    "seam_rle_bits_area": (_i, [_p, _p, _p, _p, _i64, _i, _p, _p]),
    "seam_sgd_chunk_elems": (_i, []),
    "seam_sgd_step_f32": (_i, [_p, _p, _i, C.POINTER(SgdGroups), _p, _p]),
    "seam_sgd_step_clip_f32": (_i, [_p, _p, _i, C.POINTER(SgdGroups), _p, _p, _i, _p, _p, _p]),
    "seam_grad_norm_workspace_bytes": (_i64, [_i]),
    "seam_grad_norm_f32": (_i, [_p, _p, _i, _i, _i, C.c_float, _i, _p, _i64, _p, _p]),
    "seam_grad_scale_f32": (_i, [_p, _p, _i, _p, _p]),
    "seam_repack_layout": (C.c_longlong, [C.POINTER(RepackJob), _i]),
    "seam_repack_many_f32": (_i, [_p, _i, C.c_longlong, _p]),
}

_lib = None


class SeamNativeError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load (once) and return the bound library; raise loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SeamNativeError(
            f"{LIB_PATH} not found: the HIP extension is required (there is no CPU/PyTorch fallback). "
            "Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
    try:
        handle = C.CDLL(LIB_PATH)
    except OSError as e:   # e.g. libamdhip64 missing
        raise SeamNativeError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise SeamNativeError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _apply_env_options(handle)
    _lib = handle
    return _lib


def _apply_env_options(handle) -> None:
    """The launchers' variant selectors (csrc/seam_opts.h) are plain ints behind ``seam_set_option``: the library itself never
    reads the environment.  For the parity tests and the A/B tools, SEAM_* environment variables of the same names are applied
    here, once, when the library is loaded (``SEAM_CONV_TILE=256x128`` is passed as 256128)."""
    for i in range(handle.seam_option_count()):
        name = handle.seam_option_name(i)
        raw = os.environ.get(name.decode())
        if raw is None or raw == "":
            continue
        if "x" in raw:
            bm, bn = raw.split("x")
            val = int(bm) * 1000 + int(bn)
        else:
            val = int(raw)
        check_rc = handle.seam_set_option(name, val)
        if check_rc != 0:
            raise SeamNativeError(f"seam_set_option({name!r}, {val}) failed: {check_rc}")


def set_option(name: str, value: int) -> None:
    check(lib().seam_set_option(name.encode(), int(value)), f"seam_set_option({name})")


def get_option(name: str) -> int:
    v = C.c_int(0)
    check(lib().seam_get_option(name.encode(), C.byref(v)), f"seam_get_option({name})")
    return v.value


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib().seam_error_string(code)
        raise SeamNativeError(f"{what} failed: hipError {code} ({msg.decode() if msg else '?'})")
