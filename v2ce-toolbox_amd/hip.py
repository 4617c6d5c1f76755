"""ctypes binding of ``csrc/libv2ce_hip.so`` (C ABI: ``include/v2ce_hip.h``).

PyTorch is used only for device memory and streams: every call passes ``tensor.data_ptr()`` and
the current HIP stream handle.  There is NO fallback: if the library is missing or cannot be
loaded, ``lib()`` raises, and so does every op built on it.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
SO_PATH = os.environ.get("V2CE_HIP_LIB", os.path.join(CSRC, "libv2ce_hip.so"))   # override: kernel A/B builds

RNG_REPLAY, RNG_PHILOX = 0, 1
STRATEGY_SLOPE, STRATEGY_NONE, STRATEGY_RANDOM = 0, 1, 2
POOL_NONE, POOL_AVG, POOL_WEIGHTED = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
PRECISION_F32, PRECISION_F16X2 = 0, 1

EXPORTS = [
    "v2ce_version", "v2ce_last_error", "v2ce_ldati_count", "v2ce_ldati_rank_mode", "v2ce_ldati_tile_ws_bytes", "v2ce_ldati_status", "v2ce_ldati_plan_info",
    "v2ce_ldati_selfcheck", "v2ce_ldati_fused_ws_bytes", "v2ce_ldati_count_fused", "v2ce_ldati_emit_fused", "v2ce_ldati_lds_bytes", "v2ce_ldati_workspace_bytes", "v2ce_ldati_emit", "v2ce_events_pack", "v2ce_events_unpack",
    "v2ce_conv3d_fwd",
    "v2ce_conv3d_variant", "v2ce_conv3d_variant_fused", "v2ce_pack_weights_f16x2", "v2ce_pack_weights_f16x2_bytes",
    "v2ce_pack_weights", "v2ce_sn_workspace_bytes", "v2ce_sn_power_iter", "v2ce_sn_batch_workspace_bytes", "v2ce_sn_update_batch",
    "v2ce_preprocess_pairs", "v2ce_preprocess_pairs_resize",
    "v2ce_voxelize_events", "v2ce_conv3d_fwd_pred", "v2ce_conv3d_fwd_sc", "v2ce_conv3d_fwd_tail", "v2ce_pack_pred_weights_f16x2", "v2ce_pack_pred_weights_f16x2_bytes",
    "v2ce_sampler_count", "v2ce_sampler_workspace_bytes", "v2ce_sampler_emit", "v2ce_sampler_pool",
    "v2ce_conv3d_fwd_up2", "v2ce_pack_weights_f16x2_up", "v2ce_pack_weights_f16x2_up_bytes", "v2ce_conv3d_up2_variant",
    "v2ce_conv3d_fwd_wt", "v2ce_conv3d_fwd_wt_tail", "v2ce_pack_weights_f16x2_wt", "v2ce_pack_weights_f16x2_wt_slice", "v2ce_conv3d_fwd_up2_part", "v2ce_pack_weights_f16x2_wt_bytes", "v2ce_conv3d_wt_variant",
    "v2ce_conv3d_head_f16x2", "v2ce_pack_head_weights_f16x2", "v2ce_pack_head_weights_f16x2_bytes", "v2ce_absmax_batch",
    "v2ce_pack_head_weights_f16x2_c3", "v2ce_pack_head_weights_f16x2_c3_bytes",
    "v2ce_tsdiff_workspace_bytes", "v2ce_tsdiff",
    "v2ce_voxlosses_workspace_bytes", "v2ce_voxlosses", "v2ce_volume_losses_workspace_bytes", "v2ce_volume_losses",
    "v2ce_voxmetrics_workspace_bytes", "v2ce_voxmetrics", "v2ce_voxelize_batch_workspace_bytes", "v2ce_voxelize_batch",
    "v2ce_event_frames_hist_bytes", "v2ce_event_frames_sums", "v2ce_event_frames_refine", "v2ce_event_frames_render",
    "v2ce_event_grids_workspace_bytes", "v2ce_event_grids_batch",
    "v2ce_physatt_workspace_bytes", "v2ce_physatt_batch", "v2ce_log_residual_batch",
    "v2ce_image_grad_workspace_bytes", "v2ce_image_grad_batch", "v2ce_image_units_grad",
]

# the training-side entries (include/v2ce_hip_grad.h), bound next to the others
GRAD_EXPORTS = ("v2ce_voxloss_grads_workspace_bytes", "v2ce_voxloss_grads", "v2ce_volume_loss_grads_workspace_bytes",
                "v2ce_volume_loss_grads")

# the trainable layers (include/v2ce_hip_train.h): forward and backward of the prediction head
TRAIN_EXPORTS = ("v2ce_pred_head_fwd_workspace_bytes", "v2ce_pred_head_fwd", "v2ce_pred_head_grads_workspace_bytes",
                 "v2ce_pred_head_grads")

# the weight gradients of the trunk's convolutions (include/v2ce_hip_convgrad.h)
CONVGRAD_EXPORTS = ("v2ce_conv32_wgrad_workspace_bytes", "v2ce_conv32_wgrad")
WGRAD_CHAIN = 4096                       # V2CE_WGRAD_CHAIN: positions one f32 accumulator sums before it meets the f64 sum

# the input gradients of the trunk's convolutions (include/v2ce_hip_convdgrad.h)
CONVDGRAD_EXPORTS = ("v2ce_conv32_dgrad_workspace_bytes", "v2ce_conv32_dgrad")
DGRAD_TERMS = 864                        # V2CE_DGRAD_TERMS: f32 terms of one d_x element (32 output channels x 27 taps)

# the weight gradients of the last decoder block's conv1 and shortcut on the upsample + concat input
# (include/v2ce_hip_convupgrad.h)
CONVUPGRAD_EXPORTS = ("v2ce_convup_wgrad_workspace_bytes", "v2ce_convup_wgrad")
UPWGRAD_CHAIN = 4096                     # V2CE_UPWGRAD_CHAIN: positions one f32 accumulator sums before it meets the f64 sum

# the input gradients of the same two layers, back through the concat and the upsample (include/v2ce_hip_convupdgrad.h)
CONVUPDGRAD_EXPORTS = ("v2ce_convup_dgrad_workspace_bytes", "v2ce_convup_dgrad")
UPDGRAD_TERMS = 896                      # V2CE_UPDGRAD_TERMS: f32 terms of one d_X element (32 output channels x 28 units)

# the weight and input gradients of a 3x3x3 convolution with 32 or 64 channels on either side: UNet.decoders[2].conv2
# (include/v2ce_hip_convngrad.h)
CONVNGRAD_EXPORTS = ("v2ce_convn_wgrad_workspace_bytes", "v2ce_convn_wgrad", "v2ce_convn_dgrad_workspace_bytes",
                     "v2ce_convn_dgrad")
CONVN_CHANNELS = (32, 64)                # what cin and cout may be

# the same two gradients with any width of the UNet on either side: UNet.decoders[1].conv2 and every 3x3x3 convolution in
# front of it (include/v2ce_hip_convcgrad.h)
CONVCGRAD_EXPORTS = ("v2ce_convc_wgrad_workspace_bytes", "v2ce_convc_wgrad", "v2ce_convc_dgrad_workspace_bytes",
                     "v2ce_convc_dgrad")
CONVC_CHANNELS = (32, 64, 128, 256, 512)  # what cin and cout may be

# the weight gradients of a decoder block's conv1 and shortcut on the upsample + concat input with the channel counts as
# arguments: UNet.decoders[2].conv1 and .downsample[0] (include/v2ce_hip_convupngrad.h)
CONVUPNGRAD_EXPORTS = ("v2ce_convupn_wgrad_workspace_bytes", "v2ce_convupn_wgrad")
CONVUPN_C0, CONVUPN_C1, CONVUPN_COUT = (64, 128), (32, 64), (32, 64)     # what c0, c1 and cout may be

# the input gradients of the same two layers with the channel counts as arguments, back through the concat and the upsample
# (include/v2ce_hip_convupndgrad.h); c0, c1 and cout are those of CONVUPN_C0, CONVUPN_C1 and CONVUPN_COUT
CONVUPNDGRAD_EXPORTS = ("v2ce_convupn_dgrad_workspace_bytes", "v2ce_convupn_dgrad")
UPNDGRAD_TERMS = lambda cout: 28 * cout  # V2CE_UPNDGRAD_TERMS(cout): f32 terms of one d_X element (cout output channels x 28 units)


LAYOUT_PLANAR, LAYOUT_C16 = 0, 1


class ConvDesc(ctypes.Structure):
    """``v2ce_conv3d_desc`` (include/v2ce_hip.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "B", "T", "C0", "H0", "W0", "C1", "Hin", "Win", "Cout", "Hout", "Wout", "ksize",
        "stride_hw", "act", "tile_t", "tile_h", "tile_w", "precision", "W0_pitch", "Win_pitch", "Wout_pitch", "layout",
        "absmax_batch_stride")]


class SnLayer(ctypes.Structure):
    """``v2ce_sn_layer`` (include/v2ce_hip.h): one spectral-norm layer of v2ce_sn_update_batch."""
    _fields_ = [("w_bar", ctypes.c_void_p), ("u", ctypes.c_void_p), ("v", ctypes.c_void_p), ("packed", ctypes.c_void_p),
                ("rows", ctypes.c_int32), ("cols", ctypes.c_int32), ("k3", ctypes.c_int32), ("up_c0", ctypes.c_int32),
                ("wt", ctypes.c_int32), ("flags", ctypes.c_int32), ("packed_skip", ctypes.c_void_p),
                ("bn_scale", ctypes.c_void_p), ("scale_out", ctypes.c_void_p), ("inv_sigma_out", ctypes.c_void_p),
                ("sigma_src", ctypes.c_void_p), ("wmax", ctypes.c_float), ("reserved", ctypes.c_int32)]


SN_NO_PACK, SN_NO_ITERATE = 1, 2


class LdatiOptions(ctypes.Structure):
    """``v2ce_ldati_options`` (include/v2ce_hip.h): the keyword options of sample_voxel_statistical."""
    _fields_ = [(n, ctypes.c_int32) for n in ("strategy", "bidirectional", "pooling_type", "pooling_kernel_size")]


class SamplerOptions(ctypes.Structure):
    """``v2ce_sampler_options`` (include/v2ce_hip.h): the ablation samplers of SURVEY 8f4."""
    _fields_ = [("mode", ctypes.c_int32), ("rng_mode", ctypes.c_int32), ("fps", ctypes.c_double), ("t0", ctypes.c_double),
                ("seed", ctypes.c_uint64), ("frame_base", ctypes.c_int32), ("replay_M", ctypes.c_int32),
                ("u_int", ctypes.c_void_p), ("u_dec", ctypes.c_void_p), ("u_bern", ctypes.c_void_p), ("pooled", ctypes.c_void_p)]


SAMPLER_RANDOM, SAMPLER_EVEN, SAMPLER_PURE_SLOPE = 0, 1, 2

VOXMETRICS_MAX_POOLS = 8


class VoxMetricsStats(ctypes.Structure):
    """``v2ce_voxmetrics_stats`` (include/v2ce_hip.h): the stage-1 sufficient statistics of one sequence."""
    _fields_ = [("struct_size", ctypes.c_int64), ("n", ctypes.c_int64 * 3), ("tp", ctypes.c_int64 * 3),
                ("fp", ctypes.c_int64 * 3), ("fn", ctypes.c_int64 * 3), ("abs_diff_sum", ctypes.c_double),
                ("ratio_sum", ctypes.c_double), ("n_pools", ctypes.c_int64),
                ("pool_size", ctypes.c_int64 * VOXMETRICS_MAX_POOLS), ("pool_n", ctypes.c_int64 * VOXMETRICS_MAX_POOLS),
                ("pool_sq_sum", ctypes.c_double * VOXMETRICS_MAX_POOLS)]


VOXLOSSES_PYRAMID, VOXLOSSES_TEMPORAL, VOXLOSSES_EF, VOXLOSSES_COMPENSATION, VOXLOSSES_MATCH = 1, 2, 4, 8, 16


class VoxLossesStats(ctypes.Structure):
    """``v2ce_voxlosses_stats`` (include/v2ce_hip.h): the stage-1 loss statistics of one sequence or volume."""
    _fields_ = [("struct_size", ctypes.c_int64), ("term_mask", ctypes.c_int64), ("n", ctypes.c_int64),
                ("sq_sum", ctypes.c_double), ("abs_diff_sum", ctypes.c_double), ("pred_abs_sum", ctypes.c_double),
                ("pred_sq_sum", ctypes.c_double), ("pyr_n", ctypes.c_int64 * 3), ("pyr_sq_sum", ctypes.c_double * 3),
                ("temporal_n", ctypes.c_int64 * 2), ("temporal_sq_sum", ctypes.c_double * 2),
                ("ef_n", ctypes.c_int64 * 4), ("ef_sq_sum", ctypes.c_double * 4), ("comp_n", ctypes.c_int64),
                ("comp_sq_sum", ctypes.c_double), ("match_n", ctypes.c_int64), ("match_sum", ctypes.c_double),
                ("match_low", ctypes.c_int64)]


class VoxLossGradCoeffs(ctypes.Structure):
    """``v2ce_voxloss_grad_coeffs`` (include/v2ce_hip_grad.h): one f64 factor per linear piece of the loss gradient."""
    _fields_ = [("struct_size", ctypes.c_int64), ("a_sq", ctypes.c_double), ("a_pyr", ctypes.c_double * 3),
                ("a_t3", ctypes.c_double), ("a_t5", ctypes.c_double), ("a_ef", ctypes.c_double * 4),
                ("a_comp", ctypes.c_double), ("a_match", ctypes.c_double), ("a_l1", ctypes.c_double),
                ("a_l2", ctypes.c_double)]


VOXELIZE_EMPTY, VOXELIZE_SINGLE_TIMESTAMP, VOXELIZE_BAD_XY, VOXELIZE_BAD_RANGE = 1, 2, 4, 8

EVENT_GRIDS_SIGNED, EVENT_GRIDS_SPLIT, EVENT_GRIDS_STAT = 1, 2, 4
(EVENT_GRIDS_EMPTY, EVENT_GRIDS_BAD_XY, EVENT_GRIDS_BAD_TIME, EVENT_GRIDS_STAT_TOP_EDGE,
 EVENT_GRIDS_STAT_OVERFLOW) = 1, 2, 4, 8, 16

PHYSATT_PLAIN, PHYSATT_ADVANCED, PHYSATT_RATIO = 0, 1, 2
PHYSATT_BAD_XY, PHYSATT_BAD_OFFSETS, PHYSATT_COUNT_OVERFLOW = 1, 2, 4

EVENT_FRAMES_POLARITY, EVENT_FRAMES_GREY = 0, 1
EVENT_FRAMES_LEVEL0_BINS, EVENT_FRAMES_REFINE_BINS = 2048, 1024


class V2ceHipError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile the HIP library in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j4", "libv2ce_hip.so"])
    return SO_PATH


_LIB = None


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(SO_PATH):
        raise V2ceHipError(
            f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (make -C {CSRC}).  There is no CPU fallback.")
    L = ctypes.CDLL(SO_PATH)
    vp, i32, i64, f64, u64, sz = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double,
                                  ctypes.c_uint64, ctypes.c_size_t)
    L.v2ce_version.restype = ctypes.c_char_p
    L.v2ce_last_error.restype = ctypes.c_char_p
    op = ctypes.POINTER(LdatiOptions)
    L.v2ce_ldati_count.argtypes = [vp, i32, i32, i32, op, vp, sz, vp, vp, vp]
    L.v2ce_ldati_tile_ws_bytes.argtypes = [i32, i32, i32]
    L.v2ce_ldati_tile_ws_bytes.restype = sz
    L.v2ce_ldati_lds_bytes.argtypes = [f64, f64]
    L.v2ce_ldati_lds_bytes.restype = sz
    L.v2ce_ldati_emit.argtypes = [vp, i32, i32, i32, f64, f64, op, i32, vp, i32, u64, i64, vp, vp,
                                  vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, sz, vp]
    L.v2ce_ldati_fused_ws_bytes.argtypes = [i32, i32, i32, f64, f64, op, i64, i64]
    L.v2ce_ldati_fused_ws_bytes.restype = sz
    L.v2ce_ldati_count_fused.argtypes = [vp, i32, i32, i32, f64, f64, op, i32, vp, i32, u64, i64, i64, i64, vp, sz, vp, sz, vp, vp, vp]
    L.v2ce_ldati_count_fused.restype = ctypes.c_int
    L.v2ce_ldati_emit_fused.argtypes = [vp, i32, i32, i32, f64, f64, op, i32, vp, i32, u64, i64, vp, vp,
                                        vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, sz, vp, sz, i64, i64, i64, vp]
    L.v2ce_ldati_emit_fused.restype = ctypes.c_int
    L.v2ce_ldati_workspace_bytes.argtypes = [i32, i32, i32, f64, f64, op, i64, i64, i64, i32]
    L.v2ce_ldati_workspace_bytes.restype = sz
    L.v2ce_ldati_status.argtypes = [vp, i32, i32, i32, f64, f64, op, i64, i64, i64, ctypes.POINTER(vp)]
    L.v2ce_ldati_status.restype = ctypes.c_int
    L.v2ce_ldati_plan_info.argtypes = [i32, i32, i32, f64, f64, op, i64, i64, i64, vp]
    L.v2ce_ldati_plan_info.restype = ctypes.c_int
    L.v2ce_ldati_selfcheck.argtypes = [f64, ctypes.POINTER(ctypes.c_int64)]
    L.v2ce_ldati_selfcheck.restype = ctypes.c_int
    L.v2ce_ldati_rank_mode.argtypes = [ctypes.POINTER(ctypes.c_int32)]
    L.v2ce_ldati_rank_mode.restype = ctypes.c_int
    L.v2ce_events_pack.argtypes = [vp, vp, vp, vp, i64, vp, vp]
    L.v2ce_events_unpack.argtypes = [vp, i64, vp, vp, vp, vp, vp]
    L.v2ce_events_unpack.restype = ctypes.c_int
    L.v2ce_conv3d_fwd.argtypes = [ctypes.POINTER(ConvDesc)] + [vp] * 13
    L.v2ce_pack_weights.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    L.v2ce_pack_weights_f16x2.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    L.v2ce_pack_weights_f16x2.restype = ctypes.c_int
    L.v2ce_pack_weights_f16x2_bytes.argtypes = [i32, i32, i32]
    L.v2ce_pack_weights_f16x2_bytes.restype = sz
    L.v2ce_conv3d_variant.argtypes = [ctypes.POINTER(ConvDesc), i32, ctypes.c_char_p, sz]
    L.v2ce_conv3d_variant_fused.argtypes = [ctypes.POINTER(ConvDesc), i32, i32, ctypes.c_char_p, sz]
    L.v2ce_conv3d_variant_fused.restype = ctypes.c_int
    L.v2ce_preprocess_pairs.argtypes = [vp, i32, i32, i32, ctypes.c_float, ctypes.c_float, vp, vp]
    L.v2ce_preprocess_pairs.restype = ctypes.c_int
    L.v2ce_preprocess_pairs_resize.argtypes = [vp, i32, i32, i32, i32, i32, ctypes.c_float, ctypes.c_float, vp, vp]
    L.v2ce_preprocess_pairs_resize.restype = ctypes.c_int
    L.v2ce_voxelize_events.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, vp]
    L.v2ce_voxelize_events.restype = ctypes.c_int
    L.v2ce_conv3d_fwd_pred.argtypes = [ctypes.POINTER(ConvDesc)] + [vp] * 14 + [i32, vp, vp]
    L.v2ce_conv3d_fwd_pred.restype = ctypes.c_int
    L.v2ce_conv3d_fwd_sc.argtypes = [ctypes.POINTER(ConvDesc)] + [vp] * 16
    L.v2ce_conv3d_fwd_sc.restype = ctypes.c_int
    L.v2ce_conv3d_fwd_tail.argtypes = [ctypes.POINTER(ConvDesc)] + [vp] * 11 + [ctypes.POINTER(ConvDesc)] + [vp] * 8
    L.v2ce_conv3d_fwd_tail.restype = ctypes.c_int
    L.v2ce_conv3d_fwd_up2.argtypes = [ctypes.POINTER(ConvDesc)] + [vp] * 14
    L.v2ce_conv3d_fwd_up2.restype = ctypes.c_int
    L.v2ce_pack_weights_f16x2_up.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    L.v2ce_pack_weights_f16x2_up.restype = ctypes.c_int
    L.v2ce_pack_weights_f16x2_up_bytes.argtypes = [i32, i32, i32]
    L.v2ce_pack_weights_f16x2_up_bytes.restype = sz
    L.v2ce_conv3d_up2_variant.argtypes = [ctypes.POINTER(ConvDesc), i32, ctypes.c_char_p, sz]
    L.v2ce_conv3d_up2_variant.restype = ctypes.c_int
    L.v2ce_conv3d_fwd_wt.argtypes = [ctypes.POINTER(ConvDesc)] + [vp] * 9
    L.v2ce_conv3d_fwd_wt.restype = ctypes.c_int
    L.v2ce_conv3d_fwd_wt_tail.argtypes = [ctypes.POINTER(ConvDesc)] + [vp] * 7 + [ctypes.POINTER(ConvDesc)] + [vp] * 8 + [i32, i32, vp]
    L.v2ce_conv3d_fwd_wt_tail.restype = ctypes.c_int
    L.v2ce_pack_weights_f16x2_wt_slice.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
    L.v2ce_pack_weights_f16x2_wt_slice.restype = ctypes.c_int
    L.v2ce_conv3d_fwd_up2_part.argtypes = [ctypes.POINTER(ConvDesc)] + [vp] * 9
    L.v2ce_conv3d_fwd_up2_part.restype = ctypes.c_int
    L.v2ce_pack_weights_f16x2_wt.argtypes = [vp, i32, i32, vp, vp, vp]
    L.v2ce_pack_weights_f16x2_wt.restype = ctypes.c_int
    L.v2ce_pack_weights_f16x2_wt_bytes.argtypes = [i32, i32]
    L.v2ce_pack_weights_f16x2_wt_bytes.restype = sz
    L.v2ce_conv3d_wt_variant.argtypes = [ctypes.POINTER(ConvDesc), i32, ctypes.c_char_p, sz]
    L.v2ce_conv3d_wt_variant.restype = ctypes.c_int
    L.v2ce_conv3d_head_f16x2.argtypes = [ctypes.POINTER(ConvDesc)] + [vp] * 7
    L.v2ce_conv3d_head_f16x2.restype = ctypes.c_int
    L.v2ce_pack_head_weights_f16x2.argtypes = [vp, vp, vp]
    L.v2ce_pack_head_weights_f16x2.restype = ctypes.c_int
    L.v2ce_pack_head_weights_f16x2_bytes.argtypes = []
    L.v2ce_pack_head_weights_f16x2_bytes.restype = sz
    L.v2ce_pack_head_weights_f16x2_c3.argtypes = [vp, vp, vp]
    L.v2ce_pack_head_weights_f16x2_c3.restype = ctypes.c_int
    L.v2ce_pack_head_weights_f16x2_c3_bytes.argtypes = []
    L.v2ce_pack_head_weights_f16x2_c3_bytes.restype = sz
    L.v2ce_absmax_batch.argtypes = [vp, i32, ctypes.c_longlong, vp, i32, vp]
    L.v2ce_absmax_batch.restype = ctypes.c_int
    L.v2ce_pack_pred_weights_f16x2.argtypes = [vp, i32, i32, vp, vp]
    L.v2ce_pack_pred_weights_f16x2.restype = ctypes.c_int
    L.v2ce_pack_pred_weights_f16x2_bytes.argtypes = []
    L.v2ce_pack_pred_weights_f16x2_bytes.restype = sz
    L.v2ce_sn_workspace_bytes.argtypes = [i32, i32]
    L.v2ce_sn_workspace_bytes.restype = sz
    L.v2ce_sn_power_iter.argtypes = [vp, vp, vp, i32, i32, vp, vp, sz, vp]
    L.v2ce_sn_batch_workspace_bytes.argtypes = [ctypes.POINTER(SnLayer), i32]
    L.v2ce_sn_batch_workspace_bytes.restype = sz
    L.v2ce_sn_update_batch.argtypes = [ctypes.POINTER(SnLayer), i32, vp, sz, vp]
    L.v2ce_sn_update_batch.restype = ctypes.c_int
    so = ctypes.POINTER(SamplerOptions)
    L.v2ce_sampler_count.argtypes = [vp, i32, i32, i32, so, vp, vp, vp]
    L.v2ce_sampler_count.restype = ctypes.c_int
    L.v2ce_sampler_pool.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp]
    L.v2ce_sampler_pool.restype = ctypes.c_int
    L.v2ce_sampler_workspace_bytes.argtypes = [i64]
    L.v2ce_sampler_workspace_bytes.restype = sz
    L.v2ce_sampler_emit.argtypes = [vp, i32, i32, i32, so, i64, vp, vp, vp, vp, vp, sz, vp, vp]
    L.v2ce_sampler_emit.restype = ctypes.c_int
    L.v2ce_tsdiff_workspace_bytes.argtypes = [i32, i32, i32, i64]
    L.v2ce_tsdiff_workspace_bytes.restype = sz
    L.v2ce_tsdiff.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]
    L.v2ce_tsdiff.restype = ctypes.c_int
    L.v2ce_voxmetrics_workspace_bytes.argtypes = [i32, i32, i32, i32, i32, vp, i32]
    L.v2ce_voxmetrics_workspace_bytes.restype = sz
    L.v2ce_voxmetrics.argtypes = [vp, vp, i32, i32, i32, i32, i32, ctypes.c_float, vp, i32, vp, sz, vp, sz, vp]
    L.v2ce_voxmetrics.restype = ctypes.c_int
    L.v2ce_voxlosses_workspace_bytes.argtypes = [i32, i32, i32, i32, i32, i32]
    L.v2ce_voxlosses_workspace_bytes.restype = sz
    L.v2ce_voxlosses.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, vp, sz, vp]
    L.v2ce_voxlosses.restype = ctypes.c_int
    L.v2ce_volume_losses_workspace_bytes.argtypes = [i32, i32, i32, i32, i32]
    L.v2ce_volume_losses_workspace_bytes.restype = sz
    L.v2ce_volume_losses.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, sz, vp, sz, vp]
    L.v2ce_volume_losses.restype = ctypes.c_int
    cp = ctypes.POINTER(VoxLossGradCoeffs)
    L.v2ce_voxloss_grads_workspace_bytes.argtypes = [i32, i32, i32, i32, i32, cp, sz]
    L.v2ce_voxloss_grads_workspace_bytes.restype = sz
    L.v2ce_voxloss_grads.argtypes = [vp, vp, i32, i32, i32, i32, i32, cp, sz, vp, vp, vp, sz, vp]
    L.v2ce_voxloss_grads.restype = ctypes.c_int
    L.v2ce_volume_loss_grads_workspace_bytes.argtypes = [i32, i32, i32, i32, cp, sz]
    L.v2ce_volume_loss_grads_workspace_bytes.restype = sz
    L.v2ce_volume_loss_grads.argtypes = [vp, vp, i32, i32, i32, i32, cp, sz, vp, vp, vp, sz, vp]
    L.v2ce_volume_loss_grads.restype = ctypes.c_int
    L.v2ce_pred_head_fwd_workspace_bytes.argtypes = [i32] * 6
    L.v2ce_pred_head_fwd_workspace_bytes.restype = sz
    L.v2ce_pred_head_fwd.argtypes = [vp, vp, vp] + [i32] * 6 + [vp, vp, sz, vp]
    L.v2ce_pred_head_fwd.restype = ctypes.c_int
    L.v2ce_pred_head_grads_workspace_bytes.argtypes = [i32] * 6
    L.v2ce_pred_head_grads_workspace_bytes.restype = sz
    L.v2ce_pred_head_grads.argtypes = [vp, vp, vp, vp] + [i32] * 6 + [vp, vp, vp, vp, sz, vp]
    L.v2ce_pred_head_grads.restype = ctypes.c_int
    L.v2ce_conv32_wgrad_workspace_bytes.argtypes = [i32] * 6
    L.v2ce_conv32_wgrad_workspace_bytes.restype = sz
    L.v2ce_conv32_wgrad.argtypes = [vp, vp, vp] + [i32] * 5 + [vp, vp, vp, sz, i32, vp]
    L.v2ce_conv32_wgrad.restype = ctypes.c_int
    L.v2ce_conv32_dgrad_workspace_bytes.argtypes = [i32] * 6
    L.v2ce_conv32_dgrad_workspace_bytes.restype = sz
    L.v2ce_conv32_dgrad.argtypes = [vp, vp, vp] + [i32] * 5 + [vp, vp, vp, sz, i32, vp]
    L.v2ce_conv32_dgrad.restype = ctypes.c_int
    L.v2ce_convup_wgrad_workspace_bytes.argtypes = [i32] * 7
    L.v2ce_convup_wgrad_workspace_bytes.restype = sz
    L.v2ce_convup_wgrad.argtypes = [vp, vp, vp, vp] + [i32] * 6 + [vp, vp, vp, vp, sz, i32, vp]
    L.v2ce_convup_wgrad.restype = ctypes.c_int
    L.v2ce_convup_dgrad_workspace_bytes.argtypes = [i32] * 7
    L.v2ce_convup_dgrad_workspace_bytes.restype = sz
    L.v2ce_convup_dgrad.argtypes = [vp, vp, vp, vp] + [i32] * 6 + [vp, vp, vp, sz, i32, vp]
    L.v2ce_convup_dgrad.restype = ctypes.c_int
    L.v2ce_convn_wgrad_workspace_bytes.argtypes = [i32] * 8
    L.v2ce_convn_wgrad_workspace_bytes.restype = sz
    L.v2ce_convn_wgrad.argtypes = [vp, vp, vp] + [i32] * 7 + [vp, vp, vp, sz, i32, vp]
    L.v2ce_convn_wgrad.restype = ctypes.c_int
    L.v2ce_convn_dgrad_workspace_bytes.argtypes = [i32] * 8
    L.v2ce_convn_dgrad_workspace_bytes.restype = sz
    L.v2ce_convn_dgrad.argtypes = [vp, vp, vp] + [i32] * 7 + [vp, vp, vp, sz, i32, vp]
    L.v2ce_convn_dgrad.restype = ctypes.c_int
    L.v2ce_convc_wgrad_workspace_bytes.argtypes = [i32] * 8
    L.v2ce_convc_wgrad_workspace_bytes.restype = sz
    L.v2ce_convc_wgrad.argtypes = [vp, vp, vp] + [i32] * 7 + [vp, vp, vp, sz, i32, vp]
    L.v2ce_convc_wgrad.restype = ctypes.c_int
    L.v2ce_convc_dgrad_workspace_bytes.argtypes = [i32] * 8
    L.v2ce_convc_dgrad_workspace_bytes.restype = sz
    L.v2ce_convc_dgrad.argtypes = [vp, vp, vp] + [i32] * 7 + [vp, vp, vp, sz, i32, vp]
    L.v2ce_convc_dgrad.restype = ctypes.c_int
    L.v2ce_convupn_wgrad_workspace_bytes.argtypes = [i32] * 10
    L.v2ce_convupn_wgrad_workspace_bytes.restype = sz
    L.v2ce_convupn_wgrad.argtypes = [vp, vp, vp, vp] + [i32] * 9 + [vp, vp, vp, vp, sz, i32, vp]
    L.v2ce_convupn_wgrad.restype = ctypes.c_int
    L.v2ce_convupn_dgrad_workspace_bytes.argtypes = [i32] * 10
    L.v2ce_convupn_dgrad_workspace_bytes.restype = sz
    L.v2ce_convupn_dgrad.argtypes = [vp, vp, vp, vp] + [i32] * 9 + [vp, vp, vp, sz, i32, vp]
    L.v2ce_convupn_dgrad.restype = ctypes.c_int
    L.v2ce_voxelize_batch_workspace_bytes.argtypes = [i32, i32, i32, i32, i64]
    L.v2ce_voxelize_batch_workspace_bytes.restype = sz
    L.v2ce_voxelize_batch.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, vp, vp, sz, vp]
    L.v2ce_voxelize_batch.restype = ctypes.c_int
    L.v2ce_event_grids_workspace_bytes.argtypes = [i32, i32, i32, i32, i64, i32]
    L.v2ce_event_grids_workspace_bytes.restype = sz
    L.v2ce_event_grids_batch.argtypes = [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.v2ce_event_grids_batch.restype = ctypes.c_int
    L.v2ce_physatt_workspace_bytes.argtypes = [i32, i32, i32, i32, i64]
    L.v2ce_physatt_workspace_bytes.restype = sz
    L.v2ce_physatt_batch.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, i64, i32, i32, ctypes.c_float, ctypes.c_float, i32,
                                     vp, ctypes.POINTER(ctypes.c_double), vp, vp, vp, vp, sz, vp]
    L.v2ce_physatt_batch.restype = ctypes.c_int
    L.v2ce_log_residual_batch.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    L.v2ce_log_residual_batch.restype = ctypes.c_int
    fp = ctypes.POINTER(ctypes.c_float)
    L.v2ce_image_grad_workspace_bytes.argtypes = [i32, i32, i32, i32]
    L.v2ce_image_grad_workspace_bytes.restype = sz
    L.v2ce_image_grad_batch.argtypes = [vp, i32, i32, i32, i32, fp, i32, vp, vp, vp]
    L.v2ce_image_grad_batch.restype = ctypes.c_int
    L.v2ce_image_units_grad.argtypes = [vp, i32, i32, i32, i32, fp, i32, ctypes.c_float, ctypes.c_float, vp, vp, vp, sz, vp]
    L.v2ce_image_units_grad.restype = ctypes.c_int
    L.v2ce_event_frames_hist_bytes.argtypes = [i32]
    L.v2ce_event_frames_hist_bytes.restype = sz
    L.v2ce_event_frames_sums.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
    L.v2ce_event_frames_sums.restype = ctypes.c_int
    L.v2ce_event_frames_refine.argtypes = [vp, i32, i32, i32, i32, i32, ctypes.c_uint32, ctypes.c_uint32, vp, vp]
    L.v2ce_event_frames_refine.restype = ctypes.c_int
    L.v2ce_event_frames_render.argtypes = [vp, i32, i32, i32, i32, f64, i64, i64, vp, vp]
    L.v2ce_event_frames_render.restype = ctypes.c_int
    for name in ("v2ce_ldati_count", "v2ce_ldati_emit", "v2ce_events_pack",
                 "v2ce_conv3d_fwd", "v2ce_conv3d_variant", "v2ce_pack_weights", "v2ce_sn_power_iter"):
        getattr(L, name).restype = ctypes.c_int
    _LIB = L
    return L


def source_hash() -> str:
    """16 hex digits over the kernel sources and the C ABI header of THIS tree (csrc/*.hip, csrc/*.h, include/*.h): the
    provenance stamp of the counter summaries under profiles/ -- bench.py drops a counter-derived field whose summary was
    collected from other sources (the GPU box has no .git to ask for a commit hash)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) +
                   glob.glob(os.path.join(os.path.dirname(_HERE), "include", "*.h")))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def provenance() -> dict:
    """What a profile summary records about the build it measured."""
    return {"lib_version": lib().v2ce_version().decode(), "source_hash": source_hash()}


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().v2ce_last_error().decode()
        raise V2ceHipError(f"{what} failed with code {rc}: {msg}")


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def require_device_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise V2ceHipError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if t.dtype != torch.float32:
        raise V2ceHipError(f"{name} must be float32 (got {t.dtype})")
    return t.contiguous()


def conv_wt_variant(desc: ConvDesc, with_residual) -> str:
    """with_residual: False / True, or 2 for the folded-tail form."""
    buf = ctypes.create_string_buffer(96)
    check(lib().v2ce_conv3d_wt_variant(ctypes.byref(desc), int(with_residual), buf, 96), "v2ce_conv3d_wt_variant")
    return buf.value.decode()


def conv_up2_variant(desc: ConvDesc, with_shortcut: bool) -> str:
    buf = ctypes.create_string_buffer(96)
    check(lib().v2ce_conv3d_up2_variant(ctypes.byref(desc), int(with_shortcut), buf, 96), "v2ce_conv3d_up2_variant")
    return buf.value.decode()


def conv_variant(desc: ConvDesc, mapped: bool, fuse: int = 0) -> str:
    buf = ctypes.create_string_buffer(96)
    check(lib().v2ce_conv3d_variant_fused(ctypes.byref(desc), int(mapped), int(fuse), buf, 96), "v2ce_conv3d_variant")
    return buf.value.decode()
