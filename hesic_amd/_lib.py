"""ctypes binding of ``libhesic_hip.so`` / ``libhesic_hip_f16.so`` (C ABI: ``include/hesic_hip.h``).

The libraries are built in-tree by ``__graft_entry__.build()`` / ``make -C hesic_amd/csrc`` from the same sources: one per
16-bit storage / matrix-core operand format (bfloat16: training + inference; IEEE float16: inference).  ``use_h16()`` selects
which one ``call()`` goes to; fp32 tensors are served by either.
There is NO fallback: if the shared object is missing or a kernel call fails, the caller gets
an exception -- the product path never routes through the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhesic_hip.so")
LIB_PATH_F16 = os.path.join(_HERE, "libhesic_hip_f16.so")
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")

F32, H16 = 0, 1
ABI_VERSION = 3      # include/hesic_hip.h HESIC_ABI_VERSION
BF16 = H16       # historical name: the library's 16-bit format (hesic_h16_format())
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
EB_PARAM_STRIDE = 64

_i32, _i64, _f32, _vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class ConvDesc(C.Structure):
    _fields_ = [(n, _i32) for n in (
        "B", "H", "W", "Cin", "Ho", "Wo", "Cout", "KH", "KW", "stride", "pad", "transposed", "dtype", "act",
        "in_abs", "x_pix_stride", "x_c_off", "y_pix_stride", "y_c_off", "tap_mask_lo")]


class SConvDesc(C.Structure):
    _fields_ = [(n, _i32) for n in ("B", "H", "W", "Cin", "Ho", "Wo", "Cout", "KH", "KW", "stride", "pad",
                                    "transposed", "x_dtype", "y_dtype", "act")] + \
               [("_pad", _i32)] + \
               [(n, _i64) for n in ("xs_b", "xs_c", "xs_y", "xs_x", "ys_b", "ys_c", "ys_y", "ys_x")]


class WarpDesc(C.Structure):
    _fields_ = [(n, _i32) for n in ("B", "C", "H", "W", "Ho", "Wo", "align_corners", "src_dtype", "dst_dtype", "m_is_dst_to_src")] + \
               [(n, _i64) for n in ("ss_b", "ss_c", "ss_y", "ss_x", "ds_b", "ds_c", "ds_y", "ds_x")]


ADAM_MAX_TENSORS = 24


class AdamChunk(C.Structure):
    _fields_ = [("p", _vp * ADAM_MAX_TENSORS), ("g", _vp * ADAM_MAX_TENSORS), ("m", _vp * ADAM_MAX_TENSORS),
                ("v", _vp * ADAM_MAX_TENSORS), ("step", _vp * ADAM_MAX_TENSORS), ("numel", _i64 * ADAM_MAX_TENSORS),
                ("block0", _i32 * (ADAM_MAX_TENSORS + 1)), ("n", _i32), ("lr", _f32), ("beta1", _f32), ("beta2", _f32), ("eps", _f32)]


EB_MAX_TENSORS = 16


class EbLayout(C.Structure):
    _fields_ = [("ptr", _vp * EB_MAX_TENSORS), ("width", _i32 * EB_MAX_TENSORS), ("stride", _i32 * EB_MAX_TENSORS),
                ("first", _i32 * EB_MAX_TENSORS), ("col", _i32 * EB_MAX_TENSORS), ("n", _i32), ("lik_bound", _f32)]


class GmmDesc(C.Structure):
    _fields_ = [(n, _i32) for n in ("B", "HW", "M", "K", "dtype", "use_means_in_quant", "sm_pix_stride",
                                    "s_c_off", "m_c_off")] + [("scale_bound", _f32), ("lik_bound", _f32)]


class TapeCall(C.Structure):
    """hesic_tape_call: a recorded launch (entry point id, its arguments as 64-bit words, the stream argument left out)."""
    _fields_ = [("fn", _i32), ("nargs", _i32), ("a", C.c_uint64 * 20)]


TAPE_IDS = {"hesic_joint_step": 0, "hesic_conv2d_forward": 1, "hesic_conv2d_forward_f32out": 2}


def tape_from_calls(calls):
    """``calls``: [(entry point name, ctypes arguments as passed to ``call``)] -> (TapeCall array, objects to keep alive).  Pointers and
    integers only; the trailing stream argument is dropped (the replaying C function supplies it)."""
    arr = (TapeCall * len(calls))()
    keep = []
    for t, (name, args) in zip(arr, calls):
        t.fn, t.nargs = TAPE_IDS[name], len(args) - 1
        for i, v in enumerate(args[:-1]):
            if v is None:
                w = 0
            elif isinstance(v, int):
                w = v
            elif isinstance(v, C.c_void_p):
                w = v.value or 0
            elif hasattr(v, "_obj"):                    # byref(struct)
                keep.append(v._obj)
                w = C.addressof(v._obj)
            elif isinstance(v, (C.Array, C.Structure)):
                keep.append(v)
                w = C.addressof(v)
            else:
                raise TypeError(f"tape_from_calls: {name} argument {i} of type {type(v).__name__}")
            t.a[i] = w & 0xFFFFFFFFFFFFFFFF
    return arr, keep


_P = C.POINTER
_SIGS = {
    "hesic_abi_version": ([], _i32),
    "hesic_h16_format": ([], _i32),
    "hesic_last_error": ([], C.c_char_p),
    "hesic_pack_conv_weight": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_joint_step": ([_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp], _i32),
    "hesic_probe_mfma_loop": ([_vp, _vp, _i32, _P(C.c_double), _vp], _i32),
    "hesic_joint_decode_groups": ([_i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_joint_decode_groups_tape": ([_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_ssim_scale": ([_vp, _P(_i64), _vp, _P(_i64), _i32, _i32, _i32, _i32, _f32, _vp, _vp], _i32),
    "hesic_avgpool2_pad": ([_vp, _P(_i64), _vp, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_pack_conv_weight_shaped": ([_vp, _vp, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_pack_conv_weight_shaped_tr": ([_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_pack_conv_weights_batched": ([_vp, _i32, _i32, _vp], _i32),
    "hesic_conv2d_forward": ([_P(ConvDesc), _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_gdn_forward_planar": ([_vp, _vp, _vp, _vp, _i32, _i32, _i64, _i32, _f32, _i32, _vp], _i32),
    "hesic_eb_prepare_params": ([_vp, _vp, _i32, _vp], _i32),
    "hesic_gmm_cdf": ([_P(GmmDesc), _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp], _i32),
    "hesic_gmm_cdf_rows": ([_P(GmmDesc), _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp], _i32),
    "hesic_maxpool2_forward": ([_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_perspective_transform": ([_vp, _vp, _vp, _i32, _vp], _i32),
    "hesic_h_from_delta": ([_vp, _vp, _f32, _f32, _i32, _vp, _i32, _vp], _i32),
    "hesic_conv2d_ws_bytes": ([_P(ConvDesc)], C.c_size_t),
    "hesic_conv2d_f32out_ws_bytes": ([_P(ConvDesc)], C.c_size_t),
    "hesic_conv2d_forward_ws": ([_P(ConvDesc), _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp], _i32),
    "hesic_gdn_pack_params": ([_vp, _vp, _f32, _vp, _vp, _i32, _vp], _i32),
    "hesic_conv2d_gdn_forward": ([_P(ConvDesc), _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp], _i32),
    "hesic_conv2d_gdn_forward_train": ([_P(ConvDesc), _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp], _i32),
    "hesic_conv2d_variant": ([_P(ConvDesc), _P(_i32)], _i32),
    "hesic_conv2d_hilo_variant": ([_P(ConvDesc), _i32, _i32, _P(_i32)], _i32),
    "hesic_conv2d_set_phase_fusion": ([_i32], _i32),
    "hesic_conv2d_wgrad_ws_bytes": ([_P(ConvDesc)], _i64),
    "hesic_conv2d_wgrad": ([_P(ConvDesc), _vp, _vp, _vp, _vp, _vp, _i64, _vp], _i32),
    "hesic_unpack_conv_wgrad": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_sconv2d_forward": ([_P(SConvDesc), _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_sconv2d_forward_cat": ([_P(SConvDesc), _vp, _vp, C.POINTER(C.c_int64), _i32, _i32, _vp, _vp, _vp, _vp], _i32),
    "hesic_sconv2d_forward_cat_gdn": ([_P(SConvDesc), _vp, _vp, C.POINTER(C.c_int64), _i32, _i32, _vp, _vp, _vp, _vp, C.c_float, _i32, _i32,
                                       _vp, _vp], _i32),
    "hesic_sconv2d_gdn_forward": ([_P(SConvDesc), _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp], _i32),
    "hesic_sconv_pack_weight_image": ([_i32, _vp, _vp, _vp, _vp], _i32),
    "hesic_sconv2d_forward_prepacked": ([_P(SConvDesc), _vp, _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_sconv2d_gdn_forward_prepacked": ([_P(SConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp], _i32),
    "hesic_sconv2d_dgrad": ([_P(SConvDesc), _vp, _vp, _vp, _vp], _i32),
    "hesic_sconv2d_wgrad_ws_bytes": ([_P(SConvDesc)], _i64),
    "hesic_sconv2d_wgrad": ([_P(SConvDesc), _vp, _vp, _vp, _vp, _vp, _i64, _vp], _i32),
    "hesic_gdn_forward": ([_vp, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _i32, _vp], _i32),
    "hesic_gdn_backward_ws_bytes": ([_i64, _i32], _i64),
    "hesic_gdn_backward": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _i32, _vp], _i32),
    "hesic_warp_perspective_forward": ([_P(WarpDesc), _vp, _vp, _vp, _vp], _i32),
    "hesic_warp_perspective_backward": ([_P(WarpDesc), _vp, _vp, _vp, _vp], _i32),
    "hesic_eb_forward": ([_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp], _i32),
    "hesic_eb_backward": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp], _i32),
    "hesic_gmm_forward": ([_P(GmmDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_gmm_backward": ([_P(GmmDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_upsample4_forward": ([_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_upsample4_backward": ([_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_copy_channels": ([_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_spatial_max": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_mix_weights_forward": ([_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp], _i32),
    "hesic_conv3x3_c32_forward": ([_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp], _i32),
    "hesic_pack_images_c32": ([_vp, _vp, _vp, _i32, _i32, _i32, _vp], _i32),
    "hesic_conv3x3_c32_forward_img6": ([_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp], _i32),
    "hesic_resblock_c32_forward": ([_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp], _i32),
    "hesic_adam_step": ([_vp, _vp], _i32),
    "hesic_pooled_linear_forward": ([_vp, _vp, _vp, _vp, _i32, _i32, _vp], _i32),
    "hesic_pooled_linear_backward": ([_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp], _i32),
    "hesic_softmax_k_forward": ([_vp, _vp, _i32, _i32, _i32, _vp], _i32),
    "hesic_softmax_k_backward": ([_vp, _vp, _vp, _i32, _i32, _i32, _vp], _i32),
    "hesic_sum_log2": ([_vp, _i64, _vp, _vp], _i32),
    "hesic_sum_sq_diff": ([_vp, _i32, _P(_i64), _vp, _i32, _P(_i64), _i32, _i32, _i32, _i32, _vp, _vp], _i32),
    "hesic_rd_sums": ([_i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_log_backward": ([_vp, _f32, _vp, _i64, _vp], _i32),
    "hesic_sq_diff_backward": ([_vp, _i32, _P(_i64), _vp, _i32, _P(_i64), _i32, _i32, _i32, _i32, _f32, _vp, _vp], _i32),
    "hesic_act_backward": ([_vp, _vp, _vp, _i64, _i32, _i32, _vp], _i32),
    "hesic_cast": ([_vp, _i32, _vp, _i32, _i64, _vp], _i32),
    "hesic_round": ([_vp, _i32, _vp, _i32, _i64, _vp], _i32),
    "hesic_conv2d_wgrad_direct": ([_P(ConvDesc), _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp], _i32),
    "hesic_conv2d_forward_grouped": ([_P(ConvDesc), _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp], _i32),
    "hesic_pack_conv_weight_slice": ([_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_conv2d_wgrad_partial": ([_P(ConvDesc), _vp, _vp, _vp, _i64, _vp], _i32),
    "hesic_conv2d_hilo_set_acc_scale": ([_f32], _i32),
    "hesic_sconv_pack_weight_image_hilo_scaled": ([_vp, _vp, _f32, _vp, _vp], _i32),
    "hesic_conv2d_wgrad_partial_batched": ([_i32, _P(ConvDesc), _P(_vp), _P(_vp), _P(_vp), _P(_i64), _P(_i32), _vp], _i32),
    "hesic_conv2d_wgrad_nsplit": ([_P(ConvDesc), _i32], _i32),
    "hesic_conv2d_wgrad_ws_bytes_n": ([_P(ConvDesc), _i32], _i64),
    "hesic_conv2d_wgrad_finish_batched_n": ([_i32, _P(ConvDesc), _P(_vp), _P(_vp), _P(_vp), _P(_vp), _i32, _P(_i32), _vp], _i32),
    "hesic_conv2d_wgrad_finish_batched": ([_i32, _P(ConvDesc), _P(_vp), _P(_vp), _P(_vp), _P(_vp), _i32, _vp], _i32),
    "hesic_gdn_backward_acc": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _f32, _i32, _vp], _i32),
    "hesic_gdn_backward_partial_ok": ([_i64, _i32, _i32], _i32),
    "hesic_gdn_backward_partial": ([_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _f32, _i32, _vp], _i32),
    "hesic_gdn_param_finish_batched": ([_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp], _i32),
    "hesic_gdn_backward_planar_acc": ([_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i64, _i32, _i32, _f32, _i32, _vp], _i32),
    "hesic_eb_pack_table": ([_P(EbLayout), _vp, _i32, _vp], _i32),
    "hesic_eb_scatter_grads": ([_P(EbLayout), _vp, _i32, _i32, _vp], _i32),
    "hesic_eb_aux_loss": ([_vp, _vp, _f32, _vp, _vp, _i32, _i32, _vp], _i32),
    "hesic_conv2d_forward_f32out": ([_P(ConvDesc), _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, C.c_size_t, _vp], _i32),
    "hesic_eb_forward_f32in": ([_vp, _vp, _vp, _i32, _vp, _vp, _i64, _i32, _vp], _i32),
    "hesic_gmm_forward_f32in": ([_P(GmmDesc), _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp], _i32),
    "hesic_conv2d_forward_hilo": ([_P(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, C.c_size_t, _vp], _i32),
    "hesic_conv2d_forward_hilo_w1": ([_P(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, C.c_size_t, _vp], _i32),
    "hesic_conv2d_hilo_ws_bytes": ([_P(ConvDesc)], C.c_size_t),
    "hesic_gdn_pack_params_lo": ([_vp, _vp, _i32, _vp], _i32),
    "hesic_gdn_pack_params_batched": ([_vp, _i32, _vp], _i32),
    "hesic_spatial_max_backward": ([_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_rd_loss_combine": ([_vp, C.c_double, C.c_int64, C.c_int64, _vp, _vp], _i32),
    "hesic_sconv_pack_weight_image_hilo": ([_vp, _vp, _vp, _vp], _i32),
    "hesic_sconv_pack_weight_image_hilo_out1": ([_vp, _vp, _vp, _vp], _i32),
    "hesic_sconv2d_gdn_forward_hilo": ([_P(SConvDesc), _vp, _vp, _vp, _vp, _i32, _vp, _vp], _i32),
    "hesic_sconv2d_gdn_forward_hilo_out1": ([_P(SConvDesc), _vp, _vp, _vp, _vp, _i32, _vp, _vp], _i32),
    "hesic_conv2d_gdn_forward_hilo_out": ([_P(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp], _i32),
    "hesic_conv3x3_c32_wgrad_ws_bytes": ([], _i64),
    "hesic_conv3x3_c32_wgrad": ([_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _i32, _i32, _i32, _vp], _i32),
    "hesic_im2col_hilo": ([_vp, _P(_i64), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp], _i32),
}

# include/hesic_stereo_h.h: the stereo homography estimator (hesic_amd.stereo_h), in both libraries
_u32 = C.c_uint32
_STEREO_H_SIGS = {
    "hesic_stereo_h_det_elems": ([_i32, _i32], _i64),
    "hesic_stereo_h_ws_bytes": ([_i32, _i32, _i32, _i32, _i32], C.c_size_t),
    "hesic_stereo_h_integral": ([_vp, _i32, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp], _i32),
    "hesic_stereo_h_hessian": ([_vp, _i32, _i32, _i32, _vp, _vp], _i32),
    "hesic_stereo_h_keypoints": ([_vp, _i32, _i32, _i32, _i32, _i32, _vp, C.c_size_t, _vp, _vp, _vp], _i32),
    "hesic_stereo_h_describe": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp], _i32),
    "hesic_stereo_h_match": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, C.c_size_t, _vp, _vp, _vp], _i32),
    "hesic_stereo_h_orient": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp], _i32),
    "hesic_stereo_h_describe_ex": ([_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp], _i32),
    "hesic_stereo_h_match_ex": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, C.c_size_t, _vp, _vp, _vp], _i32),
    "hesic_stereo_h_ransac": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _u32, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp, _vp],
                              _i32),
}

# include/hesic_codec.h: the device-resident range coder of the HESIC latents (HSIC.compress_batch / decompress_batch), in both libraries
CODEC_MAX_ALPHABET = 1024       # HESIC_CODEC_MAX_ALPHABET
CODEC_OVERFLOW, CODEC_BAD_SYMBOL = 1, 2
_CODEC_SIGS = {
    "hesic_rc_stream_cap": ([_i64], _i64),
    "hesic_gmm_rc_ranges": ([_P(GmmDesc), _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp], _i32),
    "hesic_rc_encode_streams": ([_vp, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp], _i32),
    "hesic_rc_compact_streams": ([_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp], _i32),
    "hesic_gmm_rc_decode": ([_P(GmmDesc), _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _i32, _vp], _i32),
    # HESIC+ (HSICJoint.compress_batch / decompress_batch): wavefront-ordered streams
    "hesic_rc_encode_streams_ordered": ([_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _vp, _vp], _i32),
    "hesic_joint_gather_batch": ([_vp, _i32, _i32, _i32, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp], _i32),
    "hesic_gmm_rc_decode_step": ([_P(GmmDesc), _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _i64, _vp],
                                 _i32),
}

# include/hesic_msssim_loss.h: the backward of hesic_ssim_scale (functional.ms_ssim, rd_loss(distortion="ms-ssim")), in both libraries
_MSSSIM_LOSS_SIGS = {
    "hesic_ssim_scale_backward": ([_vp, _P(_i64), _vp, _P(_i64), _i32, _i32, _i32, _i32, _f32, _vp, _P(_i64), _P(C.c_double), _i32, _i32, _vp,
                                   _vp, _vp, _vp], _i32),
}

# include/hesic_train_ctl.h: device-resident step controls of the training step (train.FlatAdam on the control path), in both libraries
_TRAIN_CTL_SIGS = {
    "hesic_grad_norm_ctl": ([_vp, _i64, _vp, _vp, _vp, _vp], _i32),
    "hesic_adam_step_ctl": ([_vp, _vp, _vp], _i32),
}
# the control block (HESIC_TRAIN_CTL_* of that header): fp32 entries, and the fp64 partials hesic_grad_norm_ctl needs
CTL_LR, CTL_MAX_NORM, CTL_SKIP_NONFINITE, CTL_GRAD_NORM, CTL_CLIP_COEF, CTL_APPLIED, CTL_SKIPPED, CTL_FLOATS = 0, 1, 2, 3, 4, 5, 6, 8
GRAD_NORM_MAX_BLOCKS = 1024

# include/hesic_homography_train.h: the photometric loss of HomographyNet's training, d(warp_perspective)/dM and the DLT adjoint
# (homography.photometric_loss, functional._WarpMFn, homography.get_perspective_transform / h_matrix_from_delta), in both libraries
_HOMOGRAPHY_TRAIN_SIGS = {
    "hesic_photometric_forward": ([_P(WarpDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_photometric_backward": ([_P(WarpDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_warp_perspective_backward_m": ([_P(WarpDesc), _vp, _vp, _vp, _vp, _vp, _vp], _i32),
    "hesic_perspective_transform_backward": ([_vp, _vp, _vp, _vp, _vp, _i32, _vp], _i32),
    "hesic_h_from_delta_backward": ([_vp, _vp, _f32, _f32, _i32, _vp, _vp, _i32, _vp], _i32),
}
HTRAIN_MAX_BLOCKS, HTRAIN_PARTIAL_WIDTH = 64, 9      # fp64 partials per image of the workspace those entry points take

# include/hesic_homography_net.h: HomographyNet in training mode -- max-pool backward, flatten + dropout, the small-batch Linear layer over
# the fp32 master weight (functional._MaxPool2Fn / _FlattenDropoutFn / _LinearFn, homography.Net, train.HomographyTrainer), in both libraries
_u64 = C.c_uint64
_HOMOGRAPHY_NET_SIGS = {
    "hesic_maxpool2_backward": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_flatten_dropout_forward": ([_vp, _vp, _i32, _i32, _i32, _u32, _f32, _u64, _u32, _u32, _i32, _vp], _i32),
    "hesic_flatten_dropout_backward": ([_vp, _vp, _i32, _i32, _i32, _u32, _f32, _u64, _u32, _u32, _i32, _vp], _i32),
    "hesic_linear_forward_ws_bytes": ([_i32, _i32, _i32], C.c_size_t),
    "hesic_linear_forward": ([_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, C.c_size_t, _vp], _i32),
    "hesic_linear_dgrad": ([_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_linear_wgrad": ([_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
    "hesic_bias_grad": ([_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp], _i32),
    "hesic_narrow_in_wgrad": ([_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp], _i32),
}
# include/hesic_dropout_state.h: the same dropout masks with (seed, step) in device memory (functional.dropout_state_take,
# homography.Net.dropout_on_device, train.GraphedHomographyTrainer), in both libraries
_DROPOUT_STATE_SIGS = {
    "hesic_dropout_state_take": ([_vp, _vp, _vp], _i32),
    "hesic_flatten_dropout_forward_state": ([_vp, _vp, _i32, _i32, _i32, _u32, _f32, _vp, _u32, _i32, _vp], _i32),
    "hesic_flatten_dropout_backward_state": ([_vp, _vp, _i32, _i32, _i32, _u32, _f32, _vp, _u32, _i32, _vp], _i32),
}
LINEAR_MAX_ROWS = 64            # HESIC_LINEAR_MAX_ROWS
DET_MAX_BLOCKS = 256            # HESIC_DET_MAX_BLOCKS

# include/hesic_homography_prep.h: a stereo pair on the device -> HomographyNet's inputs in one launch (functional.homonet_prepare,
# homography.prepare_inputs / h_matrix_from_pair, train.HomographyTrainer.step_pairs), in both libraries
_HOMOGRAPHY_PREP_SIGS = {
    "hesic_homonet_prepare": ([_vp, _P(_i64), _vp, _P(_i64), _vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
                              _i32),
}
PREP_U8, PREP_F32 = 0, 1        # HESIC_PREP_U8 / HESIC_PREP_F32


# include/hesic_homonet_items.h (included by hesic_homography_prep.h): the same step from stored uint8 images of per-item address and size
# (functional.homonet_prepare_items, pair_cache.DevicePairCache.homonet_batch, ``python -m hesic_amd.homography_train --cache device|stream``),
# in both libraries
class HomonetItem(C.Structure):
    """hesic_homonet_item (48 bytes)."""
    _fields_ = [("left", C.c_uint64), ("right", C.c_uint64)] + \
               [(n, _i32) for n in ("pitch_px", "rows", "x0", "y0", "cw", "ch", "wx", "wy")]


_HOMONET_ITEMS_SIGS = {
    "hesic_homonet_prepare_items": ([_vp, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
}


# include/hesic_homonet_synth.h: synthetic-warp pairs with their label from one stored view (functional.homonet_synth,
# pair_cache.DevicePairCache.homonet_synth_batch, ``python -m hesic_amd.homography_train --supervision synthetic``, ``python -m
# hesic_amd.homography_eval``), in both libraries
class HomonetSynthItem(C.Structure):
    """hesic_homonet_synth_item (72 bytes)."""
    _fields_ = [("view", C.c_uint64)] + [(n, _i32) for n in ("pitch_px", "rows", "x0", "y0", "cw", "ch", "wx", "wy")] + [("delta", _i32 * 8)]


_HOMONET_SYNTH_SIGS = {
    "hesic_homonet_synth_items": ([_vp, _i32, _i32, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _i32),
}


# include/hesic_pair_batch.h: a batch of stereo crops gathered from uint8 images resident on the device, with the re-based homographies, in one
# launch (functional.pair_batch_gather, pair_cache.DevicePairCache.batch, ``python -m hesic_amd.train_folder``), in both libraries
class PairItem(C.Structure):
    """hesic_pair_item (48 bytes)."""
    _fields_ = [("left", C.c_uint64), ("right", C.c_uint64)] + \
               [(n, _i32) for n in ("pitch_px", "rows", "x0", "y0", "hx", "hy", "h_index", "reserved")]


_PAIR_BATCH_SIGS = {
    "hesic_pair_batch_gather": ([_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp], _i32),
}

# include/hesic_pair_augment.h: the same gather with the descriptor's ``reserved`` word read as flip / swap bits (functional.pair_batch_gather_aug,
# pair_cache.DevicePairCache.batch(flags=...), ``--augment`` of the folder trainers), in both libraries
_PAIR_AUGMENT_SIGS = {
    "hesic_pair_batch_gather_aug": ([_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp], _i32),
}
PAIR_HFLIP, PAIR_VFLIP, PAIR_SWAP = 1, 2, 4         # HESIC_PAIR_HFLIP, HESIC_PAIR_VFLIP, HESIC_PAIR_SWAP

# include/hesic_pair_metrics.h: bits per likelihood map, squared error and 8-bit squared error per view as one fp64 row PER PAIR of a batch,
# without atomics (functional.pair_metrics, models.pair_metrics, ``python -m hesic_amd.eval_folder``), in both libraries
_PAIR_METRICS_SIGS = {
    "hesic_pair_metrics_ws_bytes": ([_i32, _i32, _P(_i64), _i32, _i32], _i64),
    "hesic_pair_metrics": ([_i32, _i32, _vp, _P(_i64), _vp, _P(_i32), _P(_i64), _vp, _P(_i32), _P(_i64), _i32, _i32, _i32, _vp, _vp, _i64, _vp], _i32),
}
PAIR_METRICS_MAX_LIK = 8        # HESIC_PAIR_METRICS_MAX_LIK


# include/hesic_en_train.h: the stage-2 criterion of both views, its gradient as the output layer's 32-channel map, and the data-gradient weights of
# a flat parameter buffer's convs in one launch (functional.en_criterion, train.EnhancerTrainer, ``python -m hesic_amd.train_stage2``), in both libraries
class MirrorEntry(C.Structure):
    """hesic_mirror_entry (32 bytes)."""
    _fields_ = [("src", _i64), ("dst", _i64), ("cout", _i32), ("cin", _i32), ("cout_pad", _i32), ("reserved", _i32)]


_EN_TRAIN_SIGS = {
    "hesic_en_loss_ws_bytes": ([_i32, _i32, _i32], _i64),
    "hesic_en_loss": ([_vp, _vp, _vp, _vp, _i32, _i32, _i32, C.c_double, _vp, _vp, _i64, _vp], _i32),
    "hesic_en_loss_grad": ([_vp, _vp, _vp, _vp, _i32, _i32, _i32, C.c_double, _vp, _vp, _vp, _vp], _i32),
    "hesic_c32_mirror_weights": ([_vp, _i64, _vp, _i64, _vp, _i32, _i32, _vp], _i32),
}

# include/hesic_rans.h: the device rANS coder for batches of independent streams, byte for byte the host coder's (functional.rans_encode /
# rans_decode, EntropyBottleneck.compress_device / decompress_device, compress_batch / decompress_batch(z_coder="device")), in both libraries
_RANS_SIGS = {
    "hesic_rans_slot_bytes": ([_i64], _i64),
    "hesic_rans_encode_ws_bytes": ([_i64, _i64], _i64),
    "hesic_rans_encode": ([_vp, _i64, _i64, _i64, _i32, _i64, _i64, _vp, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp,
                           _i32, _vp], _i32),
    "hesic_rans_compact": ([_vp, _i64, _vp, _vp, _i32, _vp, _i64, _vp], _i32),
    "hesic_rans_decode": ([_vp, _i64, _vp, _vp, _i32, _i64, _i64, _vp, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _i32, _vp,
                           _vp], _i32),
}
RANS_MAX_ROW = 512              # HESIC_RANS_MAX_ROW

# include/hesic_homography_refine.h: photometric Gauss-Newton / Levenberg-Marquardt refinement of a pair's homography on a grey pyramid
# (functional.homography_refine, homography.refine_h_matrix, ``codec encode --refine-homography``), in both libraries
_f64 = C.c_double
_HOMOGRAPHY_REFINE_SIGS = {
    "hesic_hrefine_levels": ([_i32, _i32, _i32], _i32),
    "hesic_hrefine_blocks": ([_i32, _i32], _i32),
    "hesic_hrefine_pyramid_elems": ([_i32, _i32, _i32, _i32], _i64),
    "hesic_homography_refine_ws_bytes": ([_i32, _i32, _i32, _i32], _i64),
    "hesic_hrefine_pyramid": ([_vp, _P(_i64), _vp, _P(_i64), _i32, _i32, _i32, _i32, _i32, _vp, _vp], _i32),
    "hesic_hrefine_normal_eq": ([_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _f64, _vp, _vp], _i32),
    "hesic_homography_refine": ([_vp, _P(_i64), _vp, _P(_i64), _i32, _i32, _i32, _i32, _vp, _i32, _i32, _f64, _f64, _vp, _i64, _vp, _vp, _vp],
                                _i32),
}
HREFINE_MAX_LEVELS, HREFINE_MIN_SIDE, HREFINE_SUMS, HREFINE_INFO = 6, 16, 46, 8      # HESIC_HREFINE_* of that header
RANS_OVERFLOW, RANS_BAD_TABLE, RANS_BAD_ESCAPE, RANS_BAD_STREAM = 1, 2, 4, 8

_libs = {}                      # torch 16-bit dtype -> CDLL
_h16 = torch.bfloat16           # the active 16-bit format
_lib = None                     # the active library (None until first use)


# every public header under include/ -> the signatures of the entry points its own text declares, in binding order.  A new header gets its
# dict above and one line here; tests/test_abi.py holds the table to the directory, to the headers' text and to both libraries' exports
HEADERS = {
    "hesic_hip.h": _SIGS,
    "hesic_stereo_h.h": _STEREO_H_SIGS,
    "hesic_codec.h": _CODEC_SIGS,
    "hesic_msssim_loss.h": _MSSSIM_LOSS_SIGS,
    "hesic_train_ctl.h": _TRAIN_CTL_SIGS,
    "hesic_homography_train.h": _HOMOGRAPHY_TRAIN_SIGS,
    "hesic_homography_net.h": _HOMOGRAPHY_NET_SIGS,
    "hesic_dropout_state.h": _DROPOUT_STATE_SIGS,
    "hesic_homography_prep.h": _HOMOGRAPHY_PREP_SIGS,
    "hesic_homonet_items.h": _HOMONET_ITEMS_SIGS,
    "hesic_homonet_synth.h": _HOMONET_SYNTH_SIGS,
    "hesic_pair_batch.h": _PAIR_BATCH_SIGS,
    "hesic_pair_augment.h": _PAIR_AUGMENT_SIGS,
    "hesic_pair_metrics.h": _PAIR_METRICS_SIGS,
    "hesic_en_train.h": _EN_TRAIN_SIGS,
    "hesic_rans.h": _RANS_SIGS,
    "hesic_homography_refine.h": _HOMOGRAPHY_REFINE_SIGS,
}


def header_path(name):
    """The path of the public header ``name`` (a key of ``HEADERS``) under include/."""
    return os.path.join(_INCLUDE, name)


def declared_symbols(header="hesic_hip.h"):
    """Every ``hesic_*`` function declared in the text of include/``header`` itself, not of the headers it includes (used by the ABI tests)."""
    with open(header_path(header)) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(hesic_[a-z0-9_]+)\s*\(", text)))


def _load(h16):
    l = _libs.get(h16)
    if l is None:
        path = LIB_PATH_F16 if h16 == torch.float16 else LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(
                f"hesic_amd: {path} is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C hesic_amd/csrc`. There is no CPU fallback.")
        l = C.CDLL(path)
        # the version check comes BEFORE the signatures are bound: a stale build then fails with the rebuild hint instead of an AttributeError
        # on the first entry point it lacks
        rebuild = "rebuild it with `python -c 'import __graft_entry__ as g; g.build()'` or `make -C hesic_amd/csrc`"
        try:
            l.hesic_abi_version.argtypes, l.hesic_abi_version.restype = [], _i32
            ver = l.hesic_abi_version()
        except AttributeError:
            raise RuntimeError(f"hesic_amd: {os.path.basename(path)} exports no hesic_abi_version -- not this package's library; {rebuild}") from None
        if ver != ABI_VERSION:
            raise RuntimeError(f"hesic_amd: {os.path.basename(path)} ABI version mismatch (library {ver}, package {ABI_VERSION}): {rebuild}")
        for sigs in HEADERS.values():
            for name, (args, res) in sigs.items():
                try:
                    fn = getattr(l, name)
                except AttributeError:
                    raise RuntimeError(f"hesic_amd: {os.path.basename(path)} lacks the entry point {name} although it reports ABI {ver}: "
                                       f"{rebuild}") from None
                fn.argtypes, fn.restype = args, res
        if l.hesic_h16_format() != (1 if h16 == torch.float16 else 0):
            raise RuntimeError(f"hesic_amd: {os.path.basename(path)} was built for the other 16-bit format")
        _libs[h16] = l
    return l


def lib(h16=None):
    """The active library (or the one built for ``h16`` = torch.bfloat16 / torch.float16)."""
    global _lib
    if h16 is not None:
        return _load(h16)
    if _lib is None:
        _lib = _load(_h16)
    return _lib


def use_h16(dtype):
    """Select the 16-bit format (torch.bfloat16 or torch.float16) -- i.e. the library -- every following call goes to."""
    global _h16, _lib
    if dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("the 16-bit storage format is torch.bfloat16 or torch.float16")
    if dtype != _h16 or _lib is None:
        _lib = _load(dtype)
        _h16 = dtype


def h16_dtype():
    """torch dtype of HESIC_H16 storage in the active library."""
    return _h16


_tls = threading.local()


class call_hook:
    """``with call_hook(fn):`` -- ``fn(name, args)`` sees every ``call`` the CURRENT THREAD makes inside the block (launch tapes, the
    segment recorder).  Thread-local: a launch from another thread (a second model, a prefetch or metrics thread) during a recording
    neither lands on the tape nor marks a segment.  Hooks nest (the inner one runs first)."""

    def __init__(self, fn):
        self.fn = fn

    def __enter__(self):
        hooks = getattr(_tls, "hooks", None)
        if hooks is None:
            hooks = _tls.hooks = []
        hooks.append(self.fn)
        return self

    def __exit__(self, *exc):
        _tls.hooks.remove(self.fn)
        return False


def call(name, *args):
    hooks = getattr(_tls, "hooks", None)
    if hooks:
        for h in reversed(hooks):
            h(name, args)
    rc = getattr(_lib or lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed (rc={rc}): {lib().hesic_last_error().decode()}")


def dt(t_or_dtype) -> int:
    d = t_or_dtype.dtype if torch.is_tensor(t_or_dtype) else t_or_dtype
    if d == torch.float32:
        return F32
    if d == _h16:
        return H16
    if d in (torch.bfloat16, torch.float16):
        raise TypeError(f"hesic_amd: a {d} tensor while the active 16-bit format is {_h16} (set_compute_dtype selects it)")
    raise TypeError(f"hesic_amd: unsupported dtype {d} (float32, bfloat16 or float16)")


def ptr(t):
    return None if t is None else _vp(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """The current device's current HIP stream as a void*.  ``torch.cuda.current_stream()`` costs ~5 us per call (device-index
    normalisation, ``is_available()`` with its environment look-ups, a Stream object): at ~70 launches per forward that was a
    quarter of the host time of an eager forward; the raw accessors are two C calls."""
    if _raw_stream is not None:
        return _vp(_raw_stream(_cur_device()))
    return _vp(torch.cuda.current_stream().cuda_stream)


def require_cuda(*tensors):
    """Every kernel is launched on the CURRENT device's current stream: refuse CPU tensors (no fallback) and tensors of
    another GPU (the launch would run on the wrong device against foreign pointers)."""
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("hesic_amd: the HIP path needs tensors on a ROCm device (no CPU fallback); "
                               f"got a tensor on {t.device}")
        if cur is None:
            cur = _cur_device() if _cur_device is not None else torch.cuda.current_device()
        if t.device.index != cur:
            raise RuntimeError(f"hesic_amd: tensor on {t.device} but the current device is cuda:{cur} -- kernels launch on the current "
                               "device's stream; wrap the call in `with torch.cuda.device(tensor.device):`")
