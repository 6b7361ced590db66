"""ctypes binding of libhdrnet_amd.so -- the C-ABI declared in include/hdrnet_amd.h.

The library is the product: there is NO fallback.  If it cannot be built / loaded the
import of the ops fails loudly (``HdrnetLibraryError``); nothing here routes to PyTorch
eager code or to any CPU checker.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional

HDRNET_OK = 0
HDRNET_INVALID_ARGUMENT = 1
HDRNET_RUNTIME_FAILURE = 2

KERNEL_AUTO = 0
GUIDE_SIGMOID_FAST = 0x10000  # HDRNET_GUIDE_SIGMOID_FAST (flags of the guide-network ..._ex entry points)
GUIDE_RELU_PRESCALED = 0x20000  # HDRNET_GUIDE_RELU_PRESCALED: conv1 / conv2 are hdrnet_guide_nn_prescale_f32's arrays
KERNEL_GENERIC = 1
KERNEL_FAST = 2
SAMPLE_EVEN_TURNS_ONLY = 1  # HDRNET_SAMPLE_EVEN_TURNS_ONLY (hdrnet_prepare_batch, include/hdrnet_amd_train.h)

_FP = ctypes.c_void_p  # device pointers travel as integers (tensor.data_ptr())
_I = ctypes.c_int
_U = ctypes.c_uint
_SZ = ctypes.c_size_t
_VP = ctypes.c_void_p

# name -> (restype, argtypes); must list every symbol include/hdrnet_amd.h declares
# (tests/test_capi_symbols.py cross-checks this table against the header).
SIGNATURES = {
    "hdrnet_version": (_I, []),
    "hdrnet_last_error": (ctypes.c_char_p, []),
    "hdrnet_last_kernel": (ctypes.c_char_p, []),
    "hdrnet_enable_kernel_names": (None, [_I]),
    "hdrnet_bilateral_slice_apply_f32": (_I, [_FP] * 4 + [_I] * 9 + [_VP]),
    "hdrnet_bilateral_slice_apply_f32_ex": (_I, [_FP] * 4 + [_I] * 9 + [_U, _VP]),
    "hdrnet_bilateral_slice_apply_rows_f32": (_I, [_FP] * 4 + [_I] * 11 + [_VP]),
    "hdrnet_bilateral_slice_apply_rows_f32_ex": (_I, [_FP] * 4 + [_I] * 11 + [_U, _VP]),
    "hdrnet_bilateral_slice_apply_nnguide_f32": (_I, [_FP] * 6 + [_I] * 10 + [_VP]),
    "hdrnet_bilateral_slice_apply_nnguide_f32_ex": (_I, [_FP] * 6 + [_I] * 10 + [_U, _VP]),
    "hdrnet_bilateral_slice_apply_io_curves": (_I, [_FP] * 3 + [_I] * 10 + [ctypes.c_float, _I] + [_FP] * 4 + [_I, _FP, _VP]),
    "hdrnet_curves_guide_prepared_bytes": (_SZ, [_I]),
    "hdrnet_curves_guide_prepare_f32": (_I, [_FP, _FP, _I, _I, _VP, _SZ, ctypes.POINTER(ctypes.c_int), _VP]),
    "hdrnet_bilateral_slice_apply_io_curves_prepared": (_I, [_FP] * 3 + [_I] * 10 + [ctypes.c_float, _I] + [_FP] * 4 + [_I, _VP, _FP, _VP]),
    "hdrnet_bilateral_slice_apply_upadd_f32": (_I, [_FP] * 4 + [_I, _I, _FP] + [_I] * 9 + [_FP, _FP, _I, _VP]),
    "hdrnet_bilateral_slice_apply_upadd_f32_ex": (_I, [_FP] * 4 + [_I, _I, _FP] + [_I] * 9 + [_FP, _FP, _I, _U, _VP]),
    "hdrnet_resize_bilinear_f32": (_I, [_FP, _FP] + [_I] * 6 + [_VP]),
    "hdrnet_pointwise_guide_grad_workspace_bytes": (_SZ, [ctypes.c_longlong, _I, _I]),
    "hdrnet_pointwise_guide_grad_f32": (_I, [_FP] * 6 + [_I] + [_FP] * 2 + [ctypes.c_longlong, _I, _I, _VP, _SZ, _VP]),
    "hdrnet_curves_guide_grad_workspace_bytes": (_SZ, [ctypes.c_longlong, _I, _I]),
    "hdrnet_curves_guide_grad_f32": (_I, [_FP] * 7 + [_I] + [_FP] * 4 + [ctypes.c_longlong, _I, _I, _VP, _SZ, _VP]),
    "hdrnet_input_moments_workspace_bytes": (_SZ, [ctypes.c_longlong, _I]),
    "hdrnet_input_moments_f32": (_I, [_FP, ctypes.c_longlong, _I, _FP, _FP, _VP, _SZ, _VP]),
    "hdrnet_l2_loss_workspace_bytes": (_SZ, [ctypes.c_longlong]),
    "hdrnet_l2_loss_f32": (_I, [_FP, _FP, ctypes.c_longlong, _FP, _VP, _SZ, _VP]),
    "hdrnet_l2_loss_grad_f32": (_I, [_FP, _FP, _FP, ctypes.c_longlong, _FP, _VP]),
    "hdrnet_guide_nn_prescale_f32": (_I, [_FP, _FP, _I, _I, ctypes.c_float, _FP, _FP, _VP]),
    "hdrnet_guide_fold_batch_f32": (_I, [_FP, _FP, ctypes.c_longlong] + [_FP] * 5 + [ctypes.c_double, ctypes.c_double, _I, _I] + [_FP] * 5 + [_VP]),
    "hdrnet_guide_fold_batch_grad_f32": (_I, [_FP, _FP, ctypes.c_longlong] + [_FP] * 3 + [ctypes.c_double, _I, _I] + [_FP] * 6 + [_VP]),
    "hdrnet_coefficients_workspace_bytes": (_SZ, [_VP, _I]),
    "hdrnet_coefficients_f32": (_I, [_FP, _VP, _FP, _I, _VP, _SZ, _VP]),
    "hdrnet_coefficients_grad_workspace_bytes": (_SZ, [_VP, _I]),
    "hdrnet_coefficients_grad_f32": (_I, [_FP, _VP, _VP, _FP, _VP, _I, _VP, _SZ, _VP]),
    "hdrnet_bilateral_slice_apply_io": (_I, [_FP] * 4 + [_I] * 10 + [ctypes.c_float, _I] + [_FP] * 2 + [_I, _FP, _VP]),
    "hdrnet_bilateral_slice_apply_io_ex": (_I, [_FP] * 4 + [_I] * 10 + [ctypes.c_float, _I] + [_FP] * 2 + [_I, _FP, _U, _VP]),
    "hdrnet_bilateral_slice_apply_grad_workspace_bytes": (_SZ, [_I] * 9),
    "hdrnet_bilateral_slice_apply_grad_f32": (_I, [_FP] * 7 + [_I] * 9 + [_VP, _SZ, _VP]),
    "hdrnet_bilateral_slice_apply_grad_f32_ex": (_I, [_FP] * 7 + [_I] * 9 + [_VP, _SZ, _U, _VP]),
    "hdrnet_bilateral_slice_f32": (_I, [_FP] * 3 + [_I] * 7 + [_VP]),
    "hdrnet_bilateral_slice_f32_ex": (_I, [_FP] * 3 + [_I] * 7 + [_U, _VP]),
    "hdrnet_bilateral_slice_grad_workspace_bytes": (_SZ, [_I] * 7),
    "hdrnet_bilateral_slice_grad_f32": (_I, [_FP] * 5 + [_I] * 7 + [_VP, _SZ, _VP]),
    "hdrnet_bilateral_slice_grad_f32_ex": (_I, [_FP] * 5 + [_I] * 7 + [_VP, _SZ, _U, _VP]),
    "hdrnet_lowres_input": (_I, [_FP, _I, ctypes.c_float] + [_I] * 3 + [_FP, _I, _VP]),
}


class CoeffNet(ctypes.Structure):
    """``hdrnet_coeff_net`` of include/hdrnet_amd.h (the coefficient network's hyper-parameters and parameters)."""

    _fields_ = [("net_input_size", _I), ("spatial_bin", _I), ("luma_bins", _I), ("channel_multiplier", _I),
                ("n_out", _I), ("n_in", _I), ("n_levels", _I),
                ("splat_w", _VP * 8), ("splat_b", _VP * 8),
                ("global_conv_w", _VP * 2), ("global_conv_b", _VP * 2),
                ("fc_w", _VP * 3), ("fc_b", _VP * 3),
                ("local_w", _VP * 2), ("local_b", _VP * 2),
                ("pred_w", _VP), ("pred_b", _VP), ("fc_layout", _I)]


class CoeffNetGrads(ctypes.Structure):
    """``hdrnet_coeff_net_grads``: where ``hdrnet_coefficients_grad_f32`` writes the parameter gradients."""

    _fields_ = [("splat_w", _VP * 8), ("splat_b", _VP * 8),
                ("global_conv_w", _VP * 2), ("global_conv_b", _VP * 2),
                ("fc_w", _VP * 3), ("fc_b", _VP * 3),
                ("local_w", _VP * 2), ("local_b", _VP * 2),
                ("pred_w", _VP), ("pred_b", _VP)]


class CoeffNetBn(ctypes.Structure):
    """``hdrnet_coeff_net_bn`` of include/hdrnet_amd_coeff_bn.h: the network description (its ``net`` member, spelled out:
    the same memory) and, per normalised layer, beta and the running statistics."""

    _fields_ = CoeffNet._fields_ + [
        ("splat_beta", _VP * 8), ("splat_running_mean", _VP * 8), ("splat_running_var", _VP * 8),
        ("global_conv_beta", _VP * 2), ("global_conv_running_mean", _VP * 2), ("global_conv_running_var", _VP * 2),
        ("fc_beta", _VP * 2), ("fc_running_mean", _VP * 2), ("fc_running_var", _VP * 2),
        ("local_beta", _VP), ("local_running_mean", _VP), ("local_running_var", _VP),
        ("eps", ctypes.c_float), ("momentum", ctypes.c_float)]


class CoeffNetBnGrads(ctypes.Structure):
    """``hdrnet_coeff_net_bn_grads``: ``hdrnet_coeff_net_grads`` (spelled out) and where the gradients of beta go."""

    _fields_ = CoeffNetGrads._fields_ + [("splat_beta", _VP * 8), ("global_conv_beta", _VP * 2), ("fc_beta", _VP * 2),
                                         ("local_beta", _VP)]


class HdrnetLibraryError(RuntimeError):
    """libhdrnet_amd.so is missing, failed to build, or failed to load."""


class HdrnetInvalidArgument(ValueError):
    """HDRNET_INVALID_ARGUMENT (the reference: tensorflow::errors::InvalidArgument)."""


class HdrnetRuntimeError(RuntimeError):
    """HDRNET_RUNTIME_FAILURE (the reference: errors::Internal("... kernel failed."))."""


# include/hdrnet_amd_train.h: training-loop helpers outside the operator boundary (same library).
TRAIN_SIGNATURES = {
    "hdrnet_l2_loss_with_grad_f32": (_I, [_FP, _FP, ctypes.c_longlong, _FP, _FP, _VP, ctypes.c_size_t, _VP]),
    "hdrnet_l2_loss_grad_scale_f32": (_I, [_FP, _FP, ctypes.c_longlong, _VP]),
    "hdrnet_loss_psnr_workspace_bytes": (_SZ, [ctypes.c_longlong, _I]),
    "hdrnet_loss_psnr_f32": (_I, [_FP, _FP, ctypes.c_longlong, _I] + [_FP] * 5 + [ctypes.c_float, _FP, _VP, _SZ, _VP]),
    "hdrnet_resize_add_f32": (_I, [_FP, _FP, _FP] + [_I] * 6 + [_VP]),
    "hdrnet_resize_bilinear_grad_f32": (_I, [_FP, _FP] + [_I] * 6 + [_VP]),
    "hdrnet_adam_step_f32": (_I, [_FP, _FP, _FP, _FP, ctypes.c_longlong, _FP] + [ctypes.c_float] * 4 + [_VP]),
    "hdrnet_adam_step_tf_f32": (_I, [_FP, _FP, _FP, _FP, ctypes.c_longlong, _FP] + [ctypes.c_float] * 4 + [_VP]),
    "hdrnet_prepare_batch": (_I, [_FP, _I, ctypes.c_float] * 2 + [_I] * 3 + [_FP, _I, _FP, _FP, _I, _I, _FP, _I, _U, _VP]),
    "hdrnet_prepare_batch_ragged": (_I, [_FP, _I, ctypes.c_float] * 2 + [ctypes.c_longlong, _FP, _I] +
                                    [_FP, _I, _FP, _FP, _I, _I, _FP, _I, _U, _VP]),
}

# include/hdrnet_amd_coeff_bn.h (included by hdrnet_amd_train.h): the coefficient network trained with batch norm.
COEFF_BN_SIGNATURES = {
    "hdrnet_coefficients_bn_workspace_bytes": (_SZ, [_VP, _I]),
    "hdrnet_coefficients_bn_train_f32": (_I, [_FP, _VP, _FP, _I, _VP, _SZ, _VP]),
    "hdrnet_coefficients_bn_grad_workspace_bytes": (_SZ, [_VP, _I]),
    "hdrnet_coefficients_bn_grad_f32": (_I, [_FP, _VP, _VP, _FP, _VP, _I, _VP, _SZ, _VP]),
}

# include/hdrnet_amd_coeff_wide.h (included by hdrnet_amd_train.h): the same training entry points for batches up to 32.
COEFF_WIDE_SIGNATURES = {
    "hdrnet_coefficients_grad_wide_workspace_bytes": (_SZ, [_VP, _I]),
    "hdrnet_coefficients_grad_wide_f32": (_I, [_FP, _VP, _VP, _FP, _VP, _I, _VP, _SZ, _VP]),
    "hdrnet_coefficients_bn_wide_workspace_bytes": (_SZ, [_VP, _I]),
    "hdrnet_coefficients_bn_train_wide_f32": (_I, [_FP, _VP, _FP, _I, _VP, _SZ, _VP]),
    "hdrnet_coefficients_bn_grad_wide_workspace_bytes": (_SZ, [_VP, _I]),
    "hdrnet_coefficients_bn_grad_wide_f32": (_I, [_FP, _VP, _VP, _FP, _VP, _I, _VP, _SZ, _VP]),
}

# include/hdrnet_amd_pyramid_io.h: the pyramid model's wire formats (the resize that reads u8 / u16, the finest level's
# slice-apply + up-add with both conversions in registers).
PYRAMID_IO_SIGNATURES = {
    "hdrnet_resize_bilinear_io": (_I, [_FP, _I, ctypes.c_float, _FP] + [_I] * 6 + [_VP]),
    "hdrnet_bilateral_slice_apply_upadd_io_ex": (_I, [_FP] * 4 + [_I, _I, _FP] + [_I] * 9 + [_I, ctypes.c_float, _I] +
                                                 [_FP, _FP, _I, _U, _VP]),
}

# include/hdrnet_amd_pixel_formats.h: uint8 / uint16 frames in BGR, RGBA and BGRA order through the low-res gather and the
# fused wire-format forwards (the hdrnet_lowres_input / ..._io_ex / ..._io_curves_prepared arguments plus the formats).
PIXEL_FORMATS = {"rgb": 0, "bgr": 1, "rgba": 2, "bgra": 3}  # HDRNET_PX_*
PIXEL_FORMAT_CHANNELS = {"rgb": 3, "bgr": 3, "rgba": 4, "bgra": 4}
PIXEL_FORMAT_SIGNATURES = {
    "hdrnet_lowres_input_px": (_I, [_FP, _I, ctypes.c_float] + [_I] * 3 + [_FP, _I, _I, _VP]),
    "hdrnet_bilateral_slice_apply_io_px": (_I, [_FP] * 4 + [_I] * 10 + [ctypes.c_float, _I] + [_FP] * 2 + [_I, _FP, _U, _I, _I,
                                                                                                      _VP]),
    "hdrnet_bilateral_slice_apply_io_curves_px": (_I, [_FP] * 3 + [_I] * 10 + [ctypes.c_float, _I] + [_FP] * 4 +
                                                  [_I, _VP, _FP, _I, _I, _VP]),
}

# include/hdrnet_amd_yuv.h: semi-planar YUV 4:2:0 surfaces (NV12, P010 / P016) through the low-res gather and the fused
# wire-format forwards, NV12 out.  A surface travels as (y, uv, sample_dtype, pitch_y, pitch_uv, image_stride_y,
# image_stride_uv); B, H, W and the 12 constants follow it.
_LL = ctypes.c_longlong
_SURFACE = [_FP, _FP, _I, _I, _I, _LL, _LL]
YUV_OUT = {"rgb_f32": 0, "rgb_u8": 1, "nv12": 2}  # HDRNET_YUV_OUT_*
_YUV_OUTPUT = [_I, _FP, _FP, _I, _I, _LL, _LL, _FP]  # output_kind, out, out_uv, pitches, image strides, from_rgb
YUV_SIGNATURES = {
    "hdrnet_yuv_to_rgb_f32": (_I, _SURFACE + [_I] * 3 + [_FP, _FP, _VP]),
    "hdrnet_lowres_input_yuv": (_I, _SURFACE + [_I] * 3 + [_FP, _FP, _I, _VP]),
    "hdrnet_bilateral_slice_apply_io_yuv": (_I, [_FP, _FP] + _SURFACE + [_I] * 3 + [_FP] + [_I] * 6 + [_FP, _FP, _I, _FP, _U] +
                                            _YUV_OUTPUT + [_VP]),
    "hdrnet_bilateral_slice_apply_io_curves_yuv": (_I, [_FP] + _SURFACE + [_I] * 3 + [_FP] + [_I] * 6 + [_FP] * 4 +
                                                   [_I, _VP, _FP] + _YUV_OUTPUT + [_VP]),
}

# include/hdrnet_amd_u16_out.h: the same fused forwards with a 16-bit output -- a uint16 frame in the input's pixel format
# (`output_dtype` replaced by `output_white_level`), a P010 / P016 surface (the output surface, from_rgb and `out_bits` in
# place of the `output_kind` ... `from_rgb` tail).
_P016_OUTPUT = [_FP, _FP, _I, _I, _LL, _LL, _FP, _I]  # out_y, out_uv, pitches, image strides, from_rgb, out_bits
U16_OUT_SIGNATURES = {
    "hdrnet_bilateral_slice_apply_io_px_u16": (_I, [_FP] * 4 + [_I] * 10 + [ctypes.c_float, ctypes.c_float] + [_FP] * 2 +
                                               [_I, _FP, _U, _I, _I, _VP]),
    "hdrnet_bilateral_slice_apply_io_curves_px_u16": (_I, [_FP] * 3 + [_I] * 10 + [ctypes.c_float, ctypes.c_float] + [_FP] * 4 +
                                                      [_I, _VP, _FP, _I, _I, _VP]),
    "hdrnet_bilateral_slice_apply_io_yuv_p016": (_I, [_FP, _FP] + _SURFACE + [_I] * 3 + [_FP] + [_I] * 6 +
                                                 [_FP, _FP, _I, _FP, _U] + _P016_OUTPUT + [_VP]),
    "hdrnet_bilateral_slice_apply_io_curves_yuv_p016": (_I, [_FP] + _SURFACE + [_I] * 3 + [_FP] + [_I] * 6 + [_FP] * 4 +
                                                        [_I, _VP, _FP] + _P016_OUTPUT + [_VP]),
}

# include/hdrnet_amd_yuv_planar.h: planar YUV 4:2:0 surfaces (I420, yuv420p10le / yuv420p16le) through the same paths, a
# planar surface out.  A surface travels as (y, u, v, sample_dtype, three pitches, three image strides); the output as
# (output_kind, out, out_u, out_v, three pitches, three image strides, from_rgb, out_bits).
_PLANAR_SURFACE = [_FP, _FP, _FP, _I, _I, _I, _I, _LL, _LL, _LL]
YUV_PLANAR_OUT = {"rgb_f32": 0, "rgb_u8": 1, "planar": 2}  # HDRNET_YUV_PLANAR_OUT_*
_PLANAR_OUTPUT = [_I, _FP, _FP, _FP, _I, _I, _I, _LL, _LL, _LL, _FP, _I]
YUV_PLANAR_SIGNATURES = {
    "hdrnet_yuv_planar_to_rgb_f32": (_I, _PLANAR_SURFACE + [_I] * 3 + [_FP, _FP, _VP]),
    "hdrnet_lowres_input_yuv_planar": (_I, _PLANAR_SURFACE + [_I] * 3 + [_FP, _FP, _I, _VP]),
    "hdrnet_bilateral_slice_apply_io_yuv_planar": (_I, [_FP, _FP] + _PLANAR_SURFACE + [_I] * 3 + [_FP] + [_I] * 6 +
                                                   [_FP, _FP, _I, _FP, _U] + _PLANAR_OUTPUT + [_VP]),
    "hdrnet_bilateral_slice_apply_io_curves_yuv_planar": (_I, [_FP] + _PLANAR_SURFACE + [_I] * 3 + [_FP] + [_I] * 6 +
                                                          [_FP] * 4 + [_I, _VP, _FP] + _PLANAR_OUTPUT + [_VP]),
}

# include/hdrnet_amd_yuv_chroma.h: the entry points of the three tables above with a chroma layout -- `chroma` follows the
# surface, and every surface output carries `out_bits`.
CHROMA = {"420": 0, "422": 1, "444": 2}  # HDRNET_CHROMA_*
CHROMA_OUT = {"rgb_f32": 0, "rgb_u8": 1, "surface_u8": 2, "surface_u16": 3}  # HDRNET_CHROMA_OUT_*
YUV_CHROMA_SIGNATURES = {
    "hdrnet_yuv_chroma_to_rgb_f32": (_I, _SURFACE + [_I] * 4 + [_FP, _FP, _VP]),
    "hdrnet_lowres_input_yuv_chroma": (_I, _SURFACE + [_I] * 4 + [_FP, _FP, _I, _VP]),
    "hdrnet_bilateral_slice_apply_io_yuv_chroma": (_I, [_FP, _FP] + _SURFACE + [_I] * 4 + [_FP] + [_I] * 6 +
                                                   [_FP, _FP, _I, _FP, _U] + _YUV_OUTPUT + [_I, _VP]),
    "hdrnet_bilateral_slice_apply_io_curves_yuv_chroma": (_I, [_FP] + _SURFACE + [_I] * 4 + [_FP] + [_I] * 6 + [_FP] * 4 +
                                                          [_I, _VP, _FP] + _YUV_OUTPUT + [_I, _VP]),
    "hdrnet_yuv_planar_chroma_to_rgb_f32": (_I, _PLANAR_SURFACE + [_I] * 4 + [_FP, _FP, _VP]),
    "hdrnet_lowres_input_yuv_planar_chroma": (_I, _PLANAR_SURFACE + [_I] * 4 + [_FP, _FP, _I, _VP]),
    "hdrnet_bilateral_slice_apply_io_yuv_planar_chroma": (_I, [_FP, _FP] + _PLANAR_SURFACE + [_I] * 4 + [_FP] + [_I] * 6 +
                                                          [_FP, _FP, _I, _FP, _U] + _PLANAR_OUTPUT + [_VP]),
    "hdrnet_bilateral_slice_apply_io_curves_yuv_planar_chroma": (_I, [_FP] + _PLANAR_SURFACE + [_I] * 4 + [_FP] + [_I] * 6 +
                                                                 [_FP] * 4 + [_I, _VP, _FP] + _PLANAR_OUTPUT + [_VP]),
}

# include/hdrnet_amd_yuv_packed.h: packed 4:2:2 surfaces (YUY2 / UYVY / YVYU, Y210 / Y216) -- the semi-planar 4:2:2 entry points
# above on one plane.  A surface travels as (surface, sample_dtype, pitch, image_stride, order); the output as (output_kind,
# out, out_pitch, out_image_stride, from_rgb, out_bits).
PACKED_ORDER = {"yuy2": 0, "yuyv": 0, "uyvy": 1, "yvyu": 2, "y210": 0, "y216": 0}  # HDRNET_PACKED_*
_PACKED_SURFACE = [_FP, _I, _I, _LL, _I]
_PACKED_OUTPUT = [_I, _FP, _I, _LL, _FP, _I]
YUV_PACKED_SIGNATURES = {
    "hdrnet_yuv_packed_to_rgb_f32": (_I, _PACKED_SURFACE + [_I] * 3 + [_FP, _FP, _VP]),
    "hdrnet_lowres_input_yuv_packed": (_I, _PACKED_SURFACE + [_I] * 3 + [_FP, _FP, _I, _VP]),
    "hdrnet_bilateral_slice_apply_io_yuv_packed": (_I, [_FP, _FP] + _PACKED_SURFACE + [_I] * 3 + [_FP] + [_I] * 6 +
                                                   [_FP, _FP, _I, _FP, _U] + _PACKED_OUTPUT + [_VP]),
    "hdrnet_bilateral_slice_apply_io_curves_yuv_packed": (_I, [_FP] + _PACKED_SURFACE + [_I] * 3 + [_FP] + [_I] * 6 + [_FP] * 4 +
                                                          [_I, _VP, _FP] + _PACKED_OUTPUT + [_VP]),
}

# include/hdrnet_amd_pyramid_yuv.h: the pyramid model on YUV 4:2:0 surfaces -- the resize that reads a surface (the
# surface, B, H, W, to_rgb, out, Hout, Wout) and the finest level's slice-apply + up-add: the single-level surface entry
# points with (coarse, Hc, Wc) after to_rgb and without guide_out.
_COARSE = [_FP, _I, _I]
PYRAMID_YUV_SIGNATURES = {
    "hdrnet_resize_bilinear_yuv": (_I, _SURFACE + [_I] * 3 + [_FP, _FP, _I, _I, _VP]),
    "hdrnet_resize_bilinear_yuv_planar": (_I, _PLANAR_SURFACE + [_I] * 3 + [_FP, _FP, _I, _I, _VP]),
    "hdrnet_bilateral_slice_apply_upadd_io_yuv": (_I, [_FP, _FP] + _SURFACE + [_I] * 3 + [_FP] + _COARSE + [_I] * 6 +
                                                  [_FP, _FP, _I, _U] + _YUV_OUTPUT + [_VP]),
    "hdrnet_bilateral_slice_apply_upadd_io_yuv_p016": (_I, [_FP, _FP] + _SURFACE + [_I] * 3 + [_FP] + _COARSE + [_I] * 6 +
                                                       [_FP, _FP, _I, _U] + _P016_OUTPUT + [_VP]),
    "hdrnet_bilateral_slice_apply_upadd_io_yuv_planar": (_I, [_FP, _FP] + _PLANAR_SURFACE + [_I] * 3 + [_FP] + _COARSE +
                                                         [_I] * 6 + [_FP, _FP, _I, _U] + _PLANAR_OUTPUT + [_VP]),
}

_lock = threading.Lock()
_lib: Optional[ctypes.CDLL] = None
_tools_lib: Optional[ctypes.CDLL] = None

# Symbols only the tools build exports (include/hdrnet_amd_tools.h).
TOOLS_SIGNATURES = {
    "hdrnet_tools_set_trace": (None, [_VP]),
    "hdrnet_tools_set_knob": (None, [ctypes.c_int, ctypes.c_int]),
}


def lib_path() -> str:
    from . import build as _build

    return _build.LIB_PATH


def _open(tools: bool) -> ctypes.CDLL:
    # torch must be imported first so that its bundled libamdhip64.so.7 is the
    # HIP runtime both sides share (same SONAME => the loader reuses it).
    import torch  # noqa: F401

    from . import build as _build

    target = _build.TOOLS_LIB_PATH if tools else _build.LIB_PATH
    try:
        path = _build.build(tools=tools)
    except Exception as e:  # noqa: BLE001
        # A library that is older than its sources is NOT silently acceptable: tests passing on a
        # stale binary is exactly what the "which .so was loaded" check cannot see.  Refuse unless
        # the caller explicitly allows it (a host without hipcc that was handed a prebuilt tree).
        if os.path.exists(target) and os.environ.get("HDRNET_AMD_ALLOW_STALE_LIB") == "1":
            import warnings

            warnings.warn(f"hdrnet_amd: rebuilding {os.path.basename(target)} FAILED ({e}); loading the "
                          "existing, possibly STALE library because HDRNET_AMD_ALLOW_STALE_LIB=1",
                          RuntimeWarning, stacklevel=3)
            path = target
        else:
            hint = (" (an older library exists; set HDRNET_AMD_ALLOW_STALE_LIB=1 to load it anyway)"
                    if os.path.exists(target) else "")
            raise HdrnetLibraryError(
                f"cannot build {os.path.basename(target)} (hipcc for gfx950 required): {e}{hint}") from e
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise HdrnetLibraryError(f"cannot load {path}: {e}") from e
    table = dict(SIGNATURES)
    table.update(TRAIN_SIGNATURES)
    table.update(COEFF_BN_SIGNATURES)
    table.update(COEFF_WIDE_SIGNATURES)
    table.update(PYRAMID_IO_SIGNATURES)
    table.update(PIXEL_FORMAT_SIGNATURES)
    table.update(YUV_SIGNATURES)
    table.update(U16_OUT_SIGNATURES)
    table.update(YUV_PLANAR_SIGNATURES)
    table.update(YUV_CHROMA_SIGNATURES)
    table.update(YUV_PACKED_SIGNATURES)
    table.update(PYRAMID_YUV_SIGNATURES)
    if tools:
        table.update(TOOLS_SIGNATURES)
    for name, (res, args) in table.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HdrnetLibraryError(f"{path} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    return lib


def load() -> ctypes.CDLL:
    """Load the product library (building first if the in-tree library is missing or stale)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            _lib = _open(tools=False)
    return _lib


def load_tools() -> ctypes.CDLL:
    """Load the TOOLS build (benchmark variants, memory skeletons, timeline trace); used by
    tools/*.py and the variant tests only -- never by the ops."""
    global _tools_lib
    if _tools_lib is not None:
        return _tools_lib
    with _lock:
        if _tools_lib is None:
            _tools_lib = _open(tools=True)
    return _tools_lib


def pixel_format(name, channels: int, dtype_is_float: bool, what: str, argument: str = "pixel_format") -> str:
    """The pixel format of a frame with ``channels`` samples per pixel, checked against the rules of
    include/hdrnet_amd_pixel_formats.h -- on the host, before anything touches the device.  ``None`` is ``"rgb"`` for three
    channels; four channels need an explicit ``"rgba"`` / ``"bgra"`` (no guessing)."""
    if name is None:
        if channels == 4:
            raise ValueError(f"{what}: a 4-channel frame needs {argument}='rgba' or {argument}='bgra' (the order of R and B "
                             "is not guessed)")
        name = "rgb"
    if not isinstance(name, str) or name not in PIXEL_FORMATS:
        raise ValueError(f"{what}: unknown {argument} {name!r} (takes {', '.join(repr(k) for k in PIXEL_FORMATS)})")
    if PIXEL_FORMAT_CHANNELS[name] != channels:
        raise ValueError(f"{what}: {argument}={name!r} is a {PIXEL_FORMAT_CHANNELS[name]}-channel format, the frame has "
                         f"{channels} channels")
    if dtype_is_float and name != "rgb":
        raise ValueError(f"{what}: float32 frames take {argument}='rgb' only ({argument}={name!r} is for uint8 / uint16 "
                         "frames)")
    return name


def enable_kernel_names(on: bool = True) -> None:
    """Switch the hdrnet_last_kernel() bookkeeping on / off (off by default)."""
    load().hdrnet_enable_kernel_names(1 if on else 0)


def last_error() -> str:
    return load().hdrnet_last_error().decode()


def last_kernel() -> str:
    return load().hdrnet_last_kernel().decode()


def check(rc: int, what: str) -> None:
    if rc == HDRNET_OK:
        return
    msg = f"{what}: {last_error()}"
    if rc == HDRNET_INVALID_ARGUMENT:
        raise HdrnetInvalidArgument(msg)
    raise HdrnetRuntimeError(msg)
