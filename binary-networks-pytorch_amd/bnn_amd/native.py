"""ctypes binding of the C-ABI declared in ``include/bnn_hip.h`` (``libbnn_hip.so``).

The library is built in-tree by ``csrc/Makefile`` / ``__graft_entry__.build()`` into
``bnn_amd/_lib/``.  ``require()`` raises ``RuntimeError`` if it cannot be loaded: the HIP path
must never silently turn into something else on a GPU box.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_BASENAME = "libbnn_hip.so"
DEFAULT_LIB_PATH = os.path.join(_HERE, "_lib", LIB_BASENAME)

OCB = 32
FLAG_FORCE_GENERIC = 1
FLAG_WEIGHT_ZEROS = 2
FLAG_WEIGHTS_SGPR = 4
FLAG_ACT_NONNEG = 32
FLAG_THROUGHPUT = 64
FLAG_OUT_F16 = 256                      # bnn_hip_bconv2d_direct only: the kernel rounds and stores 16-bit floats
FLAG_OUT_BF16 = 512
HBLOCK_CHANNEL_LANES = 128
STEM_EXACT_FP32 = 1
STEM_FP16 = 4
ABI_VERSION = 16
STEM_S2_TILE = (4, 16)                  # BNN_HIP_STEM_S2_TILE_H / _W: output pixels per workgroup of the ImageNet stem kernels
STEM_S2X2_MAX_GROUP_CHANNELS = 32       # BNN_HIP_STEM_S2X2_MAX_GROUP_CHANNELS
GCONV3X3S2_MAX_GROUP_CHANNELS = 40      # BNN_HIP_GCONV3X3S2_MAX_GROUP_CHANNELS
DTYPE_F32 = 0
DTYPE_F16 = 1
DTYPE_BF16 = 2

# status codes of include/bnn_hip.h that Python code compares against (anything else just goes through check())
OK = 0
ERR_INVALID_ARG = -1
ERR_UNSUPPORTED = -2
ERR_TOO_LARGE = -4


class ConvDesc(ctypes.Structure):
    """``bnn_hip_conv_desc``"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "N", "C", "H", "W", "O", "KH", "KW", "stride_h", "stride_w", "pad_h", "pad_w",
        "dil_h", "dil_w", "flags")]


class WLayout(ctypes.Structure):
    """``bnn_hip_wlayout``"""
    _fields_ = [("cw32", ctypes.c_int32), ("cwc", ctypes.c_int32), ("nchunk", ctypes.c_int32),
                ("taps", ctypes.c_int32), ("o_pad", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("n_words", ctypes.c_int64)]


class FlyPlan(ctypes.Structure):
    """``bnn_hip_fly_plan``"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "images_per_band", "rows_per_band", "waves", "blocks_per_unit", "pack_ahead", "fine_head", "fine_tail", "producers",
        "lds_bytes", "n_bands")]


class HBlockDesc(ctypes.Structure):
    """``bnn_hip_hblock_desc``"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "N", "C_in", "H", "W", "planes", "flags", "rows_per_band", "images_per_band", "waves", "reserved")]


class HBlockLayout(ctypes.Structure):
    """``bnn_hip_hblock_layout``"""
    _fields_ = [("weight_words", ctypes.c_int64), ("w_off", ctypes.c_int64 * 3), ("const_floats", ctypes.c_int64),
                ("alpha_off", ctypes.c_int64 * 3), ("pack_a_off", ctypes.c_int64 * 2), ("pack_b_off", ctypes.c_int64 * 2),
                ("next_a_off", ctypes.c_int64), ("next_b_off", ctypes.c_int64)]


class DevInfo(ctypes.Structure):
    """``bnn_hip_devinfo``"""
    _fields_ = [("name", ctypes.c_char * 64), ("arch", ctypes.c_char * 32),
                ("compute_units", ctypes.c_int32), ("clock_khz", ctypes.c_int32),
                ("mem_clock_khz", ctypes.c_int32), ("mem_bus_bits", ctypes.c_int32),
                ("wavefront", ctypes.c_int32), ("lds_bytes_per_block", ctypes.c_int32),
                ("total_mem_bytes", ctypes.c_int64), ("l2_bytes", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class Epilogue(ctypes.Structure):
    """``bnn_hip_epilogue``"""
    _fields_ = [("alpha", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("post_scale", ctypes.c_void_p),
                ("bn_scale", ctypes.c_void_p), ("bn_shift", ctypes.c_void_p),
                ("residual", ctypes.c_void_p), ("prelu", ctypes.c_void_p),
                ("relu", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("out_f32", ctypes.c_void_p), ("out_P", ctypes.c_void_p), ("out_M", ctypes.c_void_p),
                ("pack_scale", ctypes.c_void_p), ("pack_shift", ctypes.c_void_p),
                ("out_c_offset", ctypes.c_int32), ("out_c_total", ctypes.c_int32),
                ("sign_thresholds", ctypes.c_void_p),
                # ABI 11: the block's shortcut convolution folded into this one (include/bnn_hip.h)
                ("sc_P", ctypes.c_void_p), ("sc_wbits", ctypes.c_void_p), ("sc_alpha", ctypes.c_void_p),
                ("sc_bn_scale", ctypes.c_void_p), ("sc_bn_shift", ctypes.c_void_p),
                ("sc_C", ctypes.c_int32), ("sc_in_hw", ctypes.c_int32)]


class ConvRoute(ctypes.Structure):
    """``bnn_hip_conv_route``: the kernel the launch ladder of ``csrc/bconv.hip`` picks for a convolution."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "tiled", "kh", "kw", "cwc", "nchunk", "profile", "nonneg", "weight_zeros", "multi", "pieces", "blocks_per_wave",
        "shortcut_fold", "site", "reserved")] + [("waves", ctypes.c_int64)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


# bnn_hip_conv_route.profile (BNN_HIP_ROUTE_EP_*) and .site (BNN_HIP_SITE_*), by name
ROUTE_PROFILES = {"PLAIN": 0, "RUNTIME": 1, "MID": 2, "OUT": 3, "DS": 4, "LAST": 5, "HB": 6, "HB3": 7, "MIDT": 8, "OUTP": 9}
ROUTE_SITE_NAMES = ("SINGLE_OBW", "SINGLE_SPLIT", "SINGLE_FOLD", "SINGLE", "MULTI4_SPLIT4", "MULTI4_SPLIT2_FOLD",
                    "MULTI4_SPLIT2", "MULTI4_FOLD", "MULTI4", "CHUNKS_FOLD", "CHUNKS", "WZ_SINGLE", "WZ_CHUNKS",
                    "GENERIC_WZ", "GENERIC")
ROUTE_SITES = len(ROUTE_SITE_NAMES)     # BNN_HIP_ROUTE_SITES
SITE = {n: i for i, n in enumerate(ROUTE_SITE_NAMES)}


class FconvDesc(ctypes.Structure):
    """``bnn_hip_fconv_desc``: geometry of a FactorizedConv (1 x K stride (1, s), then K x 1 stride (s, 1))."""
    _fields_ = [(n, ctypes.c_int32) for n in ("N", "C", "H", "W", "K", "stride", "flags", "reserved")]


class FconvStage(ctypes.Structure):
    """``bnn_hip_fconv_stage``: the per-channel constants behind one of its two convolutions."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("alpha", "bias", "post_scale", "prelu")]


class F32View(ctypes.Structure):
    """``bnn_hip_f32_view``: channels ``[c_offset, c_offset + C)`` of a contiguous fp32 ``[N, c_total, H, W]`` tensor."""
    _fields_ = [("p", ctypes.c_void_p), ("c_offset", ctypes.c_int32), ("c_total", ctypes.c_int32)]


EPI_RES_AFTER_ACT = 1
EPI_PACK_BEFORE_RES = 2
EPI_PACK_RELU = 4


class NativeError(RuntimeError):
    pass


_lock = threading.Lock()
_lib: Optional[ctypes.CDLL] = None
_load_error: Optional[str] = None

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t
_dp = ctypes.POINTER(ctypes.c_double)
_conv_p = ctypes.POINTER(ConvDesc)
_hblock_p = ctypes.POINTER(HBlockDesc)
_wlayout_p = ctypes.POINTER(WLayout)
_view_p = ctypes.POINTER(F32View)
_fconv_p = ctypes.POINTER(FconvDesc)
_fstage_p = ctypes.POINTER(FconvStage)

# Every symbol include/bnn_hip.h declares: name -> (restype, argtypes).  load() resolves and declares from this table,
# so a symbol cannot be exported without its prototype (an undeclared one would pass 64-bit pointers as C ints).
_PROTOTYPES = {
    "bnn_hip_abi_version": (_i, []),
    "bnn_hip_status_string": (ctypes.c_char_p, [_i]),
    "bnn_hip_launch_count": (ctypes.c_uint64, []),
    "bnn_hip_device_info": (_i, [_i, ctypes.POINTER(DevInfo)]),
    "bnn_hip_act_words": (_i, [_i]),
    "bnn_hip_weight_layout": (_i, [_i, _i, _i, _i, _wlayout_p]),
    "bnn_hip_grouped_weight_layout": (_i, [_i, _i, _i, _i, _i, _wlayout_p]),
    "bnn_hip_pack_act_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "bnn_hip_pack_act_f16": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "bnn_hip_pack_act_bf16": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "bnn_hip_pack_act_ste_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "bnn_hip_bn_act_pack_ste_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bnn_hip_bn_act_pack_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "bnn_hip_bn_act_pack_multi_f32": (_i, [_view_p, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "bnn_hip_bn_act_pack_ste_s2_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bnn_hip_bn_act_pack_s2_f32": (_i, [_view_p, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "bnn_hip_stem3x3_bn_relu_pack_f32": (_i, [_vp] * 6 + [_i] * 5 + [_vp] * 4),
    "bnn_hip_stem_s2x2_f32": (_i, [_vp] * 7 + [_i] * 7 + [_vp] * 2),
    "bnn_hip_gconv3x3s2_bn_pack_f32": (_i, [_vp] * 6 + [_i] * 8 + [_vp] * 4),
    "bnn_hip_avgpool_pack_f32": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "bnn_hip_avgpool2_bn_pack2_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "bnn_hip_orpool_packed": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "bnn_hip_bn_relu_maxpool_pack_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "bnn_hip_stem7x7_bn_relu_pool_pack_f32": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "bnn_hip_stem7x7_bn_relu_pool_pack_affine_f32": (_i, [_vp] * 6 + [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "bnn_hip_stem7x7_conv_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "bnn_hip_stem7x7_wgrad_workspace_bytes": (_sz, [_i, _i, _i]),
    "bnn_hip_stem7x7_wgrad_f32": (_i, [_vp, _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "bnn_hip_avgpool2x2_backward_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "bnn_hip_avgpool_fc_f32": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "bnn_hip_avgpool_fc_workspace_bytes": (_sz, [_i, _i]),
    "bnn_hip_avgpool_fc_ws_f32": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "bnn_hip_pack_weight_f32": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "bnn_hip_pack_weight_grouped_f32": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "bnn_hip_sign_thresholds_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "bnn_hip_bconv2d": (_i, [_conv_p] + [_vp] * 9),
    "bnn_hip_bconv2d_grouped": (_i, [_conv_p, _i] + [_vp] * 9),
    "bnn_hip_bconv2d_grouped_fused": (_i, [_conv_p, _i] + [_vp] * 8 + [_i] + [_vp] * 3),
    "bnn_hip_bconv2d_grouped_node": (_i, [_conv_p, _i] + [_vp] * 8 + [_i, _view_p, _view_p, _vp, _i, _i, _vp]),
    "bnn_hip_fconv_supported": (_i, [_fconv_p]),
    "bnn_hip_fconv_fused": (_i, [_fconv_p, _vp, _vp, _vp, _vp, _fstage_p, _vp, _vp, _fstage_p, _vp, _vp, _i, _vp, _vp, _vp]),
    "bnn_hip_bconv2d_fused": (_i, [_conv_p] + [_vp] * 4 + [ctypes.POINTER(Epilogue), _vp]),
    "bnn_hip_shortcut_fold_supported": (_i, [_conv_p, _i]),
    "bnn_hip_weight_i8_bytes": (_sz, [_i, _i, _i, _i]),
    "bnn_hip_pack_weight_i8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "bnn_hip_bconv2d_mfma_supported": (_i, [_conv_p, ctypes.POINTER(Epilogue)]),
    "bnn_hip_bconv2d_mfma_fused": (_i, [_conv_p, _vp, _vp, _vp, ctypes.POINTER(Epilogue), _vp]),
    "bnn_hip_shortcut_weight_i8_bytes": (_sz, [_i, _i]),
    "bnn_hip_pack_shortcut_weight_i8": (_i, [_vp, _i, _i, _vp, _vp]),
    "bnn_hip_bconv2d_mfma_fold_supported": (_i, [_conv_p, ctypes.POINTER(Epilogue)]),
    "bnn_hip_bconv2d_mfma_fold_fused": (_i, [_conv_p, _vp, _vp, _vp, _vp, ctypes.POINTER(Epilogue), _vp]),
    "bnn_hip_weight_f4_bytes": (_sz, [_i, _i, _i, _i]),
    "bnn_hip_pack_weight_f4": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "bnn_hip_bconv2d_mfma4_supported": (_i, [_conv_p, ctypes.POINTER(Epilogue)]),
    "bnn_hip_bconv2d_mfma4_fused": (_i, [_conv_p, _vp, _vp, _vp, ctypes.POINTER(Epilogue), _vp]),
    "bnn_hip_bconv2d_mfma4_fold_supported": (_i, [_conv_p, ctypes.POINTER(Epilogue)]),
    "bnn_hip_bconv2d_mfma4_fold_fused": (_i, [_conv_p, _vp, _vp, _vp, _vp, ctypes.POINTER(Epilogue), _vp]),
    "bnn_hip_weight1x1_f4_bytes": (_sz, [_i, _i]),
    "bnn_hip_pack_weight1x1_f4": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "bnn_hip_bconv1x1_mfma4_supported": (_i, [_conv_p, ctypes.POINTER(Epilogue)]),
    "bnn_hip_bconv1x1_mfma4_fused": (_i, [_conv_p, _vp, _vp, _vp, ctypes.POINTER(Epilogue), _vp]),
    "bnn_hip_bconv2d_route": (_i, [_conv_p, ctypes.POINTER(Epilogue), ctypes.POINTER(ConvRoute)]),
    "bnn_hip_bconv2d_dot_route": (_i, [_conv_p, ctypes.POINTER(ConvRoute)]),
    "bnn_hip_bconv2d_dot": (_i, [_conv_p] + [_vp] * 6),
    "bnn_hip_blinear": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "bnn_hip_blinear_direct": (_i, [_i, _i, _i, _vp, _i, _vp, _vp, _i] + [_vp] * 7 + [_i, _vp]),
    "bnn_hip_blinear_grad_input_f32": (_i, [_vp] * 6 + [_i, _i, _i, _vp]),
    "bnn_hip_blinear_grad_weight_splits": (_i, [_i, _i, _i]),
    "bnn_hip_blinear_grad_weight_f32": (_i, [_vp] * 4 + [_i, _i, _i, _i, _vp]),
    "bnn_hip_conv_workspace_bytes": (_sz, [_conv_p]),
    "bnn_hip_bconv2d_f32": (_i, [_conv_p] + [_vp] * 9),
    "bnn_hip_bconv2d_direct_plan": (_i, [_conv_p, ctypes.POINTER(FlyPlan)]),
    "bnn_hip_bconv2d_direct": (_i, [_conv_p, _vp, _i] + [_vp] * 6 + [ctypes.POINTER(FlyPlan), _vp]),
    "bnn_hip_grad_weight_pack_bytes": (_sz, [_i, _i, _i]),
    "bnn_hip_grad_pack_weight_f32": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp]),
    "bnn_hip_xnor_grad_pack_weight_f32": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "bnn_hip_sconv2d_weight_pack_bytes": (_sz, [_i, _i, _i]),
    "bnn_hip_sconv2d_pack_weight_f32": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "bnn_hip_sconv2d_f32": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "bnn_hip_slinear_f32": (_i, [_i, _i, _i] + [_vp] * 9),
    "bnn_hip_ste_mask_f32": (_i, [_vp, _vp, _i, _i, _vp]),
    "bnn_hip_bconv_grad_input_f32": (_i, [_vp] * 5 + [_i] * 7 + [_vp]),
    "bnn_hip_bconv_grad_input_packed_f32": (_i, [_vp] * 5 + [_i] * 7 + [_vp]),
    "bnn_hip_bconv_grad_weight_splits": (_i, [_i, _i, _i, _i]),
    "bnn_hip_bconv_grad_weight_f32": (_i, [_vp] * 3 + [_i] * 8 + [_vp]),
    "bnn_hip_bconv_grad_weight_packed_f32": (_i, [_vp] * 4 + [_i] * 8 + [_vp]),
    "bnn_hip_bconv_grouped_grad_supported": (_i, [_conv_p, _i]),
    "bnn_hip_bconv_grouped_grad_weight_splits": (_i, [_conv_p, _i]),
    "bnn_hip_bconv_grouped_grad_input_f32": (_i, [_conv_p, _i] + [_vp] * 5),
    "bnn_hip_bconv_grouped_grad_weight_f32": (_i, [_conv_p, _i] + [_vp] * 4 + [_i, _vp]),
    "bnn_hip_xnor_weight_forward_f32": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "bnn_hip_xnor_weight_backward_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "bnn_hip_bn_act_f32": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "bnn_hip_bn_train_workspace_bytes": (_sz, [_i, _i, _i]),
    "bnn_hip_bn_train_forward_f32": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _f, _f] + [_vp] * 7),
    "bnn_hip_bn_train_backward_f32": (_i, [_vp] * 6 + [_i, _i, _i] + [_vp] * 6),
    "bnn_hip_bn_train_backward_add_f32": (_i, [_vp] * 7 + [_i, _i, _i] + [_vp] * 5),
    "bnn_hip_bn_train_pack_ste_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _f, _f] + [_vp] * 11),
    "bnn_hip_bn_train_pack_ste_s2_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _f, _f] + [_vp] * 11),
    "bnn_hip_bn_train_backward_s2_f32": (_i, [_vp] * 6 + [_i, _i, _i, _i] + [_vp] * 5),
    "bnn_hip_prelu_shuffle_backward_workspace_bytes": (_sz, [_i, _i, _i]),
    "bnn_hip_prelu_shuffle_backward_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "bnn_hip_bn_relu_maxpool_train_forward_f32": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _f, _f] + [_vp] * 8),
    "bnn_hip_bn_relu_maxpool_train_backward_f32": (_i, [_vp] * 7 + [_i, _i, _i, _i] + [_vp] * 5),
    "bnn_hip_hblock_supported": (_i, [_hblock_p]),
    "bnn_hip_hblock_layout_of": (_i, [_i, _i, ctypes.POINTER(HBlockLayout)]),
    "bnn_hip_hblock_pack_weights": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp]),
    "bnn_hip_hblock_pack_weights_cl": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp]),
    "bnn_hip_hblock_forward": (_i, [_hblock_p] + [_vp] * 7),
    "bnn_hip_hblock_pool_supported": (_i, [_hblock_p]),
    "bnn_hip_hblock_pool_forward": (_i, [_hblock_p] + [_vp] * 9),
    "bnn_hip_hblock_shortcut_supported": (_i, [_hblock_p]),
    "bnn_hip_hblock_pack_shortcut_weights": (_i, [_i, _i, _vp, _vp, _vp]),
    "bnn_hip_hblock_shortcut_forward": (_i, [_hblock_p] + [_vp] * 10),
    "bnn_hip_probe_int_alu": (_i, [_i, _i, _dp, _dp, _vp]),
    "bnn_hip_probe_clock": (_i, [_i, _dp, _dp, _vp]),
}
EXPORTED_SYMBOLS = tuple(_PROTOTYPES)   # (tests assert the .so exports exactly these)


def lib_path() -> str:
    return os.environ.get("BNN_AMD_LIB", DEFAULT_LIB_PATH)


def load() -> Optional[ctypes.CDLL]:
    """Load the library once; returns ``None`` (and remembers why) when that fails."""
    global _lib, _load_error
    with _lock:
        if _lib is not None or _load_error is not None:
            return _lib
        path = lib_path()
        try:
            lib = ctypes.CDLL(path)
            for name, (restype, argtypes) in _PROTOTYPES.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
            if lib.bnn_hip_abi_version() != ABI_VERSION:
                raise OSError(f"ABI version mismatch: {lib.bnn_hip_abi_version()} != {ABI_VERSION}")
            _lib = lib
        except (OSError, AttributeError) as exc:  # missing file, missing libamdhip64, missing symbol
            _load_error = f"{path}: {exc}"
        return _lib


def available() -> bool:
    return load() is not None


def require() -> ctypes.CDLL:
    lib = load()
    if lib is None:
        raise NativeError(
            "bnn_amd: the HIP library could not be loaded (" + str(_load_error) + "). "
            "Build it with `make -C binary-networks-pytorch_amd/csrc` or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. The GPU path does not fall "
            "back to another implementation.")
    return lib


def check(status: int, what: str) -> None:
    if status != OK:
        msg = require().bnn_hip_status_string(status).decode()
        raise NativeError(f"bnn_amd: {what} failed: {msg} (status {status})")


def weight_layout(O: int, C: int, KH: int, KW: int) -> WLayout:
    L = WLayout()
    check(require().bnn_hip_weight_layout(O, C, KH, KW, ctypes.byref(L)), "bnn_hip_weight_layout")
    return L


def grouped_weight_layout(O: int, C: int, groups: int, KH: int, KW: int) -> WLayout:
    """Windowed block-diagonal layout of a grouped weight (``cw32`` = words per tap): include/bnn_hip.h."""
    L = WLayout()
    check(require().bnn_hip_grouped_weight_layout(O, C, groups, KH, KW, ctypes.byref(L)), "bnn_hip_grouped_weight_layout")
    return L


def device_info(device: int = 0) -> dict:
    info = DevInfo()
    check(require().bnn_hip_device_info(device, ctypes.byref(info)), "bnn_hip_device_info")
    return {f: (getattr(info, f).decode() if isinstance(getattr(info, f), bytes) else getattr(info, f))
            for f, _ in DevInfo._fields_ if f != "reserved"}


def launch_count() -> int:
    return int(require().bnn_hip_launch_count())
