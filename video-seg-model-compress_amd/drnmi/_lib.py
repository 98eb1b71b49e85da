"""ctypes binding of the C-ABI in include/drnmi.h (libdrnmi.so, built in-tree).

This is the ONLY way the product path reaches compute: there is no eager-torch or
CPU fallback.  If the library is missing or a launch fails, the call raises.
"""
from __future__ import annotations

import ctypes
import os

from .build import LIB_PATH

DRNMI_F32, DRNMI_BF16, DRNMI_U8, DRNMI_I64, DRNMI_I8, DRNMI_F32X3, DRNMI_F8 = 0, 1, 2, 3, 4, 5, 6
DRNMI_BF16_SP24 = 7
DRNMI_I8_SP24 = 8
SP24_GATHER, SP24_STRIP = 0, 1          # include/drnmi.h enum drnmi_sp24_tile
ALGO_IGEMM, ALGO_PATCH = 0, 1
# include/drnmi.h enum drnmi_tile: the ids tests and micro-benchmarks force
TILE_AUTO, TILE_DMA128, TILE_PP256, TILE_HALO, TILE_STRIP, TILE_STAG = -1, 4, 16, 17, 18, 19
TILE_S2ROW, TILE_S1X2ROW, TILE_W1, TILE_W1H = 20, 21, 22, 23
HIST_BINS = 32768        # include/drnmi.h DRNMI_HIST_BINS

_STATUS = {-1: "DRNMI_EINVAL (bad shape/stride/dtype)", -2: "DRNMI_ENOTSUP (no kernel for this config)"}


class ConvArgs(ctypes.Structure):
    """Mirror of drnmi_conv_args (include/drnmi.h)."""
    _fields_ = [
        ("x", ctypes.c_void_p),
        ("wgt", ctypes.c_void_p),
        ("scale", ctypes.c_void_p),
        ("shift", ctypes.c_void_p),
        ("res", ctypes.c_void_p),
        ("y", ctypes.c_void_p),
        ("y_sn", ctypes.c_int64), ("y_sp", ctypes.c_int64), ("y_sc", ctypes.c_int64),
        ("n", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("cin", ctypes.c_int32),
        ("ho", ctypes.c_int32), ("wo", ctypes.c_int32), ("cout", ctypes.c_int32), ("cout_pad", ctypes.c_int32),
        ("ks", ctypes.c_int32), ("stride", ctypes.c_int32), ("pad", ctypes.c_int32), ("dil", ctypes.c_int32),
        ("k", ctypes.c_int32), ("k_pad", ctypes.c_int32),
        ("relu", ctypes.c_int32),
        ("dtype", ctypes.c_int32), ("out_dtype", ctypes.c_int32),
        ("tile", ctypes.c_int32),
        ("algo", ctypes.c_int32),
        ("src_u8", ctypes.c_int32),
        ("bgr", ctypes.c_int32),
        ("mean", ctypes.c_float * 3),
        ("std", ctypes.c_float * 3),
        ("unit_mask", ctypes.c_void_p),
        ("res_scale", ctypes.c_float),
        ("out_scale", ctypes.c_float),
        ("x2", ctypes.c_void_p),
        ("cin2", ctypes.c_int32), ("h2", ctypes.c_int32), ("w2", ctypes.c_int32), ("stride2", ctypes.c_int32),
        ("ws", ctypes.c_void_p), ("ws_bytes", ctypes.c_int64),
        ("stats", ctypes.c_void_p),
        ("y_sr", ctypes.c_int64),
    ]


class WgradArgs(ctypes.Structure):
    """Mirror of drnmi_wgrad_args (include/drnmi.h)."""
    _fields_ = [
        ("dy", ctypes.c_void_p),
        ("x", ctypes.c_void_p),
        ("dw", ctypes.c_void_p),
        ("ws", ctypes.c_void_p),
        ("ws_bytes", ctypes.c_int64),
        ("n", ctypes.c_int32), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("cin", ctypes.c_int32),
        ("cin_stride", ctypes.c_int32), ("ho", ctypes.c_int32), ("wo", ctypes.c_int32),
        ("cout", ctypes.c_int32), ("dy_stride", ctypes.c_int32),
        ("ks", ctypes.c_int32), ("stride", ctypes.c_int32), ("pad", ctypes.c_int32), ("dil", ctypes.c_int32),
        ("accumulate", ctypes.c_int32),
    ]


# Every symbol include/drnmi.h declares, with its ctypes signature.
_VP, _I32, _I64, _F32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
SIGNATURES = {
    "drnmi_conv2d_bn_act": (ctypes.c_int, [ctypes.POINTER(ConvArgs), _VP]),
    "drnmi_conv_status": (ctypes.c_int, [ctypes.POINTER(ConvArgs)]),
    "drnmi_conv_tile_name": (ctypes.c_char_p, [ctypes.c_int]),
    "drnmi_conv_kernel_name": (ctypes.c_char_p, [ctypes.POINTER(ConvArgs)]),
    "drnmi_stem_layer1": (ctypes.c_int, [ctypes.POINTER(ConvArgs), ctypes.POINTER(ConvArgs), _VP]),
    "drnmi_stem_layer1_kernel_name": (ctypes.c_char_p, [ctypes.POINTER(ConvArgs), ctypes.POINTER(ConvArgs)]),
    "drnmi_conv_num_tiles": (ctypes.c_int, []),
    "drnmi_front_pack_bytes": (ctypes.c_int64, []),
    "drnmi_front_pack": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP]),
    "drnmi_front_supported": (ctypes.c_int, [_I32, _I32, _I32]),
    "drnmi_video_front_u8": (ctypes.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _VP]),
    "drnmi_frame_ingest_u8": (ctypes.c_int, [_VP, _VP, _I32, _I32, _I32, _VP, _VP, _I32, _I32, _VP]),
    "drnmi_nchw_to_nhwc": (ctypes.c_int, [_VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _VP]),
    "drnmi_nhwc_to_nchw": (ctypes.c_int, [_VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _VP]),
    "drnmi_up8_logsoftmax_argmax": (ctypes.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "drnmi_up8_logsoftmax_argmax_wide": (ctypes.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "drnmi_up8_labels_nhwc": (ctypes.c_int, [_VP, _I32, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "drnmi_up8_labels_nhwc_wide": (ctypes.c_int, [_VP, _I32, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "drnmi_up8_labels_nhwc_wide_stats": (ctypes.c_int, [_VP, _I32, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP]),
    "drnmi_up8_labels_seg2": (ctypes.c_int, [_VP, _I32, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "drnmi_conv_stag_seg": (ctypes.c_int, [ctypes.POINTER(ConvArgs), _VP, _I32, _I32, _VP, _VP]),
    "drnmi_conv_stag_seg_kernel_name": (ctypes.c_char_p, [ctypes.POINTER(ConvArgs)]),
    "drnmi_up8_labels_seg2_i8": (ctypes.c_int, [_VP, _I32, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "drnmi_up8_bilinear_logsoftmax_argmax": (ctypes.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "drnmi_resize_workspace_bytes": (ctypes.c_int64, [_I32, _I32, _I32, _I32, _I32, _I32]),
    "drnmi_resize_bilinear_u8": (ctypes.c_int, [_VP, _I32, _I32, _I32, _VP, _I32, _I32, _VP, _I64, _VP]),
    "drnmi_resize_bilinear_f32": (ctypes.c_int, [_VP, _I32, _I32, _I32, _VP, _I32, _I32, _I32, _VP, _I64, _VP]),
    "drnmi_argmax_nchw_f32": (ctypes.c_int, [_VP, _I32, _I32, _I64, _VP, _I32, _VP]),
    "drnmi_render_labels": (ctypes.c_int, [_VP, _I32, _I32, _I32, _I32, _VP, _VP, _I32, _I32, _I32, _VP, _I32, _I32,
                                           _VP]),
    "drnmi_mask_apply_f32": (ctypes.c_int, [_I32, _VP, _VP, _VP, _VP]),
    "drnmi_mask_apply_bits_f32": (ctypes.c_int, [_I32, _VP, _VP, _VP, _VP]),
    "drnmi_confusion_matrix": (ctypes.c_int, [_VP, _I32, _VP, _I32, _I64, _I32, _VP, _VP]),
    "drnmi_pack_conv_weight": (ctypes.c_int, [_VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _I32, _VP, _VP]),
    "drnmi_reduce_workspace_bytes": (ctypes.c_int64, [_I64, _I32]),
    "drnmi_bn_stats_f32": (ctypes.c_int, [_VP, _I64, _I32, _F32, _F32, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "drnmi_bn_act_f32": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _I64, _I32, _VP, _VP]),
    "drnmi_bn_act_bwd_f32": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _I64, _I32, _VP, _VP, _I32,
                                            _VP, _VP, _I32, _VP, _VP]),
    "drnmi_bn_relu_bwd_y_f32": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _I64, _I32, _VP, _VP, _VP, _I32,
                                               _VP, _VP]),
    "drnmi_channel_sum_f32": (ctypes.c_int, [_VP, _I64, _I32, _I32, _VP, _I32, _VP, _VP]),
    "drnmi_conv_wgrad_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(WgradArgs)]),
    "drnmi_conv_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(ConvArgs)]),
    "drnmi_conv_stats_rows": (ctypes.c_int64, [ctypes.POINTER(ConvArgs)]),
    "drnmi_dgrad_s2_class_planes": (ctypes.c_int, [_VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _I32,
                                                   _VP]),
    "drnmi_bn_stats_partials_f32": (ctypes.c_int, [_VP, _I64, _I64, _I32, _F32, _F32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "drnmi_conv_wgrad_f32": (ctypes.c_int, [ctypes.POINTER(WgradArgs), _VP]),
    "drnmi_conv_wgrad_f32x3": (ctypes.c_int, [ctypes.POINTER(WgradArgs), _VP]),
    "drnmi_conv_wgrad_plan": (ctypes.c_int, [ctypes.POINTER(WgradArgs), _I32, ctypes.POINTER(ctypes.c_int32),
                                             ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64),
                                             ctypes.POINTER(ctypes.c_int32)]),
    "drnmi_split3_bf16": (ctypes.c_int, [_VP, ctypes.c_int64, _VP, _VP]),
    "drnmi_fake_quant_f32": (ctypes.c_int, [_VP, _I64, _F32, _F32, _VP, _VP]),
    "drnmi_fake_quant_bwd_f32": (ctypes.c_int, [_VP, _VP, _I64, _F32, _VP, _I32, _VP]),
    "drnmi_fake_quant_rows_f32": (ctypes.c_int, [_VP, _I64, _I32, _VP, _VP, _VP]),
    "drnmi_fake_quant_rows_table_check": (ctypes.c_int, [_VP, _I32, ctypes.POINTER(ctypes.c_int64)]),
    "drnmi_fake_quant_rows_batched_f32": (ctypes.c_int, [_VP, _I32, _I64, _VP]),
    "drnmi_zero_insert_f32": (ctypes.c_int, [_VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP]),
    "drnmi_up8_lsm_bwd_f32": (ctypes.c_int, [_VP, _VP, _VP, _VP, _F32, _I32, _I32, _I32, _I32, _VP, _VP, _VP]),
    "drnmi_up8_bilinear_lsm_bwd_f32": (ctypes.c_int, [_VP, _VP, _VP, _F32, _I32, _I32, _I32, _I32, _VP, _VP, _VP]),
    "drnmi_ce_workspace_bytes": (ctypes.c_int64, []),
    "drnmi_ce_loss_f32": (ctypes.c_int, [_VP, _VP, _I32, _I32, _I64, _I64, _VP, _VP, _VP, _VP]),
    "drnmi_ce_loss_bwd_f32": (ctypes.c_int, [_VP, _VP, _I32, _I32, _I64, _I64, _VP, _VP, _VP, _VP]),
    "drnmi_distill_workspace_bytes": (ctypes.c_int64, []),
    "drnmi_distill_loss_f32": (ctypes.c_int, [_VP, _VP, _VP, _I32, _I32, _I64, _I64, _F32, _F32, _F32, _I32, _VP, _VP,
                                              _VP, _VP]),
    "drnmi_distill_loss_bwd_f32": (ctypes.c_int, [_VP, _VP, _VP, _I32, _I32, _I64, _I64, _F32, _F32, _F32, _I32, _VP,
                                                  _VP, _VP, _VP]),
    "drnmi_sgd_step_f32": (ctypes.c_int, [_I32, _VP, _VP, _VP, _VP, _VP, _VP, _F32, _F32, _F32, _F32, _I32, _VP]),
    "drnmi_weight_unit_mask": (ctypes.c_int, [_VP, _I32, _I32, _I32, _VP, _VP, _VP]),
    "drnmi_sp24_pack_bytes": (ctypes.c_int64, [_I32, _I32]),
    "drnmi_sp24_pack": (ctypes.c_int, [_VP, _I32, _I32, _VP, _VP, _VP]),
    "drnmi_sp24_mma_probe": (ctypes.c_int, [_VP, _VP, _VP, _VP, _I32, _VP]),
    "drnmi_sp24_issue_probe": (ctypes.c_int, [_I32, _I32, _I32, _VP, _VP]),
    "drnmi_sp24_pack_i8_bytes": (ctypes.c_int64, [_I32, _I32]),
    "drnmi_sp24_pack_i8": (ctypes.c_int, [_VP, _I32, _I32, _VP, _VP, _VP]),
    "drnmi_sp24_mma_probe_i8": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "drnmi_quantize_i8": (ctypes.c_int, [_VP, _I32, _VP, _I64, _F32, _VP]),
    "drnmi_quantize_f8": (ctypes.c_int, [_VP, _I32, _I64, _F32, _VP, _VP]),
    "drnmi_absmax": (ctypes.c_int, [_VP, _I32, _I64, _VP, _VP]),
    "drnmi_abs_histogram": (ctypes.c_int, [_VP, _I32, _I64, _VP, _VP]),
    "drnmi_train_ingest_u8": (ctypes.c_int, [_VP, _VP, _I32, _I32, _I32, _VP, _VP, _I32, _I32, _VP, _VP, _VP, _VP, _VP]),
    "drnmi_pixel_accuracy_f32": (ctypes.c_int, [_VP, _VP, _I32, _I32, _I64, _I64, _VP, _VP]),
    "drnmi_version": (ctypes.c_char_p, []),
    "drnmi_abi_version": (ctypes.c_int32, []),
    "drnmi_conv_args_size": (ctypes.c_int64, []),
    "drnmi_conv_wgrad_f32_workspace_bytes": (ctypes.c_int64, [ctypes.POINTER(WgradArgs)]),
    "drnmi_block64_pack_bytes": (ctypes.c_int64, []),
    "drnmi_block64_pack": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "drnmi_block64_supported": (ctypes.c_int, [_I32, _I32, _I32]),
    "drnmi_basic_block64": (ctypes.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _VP]),
    "drnmi_block16_pack_bytes": (ctypes.c_int64, []),
    "drnmi_block16_pack": (ctypes.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "drnmi_block16_supported": (ctypes.c_int, [_I32, _I32, _I32]),
    "drnmi_basic_block16": (ctypes.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _VP]),
    "drnmi_pack_table_check": (ctypes.c_int, [_VP, _I32, ctypes.POINTER(ctypes.c_int64)]),
    "drnmi_pack_conv_weights_batched": (ctypes.c_int, [_VP, _I32, _I64, _VP]),
}
WGRAD_KERNELS = ("wgrad_kernel<64, false>", "wgrad_kernel<64, true>", "wgrad_kernel<128, true>", "wgrad_x6_pre_kernel",
                 "wgrad_x6_direct_kernel")      # DRNMI_WGRAD_* of drnmi_conv_wgrad_plan
WGRAD_REDUCES = ("wgrad_reduce_kernel", "wgrad_reduce_grouped_kernel")


def wgrad_plan(args: "WgradArgs", x6: bool):
    """drnmi_conv_wgrad_plan as (kernel name, splits, pix_per_split, reduce kernel name)."""
    k, s, r = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    per = ctypes.c_int64()
    check(load().drnmi_conv_wgrad_plan(ctypes.byref(args), 1 if x6 else 0, ctypes.byref(k), ctypes.byref(s),
                                       ctypes.byref(per), ctypes.byref(r)), "wgrad plan")
    return WGRAD_KERNELS[k.value], s.value, per.value, WGRAD_REDUCES[r.value]


ABI_VERSION = 7          # include/drnmi.h DRNMI_ABI_VERSION

_lib = None


def load(path: str | None = None):
    """Load libdrnmi.so (import torch first so the process shares torch's HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("DRNMI_LIB") or LIB_PATH   # DRNMI_LIB: diagnostic builds only
    if not os.path.exists(path):
        raise RuntimeError(
            f"drnmi: HIP library not built ({path}); run __graft_entry__.build() or "
            "python video-seg-model-compress_amd/drnmi/build.py")
    import torch  # noqa: F401  (binds libamdhip64.so.7 from torch before ours)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.drnmi_abi_version() != ABI_VERSION or lib.drnmi_conv_args_size() != ctypes.sizeof(ConvArgs):
        raise RuntimeError(f"drnmi: {path} has ABI {lib.drnmi_abi_version()} / drnmi_conv_args of "
                           f"{lib.drnmi_conv_args_size()} B; this binding expects {ABI_VERSION} / "
                           f"{ctypes.sizeof(ConvArgs)} B (rebuild the library)")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = _STATUS.get(rc, f"hipError {rc}")
        raise RuntimeError(f"drnmi: {what} failed: {msg}")


def stream_ptr(device=None) -> int:
    import torch
    return torch.cuda.current_stream(device).cuda_stream
