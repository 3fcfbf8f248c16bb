"""ctypes binding of libcrowdmod_hip.so (C ABI: include/crowdmod_hip.h).

The product path has no CPU fallback: if the shared library is missing or a
call fails, an exception is raised -- nothing here (or anywhere under
crowdmod-ddpm-4d_amd/) imports the oracle.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CM_LIB_PATH") or os.path.join(_HERE, "libcrowdmod_hip.so")  # override: A/B of two builds
MAX_LEVELS = 8
ABI_VERSION = 3   # CM_ABI_VERSION of include/crowdmod_hip.h


class NativeError(RuntimeError):
    """A libcrowdmod_hip call returned non-zero (message from cm_last_error)."""


class cm_unet_config(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("num_res_blocks", C.c_int32),
        ("base_channels", C.c_int32), ("n_levels", C.c_int32),
        ("channel_mult", C.c_int32 * MAX_LEVELS), ("apply_attention", C.c_int32 * MAX_LEVELS),
        ("time_multiple", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
        ("past_len", C.c_int32), ("future_len", C.c_int32), ("max_batch", C.c_int32), ("device", C.c_int32),
    ]


class cm_dit_config(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
        ("past_len", C.c_int32), ("future_len", C.c_int32), ("patch_size", C.c_int32), ("t_patch_size", C.c_int32),
        ("hidden_size", C.c_int32), ("depth", C.c_int32), ("num_heads", C.c_int32), ("mlp_hidden", C.c_int32),
        ("time_multiple", C.c_int32), ("t_max", C.c_int32), ("max_batch", C.c_int32), ("device", C.c_int32),
    ]


class cm_dit2d_config(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
        ("past_len", C.c_int32), ("future_len", C.c_int32), ("patch_size", C.c_int32),
        ("hidden_size", C.c_int32), ("depth", C.c_int32), ("num_heads", C.c_int32), ("mlp_hidden", C.c_int32),
        ("time_multiple", C.c_int32), ("t_max", C.c_int32), ("max_batch", C.c_int32), ("device", C.c_int32),
    ]


class cm_convrnn_config(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("past_len", C.c_int32),
        ("future_len", C.c_int32), ("cell", C.c_int32),
        ("enc_hidden", C.c_int32 * 6), ("forc_hidden", C.c_int32 * 7), ("enc_kernels", C.c_int32 * 6),
        ("forc_kernels", C.c_int32 * 7), ("max_batch", C.c_int32), ("device", C.c_int32),
    ]


class cm_sample_opts(C.Structure):
    _fields_ = [
        ("sampler", C.c_int32), ("guidance", C.c_int32), ("lambda_guidance", C.c_float),
        ("ddim_sigma", C.c_float), ("ddim_divider", C.c_int32), ("first_steps", C.c_int32),
        ("seed", C.c_uint64), ("sample_id_base", C.c_int64), ("use_graph", C.c_int32), ("check_finite", C.c_int32),
        ("fm_steps", C.c_int32), ("fm_time_max_pos", C.c_int32),
    ]


SAMPLER_DDPM, SAMPLER_DDIM, SAMPLER_FM_EULER = 0, 1, 2
PRECISION_F32, PRECISION_F16, PRECISION_F32R, PRECISION_F32X = 0, 1, 2, 3
PRECISION_F16A = 4   # FM-DiT (DiT2D) handles only: f16 operands in the token Linears and in both attention products
CELL_GRU, CELL_LSTM = 0, 1
GUIDANCE_NONE, GUIDANCE_SPARSITY, GUIDANCE_MASS_PRESERVATION = 0, 1, 2
TABLES = ("beta", "alpha", "alpha_bar", "sqrt_alpha_bar", "one_by_sqrt_alpha", "sqrt_one_minus_alpha_bar")

_lib: Optional[C.CDLL] = None

# name -> (restype, argtypes); the exported symbol list of include/crowdmod_hip.h
_P = C.c_void_p
_F = C.POINTER(C.c_float)
SIGNATURES = {
    "cm_last_error": (C.c_char_p, []),
    "cm_abi_version": (C.c_int, []),
    "cm_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "cm_malloc": (C.c_int, [C.c_int, C.POINTER(_P), C.c_size_t]),
    "cm_free": (C.c_int, [C.c_int, _P]),
    "cm_memcpy_h2d": (C.c_int, [C.c_int, _P, _P, C.c_size_t]),
    "cm_memcpy_d2h": (C.c_int, [C.c_int, _P, _P, C.c_size_t]),
    "cm_memcpy_d2d": (C.c_int, [C.c_int, _P, _P, C.c_size_t]),
    "cm_device_synchronize": (C.c_int, [C.c_int]),
    "cm_model_create": (C.c_int, [C.POINTER(cm_unet_config), C.POINTER(_P)]),
    "cm_model_create_dit": (C.c_int, [C.POINTER(cm_dit_config), C.POINTER(_P)]),
    "cm_model_create_dit2d": (C.c_int, [C.POINTER(cm_dit2d_config), C.POINTER(_P)]),
    "cm_model_destroy": (C.c_int, [_P]),
    "cm_model_num_params": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "cm_model_param_info": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "cm_model_set_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "cm_model_get_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "cm_model_set_precision": (C.c_int, [_P, C.c_int32]),
    "cm_model_finalize": (C.c_int, [_P]),
    "cm_unet_forward": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, _P]),
    "cm_unet_forward_host": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32]),
    "cm_model_dropout_width": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "cm_unet_forward_train": (C.c_int, [_P, _P, _P, _P, _P, C.c_float, C.c_uint64, C.c_int64, _P, C.c_int32, _P]),
    "cm_mse_loss": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_float), _P]),
    "cm_debug_activation": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, C.POINTER(C.c_int64)]),
    # test hook: (FM-DiT handle, host qkv [B][S][3E], host out [B][S][E], B): one launch of the plan's full-attention kernel
    "cm_debug_dit_attn": (C.c_int, [_P, _P, _P, C.c_int32]),
    "cm_schedule_create": (C.c_int, [C.c_int32, C.c_float, C.c_float, C.c_float, C.c_int32, C.POINTER(_P)]),
    "cm_schedule_destroy": (C.c_int, [_P]),
    "cm_schedule_table": (C.c_int, [_P, C.c_int32, _P, C.c_int32]),
    "cm_q_sample": (C.c_int, [_P, _P, _P, _P, _P, C.c_int32, C.c_int64, _P]),
    "cm_ddpm_step": (C.c_int, [_P, _P, _P, C.c_int32, _P, C.c_uint64, C.c_int64, C.c_int32, C.c_int64, _P]),
    "cm_sample_loop": (C.c_int, [_P, _P, _P, _P, _P, C.POINTER(cm_sample_opts), _P, _P, C.c_int32, _P]),
    "cm_sample_loop_host": (C.c_int, [_P, _P, _P, _P, _P, C.POINTER(cm_sample_opts), _P, _P, C.c_int32]),
    "cm_sample_num_steps": (C.c_int, [_P, C.POINTER(cm_sample_opts), C.POINTER(C.c_int32)]),
    "cm_profile_enable": (C.c_int, [_P, C.c_int32]),
    "cm_profile_read": (C.c_int, [_P, _F, C.POINTER(C.c_int64)]),
    "cm_profile_read_union": (C.c_int, [_P, _F]),
    "cm_profile_report": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "cm_model_cost": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "cm_model_class_flops": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double)]),
    "cm_model_exec_flops": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double)]),
    "cm_train_exec_flops": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "cm_model_issue_flops": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "cm_frame_metrics": (C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "cm_ssim_frames": (C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "cm_energy": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, _P, _P]),
    "cm_motion_feature_vectors": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_double, _P, _P]),
    "cm_motion_feature_tables": (C.c_int, [C.c_int32, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_double, _P]),
    "cm_mass_preservation_grad": (C.c_int, [C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_float, C.c_float, C.c_float, _P, _P]),
    "cm_debug_conv_flags": (C.c_int, [C.c_int32]),
    "cm_debug_conv_count": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "cm_debug_conv_info": (C.c_int, [_P, C.c_int32, C.c_char_p, C.c_int64]),
    "cm_debug_bwd_plan": (C.c_int, [_P, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]),
    "cm_debug_conv_io": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32]),
    "cm_debug_conv_stats": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "cm_debug_wino_form_counts": (C.c_int, [_P, C.c_int32]),
    "cm_debug_wino_ahead_count": (C.c_int, [_P, C.c_int32]),
    "cm_debug_wino_under_count": (C.c_int, [_P, C.c_int32]),
    "cm_debug_time_conv": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(C.c_float)]),
    "cm_train_init": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "cm_train_set_lr": (C.c_int, [_P, C.c_float]),
    "cm_train_set_autocast": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "cm_train_get_autocast": (C.c_int, [_P, _P, _P]),
    "cm_train_set_sample_base": (C.c_int, [_P, C.c_int64]),
    "cm_train_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_float), C.c_int32, C.c_int32, _P]),
    "cm_train_step_xt": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_float), C.c_int32, C.c_int32, _P]),
    "cm_train_get_grad": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "cm_train_sync": (C.c_int, [_P]),
    "cm_train_flat_grads": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "cm_train_apply": (C.c_int, [_P, _P]),
    "cm_train_get_opt_state": (C.c_int, [_P, C.c_char_p, C.c_int32, _P, C.c_int64]),
    "cm_train_set_opt_state": (C.c_int, [_P, C.c_char_p, C.c_int32, _P, C.c_int64]),
    "cm_train_opt_step": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int32]),
    "cm_dit_train_init": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "cm_dit_train_set_lr": (C.c_int, [_P, C.c_float]),
    "cm_dit_train_set_sample_base": (C.c_int, [_P, C.c_int64]),
    "cm_dit_train_step_xt": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_float), C.c_int32, C.c_int32, _P]),
    "cm_dit_train_flat_grads": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "cm_dit_train_apply": (C.c_int, [_P, _P]),
    "cm_dit_train_get_grad": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "cm_dit_train_get_opt_state": (C.c_int, [_P, C.c_char_p, C.c_int32, _P, C.c_int64]),
    "cm_dit_train_set_opt_state": (C.c_int, [_P, C.c_char_p, C.c_int32, _P, C.c_int64]),
    "cm_dit_train_opt_step": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int32]),
    "cm_dit_train_sync": (C.c_int, [_P]),
    "cm_dit_train_get_pred": (C.c_int, [_P, _P, C.c_int64]),
    "cm_dit4d_train_init": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "cm_dit4d_train_set_lr": (C.c_int, [_P, C.c_float]),
    "cm_dit4d_train_set_sample_base": (C.c_int, [_P, C.c_int64]),
    "cm_dit4d_train_set_autocast": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "cm_dit4d_train_get_autocast": (C.c_int, [_P, _P, _P]),
    "cm_dit4d_train_step_xt": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_float), C.c_int32, C.c_int32, _P]),
    "cm_dit4d_train_step": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_float), C.c_int32, C.c_int32, _P]),
    "cm_dit4d_train_flat_grads": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "cm_dit4d_train_apply": (C.c_int, [_P, _P]),
    "cm_dit4d_train_get_grad": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "cm_dit4d_train_get_opt_state": (C.c_int, [_P, C.c_char_p, C.c_int32, _P, C.c_int64]),
    "cm_dit4d_train_set_opt_state": (C.c_int, [_P, C.c_char_p, C.c_int32, _P, C.c_int64]),
    "cm_dit4d_train_opt_step": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int32]),
    "cm_dit4d_train_sync": (C.c_int, [_P]),
    "cm_dit4d_train_get_pred": (C.c_int, [_P, _P, C.c_int64]),
    "cm_convrnn_create": (C.c_int, [C.POINTER(cm_convrnn_config), C.POINTER(_P)]),
    "cm_convrnn_destroy": (C.c_int, [_P]),
    "cm_convrnn_num_params": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "cm_convrnn_param_info": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "cm_convrnn_set_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "cm_convrnn_get_param": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "cm_convrnn_finalize": (C.c_int, [_P]),
    # (handle, PRECISION_F32 | PRECISION_F16) before finalize: the f16 forecast plan (inference only)
    "cm_convrnn_set_precision": (C.c_int, [_P, C.c_int32]),
    # test hook: (handle, layer 0-11, part, x0, x1, hprev, u, c, y0, y1, B), host arrays in the reference's NCHW
    "cm_convrnn_debug_launch": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, _P, _P, _P, C.c_int32]),
    "cm_convrnn_forecast": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    "cm_convrnn_forecast_host": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.c_int32]),
    "cm_convrnn_debug_state": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "cm_convrnn_cost": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "cm_convrnn_train_init": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]),
    "cm_convrnn_loss": (C.c_int, [_P, _P, _P, C.c_int32, C.c_double, C.POINTER(C.c_double), C.c_int32, _P]),
    "cm_convrnn_train_step": (C.c_int, [_P, _P, _P, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_double), C.c_int32,
                                        C.c_int32, _P]),
    "cm_convrnn_train_apply": (C.c_int, [_P, _P]),
    "cm_convrnn_train_set_lr": (C.c_int, [_P, C.c_float]),
    "cm_convrnn_train_get_forecast": (C.c_int, [_P, _P, C.c_int64]),
    "cm_convrnn_train_get_grad": (C.c_int, [_P, C.c_char_p, _P, C.c_int64]),
    "cm_convrnn_train_get_opt_state": (C.c_int, [_P, C.c_char_p, C.c_int32, _P, C.c_int64]),
    "cm_convrnn_train_set_opt_state": (C.c_int, [_P, C.c_char_p, C.c_int32, _P, C.c_int64]),
    "cm_convrnn_train_opt_step": (C.c_int, [_P, C.POINTER(C.c_int32), C.c_int32]),
    "cm_convrnn_train_sync": (C.c_int, [_P]),
    "cm_convrnn_train_forward": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double)]),
    "cm_convrnn_train_backward": (C.c_int, [_P, C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(C.c_double), _P]),
    "cm_convrnn_train_flat_grads": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_int64)]),
    "cm_convrnn_loss_sums": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_double)]),
    "cm_convrnn_loss_terms_from_sums": (C.c_int, [C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double)]),
}


def _preload_hip_runtime():
    """Make this process use ONE HIP runtime.

    PyTorch-ROCm bundles its own libamdhip64.so (same SONAME as /opt/rocm's).  If
    our library pulled in the system copy and torch later loaded its own, two HIP
    runtimes would share the process.  Loading torch's copy first (by path, without
    importing torch) lets the dynamic loader resolve our DT_NEEDED to it too.
    """
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib() -> C.CDLL:
    """Load (once) and return the shared library; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C crowdmod-ddpm-4d_amd/csrc`). There is no CPU fallback.")
    _preload_hip_runtime()
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.cm_abi_version() != ABI_VERSION:
        raise NativeError("libcrowdmod_hip.so ABI version mismatch")
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().cm_last_error()
        raise NativeError(msg.decode("utf-8", "replace") if msg else f"libcrowdmod_hip call failed ({rc})")


# Test hooks exported outside the public header (SIGNATURES mirrors the header): bound on first use.
_HOOKS = {
    "cm_debug_attn_block": (C.c_int, [_P, C.c_int32, C.c_int32, _P, _P, _P, _P, C.c_int32]),
    "cm_debug_attn_pack": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_float)]),
    "cm_debug_attn_sample_ok": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "cm_debug_conv_info_ext": (C.c_int, [_P, C.c_int32, _P, C.c_int64]),
    "cm_debug_conv_tail": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, C.c_int32]),
    "cm_debug_attn_core": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
}


def hook(name: str):
    fn = getattr(lib(), name)
    fn.restype, fn.argtypes = _HOOKS[name]
    return fn


def debug_attn_block(handle, index: int, mode: int, x: np.ndarray):
    """One fused attention block (op `index`) of a UNet handle on the host array x [B, S, E] (channels-last).
    mode 0: the (head, sample) launch and the head sum; mode 1: the whole-sample kernel (NativeError where the
    handle's plan does not take it).  Returns (out [B, S, E], slot partials [B, ns, E, 2], slot counts [B, ns])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, S, E = x.shape
    ns = (S + 31) // 32
    out = np.empty_like(x)
    part = np.empty((B, ns, E, 2), np.float32)
    cnt = np.empty((B, ns), np.float32)
    check(hook("cm_debug_attn_block")(handle, index, mode, x.ctypes.data, out.ctypes.data, part.ctypes.data,
                                      cnt.ctypes.data, B))
    return out, part, cnt


def debug_conv_tail(handle, index: int, x0: np.ndarray, x1, t0: np.ndarray, t1, out_shape):
    """Conv op `index` of a UNet handle as ONE raw launch (no GroupNorm / SiLU on load, no time row) that keeps its residual or its
    fused 1x1x1 skip conv, on host data: x0 / x1 the sources [B, Zs, Ys, Xs, C0 / C1] (x1 None for one source), t0 the residual, or
    t0 / t1 the skip conv's one or two sources, [B, Zo, Yo, Xo, C].  Returns the output tensor, out_shape = [B, Zo, Yo, Xo, stride]."""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (x0, x1, t0, t1)]
    out = np.empty(out_shape, np.float32)
    check(hook("cm_debug_conv_tail")(handle, index, *[None if a is None else a.ctypes.data for a in arrs], out.ctypes.data, arrs[0].shape[0]))
    return out


def debug_attn_core(qkv: np.ndarray, heads: int, f16: bool):
    """One attention core launch alone on qkv [B, S, 3 E] (q | k | v per token): attn_core_f16_kernel (f16) or attn_core_kernel.
    Returns out [B, S, E].  Needs no handle."""
    qkv = np.ascontiguousarray(qkv, dtype=np.float32)
    B, S, E3 = qkv.shape
    out = np.empty((B, S, E3 // 3), np.float32)
    check(hook("cm_debug_attn_core")(qkv.ctypes.data, out.ctypes.data, B, S, E3 // 3, heads, 1 if f16 else 0))
    return out


def debug_attn_pack(w: np.ndarray):
    """Host-side h2 fragment pack of a dense weight [N, K] for the whole-sample attention kernel: (hi, mid) as float32
    arrays [N, K] of the f16 values (un-permuted from the kernel's lane order) and the power-of-two scale."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    N, K = w.shape
    halves = np.empty(N * K * 2, np.uint16)
    scale = C.c_float(0.0)
    check(hook("cm_debug_attn_pack")(w.ctypes.data, N, K, halves.ctypes.data, C.byref(scale)))
    f = halves.view(np.float16).astype(np.float32).reshape(N // 16, K // 32, 2, 4, 16, 8)   # [cb][ks][term][g][n % 16][i]
    t = f.transpose(2, 0, 4, 1, 3, 5).reshape(2, N, K)                                      # [term][cb, n % 16][ks, g, i]
    return t[0], t[1], float(scale.value)


def device_count() -> int:
    n = C.c_int(0)
    check(lib().cm_device_count(C.byref(n)))
    return n.value


def ptr(x) -> int:
    """Device or host address of a numpy array / torch tensor / DeviceBuffer / int / None."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    raise TypeError(f"cannot take the address of {type(x)}")


class DeviceBuffer:
    """Raw device allocation owned by Python (cm_malloc / cm_free)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.device, self.nbytes = device, int(nbytes)
        p = C.c_void_p()
        check(lib().cm_malloc(device, C.byref(p), self.nbytes))
        self.ptr = p.value

    def upload(self, arr: np.ndarray) -> "DeviceBuffer":
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(lib().cm_memcpy_h2d(self.device, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, shape, dtype=np.float32) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(lib().cm_memcpy_d2h(self.device, out.ctypes.data, self.ptr, out.nbytes))
        return out

    @classmethod
    def from_array(cls, arr: np.ndarray, device: int = 0) -> "DeviceBuffer":
        arr = np.ascontiguousarray(arr)
        return cls(arr.nbytes, device).upload(arr)

    def free(self):
        if getattr(self, "ptr", None):
            lib().cm_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
