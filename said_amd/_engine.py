"""ctypes binding of libsaid_hip.so.

`ABI` below is the one description of the library's C surface: group -> Group(headers, feature, table).  The "core" group (include/said_hip.h
and csrc/said_hip_debug.h) is bound when the library is loaded and guarded by said_abi_version; every other group is bound on first use
(load_library(group)) and lies outside the ABI version, so a library built before a group still loads and only what uses the group raises
"rebuild".  tests/test_host_cpu.py checks every group against its headers: names, parameter counts, kinds and sizes.

To add a context: declare its entry points in a header of their own, add one Group to `ABI`, and write one subclass of _Context that names
its prefix and group.  Host arrays go through _f32 / _f64 / _i32 / _i64 and the pointer helpers _fp / _dp / _ip / _lp / _vp, device tensors
through _dev and _ptr, and calls through _Context._go (entries that end in a stream) or _Context._call (the others).

There is deliberately no fallback: if the library is missing, cannot be loaded,
or no gfx950 device is visible, every entry point raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_void_p
from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np
import torch

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libsaid_hip.so")
_lib = None

PRED = {"epsilon": 0, "sample": 1, "v_prediction": 2}
PRECISIONS = {"fp32": 0, "bf16": 1, "fp32_strict": 2}   # SAID_PREC_* of include/said_hip.h
NCOEF = 8
COEF_SOLVER = 7   # SAID_COEF_SOLVER: column 7 of a coefficient row
SOLVER = {"ddim": 0, "ddpm": 1, "dpm1": 2, "dpm2": 3}
ABI_VERSION = 9   # include/said_hip.h as bound below; a stale libsaid_hip.so is refused at load time


class EngineError(RuntimeError):
    pass


class NoCpuPathError(EngineError, NotImplementedError):
    """A model method called on a CPU-resident model: said_amd computes on the MI355X only."""


_c_ll, _c_ull = ctypes.c_longlong, ctypes.c_ulonglong
_c_float_p, _c_double_p, _c_int_p, _c_ll_p, _c_void_pp = POINTER(c_float), POINTER(c_double), POINTER(c_int), POINTER(_c_ll), POINTER(c_void_p)

# ---- the constants and structs of the headers
METRICS_DIM, METRICS_MAX_K = 64, 8     # include/said_metrics.h
W_UNIT, W_LABELS, W_RESP = 0, 1, 2   # SAID_METRICS_W_*
OPTIMIZE_MAX_K = 64                    # include/said_optimize.h
OPT_CONVERGED, OPT_MAX_ITER, OPT_NOT_FINITE = 0, 1, 2   # SAID_OPTIMIZE_*
# SAID_TRAIN_* of include/said_train.h
TRAIN_NSCAL, TRAIN_NACC, TRAIN_ITEM = 16, 8, 4
(TRAIN_S_LR, TRAIN_S_WD_FACTOR, TRAIN_S_STEP_SIZE, TRAIN_S_BC2_SQRT, TRAIN_S_EMA_OMD, TRAIN_S_BETA, TRAIN_S_WVEL, TRAIN_S_OMB1, TRAIN_S_B2,
 TRAIN_S_OMB2, TRAIN_S_EPS, TRAIN_S_USE_EMA) = range(12)
TRAIN_STATE, TRAIN_EMA, TRAIN_GRAD, TRAIN_EXP_AVG, TRAIN_EXP_AVG_SQ = range(5)
TRAIN_OK, TRAIN_NOT_FINITE = 0, 1
TRAIN_SET_TRAIN, TRAIN_SET_VAL = 0, 1
UT_NSCAL, UT_NACC, UT_NUM_TENSORS = 16, 8, 161   # SAID_UT_* of include/said_unet_train.h
(UT_S_LR, UT_S_WD_FACTOR, UT_S_STEP_SIZE, UT_S_BC2_SQRT, UT_S_EMA_OMD, UT_S_WVEL, UT_S_WVERTEX, UT_S_OMB1, UT_S_B2, UT_S_OMB2, UT_S_EPS,
 UT_S_USE_EMA, UT_S_PRED_TYPE, UT_S_DROPOUT) = range(14)
UT_STATE, UT_EMA, UT_GRAD, UT_EXP_AVG, UT_EXP_AVG_SQ, UT_STASH = range(6)
RENDER_MAX_K, RENDER_MAX_LIGHTS, RENDER_LUT = 64, 4, 256   # SAID_RENDER_* of include/said_render.h
JPEG_OVERFLOW = 1   # SAID_JPEG_OVERFLOW
BEAT_N_FFT, BEAT_HOP, BEAT_N_MELS = 2048, 512, 128   # SAID_BEAT_* of include/said_beat.h
TRANSFER_CONVERGED, TRANSFER_MAX_ITER, TRANSFER_NOT_FINITE = 0, 1, 2   # SAID_TRANSFER_* of include/said_transfer.h
TRANSFER_ROW_SMOOTH, TRANSFER_ROW_IDENTITY, TRANSFER_ROW_CLOSEST, TRANSFER_ROW_UNIT = range(4)
TRANSFER_RHS_PAIR, TRANSFER_RHS_IDENTITY, TRANSFER_RHS_ANCHOR = range(3)
_TRANSFER_ARRAYS = ("rowptr", "col", "c0", "c1", "rowclass", "rowaux", "rhsclass", "at_rowptr", "at_col", "at_src")


class LoopParams(ctypes.Structure):
    """said_loop_params."""
    _fields_ = [
        ("batch", c_int), ("frames", c_int), ("num_steps", c_int), ("prediction_type", c_int),
        ("guidance_scale", c_float), ("guidance_rescale", c_float), ("latent_scale", c_float),
        ("use_step_noise", c_int), ("use_mask", c_int), ("save_intermediate", c_int),
        ("timesteps_host", _c_ll_p), ("coef_host", _c_float_p),
        ("context_dev", c_void_p), ("latents_dev", c_void_p), ("step_noise_dev", c_void_p),
        ("init_latents_dev", c_void_p), ("edit_noise_dev", c_void_p), ("mask_dev", c_void_p),
        ("intermediates_dev", c_void_p), ("result_dev", c_void_p), ("noise_seed", ctypes.c_uint64),
        ("noise_batch_offset", c_int), ("concurrent", c_int),
    ]


class AudioTrainParams(ctypes.Structure):
    """Mirror of said_audio_train_params (include/said_audio_train.h)."""
    _fields_ = [("p_feat_proj", c_float), ("p_hidden", c_float), ("p_attention", c_float), ("p_activation", c_float),
                ("seed", ctypes.c_uint64), ("time_mask_dev", c_void_p), ("skip_layers", ctypes.c_uint32)]


class RenderScene(ctypes.Structure):
    """said_render_scene."""
    _fields_ = [
        ("width", c_int), ("height", c_int),
        ("fx", c_float), ("fy", c_float), ("cx", c_float), ("cy", c_float), ("znear", c_float), ("zfar", c_float),
        ("cam_pos", c_float * 3), ("n_lights", c_int),
        ("light_pos", (c_float * 3) * RENDER_MAX_LIGHTS), ("light_intensity", c_float * RENDER_MAX_LIGHTS),
        ("ambient", c_float), ("base_color", c_float * 3),
        ("metallic", c_float), ("roughness", c_float), ("vc_metallic", c_float), ("vc_roughness", c_float),
    ]


class TransferSystem(ctypes.Structure):
    """said_transfer_system: the host-built index structure of a system."""
    _fields_ = [("m", c_int), ("n", c_int), ("nnz", c_int)] + [(name, _c_int_p) for name in _TRANSFER_ARRAYS]


class Group(NamedTuple):
    """The entry points that are bound together."""
    headers: tuple   # the headers that declare them, relative to the repository root
    feature: str     # what a library without them predates, for the "rebuild" error
    table: dict      # {name: (restype, argtypes)}
    late: dict = {}  # {group: (feature, names)}: entries of `table` that these headers declare but that are bound as a group of their own


ABI = {
    "core": Group(("include/said_hip.h", "said_amd/csrc/said_hip_debug.h"), f"ABI version {ABI_VERSION}", {
        "said_abi_version": (c_int, []),
        "said_create": (c_int, [_c_void_pp, c_int, c_int, c_int, c_int, c_int]),
        "said_destroy": (c_int, [c_void_p]),
        "said_reserve": (c_int, [c_void_p, c_int, c_int]),
        "said_capacity": (c_int, [c_void_p, _c_int_p, _c_int_p]),
        "said_clone": (c_int, [c_void_p, _c_void_pp, c_int, c_int]),
        "said_stream": (c_void_p, [c_void_p]),
        "said_loop_prepare": (c_int, [c_void_p, POINTER(LoopParams), c_void_p]),
        "said_last_error": (c_char_p, [c_void_p]),
        "said_set_weight": (c_int, [c_void_p, c_char_p, c_void_p, _c_ll_p, c_int]),
        "said_finalize_weights": (c_int, [c_void_p, c_void_p]),
        "said_set_timestep_freqs": (c_int, [c_void_p, c_void_p, c_int]),
        "said_audio_encode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, _c_int_p, c_void_p]),
        "said_unet_forward": (c_int, [c_void_p, c_void_p, _c_ll_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
        "said_denoise_loop": (c_int, [c_void_p, POINTER(LoopParams), c_void_p]),
        "said_ddim_step": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, _c_float_p, c_int, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
        "said_solver_step": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_void_p, _c_float_p, c_int, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
        "said_axpby": (c_int, [c_void_p, _c_float_p, c_void_p, _c_float_p, c_void_p, c_void_p, c_int, c_int64, c_void_p]),
        "said_graph_num_nodes": (c_int, [c_void_p]),
        "said_loop_progress": (c_int, [c_void_p, _c_int_p]),
        "said_loop_progress_reset": (c_int, [c_void_p]),
        "said_set_precision": (c_int, [c_void_p, c_int]),
        "said_get_precision": (c_int, [c_void_p]),
        "said_effective_precision": (c_int, [c_void_p]),
        "said_precision_note": (c_char_p, [c_void_p]),
        "said_numeric_status": (c_int, [c_void_p, c_void_p, _c_int_p, _c_int_p]),
        "said_profile_unet": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, _c_int_p, c_void_p]),
        "said_philox_normal": (c_int, [c_void_p, ctypes.c_uint64, c_int, c_int, c_int64, c_void_p, c_void_p]),
        "said_debug_option": (c_int, [c_void_p, c_char_p, _c_ll]),
        "said_debug_get": (_c_ll, [c_void_p, c_char_p]),
        "said_debug_stop_after": (c_int, [c_void_p, c_int]),
        "said_debug_clocks": (c_int, [c_void_p, c_int, c_void_p]),
        "said_debug_read": (c_int, [c_void_p, c_char_p, c_void_p, c_int64]),
        "said_debug_ws_count": (c_int, [c_void_p]),
        "said_debug_ws_info": (c_int, [c_void_p, c_int, _c_void_pp, _c_ll_p, POINTER(c_char_p)]),
        "said_debug_ws_fill": (c_int, [c_void_p, c_int]),
        "said_debug_ws_copy": (c_int, [c_void_p, c_int, c_void_p, _c_ll, c_void_p]),
        "said_debug_audio_copy": (c_int, [c_void_p, c_char_p, c_void_p, _c_ll, c_void_p]),
        "said_debug_audio_fill": (c_int, [c_void_p, c_int]),
        "said_unet_algorithmic_bytes": (c_double, [c_int, c_int, c_int]),
        "said_unet_algorithmic_flops": (c_double, [c_int, c_int]),
        "said_vae_create": (c_int, [_c_void_pp, c_int, c_int, c_int, c_int]),
        "said_vae_destroy": (c_int, [c_void_p]),
        "said_vae_last_error": (c_char_p, [c_void_p]),
        "said_vae_set_weight": (c_int, [c_void_p, c_char_p, c_void_p, _c_ll_p, c_int]),
        "said_vae_finalize_weights": (c_int, [c_void_p]),
        "said_vae_encode": (c_int, [c_void_p, c_void_p, _c_ll, c_int, c_void_p, c_void_p, c_void_p]),
        "said_vae_has_decoder": (c_int, [c_void_p]),
        "said_vae_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    }, late={   # added to said_hip.h without an ABI version bump: load_library("vae_decoder") binds them
        "vae_decoder": ("the VAE decoder", ("said_vae_has_decoder", "said_vae_decode")),
    }),
    "metrics": Group(("include/said_metrics.h",), "the metrics passes", {
        "said_metrics_create": (c_int, [_c_void_pp, c_int, _c_ll]),
        "said_metrics_destroy": (c_int, [c_void_p]),
        "said_metrics_last_error": (c_char_p, [c_void_p]),
        "said_metrics_max_points": (_c_ll, [c_void_p]),
        "said_metrics_weighted_sums": (c_int, [c_void_p, c_void_p, _c_ll, c_int, c_int, _c_double_p, _c_double_p, c_void_p]),
        "said_metrics_weighted_scatter": (c_int, [c_void_p, c_void_p, _c_ll, c_int, c_int, _c_double_p, _c_double_p, c_void_p]),
        "said_metrics_gmm_estep": (c_int, [c_void_p, c_void_p, _c_ll, c_int, _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                           _c_double_p, c_void_p, c_void_p, c_void_p]),
        "said_metrics_kmeans_assign": (c_int, [c_void_p, c_void_p, _c_ll, c_int, _c_double_p, c_int, _c_ll_p, _c_double_p, c_void_p]),
        "said_metrics_kmeans_read": (c_int, [c_void_p, _c_ll, _c_int_p, _c_double_p, c_void_p]),
        "said_metrics_kmeans_set_labels": (c_int, [c_void_p, _c_ll, c_int, _c_int_p, c_void_p]),
        "said_metrics_kmeanspp_first": (c_int, [c_void_p, c_void_p, _c_ll, _c_ll, _c_double_p, c_void_p]),
        "said_metrics_kmeanspp_step": (c_int, [c_void_p, c_void_p, _c_ll, _c_double_p, c_int, _c_ll_p, _c_double_p, c_void_p]),
    }),
    "optimize": Group(("include/said_optimize.h",), "the blendshape fit", {
        "said_optimize_create": (c_int, [_c_void_pp, c_int]),
        "said_optimize_destroy": (c_int, [c_void_p]),
        "said_optimize_last_error": (c_char_p, [c_void_p]),
        "said_optimize_set_bases": (c_int, [c_void_p, c_int, c_int, _c_ll, _c_double_p, _c_double_p, _c_double_p, c_void_p]),
        "said_optimize_rhs": (c_int, [c_void_p, c_int, c_void_p, _c_ll, c_void_p, c_void_p]),
        "said_optimize_solve": (c_int, [c_void_p, c_int, _c_ll_p, _c_int_p, c_void_p, c_double, c_int, c_int, c_double, c_void_p, c_void_p,
                                        _c_int_p, _c_int_p, _c_double_p, c_void_p]),
    }),
    "train": Group(("include/said_train.h",), "the BCVAE trainer", {
        "said_train_create": (c_int, [_c_void_pp, c_int, c_int]),
        "said_train_destroy": (c_int, [c_void_p]),
        "said_train_last_error": (c_char_p, [c_void_p]),
        "said_train_tensor_name": (c_char_p, [c_int]),
        "said_train_tensor_numel": (_c_ll, [c_int]),
        "said_train_tensor_is_counter": (c_int, [c_int]),
        "said_train_set_tensor": (c_int, [c_void_p, c_int, c_char_p, c_void_p, _c_ll]),
        "said_train_get_tensor": (c_int, [c_void_p, c_int, c_char_p, c_void_p, _c_ll]),
        "said_train_reset_optimizer": (c_int, [c_void_p]),
        "said_train_set_data": (c_int, [c_void_p, c_int, _c_float_p, _c_ll, _c_ll_p, _c_int_p, c_int, _c_int_p]),
        "said_train_gather": (c_int, [c_void_p, c_int, c_int, _c_int_p, _c_float_p]),
        "said_train_step": (c_int, [c_void_p, c_int, _c_int_p, _c_float_p, _c_float_p, _c_float_p, c_int]),
        "said_train_apply_update": (c_int, [c_void_p, _c_float_p]),
        "said_train_eval_loss": (c_int, [c_void_p, c_int, c_int, _c_int_p, _c_float_p, _c_float_p, _c_float_p, c_int]),
        "said_train_read_losses": (c_int, [c_void_p, c_int, _c_double_p, _c_int_p, c_int]),
        "said_train_last_losses": (c_int, [c_void_p, _c_float_p]),
        "said_train_bn_stats": (c_int, [c_void_p, c_int, _c_float_p]),
        "said_train_graph_count": (c_int, [c_void_p]),
    }),
    "render": Group(("include/said_render.h",), "the renderer", {
        "said_render_create": (c_int, [_c_void_pp, c_int]),
        "said_render_destroy": (c_int, [c_void_p]),
        "said_render_last_error": (c_char_p, [c_void_p]),
        "said_render_set_mesh": (c_int, [c_void_p, c_int, c_int, c_int, _c_double_p, _c_int_p, _c_double_p, c_void_p]),
        "said_render_set_scene": (c_int, [c_void_p, c_void_p]),
        "said_render_set_colormap": (c_int, [c_void_p, _c_float_p, c_void_p]),
        "said_render_render": (c_int, [c_void_p, c_void_p, c_void_p, _c_ll, c_int, c_float, _c_double_p, _c_double_p, c_void_p, c_void_p,
                                       c_void_p]),
        "said_render_read_vertices": (c_int, [c_void_p, c_int, _c_float_p, c_void_p]),
        "said_render_read_normals": (c_int, [c_void_p, c_int, _c_float_p, c_void_p]),
        "said_render_read_colors": (c_int, [c_void_p, c_int, _c_float_p, c_void_p]),
    }),
    # the sample count is an argument of this one call: the renderer's own header and scene keep their shape
    "render_ms": Group(("include/said_render_ms.h",), "multisampled rendering", {
        "said_render_render_ms": (c_int, [c_void_p, c_int, c_void_p, c_void_p, _c_ll, c_int, c_float, _c_double_p, _c_double_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    }),
    "jpeg": Group(("include/said_jpeg.h",), "the JPEG encoder", {
        "said_jpeg_create": (c_int, [_c_void_pp, c_int]),
        "said_jpeg_destroy": (c_int, [c_void_p]),
        "said_jpeg_last_error": (c_char_p, [c_void_p]),
        "said_jpeg_configure": (c_int, [c_void_p, c_int, c_int, c_int]),
        "said_jpeg_header": (c_int, [c_void_p, c_void_p, _c_ll, _c_ll_p]),
        "said_jpeg_encode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, _c_ll, c_void_p, _c_ll_p, c_void_p]),
        "said_jpeg_read_coefficients": (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    }),
    "unet_train": Group(("include/said_unet_train.h",), "the UNet trainer", {
        "said_unet_train_create": (c_int, [_c_void_pp, c_int, c_int, c_int]),
        "said_unet_train_create_dim": (c_int, [_c_void_pp, c_int, c_int, c_int, c_int]),
        "said_unet_train_destroy": (c_int, [c_void_p]),
        "said_unet_train_last_error": (c_char_p, [c_void_p]),
        "said_unet_train_tensor_name": (c_char_p, [c_int]),
        "said_unet_train_tensor_numel": (_c_ll, [c_int]),
        "said_unet_train_table_size": (c_int, [c_int]),
        "said_unet_train_table_name": (c_char_p, [c_int, c_int]),
        "said_unet_train_table_numel": (_c_ll, [c_int, c_int]),
        "said_unet_train_num_tensors": (c_int, [c_void_p]),
        "said_unet_train_context_tensor_name": (c_char_p, [c_void_p, c_int]),
        "said_unet_train_context_tensor_numel": (_c_ll, [c_void_p, c_int]),
        "said_unet_train_feature_dim": (c_int, [c_void_p]),
        "said_unet_train_set_tensor": (c_int, [c_void_p, c_int, c_char_p, _c_float_p, _c_ll]),
        "said_unet_train_get_tensor": (c_int, [c_void_p, c_int, c_char_p, _c_float_p, _c_ll]),
        "said_unet_train_reset_optimizer": (c_int, [c_void_p]),
        "said_unet_train_copy": (c_int, [c_void_p, c_int, c_int]),
        "said_unet_train_set_alphas": (c_int, [c_void_p, _c_float_p, c_int]),
        "said_unet_train_step": (c_int, [c_void_p, c_int, c_int, _c_float_p, _c_float_p, _c_ll_p, _c_int_p, c_void_p, c_int, _c_ull, _c_float_p,
                                         _c_float_p, _c_float_p, c_int]),
        "said_unet_train_eval_loss": (c_int, [c_void_p, c_int, c_int, _c_float_p, _c_float_p, _c_ll_p, _c_int_p, c_void_p, c_int, _c_float_p,
                                              _c_float_p, _c_float_p, c_int, c_int]),
        "said_unet_train_forward_only": (c_int, [c_void_p, c_int, c_int, _c_float_p, _c_ll_p, _c_int_p, c_void_p, c_int, c_int, _c_float_p]),
        "said_unet_train_apply_update": (c_int, [c_void_p, _c_float_p]),
        "said_unet_train_read_losses": (c_int, [c_void_p, c_int, _c_double_p, _c_int_p, c_int]),
        "said_unet_train_last_losses": (c_int, [c_void_p, _c_float_p]),
    }),
    "beat": Group(("include/said_beat.h",), "the beat-consistency passes", {
        "said_beat_create": (c_int, [_c_void_pp, c_int]),
        "said_beat_destroy": (c_int, [c_void_p]),
        "said_beat_last_error": (c_char_p, [c_void_p]),
        "said_beat_set_sampling_rate": (c_int, [c_void_p, c_int, _c_int_p]),
        "said_beat_clips": (c_int, [c_void_p, c_void_p, c_int, _c_ll_p, c_void_p]),
        "said_beat_coeffs": (c_int, [c_void_p, c_void_p, c_int, _c_ll_p, c_int, c_double, c_void_p]),
        "said_beat_score": (c_int, [c_void_p, _c_int_p, c_double, c_double, _c_double_p, c_void_p]),
        "said_beat_set_deltas": (c_int, [c_void_p, c_int, c_int, c_int, _c_double_p, c_void_p]),
        "said_beat_vertex_error": (c_int, [c_void_p, c_void_p, _c_ll, c_int, _c_ll_p, _c_ll_p, _c_int_p, _c_int_p, _c_double_p, c_void_p]),
        "said_beat_read_mel": (c_int, [c_void_p, _c_double_p, c_void_p]),
        "said_beat_read_envelope": (c_int, [c_void_p, _c_double_p, c_void_p]),
        "said_beat_read_onsets": (c_int, [c_void_p, _c_int_p, _c_int_p, c_void_p]),
        "said_beat_read_rates": (c_int, [c_void_p, _c_double_p, c_void_p]),
        "said_beat_read_minima": (c_int, [c_void_p, _c_int_p, _c_int_p, c_void_p]),
    }),
    "transfer": Group(("include/said_transfer.h",), "deformation transfer", {
        "said_transfer_create": (c_int, [_c_void_pp, c_int]),
        "said_transfer_destroy": (c_int, [c_void_p]),
        "said_transfer_last_error": (c_char_p, [c_void_p]),
        "said_transfer_set_source": (c_int, [c_void_p, c_int, c_int, c_int, _c_double_p, _c_int_p, _c_double_p, c_void_p]),
        "said_transfer_set_target": (c_int, [c_void_p, c_int, c_int, _c_double_p, _c_int_p, c_void_p]),
        "said_transfer_solve": (c_int, [c_void_p, c_int, c_int, c_int, c_int, _c_int_p, _c_int_p, _c_double_p, _c_int_p, _c_int_p,
                                        _c_double_p, _c_double_p, _c_double_p, c_double, c_int, c_int, _c_double_p, _c_int_p, _c_int_p,
                                        _c_double_p, c_void_p]),
        "said_transfer_register": (c_int, [c_void_p, c_void_p, c_int, _c_int_p, _c_double_p, c_double, c_double, c_int, _c_double_p, c_double, c_int,
                                           _c_double_p, _c_int_p, _c_int_p, _c_int_p, _c_double_p, c_void_p]),
        "said_transfer_correspond": (c_int, [c_void_p, _c_double_p, c_double, _c_int_p, _c_int_p, _c_double_p, _c_double_p, c_void_p]),
        "said_transfer_transfer": (c_int, [c_void_p, c_void_p, c_double, c_int, _c_double_p, _c_int_p, _c_int_p, _c_double_p, c_void_p]),
        "said_transfer_mesh": (c_int, [c_void_p, c_int, c_int, _c_double_p, _c_int_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                       c_void_p]),
        "said_transfer_gradients": (c_int, [c_void_p, c_int, c_int, _c_double_p, _c_int_p, c_int, _c_double_p, _c_double_p, c_void_p]),
        "said_transfer_closest": (c_int, [c_void_p, c_int, _c_double_p, _c_double_p, c_int, _c_double_p, _c_double_p, _c_int_p, _c_double_p, c_void_p]),
    }),
    # an entry point of the said_ctx context, added without an ABI version bump
    "audio_train": Group(("include/said_audio_train.h",), "the audio encoder's train mode", {
        "said_audio_encode_train": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(AudioTrainParams), c_void_p, _c_int_p, c_void_p]),
    }),
}
# Groups added since: entry points of existing contexts, declared in headers of their own and bound on first use, outside the ABI version
_ABI_ADDED = {
    "unet_finetune": Group(("said_amd/csrc/said_unet_finetune.h",), "fine-tuning the audio encoder in the UNet trainer", {
        "said_unet_train_create_ft": (c_int, [_c_void_pp, c_int, c_int, c_int, c_int, c_int]),
        "said_unet_train_table_size_ft": (c_int, [c_int, c_int]),
        "said_unet_train_table_name_ft": (c_char_p, [c_int, c_int, c_int]),
        "said_unet_train_table_numel_ft": (_c_ll, [c_int, c_int, c_int]),
        "said_unet_train_finetune_layers": (c_int, [c_void_p]),
        "said_unet_train_step_ft": (c_int, [c_void_p, c_int, c_int, _c_float_p, _c_float_p, _c_ll_p, _c_int_p, c_void_p, c_int, POINTER(AudioTrainParams),
                                            _c_ull, _c_float_p, _c_float_p, _c_float_p, c_int]),
        "said_unet_train_eval_loss_ft": (c_int, [c_void_p, c_int, c_int, _c_float_p, _c_float_p, _c_ll_p, _c_int_p, c_void_p, c_int,
                                                 POINTER(AudioTrainParams), _c_float_p, _c_float_p, _c_float_p, c_int, c_int]),
        "said_unet_train_forward_only_ft": (c_int, [c_void_p, c_int, c_int, _c_float_p, _c_ll_p, _c_int_p, c_void_p, c_int, POINTER(AudioTrainParams),
                                                    c_int, _c_float_p]),
        "said_unet_train_last_conditioning": (c_int, [c_void_p, c_int, c_int, _c_float_p]),
    }),
    "unet_products": Group(("said_amd/csrc/said_unet_train_products.h",), "split-fp16 products of the fine-tuned audio encoder", {
        "said_unet_train_set_encoder_products": (c_int, [c_void_p, c_int]),
        "said_unet_train_encoder_products": (c_int, [c_void_p]),
        "said_unet_train_dense_product": (c_int, [c_void_p, c_int, c_int, c_int, c_int, _c_float_p, _c_float_p, _c_float_p, _c_float_p, c_int, c_int,
                                                  _c_float_p]),
    }),
    "audio_features": Group(("said_amd/csrc/said_audio_features.h",), "the audio encoder's front end as a callable", {
        "said_audio_extract_features": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, _c_int_p, c_void_p]),
    }),
}


def added_groups() -> dict:
    """{group: Group} of the groups added beside ABI."""
    return dict(_ABI_ADDED)


_bound = set()   # the groups bound so far


def library_path() -> str:
    return _LIB_PATH


def _group(group: str):
    """(feature, table) of a group of ABI, without its late entries, or of a late part of one."""
    if group in ABI or group in _ABI_ADDED:
        g = ABI[group] if group in ABI else _ABI_ADDED[group]
        late = {name for _, names in g.late.values() for name in names}
        return g.feature, {name: sig for name, sig in g.table.items() if name not in late}
    for g in ABI.values():
        if group in g.late:
            feature, names = g.late[group]
            return feature, {name: g.table[name] for name in names}
    raise KeyError(group)


def _bind(lib, group: str) -> None:
    feature, table = _group(group)
    for name in table:
        if not hasattr(lib, name):
            raise EngineError(f"{_LIB_PATH} predates {feature} ({name} is not exported): rebuild it with `python -m said_amd.build --force`")
    for name, (res, args) in table.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _bound.add(group)


def load_library(group: Optional[str] = None):
    """dlopen the engine and bind the core group of ABI (no compute); with `group`, also that group."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise EngineError(
                f"{_LIB_PATH} not found: build it with `python -m said_amd.build` (hipcc, gfx950). "
                "said_amd has no CPU fallback.")
        lib = ctypes.CDLL(_LIB_PATH)
        _bind(lib, "core")
        got = lib.said_abi_version()
        if got != ABI_VERSION:
            raise EngineError(f"{_LIB_PATH} has ABI version {got}, this binding expects {ABI_VERSION}: rebuild it with "
                              "`python -m said_amd.build --force`")
        _lib = lib
    if group is not None and group not in _bound:
        _bind(_lib, group)
    return _lib


# ---- marshalling: host arrays, pointers to them, device tensors
def _array_of(dtype):
    """The helper of one element type: a C-contiguous host array of it (no copy of what already is one); None passes through."""
    return lambda a: None if a is None else np.ascontiguousarray(a, dtype=dtype)


def _pointer_to(ctype):
    """The helper of one pointee type: a host array's memory as that ctypes pointer; None passes through."""
    return lambda a: None if a is None else a.ctypes.data_as(ctype)


_f32, _f64, _i32, _i64 = _array_of(np.float32), _array_of(np.float64), _array_of(np.int32), _array_of(np.int64)
_fp, _dp, _ip, _lp, _vp = _pointer_to(_c_float_p), _pointer_to(_c_double_p), _pointer_to(_c_int_p), _pointer_to(_c_ll_p), _pointer_to(c_void_p)


def host_f32(a) -> np.ndarray:
    """A contiguous float32 host array of an array, a list or a tensor (on any device)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return _f32(a)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else c_void_p(t.data_ptr())


def _stream() -> c_void_p:
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t: torch.Tensor, name: str, dtype=torch.float32, index: Optional[int] = None, trailing: Optional[tuple] = None, numel: int = 0,
         strict: bool = False) -> torch.Tensor:
    """`t` as a contiguous `dtype` tensor on the GPU; where given: on cuda:`index`, of shape (n, *trailing), of at least `numel` elements.
    A tensor that is not contiguous is copied; with `strict` it is refused (an output, or an input whose owner promised the layout)."""
    if not strict:
        t = t.contiguous()
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and (index is None or t.device.index == index)
            and (trailing is None or tuple(t.shape[1:]) == tuple(trailing)) and t.numel() >= numel):
        shape = "" if trailing is None else f" of shape (n, {', '.join(str(n) for n in trailing)})"
        raise EngineError(f"{name} must be a contiguous {dtype} tensor{shape} on " + ("the MI355X" if index is None else f"cuda:{index}")
                          + (f" with at least {numel} elements" if numel else "") + f", got {tuple(t.shape)} {t.dtype} on {t.device}"
                          + ("" if t.is_cuda else "; said_amd has no CPU path"))
    return t


def _w2v_frames(num_samples: int) -> int:
    """Frames that Wav2Vec2's seven feature-extractor convolutions leave of `num_samples` samples."""
    for k, s in zip((10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)):
        num_samples = (num_samples - k) // s + 1
    return num_samples


class _Context:
    """One C context of the library on one GPU, created by <prefix>_create, released by <prefix>_destroy; <prefix>_last_error gives
    the message of a failed call (NULL: of a failed create).  A subclass names its prefix, its group of ABI and how it refuses a
    device that is not a GPU."""
    prefix = ""
    group: Optional[str] = None
    cpu_error = EngineError
    cpu_message = "said_amd runs on MI355X only (device={}); there is no CPU fallback"

    def __init__(self, device: torch.device):
        device = torch.device(device)
        if device.type != "cuda":   # refused before the library is looked for: the answer does not depend on a build
            raise self.cpu_error(self.cpu_message.format(device))
        self.lib = load_library(self.group)
        self.device = device
        self.index = device.index if device.index is not None else torch.cuda.current_device()

    def _create(self, *args, entry: Optional[str] = None) -> None:
        """<entry, default <prefix>_create>(&h, device index, *args)."""
        entry = entry or self.prefix + "_create"
        h = c_void_p()
        if getattr(self.lib, entry)(ctypes.byref(h), self.index, *args) != 0:
            raise EngineError(f"{entry}: " + self._last_error(None))
        self.h = h

    def _last_error(self, h) -> str:
        return (getattr(self.lib, self.prefix + "_last_error")(h) or b"?").decode()

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, self.prefix + "_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name: str, *args, what: Optional[str] = None) -> None:
        """name(h, *args); EngineError("<what or name>: <last error>") when it fails."""
        if getattr(self.lib, name)(self.h, *args) != 0:
            raise EngineError(f"{what or name}: " + self._last_error(self.h))

    def _go(self, name: str, *args) -> None:
        """_call with this context's GPU current and the current stream as the last argument: for the entries that end in a stream."""
        with torch.cuda.device(self.index):
            self._call(name, *args, _stream())


def audio_train_params(draws, cfg, B: int, frames: int, device):
    """(said_audio_train_params, the device tensor its mask pointer refers to or None) of an AudioTrainDraws and an AudioTrainConfig
    (said_amd.model.wav2vec2) for B clips of `frames` frames."""
    mask = None
    if draws.mask is not None:
        m = np.ascontiguousarray(np.asarray(draws.mask) != 0, dtype=np.uint8)
        if m.shape != (B, frames):
            raise EngineError(f"time mask of shape {m.shape} does not match {B} clips of {frames} frames")
        mask = torch.from_numpy(m).to(device)
    skip = 0
    for l, sk in enumerate(draws.skip):
        skip |= int(bool(sk)) << l
    if skip >> 32:
        raise EngineError("skip list longer than 32 layers")
    return AudioTrainParams(cfg.feat_proj_dropout, cfg.hidden_dropout, cfg.attention_dropout, cfg.activation_dropout,
                            int(draws.seed) & 0xFFFFFFFFFFFFFFFF, _ptr(mask), skip), mask


class Engine(_Context):
    """One engine context on one GPU (one process per GPU)."""
    prefix = "said"

    def __init__(self, device: torch.device, max_batch_eff: int, max_frames: int, in_channels: int = 32, ctx_dim: int = 768, _clone_of=None):
        super().__init__(device)
        self.max_batch_eff, self.max_frames = int(max_batch_eff), int(max_frames)
        self.in_channels, self.ctx_dim = in_channels, ctx_dim
        self._parent = _clone_of   # a clone shares its parent's packed weights: keep the parent alive, destroy the clone first
        if _clone_of is not None:
            h = c_void_p()
            _clone_of._call("said_clone", ctypes.byref(h), self.max_batch_eff, self.max_frames)
            self.h = h
        else:
            self._create(self.max_batch_eff, self.max_frames, in_channels, ctx_dim)
        self.has_audio = _clone_of.has_audio if _clone_of is not None else False
        self._clones = []
        self._keep = []  # host buffers referenced by in-flight async copies
        sp = self.lib.said_stream(self.h) if _clone_of is not None else None
        self.stream = torch.cuda.ExternalStream(sp, device=self.device) if sp else None   # a clone's own stream

    def clone(self, max_batch_eff: int, max_frames: int) -> "Engine":
        """A context sharing this one's packed weights, with its own workspace and step graph (said_clone): for concurrent
        denoising loops on a second stream.  Closed together with this engine."""
        c = Engine(self.device, max_batch_eff, max_frames, self.in_channels, self.ctx_dim, _clone_of=self)
        self._clones.append(c)
        return c

    def close(self):
        for c in getattr(self, "_clones", []):
            c.close()      # clones first: they point into this context's weights
        self._clones = []
        super().close()

    def reserve(self, max_batch_eff: int, max_frames: int) -> None:
        """Grow the workspace (never shrinks); the packed weights stay on the device (said_reserve)."""
        with torch.cuda.device(self.index):
            rc = self.lib.said_reserve(self.h, int(max_batch_eff), int(max_frames))
        msg = self._last_error(self.h) if rc != 0 else ""
        b, t = c_int(0), c_int(0)
        self._call("said_capacity", ctypes.byref(b), ctypes.byref(t))
        self.max_batch_eff, self.max_frames = b.value, t.value   # (0, 0) after a failed growth: the context refuses every size
        if rc != 0:
            raise EngineError("said_reserve: " + msg)

    # ---- weights ----
    def load_weights(self, state_dict: Dict[str, torch.Tensor]):
        """`state_dict` uses the reference's SAID key layout."""
        with torch.cuda.device(self.index):
            half = 96
            freqs = torch.exp(-np.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
            self._call("said_set_timestep_freqs", _vp(_f32(freqs.numpy())), half)
            for k, v in state_dict.items():
                a = _f32(v.detach().to("cpu", torch.float32).numpy())
                shape = (_c_ll * a.ndim)(*a.shape)
                self._call("said_set_weight", k.encode(), _vp(a), shape, a.ndim, what=f"said_set_weight({k})")
            self._call("said_finalize_weights", _stream())
        self.has_audio = any(k.startswith("audio_encoder.") for k in state_dict)

    # ---- compute ----
    def audio_encode(self, waveform: torch.Tensor, num_frames: Optional[int], apply_proj: bool = False, _train=None) -> torch.Tensor:
        waveform = _dev(waveform, "waveform")
        B, Ta = waveform.shape
        nf = int(num_frames) if num_frames is not None else 0
        # the frame count without interpolation is decided by the library
        out = torch.empty(B, nf if nf > 0 else max(_w2v_frames(Ta), 1), self.ctx_dim if apply_proj else 768, device=waveform.device, dtype=torch.float32)
        got = c_int(0)
        if _train is None:
            self._go("said_audio_encode", _ptr(waveform), B, Ta, nf, int(apply_proj), _ptr(out), ctypes.byref(got))
        else:
            self._go("said_audio_encode_train", _ptr(waveform), B, Ta, nf, int(apply_proj), ctypes.byref(_train), _ptr(out), ctypes.byref(got))
        assert got.value == out.shape[1], (got.value, out.shape)
        return out

    def extract_features(self, waveform: torch.Tensor, num_frames: Optional[int]) -> torch.Tensor:
        """(B, frames, 512): the frozen feature extractor's output after the interpolation, token-major (said_audio_extract_features):
        what a fine-tuning UNetTrainEngine takes as `features`."""
        load_library("audio_features")
        waveform = _dev(waveform, "waveform")
        B, Ta = waveform.shape
        nf = int(num_frames) if num_frames is not None else 0
        out = torch.empty(B, nf if nf > 0 else max(_w2v_frames(Ta), 1), 512, device=waveform.device, dtype=torch.float32)
        got = c_int(0)
        self._go("said_audio_extract_features", _ptr(waveform), B, Ta, nf, _ptr(out), ctypes.byref(got))
        assert got.value == out.shape[1], (got.value, out.shape)
        return out

    def audio_encode_train(self, waveform: torch.Tensor, num_frames: Optional[int], draws, cfg, apply_proj: bool = False) -> torch.Tensor:
        """audio_encode in Wav2Vec2's train mode (include/said_audio_train.h): `draws` is an AudioTrainDraws (time mask, skipped layers,
        dropout seed), `cfg` an AudioTrainConfig (the dropout probabilities) — said_amd.model.wav2vec2."""
        load_library("audio_train")
        cfg.check()
        B, frames = waveform.shape[0], int(num_frames or 0)
        if frames <= 0:   # no interpolation: the feature extractor's own frame count
            frames = _w2v_frames(waveform.shape[1])
        p, mask = audio_train_params(draws, cfg, B, frames, waveform.device)
        out = self.audio_encode(waveform, num_frames, apply_proj, _train=p)
        if mask is not None:
            mask.record_stream(torch.cuda.current_stream(waveform.device))
        return out

    def unet_forward(self, sample: torch.Tensor, timesteps: torch.Tensor, context: torch.Tensor) -> torch.Tensor:
        sample = _dev(sample, "sample")
        context = _dev(context, "encoder_hidden_states")
        Be, T, C = sample.shape
        if context.shape[0] != Be or context.shape[2] != self.ctx_dim:
            raise EngineError(f"context shape {tuple(context.shape)} does not match batch {Be} / ctx_dim {self.ctx_dim}")
        ts = _i64(timesteps.detach().to("cpu", torch.int64).reshape(-1).numpy())
        if ts.shape[0] != Be:
            raise EngineError(f"timesteps must have {Be} entries, got {ts.shape[0]}")
        out = torch.empty_like(sample)
        self._go("said_unet_forward", _ptr(sample), _lp(ts), _ptr(context), Be, T, context.shape[1], _ptr(out))
        return out

    def loop_job(self, *, latents: torch.Tensor, context: torch.Tensor, timesteps: np.ndarray, coef: np.ndarray,
                     prediction_type: str, guidance_scale: float, guidance_rescale: float, latent_scale: float,
                     step_noise: Optional[torch.Tensor] = None, init_latents: Optional[torch.Tensor] = None,
                     edit_noise: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                     save_intermediate: bool = False, noise_seed: Optional[int] = None, noise_batch_offset: int = 0, concurrent: bool = False):
        """Validates the arguments and allocates the outputs of one denoising loop (on the current stream): a job for
        prepare_loop / run_loop.  `noise_seed` (with step_noise None): the eta noise is generated inside the step's last
        kernel (Philox4x32-10 keyed by the seed) instead of being read from a tensor."""
        latents = _dev(latents, "latents").clone()
        context = _dev(context, "audio_embedding")
        B, T, C = latents.shape
        N = int(len(timesteps))
        ts = _i64(timesteps)
        cf = _f32(coef).reshape(N, NCOEF)
        result = torch.empty_like(latents)
        inter = torch.empty(N, B, T, C, device=latents.device, dtype=torch.float32) if save_intermediate else None
        use_mask = mask is not None and init_latents is not None
        keep = [ts, cf, latents, context, result, inter]
        p = LoopParams()
        p.batch, p.frames, p.num_steps, p.prediction_type = B, T, N, PRED[prediction_type]
        p.guidance_scale, p.guidance_rescale, p.latent_scale = float(guidance_scale), float(guidance_rescale), float(latent_scale)
        p.use_step_noise = int(step_noise is not None)
        p.use_mask = int(use_mask)
        p.save_intermediate = int(save_intermediate)
        p.concurrent = int(bool(concurrent))
        p.timesteps_host = _lp(ts)
        p.coef_host = _fp(cf)
        p.context_dev = context.data_ptr()
        p.latents_dev = latents.data_ptr()
        if step_noise is not None:
            step_noise = _dev(step_noise, "step_noise")
            assert tuple(step_noise.shape) == (N, B, T, C), step_noise.shape
            p.step_noise_dev = step_noise.data_ptr()
            keep.append(step_noise)
        elif noise_seed is not None:
            p.use_step_noise = 2
            p.noise_seed = int(noise_seed) & 0xFFFFFFFFFFFFFFFF
            p.noise_batch_offset = int(noise_batch_offset)
        if use_mask:
            init_latents = _dev(init_latents, "init_latents")
            edit_noise = _dev(edit_noise, "edit_noise")
            mask = _dev(mask.expand_as(latents) if mask.shape != latents.shape else mask, "mask")
            p.init_latents_dev, p.edit_noise_dev, p.mask_dev = init_latents.data_ptr(), edit_noise.data_ptr(), mask.data_ptr()
            keep += [init_latents, edit_noise, mask]
        if inter is not None:
            p.intermediates_dev = inter.data_ptr()
        p.result_dev = result.data_ptr()
        return p, keep, (result, latents, inter)

    # prepare_loop and run_loop are the loop's path: they stay spelled out, one frame shallower than _go
    def prepare_loop(self, job):
        """Builds the job's step graph if this context does not hold it yet (said_loop_prepare); launches nothing of the loop."""
        with torch.cuda.device(self.index):
            self._call("said_loop_prepare", ctypes.byref(job[0]), _stream())

    def run_loop(self, job):
        """Enqueues the job's loop on the current stream; returns (result, final_latents, intermediates or None)."""
        with torch.cuda.device(self.index):
            self._call("said_denoise_loop", ctypes.byref(job[0]), _stream())
        self._keep = job[1]  # alive until the next call (async copies / kernels may still reference them)
        return job[2]

    def denoise_loop(self, **kw):
        """loop_job + run_loop: returns (result, final_latents, intermediates or None)."""
        return self.run_loop(self.loop_job(**kw))

    def ddim_step(self, eps: torch.Tensor, sample: torch.Tensor, coef_row: np.ndarray, prediction_type: str,
                  eps_uncond: Optional[torch.Tensor] = None, guidance_scale: float = 1.0,
                  step_noise: Optional[torch.Tensor] = None, init_latents: Optional[torch.Tensor] = None,
                  edit_noise: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        eps, sample = _dev(eps, "model_output"), _dev(sample, "sample")
        out = torch.empty_like(sample)
        cf = _f32(coef_row).reshape(NCOEF)
        opt = [None if t is None else _dev(t, "tensor") for t in (eps_uncond, step_noise, init_latents, edit_noise, mask)]
        self._go("said_ddim_step", _ptr(eps), _ptr(opt[0]), float(guidance_scale), _ptr(sample), _fp(cf), PRED[prediction_type], _ptr(opt[1]),
                 _ptr(opt[2]), _ptr(opt[3]), _ptr(opt[4]), _ptr(out), sample.numel())
        torch.cuda.current_stream(self.index).synchronize()  # cf is a temporary
        return out

    def solver_step(self, model_output: torch.Tensor, sample: torch.Tensor, coef_row: np.ndarray, prediction_type: str,
                    x0_hist: Optional[torch.Tensor] = None, model_output_uncond: Optional[torch.Tensor] = None, guidance_scale: float = 1.0,
                    step_noise: Optional[torch.Tensor] = None, init_latents: Optional[torch.Tensor] = None,
                    edit_noise: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One DDPM / DPM-Solver++ row (said_solver_step).  `x0_hist` (DPM rows): the previous step's x0 in, this step's out (updated in place)."""
        model_output, sample = _dev(model_output, "model_output"), _dev(sample, "sample")
        out = torch.empty_like(sample)
        cf = _f32(coef_row).reshape(NCOEF)
        opt = [None if t is None else _dev(t, "tensor") for t in (model_output_uncond, step_noise, init_latents, edit_noise, mask)]
        for t in [x0_hist] + opt:
            if t is not None and t.numel() != sample.numel():
                raise EngineError(f"solver_step: every tensor must hold {sample.numel()} values, got {t.numel()}")
        if x0_hist is not None and (_dev(x0_hist, "x0_hist") is not x0_hist):
            raise EngineError("x0_hist must be contiguous: it is updated in place")
        self._go("said_solver_step", _ptr(model_output), _ptr(opt[0]), float(guidance_scale), _ptr(sample), _fp(cf), PRED[prediction_type],
                 _ptr(x0_hist), _ptr(opt[1]), _ptr(opt[2]), _ptr(opt[3]), _ptr(opt[4]), _ptr(out), sample.numel())
        torch.cuda.current_stream(self.index).synchronize()  # cf is a temporary
        return out

    def axpby(self, a: Sequence[float], x: torch.Tensor, c: Optional[Sequence[float]] = None, y: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev(x, "x")
        B = x.shape[0]
        if len(a) != B or (c is not None and len(c) != B):
            raise EngineError(f"axpby: need one coefficient per sample ({B}), got {len(a)}" + (f" / {len(c)}" if c is not None else ""))
        av = (c_float * B)(*[float(v) for v in a])
        cv = (c_float * B)(*[float(v) for v in (c if c is not None else [0.0] * B)])
        if y is not None:
            y = _dev(y, "y")
        out = torch.empty_like(x)
        self._go("said_axpby", av, _ptr(x), cv, _ptr(y), _ptr(out), B, x.numel() // B)
        return out

    def profile_unet(self, batch_eff: int, frames: int, reps: int = 50, cfg_clips: int = 0):
        """Per-launch (us, bytes, flops, kind, epi, NB, KS) of the UNet kernel schedule, HIP-event timed."""
        M = 128
        us = np.zeros(M, np.float32); by = np.zeros(M, np.float64); fl = np.zeros(M, np.float64)
        kind = np.zeros(M, np.int32); epi = np.zeros(M, np.int32); nb = np.zeros(M, np.int32); ks = np.zeros(M, np.int32)
        n = c_int(0)
        self._go("said_profile_unet", batch_eff, frames, cfg_clips, reps, M, _vp(us), _vp(by), _vp(fl), _vp(kind), _vp(epi), _vp(nb), _vp(ks),
                 ctypes.byref(n))
        k = n.value
        return [dict(us=float(us[i]), bytes=float(by[i]), flops=float(fl[i]), kind=int(kind[i]), epi=int(epi[i]), NB=int(nb[i]), KS=int(ks[i]))
                for i in range(k)]

    def philox_normal(self, seed: int, step0: int, nsteps: int, shape) -> torch.Tensor:
        """(nsteps, *shape) standard normals: exactly what denoise_loop(noise_seed=seed) adds at steps step0 .. step0 + nsteps - 1."""
        n = int(np.prod(shape))
        out = torch.empty((nsteps,) + tuple(shape), device=self.device, dtype=torch.float32)
        self._go("said_philox_normal", int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), int(nsteps), n, _ptr(out))
        return out

    # ---- debugging aids (tests only) ----
    def debug_option(self, name: str, value: int) -> None:
        self._call("said_debug_option", name.encode(), int(value))

    def debug_get(self, name: str) -> int:
        return int(self.lib.said_debug_get(self.h, name.encode()))

    def debug_stop_after(self, n: int):
        self._call("said_debug_stop_after", int(n))

    def debug_clocks(self, enable: bool, read: bool = False):
        out = np.zeros((64, 8, 16), dtype=np.int64) if read else None
        self._call("said_debug_clocks", int(enable), _vp(out))
        return out

    def debug_read(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape, dtype=np.float32)
        self._call("said_debug_read", name.encode(), _vp(out), out.size)
        return out

    def ws_buffers(self):
        """[(index, name, bytes)] of the context's workspace buffers (said_debug_ws_info)."""
        out = []
        for i in range(int(self.lib.said_debug_ws_count(self.h))):
            p, nb, nm = c_void_p(), _c_ll(0), c_char_p()
            self._call("said_debug_ws_info", i, ctypes.byref(p), ctypes.byref(nb), ctypes.byref(nm))
            out.append((i, (nm.value or b"?").decode(), int(nb.value)))
        return out

    def ws_fill(self, byte_value: int) -> None:
        self._call("said_debug_ws_fill", int(byte_value) & 0xFF)

    def ws_snapshot(self, idx: int, nbytes: int) -> torch.Tensor:
        """Device copy (uint8) of workspace buffer `idx`, enqueued on the current stream."""
        out = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._go("said_debug_ws_copy", idx, _ptr(out), nbytes)
        return out

    def audio_snapshot(self, name: str, nbytes: int) -> torch.Tensor:
        """Device copy (uint8) of the first `nbytes` bytes of the audio encoder's buffer `name` (said_debug_audio_copy), enqueued on the current stream."""
        out = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._go("said_debug_audio_copy", name.encode(), _ptr(out), nbytes)
        return out

    def audio_fill(self, byte_value: int) -> None:
        """Every byte of every allocated audio-encoder buffer set to `byte_value` (said_debug_audio_fill); synchronises the device."""
        self._call("said_debug_audio_fill", int(byte_value) & 0xFF)

    def loop_progress(self) -> int:
        """Denoise steps started so far by the loop running (or last run) on this context; never blocks the loop's stream."""
        v = c_int(0)
        if self.lib.said_loop_progress(self.h, ctypes.byref(v)) != 0:   # (the entry does not record an error text: it runs beside the loop's thread)
            raise EngineError("said_loop_progress failed")
        return v.value

    def loop_progress_reset(self) -> None:
        """Forget the previous loop's step count before a polling thread is started."""
        self._call("said_loop_progress_reset")

    def graph_num_nodes(self) -> int:
        return int(self.lib.said_graph_num_nodes(self.h))

    def set_precision(self, mode) -> None:
        """"fp32" (split-fp16 products), "fp32_strict" (fp32 matrix instructions) or "bf16"; see said_set_precision.  (True / False: "bf16" / "fp32".)"""
        if isinstance(mode, str):
            if mode not in PRECISIONS:
                raise EngineError(f"unknown precision mode {mode!r}: one of {sorted(PRECISIONS)}")
            mode = PRECISIONS[mode]
        else:
            mode = 1 if mode else 0
        self._call("said_set_precision", int(mode))

    def get_precision(self) -> str:
        """The mode asked for."""
        return {v: k for k, v in PRECISIONS.items()}[int(self.lib.said_get_precision(self.h))]

    def effective_precision(self) -> str:
        """The mode that runs: "fp32" becomes "fp32_strict" when a weight tensor lies outside the split-fp16 range (precision_note() says which)."""
        return {v: k for k, v in PRECISIONS.items()}[int(self.lib.said_effective_precision(self.h))]

    def precision_note(self) -> str:
        return (self.lib.said_precision_note(self.h) or b"").decode()

    def numeric_status(self):
        """(first_bad_step, result_nonfinite) of the last loop / forward call on this context: the index of the first denoise step whose model output
        held an inf / NaN (-1: none) and whether the final latents / the model output hold one.  Synchronises the current stream."""
        a, b = c_int(-1), c_int(0)
        with torch.cuda.device(self.index):
            self._call("said_numeric_status", _stream(), ctypes.byref(a), ctypes.byref(b))
        return a.value, bool(b.value)


class VaeEngine(_Context):
    """BCVAE context on one GPU (include/said_hip.h, "VAE"): the encoder always, the decoder when its weights were loaded."""
    prefix = "said_vae"

    def __init__(self, device: torch.device, in_channels: int = 32, seq_len: int = 120, z_dim: int = 64):
        super().__init__(device)
        self.seq_len, self.in_channels, self.z_dim = seq_len, in_channels, z_dim
        self._create(in_channels, seq_len, z_dim)

    def load_weights(self, state_dict: Dict[str, torch.Tensor]):
        for k, v in state_dict.items():
            if k.endswith("num_batches_tracked"):
                continue   # a counter, not a weight
            a = _f32(v.detach().to("cpu", torch.float32).numpy())
            shape = (_c_ll * max(a.ndim, 1))(*(a.shape if a.ndim else (1,)))
            self._call("said_vae_set_weight", k.encode(), _vp(a), shape, max(a.ndim, 1), what=f"said_vae_set_weight({k})")
        self._call("said_vae_finalize_weights")

    def encode(self, coeffs: torch.Tensor, n_windows: int, window_stride: int, want_logvar: bool = True):
        """`coeffs`: contiguous fp32 device tensor holding the windows at `window_stride` floats apart."""
        coeffs = _dev(coeffs, "coeffs", index=self.index)
        need = (n_windows - 1) * window_stride + self.seq_len * self.in_channels if n_windows > 0 else 0
        if coeffs.numel() < need:
            raise EngineError(f"coeffs holds {coeffs.numel()} floats, {n_windows} windows at stride {window_stride} need {need}")
        mean = torch.empty(n_windows, self.z_dim, device=coeffs.device, dtype=torch.float32)
        logvar = torch.empty_like(mean) if want_logvar else None
        self._go("said_vae_encode", _ptr(coeffs), int(window_stride), int(n_windows), _ptr(mean), _ptr(logvar))
        return mean, logvar

    @property
    def has_decoder(self) -> bool:
        return bool(load_library("vae_decoder").said_vae_has_decoder(self.h))

    def decode(self, mean: torch.Tensor, log_var: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(n, z_dim) latents -> (n, seq_len, in_channels) coefficients.  With `eps`, the latent is mean + exp(0.5 log_var) eps,
        computed in the decoder launch's prologue."""
        load_library("vae_decoder")
        z = self.z_dim
        if eps is not None and log_var is None:
            raise ValueError("eps needs log_var")
        args = {"mean": mean, "log_var": log_var, "eps": eps}
        for k, t in args.items():
            if t is None:
                continue
            if t.dim() != 2 or t.shape[1] != z or t.shape[0] != mean.shape[0]:
                raise ValueError(f"{k} must be (n, {z}) like mean {tuple(mean.shape)}, got {tuple(t.shape)}")
            args[k] = _dev(t, k, index=self.index)
        n = int(mean.shape[0])
        out = torch.empty(n, self.seq_len, self.in_channels, device=self.device if n == 0 else args["mean"].device, dtype=torch.float32)
        if n == 0:
            return out
        lv = args["log_var"] if eps is not None else None
        self._go("said_vae_decode", _ptr(args["mean"]), _ptr(lv), _ptr(args["eps"]), n, _ptr(out))
        return out


def unet_algorithmic_bytes(batch_eff: int, frames: int, bytes_per_elem: int = 4) -> float:
    return float(load_library().said_unet_algorithmic_bytes(batch_eff, frames, bytes_per_elem))


def unet_algorithmic_flops(batch_eff: int, frames: int) -> float:
    return float(load_library().said_unet_algorithmic_flops(batch_eff, frames))


class MetricsEngine(_Context):
    """said_metrics context on one GPU (include/said_metrics.h): workspace for up to `max_points` (n, 64) fp32 latents."""
    prefix, group = "said_metrics", "metrics"
    cpu_error, cpu_message = NoCpuPathError, "said_amd computes the metrics on MI355X only (device={}); there is no CPU path"

    def __init__(self, device: torch.device, max_points: int):
        super().__init__(device)
        self._create(int(max_points))
        self.max_points = int(max_points)

    def _x(self, x: torch.Tensor) -> torch.Tensor:
        x = _dev(x, "latents", index=self.index, trailing=(METRICS_DIM,), strict=True)
        if x.shape[0] > self.max_points:
            raise EngineError(f"{x.shape[0]} latents exceed this context's max_points {self.max_points}")
        return x

    def weighted_sums(self, x: torch.Tensor, k: int, wsrc: int):
        """(n_k (k,), sum r x (k, 64)) in float64."""
        x = self._x(x)
        nk, sx = np.zeros(k), np.zeros((k, METRICS_DIM))
        self._go("said_metrics_weighted_sums", _ptr(x), x.shape[0], k, wsrc, _dp(nk), _dp(sx))
        return nk, sx

    def weighted_scatter(self, x: torch.Tensor, k: int, wsrc: int, means: np.ndarray) -> np.ndarray:
        """sum r (x - mu_k)(x - mu_k)^T, (k, 64, 64) float64."""
        x = self._x(x)
        mu = _f64(means).reshape(k, METRICS_DIM)
        out = np.zeros((k, METRICS_DIM, METRICS_DIM))
        self._go("said_metrics_weighted_scatter", _ptr(x), x.shape[0], k, wsrc, _dp(mu), _dp(out))
        return out

    def gmm_estep(self, x: torch.Tensor, prec_chol: np.ndarray, mean_prec: np.ndarray, log_det: np.ndarray, log_weights: np.ndarray,
                  want_resp: bool = False):
        """Mean log_prob_norm (the lower bound); with want_resp also the (n, k) log-responsibilities and (n,) log_prob_norm, float64 device tensors."""
        x = self._x(x)
        k = prec_chol.shape[0]
        args = [_f64(a) for a in (prec_chol, mean_prec, log_det, log_weights)]
        lb = np.zeros(1)
        lr = lpn = None
        if want_resp:
            lr = torch.empty(x.shape[0], k, dtype=torch.float64, device=x.device)
            lpn = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
        self._go("said_metrics_gmm_estep", _ptr(x), x.shape[0], k, *[_dp(a) for a in args], _dp(lb), _ptr(lr), _ptr(lpn))
        return (float(lb[0]), lr, lpn) if want_resp else float(lb[0])

    def kmeans_assign(self, x: torch.Tensor, centres: np.ndarray, compare: bool):
        """(labels changed since the previous assignment (n when not compared), inertia)."""
        x = self._x(x)
        c = _f64(centres)
        changed, inertia = _c_ll(0), np.zeros(1)
        self._go("said_metrics_kmeans_assign", _ptr(x), x.shape[0], c.shape[0], _dp(c), int(bool(compare)), ctypes.byref(changed), _dp(inertia))
        return int(changed.value), float(inertia[0])

    def kmeans_read(self, n: int):
        """(labels int32 (n,), squared distance to the assigned centre float64 (n,)) of the last assignment."""
        lab, dist = np.zeros(n, dtype=np.int32), np.zeros(n)
        self._go("said_metrics_kmeans_read", n, _ip(lab), _dp(dist))
        return lab, dist

    def kmeans_set_labels(self, labels: np.ndarray, k: int):
        lab = _i32(labels)
        self._go("said_metrics_kmeans_set_labels", lab.shape[0], k, _ip(lab))

    def kmeanspp_first(self, x: torch.Tensor, centre_id: int) -> float:
        x = self._x(x)
        pot = np.zeros(1)
        self._go("said_metrics_kmeanspp_first", _ptr(x), x.shape[0], int(centre_id), _dp(pot))
        return float(pot[0])

    def kmeanspp_step(self, x: torch.Tensor, rand_vals: np.ndarray):
        """(chosen point index, its potential) for candidate values rand_vals (uniform * current potential)."""
        x = self._x(x)
        r = _f64(rand_vals)
        cid, pot = _c_ll(0), np.zeros(1)
        self._go("said_metrics_kmeanspp_step", _ptr(x), x.shape[0], _dp(r), r.shape[0], ctypes.byref(cid), _dp(pot))
        return int(cid.value), float(pot[0])


class OptimizeEngine(_Context):
    """said_optimize context on one GPU (include/said_optimize.h): the bases of a batch, the rhs kernel and the batched QP solver."""
    prefix, group = "said_optimize", "optimize"
    cpu_error, cpu_message = NoCpuPathError, "said_amd fits blendshape coefficients on MI355X only (device={}); there is no CPU path"

    def __init__(self, device: torch.device):
        super().__init__(device)
        self._create()
        self.k = 0
        self.n3v = 0
        self.nbasis = 0

    def set_bases(self, neutrals: np.ndarray, bdeltas: np.ndarray, ps: np.ndarray):
        """neutrals (nb, 3V), bdeltas (nb, 3V, K) = B - n, ps (nb, K, K) = B_delta' B_delta, float64."""
        n, b, p = _f64(neutrals), _f64(bdeltas), _f64(ps)
        nb, n3v, k = b.shape
        self._go("said_optimize_set_bases", nb, k, n3v, _dp(n), _dp(b), _dp(p))
        self.nbasis, self.n3v, self.k = nb, n3v, k

    def rhs(self, basis: int, verts: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """q (frames, K) float64 device tensor for verts, a contiguous (frames, 3V) float64 device tensor."""
        _dev(verts, "vertices", torch.float64, trailing=(self.n3v,), strict=True)
        if out is None:
            out = torch.empty(verts.shape[0], self.k, dtype=torch.float64, device=verts.device)
        self._go("said_optimize_rhs", int(basis), _ptr(verts), verts.shape[0], _ptr(out))
        return out

    def solve(self, q: torch.Tensor, offsets: np.ndarray, basis: np.ndarray, delta: float, coupled: bool, max_iter: int, tol: float,
              want_duals: bool = False):
        """(w (frames, K), z (frames, 4, K) or None, status, iters, resid (nseq, 3)); w and z float64 device tensors."""
        _dev(q, "q", torch.float64, trailing=(self.k,), strict=True)
        offs, bas = _i64(offsets), _i32(basis)
        nseq = bas.shape[0]
        if offs.shape != (nseq + 1,) or offs[-1] != q.shape[0]:
            raise EngineError(f"offsets must have nseq + 1 = {nseq + 1} entries ending at the {q.shape[0]} frames of q")
        w = torch.empty_like(q)
        z = torch.empty(q.shape[0], 4, self.k, dtype=torch.float64, device=q.device) if want_duals else None
        st, it = np.zeros(nseq, dtype=np.int32), np.zeros(nseq, dtype=np.int32)
        res = np.zeros((nseq, 3))
        self._go("said_optimize_solve", nseq, _lp(offs), _ip(bas), _ptr(q), float(delta), int(bool(coupled)), int(max_iter), float(tol), _ptr(w),
                 _ptr(z), _ip(st), _ip(it), _dp(res))
        return w, z, st, it, res


class _TrainContext(_Context):
    """What the two trainer contexts bind alike (<prefix>_set_tensor, _get_tensor, _reset_optimizer, _apply_update, _read_losses,
    _last_losses); a subclass names how many values its _last_losses gives and the pointer helper of the type its tensor entries are bound with."""
    n_last, _tensor_ptr = 0, staticmethod(_fp)

    @staticmethod
    def _dtype(name: str):
        """The element type of tensor `name` on the host."""
        return np.float32

    def set_tensor(self, which: int, name: str, value) -> None:
        a = np.ascontiguousarray(value, dtype=self._dtype(name)).reshape(-1)
        self._call(self.prefix + "_set_tensor", which, name.encode(), self._tensor_ptr(a), a.size)

    def get_tensor(self, which: int, name: str, numel: int) -> np.ndarray:
        a = np.empty(numel, dtype=self._dtype(name))
        self._call(self.prefix + "_get_tensor", which, name.encode(), self._tensor_ptr(a), numel)
        return a

    def reset_optimizer(self) -> None:
        self._call(self.prefix + "_reset_optimizer")

    def apply_update(self, scalars: np.ndarray) -> None:
        self._call(self.prefix + "_apply_update", _fp(_f32(scalars)))

    def read_losses(self, val: bool, reset: bool = True):
        acc = np.zeros(TRAIN_NACC, dtype=np.float64)   # SAID_UT_NACC is the same
        st = c_int(0)
        self._call(self.prefix + "_read_losses", int(bool(val)), _dp(acc), ctypes.byref(st), int(bool(reset)))
        return acc, int(st.value)

    def last_losses(self) -> np.ndarray:
        out = np.zeros(self.n_last, dtype=np.float32)
        self._call(self.prefix + "_last_losses", _fp(out))
        return out


class TrainEngine(_TrainContext):
    """said_train context on one GPU (include/said_train.h): the BCVAE's parameters, buffers, gradients, Adam moments and EMA shadow, the
    window sets, and the captured training step.  Host arrays in and out (numpy); the context keeps its own stream."""
    prefix, group, n_last = "said_train", "train", 4   # last_losses: reconst, regularize, velocity, total
    cpu_error, cpu_message = NoCpuPathError, "said_amd trains the BCVAE on MI355X only (device={}); there is no CPU path"
    _tensor_ptr = staticmethod(_vp)   # float32, or the int64 of a num_batches_tracked

    def __init__(self, device: torch.device, max_batch: int):
        super().__init__(device)
        self._create(int(max_batch))
        self.max_batch = int(max_batch)
        self.tensors = [(self.lib.said_train_tensor_name(i).decode(), int(self.lib.said_train_tensor_numel(i)),
                         bool(self.lib.said_train_tensor_is_counter(i))) for i in range(70)]

    @staticmethod
    def _dtype(name: str):
        return np.int64 if name.endswith("num_batches_tracked") else np.float32

    def set_data(self, which_set: int, frames: np.ndarray, offsets: np.ndarray, lengths: np.ndarray, mirror: np.ndarray) -> None:
        fr, off, ln, mi = _f32(frames), _i64(offsets), _i32(lengths), _i32(mirror)
        self._call("said_train_set_data", which_set, _fp(fr), fr.shape[0], _lp(off), _ip(ln), ln.size, _ip(mi))

    def gather(self, which_set: int, items: np.ndarray) -> np.ndarray:
        it = _i32(items)
        x = np.empty((it.shape[0], 120, 32), dtype=np.float32)
        self._call("said_train_gather", which_set, it.shape[0], _ip(it), _fp(x))
        return x

    def step(self, items: np.ndarray, eps: np.ndarray, scalars: np.ndarray, std: Optional[np.ndarray], use_graph: bool = True) -> None:
        it, ep, sc, sd = _i32(items), _f32(eps), _f32(scalars), _f32(std)
        self._call("said_train_step", it.shape[0], _ip(it), _fp(ep), _fp(sc), _fp(sd), int(bool(use_graph)))

    def eval_loss(self, which_set: int, items: np.ndarray, eps: np.ndarray, scalars: np.ndarray, std: Optional[np.ndarray], ema: bool) -> None:
        it, ep, sc, sd = _i32(items), _f32(eps), _f32(scalars), _f32(std)
        self._call("said_train_eval_loss", which_set, it.shape[0], _ip(it), _fp(ep), _fp(sc), _fp(sd), int(bool(ema)))

    def bn_stats(self, bn: int, channels: int) -> np.ndarray:
        out = np.zeros(2 * channels, dtype=np.float32)
        self._call("said_train_bn_stats", bn, _fp(out))
        return out.reshape(2, channels)

    def graph_count(self) -> int:
        return int(self.lib.said_train_graph_count(self.h))


ENCODER_PRODUCTS = ("fp32", "split_fp16")   # a mode's index is its SAID_UT_PRODUCTS_* value


class UNetTrainEngine(_TrainContext):
    """said_unet_train context on one GPU (include/said_unet_train.h): the denoiser's parameters, gradients, Adam moments and EMA shadow, and
    the training step.  Host arrays in and out (numpy); the audio embedding may be a device tensor.  The context keeps its own stream."""
    prefix, group, n_last = "said_unet_train", "unet_train", 6   # last_losses: predict, velocity, vertex, total, clip factor, gradient norm
    cpu_error, cpu_message = NoCpuPathError, "said_amd trains the denoiser on MI355X only (device={}); there is no CPU path"

    def __init__(self, device: torch.device, max_batch: int, max_frames: int, feature_dim: Optional[int] = -1, finetune_layers: int = 0):
        super().__init__(device)
        self.finetune_layers = max(int(finetune_layers), 0)
        if self.finetune_layers > 0:   # the Wav2Vec2 transformer trains with the denoiser: the batch's input is the conv features
            load_library("unet_finetune")
            self._create(int(max_batch), int(max_frames), -1 if feature_dim is None else int(feature_dim), self.finetune_layers,
                         entry="said_unet_train_create_ft")
        elif feature_dim is None:   # the entry point without a feature_dim: the default context, as feature_dim=-1 is
            self._create(int(max_batch), int(max_frames))
        else:
            self._create(int(max_batch), int(max_frames), int(feature_dim), entry="said_unet_train_create_dim")
        self.max_batch, self.max_frames = int(max_batch), int(max_frames)
        self.feature_dim = int(self.lib.said_unet_train_feature_dim(self.h))   # -1: no audio_proj_layer
        self.tensors = [(self.lib.said_unet_train_context_tensor_name(self.h, i).decode(), int(self.lib.said_unet_train_context_tensor_numel(self.h, i)))
                        for i in range(self.lib.said_unet_train_num_tensors(self.h))]

    def copy(self, dst: int, src: int) -> None:
        self._call("said_unet_train_copy", dst, src)

    # ---- the arithmetic of the fine-tuned encoder's dense products (said_amd/csrc/said_unet_train_products.h)
    def set_encoder_products(self, mode: str) -> None:
        """"fp32" or "split_fp16", from the next call on; refused on a context without a fine-tuned encoder."""
        if mode not in ENCODER_PRODUCTS:
            raise ValueError(f"encoder_products must be one of {sorted(ENCODER_PRODUCTS)}, got {mode!r}")
        load_library("unet_products")
        self._call("said_unet_train_set_encoder_products", ENCODER_PRODUCTS.index(mode))

    def encoder_products(self) -> str:
        load_library("unet_products")
        return ENCODER_PRODUCTS[int(self.lib.said_unet_train_encoder_products(self.h))]

    def dense_product(self, layout: str, a, b, bias=None, res=None, out=None, mode: str = "fp32") -> np.ndarray:
        """One dense product of a linear layer with weight W (n, k), by the route the encoder's products take in `mode`:
        "forward": a = x (rows, k), b = W -> x W^T + bias (+ res) (+ out);  "dgrad": a = dy (rows, n), b = W -> dy W (+ out);
        "wgrad": a = dy (rows, n), b = x (rows, k) -> dy^T x.  `out`: the destination's value before the call, added to."""
        load_library("unet_products")
        a, b, bias, res = _f32(a), _f32(b), _f32(bias), _f32(res)
        rows = a.shape[0]
        if layout == "forward":
            n, k, shape = b.shape[0], b.shape[1], (rows, b.shape[0])
        elif layout == "dgrad":
            n, k, shape = b.shape[0], b.shape[1], (rows, b.shape[1])
        elif layout == "wgrad":
            n, k, shape = a.shape[1], b.shape[1], (a.shape[1], b.shape[1])
        else:
            raise ValueError(f"layout must be forward, dgrad or wgrad, got {layout!r}")
        want_a, want_b = ((rows, k), (n, k)) if layout == "forward" else ((rows, n), (n, k)) if layout == "dgrad" else ((rows, n), (rows, k))
        if a.shape != want_a or b.shape != want_b or (bias is not None and bias.shape != (n,)) or (res is not None and res.shape != shape) \
                or (out is not None and tuple(np.shape(out)) != shape):
            raise EngineError(f"dense_product {layout}: a {a.shape}, b {b.shape}, bias {None if bias is None else bias.shape}, "
                              f"res {None if res is None else res.shape}, out {None if out is None else np.shape(out)}")
        y = np.empty(shape, dtype=np.float32) if out is None else np.array(out, dtype=np.float32, order="C")
        self._call("said_unet_train_dense_product", ("forward", "dgrad", "wgrad").index(layout), rows, n, k, _fp(a), _fp(b), _fp(bias), _fp(res),
                   int(out is not None), ENCODER_PRODUCTS.index(mode), _fp(y))
        return y

    def set_alphas(self, alphas_cumprod) -> None:
        a = _f32(alphas_cumprod).reshape(-1)
        self._call("said_unet_train_set_alphas", _fp(a), a.size)

    def _batch(self, x, timesteps, cond, audio):
        """(B, T, x, timesteps, cond, the audio embedding, its pointer, whether that is a device pointer) of a batch, as arrays of the bound types."""
        x = _f32(x)
        B, T = x.shape[0], x.shape[1]
        ts = _i64(timesteps).reshape(-1)
        cd = _i32(np.asarray(cond).astype(np.int32)).reshape(-1)
        if isinstance(audio, torch.Tensor) and audio.is_cuda:
            au = _dev(audio, "audio_embedding")
            torch.cuda.current_stream(au.device).synchronize()   # the context copies it on its own stream
            ap, on_dev = _ptr(au), 1
        else:
            au = host_f32(audio)
            ap, on_dev = _vp(au), 0
        width = 512 if self.finetune_layers > 0 else 768
        if x.shape != (B, T, 32) or ts.size != B or cd.size != B or tuple(au.shape) != (B, T, width):
            raise EngineError(f"batch shapes: x {x.shape}, timesteps {ts.shape}, cond {cd.shape}, "
                              f"{'features' if self.finetune_layers > 0 else 'audio embedding'} {tuple(au.shape)}")
        return B, T, x, ts, cd, au, ap, on_dev

    def _audio_params(self, draws, cfg, B: int, T: int):
        """(pointer to said_audio_train_params or None, what it must keep alive) for the _ft entry points; draws None: eval mode."""
        if draws is None:
            return None, None
        cfg.check()
        p, mask = audio_train_params(draws, cfg, B, T, self.device)
        if mask is not None:
            torch.cuda.current_stream(self.device).synchronize()   # the context copies the mask on its own stream
        return ctypes.byref(p), (p, mask)

    def step(self, coeffs, noise, timesteps, cond, audio, dropout_seed: int, scalars, std=None, deltas=None, audio_draws=None, audio_cfg=None) -> None:
        """`audio`: the audio embedding (B, T, 768), or with finetune_layers > 0 the conv features (B, T, 512); there audio_draws /
        audio_cfg (AudioTrainDraws / AudioTrainConfig) put the encoder in train mode, None leaves it in eval mode."""
        B, T, x, ts, cd, au, ap, on_dev = self._batch(coeffs, timesteps, cond, audio)
        nz, sc, sd, dl = _f32(noise), _f32(scalars), _f32(std), _f32(deltas)
        V = 0 if dl is None else dl.shape[-1] // 3
        if self.finetune_layers > 0:
            pp, keep = self._audio_params(audio_draws, audio_cfg, B, T)
            self._call("said_unet_train_step_ft", B, T, _fp(x), _fp(nz), _lp(ts), _ip(cd), ap, on_dev, pp, _c_ull(int(dropout_seed) & (2 ** 64 - 1)),
                       _fp(sc), _fp(sd), _fp(dl), V)
            return
        self._call("said_unet_train_step", B, T, _fp(x), _fp(nz), _lp(ts), _ip(cd), ap, on_dev, _c_ull(int(dropout_seed) & (2 ** 64 - 1)), _fp(sc),
                   _fp(sd), _fp(dl), V)

    def eval_loss(self, coeffs, noise, timesteps, cond, audio, scalars, std=None, deltas=None, ema: bool = False) -> None:
        B, T, x, ts, cd, au, ap, on_dev = self._batch(coeffs, timesteps, cond, audio)
        nz, sc, sd, dl = _f32(noise), _f32(scalars), _f32(std), _f32(deltas)
        V = 0 if dl is None else dl.shape[-1] // 3
        if self.finetune_layers > 0:
            self._call("said_unet_train_eval_loss_ft", B, T, _fp(x), _fp(nz), _lp(ts), _ip(cd), ap, on_dev, None, _fp(sc), _fp(sd), _fp(dl), V,
                       int(bool(ema)))
            return
        self._call("said_unet_train_eval_loss", B, T, _fp(x), _fp(nz), _lp(ts), _ip(cd), ap, on_dev, _fp(sc), _fp(sd), _fp(dl), V, int(bool(ema)))

    def forward_only(self, sample, timesteps, cond, audio, ema: bool = False) -> np.ndarray:
        B, T, x, ts, cd, au, ap, on_dev = self._batch(sample, timesteps, cond, audio)
        out = np.empty((B, T, 32), dtype=np.float32)
        if self.finetune_layers > 0:
            self._call("said_unet_train_forward_only_ft", B, T, _fp(x), _lp(ts), _ip(cd), ap, on_dev, None, int(bool(ema)), _fp(out))
        else:
            self._call("said_unet_train_forward_only", B, T, _fp(x), _lp(ts), _ip(cd), ap, on_dev, int(bool(ema)), _fp(out))
        return out

    def last_conditioning(self, B: int, T: int) -> np.ndarray:
        """(B, T, context width): what the denoiser saw in the last call of that shape on a fine-tuning context."""
        out = np.empty((B, T, self.feature_dim if self.feature_dim > 0 else 768), dtype=np.float32)
        self._call("said_unet_train_last_conditioning", B, T, _fp(out))
        return out


class RenderEngine(_Context):
    """said_render context on one GPU (include/said_render.h): a mesh with its blendshape basis, a scene, and the four kernels of a chunk."""
    prefix, group = "said_render", "render"
    cpu_error, cpu_message = NoCpuPathError, "said_amd renders on MI355X only (device={}); there is no CPU path"

    def __init__(self, device: torch.device):
        super().__init__(device)
        self._create()
        self.nv = self.nf = self.k = 0
        self.width = self.height = 0

    def set_mesh(self, neutral: np.ndarray, faces: np.ndarray, blendshapes_matrix: np.ndarray) -> None:
        """neutral (V, 3), faces (F, 3) vertex indices, blendshapes_matrix (3V, K) = [b_1 | ... | b_K] (not deltas)."""
        n = _f64(neutral).reshape(-1, 3)
        fa = np.asarray(faces)
        if fa.ndim != 2 or fa.shape[1] != 3 or fa.dtype.kind not in "iu":
            raise EngineError(f"faces must be an (F, 3) integer array, got {fa.shape} {fa.dtype}")
        if fa.size and (fa.min() < -2**31 or fa.max() >= 2**31):
            raise EngineError("faces hold indices outside int32")
        fa = _i32(fa)
        b = _f64(blendshapes_matrix)
        if b.ndim != 2 or b.shape[0] != n.size:
            raise EngineError(f"blendshapes_matrix must be (3V, K) = ({n.size}, K), got {b.shape}")
        self.nv = self.nf = self.k = 0
        self._go("said_render_set_mesh", n.shape[0], fa.shape[0], b.shape[1], _dp(n), _ip(fa), _dp(b))
        self.nv, self.nf, self.k = n.shape[0], fa.shape[0], b.shape[1]

    def set_scene(self, scene: RenderScene) -> None:
        self._call("said_render_set_scene", ctypes.byref(scene))
        self.width, self.height = int(scene.width), int(scene.height)

    def set_colormap(self, lut: np.ndarray) -> None:
        """lut (256, 3) RGB in [0, 1]."""
        a = _f32(lut)
        if a.shape != (RENDER_LUT, 3):
            raise EngineError(f"the colour table must be ({RENDER_LUT}, 3), got {a.shape}")
        self._go("said_render_set_colormap", _fp(a))

    def render(self, coeffs: torch.Tensor, t0: int, n_frames: int, out: torch.Tensor, target: Optional[torch.Tensor] = None, max_diff: float = 0.001,
               rot=None, t_center=None, face_ids: Optional[torch.Tensor] = None, samples: int = 1, sample_ids: Optional[torch.Tensor] = None) -> None:
        """Frames [t0, t0 + n_frames) of coeffs (T, K) into out, a contiguous (>= n_frames, H, W, 3) uint8 device tensor, B G R; enqueued on the
        current stream.  face_ids: a contiguous (>= n_frames, H, W) int32 device tensor that receives the face drawn at each pixel (-1: none).
        samples: 1, or 4 for the multisampled render of include/said_render_ms.h, which takes no face_ids and fills sample_ids instead, a
        contiguous (>= n_frames, H, W, 4) int32 device tensor: the face of each of a pixel's four samples."""
        if self.nf == 0:
            raise EngineError(("said_render_render" if samples == 1 and sample_ids is None else "said_render_render_ms") + ": no mesh set (set_mesh)")
        coeffs = _dev(coeffs, "blendshape_coeffs", index=self.index)
        if coeffs.dim() != 2 or coeffs.shape[1] != self.k:
            raise EngineError(f"blendshape_coeffs must be (T, {self.k}), got {tuple(coeffs.shape)}")
        if t0 < 0 or n_frames < 1 or t0 + n_frames > coeffs.shape[0]:
            raise EngineError(f"frames [{t0}, {t0 + n_frames}) lie outside the {coeffs.shape[0]} frames of blendshape_coeffs")
        if target is not None:
            target = _dev(target, "target_blendshape_coeffs")
            if target.shape != coeffs.shape:
                raise EngineError(f"target_blendshape_coeffs must have the shape of blendshape_coeffs {tuple(coeffs.shape)}, got {tuple(target.shape)}")
        need = n_frames * self.height * self.width   # room for n_frames frames of height x width
        for t, name, dt, per in ((out, "out", torch.uint8, 3), (face_ids, "face_ids", torch.int32, 1), (sample_ids, "sample_ids", torch.int32, 4)):
            if t is not None:
                _dev(t, name, dt, self.index, numel=need * per, strict=True)
        r, c = (None if a is None else _f64(a).reshape(3) for a in (rot, t_center))
        if samples == 1 and sample_ids is None:
            self._go("said_render_render", _ptr(coeffs), _ptr(target), int(t0), int(n_frames), float(max_diff), _dp(r), _dp(c), _ptr(out), _ptr(face_ids))
        else:   # what goes with which sample count is said_render_render_ms's to refuse
            load_library("render_ms")
            self._go("said_render_render_ms", int(samples), _ptr(coeffs), _ptr(target), int(t0), int(n_frames), float(max_diff), _dp(r), _dp(c),
                     _ptr(out), _ptr(face_ids), _ptr(sample_ids))
        self._keep = (coeffs, target)   # alive until the next call: the kernels may still be reading them

    def _read(self, name: str, n_frames: int) -> np.ndarray:
        out = np.empty((n_frames, self.nv, 3), dtype=np.float32)
        self._go(name, int(n_frames), _fp(out))
        return out

    def read_vertices(self, n_frames: int) -> np.ndarray:
        """(n_frames, V, 3) vertices of the last render's chunk, before the rotation."""
        return self._read("said_render_read_vertices", n_frames)

    def read_normals(self, n_frames: int) -> np.ndarray:
        return self._read("said_render_read_normals", n_frames)

    def read_colors(self, n_frames: int) -> np.ndarray:
        """(n_frames, V, 3) difference colours (R, G, B) of the last render's chunk."""
        return self._read("said_render_read_colors", n_frames)


class JpegEngine(_Context):
    """said_jpeg context on one GPU (include/said_jpeg.h): (n, H, W, 3) uint8 device frames -> one baseline JFIF scan per frame, back to back
    in one device buffer."""
    prefix, group = "said_jpeg", "jpeg"
    cpu_error, cpu_message = NoCpuPathError, "said_amd encodes JPEG on MI355X only (device={}); there is no CPU path (PIL is the host encoder)"

    def __init__(self, device: torch.device, width: int, height: int, quality: int = 90):
        super().__init__(device)
        self._create()
        self.configure(width, height, quality)

    def configure(self, width: int, height: int, quality: int) -> None:
        self.width = self.height = self.quality = self.blocks = 0   # nothing is configured until every call below has succeeded
        self.header = b""
        with torch.cuda.device(self.index):
            self._call("said_jpeg_configure", int(width), int(height), int(quality))
        self.width, self.height, self.quality = int(width), int(height), int(quality)
        self.blocks = ((self.width + 15) // 16) * ((self.height + 15) // 16) * 6
        buf, size = ctypes.create_string_buffer(1024), _c_ll(0)
        self._call("said_jpeg_header", buf, 1024, ctypes.byref(size))
        self.header = buf.raw[:size.value]   # SOI .. SOS: the same for every frame

    def encode(self, frames: torch.Tensor, n_frames: int, out: Optional[torch.Tensor], offsets: torch.Tensor, bgr: bool = True,
               capacity: Optional[int] = None):
        """The first n_frames of frames, a contiguous (>= n_frames, H, W, 3) uint8 device tensor, into out (uint8, device): each frame's scan and
        EOI, back to back; offsets, a contiguous int64 device tensor of at least n_frames + 1 elements, receives where each starts and the
        total.  `capacity` (default: all of out) bounds what may be written.  Returns (fits, bytes required); synchronises the current stream."""
        if n_frames < 1:
            raise EngineError(f"n_frames must be at least 1, got {n_frames}")
        _dev(frames, "frames", torch.uint8, self.index, numel=n_frames * self.height * self.width * 3, strict=True)   # n_frames of height x width x 3
        _dev(offsets, "offsets", torch.int64, self.index, numel=n_frames + 1, strict=True)
        if out is not None:
            _dev(out, "out", torch.uint8, self.index, strict=True)
        room = 0 if out is None else out.numel()
        cap = room if capacity is None else int(capacity)
        if cap < 0 or cap > room:
            raise EngineError(f"capacity {cap} lies outside the {room} bytes of out")
        required = _c_ll(0)
        with torch.cuda.device(self.index):   # (1, SAID_JPEG_OVERFLOW, is an answer, not an error: no _go)
            rc = self.lib.said_jpeg_encode(self.h, _ptr(frames), int(n_frames), 1 if bgr else 0, _ptr(out), cap, _ptr(offsets), ctypes.byref(required), _stream())
        if rc not in (0, JPEG_OVERFLOW):
            raise EngineError("said_jpeg_encode: " + self._last_error(self.h))
        return rc == 0, int(required.value)

    def read_coefficients(self, n_frames: int) -> np.ndarray:
        """(n_frames, blocks, 64) int16: the last encode's quantised coefficients, blocks in scan order, each in zigzag order."""
        out = np.empty((n_frames, self.blocks, 64), dtype=np.int16)
        self._go("said_jpeg_read_coefficients", int(n_frames), _vp(out))
        return out


class BeatEngine(_Context):
    """said_beat context on one GPU (include/said_beat.h): onsets of audio clips, change-rate minima of coefficient
    sequences, the beat-consistency score of each sequence, and the vertex error of (real, generated) pairs; all in float64."""
    prefix, group = "said_beat", "beat"
    cpu_error, cpu_message = NoCpuPathError, "said_amd computes beat consistency and vertex error on MI355X only (device={}); there is no CPU path"

    def __init__(self, device: torch.device, sampling_rate: Optional[int] = None):
        super().__init__(device)
        self._create()
        self.sampling_rate, self.peak_pick = 0, None
        self.frame_start = self.seq_off = self.delta_shape = None
        if sampling_rate is not None:
            self.set_sampling_rate(sampling_rate)

    def set_sampling_rate(self, sampling_rate: int):
        """Forms the mel bank of the rate; returns librosa's peak-pick windows in frames (pre_max, post_max, pre_avg, post_avg, wait)."""
        pick = (c_int * 5)()
        self.sampling_rate, self.frame_start = 0, None
        with torch.cuda.device(self.index):
            self._call("said_beat_set_sampling_rate", int(sampling_rate), pick)
        self.sampling_rate, self.peak_pick = int(sampling_rate), tuple(pick)
        return self.peak_pick

    def clips(self, wave: torch.Tensor, offsets) -> np.ndarray:
        """Analyse the clips wave[offsets[i]:offsets[i + 1]] (one float32 device vector); returns the first frame number of each clip, (n + 1)."""
        wave, offs = _dev(wave, "the waveforms", index=self.index, strict=True), _i64(offsets)
        if wave.dim() != 1 or offs.ndim != 1 or offs.shape[0] < 2 or offs[-1] != wave.shape[0]:
            raise EngineError(f"offsets must have n + 1 >= 2 entries ending at the {wave.numel()} samples of the waveforms")
        self.frame_start = None
        self._go("said_beat_clips", _ptr(wave), offs.shape[0] - 1, _lp(offs))
        self.frame_start = np.concatenate([[0], np.cumsum(1 + np.diff(offs) // BEAT_HOP)]).astype(np.int64)
        return self.frame_start

    def coeffs(self, coeffs: torch.Tensor, offsets, threshold: float) -> None:
        """Change rates and their minima of the sequences coeffs[offsets[i]:offsets[i + 1]], a (frames, channels) float32 device tensor."""
        coeffs, offs = _dev(coeffs, "the coefficients", index=self.index, strict=True), _i64(offsets)
        if coeffs.dim() != 2 or offs.ndim != 1 or offs.shape[0] < 2 or offs[-1] != coeffs.shape[0]:
            raise EngineError(f"offsets must have n + 1 >= 2 entries ending at the {coeffs.shape[0]} frames of the coefficients")
        self.seq_off = None
        self._go("said_beat_coeffs", _ptr(coeffs), offs.shape[0] - 1, _lp(offs), coeffs.shape[1], float(threshold))
        self.seq_off = offs

    def score(self, clip_index, fps: float, sigma: float) -> np.ndarray:
        """(n_seq,) float64: the score of each sequence of the last coeffs() against clip clip_index[s] of the last clips()."""
        if self.seq_off is None or self.frame_start is None:
            raise EngineError("score() needs clips() and coeffs() first")
        idx = _i32(clip_index)
        if idx.shape != (self.seq_off.shape[0] - 1,):
            raise EngineError(f"clip_index must name one clip for each of the {self.seq_off.shape[0] - 1} sequences")
        out = np.empty(idx.shape[0])
        self._go("said_beat_score", _ip(idx), float(fps), float(sigma), _dp(out))
        return out

    def set_deltas(self, deltas: np.ndarray) -> None:
        """deltas (persons, channels, 3V) float64."""
        d = _f64(deltas)
        if d.ndim != 3:
            raise EngineError(f"deltas must be (persons, channels, 3V), got {d.shape}")
        self.delta_shape = None
        self._go("said_beat_set_deltas", d.shape[0], d.shape[1], d.shape[2], _dp(d))
        self.delta_shape = d.shape

    def vertex_error(self, coeffs: torch.Tensor, real_off, eval_off, length, person) -> np.ndarray:
        """(n_pairs,) float64: max over t < length[p] of |(coeffs[real_off[p] + t] - coeffs[eval_off[p] + t]) @ deltas[person[p]]|."""
        if self.delta_shape is None:
            raise EngineError("vertex_error() needs set_deltas() first")
        coeffs = _dev(coeffs, "the coefficients", index=self.index, strict=True)
        ro, eo, ln, pe = _i64(real_off), _i64(eval_off), _i32(length), _i32(person)
        if coeffs.dim() != 2 or coeffs.shape[1] != self.delta_shape[1] or not (ro.shape == eo.shape == ln.shape == pe.shape) or ro.ndim != 1:
            raise EngineError(f"coefficients must be (frames, {self.delta_shape[1]}) and the four pair tables of one length")
        out = np.empty(ro.shape[0])
        self._go("said_beat_vertex_error", _ptr(coeffs), coeffs.shape[0], ro.shape[0], _lp(ro), _lp(eo), _ip(ln), _ip(pe), _dp(out))
        return out

    def _lists(self, name: str, start: np.ndarray):
        counts, flat = np.zeros(start.shape[0] - 1, dtype=np.int32), np.zeros(int(start[-1]), dtype=np.int32)
        self._go(name, _ip(counts), _ip(flat))
        return [flat[int(s):int(s) + int(n)].copy() for s, n in zip(start[:-1], counts)]

    def _array(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape)
        self._go(name, _dp(out))
        return out

    def read_mel(self) -> np.ndarray:
        """(frames, 128) mel power of all clips' frames."""
        return self._array("said_beat_read_mel", (int(self.frame_start[-1]), BEAT_N_MELS))

    def read_envelope(self) -> np.ndarray:
        """(frames,) onset envelope of all clips' frames."""
        return self._array("said_beat_read_envelope", (int(self.frame_start[-1]),))

    def read_onsets(self):
        """Per clip its onset frame indices, ascending."""
        return self._lists("said_beat_read_onsets", self.frame_start)

    def read_rates(self):
        """Per sequence its (frames - 1,) change rates."""
        flat = self._array("said_beat_read_rates", (int(self.seq_off[-1]),))
        return [flat[int(a):int(b) - 1].copy() for a, b in zip(self.seq_off[:-1], self.seq_off[1:])]

    def read_minima(self):
        """Per sequence the indices of its change rate's minima, ascending."""
        return self._lists("said_beat_read_minima", self.seq_off)


class TransferEngine(_Context):
    """said_transfer context on one GPU (include/said_transfer.h): the mesh passes, the three stages and the solver
    alone; float64 host arrays in and out."""
    prefix, group = "said_transfer", "transfer"
    cpu_error, cpu_message = NoCpuPathError, "said_amd transfers blendshapes on MI355X only (device={}); there is no CPU path"

    def __init__(self, device: torch.device):
        super().__init__(device)
        self._create()
        self.source = self.target = None   # (V, F, K) and (V, F)

    @staticmethod
    def _system(structure: dict):
        """(TransferSystem, the arrays it points into) of a structure from said_amd.optimize.deformation_transfer."""
        keep = {name: _i32(structure.get(name)) for name in _TRANSFER_ARRAYS}
        sys_ = TransferSystem(int(structure["m"]), int(structure["n"]), int(keep["col"].shape[0]), *[_ip(keep[name]) for name in _TRANSFER_ARRAYS])
        return sys_, keep

    def set_source(self, neutral, faces, shapes=None) -> None:
        v, f = _f64(neutral), _i32(faces)
        sh = None if shapes is None or len(shapes) == 0 else _f64(shapes)
        if sh is not None and sh.shape[1:] != v.shape:
            raise EngineError(f"shapes must be (K, {v.shape[0]}, 3), got {sh.shape}")
        k = 0 if sh is None else sh.shape[0]
        self._go("said_transfer_set_source", v.shape[0], f.shape[0], k, _dp(v), _ip(f), _dp(sh))
        self.source = (v.shape[0], f.shape[0], k)

    def set_target(self, neutral, faces) -> None:
        v, f = _f64(neutral), _i32(faces)
        self._go("said_transfer_set_target", v.shape[0], f.shape[0], _dp(v), _ip(f))
        self.target = (v.shape[0], f.shape[0])

    def solve(self, a_rowptr, a_col, a_val, at_rowptr, at_col, at_val, b, x0=None, tol: float = 1e-10, max_iter: int = 20000, check_every: int = 50):
        """(x (n, R), status (R), iters (R), relative residual (R)) of min |A x - b| by the device solver; A (m, n) and A' in CSR."""
        b = _f64(b)
        m, r = b.shape
        n = len(at_rowptr) - 1
        arp, ac, av, trp, tc, tv = _i32(a_rowptr), _i32(a_col), _f64(a_val), _i32(at_rowptr), _i32(at_col), _f64(at_val)
        if arp.shape[0] != m + 1 or ac.shape != av.shape or tc.shape != tv.shape or ac.shape != tc.shape:
            raise EngineError("the CSR arrays of A and A' do not fit the right-hand side")
        x0 = _f64(x0)
        if x0 is not None and x0.shape != (n, r):
            raise EngineError(f"x0 must be ({n}, {r}), got {x0.shape}")
        x = np.empty((n, r))
        st, it, res = np.zeros(r, dtype=np.int32), np.zeros(r, dtype=np.int32), np.zeros(r)
        self._go("said_transfer_solve", m, n, ac.shape[0], r, _ip(arp), _ip(ac), _dp(av), _ip(trp), _ip(tc), _dp(tv), _dp(b), _dp(x0), float(tol),
                 int(max_iter), int(check_every), _dp(x), _ip(st), _ip(it), _dp(res))
        return x, st, it, res

    def register(self, structure: dict, marker_src, marker_pos, w_s: float, w_i: float, schedule, tol: float, max_iter: int):
        """(x (solves, V_s + F_s, 3), closest (solves, V_s), status, iters, resid (solves, 3))."""
        sys_, keep = self._system(structure)
        ms, mp, wc = _i32(marker_src), _f64(marker_pos), _f64(schedule)
        ns, nv = wc.shape[0], self.source[0]
        x = np.empty((ns, sys_.n, 3))
        closest = np.empty((ns, nv), dtype=np.int32)
        st, it, res = np.zeros((ns, 3), dtype=np.int32), np.zeros((ns, 3), dtype=np.int32), np.zeros((ns, 3))
        self._go("said_transfer_register", ctypes.byref(sys_), ms.shape[0], _ip(ms), _dp(mp), float(w_s), float(w_i), ns, _dp(wc), float(tol), int(max_iter),
                 _dp(x), _ip(closest), _ip(st), _ip(it), _dp(res))
        del keep
        return x, closest, st, it, res

    def correspond(self, threshold: float, registered=None):
        """(t2s (F_t), s2t (F_s), their squared centroid distances): -1 where a triangle has no partner within the threshold."""
        reg = _f64(registered)
        if reg is not None and reg.shape != (self.source[0], 3):
            raise EngineError(f"the registered source must be ({self.source[0]}, 3), got {reg.shape}")
        t2s, s2t = np.empty(self.target[1], dtype=np.int32), np.empty(self.source[1], dtype=np.int32)
        dt, ds = np.empty(self.target[1]), np.empty(self.source[1])
        self._go("said_transfer_correspond", _dp(reg), float(threshold), _ip(t2s), _ip(s2t), _dp(dt), _dp(ds))
        return t2s, s2t, dt, ds

    def transfer(self, structure: dict, tol: float, max_iter: int):
        """(residuals (K, V_t, 3), status, iters, resid (3 K))."""
        sys_, keep = self._system(structure)
        k, nv = self.source[2], self.target[0]
        out = np.empty((k, nv, 3))
        st, it, res = np.zeros(3 * k, dtype=np.int32), np.zeros(3 * k, dtype=np.int32), np.zeros(3 * k)
        self._go("said_transfer_transfer", ctypes.byref(sys_), float(tol), int(max_iter), _dp(out), _ip(st), _ip(it), _dp(res))
        del keep
        return out, st, it, res

    def mesh(self, verts, faces):
        """{"w": (F, 3, 3) V^-T, "gc": (F, 3, 4), "fn": (F, 3), "centroid": (F, 3), "vn": (V, 3)} of a mesh."""
        v, f = _f64(verts), _i32(faces)
        nv, nf = v.shape[0], f.shape[0]
        out = {"w": np.empty((nf, 3, 3)), "gc": np.empty((nf, 3, 4)), "fn": np.empty((nf, 3)), "centroid": np.empty((nf, 3)), "vn": np.empty((nv, 3))}
        self._go("said_transfer_mesh", nv, nf, _dp(v), _ip(f), *[_dp(out[name]) for name in ("w", "gc", "fn", "centroid", "vn")])
        return out

    def gradients(self, ref, faces, deformed) -> np.ndarray:
        """(K, F, 3, 3) deformation gradients of deformed (K, V, 3) against ref."""
        v, f, d = _f64(ref), _i32(faces), _f64(deformed)
        if d.ndim != 3 or d.shape[1:] != v.shape:
            raise EngineError(f"deformed must be (K, {v.shape[0]}, 3), got {d.shape}")
        q = np.empty((d.shape[0], f.shape[0], 3, 3))
        self._go("said_transfer_gradients", v.shape[0], f.shape[0], _dp(v), _ip(f), d.shape[0], _dp(d), _dp(q))
        return q

    def closest(self, qpos, qnrm, tpos, tnrm):
        """(index per query, squared distance): the nearest target whose normal has a positive dot product with the query's (both None: the nearest)."""
        qp, tp = _f64(qpos), _f64(tpos)
        qn, tn = (None, None) if qnrm is None else (_f64(qnrm), _f64(tnrm))
        idx, d2 = np.empty(qp.shape[0], dtype=np.int32), np.empty(qp.shape[0])
        self._go("said_transfer_closest", qp.shape[0], _dp(qp), _dp(qn), tp.shape[0], _dp(tp), _dp(tn), _ip(idx), _dp(d2))
        return idx, d2
