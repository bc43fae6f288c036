"""ctypes binding of libgligen_amd.so (C ABI declared in include/gligen_amd.h, include/gligen_amd_image.h, include/gligen_amd_maps.h and
include/gligen_amd_train_maps.h, include/gligen_amd_train_inputs.h, include/gligen_amd_train_fusers.h, include/gligen_amd_train_prims.h,
include/gligen_amd_trainer.h, include/gligen_amd_sampler.h, include/gligen_amd_solver.h, include/gligen_amd_gemm_plans.h, include/gligen_amd_attention_core.h, include/gligen_amd_conv8.h, include/gligen_amd_ffn_rows.h, include/gligen_amd_norm.h, include/gligen_amd_vae.h, include/gligen_amd_latent.h, include/gligen_amd_lora.h, include/gligen_amd_tiling.h, include/gligen_amd_train_lora.h, include/gligen_amd_train_lora_conv.h and include/gligen_amd_train_run.h).

The library is the only compute path: if it is missing or a call fails, this module raises —
there is no PyTorch/CPU fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "libgligen_amd.so"


class GligenAmdError(RuntimeError):
    pass


class UNetConfig(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int), ("out_channels", C.c_int), ("model_channels", C.c_int),
        ("num_res_blocks", C.c_int), ("num_heads", C.c_int), ("context_dim", C.c_int),
        ("n_mult", C.c_int), ("channel_mult", C.c_int * 8),
        ("n_attn", C.c_int), ("attention_resolutions", C.c_int * 8),
        ("inpaint_mode", C.c_int), ("grounding_kind", C.c_int),
        ("gr_in_dim", C.c_int), ("gr_out_dim", C.c_int), ("max_persons", C.c_int), ("fuser_kind", C.c_int),
        ("extra_channels", C.c_int), ("tok_resize", C.c_int), ("tok_in_dim", C.c_int),
    ]


class VaeConfig(C.Structure):
    _fields_ = [
        ("ch", C.c_int), ("out_ch", C.c_int), ("z_channels", C.c_int), ("num_res_blocks", C.c_int),
        ("embed_dim", C.c_int), ("n_mult", C.c_int), ("ch_mult", C.c_int * 8), ("scale_factor", C.c_float),
    ]


class ClipTextConfig(C.Structure):   # = gl_clip_text_config
    _fields_ = [(n, C.c_int) for n in ("vocab", "width", "heads", "layers", "intermediate", "max_positions")] + [("ln_eps", C.c_float)]


class ClipVisionConfig(C.Structure):   # = gl_clip_vision_config
    _fields_ = [(n, C.c_int) for n in ("image_size", "patch", "width", "heads", "layers", "intermediate", "projection_dim")] + [("ln_eps", C.c_float)]


class ImageDesc(C.Structure):   # = gl_image_desc
    _fields_ = [("pixels", C.c_void_p)] + [(n, C.c_int) for n in ("width", "height", "row_stride", "resized_w", "resized_h",
                                                                  "crop_x", "crop_y", "crop_w", "crop_h")]


class ClassMapDesc(C.Structure):   # = gl_class_map_desc
    _fields_ = [("pixels", C.c_void_p)] + [(n, C.c_int) for n in ("width", "height", "row_stride", "box_x", "box_y", "box_w", "box_h")]


class Grounding(C.Structure):
    _fields_ = [
        ("n", C.c_int),
        ("boxes", C.c_void_p), ("masks", C.c_void_p), ("text_masks", C.c_void_p), ("image_masks", C.c_void_p),
        ("text_embeddings", C.c_void_p), ("image_embeddings", C.c_void_p), ("points", C.c_void_p), ("tokens", C.c_void_p),
    ]


class PlmsArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint), ("B", C.c_int), ("h", C.c_int), ("w", C.c_int), ("n_steps", C.c_int),
        ("timesteps", C.POINTER(C.c_int64)), ("a_t", C.POINTER(C.c_float)), ("a_prev", C.POINTER(C.c_float)),
        ("fuser_scale", C.POINTER(C.c_float)), ("guidance_scale", C.c_float),
        ("x", C.c_void_p), ("inpaint_extra", C.c_void_p), ("mask", C.c_void_p), ("x0", C.c_void_p),
        ("noise", C.c_void_p), ("mask_B", C.c_int), ("x0_B", C.c_int), ("noise_B", C.c_int),
        ("sqrt_ac", C.POINTER(C.c_float)), ("sqrt_1mac", C.POINTER(C.c_float)),
        ("use_graph", C.c_int), ("sd_conv_w", C.c_void_p), ("sd_conv_b", C.c_void_p), ("sd_conv_step", C.c_int), ("ddim", C.c_int),
    ]


class SolverArgs(C.Structure):   # = gl_solver_args
    _fields_ = [
        ("struct_size", C.c_uint), ("B", C.c_int), ("h", C.c_int), ("w", C.c_int), ("n_steps", C.c_int),
        ("timesteps", C.POINTER(C.c_int64)), ("a_t", C.POINTER(C.c_float)),
        ("cx", C.POINTER(C.c_float)), ("c0", C.POINTER(C.c_float)), ("c1", C.POINTER(C.c_float)), ("c2", C.POINTER(C.c_float)),
        ("cn", C.POINTER(C.c_float)), ("step_noise", C.c_void_p),
        ("fuser_scale", C.POINTER(C.c_float)), ("guidance_scale", C.c_float),
        ("x", C.c_void_p), ("inpaint_extra", C.c_void_p), ("mask", C.c_void_p), ("x0", C.c_void_p),
        ("noise", C.c_void_p), ("mask_B", C.c_int), ("x0_B", C.c_int), ("noise_B", C.c_int),
        ("sqrt_ac", C.POINTER(C.c_float)), ("sqrt_1mac", C.POINTER(C.c_float)),
        ("use_graph", C.c_int), ("sd_conv_w", C.c_void_p), ("sd_conv_b", C.c_void_p), ("sd_conv_step", C.c_int),
    ]


class TrainUNetIn(C.Structure):   # = gl_train_unet_in
    _fields_ = [(n, C.c_int) for n in ("B", "H", "W", "ctx_T", "Ng")] + \
               [(n, C.c_void_p) for n in ("x", "timesteps", "context", "boxes", "masks", "positive_embeddings", "target")] + \
               [("fuser_scale", C.c_float)] + [(n, C.c_void_p) for n in ("text_masks", "image_masks", "image_embeddings")] + [("checkpoint", C.c_int), ("use_weight_cache", C.c_int)]


class TrainSpatialIn(C.Structure):   # = gl_train_spatial_in
    _fields_ = [("map", C.c_void_p)] + [(n, C.c_int) for n in ("map_channels", "map_h", "map_w")] + [("mask", C.c_void_p), ("extra", C.c_void_p)] + \
               [(n, C.c_int) for n in ("extra_in_channels", "extra_h", "extra_w", "ds_resize", "ds_mode", "ds_n_in", "ds_mid")]


class TrainSpatialClassesIn(C.Structure):   # = gl_train_spatial_classes_in
    _fields_ = [("map", C.c_void_p), ("map_h", C.c_int), ("map_w", C.c_int), ("mask", C.c_void_p), ("extra", C.c_void_p)] + \
               [(n, C.c_int) for n in ("extra_h", "extra_w", "ds_resize", "ds_mode", "ds_n_in", "ds_mid")]


class TrainStepInputsArgs(C.Structure):   # = gl_train_step_inputs_args
    _fields_ = [("struct_size", C.c_uint)] + [(n, C.c_int) for n in ("B", "C", "H", "W", "n_t", "n_boxes", "inpaint")] + \
               [(n, C.c_void_p) for n in ("z", "noise", "timesteps", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "boxes", "mask",
                                          "x_rows", "target_rows", "t_float")]


class BoxCalibration(C.Structure):   # = gl_box_calibration
    _fields_ = [("hbm_copy_gbs", C.c_float), ("lds_dma_tbs", C.c_float), ("mfma_bf16_tflops", C.c_float)]


class MfmaCalibration(C.Structure):   # = gl_mfma_calibration
    _fields_ = [("tflops", C.c_float), ("sclk_mhz", C.c_float), ("ms", C.c_float), ("cycles_per_mfma", C.c_float)]


class ProfRec(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("calls", C.c_int), ("ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


# every symbol include/gligen_amd.h declares: (name, restype, argtypes)
_P = C.c_void_p
_I = C.c_int
SYMBOLS = {
    "gl_last_error": (C.c_char_p, []),
    "gl_ctx_create": (_I, [_I, C.c_size_t, C.POINTER(_P)]),
    "gl_ctx_fork": (_I, [_P, C.c_size_t, C.POINTER(_P)]),
    "gl_ctx_memory": (_I, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(_I)]),
    "gl_ctx_destroy": (_I, [_P]),
    "gl_unet_configure": (_I, [_P, C.POINTER(UNetConfig)]),
    "gl_vae_configure": (_I, [_P, C.POINTER(VaeConfig)]),
    "gl_weight_upload": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I]),
    "gl_finalize": (_I, [_P]),
    "gl_clip_text_configure": (_I, [_P, C.POINTER(ClipTextConfig)]),
    "gl_clip_text_encode": (_I, [_P, _P, _P, _I, _I, _P, _P, _P]),
    "gl_clip_vision_configure": (_I, [_P, C.POINTER(ClipVisionConfig)]),
    "gl_clip_vision_encode": (_I, [_P, _P, _I, _P, _P, _P, _P]),
    "gl_op_clip_attention": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "gl_unet_set_cond": (_I, [_P, _I, _P, _I, C.POINTER(Grounding), _P]),
    "gl_unet_set_fuser_scale": (_I, [_P, C.c_float, _P]),
    "gl_unet_set_fuser_scales": (_I, [_P, C.POINTER(C.c_float), _I, _P]),
    "gl_unet_grounding_tokens": (_I, [_P, _P, _P]),
    "gl_op_spatial_tokens": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "gl_op_grounding_downsample": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P]),
    "gl_unet_restore_first_conv": (_I, [_P, _P, _P, _P]),
    "gl_unet_forward": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _I, _P, _P]),
    "gl_vae_decode": (_I, [_P, _I, _I, _I, _P, _P, _P]),
    "gl_vae_encode": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "gl_sample_plms": (_I, [_P, C.POINTER(PlmsArgs), _P]),
    "gl_sampler_timing": (_I, [_P, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(_I)]),
    "gl_unet_profile": (_I, [_P, _I, _I, _I, _P, _I, _P, _P, _I, _P, C.POINTER(ProfRec), _I, C.POINTER(_I), _P]),
    "gl_to_uint8": (_I, [_P, _P, _I, _I, _I, _P]),
    "gl_arena_high_water": (_I, [_P, C.POINTER(C.c_size_t)]),
    "gl_launch_count": (_I, [_P, C.POINTER(C.c_int64)]),
    "gl_set_ff_rows_policy": (_I, [_I]),
    "gl_ff_rows_policy_report": (_I, [C.c_char_p, C.c_size_t]),
    "gl_box_calibrate": (_I, [_P, C.POINTER(BoxCalibration), _P]),
    "gl_mfma_calibrate": (_I, [_P, _I, _I, _I, _I, C.c_float, C.POINTER(MfmaCalibration), _P]),
    "gl_op_linear": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "gl_op_geglu": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "gl_op_ln_linear": (_I, [_P, _P, _I, _I, _P, _P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _P, _P, C.POINTER(_I), _P]),
    "gl_op_feedforward": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(_I), _P]),
    "gl_train_block_param_names": (C.POINTER(C.c_char_p), []),
    "gl_op_block_train": (_I, [_P, _P, C.POINTER(_P), _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(_P), _P]),
    "gl_train_st_param_names": (C.POINTER(C.c_char_p), []),
    "gl_op_st_train": (_I, [_P, _P, C.POINTER(_P), _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(_P), _P]),
    "gl_train_resblock_param_names": (C.POINTER(C.c_char_p), []),
    "gl_op_resblock_train": (_I, [_P, _P, C.POINTER(_P), _P, _P, _P, _P, _P, _P, _P]),
    "gl_op_resample_train": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gl_unet_train_step": (_I, [_P, C.POINTER(UNetConfig), C.POINTER(TrainUNetIn), _I, C.POINTER(C.c_char_p), C.POINTER(_P), C.POINTER(_P), _P, _P, _P]),
    "gl_unet_train_step_spatial": (_I, [_P, C.POINTER(UNetConfig), C.POINTER(TrainUNetIn), C.POINTER(TrainSpatialIn), _I, C.POINTER(C.c_char_p),
                                        C.POINTER(_P), C.POINTER(_P), _P, _P, _P]),
    "gl_train_wait_grads": (_I, [_P, _I, _P]),
    "gl_train_weight_cache": (_I, [_P, _I, C.POINTER(C.c_size_t)]),
    "gl_op_adamw_step": (_I, [_P, _P, _P, _P, _P, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _I, _P]),
    "gl_op_ff_chain": (_I, [_P, _P, _I, _I] + [_P] * 16),
    "gl_op_conv3x3": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "gl_op_groupnorm": (_I, [_P, _P, _I, _P, _I, _I, _I, _P, _P, C.c_float, _I, _P, _P]),
    "gl_op_gn_silu_conv3x3": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P, C.c_float, _P, _P, _I, _P, _P, _P, _I, _P, _P]),
    "gl_op_layernorm": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P, C.c_float, _P, _P]),
    "gl_op_attention": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "gl_attn_regime_counters": (_I, [_P, _I, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "gl_op_ff_chain_q": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gl_op_proj_attention": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, C.POINTER(_I), _P]),
}

# every symbol include/gligen_amd_image.h declares (the image front end)
IMAGE_SYMBOLS = {
    "gl_op_image_resample": (_I, [_P, C.POINTER(ImageDesc), _I, _I, _I, C.POINTER(C.c_float), _P, _P]),
    "gl_image_resample_coeffs": (_I, [_I, _I, _I, C.POINTER(_I), C.POINTER(_I), _I, C.POINTER(_I), _I]),
}

# every symbol include/gligen_amd_maps.h declares (semantic maps as class indices)
MAP_SYMBOLS = {
    "gl_op_class_map_resize": (_I, [_P, C.POINTER(ClassMapDesc), _I, _I, _I, _P, _P]),
    "gl_class_map_index_table": (_I, [_I, _I, _I, C.POINTER(_I), _I]),
    "gl_op_spatial_tokens_classes": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "gl_op_grounding_downsample_classes": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _P, _P]),
}

# every symbol include/gligen_amd_train_maps.h declares (training from class maps)
TRAIN_MAP_SYMBOLS = {
    "gl_unet_train_step_spatial_classes": (_I, [_P, C.POINTER(UNetConfig), C.POINTER(TrainUNetIn), C.POINTER(TrainSpatialClassesIn), _I, C.POINTER(C.c_char_p),
                                                C.POINTER(_P), C.POINTER(_P), _P, _P, _P]),
    "gl_op_class_conv_wgrad": (_I, [_P, _I, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P, _P]),
}

# every symbol include/gligen_amd_train_inputs.h declares (the input stage of a training iteration)
TRAIN_INPUT_SYMBOLS = {
    "gl_train_step_inputs": (_I, [_P, C.POINTER(TrainStepInputsArgs), _P]),
}

# every symbol include/gligen_amd_train_fusers.h declares (the block slice by fuser kind, the fp32 grid resize and its adjoint)
TRAIN_FUSER_SYMBOLS = {
    "gl_op_block_train_fuser": (_I, [_P, _I, _P, C.POINTER(_P), _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(_P), _P]),
    "gl_op_grid_resize": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "gl_op_grid_resize_backward": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
}

# every symbol include/gligen_amd_train_prims.h declares (the training path's primitives one by one)
_F = C.c_float
TRAIN_PRIM_SYMBOLS = {
    "gl_op_train_attention": (_I, [_P, _I, _I, _I, _I, _I] + [_P] * 9 + [_P]),
    "gl_op_train_linear": (_I, [_P, _I, _I, _I] + [_P] * 8 + [_P]),
    "gl_op_train_layernorm": (_I, [_P, _I, _I, _F, _P, _P, _P, _P, _I] + [_P] * 6 + [_P]),
    "gl_op_train_groupnorm": (_I, [_P, _I, _I, _I, _I, _F, _P, _P, _P, _P, _I] + [_P] * 4 + [_P]),
    "gl_op_train_geglu": (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    "gl_op_train_dot": (_I, [_P, C.c_int64, _P, _P, _P, _F, _I, _P, _P]),
    "gl_op_train_conv3": (_I, [_P] + [_I] * 6 + [_P] * 6 + [_P]),
    "gl_op_train_conv_direct": (_I, [_P] + [_I] * 7 + [_P] * 7 + [_P]),
}

class LoraAdapter(C.Structure):   # = gl_lora_adapter
    _fields_ = [("name", C.c_char_p), ("down", C.c_void_p), ("up", C.c_void_p), ("g_down", C.c_void_p), ("g_up", C.c_void_p), ("rank", C.c_int),
                ("scale", C.c_float)]


# every symbol include/gligen_amd_train_lora.h declares (the training iteration with LoRA adapters; one adapted Linear's low-rank part)
TRAIN_LORA_SYMBOLS = {
    "gl_unet_train_step_lora": (_I, [_P, C.POINTER(UNetConfig), C.POINTER(TrainUNetIn), _I, C.POINTER(C.c_char_p), C.POINTER(_P), C.POINTER(_P),
                                     C.POINTER(LoraAdapter), _I, _P, _P, _P]),
    "gl_op_lora_linear": (_I, [_P, _I, _I, _I, _I, _F, _I, _I] + [_P] * 10 + [_P]),
    "gl_lora_wgrad_chunk_rows": (_I, [_I]),
}

# every symbol include/gligen_amd_train_lora_conv.h declares (one adapted 3 x 3 conv's low-rank part: ResBlock, Downsample, Upsample)
TRAIN_LORA_CONV_SYMBOLS = {
    "gl_op_lora_conv3": (_I, [_P, _I, _I, _I, _I, _I, _I, _F, _I] + [_P] * 10 + [_P]),
}

# every symbol include/gligen_amd_trainer.h declares (the optimizer unit of a training run: AdamW + EMA in one pass)
TRAINER_SYMBOLS = {
    "gl_op_adamw_ema_step": (_I, [_P, _P, _P, _P, _P, _P, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _I, _P]),
}

# every symbol include/gligen_amd_train_run.h declares (gradient accumulation, the global norm and its clipping coefficient, the clipped
# AdamW (+ EMA) update, per-sample loss weights for the next training step)
_D = C.c_double
TRAIN_RUN_SYMBOLS = {
    "gl_op_grad_accumulate": (_I, [_P, _P, _P, C.c_int64, _I, _I, _P]),
    "gl_grad_sqnorm_partials": (C.c_int64, [C.c_int64]),
    "gl_op_grad_sqnorm": (_I, [_P, _P, C.c_int64, _P, _P]),
    "gl_op_clip_coef": (_I, [_P, _P, C.c_int64, C.c_float, _P, _P]),
    "gl_op_adamw_clip_step": (_I, [_P, _P, _P, _P, _P, C.c_int64, _D, _D, _D, _D, _D, _I, _P, _P]),
    "gl_op_adamw_ema_clip_step": (_I, [_P, _P, _P, _P, _P, _P, C.c_int64, _D, _D, _D, _D, _D, _D, _I, _P, _P]),
    "gl_train_set_loss_weights": (_I, [_P, _P, _I]),
}
GRAD_ACCUM_MODES = {"first": 0, "middle": 1, "last": 2}   # = GL_GRAD_ACCUM_*

# every symbol include/gligen_amd_sampler.h declares (how the sampler schedules the guidance pair)
SAMPLER_SYMBOLS = {
    "gl_set_cfg_shared_prefix": (_I, [_I]),
}

# every symbol include/gligen_amd_solver.h declares (the linear multistep solver loop and its update kernel)
SOLVER_SYMBOLS = {
    "gl_sample_solver": (_I, [_P, C.POINTER(SolverArgs), _P]),
    "gl_op_solver_update": (_I, [_P, _P, _I, C.c_float, C.c_float, _P, _P, _P, _P, _P, _P] + [C.c_float] * 5 + [C.c_int64, _P]),
}


class GemmPlanRecord(C.Structure):   # = gl_gemm_plan_record
    _fields_ = [("kernel", C.c_char * 96)] + [(n, C.c_int) for n in ("family", "M", "N", "K", "tm", "tn", "splits", "grid", "n_items", "box", "rm", "rz",
                                                                     "units_per_split", "xcd")]


class AttnProjLayout(C.Structure):   # = gl_attn_proj_layout
    _fields_ = [(n, C.c_int) for n in ("d", "dp", "dpv", "tq", "tk", "tq_pad", "tk_pad", "vt_perm32")]


class GemmEpilogueArgs(C.Structure):   # = gl_gemm_epilogue_args
    _fields_ = [("struct_size", C.c_uint), ("conv", _I), ("M", _I), ("N", _I), ("K", _I), ("x0", _P), ("x1", _P)] + \
               [(n, _I) for n in ("C0", "C1", "B", "H", "W", "stride", "ups", "pad_lo")] + \
               [("w", _P), ("bias", _P), ("bias2", _P), ("bias2_ld", _I), ("rows_per_b", _I), ("res", _P), ("ldres", _I), ("gate", _P)] + \
               [(n, _I) for n in ("act", "out_f32", "mode", "n_real", "remap_in", "remap_out", "remap_off")] + [("out", _P), ("ldo", _I)]


# every symbol include/gligen_amd_gemm_plans.h declares (one named GEMM plan at a time, and the log of what ran)
GEMM_PLAN_SYMBOLS = {
    "gl_op_attention_project_range": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, C.POINTER(AttnProjLayout), _P]),
    "gl_op_gemm_epilogue": (_I, [_P, C.POINTER(GemmEpilogueArgs), _P]),
    "gl_gemm_force_plan": (_I, [_I, _I, _I, _I]),
    "gl_gemm_force_knobs": (_I, [_I, _I, _I, _I, _I, _I]),
    "gl_gemm_force_clear": (_I, []),
    "gl_gemm_plan_log_clear": (_I, []),
    "gl_gemm_plan_log": (_I, [C.POINTER(GemmPlanRecord), _I, C.POINTER(_I), C.POINTER(_I)]),
    "gl_op_attention_project": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, C.POINTER(AttnProjLayout), _P]),
}

# every symbol include/gligen_amd_attention_core.h declares (one attention kernel on the caller's q, k, v^T buffers)
ATTENTION_CORE_SYMBOLS = {
    "gl_op_attention_core": (_I, [_P, _P, _P, _P, C.POINTER(AttnProjLayout), _I, _I, _I, _I, _P, _I, _I, _I, _P]),
}


class Conv8Args(C.Structure):   # = gl_conv8_args
    _fields_ = [("struct_size", C.c_uint), ("x0", _P), ("x1", _P)] + [(n, _I) for n in ("C0", "C1", "B", "H", "W", "N", "stride", "ups", "pad_lo")] + \
               [("w", _P), ("bias", _P), ("bias2", _P), ("bias2_ld", _I), ("rows_per_b", _I), ("res", _P), ("ldres", _I), ("act", _I), ("out_f32", _I),
                ("out", _P), ("ldo", _I), ("bn", _I), ("splits", _I), ("grid_cap", _I), ("slabs", _P), ("slab_bytes", C.c_size_t)]


# every symbol include/gligen_amd_conv8.h declares (conv8_kernel by name on the caller's buffers, the router's answer, the family's knobs)
CONV8_SYMBOLS = {
    "gl_op_conv8x8": (_I, [_P, C.POINTER(Conv8Args), _P]),
    "gl_conv8_routed": (_I, [C.POINTER(Conv8Args)]),
    "gl_conv8_force_knobs": (_I, [_I, _I, _I]),
}
ATTN_CORE_KERNELS = {"auto": 0, "attn_kernel": 1, "attn2_kernel_w4": 2, "attn2_kernel_w8": 3, "attn3_kernel": 4}   # = GL_ATTN_CORE_*
GL_ERR_UNSUPPORTED = 5


class FFRowsArgs(C.Structure):   # = gl_ff_rows_args
    _fields_ = [("struct_size", C.c_uint), ("M", _I), ("C", _I), ("x", _P), ("ldx", _I), ("normalize", _I), ("eps", C.c_float), ("gamma", _P), ("beta", _P),
                ("w1", _P), ("b1", _P), ("w2", _P), ("b2", _P), ("res", _P), ("ldres", _I), ("gate", _P), ("out", _P), ("ldo", _I), ("stats_out", _P),
                ("stats_ld", _I), ("pre", _I), ("post", _I), ("pre_w", _P), ("pre_b", _P), ("pre_res", _P), ("ld_pre_res", _I), ("pre_gate", _P),
                ("mid_out", _P), ("ld_mid", _I), ("post_w", _P), ("post_b", _P), ("post_res", _P), ("ld_post_res", _I), ("gamma_q", _P), ("beta_q", _P),
                ("q", _P), ("qDP", _I), ("qT", _I), ("qTpad", _I)]


class QkvRowsArgs(C.Structure):   # = gl_qkv_rows_args
    _fields_ = [("struct_size", C.c_uint), ("M", _I), ("C", _I), ("H", _I), ("x", _P), ("ldx", _I), ("normalize", _I), ("eps", C.c_float), ("pre", _I),
                ("pre_w", _P), ("pre_b", _P), ("pre_res", _P), ("ld_pre_res", _I), ("mid_out", _P), ("ld_mid", _I), ("stats_out", _P), ("gamma", _P),
                ("beta", _P), ("np", _I), ("w", _P), ("bias", _P), ("q", _P), ("k", _P), ("vt", _P), ("DP", _I), ("DPV", _I), ("T", _I), ("Tpad_q", _I),
                ("Tpad_k", _I), ("in_period", _I)]


# every symbol include/gligen_amd_ffn_rows.h declares (the row-local feed-forward and q,k,v^T kernels on the caller's buffers)
FFN_ROWS_SYMBOLS = {
    "gl_op_ff_rows": (_I, [_P, C.POINTER(FFRowsArgs), _P]),
    "gl_op_qkv_rows": (_I, [_P, C.POINTER(QkvRowsArgs), _P]),
}

class LayerNormRowsArgs(C.Structure):   # = gl_layernorm_rows_args
    _fields_ = [("struct_size", C.c_uint), ("x", _P), ("x2", _P), ("B", _I), ("N1", _I), ("N2", _I), ("Tpad", _I), ("C", _I), ("eps", C.c_float),
                ("gamma", _P), ("beta", _P), ("y", _P), ("ldx", _I), ("ldy", _I)]


# every symbol include/gligen_amd_norm.h declares (the statistics-only GroupNorm and the strided LayerNorm on the caller's buffers)
NORM_SYMBOLS = {
    "gl_op_groupnorm_coef": (_I, [_P, _P, _I, _P, _I, _I, _I, _P, _P, C.c_float, _P, C.POINTER(_I), _P]),
    "gl_op_layernorm_rows": (_I, [_P, C.POINTER(LayerNormRowsArgs), _P]),
}

# every symbol include/gligen_amd_vae.h declares (the form of the autoencoder's attention, and the operator by itself)
VAE_SYMBOLS = {
    "gl_vae_set_attention": (_I, [_P, _I]),
    "gl_op_vae_attention": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _P]),
}
VAE_ATTN_MODES = {"auto": 0, "matrix": 1, "flash": 2}   # = GL_VAE_ATTN_*

# every symbol include/gligen_amd_latent.h declares (resize + q_sample in one launch: the start point of a partial sampling)
LATENT_SYMBOLS = {
    "gl_op_latent_renoise": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _F, _F, _P, _I, _P]),
    "gl_latent_resize_taps": (_I, [_I, _I, _I, C.POINTER(_I), C.POINTER(_F)]),
}
LATENT_RESIZE_MODES = {"nearest-exact": 0, "bilinear": 1, "bicubic": 2}   # = GL_LATENT_*

# every symbol include/gligen_amd_lora.h declares (a LoRA adapter merged into fp32 parameters in place)
LORA_SYMBOLS = {
    "gl_op_lora_merge": (_I, [_P, _P, _P, _P, _I, _I, _I, _F, _P]),
}



class TilePlan(C.Structure):   # = gl_tile_plan
    _fields_ = [("struct_size", C.c_uint)] + [(n, C.c_int) for n in ("ny", "nx", "th_in", "tw_in", "th_out", "tw_out")] + \
               [(n, C.c_void_p) for n in ("windows", "oy", "ox", "wy", "wx")]


# every symbol include/gligen_amd_tiling.h declares (the autoencoder over overlapping tiles; the gather and the blend by themselves)
TILING_SYMBOLS = {
    "gl_vae_decode_tiled": (_I, [_P, _I, _I, _I, _P, _P, C.POINTER(TilePlan), _I, _P]),
    "gl_vae_encode_tiled": (_I, [_P, _I, _I, _I, _P, _P, _P, _P, C.POINTER(TilePlan), _I, _P]),
    "gl_op_tile_gather": (_I, [_P, _P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P]),
    "gl_op_tile_blend": (_I, [_P, _P, _I, _I, C.POINTER(TilePlan), _P, _I, _I, _I, _I, _P]),
}

# gl_unet_config.fuser_kind / the fuser_kind of gl_op_block_train_fuser, by the reference's fuser_type
FUSER_KINDS = {"gatedSA": 0, "gatedSA2": 1, "gatedCA": 2}


def fuser_kind(fuser_type) -> int:
    """UNetModel's fuser_type (None: the default gatedSA) as the library's fuser_kind."""
    try:
        return FUSER_KINDS[fuser_type or "gatedSA"]
    except KeyError:
        raise ValueError(f"fuser_type {fuser_type!r}: one of {sorted(FUSER_KINDS)}") from None


_lib = None


def load() -> C.CDLL:
    """Load the shared library and bind every declared symbol (raises if anything is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise GligenAmdError(
            f"{LIB_PATH} not found: build it with `python -m gligen_amd.build` "
            "(gligen_amd has no fallback path without its HIP library)")
    # torch first: its wheel bundles its own libamdhip64.so. Loaded after ours (which resolves /opt/rocm's copy) the process ends up
    # with two HIP runtimes and the second one finds no device ("no HIP device available" from gl_context_create although
    # torch.cuda.is_available() is True) -- seen with build() called before the first `import torch` of the process.
    import torch  # noqa: F401
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in {**SYMBOLS, **IMAGE_SYMBOLS, **MAP_SYMBOLS, **TRAIN_MAP_SYMBOLS, **TRAIN_INPUT_SYMBOLS, **TRAIN_FUSER_SYMBOLS, **TRAIN_PRIM_SYMBOLS,
                              **TRAINER_SYMBOLS, **SAMPLER_SYMBOLS, **SOLVER_SYMBOLS, **GEMM_PLAN_SYMBOLS, **ATTENTION_CORE_SYMBOLS, **CONV8_SYMBOLS, **FFN_ROWS_SYMBOLS, **NORM_SYMBOLS, **VAE_SYMBOLS, **LATENT_SYMBOLS, **LORA_SYMBOLS, **TILING_SYMBOLS, **TRAIN_LORA_SYMBOLS, **TRAIN_LORA_CONV_SYMBOLS,
                              **TRAIN_RUN_SYMBOLS}.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().gl_last_error()
        raise GligenAmdError(f"libgligen_amd error {rc}: {msg.decode() if msg else '?'}")
