"""ctypes binding of libcfgpp_hip.so (the C ABI declared in include/cfgpp.h).

There is NO fallback: if the shared library is missing or a call fails, a
``CfgppError`` is raised.  The product path never routes through ``oracle/``.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CFGPP_LIB") or os.path.join(HERE, "libcfgpp_hip.so")   # CFGPP_LIB: A/B a second build (development only)


class CfgppError(RuntimeError):
    pass


class UNetConfigC(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int), ("out_channels", C.c_int),
        ("num_levels", C.c_int),
        ("block_out_channels", C.c_int * 4),
        ("layers_per_block", C.c_int),
        ("level_has_attn", C.c_int * 4),
        ("transformer_depth", C.c_int * 4),
        ("num_heads", C.c_int * 4),
        ("cross_attention_dim", C.c_int),
        ("addition_embed", C.c_int),
        ("addition_time_embed_dim", C.c_int),
        ("addition_pooled_dim", C.c_int),
        ("norm_groups", C.c_int),
        ("sample_h", C.c_int), ("sample_w", C.c_int),
        ("max_rows", C.c_int),
    ]


_P, _I, _F, _L = C.c_void_p, C.c_int, C.c_float, C.c_long

# name -> (restype, argtypes); every symbol include/cfgpp.h declares (the drop-in boundary)
PROTOTYPES = {
    "cfgpp_last_error": (C.c_char_p, []),
    "cfgpp_build_id": (C.c_char_p, []),
    "cfgpp_step_ddim": (_I, [_P, _P, _P, _P, _I, _F, _F, _F, _F, _F, _I, _I, _L, _P]),
    "cfgpp_step_ddim_h": (_I, [_P, _P, _P, _P, _F, _F, _F, _F, _F, _I, _I, _L, _P]),
    "cfgpp_step_ddim_masked": (_I, [_P, _P, _P, _P, _F, _F, _F, _F, _F, _I, _I, _P, _P, _P, _F, _F, _I, _L, _P]),
    "cfgpp_kdiff_input": (_I, [_P, _P, _F, _I, _L, _P]),
    "cfgpp_step_kdiff": (_I, [_P, _P, _P, _P, _P, C.POINTER(C.c_float), _I, _I, _I, _I, _L, _P]),
    "cfgpp_kdiff_denoise": (_I, [_P, _P, _P, _F, _F, _P, _P, _L, _P]),
    "cfgpp_lincomb": (_I, [_P, _P, _P, _P, _F, _F, _I, _L, _P]),
    "cfgpp_unet_create": (_P, [C.POINTER(UNetConfigC), _I]),
    "cfgpp_unet_destroy": (None, [_P]),
    "cfgpp_unet_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_long), _I]),
    "cfgpp_unet_missing": (_I, [_P]),
    "cfgpp_unet_finalize": (_I, [_P]),
    "cfgpp_unet_set_context": (_I, [_P, _P, _I, _I, _P, _P, _I, _P]),
    "cfgpp_unet_image_condition": (_I, [_P, _P, _I, _P]),
    "cfgpp_unet_forward": (_I, [_P, _P, _I, _I, _F, _P, _I, _P]),
    "cfgpp_sample_graph_ddim": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _I, C.POINTER(C.c_float), _I, _F, _I, _I, _P]),
    "cfgpp_unet_profile": (_I, [_P, _P, _I, _I, _F, _P, _I, _P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_char_p, _L]),
    "cfgpp_unet_tuning": (_I, [_P, _I, C.POINTER(C.c_int), _I, _I]),
    "cfgpp_unet_attach_control": (_I, [_P, _P, _F]),
    "cfgpp_unet_lora": (_I, [_P, C.c_char_p, _P, _P, _I, _P]),
    "cfgpp_unet_flops": (C.c_double, [_P, _I]),
    "cfgpp_unet_device_bytes": (C.c_double, [_P]),
    "cfgpp_vae_create": (_P, [_I, _I, _I, _F, _I]),
    "cfgpp_vae_destroy": (None, [_P]),
    "cfgpp_vae_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_long), _I]),
    "cfgpp_vae_finalize": (_I, [_P]),
    "cfgpp_vae_decode": (_I, [_P, _P, _P, _I, _P]),
    "cfgpp_vae_decode_image": (_I, [_P, _P, _P, _I, _P]),
    "cfgpp_vae_encode": (_I, [_P, _P, _P, _P, _P, _I, _P]),
    "cfgpp_vae_flops": (C.c_double, [_P, _I]),
    "cfgpp_text_create": (_P, [_I, _I, _I, _I, _I, _I, _I, _I, _I]),
    "cfgpp_text_destroy": (None, [_P]),
    "cfgpp_text_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_long), _I]),
    "cfgpp_text_finalize": (_I, [_P]),
    "cfgpp_text_encode": (_I, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), _I, _I, _P, _P, _P]),
    "cfgpp_text_device_bytes": (C.c_double, [_P]),
    "cfgpp_vae_encode_flops": (C.c_double, [_P, _I]),
    "cfgpp_vae_device_bytes": (C.c_double, [_P]),
}

# the IP-Adapter extension header (include/cfgpp_ip_adapter.h): product entry points outside the reference's seam
IP_ADAPTER_PROTOTYPES = {
    "cfgpp_unet_ip_load": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_long), _I]),
    "cfgpp_unet_image_context": (_I, [_P, _P, _I, _I, _F, _P]),
}

# the IP-Adapter "plus" extension header (include/cfgpp_ip_plus.h): the Resampler image projection
IP_PLUS_PROTOTYPES = {
    "cfgpp_unet_image_context_seq": (_I, [_P, _P, _I, _I, _I, _F, _P]),
}

# the long-prompt extension header (include/cfgpp_long_prompt.h)
LONG_PROMPT_PROTOTYPES = {
    "cfgpp_unet_set_max_tokens": (_I, [_P, _I]),
}

# the regional-prompt extension header (include/cfgpp_regions.h)
REGIONS_PROTOTYPES = {
    "cfgpp_unet_set_regions": (_I, [_P, _P, _I, _I]),
}

# the soft regional-prompt extension header (include/cfgpp_regions_soft.h)
REGIONS_SOFT_PROTOTYPES = {
    "cfgpp_unet_enable_region_weights": (_I, [_P]),
    "cfgpp_unet_set_region_weights": (_I, [_P, _P, _I, _I]),
}

# the FreeU extension header (include/cfgpp_freeu.h)
FREEU_PROTOTYPES = {
    "cfgpp_unet_set_freeu": (_I, [_P, _F, _F, _F, _F, _I]),
}

# the v-prediction extension header (include/cfgpp_vpred.h)
VPRED_PROTOTYPES = {
    "cfgpp_step_ddim_v": (_I, [_P, _P, _P, _P, _I, _F, C.POINTER(C.c_float), _I, _I, _P, _L, _L, _P]),
    "cfgpp_v_to_eps": (_I, [_P, _P, _P, _P, _P, _I, _F, _F, _L, _P]),
    "cfgpp_cfg_rescale": (_I, [_P, _P, _F, _F, _P, _I, _L, _P]),
}

# the LCM extension header (include/cfgpp_lcm.h): Philox normals and the fused consistency step
_U, _S = C.c_uint, C.POINTER(C.c_ulonglong)
LCM_PROTOTYPES = {
    "cfgpp_philox_normal": (_I, [_P, _I, _S, _I, _L, _U, _U, _P]),
    "cfgpp_step_lcm": (_I, [_P, _P, _P, _P, _F, C.POINTER(C.c_float), _I, _I, _P, _S, _I, _L, _U, _P]),
    "cfgpp_unet_set_time_cond": (_I, [_P, _I]),
    "cfgpp_unet_guidance_embedding": (_I, [_P, C.POINTER(C.c_float), _P]),
}

# the SDE extension header (include/cfgpp_sde.h): the fused DPM++ 2M / 3M SDE step and the job's first UNet input
SDE_PROTOTYPES = {
    "cfgpp_sde_input": (_I, [_P, _P, _F, _L, _P]),
    "cfgpp_step_sde": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _F, C.POINTER(C.c_float), _I, _I, _I, _P, _S, _I, _L, _U, _P]),
}

# the DPM++ SDE extension header (include/cfgpp_dpmpp_sde.h): one stage of the two-stage stochastic step
DPMPP_SDE_PROTOTYPES = {
    "cfgpp_step_sde_stage": (_I, [_P, _P, _P, _P, _P, _P, _P, _F, C.POINTER(C.c_float), _I, _I, _P, _P, _S, _I, _L, _U, _U, _P]),
}

# the img2img / hires-fix extension header (include/cfgpp_img2img.h): the fused resample + forward-noise start
IMG2IMG_PROTOTYPES = {
    "cfgpp_img2img_start": (_I, [_P, _P, _P, _S, _F, _F, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
}

# the MultiDiffusion panorama extension header (include/cfgpp_panorama.h): the window gather and the fused view step
class PanoViewsC(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("B", "C", "Hp", "Wp", "h", "w", "stride", "circular", "chunk_views")]


PANORAMA_PROTOTYPES = {
    "cfgpp_views_gather": (_I, [C.POINTER(PanoViewsC), _P, _P, _P]),
    "cfgpp_step_ddim_views": (_I, [C.POINTER(PanoViewsC), _P, _P, _P, _P, _F, _F, _F, _F, _F, _I, _I, _P]),
}

# the CLIP image tower extension header (include/cfgpp_vision.h)
VISION_PROTOTYPES = {
    "cfgpp_vision_create": (_P, [_I, _I, _I, _I, _I, _I, _I, _I, _I, _I]),
    "cfgpp_vision_destroy": (None, [_P]),
    "cfgpp_vision_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_long), _I]),
    "cfgpp_vision_finalize": (_I, [_P]),
    "cfgpp_vision_preprocess": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "cfgpp_vision_encode": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "cfgpp_vision_flops": (C.c_double, [_P, _I]),
    "cfgpp_vision_device_bytes": (C.c_double, [_P]),
}

# test hooks and development switches (cfgpp_amd/csrc/cfgpp_debug.h): same library, not part of the boundary
DEBUG_PROTOTYPES = {
    "cfgpp_op_philox_raw": (_I, [_P, C.POINTER(C.c_uint), C.POINTER(C.c_uint), _L, _P]),
    "cfgpp_op_softmax_rows": (_I, [_P, _L, _I, _P]),
    "cfgpp_op_conv_in_ex": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _F, _P]),
    "cfgpp_op_groupnorm": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _I, _P]),
    "cfgpp_op_groupnorm_pre": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _I, _P]),
    "cfgpp_op_igemm_set_gstat": (None, [_P]),
    "cfgpp_op_igemm_gstat_written": (_I, []),
    "cfgpp_groupnorm_set_prestats": (None, [_I]),
    "cfgpp_groupnorm_prestats_enabled": (_I, []),
    "cfgpp_unet_set_share_prefix": (None, [_I]),
    "cfgpp_unet_share_prefix_enabled": (_I, []),
    "cfgpp_unet_shared_prefix_ops": (_I, [_P, _I, _I]),
    "cfgpp_op_layernorm": (_I, [_P, _P, _P, _P, _L, _I, _F, _P]),
    "cfgpp_op_attention_prepare_vt": (_I, [_P, _I, _I, _I, _P]),
    "cfgpp_op_attention": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "cfgpp_op_attention_cross": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "cfgpp_attention_set_cross_long": (None, [_I]),
    "cfgpp_op_attention_clear_slots": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "cfgpp_op_attention_ip": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _F, _I, _I, _P]),
    "cfgpp_op_attention_region": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _P]),
    "cfgpp_op_attention_region_soft": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _P]),
    "cfgpp_op_perceiver_attention": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "cfgpp_op_attention_vit": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "cfgpp_vit_attention_last_launch": (None, [C.POINTER(C.c_int)]),
    "cfgpp_op_vit_preprocess": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "cfgpp_op_vit_patch_rows": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "cfgpp_op_text_embed": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "cfgpp_op_text_attention": (_I, [_P, _P, _I, _I, _I, _P]),
    "cfgpp_op_text_pool": (_I, [_P, _P, _P, _I, _I, _P]),
    "cfgpp_op_act_inplace": (_I, [_P, _L, _I, _P]),
    "cfgpp_op_vit_assemble": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "cfgpp_op_vit_cls_rows": (_I, [_P, _P, _I, _I, _I, _P]),
    "cfgpp_op_gelu_inplace": (_I, [_P, _L, _P]),
    "cfgpp_op_broadcast_rows": (_I, [_P, _P, _L, _I, _P]),
    "cfgpp_unet_ip_tokens": (_I, [_P, _P, _I]),
    "cfgpp_op_conv_in": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "cfgpp_op_conv_in_cond": (_I, [_P, _I, _P, _I, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "cfgpp_op_conv_in_add": (_I, [_P, _I, _P, _I, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "cfgpp_op_cn_conv3x3": (_I, [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "cfgpp_op_residual_add": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int), _I, _I, _F, _P]),
    "cfgpp_op_residual_nchw": (_I, [_P, _P, _I, _I, _I, _I, _F, _P]),
    "cfgpp_controlnet_residual": (_I, [_P, _I, _F, _P, _I, C.POINTER(C.c_int), _P]),
    "cfgpp_vae_profile": (_I, [_P, _P, _P, _I, _P, C.c_char_p, C.c_long]),
    "cfgpp_unet_read_weight": (_I, [_P, C.c_char_p, _P]),
    "cfgpp_op_vae_posterior": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _F, _P]),
    "cfgpp_op_conv_out": (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P]),
    "cfgpp_op_conv_out_ex": (_I, [_P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _F, _I, _P]),
    "cfgpp_conv_out_set_tiled": (None, [_I]),
    "cfgpp_conv_out_last_launch": (None, [C.POINTER(C.c_int)]),
    "cfgpp_op_sinusoid": (_I, [_P, _F, _P, _I, _I, _I, _I, _P]),
    "cfgpp_op_skinny_gemm": (_I, [_P, _I, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P]),
    "cfgpp_op_f16_to_f32_rows": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "cfgpp_op_fanout_rows": (_I, [C.POINTER(C.c_void_p), C.POINTER(C.c_long), _I, _I, _P]),
    "cfgpp_op_igemm": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _I, _P, _P, _I, _P, _I, _I, _P, _I, _I, _I, _P]),
    "cfgpp_op_igemm_heads": (_I, [_P, _I, _P, _I, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "cfgpp_op_igemm_ex": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _I, _P, _P, _I, _P, _I, _I, _P, _I, _I, _I, _I, _F, _I, _P]),
    "cfgpp_op_igemm_heads_ex": (_I, [_P, _I, _P, _I, _I, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "cfgpp_igemm_last_launch": (None, [C.POINTER(C.c_int)]),
    "cfgpp_op_fold_upsample": (_I, [_P, _P, _I, _I, _P]),
    "cfgpp_op_upsample_conv3x3": (_I, [_P, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P]),
    "cfgpp_igemm_set_upsample_phase": (None, [_I]),
    "cfgpp_igemm_last_amode": (_I, []),
    "cfgpp_igemm_last_config_ran": (_I, []),
    "cfgpp_igemm_force_config": (None, [_I]),
    "cfgpp_igemm_set_staging": (None, [_I]),
    "cfgpp_igemm_set_staged_epilogue": (None, [_I]),
    "cfgpp_igemm_set_big_tiles": (None, [_I]),
    "cfgpp_igemm_set_tail_split": (None, [_I]),
    "cfgpp_igemm_set_autotune": (None, [_I]),
    "cfgpp_igemm_set_blocked_walk": (None, [_I]),
    "cfgpp_igemm_walk_plan_probe": (None, [_I, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_int)]),
    "cfgpp_igemm_set_n_major": (None, [_I]),
    "cfgpp_igemm_force_split": (None, [_I]),
    "cfgpp_igemm_set_split_tile": (None, [_I]),
    "cfgpp_igemm_set_mf16": (None, [_I]),
    "cfgpp_igemm_set_mf16_rounds": (None, [_I]),
    "cfgpp_igemm_set_mf16_heads": (None, [_I]),
    "cfgpp_igemm_set_mf16_linear": (None, [_I]),
    "cfgpp_igemm_set_big_split": (None, [_I]),
    "cfgpp_igemm_set_tune_mask": (None, [C.c_uint]),
    "cfgpp_igemm_tuner_state": (C.c_uint, []),
    "cfgpp_igemm_timeline": (None, [_P, _L, _I]),
    "cfgpp_igemm_timeline_info": (None, [C.POINTER(C.c_int)]),
    "cfgpp_groupnorm_set_mode": (None, [_I]),
    "cfgpp_layernorm_set_rows_per_wave": (None, [_I]),
    "cfgpp_attention_set_dma": (None, [_I]),
    "cfgpp_attention_set_stagger": (None, [_I]),
    "cfgpp_attention_set_cross": (None, [_I]),
    "cfgpp_attention_last_launch": (None, [C.POINTER(C.c_int)]),
    "cfgpp_groupnorm_last_launch": (None, [C.POINTER(C.c_int)]),
    "cfgpp_layernorm_last_launch": (None, [C.POINTER(C.c_int)]),
    "cfgpp_softmax_last_launch": (None, [C.POINTER(C.c_int)]),
    "cfgpp_op_freeu": (_I, [_P, _I, _P, _I, _I, _I, _I, _F, _F, _P]),
    "cfgpp_freeu_last_launch": (None, [C.POINTER(C.c_int)]),
}

_lib = None


def load():
    """dlopen the library and attach prototypes.  Raises CfgppError when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CfgppError(
            f"{LIB_PATH} not found: build it with `python -m cfgpp_amd.build` "
            "(__graft_entry__.build()).  The HIP path has no CPU fallback.")
    # torch first: it brings its own copy of the HIP runtime; loaded after libcfgpp_hip.so (which would pull in the system one)
    # the process ends up with two runtimes and the engine cannot use torch's device pointers / streams
    import torch  # noqa: F401
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise CfgppError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in list(PROTOTYPES.items()) + list(IP_ADAPTER_PROTOTYPES.items()) + list(IP_PLUS_PROTOTYPES.items()) + list(LONG_PROMPT_PROTOTYPES.items()) + list(REGIONS_PROTOTYPES.items()) + list(REGIONS_SOFT_PROTOTYPES.items()) + list(FREEU_PROTOTYPES.items()) + list(VPRED_PROTOTYPES.items()) + list(LCM_PROTOTYPES.items()) + list(SDE_PROTOTYPES.items()) + list(DPMPP_SDE_PROTOTYPES.items()) + list(IMG2IMG_PROTOTYPES.items()) + list(PANORAMA_PROTOTYPES.items()) + list(VISION_PROTOTYPES.items()) + list(DEBUG_PROTOTYPES.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise CfgppError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if os.environ.get("CFGPP_AUTOTUNE", "1") == "0":      # e.g. under rocprofv3 --pmc: no timing passes
        lib.cfgpp_igemm_set_autotune(0)
    _lib = lib
    return lib


def build_id() -> str:
    """provenance string of the loaded binary (include/cfgpp.h: cfgpp_build_id)"""
    return load().cfgpp_build_id().decode("utf-8", "replace")


def last_error() -> str:
    return load().cfgpp_last_error().decode("utf-8", "replace")


def check(rc: int, what: str):
    if rc != 0:
        raise CfgppError(f"{what} failed (rc={rc}): {last_error()}")
