"""A diffusers-layout checkpoint directory -> the keyword arguments of ``get_solver``.

The reference builds everything with ``StableDiffusionPipeline.from_pretrained(model_key)`` /
``StableDiffusionXLPipeline.from_pretrained(model_key)`` (latent_diffusion.py:56-66, latent_sdxl.py:40-54).  With a local
copy of such a checkpoint (no hub access here) the same components map onto this package as

    <dir>/unet/diffusion_pytorch_model.safetensors          -> unet_weights=   (HIP UNet engine)
    <dir>/unet/config.json, "in_channels": 9                -> unet_config=    (SD15_INPAINT / SDXL_INPAINT: an inpaint checkpoint)
    <dir>/unet/config.json, cross_attention_dim / attention_head_dim / use_linear_projection / sample_size
                                                            -> unet_config=    (SD21 / SD21_BASE: a Stable Diffusion 2.x UNet)
    <dir>/scheduler/scheduler_config.json                   -> prediction_type= / zero_terminal_snr= / timestep_spacing=
                                                               (only what differs from "epsilon" / false / "leading")
    <dir>/tokenizer/special_tokens_map.json, pad_token      -> the text tower's padding ("!" for SD2.x)
    <dir>/vae/diffusion_pytorch_model.safetensors           -> vae_weights=    (HIP VAE engine; SD1.5 only)
    <dir>/vae_fp16_fix/diffusion_pytorch_model.safetensors  -> vae_weights=    (SDXL: the reference REPLACES the pipeline's VAE with
                                                               madebyollin/sdxl-vae-fp16-fix, latent_sdxl.py:44,396 - the stock
                                                               SDXL VAE overflows in fp16, which is what the HIP VAE computes in;
                                                               <dir>/vae is never used for SDXL unless vae_dir= says so)
    <dir>/text_encoder/{config.json, model.safetensors} + <dir>/tokenizer/{vocab.json, merges.txt}        -> text_encoder=
    <dir>/text_encoder_2/... + <dir>/tokenizer_2/...        (SDXL: second tower, projected pooled output, "!" padding)

On a GPU device the text towers are ``text.HipClipTextTower`` - the CLIP transformer on the engine's own kernels
(csrc/text.hip), pinned against ``transformers`` in tests/test_gpu_text.py; the torch-ops ``ClipTextTower`` is what a CPU
device (tests only) gets.

Missing pieces are left to the solver's defaults (synthetic weights / synthetic text encoder) and reported in ``missing``.
"""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import torch

from ._lib import CfgppError


# filled by solver_kwargs_from_dir: one line per CLIP tower that fell back from the HIP kernels to the torch-ops tower (callers and
# tests can assert on it; the GPU tests pin the HIP tower, so a silent fallback would be a different implementation)
last_text_tower_fallbacks: List[str] = []


def _first(*paths):
    for p in paths:
        if os.path.exists(p):
            return p
    return None


def _weights_in(folder, stem="diffusion_pytorch_model"):
    return _first(os.path.join(folder, stem + ".safetensors"), os.path.join(folder, stem + ".fp16.safetensors"))


def _default_unet_config(sdxl: bool):
    from .unet_config import SD15, SDXL
    return SDXL if sdxl else SD15


def unet_config_from_json(conf: dict, base):
    """``base`` with the fields a diffusers ``unet/config.json`` may set differently inside one family - ``cross_attention_dim``,
    ``attention_head_dim`` (an int or one entry per level: diffusers' name for the head COUNT), ``use_linear_projection``,
    ``sample_size`` - or None when the file describes ``base`` itself.  A config that is one of the named SD2.x ones is returned as
    that object (``SD21``, ``SD21_BASE``)."""
    from dataclasses import replace
    from .unet_config import SD21, SD21_BASE
    L = base.num_levels
    heads = conf.get("attention_head_dim")
    if heads is None:
        heads = base.num_heads
    heads = tuple(int(h) for h in heads) if isinstance(heads, (list, tuple)) else (int(heads),) * L
    if len(heads) != L:
        raise CfgppError(f"unet/config.json: attention_head_dim has {len(heads)} entries for {L} levels")
    lin = conf.get("use_linear_projection")
    lin = base.linear_projection if lin is None or bool(lin) == base.use_linear_projection else bool(lin)
    cand = replace(base, num_heads=heads, cross_attention_dim=int(conf.get("cross_attention_dim") or base.cross_attention_dim),
                   linear_projection=lin, sample_size=int(conf.get("sample_size") or base.sample_size))
    if cand == base:
        return None
    for named in (SD21, SD21_BASE):
        if replace(cand, name=named.name) == named:
            return named
    return replace(cand, name=base.name + "_custom")


def _pad_token(path):
    """the pad token of a ``special_tokens_map.json`` when it is not CLIP's default ``<|endoftext|>`` (None otherwise)"""
    if not os.path.exists(path):
        return None
    import json
    with open(path) as f:
        tok = json.load(f).get("pad_token")
    if isinstance(tok, dict):
        tok = tok.get("content")
    return tok if tok and tok != "<|endoftext|>" else None


def solver_kwargs_from_dir(model_dir, sdxl: bool, device="cuda", vae_dir=None, text_tower: str = "") -> Tuple[Dict, List[str]]:
    """(kwargs for ``get_solver``, names of the components not found).  ``vae_dir``: a folder holding the VAE weights,
    overriding the default lookup (SD1.5: ``<dir>/vae``; SDXL: ``<dir>/vae_fp16_fix`` or ``<dir>/sdxl-vae-fp16-fix`` -
    NEVER ``<dir>/vae``, whose fp16 activations overflow).  ``text_tower`` (or ``$CFGPP_TEXT_TOWER``): ``"hip"`` = the HIP CLIP
    tower or an error, ``"torch"`` = the torch-ops ``ClipTextTower`` even on a GPU; default = the HIP tower on a GPU, and when
    that one cannot take the checkpoint (an activation it has no kernel for, keys of a fine-tune it does not know) the torch-ops
    tower with a logged warning - the text encoder runs once per prompt and is not on the hot path."""
    import logging
    from .conditioning import ClipTextTower
    text_tower = (text_tower or os.environ.get("CFGPP_TEXT_TOWER", "")).lower()
    if text_tower not in ("", "hip", "torch"):
        raise ValueError(f"text_tower={text_tower!r}: expected 'hip', 'torch' or ''")
    d = str(model_dir)
    kw, missing = {}, []
    unet = _weights_in(os.path.join(d, "unet"))
    if vae_dir is not None:
        vae = _weights_in(str(vae_dir))
    elif sdxl:
        vae = _weights_in(os.path.join(d, "vae_fp16_fix")) or _weights_in(os.path.join(d, "sdxl-vae-fp16-fix"))
    else:
        vae = _weights_in(os.path.join(d, "vae"))
    if unet:
        kw["unet_weights"] = unet
    else:
        missing.append("unet")
    ucfg = os.path.join(d, "unet", "config.json")
    if os.path.exists(ucfg):            # an inpaint checkpoint's UNet takes 9 input channels (latent, mask, masked-image latent)
        import json
        with open(ucfg) as f:
            uconf = json.load(f)
        cin = int(uconf.get("in_channels", 4))
        if cin == 9:
            from .unet_config import SD15_INPAINT, SDXL_INPAINT
            kw["unet_config"] = SDXL_INPAINT if sdxl else SD15_INPAINT
        shaped = unet_config_from_json(uconf, kw.get("unet_config") or _default_unet_config(sdxl))
        if shaped is not None:          # an SD2.x UNet, or another head count / context width / projection kind than the family's
            kw["unet_config"] = shaped
        tdim = int(uconf.get("time_cond_proj_dim") or 0)
        if tdim:                        # a guidance-embedded (LCM-distilled) UNet: time_embedding.cond_proj (cfgpp_amd/lcm.py)
            from dataclasses import replace
            from .unet_config import SD15_LCM, SDXL_LCM
            base = kw.get("unet_config") or _default_unet_config(sdxl)
            cand = replace(base, time_cond_proj_dim=tdim)
            named = SDXL_LCM if sdxl else SD15_LCM
            kw["unet_config"] = named if replace(cand, name=named.name) == named else replace(cand, name=base.name + "_lcm")
    # what the UNet predicts and the schedule it was trained on: only what differs from the reference's models is passed on, so a
    # plain SD1.5 / SDXL directory yields the keyword arguments it always did
    scfg = os.path.join(d, "scheduler", "scheduler_config.json")
    if os.path.exists(scfg):
        import json
        with open(scfg) as f:
            sconf = json.load(f)
        pt = sconf.get("prediction_type", "epsilon")
        if pt != "epsilon":
            kw["prediction_type"] = pt          # "v_prediction"; anything else is refused by the solver, by name
        if sconf.get("rescale_betas_zero_snr"):
            kw["zero_terminal_snr"] = True
        if sconf.get("timestep_spacing") == "trailing":
            kw["timestep_spacing"] = "trailing"
        if sconf.get("_class_name") == "LCMScheduler":      # the `lcm` solvers' schedule (cfgpp_amd/lcm.py); other solvers ignore the keys
            kw["lcm_original_steps"] = int(sconf.get("original_inference_steps", 50))
            kw["timestep_scaling"] = float(sconf.get("timestep_scaling", 10.0))
            kw.pop("timestep_spacing", None)                # LCMScheduler's own timesteps: its "leading" default is not DDIM's
    pad_token = _pad_token(os.path.join(d, "tokenizer", "special_tokens_map.json"))
    if pad_token is not None:
        kw["pad_token"] = pad_token             # SD2.x pads with "!" (the solvers ignore the key; the text tower below takes it)
    lora = _first(os.path.join(d, "pytorch_lora_weights.safetensors"), os.path.join(d, "lora.safetensors"))
    if lora:
        # a LoRA file next to the model (diffusers' save_lora_weights name, or lora.safetensors): merged into the UNet at scale 1
        # (get_solver(lora=...)); its text-encoder entries, if any, are set aside - the text encoders take no adapter.  Said aloud,
        # because it changes what the checkpoint computes; the CLIs' --lora replaces it, a caller drops kw["lora"] to opt out
        logging.getLogger("cfgpp_amd").warning("%s: merging the LoRA file found next to the model (%s) at scale 1; pass --lora / "
                                               "lora= to choose adapters yourself", d, os.path.basename(lora))
        kw["lora"] = [(lora, 1.0)]
        kw["lora_ignore_text_encoder"] = True
    if vae:
        kw["vae_weights"] = vae
    else:
        missing.append("vae (SDXL needs madebyollin/sdxl-vae-fp16-fix in <dir>/vae_fp16_fix)" if sdxl else "vae")
    on_gpu = torch.device(device).type == "cuda"
    dtype = torch.float16 if on_gpu else torch.float32          # the reference runs the text encoders in the pipeline's fp16

    fallbacks = last_text_tower_fallbacks
    del fallbacks[:]

    def tower(enc, tok, **args):
        e, t = os.path.join(d, enc), os.path.join(d, tok)
        ok = os.path.exists(os.path.join(e, "config.json")) and _weights_in(e, "model") is not None and \
            all(os.path.exists(os.path.join(t, f)) for f in ("vocab.json", "merges.txt"))
        if not ok:
            missing.append(enc)
            return None
        if on_gpu and text_tower != "torch":
            from .text import HipClipTextTower
            try:
                return HipClipTextTower.from_dir(e, t, device=device, **args)
            except (CfgppError, KeyError, ValueError, NotImplementedError) as exc:
                # "this checkpoint is not one the HIP tower takes" (activation, missing / unexpected keys, shapes).  Anything else -
                # a missing library symbol, a HIP out-of-memory, a bug in the tower - propagates: it must not hide behind a fallback.
                if text_tower == "hip":
                    raise
                fallbacks.append(f"{enc}: torch-ops tower ({type(exc).__name__}: {exc})")
                logging.getLogger("cfgpp_amd").warning("HIP text tower cannot load %s (%s: %s); using the torch-ops ClipTextTower",
                                                       e, type(exc).__name__, exc)
        return ClipTextTower.from_dir(e, t, device=device, dtype=dtype, **args)

    if sdxl:
        t1 = tower("text_encoder", "tokenizer", penultimate=True, with_projection=False)
        t2 = tower("text_encoder_2", "tokenizer_2", penultimate=True, with_projection=True, pad_token="!")
        if t1 is not None and t2 is not None:
            kw["text_encoder"] = (t1, t2)
    else:
        t1 = tower("text_encoder", "tokenizer", penultimate=False, with_projection=False, **({} if pad_token is None else {"pad_token": pad_token}))
        if t1 is not None:
            kw["text_encoder"] = t1
    return kw, missing


def controlnet_config_from_json(conf: dict, base):
    """the ``UNetConfig`` of a diffusers ``ControlNetModel`` config.json (its UNet-shaped fields), starting from the solver's
    UNet config ``base``.  Refuses what the engine does not build, naming the field."""
    from dataclasses import replace
    from .controlnet import EMBED_CHANNELS
    if conf.get("global_pool_conditions"):
        raise CfgppError("controlnet config.json: global_pool_conditions=true (a pooled 'shuffle'-style ControlNet) is not supported")
    if str(conf.get("controlnet_conditioning_channel_order", "rgb")).lower() != "rgb":
        raise CfgppError(f"controlnet config.json: controlnet_conditioning_channel_order={conf['controlnet_conditioning_channel_order']!r} "
                         "is not supported (rgb only)")
    emb = tuple(conf.get("conditioning_embedding_out_channels", EMBED_CHANNELS))
    if emb != EMBED_CHANNELS:
        raise CfgppError(f"controlnet config.json: conditioning_embedding_out_channels={list(emb)} is not supported "
                         f"(the engine builds {list(EMBED_CHANNELS)})")
    if int(conf.get("conditioning_channels", 3)) != 3:
        raise CfgppError(f"controlnet config.json: conditioning_channels={conf['conditioning_channels']} is not supported (3)")
    boc = tuple(int(c) for c in conf.get("block_out_channels", base.block_out_channels))
    L = len(boc)

    def per_level(v, default):
        if v is None:
            return tuple(default)
        return tuple(int(x) for x in v) if isinstance(v, (list, tuple)) else (int(v),) * L

    types_ = conf.get("down_block_types")
    attn = tuple(int("CrossAttn" in t) for t in types_) if types_ else tuple(base.level_has_attn)
    depth = per_level(conf.get("transformer_layers_per_block"), base.transformer_depth)
    heads = per_level(conf.get("num_attention_heads") or conf.get("attention_head_dim"), base.num_heads)   # diffusers' naming quirk
    add = 1 if conf.get("addition_embed_type") == "text_time" else 0
    tdim = int(conf.get("addition_time_embed_dim") or base.addition_time_embed_dim)
    pooled = int(conf["projection_class_embeddings_input_dim"]) - 6 * tdim if add and conf.get("projection_class_embeddings_input_dim") \
        else base.addition_pooled_dim
    return replace(base, name=base.name + "_controlnet", in_channels=int(conf.get("in_channels", base.out_channels)),
                   out_channels=base.out_channels, block_out_channels=boc, layers_per_block=int(conf.get("layers_per_block", base.layers_per_block)),
                   level_has_attn=attn, transformer_depth=depth, num_heads=heads,
                   cross_attention_dim=int(conf.get("cross_attention_dim", base.cross_attention_dim)), addition_embed=add,
                   addition_time_embed_dim=tdim, addition_pooled_dim=pooled, norm_groups=int(conf.get("norm_num_groups", base.norm_groups)))


def controlnet_from_dir(path, base):
    """a diffusers ``controlnet/`` folder (config.json + diffusion_pytorch_model[.fp16].safetensors), or a safetensors file
    (with a config.json next to it, or the solver's UNet config) -> (UNetConfig, state-dict items)"""
    import json
    from .weights import load_safetensors_iter
    folder, weights = (path, _weights_in(path)) if os.path.isdir(path) else (os.path.dirname(path), path)
    if not weights or not os.path.exists(weights):
        raise CfgppError(f"controlnet: no diffusion_pytorch_model[.fp16].safetensors in {path}")
    conf_path = os.path.join(folder, "config.json")
    cfg = base
    if os.path.exists(conf_path):
        with open(conf_path) as f:
            cfg = controlnet_config_from_json(json.load(f), base)
    return cfg, load_safetensors_iter(weights)
