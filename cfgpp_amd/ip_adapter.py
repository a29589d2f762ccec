"""IP-Adapter image prompts for the HIP UNet (diffusers ``load_ip_adapter`` with ``ip-adapter_sd15`` / ``ip-adapter_sdxl`` /
``ip-adapter_sdxl_vit-h``): parsing of the published checkpoints into the engine's keys (include/cfgpp_ip_adapter.h: cfgpp_unet_ip_load),
a seeded synthetic adapter for tests, and the CLIP image tower that turns a picture into ``image_embeds``.

No reference counterpart: the reference conditions on text only.

Checkpoint layout (h94/IP-Adapter ``*.safetensors`` / ``*.bin``): two groups, ``image_proj`` (``proj.weight`` [n_img * cross,
embed], ``proj.bias``, ``norm.weight``, ``norm.bias``) and ``ip_adapter`` (``<id>.to_k_ip.weight`` / ``<id>.to_v_ip.weight``),
nested in one dict or flattened with those prefixes.

[D] The numeric ids are positions in diffusers' ``unet.attn_processors``: every attention module contributes attn1 (even
position, no adapter weights) and attn2 (odd position), so cross-attention block i has id 2 * i + 1, the blocks counted in
the order down blocks, UP blocks, then the mid block LAST; within each, attention modules in order, then ``transformer_blocks.k``
in order.  This order is knowledge of diffusers and of the IP-Adapter repository, not read from source that ships with this
project: it is kept in ONE table, :func:`block_table`, which the parser and the tests both read.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from ._lib import CfgppError
from .unet_config import UNetConfig

MAX_IMAGE_TOKENS = 32            # key slots [96, 128) of the cross-attention buffers
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def block_table(cfg: UNetConfig) -> List[Tuple[int, str]]:
    """[D] [(checkpoint id, diffusers transformer-block name)] of every cross-attention, in ``unet.attn_processors`` order"""
    L = cfg.num_levels
    names = []
    for i in range(L):
        if cfg.level_has_attn[i]:
            for j in range(cfg.layers_per_block):
                names += [f"down_blocks.{i}.attentions.{j}.transformer_blocks.{k}" for k in range(cfg.transformer_depth[i])]
    for i in range(L):
        lvl = L - 1 - i
        if cfg.level_has_attn[lvl]:
            for j in range(cfg.layers_per_block + 1):
                names += [f"up_blocks.{i}.attentions.{j}.transformer_blocks.{k}" for k in range(cfg.transformer_depth[lvl])]
    names += [f"mid_block.attentions.0.transformer_blocks.{k}" for k in range(cfg.transformer_depth[-1])]
    return [(2 * i + 1, n) for i, n in enumerate(names)]


class ParsedIPAdapter(dict):
    """engine key -> tensor (``image_proj.*``, ``<block>.attn2.to_k_ip.weight`` / ``.to_v_ip.weight``), plus the geometry"""
    n_img: int = 0
    embed_dim: int = 0


def _flatten(src) -> Dict[str, torch.Tensor]:
    if isinstance(src, str):
        from safetensors import safe_open
        out = {}
        with safe_open(src, framework="pt", device="cpu") as f:
            for k in f.keys():
                out[k] = f.get_tensor(k)
        return out
    if not isinstance(src, dict):
        raise CfgppError(f"ip_adapter: expected a safetensors path or a state dict, got {type(src).__name__}")
    if "image_proj" in src or "ip_adapter" in src:
        out = {}
        for grp in ("image_proj", "ip_adapter"):
            for k, v in (src.get(grp) or {}).items():
                out[f"{grp}.{k}"] = v
        return out
    return dict(src)


def parse_ip_adapter(src, cfg: UNetConfig) -> ParsedIPAdapter:
    """``src``: safetensors path, nested ``{"image_proj": ..., "ip_adapter": ...}`` dict or flat dict with those prefixes."""
    if isinstance(src, ParsedIPAdapter):
        return src
    flat = _flatten(src)
    if any(k.startswith("image_proj.latents") for k in flat):
        raise CfgppError("ip_adapter: this is a Resampler (\"plus\" / \"plus-face\") adapter (image_proj.latents): only the Linear + LayerNorm "
                         "image projection of ip-adapter_sd15 / ip-adapter_sdxl / ip-adapter_sdxl_vit-h is supported")
    if any(k.startswith("image_proj.proj.0.") for k in flat):
        raise CfgppError("ip_adapter: this is a FaceID / MLP-projection adapter (image_proj.proj.0.weight): not supported")
    for k in ("image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias"):
        if k not in flat:
            raise CfgppError(f"ip_adapter: {k} is missing")
    cross = cfg.cross_attention_dim
    w = flat["image_proj.proj.weight"]
    got_cross = int(flat["image_proj.norm.weight"].shape[0])
    if got_cross != cross or w.dim() != 2 or int(w.shape[0]) % cross != 0:
        raise CfgppError(f"ip_adapter: cross_dim {got_cross} (image_proj.norm) / proj rows {tuple(w.shape)} do not match the UNet's "
                         f"cross_attention_dim {cross} ({cfg.name})")
    n_img = int(w.shape[0]) // cross
    if n_img > MAX_IMAGE_TOKENS or n_img < 1:
        raise CfgppError(f"ip_adapter: {n_img} image tokens (1 .. {MAX_IMAGE_TOKENS} fit the cross-attention key slots)")
    table = block_table(cfg)
    ids = sorted({int(k.split(".")[1]) for k in flat if k.startswith("ip_adapter.") and k.split(".")[1].isdigit()})
    if ids != [i for i, _ in table]:
        raise CfgppError(f"ip_adapter: block count {len(ids)} (ids {ids[:3]} .. {ids[-3:] if ids else []}) does not match the UNet's "
                         f"{len(table)} cross-attention blocks ({cfg.name})")
    out = ParsedIPAdapter()
    for k in ("image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias"):
        out[k] = flat[k]
    for i, name in table:
        for part in ("to_k_ip", "to_v_ip"):
            k = f"ip_adapter.{i}.{part}.weight"
            if k not in flat:
                raise CfgppError(f"ip_adapter: {k} is missing")
            if int(flat[k].shape[1]) != cross:
                raise CfgppError(f"ip_adapter: {k} has cross_dim {int(flat[k].shape[1])}, the UNet's cross_attention_dim is {cross}")
            out[f"{name}.attn2.{part}.weight"] = flat[k]
    out.n_img, out.embed_dim = n_img, int(w.shape[1])
    return out


def synthetic_ip_adapter(cfg: UNetConfig, n_img: int = 4, embed_dim: Optional[int] = None, seed: int = 0) -> Dict[str, Dict[str, torch.Tensor]]:
    """a seeded adapter in the published nested checkpoint form (fp16-representable fp32 values, as weights.synth_tensor)"""
    from .weights import synth_tensor
    cross = cfg.cross_attention_dim
    embed_dim = int(embed_dim or max(64, cross))
    C = {}
    L = cfg.num_levels
    for i, name in block_table(cfg):
        blk = name.split(".")
        lvl = int(blk[1]) if blk[0] == "down_blocks" else (L - 1 - int(blk[1]) if blk[0] == "up_blocks" else L - 1)
        C[i] = cfg.block_out_channels[lvl]
    ip = {}
    for i, c in C.items():
        ip[f"{i}.to_k_ip.weight"] = synth_tensor(f"ip_adapter.{i}.to_k_ip.weight", (c, cross), seed)
        ip[f"{i}.to_v_ip.weight"] = synth_tensor(f"ip_adapter.{i}.to_v_ip.weight", (c, cross), seed)
    proj = {"proj.weight": synth_tensor("image_proj.proj.weight", (n_img * cross, embed_dim), seed),
            "proj.bias": synth_tensor("image_proj.proj.bias", (n_img * cross,), seed),
            "norm.weight": synth_tensor("image_proj.norm.weight", (cross,), seed),
            "norm.bias": synth_tensor("image_proj.norm.bias", (cross,), seed)}
    return {"image_proj": proj, "ip_adapter": ip}


def resolve(spec, cfg: UNetConfig) -> Optional[ParsedIPAdapter]:
    """``spec`` of get_solver / set_ip_adapter: None, "synthetic", a path, a state dict or a parsed adapter"""
    if spec is None:
        return None
    if isinstance(spec, str) and spec == "synthetic":
        spec = synthetic_ip_adapter(cfg)
    return parse_ip_adapter(spec, cfg)


def assemble_embeds(pos: torch.Tensor, neg: Optional[torch.Tensor], B: int) -> torch.Tensor:
    """[2B, embed] fp16: the uc rows first (``negative`` embeds; None = zeros, diffusers' ``torch.zeros_like`` before the
    projection, so the uncond tokens are LayerNorm(proj.bias)), then the c rows; one row broadcasts to B chains"""
    if pos.dim() == 3 and pos.shape[1] == 1:
        pos = pos[:, 0]
    if pos.dim() != 2 or int(pos.shape[0]) not in (1, B):
        raise CfgppError(f"ip_adapter_image_embeds: shape {tuple(pos.shape)}, expected [1 or {B}, embed_dim]")
    if neg is None:
        neg = torch.zeros_like(pos)
    if tuple(neg.shape) != tuple(pos.shape):
        raise CfgppError(f"negative_ip_adapter_image_embeds: shape {tuple(neg.shape)} != {tuple(pos.shape)}")
    return torch.cat([neg.expand(B, -1), pos.expand(B, -1)], 0).to(torch.float16).contiguous()


# ---- the image tower (torch ops, once per job; a HIP vision tower is out of scope) ---------------------------------------
def preprocess_image(image: torch.Tensor, size: int = 224) -> torch.Tensor:
    """[N, 3, H, W] in [0, 1] -> CLIP input [N, 3, size, size]: short side to ``size`` (torch bicubic, antialiased), centre crop,
    CLIP mean / std.  Not bit-identical to CLIPImageProcessor, which resizes with PIL."""
    if image.dim() != 4 or image.shape[1] != 3:
        raise CfgppError(f"ip_adapter_image: shape {tuple(image.shape)}, expected [N, 3, H, W] in [0, 1]")
    x = image.float()
    H, W = int(x.shape[2]), int(x.shape[3])
    s = size / min(H, W)
    nh, nw = max(size, round(H * s)), max(size, round(W * s))
    x = torch.nn.functional.interpolate(x, size=(nh, nw), mode="bicubic", align_corners=False, antialias=True).clamp(0, 1)
    t, l = (nh - size) // 2, (nw - size) // 2
    x = x[:, :, t:t + size, l:l + size]
    mean = torch.tensor(CLIP_MEAN, device=x.device)[None, :, None, None]
    std = torch.tensor(CLIP_STD, device=x.device)[None, :, None, None]
    return (x - mean) / std


class ImageEncoder:
    """``transformers.CLIPVisionModelWithProjection`` from a local ``image_encoder/`` folder, in torch-ROCm: the torch-ops part of
    an image-prompted job (as the text tower's fallback is), run once per job."""

    torch_ops = True

    def __init__(self, folder: str, device="cuda"):
        import os
        from transformers import CLIPVisionModelWithProjection
        path = os.path.join(folder, "image_encoder") if os.path.isdir(os.path.join(folder, "image_encoder")) else folder
        self.model = CLIPVisionModelWithProjection.from_pretrained(path, local_files_only=True, torch_dtype=torch.float16).to(device).eval()
        self.device = device

    @torch.no_grad()
    def __call__(self, image: torch.Tensor) -> torch.Tensor:
        x = preprocess_image(image.to(self.device)).to(torch.float16)
        return self.model(pixel_values=x).image_embeds
