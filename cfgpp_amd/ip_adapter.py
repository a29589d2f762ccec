"""IP-Adapter image prompts for the HIP UNet (diffusers ``load_ip_adapter`` with ``ip-adapter_sd15`` / ``ip-adapter_sdxl`` /
``ip-adapter_sdxl_vit-h`` and the Resampler "plus" family ``ip-adapter-plus_sd15`` / ``ip-adapter-plus-face_sd15`` /
``ip-adapter-plus_sdxl_vit-h`` / ``ip-adapter-plus-face_sdxl_vit-h``, include/cfgpp_ip_plus.h): parsing of the published checkpoints into the engine's keys (include/cfgpp_ip_adapter.h: cfgpp_unet_ip_load),
a seeded synthetic adapter for tests, and the CLIP image tower that turns a picture into ``image_embeds``.

No reference counterpart: the reference conditions on text only.

Checkpoint layout (h94/IP-Adapter ``*.safetensors`` / ``*.bin``): two groups, ``image_proj`` (``proj.weight`` [n_img * cross,
embed], ``proj.bias``, ``norm.weight``, ``norm.bias``) and ``ip_adapter`` (``<id>.to_k_ip.weight`` / ``<id>.to_v_ip.weight``),
nested in one dict or flattened with those prefixes.  A "plus" checkpoint has a Perceiver Resampler as its ``image_proj`` instead:
``latents`` [1, n_q, D], ``proj_in``, ``proj_out``, ``norm_out`` and ``layers.<i>.0`` (PerceiverAttention: ``norm1``, ``norm2``, ``to_q``,
``to_kv``, ``to_out``) / ``layers.<i>.1`` (FeedForward: ``0`` LayerNorm, ``1`` and ``3`` bias-free Linears around an erf GELU); it takes
the image tower's penultimate hidden states [rows, seq, E] instead of the pooled embeds.

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
    kind: str = "linear"             # "linear" (Linear + LayerNorm ImageProjection) | "resampler" ("plus" / "plus-face")
    hidden_dim: int = 0              # Resampler: D, the width of the latents
    heads: int = 0                   # Resampler: inner / 64
    depth: int = 0                   # Resampler: number of layers
    ff_inner: int = 0
    seq_input: bool = False          # True: the adapter takes hidden states [rows, seq, embed_dim], not pooled embeds [rows, embed_dim]


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


RESAMPLER_DIM_HEAD = 64          # dim_head of every published Resampler
RESAMPLER_MAX_DEPTH = 8
_RES_GLOBAL = ("latents", "proj_in.weight", "proj_in.bias", "proj_out.weight", "proj_out.bias", "norm_out.weight", "norm_out.bias")
_RES_LAYER = ("0.norm1.weight", "0.norm1.bias", "0.norm2.weight", "0.norm2.bias", "0.to_q.weight", "0.to_kv.weight", "0.to_out.weight",
              "1.0.weight", "1.0.bias", "1.1.weight", "1.3.weight")


def _attn_blocks(flat, cfg: UNetConfig, out: "ParsedIPAdapter") -> None:
    """the ``ip_adapter`` group: to_k_ip / to_v_ip of every cross-attention, checkpoint ids -> engine block names"""
    cross = cfg.cross_attention_dim
    table = block_table(cfg)
    ids = sorted({int(k.split(".")[1]) for k in flat if k.startswith("ip_adapter.") and k.split(".")[1].isdigit()})
    if ids != [i for i, _ in table]:
        raise CfgppError(f"ip_adapter: block count {len(ids)} (ids {ids[:3]} .. {ids[-3:] if ids else []}) does not match the UNet's "
                         f"{len(table)} cross-attention blocks ({cfg.name})")
    for i, name in table:
        for part in ("to_k_ip", "to_v_ip"):
            k = f"ip_adapter.{i}.{part}.weight"
            if k not in flat:
                raise CfgppError(f"ip_adapter: {k} is missing")
            if int(flat[k].shape[1]) != cross:
                raise CfgppError(f"ip_adapter: {k} has cross_dim {int(flat[k].shape[1])}, the UNet's cross_attention_dim is {cross}")
            out[f"{name}.attn2.{part}.weight"] = flat[k]


def _parse_resampler(flat, cfg: UNetConfig) -> "ParsedIPAdapter":
    """a "plus" checkpoint: geometry from the tensors' shapes (E = proj_in columns, D and n_q from latents, depth = number of
    layers.<i>, inner = to_q rows, heads = inner / 64, ff_inner = layers.<i>.1.1 rows, cross = norm_out), every refusal by name"""
    pre = "Resampler adapter (image_proj.latents present)"
    P = "image_proj."

    def shape(k):
        return tuple(int(x) for x in flat[P + k].shape)

    for k in _RES_GLOBAL:
        if P + k not in flat:
            raise CfgppError(f"ip_adapter: {pre}: {P}{k} is missing")
    layer_ids = sorted({int(k.split(".")[2]) for k in flat if k.startswith(P + "layers.") and k.split(".")[2].isdigit()})
    depth = len(layer_ids)
    if depth < 1 or depth > RESAMPLER_MAX_DEPTH or layer_ids != list(range(depth)):
        raise CfgppError(f"ip_adapter: {pre}: depth {depth} (layers {layer_ids}): 1 .. {RESAMPLER_MAX_DEPTH} layers numbered from 0 are supported")
    for i in range(depth):
        for k in _RES_LAYER:
            if f"{P}layers.{i}.{k}" not in flat:
                raise CfgppError(f"ip_adapter: {pre}: {P}layers.{i}.{k} is missing")
    lat = shape("latents")
    if len(lat) == 3 and lat[0] == 1:
        lat = lat[1:]
    if len(lat) != 2:
        raise CfgppError(f"ip_adapter: {pre}: {P}latents has shape {shape('latents')}, expected [1, n_q, D]")
    n_q, D = lat
    if n_q < 1 or n_q > MAX_IMAGE_TOKENS:
        raise CfgppError(f"ip_adapter: {pre}: n_q = {n_q} image tokens (1 .. {MAX_IMAGE_TOKENS} fit the cross-attention key slots)")
    pin = shape("proj_in.weight")
    if len(pin) != 2 or pin[0] != D:
        raise CfgppError(f"ip_adapter: {pre}: {P}proj_in.weight has shape {pin}, expected [D = {D}, E]")
    E = pin[1]
    inner = shape("layers.0.0.to_q.weight")[0]
    ff = shape("layers.0.1.1.weight")[0]
    for name, v in (("D", D), ("E", E), ("inner", inner), ("ff_inner", ff)):
        if v < 64 or v % 64 != 0:
            raise CfgppError(f"ip_adapter: {pre}: {name} = {v} is not a multiple of 64 (heads are {RESAMPLER_DIM_HEAD} wide, GEMM operands 64-channel blocks)")
    cross = cfg.cross_attention_dim
    got_cross = shape("norm_out.weight")[0]
    if got_cross != cross:
        raise CfgppError(f"ip_adapter: {pre}: norm_out length {got_cross} does not match the UNet's cross_attention_dim {cross} ({cfg.name})")
    kv_rows = shape("layers.0.0.to_kv.weight")[0]
    if kv_rows != 2 * inner:
        raise CfgppError(f"ip_adapter: {pre}: {P}layers.0.0.to_kv.weight has {kv_rows} rows, expected 2 * inner = {2 * inner} (to_q has {inner})")
    want_g = {"proj_in.bias": (D,), "proj_out.weight": (cross, D), "proj_out.bias": (cross,), "norm_out.weight": (cross,), "norm_out.bias": (cross,)}
    for k, w in want_g.items():
        if shape(k) != w:
            raise CfgppError(f"ip_adapter: {pre}: {P}{k} has shape {shape(k)}, expected {w}")
    want_l = {"0.norm1.weight": (D,), "0.norm1.bias": (D,), "0.norm2.weight": (D,), "0.norm2.bias": (D,), "0.to_q.weight": (inner, D),
              "0.to_kv.weight": (2 * inner, D), "0.to_out.weight": (D, inner), "1.0.weight": (D,), "1.0.bias": (D,), "1.1.weight": (ff, D),
              "1.3.weight": (D, ff)}
    for i in range(depth):
        for k, w in want_l.items():
            if shape(f"layers.{i}.{k}") != w:
                raise CfgppError(f"ip_adapter: {pre}: {P}layers.{i}.{k} has shape {shape(f'layers.{i}.{k}')}, layer 0 fixes {w} "
                                 "(layers whose shapes disagree with layer 0 are refused)")
    out = ParsedIPAdapter()
    for k in _RES_GLOBAL:
        out[P + k] = flat[P + k]
    for i in range(depth):
        for k in _RES_LAYER:
            out[f"{P}layers.{i}.{k}"] = flat[f"{P}layers.{i}.{k}"]
    _attn_blocks(flat, cfg, out)
    out.n_img, out.embed_dim = n_q, E
    out.kind, out.hidden_dim, out.heads, out.depth, out.ff_inner, out.seq_input = "resampler", D, inner // RESAMPLER_DIM_HEAD, depth, ff, True
    return out


def parse_ip_adapter(src, cfg: UNetConfig) -> ParsedIPAdapter:
    """``src``: safetensors path, nested ``{"image_proj": ..., "ip_adapter": ...}`` dict or flat dict with those prefixes."""
    if isinstance(src, ParsedIPAdapter):
        return src
    flat = _flatten(src)
    if any(k.startswith("image_proj.proj.0.") for k in flat):
        raise CfgppError("ip_adapter: this is a FaceID / MLP-projection adapter (image_proj.proj.0.weight): not supported")
    if any(k.startswith("image_proj.latents") for k in flat):
        return _parse_resampler(flat, cfg)
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
    out = ParsedIPAdapter()
    for k in ("image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias"):
        out[k] = flat[k]
    _attn_blocks(flat, cfg, out)
    out.n_img, out.embed_dim = n_img, int(w.shape[1])
    return out


def synthetic_ip_adapter(cfg: UNetConfig, n_img: Optional[int] = None, embed_dim: Optional[int] = None, seed: int = 0, kind: str = "linear",
                         hidden_dim: int = 128, heads: int = 2, depth: int = 2, ff_mult: int = 4) -> Dict[str, Dict[str, torch.Tensor]]:
    """a seeded adapter in the published nested checkpoint form (fp16-representable fp32 values, as weights.synth_tensor).
    ``kind="linear"`` (n_img 4, embed_dim max(64, cross)): the Linear + LayerNorm projection.  ``kind="plus"`` (n_img 16, embed_dim
    128, and ``hidden_dim`` / ``heads`` / ``depth`` / ``ff_mult``): a Resampler, latents ~ D^-1/2 as published, matrices at fan-in
    scale, so every LayerNorm sees O(1) rows and the tokens depend on the hidden states at O(1)."""
    from .weights import synth_tensor
    if kind not in ("linear", "plus"):
        raise CfgppError(f"synthetic_ip_adapter: kind {kind!r} ('linear' or 'plus')")
    cross = cfg.cross_attention_dim
    if kind == "plus":
        n_img, embed_dim = int(n_img or 16), int(embed_dim or 128)
    else:
        n_img = int(n_img or 4)
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
    if kind == "plus":
        D, inner, ff = int(hidden_dim), int(heads) * RESAMPLER_DIM_HEAD, int(ff_mult) * int(hidden_dim)

        def T(name, shape, as_key=None):
            return synth_tensor("image_proj." + (as_key or name), shape, seed)

        g = torch.Generator().manual_seed(seed + 4242)
        res = {"latents": (torch.randn((1, n_img, D), generator=g) / D ** 0.5).half().float(),
               "proj_in.weight": T("proj_in.weight", (D, embed_dim)), "proj_in.bias": T("proj_in.bias", (D,)),
               "proj_out.weight": T("proj_out.weight", (cross, D), "proj_out_lin.weight"), "proj_out.bias": T("proj_out.bias", (cross,)),
               "norm_out.weight": T("norm_out.weight", (cross,)), "norm_out.bias": T("norm_out.bias", (cross,))}
        for i in range(int(depth)):
            p = f"layers.{i}."
            for n in ("norm1", "norm2"):
                res[p + f"0.{n}.weight"] = T(p + f"0.{n}.weight", (D,))
                res[p + f"0.{n}.bias"] = T(p + f"0.{n}.bias", (D,))
            # q / k at 2x fan-in scale: scores of O(1) spread, so the softmax is neither flat nor one-hot
            res[p + "0.to_q.weight"] = (2.0 * T(p + "0.to_q.weight", (inner, D))).half().float()
            res[p + "0.to_kv.weight"] = (2.0 * T(p + "0.to_kv.weight", (2 * inner, D))).half().float()
            res[p + "0.to_out.weight"] = T(p + "0.to_out.weight", (D, inner))
            res[p + "1.0.weight"] = T(p + "1.0.weight", (D,), p + "1.0.norm.weight")        # (the FeedForward's LayerNorm: synth_tensor
            res[p + "1.0.bias"] = T(p + "1.0.bias", (D,), p + "1.0.norm.bias")              # recognises norms by ".norm" in the key)
            res[p + "1.1.weight"] = T(p + "1.1.weight", (ff, D))
            res[p + "1.3.weight"] = T(p + "1.3.weight", (D, ff))
        return {"image_proj": res, "ip_adapter": ip}
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
    elif isinstance(spec, str) and spec == "synthetic_plus":
        spec = synthetic_ip_adapter(cfg, kind="plus")
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


def assemble_hidden(pos: torch.Tensor, neg: Optional[torch.Tensor], B: int) -> torch.Tensor:
    """the Resampler form of :func:`assemble_embeds`: hidden states [1 or B, seq, embed] -> [2B, seq, embed] fp16, the uc rows
    (``negative``; None = zeros of the same shape) first; one row broadcasts to B chains.  A 2-D tensor is refused: a Resampler
    adapter reads the image tower's token sequence, not the pooled embeds."""
    if pos.dim() != 3 or int(pos.shape[0]) not in (1, B):
        raise CfgppError(f"ip_adapter_image_embeds: shape {tuple(pos.shape)}, a Resampler (\"plus\") adapter expects the image tower's "
                         f"penultimate hidden states [1 or {B}, seq, embed_dim]")
    if neg is None:
        neg = torch.zeros_like(pos)
    if tuple(neg.shape) != tuple(pos.shape):
        raise CfgppError(f"negative_ip_adapter_image_embeds: shape {tuple(neg.shape)} != {tuple(pos.shape)}")
    return torch.cat([neg.expand(B, -1, -1), pos.expand(B, -1, -1)], 0).to(torch.float16).contiguous()


# ---- the image tower in torch ops (CPU devices and the fallback; on a GPU the solvers build vision.HipClipImageTower) ------
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
    def __call__(self, image: torch.Tensor, hidden: bool = False) -> torch.Tensor:
        """``image_embeds`` [N, projection_dim]; with ``hidden=True`` the penultimate hidden states ``hidden_states[-2]``
        [N, 1 + patches, hidden_size], which is what a Resampler ("plus") adapter reads."""
        x = preprocess_image(image.to(self.device)).to(self.model.dtype)
        return self.encode_pixels(x, hidden)

    @torch.no_grad()
    def encode_pixels(self, pixel_values: torch.Tensor, hidden: bool = False) -> torch.Tensor:
        """the tower on an already preprocessed pixel tensor [N, 3, size, size]"""
        if hidden:
            return self.model(pixel_values=pixel_values, output_hidden_states=True).hidden_states[-2]
        return self.model(pixel_values=pixel_values).image_embeds

    @torch.no_grad()
    def negative_hidden(self, image: torch.Tensor) -> torch.Tensor:
        """the default negative of a Resampler adapter: the tower's hidden states of an ALL-ZERO PIXEL tensor - the published
        pipeline's ``torch.zeros_like`` of the preprocessed image - and NOT zeros of the hidden states."""
        x = preprocess_image(image.to(self.device)).to(self.model.dtype)
        return self.encode_pixels(torch.zeros_like(x), hidden=True)
