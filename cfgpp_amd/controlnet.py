"""ControlNet on the HIP path: diffusers ``ControlNetModel`` (one net, non-guess mode) as a UNet engine built in control
mode, attached to the UNet engine of a solver.

A ControlNet is the UNet's conv_in, time (+ added-condition) embedding, down blocks and mid block - the same diffusers keys -
plus ``controlnet_cond_embedding`` (a small conv stack on the control image, once per job) whose output is added to conv_in's,
and one 1x1 "zero convolution" per skip connection (``controlnet_down_blocks.N``) and for the mid block
(``controlnet_mid_block``).  Its outputs, times ``conditioning_scale``, are added to the UNet's skip connections and mid-block
output (include/cfgpp.h: cfgpp_unet_attach_control).
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Iterable, Optional, Tuple

import torch

from . import _lib
from ._lib import CfgppError, check
from .engine import HipUNet, _stream_ptr, unet_config_c
from .unet_config import UNetConfig, param_shapes
from .weights import synth_tensor

# diffusers ControlNetModel's default conditioning_embedding_out_channels - the only embedding the engine builds
EMBED_CHANNELS = (16, 32, 96, 256)


def _skip_channels(cfg: UNetConfig):
    """channels of the UNet's skip connections in diffusers' down_block_res_samples order"""
    c0 = cfg.block_out_channels[0]
    out = [c0]
    for i, co in enumerate(cfg.block_out_channels):
        out += [co] * cfg.layers_per_block
        if i != cfg.num_levels - 1:
            out.append(co)
    return out


def num_down_residuals(cfg: UNetConfig) -> int:
    return len(_skip_channels(cfg))


def controlnet_param_shapes(cfg: UNetConfig, embed_channels: Tuple[int, ...] = EMBED_CHANNELS) -> "OrderedDict[str, tuple]":
    """diffusers ``ControlNetModel`` state-dict key -> shape: the UNet's keys up to the mid block (``unet_config.param_shapes``),
    the conditioning embedding and the zero convolutions."""
    P: "OrderedDict[str, tuple]" = OrderedDict()
    for k, s in param_shapes(cfg).items():
        if k.startswith(("up_blocks.", "conv_norm_out.", "conv_out.", "time_embedding.cond_proj.")):     # (a ControlNet has no guidance embedding)
            continue
        P[k] = s

    def conv(p, o, i, k):
        P[p + ".weight"] = (o, i, k, k)
        P[p + ".bias"] = (o,)

    e = tuple(int(c) for c in embed_channels)
    q = "controlnet_cond_embedding."
    conv(q + "conv_in", e[0], 3, 3)
    for i in range(len(e) - 1):
        conv(f"{q}blocks.{2 * i}", e[i], e[i], 3)
        conv(f"{q}blocks.{2 * i + 1}", e[i + 1], e[i], 3)
    conv(q + "conv_out", cfg.block_out_channels[0], e[-1], 3)
    for k, c in enumerate(_skip_channels(cfg)):
        conv(f"controlnet_down_blocks.{k}", c, c, 1)
    cm = cfg.block_out_channels[-1]
    conv("controlnet_mid_block", cm, cm, 1)
    return P


def controlnet_param_count(cfg: UNetConfig, embed_channels: Tuple[int, ...] = EMBED_CHANNELS) -> int:
    n = 0
    for s in controlnet_param_shapes(cfg, embed_channels).values():
        k = 1
        for d in s:
            k *= d
        n += k
    return n


def synth_controlnet_state_dict(cfg: UNetConfig, seed: int = 0, embed_channels: Tuple[int, ...] = EMBED_CHANNELS):
    """seeded synthetic ControlNet weights (weights.synth_tensor's initialisation).  The zero convolutions are NOT zero: a
    trained ControlNet has moved away from its zero start, and zero residuals would make every parity test pass vacuously."""
    return OrderedDict((k, synth_tensor("controlnet:" + k, s, seed)) for k, s in controlnet_param_shapes(cfg, embed_channels).items())


class HipControlNet:
    """A ControlNet on the HIP engine (include/cfgpp.h: cfgpp_unet_create with out_channels = 0).  Mirrors ``engine.HipUNet``:
    load weights, finalize, ``set_context`` (the same conditioning as the UNet), ``set_image`` once per job, then attach it to a
    UNet of the same geometry (``HipUNet.attach_control``)."""

    def __init__(self, cfg: UNetConfig, max_rows: int, sample_hw: Optional[Tuple[int, int]] = None, device: int = 0,
                 embed_channels: Tuple[int, ...] = EMBED_CHANNELS, max_tokens: int = 77):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise CfgppError("HipControlNet needs a ROCm GPU; the HIP path has no CPU fallback")
        if tuple(embed_channels) != EMBED_CHANNELS:
            raise CfgppError(f"HipControlNet: conditioning_embedding_out_channels={tuple(embed_channels)}: the engine builds "
                             f"diffusers' default {EMBED_CHANNELS} only")
        if cfg.in_channels != cfg.out_channels:
            raise CfgppError(f"HipControlNet: {cfg.name} is an inpaint UNet config (in_channels {cfg.in_channels}); "
                             "a ControlNet takes the plain latent")
        self.cfg = cfg
        self.device = int(device)
        self.max_rows = int(max_rows)
        H, W = sample_hw if sample_hw is not None else (cfg.sample_size, cfg.sample_size)
        self.H, self.W = int(H), int(W)
        self.image_hw = (self.H * 8, self.W * 8)
        cc = unet_config_c(cfg, self.H, self.W, self.max_rows, out_channels=0)
        self._h = self.lib.cfgpp_unet_create(C.byref(cc), self.device)
        if not self._h:
            raise CfgppError("cfgpp_unet_create (ControlNet) failed: " + _lib.last_error())
        self._keep = {}
        self.finalized = False
        self.max_tokens = 77
        if int(max_tokens) != 77:      # the UNet's: both see the same text context
            self.set_max_tokens(max_tokens)
        self.rows = 0
        self.image_rows = 0

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                torch.cuda.synchronize()
            except Exception:
                pass
            self.lib.cfgpp_unet_destroy(h)
            self._h = None

    def load_tensor(self, key: str, t: torch.Tensor):
        t = t.detach().cpu().contiguous()
        if t.dtype == torch.float16:
            dt = 1
        else:
            t = t.to(torch.float32)
            dt = 0
        shape = (C.c_long * t.dim())(*t.shape)
        check(self.lib.cfgpp_unet_load_tensor(self._h, key.encode(), t.data_ptr(), dt, shape, t.dim()),
              f"cfgpp_unet_load_tensor({key})")

    def load_state_dict(self, items: Iterable[Tuple[str, torch.Tensor]]):
        if isinstance(items, dict):
            items = items.items()
        for k, v in items:
            self.load_tensor(k, v)
        return self

    def set_max_tokens(self, max_tokens: int):
        """before ``finalize``: the longest text context, 77 * j with j <= 4 (include/cfgpp_long_prompt.h: cfgpp_unet_set_max_tokens)"""
        check(self.lib.cfgpp_unet_set_max_tokens(self._h, int(max_tokens)), "cfgpp_unet_set_max_tokens (ControlNet)")
        self.max_tokens = int(max_tokens)
        return self

    def finalize(self):
        check(self.lib.cfgpp_unet_finalize(self._h), "cfgpp_unet_finalize (ControlNet)")
        self.finalized = True
        return self

    # LoRA on the ControlNet's own matrices (same entry point and slot table as the UNet's: engine.HipUNet.lora / read_weight)
    def _matrix_shape(self, key: str):
        shapes = getattr(self, "_shapes", None)
        if shapes is None:
            shapes = self._shapes = dict(controlnet_param_shapes(self.cfg))
        return shapes.get(key)

    lora = HipUNet.lora
    read_weight = HipUNet.read_weight

    def set_context(self, ehs: torch.Tensor, text_embeds: Optional[torch.Tensor] = None, time_ids: Optional[torch.Tensor] = None):
        """the UNet's conditioning (``HipUNet.set_context``): the ControlNet sees the same text (and SDXL added) conditioning"""
        dev = torch.device("cuda", self.device)
        ehs = ehs.to(device=dev, dtype=torch.float16).contiguous()
        te = ti = None
        cond_rows = 0
        if self.cfg.addition_embed:
            if text_embeds is None or time_ids is None:
                raise CfgppError("set_context: SDXL needs text_embeds and time_ids")
            te = text_embeds.to(device=dev, dtype=torch.float16).contiguous()
            ti = time_ids.to(device=dev, dtype=torch.float32).contiguous()
            cond_rows = int(te.shape[0])
        self._keep["ctx"] = (ehs, te, ti)
        self.rows = int(ehs.shape[0])
        check(self.lib.cfgpp_unet_set_context(self._h, ehs.data_ptr(), self.rows, int(ehs.shape[1]), None if te is None else te.data_ptr(),
                                              None if ti is None else ti.data_ptr(), cond_rows, _stream_ptr(ehs)),
              "cfgpp_unet_set_context (ControlNet)")

    def set_image(self, image: torch.Tensor):
        """the control image [1 or B, 3, 8H, 8W] in [0, 1] (no normalisation: diffusers' do_normalize=False), embedded once on
        the device (include/cfgpp.h: cfgpp_unet_image_condition on a ControlNet)"""
        if image.dim() != 4 or tuple(image.shape[1:]) != (3,) + self.image_hw:
            raise CfgppError(f"set_image: control image shape {tuple(image.shape)} != [*, 3, {self.image_hw[0]}, {self.image_hw[1]}]")
        img = image.to(device=torch.device("cuda", self.device), dtype=torch.float16).contiguous()
        check(self.lib.cfgpp_unet_image_condition(self._h, img.data_ptr(), int(img.shape[0]), _stream_ptr(img)),
              "cfgpp_unet_image_condition (ControlNet image)")
        self._keep["image"] = img          # enqueued on the current stream: keep the source alive
        self.image_rows = int(img.shape[0])

    def num_residuals(self) -> int:
        return int(self.lib.cfgpp_controlnet_residual(self._h, 0, 1.0, None, 0, None, None))

    def residual(self, i: int, scale: float = 1.0, rows: Optional[int] = None) -> torch.Tensor:
        """test hook: residual i of the last forward (0 .. n-2 down blocks, n-1 the mid block), ``* scale`` rounded to fp16 as
        the UNet adds it, as fp32 [rows, C, h, w]"""
        rows = self.rows if rows is None else int(rows)
        hwc = (C.c_int * 3)()
        n = self.lib.cfgpp_controlnet_residual(self._h, int(i), float(scale), None, 0, hwc, None)
        if n < 0:
            raise CfgppError("cfgpp_controlnet_residual: " + _lib.last_error())
        out = torch.empty((rows, hwc[2], hwc[0], hwc[1]), dtype=torch.float32, device=torch.device("cuda", self.device))
        n = self.lib.cfgpp_controlnet_residual(self._h, int(i), float(scale), out.data_ptr(), rows, hwc, _stream_ptr(out))
        if n < 0:
            raise CfgppError("cfgpp_controlnet_residual: " + _lib.last_error())
        return out

    def device_bytes(self) -> float:
        return float(self.lib.cfgpp_unet_device_bytes(self._h))


def build_controlnet(spec, cfg: UNetConfig, max_rows: int, latent_hw: Tuple[int, int], device: int = 0, seed: int = 0,
                     max_tokens: int = 77) -> HipControlNet:
    """``spec``: "synthetic" (seeded weights), a path (a diffusers ``controlnet/`` folder or a safetensors file) or a state dict"""
    if isinstance(spec, HipControlNet):
        return spec
    if spec == "synthetic":
        items = synth_controlnet_state_dict(cfg, seed).items()
    elif isinstance(spec, str):
        from .checkpoint import controlnet_from_dir
        cn_cfg, items = controlnet_from_dir(spec, cfg)
        cfg = cn_cfg
    else:
        items = spec.items() if isinstance(spec, dict) else spec
    return HipControlNet(cfg, max_rows=max_rows, sample_hw=latent_hw, device=device, max_tokens=max_tokens).load_state_dict(items).finalize()
