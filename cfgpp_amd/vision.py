"""CLIP image tower on libcfgpp_hip.so (``csrc/vision.hip``, ``include/cfgpp_vision.h``): same call contract as
``ip_adapter.ImageEncoder`` - ``tower(image, hidden=False)``, ``encode_pixels``, ``negative_hidden`` - without torch ops:
the resize / crop / normalise front end, the patch embedding, every transformer layer and the pooled projection are HIP launches.

What the solvers build for ``ip_adapter_image=`` on a GPU device (``latent_diffusion.Solver._ip_prepare``); also usable directly
(``get_solver(..., image_encoder=HipClipImageTower.from_dir(...))``).  ``tests/test_gpu_vision.py`` compares it with
``transformers.CLIPVisionModelWithProjection`` on the same weights (head dims 64 / 80 / 104, ViT-H and ViT-bigG widths, both
activations, hidden states and pooled embeds).

Towers the HIP path does not take are refused BY NAME with :class:`UnsupportedTower` before anything is built; that - and only
that - is what the solver answers with the torch tower, recording the refusal in :data:`last_image_tower_fallbacks`.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import List

import torch

from . import _lib
from ._lib import CfgppError, check

HEAD_DIMS = (64, 80, 104)           # ViT-L/14, ViT-H/14, ViT-bigG/14
MAX_TOKENS = 320                    # 257 for every shipped 224-px tower; ViT-L/14-336 (577) and larger are out of scope

# one line per fallback to ``ip_adapter.ImageEncoder`` a solver took since the process started ("<folder>: <refusal>"), newest
# last: the image-side twin of ``checkpoint.last_text_tower_fallbacks``
last_image_tower_fallbacks: List[str] = []


class UnsupportedTower(CfgppError):
    """this is not a tower the HIP path takes (geometry / activation); nothing was built"""


def check_geometry(hidden: int, layers: int, heads: int, intermediate: int, act: str, proj_dim: int, image_size: int,
                   patch_size: int) -> int:
    """refuse, by name, every geometry ``cfgpp_vision_create`` refuses; returns the token count.  Pure Python: no GPU needed."""
    if min(hidden, layers, heads, intermediate, proj_dim, image_size, patch_size) <= 0:
        raise UnsupportedTower(f"image tower: non-positive geometry (hidden={hidden} layers={layers} heads={heads} "
                               f"intermediate={intermediate} proj_dim={proj_dim} image_size={image_size} patch_size={patch_size})")
    if hidden % heads != 0 or hidden // heads not in HEAD_DIMS:
        raise UnsupportedTower(f"image tower: unsupported head dim: hidden={hidden} over heads={heads} "
                               f"(hidden must be heads x one of {HEAD_DIMS})")
    if hidden % 64 != 0 or intermediate % 64 != 0:
        raise UnsupportedTower(f"image tower: hidden={hidden} and intermediate={intermediate} must be multiples of 64")
    if image_size % patch_size != 0:
        raise UnsupportedTower(f"image tower: image_size={image_size} is not a multiple of patch_size={patch_size}")
    tokens = 1 + (image_size // patch_size) ** 2
    if tokens > MAX_TOKENS:
        raise UnsupportedTower(f"image tower: {tokens} tokens (image_size={image_size}, patch_size={patch_size}): towers beyond "
                               f"{MAX_TOKENS} tokens are not supported")
    if act not in ("quick_gelu", "gelu"):
        raise UnsupportedTower(f"image tower: activation '{act}' (quick_gelu | gelu)")
    if proj_dim % 4 != 0:
        raise UnsupportedTower(f"image tower: projection_dim={proj_dim} must be a multiple of 4")
    return tokens


class HipClipImageTower:
    torch_ops = False

    def __init__(self, hidden: int, layers: int, heads: int, intermediate: int, act: str, proj_dim: int, image_size: int,
                 patch_size: int, state_dict, max_batch: int = 2, device=None):
        """``state_dict``: ``transformers`` CLIPVisionModelWithProjection tensors (dict / iterable of pairs / safetensors path), keys
        with or without the ``vision_model.`` prefix"""
        self.tokens = check_geometry(int(hidden), int(layers), int(heads), int(intermediate), act, int(proj_dim), int(image_size),
                                     int(patch_size))
        if not torch.cuda.is_available():
            raise CfgppError("HipClipImageTower needs a ROCm GPU; the HIP path has no CPU fallback")
        self.lib = _lib.load()
        dev = torch.device(device if device is not None else "cuda")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.hidden, self.layers, self.proj, self.max_batch = int(hidden), int(layers), int(proj_dim), int(max_batch)
        self.size = int(image_size)
        self._h = self.lib.cfgpp_vision_create(self.hidden, self.layers, int(heads), int(intermediate), 0 if act == "quick_gelu" else 1,
                                               self.proj, self.size, int(patch_size), self.max_batch, self.device.index)
        if not self._h:
            raise CfgppError("cfgpp_vision_create failed: " + _lib.last_error())
        if isinstance(state_dict, str):
            from .weights import load_safetensors_iter
            state_dict = load_safetensors_iter(state_dict)
        items = state_dict.items() if isinstance(state_dict, dict) else state_dict
        for k, v in items:
            if k.endswith("position_ids"):
                continue
            t = v.detach().cpu().contiguous()
            dt = 1 if t.dtype == torch.float16 else 0
            if dt == 0:
                t = t.to(torch.float32)
            shape = (C.c_long * max(t.dim(), 1))(*t.shape)
            check(self.lib.cfgpp_vision_load_tensor(self._h, k.encode(), t.data_ptr(), dt, shape, t.dim()), f"cfgpp_vision_load_tensor({k})")
        check(self.lib.cfgpp_vision_finalize(self._h), "cfgpp_vision_finalize")

    @classmethod
    def from_dir(cls, folder, max_batch: int = 2, device=None):
        """the HIP twin of ``ImageEncoder(folder)``: ``folder`` holds ``image_encoder/`` (or is it), with ``config.json`` and
        ``model.safetensors`` / ``model.fp16.safetensors``"""
        folder = str(folder)
        path = os.path.join(folder, "image_encoder") if os.path.isdir(os.path.join(folder, "image_encoder")) else folder
        with open(os.path.join(path, "config.json"), "r") as f:
            cfg = json.load(f)
        if "hidden_size" not in cfg and "vision_config" in cfg:      # a whole CLIPConfig
            cfg = cfg["vision_config"]
        weights = next((p for p in (os.path.join(path, n) for n in ("model.safetensors", "model.fp16.safetensors")) if os.path.exists(p)),
                       os.path.join(path, "model.safetensors"))
        return cls(cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["intermediate_size"],
                   cfg.get("hidden_act", "quick_gelu"), cfg.get("projection_dim", 512), cfg.get("image_size", 224), cfg.get("patch_size", 32),
                   weights, max_batch=max_batch, device=device)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                torch.cuda.synchronize()
            except Exception:  # noqa: BLE001
                pass
            self.lib.cfgpp_vision_destroy(h)
            self._h = None

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    @torch.no_grad()
    def preprocess(self, image: torch.Tensor) -> torch.Tensor:
        """[N, 3, H, W] in [0, 1] -> fp16 pixel values [N, 3, size, size] (``ip_adapter.preprocess_image`` in one HIP launch)"""
        if image.dim() != 4 or image.shape[1] != 3:
            raise CfgppError(f"ip_adapter_image: shape {tuple(image.shape)}, expected [N, 3, H, W] in [0, 1]")
        x = image.to(self.device, torch.float32).contiguous()
        n, _, H, W = (int(s) for s in x.shape)
        out = torch.empty((n, 3, self.size, self.size), dtype=torch.float16, device=self.device)
        check(self.lib.cfgpp_vision_preprocess(self._h, x.data_ptr(), n, H, W, out.data_ptr(), self._stream()), "cfgpp_vision_preprocess")
        return out

    @torch.no_grad()
    def __call__(self, image: torch.Tensor, hidden: bool = False) -> torch.Tensor:
        """``image_embeds`` [N, projection_dim] fp16; with ``hidden=True`` the penultimate hidden states ``hidden_states[-2]``
        [N, 1 + patches, hidden_size] fp16, which is what a Resampler ("plus") adapter reads"""
        return self.encode_pixels(self.preprocess(image), hidden)

    @torch.no_grad()
    def encode_pixels(self, pixel_values: torch.Tensor, hidden: bool = False, layer=None) -> torch.Tensor:
        """the tower on an already preprocessed pixel tensor [N, 3, size, size], in slices of ``max_batch`` images.  ``layer``
        (with ``hidden=True``): which of ``hidden_states[0 .. layers]``, negative counts from the end; default -2."""
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, self.size, self.size):
            raise CfgppError(f"pixel_values: shape {tuple(pixel_values.shape)}, expected [N, 3, {self.size}, {self.size}]")
        x = pixel_values.to(self.device, torch.float16).contiguous()
        n = int(x.shape[0])
        if hidden:
            k = -2 if layer is None else int(layer)
            k = k + self.layers + 1 if k < 0 else k
            if not 0 <= k <= self.layers:
                raise ValueError(f"hidden_states[{layer}] of a {self.layers}-layer tower")
            out = torch.empty((n, self.tokens, self.hidden), dtype=torch.float16, device=self.device)
        else:
            k = -1
            emb = torch.empty((n, self.proj), dtype=torch.float32, device=self.device)
        stream = self._stream()
        for s in range(0, n, self.max_batch):
            e = min(s + self.max_batch, n)
            check(self.lib.cfgpp_vision_encode(self._h, x[s:e].data_ptr(), e - s, k, out[s:e].data_ptr() if hidden else None,
                                               None if hidden else emb[s:e].data_ptr(), stream), "cfgpp_vision_encode")
        return out if hidden else emb.to(torch.float16)

    @torch.no_grad()
    def negative_hidden(self, image: torch.Tensor) -> torch.Tensor:
        """the default negative of a Resampler adapter: the tower's hidden states of an ALL-ZERO PIXEL tensor - the published
        pipeline's ``torch.zeros_like`` of the preprocessed image - and NOT zeros of the hidden states (``ImageEncoder.negative_hidden``)"""
        n = int(image.shape[0])
        return self.encode_pixels(torch.zeros((n, 3, self.size, self.size), dtype=torch.float16, device=self.device), hidden=True)

    def flops(self, n: int = 1) -> float:
        return float(self.lib.cfgpp_vision_flops(self._h, int(n)))

    def device_bytes(self) -> float:
        return float(self.lib.cfgpp_vision_device_bytes(self._h))


def build_image_encoder(folder, device, image_tower: str = "hip"):
    """the image tower of a solver: the HIP tower on a GPU device; ``ip_adapter.ImageEncoder`` (torch ops) when ``image_tower="torch"``,
    on a CPU device, or when the HIP tower refuses the folder's geometry by name (recorded in :data:`last_image_tower_fallbacks`).
    Any other failure propagates."""
    from .ip_adapter import ImageEncoder
    if image_tower not in ("hip", "torch"):
        raise ValueError(f"image_tower={image_tower!r}: 'hip' or 'torch'")
    dev = torch.device(device)
    if image_tower == "torch" or dev.type != "cuda":
        return ImageEncoder(folder, device)
    try:
        return HipClipImageTower.from_dir(folder, device=dev)
    except UnsupportedTower as e:
        last_image_tower_fallbacks.append(f"{folder}: {e}")
        return ImageEncoder(folder, device)
