"""The engine object a Solver drives: UNet forward + fused step kernels on ONE GPU.

``HipEngine`` is the only engine the product path constructs.  Tests may inject
another object with the same methods (``tests/mock_engine.py`` runs the solver
control flow on CPU against the oracle); nothing in this package falls back to
it.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from . import engine as E
from . import _lib
from ._lib import CfgppError
from .tune_cache import PinCache, build_id
from .unet_config import CONFIGS, UNetConfig
from .weights import load_safetensors_iter, synth_state_dict_iter


class HipEngine:
    """One UNet executor on one HIP stream (the caller's current stream).  Round 4 measured the alternative - the UNet batch
    split into row groups on concurrent streams, so that one group's launch prologues / epilogue bursts overlap the other's
    K loops - on the MI355X: 2 streams 20.75 ms against 19.35 ms per SD1.5 forward at 16 rows, 4 streams 26.4 ms (SDXL: 37.5 ->
    41.8 / 56.5 ms; profiles/r04/ab/forward_ab_fuse_ln_x_lanes_*): halving M per launch costs more than the overlap returns,
    so there is one stream."""

    def __init__(self, cfg: UNetConfig, max_batch: int = 1, latent_hw: Optional[Tuple[int, int]] = None,
                 device=None, weights="synthetic", weight_seed: int = 0, max_tokens: int = 77, soft_regions: bool = False):
        """``max_tokens``: the longest text context (77 * j, j <= 4) the UNet - and a ControlNet built by ``build_controlnet`` -
        accepts; 77 is the default engine, bit for bit.  ``soft_regions``: the UNet also allocates its region-weight buffers
        (``set_region_weights``; needs max_tokens > 77); False is the engine without them, byte for byte"""
        if isinstance(cfg, str):
            cfg = CONFIGS[cfg]
        if not torch.cuda.is_available():
            raise CfgppError("HipEngine needs a ROCm GPU; the HIP path has no CPU fallback")
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise CfgppError(f"HipEngine cannot run on device '{dev}': the HIP path has no CPU fallback")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.cfg = cfg
        self.max_batch = int(max_batch)
        # One device per process (the torchrun layout; cfgpp_unet_create / cfgpp_vae_create refuse a second one): the engine's
        # device BECOMES the process's current device and stays it - cfgpp_unet_finalize, the lazily allocated K-split
        # workspaces and every launch run against the current device, and none of the C entry points carries a device guard.
        torch.cuda.set_device(self.device)
        self.max_tokens = int(max_tokens)
        self.soft_regions = bool(soft_regions)
        self.unet = E.HipUNet(cfg, max_rows=2 * self.max_batch, sample_hw=latent_hw, device=self.device.index, max_tokens=self.max_tokens,
                              soft_regions=self.soft_regions)
        if weights == "synthetic":
            items = synth_state_dict_iter(cfg, weight_seed)
        elif isinstance(weights, str):
            items = load_safetensors_iter(weights)
        else:
            items = weights.items() if isinstance(weights, dict) else weights
        self.unet.load_state_dict(items).finalize()
        self.H, self.W = self.unet.H, self.unet.W
        # tile pins persist across processes (tune_cache.py): only the first process on a box runs the in-situ tuning passes
        self._pins = PinCache(getattr(cfg, "name", type(cfg).__name__), (self.H, self.W), torch.cuda.get_device_properties(self.device).name,
                              build_id(_lib.LIB_PATH), lambda rows: self.unet.export_tuning(rows), lambda h, rows: self.unet.import_tuning(h, rows),
                              knobs=lambda: (int(self.unet.lib.cfgpp_igemm_tuner_state()),),
                              mode=lambda rows: "shared" if self.unet.shared_prefix_ops(rows, rows // 2) else "")
        self._ctx_key = None
        self._ctx = None
        from .lora import LoraState
        self._lora = LoraState(cfg, self.unet.lora)
        self._control = None         # (HipControlNet, scale) while a control is set
        self._ip = None              # the parsed IP-Adapter while one is loaded
        self._regions = 0            # n_regions while a region map is set (set_regions)
        self._eps = None
        self._g_buf = None
        # opt-in guard for the first runs with a real checkpoint (real SDXL activations approach the fp16 maximum in the deep
        # blocks; the synthetic weights of the tests do not): scan eps after every forward - one host sync per step - and stop
        # with the timestep instead of decoding a NaN image
        self.check_finite = os.environ.get("CFGPP_CHECK_FINITE", "0") not in ("", "0")

    def _finite_or_raise(self, t):
        if not bool(torch.isfinite(self._eps).all()):
            bad = int((~torch.isfinite(self._eps)).sum())
            raise CfgppError(f"UNet output at t={t} holds {bad} non-finite values (fp16 overflow inside the UNet?) - CFGPP_CHECK_FINITE")

    # -- conditioning ------------------------------------------------------------
    def set_context(self, uc: torch.Tensor, c: torch.Tensor, text_embeds=None, time_ids=None):
        """uc, c: [B or 1, 77 * j, D], the same j <= max_tokens / 77 for both.  Rows are laid out [uc_1..uc_B, c_1..c_B]
        (the batched form of torch.cat([uc, c]), latent_diffusion.py:152)."""
        B = max(int(uc.shape[0]), int(c.shape[0]))
        if B > self.max_batch:
            raise CfgppError(f"batch {B} exceeds engine max_batch {self.max_batch}")
        if uc.shape[0] != B:
            uc = uc.expand(B, -1, -1)
        if c.shape[0] != B:
            c = c.expand(B, -1, -1)
        if int(uc.shape[1]) != int(c.shape[1]):
            raise CfgppError(f"set_context: uc has {int(uc.shape[1])} tokens, c {int(c.shape[1])}: pad the shorter prompt with chunks of the "
                             "empty prompt (cfgpp_amd.prompt)")
        ehs = torch.cat([uc, c], dim=0)
        self.unet.set_context(ehs, text_embeds, time_ids)
        self._ctx = (ehs, text_embeds, time_ids)
        if self._control is not None:         # the ControlNet sees the UNet's conditioning
            self._control[0].set_context(ehs, text_embeds, time_ids)
        self._pins.load(2 * B)
        self.B = B
        if self._eps is None or int(self._eps.shape[0]) != 2 * B:      # kept across calls: a captured graph holds its address
            self._eps = torch.empty((2 * B, self.cfg.out_channels, self.H, self.W), dtype=torch.float16, device=self.device)

    def image_condition(self, cond: torch.Tensor):
        """inpaint UNets: the step-invariant [mask, masked-image latent] channels, [1 or B, in - out, H, W]
        (include/cfgpp.h: cfgpp_unet_image_condition).  Once per job, before predict / ddim_loop_graph."""
        self.unet.image_condition(cond)

    # -- ControlNet ------------------------------------------------------------------
    def set_control(self, cn, image: torch.Tensor, scale: float = 1.0):
        """attach ControlNet ``cn`` (``controlnet.HipControlNet`` of this engine's geometry) with its control image
        [1 or B, 3, 8H, 8W] in [0, 1] and ``controlnet_conditioning_scale``: every later ``predict`` runs the ControlNet first and
        adds its residuals (include/cfgpp.h: cfgpp_unet_attach_control).  While a control is set the loops stay eager."""
        cn.set_image(image)
        if self._ctx is not None:
            cn.set_context(*self._ctx)
        self.unet.attach_control(cn, float(scale))
        self._control = (cn, float(scale))

    def clear_control(self):
        """detach the ControlNet: predictions are the plain UNet's again, bit for bit"""
        if self._control is not None:
            self.unet.attach_control(None, 0.0)
        self._control = None

    def build_controlnet(self, spec, seed: int = 0):
        """a ControlNet for this engine's geometry (max_batch, latent size, device): ``spec`` = "synthetic", a diffusers
        ``controlnet/`` folder / safetensors file, or a state dict (controlnet.build_controlnet)"""
        from .controlnet import build_controlnet
        return build_controlnet(spec, self.cfg, 2 * self.max_batch, (self.H, self.W), self.device.index, seed, max_tokens=self.max_tokens)

    @property
    def control(self):
        return self._control

    # -- IP-Adapter -------------------------------------------------------------------
    def set_ip_adapter(self, spec):
        """load an IP-Adapter (``ip_adapter.resolve``: "synthetic", a safetensors path, a state dict, a parsed adapter) into the
        UNet, or drop it (None).  UNet weights, tile pins and captured graphs are untouched (include/cfgpp_ip_adapter.h: cfgpp_unet_ip_load)."""
        from .ip_adapter import resolve
        if spec is not None and self.max_tokens != 77:
            raise CfgppError(f"ip_adapter=...: IP-Adapter on an engine with max_tokens={self.max_tokens} (max_prompt_chunks > 1) is not "
                             "supported: the image tokens' key slots sit at key 96 of a 128-slot buffer")
        parsed = resolve(spec, self.cfg)
        if self._ip is not None:     # the drop synchronises the device and clears every block's image slots: only when there is one
            self.unet.ip_load(None)
        self._ip = None
        if parsed is not None:
            for k, v in parsed.items():
                self.unet.ip_load(k, v)
            self._ip = parsed
        return self

    @property
    def ip_adapter(self):
        return self._ip

    def set_image_embeds(self, embeds: Optional[torch.Tensor], negative: Optional[torch.Tensor] = None, scale: float = 1.0):
        """image prompt of the next predictions: ``embeds`` [1 or B, embed_dim] - for a Resampler ("plus") adapter the image tower's
        penultimate hidden states [1 or B, seq, embed_dim] - (None deactivates), ``negative`` None = zeros of the same shape; call after
        ``set_context`` (the rows are the text context's)."""
        if embeds is None or float(scale) == 0.0:
            self.unet.set_image_context(None)
            return
        if self.ip_adapter is None:
            raise CfgppError("ip_adapter_image_embeds given but no IP-Adapter is loaded (get_solver(..., ip_adapter=...) / set_ip_adapter)")
        from .ip_adapter import assemble_embeds, assemble_hidden
        if int(embeds.shape[-1]) != self.ip_adapter.embed_dim:
            raise CfgppError(f"ip_adapter_image_embeds: embed_dim {int(embeds.shape[-1])}, the adapter takes {self.ip_adapter.embed_dim}")
        if self.ip_adapter.seq_input:
            self.unet.set_image_context(assemble_hidden(embeds, negative, self.B), float(scale))
        else:
            self.unet.set_image_context(assemble_embeds(embeds, negative, self.B), float(scale))

    # -- regional prompts ---------------------------------------------------------------
    def set_regions(self, ids: Optional[torch.Tensor], n_regions: int = 0):
        """region map ``ids`` [1 or B, H, W] (integer ids < ``n_regions`` = 2 .. 4) for the contexts to follow, whose uc / c hold
        ``n_regions`` chunks of 77 tokens; None: off, the plain engine (include/cfgpp_regions.h: cfgpp_unet_set_regions).  The
        unconditional rows use the same map: a [B, H, W] map is laid out for the rows [uc_1..uc_B, c_1..c_B].  While regions
        are on the loops stay eager."""
        if ids is None:
            if self._regions:
                self.unet.set_region_weights(None) if self.unet.soft_regions else self.unet.set_regions(None)
            self._regions = 0
            return self
        if self._control is not None:
            raise CfgppError("set_regions: a ControlNet is set (control_image with regions is not built)")
        if self._ip is not None:
            raise CfgppError("set_regions: an IP-Adapter is loaded (ip_adapter with regions is not built)")
        ids = torch.as_tensor(ids)
        if ids.dim() == 3 and int(ids.shape[0]) > 1:
            ids = torch.cat([ids, ids], 0)
        self.unet.set_regions(ids, int(n_regions))
        self._regions = int(n_regions)
        return self

    def set_region_weights(self, w: Optional[torch.Tensor]):
        """soft regional prompts: weights ``w`` [1 or B, R, H, W] (float, every pixel summing to 1; R = 2 .. 4) for the contexts to
        follow, whose uc / c hold R chunks of 77 tokens; None: off (include/cfgpp_regions_soft.h: cfgpp_unet_set_region_weights).
        The unconditional rows use the same weights.  Needs an engine built with ``soft_regions=True``.  While on the loops stay
        eager; weights and a hard region map are exclusive."""
        if w is None:
            if self._regions:
                self.unet.set_region_weights(None) if self.unet.soft_regions else self.unet.set_regions(None)
            self._regions = 0
            return self
        if not self.soft_regions:
            raise CfgppError("set_region_weights: the engine was built without soft_regions=True (get_solver(..., max_regions=R, soft_regions=True))")
        if self._control is not None:
            raise CfgppError("set_region_weights: a ControlNet is set (control_image with regions is not built)")
        if self._ip is not None:
            raise CfgppError("set_region_weights: an IP-Adapter is loaded (ip_adapter with regions is not built)")
        w = torch.as_tensor(w)
        if w.dim() == 4 and int(w.shape[0]) > 1:
            w = torch.cat([w, w], 0)
        self.unet.set_region_weights(w)
        self._regions = int(self.unet.soft_regions)
        return self

    @property
    def regions(self) -> int:
        return self._regions

    # -- FreeU -----------------------------------------------------------------------
    def set_freeu(self, spec):
        """``(s1, s2, b1, b2)`` (diffusers ``enable_freeu``; a mapping with those keys works too) or None (off: the plain engine, bit
        for bit and launch for launch).  A property of the UNet: an attached ControlNet is not touched.  Weights, tile pins and the
        conditioning stay; a captured graph of another FreeU state is never replayed (include/cfgpp_freeu.h)."""
        self.unet.set_freeu(spec)
        return self

    @property
    def freeu(self):
        return self.unet.freeu

    # -- LoRA ------------------------------------------------------------------------
    def set_lora(self, adapters, ignore_text_encoder: bool = False):
        """``adapters``: list of ``(parsed | safetensors path | state dict, scale)``; ``[]`` restores the base weights.  One merge
        kernel per touched weight (lora.LoraState); an attached ControlNet is left alone.  The weights' addresses do not move, so
        tile pins and captured graphs stay valid; the conditioning has to be set again (``lora_epoch`` is part of the solvers'
        context-cache key): the cross-attention K / V^T are computed from attn2.to_k / to_v."""
        self._lora.set(adapters, ignore_text_encoder=ignore_text_encoder)
        return self

    @property
    def lora_epoch(self) -> int:
        return self._lora.epoch

    @property
    def lora_adapters(self):
        return list(self._lora.adapters)

    def predict(self, z: torch.Tensor, t: float):
        """(eps_uc, eps_c), each [B,4,H,W] fp16 - replaces predict_noise's UNet call + chunk(2)."""
        eps = self.unet.forward(z, float(t), self._eps)
        self._pins.save(self.unet.rows)          # (no-op after the first forward at this batch)
        if self.check_finite:
            self._finite_or_raise(t)
        return eps[: self.B], eps[self.B:]

    def predict_into(self, z_chunk: torch.Tensor, t: float, eps_chunk: torch.Tensor):
        """one forward into a caller-owned slice: ``eps_chunk`` [2 * rows, 4, H, W] fp16 (uc rows, then c rows) = UNet(``z_chunk``
        [rows, 4, H, W], t), rows = the context's B.  The panorama loop's form of ``predict``: the views' eps land where the fused
        view step reads them, ``_eps`` is not touched."""
        if eps_chunk.dtype != torch.float16 or tuple(eps_chunk.shape) != (2 * self.B, self.cfg.out_channels, self.H, self.W) \
                or not eps_chunk.is_contiguous() or not eps_chunk.is_cuda:
            raise CfgppError(f"predict_into: eps_chunk must be a contiguous fp16 GPU tensor [{2 * self.B}, {self.cfg.out_channels}, "
                             f"{self.H}, {self.W}], got {eps_chunk.dtype} {list(eps_chunk.shape)}")
        if int(z_chunk.shape[0]) != self.B:
            raise CfgppError(f"predict_into: z_chunk has {int(z_chunk.shape[0])} rows, the context {self.B}")
        self.unet.forward(z_chunk, float(t), eps_chunk)
        self._pins.save(self.unet.rows)
        if self.check_finite and not bool(torch.isfinite(eps_chunk).all()):
            raise CfgppError(f"UNet output at t={t} holds non-finite values (fp16 overflow inside the UNet?) - CFGPP_CHECK_FINITE")

    # -- whole-loop graph replay ---------------------------------------------------------
    @property
    def graph_enabled(self) -> bool:
        """$CFGPP_GRAPH=1: DDIM loops without a callback run as hipGraph replays of one captured step (default off: see DESIGN.md)"""
        # a controlled step is not captured, nor a region-masked one
        return os.environ.get("CFGPP_GRAPH", "0") not in ("", "0") and self._control is None and not self._regions

    def ddim_loop_graph(self, zt: torch.Tensor, steps, lam: float, tweedie_uc: bool, renoise_uc: bool, single: str = ""):
        """run the whole loop on (a persistent copy of) ``zt``; returns (z0t, zt) as fresh tensors.  ``single``: "uc" / "c" when the
        caller passed only one conditioning (both eps halves are then the same rows, like predict_noise's)"""
        key = (int(zt.shape[0]), zt.dtype)
        if self._g_buf is None or self._g_buf[0] != key:
            self._g_buf = (key, torch.empty_like(zt), torch.empty_like(zt))      # stable addresses: one capture serves every sample() call
        _, gz, gz0 = self._g_buf
        gz.copy_(zt)
        eps = self._eps
        euc, ec = eps[: self.B], eps[self.B:]
        if single == "uc":
            ec = euc
        elif single == "c":
            euc = ec
        self.unet.sample_graph_ddim(gz, gz0, eps, euc, ec, steps, lam, tweedie_uc, renoise_uc)
        self._pins.save(self.unet.rows)
        if self.check_finite:
            self._finite_or_raise(steps[-1][0])
        return gz0.clone(), gz.clone()

    # -- tile pins (bench.py: rank 0 tunes, every rank imports) ----
    def export_tuning(self):
        return self.unet.export_tuning(self.unet.rows)

    def import_tuning(self, hints, batch: int):
        self.unet.import_tuning(hints, 2 * int(batch))
        self._pins.mark_imported(2 * int(batch))       # an explicit import wins over whatever this rank's disk cache holds

    def device_bytes(self) -> float:
        return self.unet.device_bytes()

    # -- fused sampler arithmetic ---------------------------------------------------
    step_ddim = staticmethod(E.step_ddim)
    step_ddim_masked = staticmethod(E.step_ddim_masked)
    kdiff_input = staticmethod(E.kdiff_input)
    step_kdiff = staticmethod(E.step_kdiff)
    kdiff_denoise = staticmethod(E.kdiff_denoise)
    lincomb = staticmethod(E.lincomb)
    # v-prediction (include/cfgpp_vpred.h)
    step_ddim_v = staticmethod(E.step_ddim_v)
    v_to_eps = staticmethod(E.v_to_eps)
    cfg_rescale = staticmethod(E.cfg_rescale)
    # LCM (include/cfgpp_lcm.h)
    step_lcm = staticmethod(E.step_lcm)
    philox_normal = staticmethod(E.philox_normal)
    # DPM++ 2M / 3M SDE (include/cfgpp_sde.h)
    sde_input = staticmethod(E.sde_input)
    step_sde = staticmethod(E.step_sde)
    # DPM++ SDE (include/cfgpp_dpmpp_sde.h)
    step_sde_stage = staticmethod(E.step_sde_stage)
    # img2img / latent hires fix (include/cfgpp_img2img.h)
    img2img_start = staticmethod(E.img2img_start)
    # MultiDiffusion panoramas (include/cfgpp_panorama.h)
    gather_views = staticmethod(E.gather_views)
    step_ddim_views = staticmethod(E.step_ddim_views)

    @property
    def time_cond_proj_dim(self) -> int:
        """width of the guidance-scale embedding of a guidance-embedded (LCM-distilled) UNet; 0: a plain UNet"""
        return self.unet.time_cond

    def set_guidance_embedding(self, w_emb):
        """guidance-embedded UNets, once per job before ``predict``: the embedding of the job's guidance scale
        (``lcm.guidance_scale_embedding``; include/cfgpp_lcm.h: cfgpp_unet_guidance_embedding)"""
        self.unet.guidance_embedding(w_emb)

    def randn_like(self, x):
        """ancestral noise: device RNG, like the reference's torch.randn_like on the GPU"""
        return torch.randn_like(x)

    def flops_per_forward(self, rows: int) -> float:
        return self.unet.flops(rows)
