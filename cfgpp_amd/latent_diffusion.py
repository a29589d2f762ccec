"""SD1.5 solvers on the MI355X-native engine - same registry names, ``Solver``
class API, scheduler-index conventions and callback protocol as the reference's
``latent_diffusion.py`` (registry :13-26, wrapper :54-241, solvers :247-1010),
re-built so that the loop body is two asynchronous launches: the HIP UNet
(``engine.predict``) and one fused step kernel.  The host only walks
pre-computed fp32 coefficient tables; it never synchronises with the device
inside the loop unless a callback asks for tensors.

Extension beyond the reference: batches.  ``prompt=[null,
[text_1..text_B]]`` (or ``prompt_embeds=(uc, c)``) with ``seeds=[s_1..s_B]`` runs
B independent chains; chain b equals the reference run with ``set_seed(s_b)``.
"""
from __future__ import annotations

import contextlib
import functools
import os
import sys
from typing import Any, Callable, Dict, List, Optional

import torch

from . import coeffs as K
from ._lib import CfgppError
from .conditioning import SyntheticTextEncoder, as_list
from .registry import Registry
from .schedule import SchedulerTables, get_ancestral_step, get_sigmas_karras  # noqa: F401
from .unet_config import SD15, UNetConfig

# ---- solver registry (names: Appendix A of SURVEY.md) ----
__SOLVER__ = Registry("Solver")
register_solver = __SOLVER__.register        # @register_solver(name)
get_solver = __SOLVER__.create               # get_solver(name, solver_config=..., device=..., **kw)


class _SchedulerView:
    """The two attributes of ``self.scheduler`` the reference's solvers touch."""

    def __init__(self, tables: SchedulerTables):
        self.timesteps = tables.timesteps
        self.alphas_cumprod = tables.alphas_cumprod
        self.final_alpha_cumprod = tables.final_alpha_cumprod


def controlled(sample):
    """``sample(..., control_image=None, controlnet_conditioning_scale=1.0)``: with a control image, the solver's ControlNet
    (``get_solver(..., controlnet=...)``) is attached to the engine for this call - every UNet prediction of the loop, whatever
    the solver, follows it (diffusers StableDiffusion(XL)ControlNetPipeline, one net, non-guess mode); without one the engine
    runs the plain UNet.  Solvers whose ``controllable`` is False (inversion, edit, inpaint) refuse a control image.

    ``sample(..., ip_adapter_image_embeds=[1 or B, embed_dim] | ip_adapter_image=[1 or B, 3, H, W] in [0, 1],
    negative_ip_adapter_image_embeds=None, ip_adapter_scale=1.0)``: an image prompt for the solver's IP-Adapter
    (``get_solver(..., ip_adapter=...)`` / ``set_ip_adapter``) for this call; the same solvers refuse these arguments.

    ``sample(..., guidance_rescale=phi)``: diffusers' ``rescale_noise_cfg`` factor for this call, overriding
    ``get_solver(..., guidance_rescale=)``; `ddim` / `ddim_cfg++` with ``prediction_type="v_prediction"`` only, refused by name
    elsewhere."""
    @functools.wraps(sample)
    def run(self, *args, **kwargs):
        image = kwargs.pop("control_image", None)
        scale = kwargs.pop("controlnet_conditioning_scale", 1.0)
        ip = {k: kwargs.pop(k, None) for k in ("ip_adapter_image_embeds", "negative_ip_adapter_image_embeds", "ip_adapter_image")}
        ip_scale = kwargs.pop("ip_adapter_scale", 1.0)
        if any(v is not None for v in ip.values()) and not self.controllable:
            raise ValueError(f"{type(self).__name__}.sample() does not take ip_adapter_image_embeds / ip_adapter_image: IP-Adapter image "
                             "prompts are for the text-to-image solvers (inversion, edit and inpaint solvers refuse them)")
        # sample(..., region_prompts=[p1, ..], region_masks=[m1, ..]): regional prompts (cfgpp_amd/regions.py); empty = the plain call
        # region_base_ratio=beta and region_negative_prompts=[n1, ..] go with them (soft masks need get_solver(..., soft_regions=True))
        if any(k in kwargs for k in ("region_prompts", "region_masks", "region_base_ratio", "region_negative_prompts")):
            self._region_job = self._regions_prepare(kwargs.pop("region_prompts", None), kwargs.pop("region_masks", None), image, ip,
                                                     base_ratio=kwargs.pop("region_base_ratio", 0.0),
                                                     negative_prompts=kwargs.pop("region_negative_prompts", None))
        self._ip_job = self._ip_prepare(ip, ip_scale)
        lora_scale = kwargs.pop("lora_scale", None)
        if lora_scale is not None:          # shorthand: every adapter of the solver at this scale, from this job on
            self.set_lora_scale(lora_scale)
        if "guidance_rescale" in kwargs:    # this job's rescale_noise_cfg factor, overriding get_solver(guidance_rescale=)
            phi = kwargs.pop("guidance_rescale")
            self._job_rescale = None if phi is None else self._check_guidance_rescale(phi)
        if image is not None and not self.controllable:
            raise ValueError(f"{type(self).__name__}.sample() does not take control_image: ControlNet conditioning is for the "
                             "text-to-image solvers (inversion, edit and inpaint solvers refuse it)")
        try:
            with self._control(image, scale):
                return sample(self, *args, **kwargs)
        finally:
            self._ip_job = None
            self._job_rescale = None
            self._region_job = None
    return run


def _progress(it, desc):
    try:
        from tqdm import tqdm
        return tqdm(it, desc=desc, leave=False, disable=None)
    except Exception:  # noqa: BLE001
        return it


class StableDiffusion:
    """Model wrapper (reference: latent_diffusion.py:54-241)."""

    unet_config: UNetConfig = SD15
    scheduler_kind = "ddim"
    latent_scale = 8

    def __init__(self, solver_config, model_key: str = "runwayml/stable-diffusion-v1-5",
                 device: Optional[torch.device] = None, **kwargs):
        self.device = device
        self.model_key = model_key
        self.dtype = kwargs.get("pipe_dtype", torch.float16)
        # how a 0-dim fp32 scalar written first in `s * fp16_tensor` enters the product (coeffs.py): the
        # reference RUNS on the GPU, where torch keeps it fp32 ("cuda"); the golden vectors were recorded on
        # torch-CPU, which rounds it to fp16 first ("cpu": the default only when a test injects an engine).
        self.scalar_semantics = kwargs.get("scalar_semantics", "cpu" if kwargs.get("engine") is not None else "cuda")
        cfg = kwargs.get("unet_config", self.unet_config)
        self.cfg = cfg
        self.latent_hw = tuple(kwargs.get("latent_hw", (cfg.sample_size, cfg.sample_size)))
        self.max_batch = int(kwargs.get("max_batch", 1))
        # long / weighted prompts (cfgpp_amd/prompt.py): 1 = off (prompts cut at 75 ids, brackets literal); K = 2 .. 4: prompts are
        # parsed, cut into up to K chunks of 75 ids and the engine is built for text contexts of 77 * K tokens
        self.max_prompt_chunks = int(kwargs.get("max_prompt_chunks", 1))
        if not 1 <= self.max_prompt_chunks <= 4:
            raise ValueError(f"max_prompt_chunks={self.max_prompt_chunks}: 1 (off) .. 4")
        if self.max_prompt_chunks > 1 and kwargs.get("ip_adapter") is not None:
            raise ValueError(f"ip_adapter=... together with max_prompt_chunks={self.max_prompt_chunks} is not supported: the IP-Adapter's "
                             "image tokens sit at key 96 of a 128-slot cross-attention buffer (max_prompt_chunks must be 1)")
        # regional prompts (cfgpp_amd/regions.py): 1 = off (no new call anywhere); R = 2 .. 4: sample() takes up to R - 1 region
        # prompts with their masks, and the engine is built for text contexts of 77 * R tokens
        self.max_regions = int(kwargs.get("max_regions", 1))
        self._region_job = None
        self._region_serial = 0
        if not 1 <= self.max_regions <= 4:
            raise ValueError(f"max_regions={self.max_regions}: 1 (off) .. 4")
        if self.max_regions > 1:
            if self.max_prompt_chunks > 1:
                raise ValueError(f"max_regions={self.max_regions} together with max_prompt_chunks={self.max_prompt_chunks} is not supported: "
                                 "region prompts are plain 77-token prompts (long region prompts are not built)")
            if kwargs.get("ip_adapter") is not None:
                raise ValueError(f"max_regions={self.max_regions} together with ip_adapter=... is not supported (IP-Adapter with regions is not built)")
            if not self.controllable:
                raise ValueError(f"max_regions={self.max_regions}: {type(self).__name__} takes no regional prompts - they are for the "
                                 "text-to-image solvers (inversion, edit, inpaint and panorama solvers refuse them)")
        # soft regions (float masks, region_base_ratio): the engine also carries fp32 weight maps and runs the soft regional kernel
        self.soft_regions = bool(kwargs.get("soft_regions", False))
        if self.soft_regions and self.max_regions < 2:
            raise ValueError(f"soft_regions=True needs max_regions=R with R = 2 .. 4 (max_regions={self.max_regions})")

        # what the UNet predicts and on which schedule (DESIGN.md "v-prediction"): "epsilon" / "leading" / no rescaling are the
        # reference's models, bit for bit
        self.prediction_type = kwargs.get("prediction_type") or "epsilon"
        zero_snr = bool(kwargs.get("zero_terminal_snr", False))
        spacing = kwargs.get("timestep_spacing") or "leading"
        if self.scheduler_kind == "lightning":      # its Euler scheduler has its own (trailing) timesteps, whatever a checkpoint's file says
            spacing = "leading"
        self._job_rescale = None
        self._refuse_unsupported_prediction(zero_snr, spacing)
        self.guidance_rescale = self._check_guidance_rescale(kwargs.get("guidance_rescale") or 0.0)
        # per-step noise of the ancestral solvers: "torch" (torch.randn_like, the reference's) or "philox" (seeded, in HIP: cfgpp_lcm.h)
        self.noise = kwargs.get("noise") or "torch"
        if self.noise not in ("torch", "philox"):
            raise ValueError(f"noise={self.noise!r}: 'torch' or 'philox'")
        if self.noise == "philox" and not self.ancestral:
            raise ValueError(f"{self._name()}: noise='philox' is for the ancestral solvers (euler_a*, dpm++_2s_a*): no other solver "
                             "draws per-step noise")

        # scheduler tables (host)
        self.tables = SchedulerTables(solver_config.num_sampling, self.scheduler_kind, zero_terminal_snr=zero_snr, timestep_spacing=spacing)
        self.scheduler = _SchedulerView(self.tables)
        self.total_alphas = self.tables.total_alphas
        self.sigmas = self.tables.sigmas
        self.log_sigmas = self.tables.log_sigmas
        self.skip = self.tables.skip
        self.final_alpha_cumprod = self.tables.final_alpha_cumprod

        # engine: the HIP UNet + fused step kernels.  No fallback.
        engine = kwargs.get("engine")
        if engine is None:
            from .hip_engine import HipEngine
            engine = HipEngine(cfg, max_batch=self.max_batch, latent_hw=self.latent_hw, device=device,
                               weights=kwargs.get("unet_weights", "synthetic"), weight_seed=kwargs.get("weight_seed", 0),
                               max_tokens=77 * max(self.max_prompt_chunks, self.max_regions),
                               **(dict(soft_regions=True) if self.soft_regions else {}))
        self.engine = engine
        self.unet = engine
        self.work_device = getattr(engine, "device", torch.device("cpu"))
        # ControlNet ("synthetic", a diffusers controlnet/ folder or safetensors file, or a state dict), built by the engine at
        # its own max_batch and latent size; attached per sample() call that passes control_image
        self.controlnet = None
        cn = kwargs.get("controlnet")
        if cn is not None:
            if not hasattr(engine, "build_controlnet"):
                raise ValueError(f"controlnet=...: the engine {type(engine).__name__} cannot build a ControlNet")
            self.controlnet = engine.build_controlnet(cn, seed=kwargs.get("controlnet_seed", 0))

        # IP-Adapter ("synthetic", a safetensors path, a state dict): loaded into the UNet; used by the sample() calls that pass
        # ip_adapter_image_embeds / ip_adapter_image.  ip_adapter_dir: the folder that holds the CLIP `image_encoder/`.
        # image_tower: "hip" (default: vision.HipClipImageTower on a GPU device) | "torch" (ip_adapter.ImageEncoder); image_encoder=
        # overrides both.
        self._ip_job = None                 # (embeds, negative, scale, serial) of the running sample() call
        self._ip_key = None                 # what the engine's image context was last set from
        self._ip_serial = 0
        self.ip_adapter_dir = kwargs.get("ip_adapter_dir")
        self.image_encoder = kwargs.get("image_encoder")
        self.image_tower = kwargs.get("image_tower", "hip")
        if self.image_tower not in ("hip", "torch"):
            raise ValueError(f"image_tower={self.image_tower!r}: 'hip' or 'torch'")
        if kwargs.get("ip_adapter") is not None:
            self.set_ip_adapter(kwargs["ip_adapter"])

        # FreeU (diffusers enable_freeu): (s1, s2, b1, b2) or a mapping with those keys; a property of the UNet, so every solver
        # takes it - inversion and edit included - and a ControlNet is not affected.  None / absent: the plain engine.
        if kwargs.get("freeu") is not None:
            self.set_freeu(kwargs["freeu"])

        if kwargs.get("lora"):              # [(safetensors path | state dict | parsed, scale), ...] merged into the UNet on the device
            self.set_lora(kwargs["lora"], ignore_text_encoder=kwargs.get("lora_ignore_text_encoder", False))

        # boundary components (off the per-step path)
        self.text_encoder = kwargs.get("text_encoder") or SyntheticTextEncoder(cfg.cross_attention_dim, None)
        self.vae = kwargs.get("vae")
        self._vae_kwargs = dict(seed=kwargs.get("vae_seed", 0))
        vw = kwargs.get("vae_weights")                  # diffusers AutoencoderKL state dict, or a safetensors path
        if vw is not None:
            if isinstance(vw, str):
                from .weights import load_safetensors_iter
                vw = dict(load_safetensors_iter(vw))
            self._vae_kwargs["state_dict"] = vw

    # ------------------------------------------------------------------ reference API
    def __call__(self, *args: Any, **kwargs: Any) -> Any:
        self.sample(*args, **kwargs)        # return value dropped, as in the reference (quirk Q4)

    def sample(self, *args: Any, **kwargs: Any) -> Any:
        raise NotImplementedError("Solver must implement sample() method.")

    def alpha(self, t):
        return self.tables.alpha(t)

    controllable = True         # text-to-image: sample() takes control_image (see `controlled`)

    # ------------------------------------------------------------------ v-prediction, zero terminal SNR, guidance rescale
    solver_name = None          # the registry name (registry.py)
    sigma_solver = False        # Karras-sigma (k-diffusion) loop: sigma_max of a zero-terminal-SNR schedule is infinite
    ancestral = False           # draws fresh noise every step (euler_a*, dpm++_2s_a*): takes noise="philox"
    vpred_ok = True             # False: the solver's update has no v form (inpaint blend)
    rescale_ok = False          # True on `ddim` / `ddim_cfg++`: the text-to-image DDIM loops take guidance_rescale

    def _name(self) -> str:
        return f"solver '{self.solver_name or type(self).__name__}'"

    def _refuse_unsupported_prediction(self, zero_snr: bool, spacing: str):
        """every combination the v-prediction path does not cover is refused here, by name, before anything is built"""
        pt = self.prediction_type
        if pt not in ("epsilon", "v_prediction"):
            raise ValueError(f"prediction_type={pt!r}: 'epsilon' or 'v_prediction' ('sample'-prediction models are not supported)")
        if pt == "v_prediction" and self.scheduler_kind == "lightning":
            raise ValueError(f"{self._name()}: prediction_type='v_prediction' is not supported by the *_lightning solvers")
        if pt == "v_prediction" and not self.vpred_ok:
            raise ValueError(f"{self._name()}: prediction_type='v_prediction' is not supported by the inpaint solvers")
        if zero_snr and self.sigma_solver:
            raise ValueError(f"{self._name()}: zero_terminal_snr=True is not supported by the Karras-sigma solvers (euler*, dpm++_2m*, "
                             "dpm++_2s_a*): sigma_max is infinite")
        if zero_snr and pt == "epsilon":
            raise ValueError(f"{self._name()}: zero_terminal_snr=True needs prediction_type='v_prediction': the epsilon update divides by "
                             "sqrt(alpha_T) = 0")

    def _check_guidance_rescale(self, phi) -> float:
        phi = float(phi)
        if not 0.0 <= phi <= 1.0:
            raise ValueError(f"guidance_rescale={phi}: 0 (off) .. 1")
        if phi > 0.0 and self.prediction_type != "v_prediction":
            raise ValueError(f"{self._name()}: guidance_rescale={phi} needs prediction_type='v_prediction' (not supported for epsilon models)")
        if phi > 0.0 and not self.rescale_ok:
            raise ValueError(f"{self._name()}: guidance_rescale={phi} is supported by 'ddim' and 'ddim_cfg++' only (inversion, edit and "
                             "k-diffusion solvers refuse it)")
        return phi

    def _update_hook(self):
        """the ``update=`` of ``_ddim_loop``: None (``_ddim_update``, epsilon) or the v-prediction update"""
        return self._ddim_update_v if self.prediction_type == "v_prediction" else None

    def _ddim_update_v(self, zt, z0t, v_uc, v_c, lam, sqrt4, tweedie_uc, renoise_uc, device_alpha=None, last=False):
        """``_ddim_update`` for a v-prediction UNet: one cfgpp_step_ddim_v launch, after one cfgpp_cfg_rescale launch when
        guidance_rescale > 0 (include/cfgpp_vpred.h)"""
        co = K.ddim_v_coeffs_pinned(sqrt4, semantics=self.scalar_semantics, z_half=(zt.dtype == torch.float16), device_alpha=device_alpha)
        phi = self.guidance_rescale if self._job_rescale is None else self._job_rescale
        row_scale = self.engine.cfg_rescale(v_uc, v_c, lam, phi) if phi > 0.0 else None
        self.engine.step_ddim_v(zt, z0t, v_uc, v_c, lam, co, tweedie_uc, renoise_uc, row_scale)

    def _eps_from_v(self, noise_uc, noise_c, xc, sigma):
        """k-diffusion loops: the UNet's v at the scaled input ``xc`` -> eps, in place (one cfgpp_v_to_eps launch); a no-op for
        epsilon models"""
        if self.prediction_type == "v_prediction":
            a, s = K.v_to_eps_coeffs(sigma, self.scalar_semantics)
            self.engine.v_to_eps(noise_uc, noise_c, noise_uc, noise_c, xc, a, s)

    # ------------------------------------------------------------------ LoRA
    def set_lora(self, adapters, ignore_text_encoder: bool = False):
        """merge ``adapters`` = ``[(safetensors path | state dict | lora.parse_lora result, scale), ...]`` into the engine's UNet
        (``[]``: back to the base weights).  Takes effect with the next prediction; the conditioning cache follows the engine's
        ``lora_epoch``."""
        if not hasattr(self.engine, "set_lora"):
            raise ValueError(f"lora=...: the engine {type(self.engine).__name__} cannot merge LoRA adapters")
        self.engine.set_lora(adapters or [], ignore_text_encoder=ignore_text_encoder)

    def set_lora_scale(self, scale: float):
        """every adapter of the current set at ``scale`` (``sample(..., lora_scale=)``)"""
        eng = self.engine
        if not hasattr(eng, "set_lora"):
            raise ValueError(f"lora_scale=...: the engine {type(eng).__name__} cannot merge LoRA adapters")
        cur = eng.lora_adapters
        if any(float(s) != float(scale) for _, s in cur):
            eng.set_lora([(p, float(scale)) for p, _ in cur])

    # ------------------------------------------------------------------ FreeU
    def set_freeu(self, spec):
        """``(s1, s2, b1, b2)`` | mapping with those keys | None (off) for the engine's UNet (cfgpp_amd/freeu.py); takes effect
        with the next prediction"""
        from .freeu import parse_freeu
        vals = parse_freeu(spec)            # a bad spec is refused here, by name, before anything reaches the engine
        if not hasattr(self.engine, "set_freeu"):
            raise ValueError(f"freeu=...: the engine {type(self.engine).__name__} has no FreeU")
        self.engine.set_freeu(vals)

    @property
    def freeu(self):
        """the (s1, s2, b1, b2) in force, or None"""
        return getattr(self.engine, "freeu", None)

    # ------------------------------------------------------------------ IP-Adapter
    def set_ip_adapter(self, spec):
        """load an IP-Adapter into the engine's UNet (``ip_adapter.resolve``: "synthetic" | safetensors path | state dict), or drop
        it (None)"""
        if not hasattr(self.engine, "set_ip_adapter"):
            raise ValueError(f"ip_adapter=...: the engine {type(self.engine).__name__} cannot load an IP-Adapter")
        self.engine.set_ip_adapter(spec)
        self._ip_key = object()         # whatever image context the engine had is gone

    def _ip_prepare(self, ip, scale):
        """the image prompt of one sample() call -> (embeds, negative embeds | None, scale) or None"""
        emb, neg, img = ip["ip_adapter_image_embeds"], ip["negative_ip_adapter_image_embeds"], ip["ip_adapter_image"]
        if emb is None and img is None:
            if neg is not None:
                raise ValueError("negative_ip_adapter_image_embeds without ip_adapter_image_embeds / ip_adapter_image")
            return None
        if emb is not None and img is not None:
            raise ValueError("pass ip_adapter_image_embeds or ip_adapter_image, not both")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("IP-Adapter image prompts are not supported in sharded runs (world size > 1): the per-chain embeds are not sharded")
        if not hasattr(self.engine, "set_image_embeds") or getattr(self.engine, "ip_adapter", None) is None:
            raise ValueError("ip_adapter_image_embeds / ip_adapter_image given, but the solver has no IP-Adapter: "
                             "get_solver(..., ip_adapter=\"synthetic\" | path | state_dict)")
        if img is not None:                 # CLIP image tower, once per job: HIP launches (vision.HipClipImageTower) on a GPU device
            if self.image_encoder is None:
                if not self.ip_adapter_dir:
                    raise ValueError("ip_adapter_image needs the CLIP image encoder: get_solver(..., ip_adapter_dir=<folder holding image_encoder/>)")
                # the torch tower (ip_adapter.ImageEncoder) only on request, on a CPU device, or for a geometry the HIP tower
                # refuses by name (vision.last_image_tower_fallbacks records it)
                from .vision import build_image_encoder
                self.image_encoder = build_image_encoder(self.ip_adapter_dir, self.work_device, self.image_tower)
            if getattr(self.engine.ip_adapter, "seq_input", False):
                # a Resampler ("plus") adapter reads the tower's penultimate hidden states; its default negative is the tower on an
                # all-zero pixel tensor (the published pipeline's zeros_like of the preprocessed image), not zero hidden states
                emb = self.image_encoder(img, hidden=True)
                if neg is None:
                    neg = self.image_encoder.negative_hidden(img)
            else:
                emb = self.image_encoder(img)
        self._ip_serial += 1
        return (emb, neg, float(scale), self._ip_serial)

    def _ensure_image_context(self, ctx_changed: bool, uc, c):
        """after the text context: (re)project the call's image prompt, or switch the adapter off (once per sampling loop)"""
        job, eng = self._ip_job, self.engine
        if not hasattr(eng, "set_image_embeds"):
            return
        key = None if job is None else (job[3], uc is None, c is None)
        if not ctx_changed and self._ip_key == key:
            return
        if job is None:
            eng.set_image_embeds(None)
        else:
            emb, neg, scale = job[:3]
            if uc is None:                  # single forward on the conditional rows: both halves carry the image prompt
                neg = emb
            elif c is None:
                emb = torch.zeros_like(emb) if neg is None else neg
                neg = emb
            eng.set_image_embeds(emb, neg, scale)
        self._ip_key = key

    def _lora_epoch(self) -> int:
        return int(getattr(self.engine, "lora_epoch", 0))

    @contextlib.contextmanager
    def _control(self, image, scale):
        eng = self.engine
        if image is None:
            if getattr(eng, "control", None) is not None:
                eng.clear_control()
            yield
            return
        if self.controlnet is None:
            raise ValueError("control_image given, but the solver has no ControlNet: get_solver(..., controlnet=\"synthetic\" | path | state_dict)")
        if not torch.is_tensor(image) or image.dim() != 4 or int(image.shape[1]) != 3:
            raise ValueError(f"control_image must be a [1 or B, 3, 8h, 8w] tensor in [0, 1], got {getattr(image, 'shape', type(image))}")
        eng.set_control(self.controlnet, image, float(scale))
        try:
            yield
        finally:
            eng.clear_control()

    @torch.no_grad()
    def get_text_embed(self, null_prompt, prompt):
        """-> (null_text_embed [1 or B,77,D], text_embed [B,77,D]), fp16.  With ``max_prompt_chunks`` > 1: [.., 77 * j, D], the same
        j for both (cfgpp_amd/prompt.py)."""
        if self.max_prompt_chunks > 1:
            uc, c = self._long_text_embed(self.text_encoder, [as_list(null_prompt), as_list(prompt)])[0]
            return uc.to(self.work_device), c.to(self.work_device)
        uc, _ = self.text_encoder(as_list(null_prompt))
        c, _ = self.text_encoder(as_list(prompt))
        return uc.to(self.work_device), c.to(self.work_device)

    @staticmethod
    def _refuse_long_context_when_sharded(tokens: int):
        """sharded runs (world size > 1) take one 77-token chunk: every text context - from prompts or from ``prompt_embeds=`` -
        passes here before it reaches the engine"""
        if int(tokens) > 77:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError(f"a text context of {int(tokens)} tokens ({int(tokens) // 77} prompt chunks) in a sharded run (world size > 1) is "
                                 "not supported: the packed broadcast of the conditioning has the shapes of one 77-token chunk")

    def _long_text_embed(self, encoder, groups, n_chunks=None, clip_skip=None):
        """``groups`` of prompt lists (uncond, cond, ...) through ``prompt.encode_prompts`` at ONE chunk count, that of the longest
        prompt of all groups (or ``n_chunks`` if larger) -> ([hidden per group], [pooled per group], j)"""
        from . import prompt as P
        K = self.max_prompt_chunks
        j = max([P.chunks_needed(encoder, g, K) for g in groups] + [int(n_chunks or 1)])
        self._refuse_long_context_when_sharded(77 * j)
        enc = [P.encode_prompts(encoder, g, K, n_chunks=j, clip_skip=clip_skip) for g in groups]
        return [e[0] for e in enc], [e[1] for e in enc], j

    def _get_vae(self):
        if self.vae is None:
            if self.work_device.type != "cuda":      # CPU is only reachable with an injected (test) engine: inject the VAE too
                raise CfgppError("decode/encode need the HIP VAE (ROCm GPU); on CPU pass vae=<object with decode/encode>")
            from .vae import HipVAE                  # decoder + encoder on the HIP kernels; no fallback
            self.vae = HipVAE(self.cfg.vae_scale, self.latent_hw, max_batch=self.max_batch, device=self.work_device,
                              **self._vae_kwargs)
        return self.vae

    def encode(self, x):
        """xt -> zt (posterior sample * scale; latent_diffusion.py:117-121).  The reference's VAE runs in
        ``pipe_dtype`` (fp16), so the latent it returns - and with it the whole inversion / edit chain - is
        fp16; the HIP encoder's fp32 posterior sample is rounded to that dtype here."""
        return self._get_vae().encode(x.to(self.work_device)).to(self.dtype)

    def decode(self, zt):
        """zt -> xt (latent_diffusion.py:123-129)."""
        return self._get_vae().decode(zt.to(self.work_device))

    def predict_noise(self, zt: torch.Tensor, t, uc: Optional[torch.Tensor], c: Optional[torch.Tensor]):
        """epsilon_theta for null and condition (latent_diffusion.py:131-158).  One
        UNet launch over rows [uc_1..uc_B, c_1..c_B]; ``zt`` is read twice by index."""
        return self._predict(zt, t, uc, c)

    def _predict(self, zt, t, uc, c, added=None):
        """``predict_noise`` of both families; ``added``: SDXL's ``added_cond_kwargs``"""
        self._ensure_context(uc, c, added)
        noise_uc, noise_c = self.engine.predict(zt, float(t))
        if uc is None:
            return noise_c, noise_c
        if c is None:
            return noise_uc, noise_uc
        return noise_uc, noise_c

    def _ensure_context(self, uc, c, added=None):
        """(re)build the engine's conditioning when the embeddings changed (once per sampling loop)"""
        if uc is None and c is None:
            raise ValueError("predict_noise needs at least one of uc / c")
        a = c if uc is None else uc
        b = uc if c is None else c
        extra, extra_key = self._added_context(added)
        key = (a.data_ptr(), b.data_ptr(), tuple(a.shape), tuple(b.shape), a._version, b._version, self._lora_epoch(), *extra_key)
        job = self._region_job
        if self.max_regions > 1:
            key = (*key, job.serial if job is not None else 0)
        changed = getattr(self, "_ctx_key", None) != key
        if changed:
            self._refuse_long_context_when_sharded(max(int(a.shape[1]), int(b.shape[1])))      # (prompt_embeds= comes this way too)
            if job is not None:         # regional prompts: the stacked context, then the map the cross-attentions select by
                from .regions import stack_context
                nk = {} if job.negative_embeds is None else dict(negative_embeds=job.negative_embeds)      # [uc | uc_1 | ..]
                sa = stack_context(a, None, job.embeds, **nk)[0] if uc is not None else stack_context(None, a, job.embeds)[1]
                sb = stack_context(None, b, job.embeds)[1] if c is not None else stack_context(b, None, job.embeds, **nk)[0]
                self._set_context(sa, sb, *extra)
                if job.weights is not None:      # soft regions: the weights the cross-attentions blend by
                    self.engine.set_region_weights(job.weights)
                else:
                    self.engine.set_regions(job.ids, job.n_regions)
            else:
                self._set_context(a, b, *extra)
                if self.max_regions > 1 and getattr(self.engine, "regions", 0):
                    self.engine.set_regions(None)
            self._ctx_key = key
            self._ctx_keep = (a, b, *extra)
        self._ensure_image_context(changed, uc, c)

    def _added_context(self, added):
        """-> (tensors that travel with the text context, what they add to the cache key): none for SD1.5"""
        return (), ()

    # ------------------------------------------------------------------ regional prompts (cfgpp_amd/regions.py)
    def _region_hidden(self, prompt):
        """hidden states [1 or B, 77, D] of one region prompt: a plain 77-token prompt, through every text tower alike"""
        towers = self.text_encoder if isinstance(self.text_encoder, (tuple, list)) else (self.text_encoder,)
        return torch.cat([enc(as_list(prompt))[0] for enc in towers], dim=-1).to(self.work_device, torch.float16)

    def _regions_prepare(self, region_prompts, region_masks, control_image=None, ip=None, base_ratio=0.0, negative_prompts=None):
        """the region job of one sample() call, or None for a plain call (empty lists): refusals by name, the region map (or, on a
        soft_regions solver, the region weights), the hidden states of the region prompts and of their negative prompts"""
        from . import regions as RG
        R = RG.check_lists(region_prompts, region_masks, self.max_regions if self.max_regions > 1 else RG.MAX_REGIONS)
        beta = RG.check_base_ratio(base_ratio)
        if R == 1:
            if beta != 0.0 or negative_prompts:
                raise ValueError("region_base_ratio / region_negative_prompts given without region_prompts")
            return None
        if beta != 0.0 and not getattr(self, "soft_regions", False):
            raise ValueError(f"region_base_ratio={beta:g} needs a soft-regions solver: get_solver(..., max_regions=R, soft_regions=True) "
                             "(with soft_regions=False the masks are binarized into a hard partition and the ratio must be 0)")
        negatives = RG.check_negatives(negative_prompts, R - 1)
        if not self.controllable:
            raise ValueError(f"{type(self).__name__}.sample() does not take region_prompts: regional prompts are for the text-to-image "
                             "solvers (inversion, edit, inpaint and panorama solvers refuse them)")
        if self.max_regions < 2:
            raise ValueError(f"region_prompts given, but the solver was built with max_regions={self.max_regions}: "
                             "get_solver(..., max_regions=R) with R = 2 .. 4 sizes the engine for R regions")
        if control_image is not None:
            raise ValueError("control_image together with region_prompts is not supported (ControlNet with regions is not built)")
        if ip is not None and any(v is not None for v in ip.values()):
            raise ValueError("ip_adapter_image / ip_adapter_image_embeds together with region_prompts is not supported (IP-Adapter with regions is not built)")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("region_prompts in a sharded run (world size > 1) is not supported: the packed broadcast of the conditioning "
                             "has the shapes of one 77-token chunk")
        if not hasattr(self.engine, "set_regions"):
            raise ValueError(f"region_prompts: the engine {type(self.engine).__name__} has no set_regions")
        embeds = tuple(self._region_hidden(p) for p in region_prompts)
        B = max(int(e.shape[0]) for e in embeds)
        neg = None if negatives is None else tuple(None if n is None else self._region_hidden(n) for n in negatives)
        self._region_serial += 1
        if getattr(self, "soft_regions", False):
            if not hasattr(self.engine, "set_region_weights"):
                raise ValueError(f"soft_regions: the engine {type(self.engine).__name__} has no set_region_weights")
            w = RG.build_region_weights(list(region_masks), self.latent_hw, B if B > 1 else None, beta)
            return RG.RegionJob(None, embeds, self._region_serial, w, neg)
        ids = RG.build_region_map(list(region_masks), self.latent_hw, B if B > 1 else None)     # (B = 1: the engine checks the rows)
        if neg is None:
            return RG.RegionJob(ids, embeds, self._region_serial)
        return RG.RegionJob(ids, embeds, self._region_serial, None, neg)

    # ------------------------------------------------------------------ the DDIM step rule; whole-loop graph replay
    def _ddim_step_coeffs(self, t, inversion: bool, wrap: bool):
        """The DDIM step at timestep ``t`` -> (sqrt4, device_alpha), for the eager loop and the graph's step table alike.
        sqrt4: the pinned sqrt(at) etc. of at = alpha(t), at_prev = alpha(t - skip), swapped for an inversion.  device_alpha:
        which of the two is a DEVICE scalar (coeffs.py) - alpha(t - skip) of the step that leaves the table is
        ``final_alpha_cumprod.to(device)``: the renoising alpha ("rn") forward, the x0-estimate alpha ("tw") in an inversion.
        ``wrap`` (quirk Q3): SDXL's `ddim` loops index the shifted table unguarded and never take the final alpha."""
        sqrt4 = self.tables.ddim_sqrt_coeffs(t, wrap=wrap, inversion=inversion)
        if self.tables.timestep_spacing == "trailing":      # diffusers' indexing: abar[0] past the start is a table entry like the rest
            return sqrt4, None
        final = not wrap and int(t) - self.tables.skip < 0
        return sqrt4, (("tw" if inversion else "rn") if final else None)

    def _graph_loop(self, zt, ts, uc, c, lam, tweedie_uc, renoise_uc, inversion, wrap):
        """The DDIM loop with callback_fn None as hipGraph replays of ONE captured step (UNet + fused update; include/cfgpp.h:
        cfgpp_sample_graph_ddim) when the engine offers it ($CFGPP_GRAPH=1 on the HIP engine): the per-step scalars - exactly
        what the eager loop hands to ``predict`` / ``step_ddim`` - are computed up front.
        Returns (z0t, zt) or None when the eager loop has to run (mock engine, switch off, a v-prediction model: the captured
        step is the epsilon update)."""
        if not getattr(self.engine, "graph_enabled", False) or self.prediction_type != "epsilon":
            return None
        z_half = zt.dtype == torch.float16
        steps = []
        for t in ts:
            sqrt4, dev_a = self._ddim_step_coeffs(t, inversion, wrap)
            co = K.ddim_coeffs_pinned(sqrt4, eps_half=True, semantics=self.scalar_semantics, z_half=z_half, device_alpha=dev_a)
            steps.append((float(t), *[float(v) for v in co]))
        single = "c" if uc is None else ("uc" if c is None else "")
        return self.engine.ddim_loop_graph(zt, steps, lam, tweedie_uc, renoise_uc, single)

    def _set_context(self, uc, c):
        self.engine.set_context(uc, c)

    # ------------------------------------------------------------------ latents
    def initialize_latent(self, method: str = "random", src_img: Optional[torch.Tensor] = None, **kwargs):
        if method == "ddim":
            z = self.inversion(self.encode(src_img.to(self.dtype)), kwargs.get("uc"), kwargs.get("c"),
                               cfg_guidance=kwargs.get("cfg_guidance", 0.0))
        elif method == "npi":
            z = self.inversion(self.encode(src_img.to(self.dtype)), kwargs.get("c"), kwargs.get("c"), cfg_guidance=1.0)
        elif method in ("random", "random_kdiffusion"):
            size = tuple(kwargs.get("latent_dim", (1, self.cfg.out_channels) + self.latent_hw))
            z = self._randn(size, kwargs.get("seeds"))
            if method == "random_kdiffusion":
                sigmas = kwargs.get("sigmas", [14.6146])
                z = z * (sigmas[0] ** 2 + 1) ** 0.5
            z = z.to(self.work_device)
        else:
            raise NotImplementedError
        return z

    @staticmethod
    def _randn(size, seeds=None) -> torch.Tensor:
        """CPU-generator noise, as the reference draws it (latent_diffusion.py:200).
        With ``seeds`` chain b is ``torch.manual_seed(s_b); torch.randn(1, ...)``."""
        if seeds is None:
            return torch.randn(size)
        if len(seeds) != size[0]:
            raise ValueError(f"{len(seeds)} seeds for a batch of {size[0]}")
        out = []
        for s in seeds:
            g = torch.Generator().manual_seed(int(s))
            out.append(torch.randn((1,) + tuple(size[1:]), generator=g))
        return torch.cat(out, dim=0)

    @staticmethod
    def _chain_seeds(seeds, B: int, who: str) -> List[int]:
        """the 64-bit seeds that key the chains' in-kernel noise (include/cfgpp_lcm.h): the caller's ``seeds`` - the ones that made the
        start latent - or, with None, B values drawn once per job from torch's CPU generator.  A sharded run has to pass its rank's
        seeds: ranks that draw their own would repeat each other's noise."""
        if seeds is None:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise ValueError(f"{who} in a sharded run (world size > 1) needs seeds=[...] for this rank's chains: ranks that draw "
                                 "their own seeds would repeat each other's noise")
            return [int(v) for v in torch.randint(0, 2 ** 63 - 1, (int(B),), dtype=torch.int64)]
        if len(seeds) != int(B):
            raise ValueError(f"{len(seeds)} seeds for a batch of {B}")
        return [int(s) for s in seeds]

    # ------------------------------------------------------------------ k-diffusion helpers
    def timestep(self, sigma):
        return self.tables.timestep(sigma)

    def to_d(self, x, sigma, denoised):
        return (x - denoised) / sigma.item()

    get_ancestral_step = staticmethod(get_ancestral_step)

    def calculate_input(self, x, sigma):
        return x / (sigma ** 2 + 1) ** 0.5

    def calculate_denoised(self, x, model_pred, sigma):
        return x - model_pred * sigma

    # ------------------------------------------------------------------ fused loops
    def _ddim_update(self, zt, z0t, noise_uc, noise_c, lam, sqrt4, tweedie_uc, renoise_uc, device_alpha=None, last=False):
        co = K.ddim_coeffs_pinned(sqrt4, eps_half=(noise_uc.dtype == torch.float16), semantics=self.scalar_semantics,
                                  z_half=(zt.dtype == torch.float16), device_alpha=device_alpha)
        self.engine.step_ddim(zt, z0t, noise_uc, noise_c, lam, co, tweedie_uc, renoise_uc)

    def _own_latent(self, z):
        """private, contiguous copy on the engine device (the loops update it in place); fp16 stays fp16
        (the reference's inversion / edit latents), everything else runs as fp32 like ``torch.randn``."""
        dt = torch.float16 if z.dtype == torch.float16 else torch.float32
        return z.detach().to(device=self.work_device, dtype=dt, copy=True).contiguous()

    def _run_callback(self, callback_fn, step, t, z0t, zt):
        kw = callback_fn(step, t, {"z0t": z0t.detach(), "zt": zt.detach(), "decode": self.decode})
        if kw["z0t"] is not z0t:
            z0t.copy_(kw["z0t"])
        if kw["zt"] is not zt:
            zt.copy_(kw["zt"])

    def _ddim_loop(self, zt, uc, c, lam, tweedie_uc: bool, renoise_uc: bool, *, inversion=False, wrap=False, added=None, ts=None,
                   callback_fn=None, desc="SD", update=None):
        """THE DDIM loop of both families: reverse DDIM / DDIM-CFG++ (latent_diffusion.py:272-294 / 652-674, latent_sdxl.py:
        425-467 / 679-703) and, with ``inversion``, DDIM inversion over the reversed timesteps (latent_diffusion.py:160-182 CFG,
        888-910 CFG++; latent_sdxl.py:301-320).  ``tweedie_uc`` / ``renoise_uc``: eps_uc rather than eps_hat in the x0
        estimate / the renoising.  ``zt`` [B,4,H,W]: fp32 (text-to-image: ``torch.randn``) or fp16 (an inversion that starts
        from the fp16 VAE latent, and the regeneration after it); a private copy is updated in place.  ``added``: SDXL's
        ``added_cond_kwargs``; ``ts``: other timesteps than the scheduler's; ``update``: another fused update than
        ``_ddim_update``, same arguments (``last``: the loop's last step).  Returns (z0t, zt)."""
        zt = self._own_latent(zt)
        if ts is None:
            ts = self.scheduler.timesteps.flip(0) if inversion else self.scheduler.timesteps
        ts = ts.int() if wrap else ts
        self._ensure_context(uc, c, added)
        if callback_fn is None:
            done = self._graph_loop(zt, ts, uc, c, lam, tweedie_uc, renoise_uc, inversion, wrap)
            if done is not None:
                return done
        update = update or self._ddim_update
        z0t = torch.empty_like(zt)
        n = len(ts)
        for step, t in enumerate(_progress(ts, desc)):
            sqrt4, dev_a = self._ddim_step_coeffs(t, inversion, wrap)
            noise_uc, noise_c = self._predict(zt, t, uc, c, added)
            update(zt, z0t, noise_uc, noise_c, lam, sqrt4, tweedie_uc, renoise_uc, dev_a, last=(step == n - 1))
            if callback_fn is not None:
                self._run_callback(callback_fn, step, t, z0t, zt)
        return z0t, zt

    inversion_cfgpp = False     # CFG++ inversion: x0 from eps_uc (the renoising keeps eps_hat)

    @torch.no_grad()
    def inversion(self, z0, uc, c, cfg_guidance: float = 1.0):
        return self._ddim_loop(z0, uc, c, cfg_guidance, self.inversion_cfgpp, False, inversion=True, desc="DDIM Inversion",
                               update=self._update_hook())[1]

    def _result(self, return_latents, latents, z):
        """what ``sample`` returns: ``latents`` when asked for them, else the decoded image of ``z``"""
        return latents if return_latents else self._finish(z)

    def _finish(self, z):
        if os.environ.get("CFGPP_TRACE"):
            torch.cuda.synchronize() if z.is_cuda else None
            print("[cfgpp] sampling loop done, decoding", file=sys.stderr, flush=True)
        vae = self._get_vae()
        if hasattr(vae, "decode_image"):        # HIP VAE: `/ 2 + 0.5` and the clamp are folded into its last kernel
            img = vae.decode_image(z.to(self.work_device))
        else:
            img = (self.decode(z) / 2 + 0.5).clamp(0, 1)
        return img.detach().cpu()

    def _embeds(self, prompt, kwargs, n_cond=1):
        """(uc, c_1, ..) either from ``prompt_embeds=`` or from the text encoder."""
        pe = kwargs.get("prompt_embeds")
        if pe is not None:
            return tuple(e.to(self.work_device, torch.float16) for e in pe)
        if self.max_prompt_chunks > 1:     # every prompt of the call at one chunk count
            hs = self._long_text_embed(self.text_encoder, [as_list(prompt[k]) for k in range(1 + n_cond)])[0]
            return tuple(h.to(self.work_device) for h in hs)
        out = []
        uc = None
        for k in range(n_cond):
            uc, c = self.get_text_embed(null_prompt=prompt[0], prompt=prompt[1 + k])
            out.append(c)
        return (uc, *out)

    def _batch_of(self, c, kwargs):
        return int(c.shape[0])

    # ------------------------------------------------------------------ k-diffusion loop
    def _kdiff_start(self, size, sigmas, seeds):
        """randn * sqrt(sigma0^2 + 1) in fp32, then cast: the fp16 start latent of the Karras-sigma loops (latent_sdxl.py:290-294)"""
        return self.initialize_latent(method="random_kdiffusion", latent_dim=size, sigmas=sigmas, seeds=seeds).to(torch.float16).contiguous()

    def _kdiff_loop(self, x, sigmas, uc, c, cfg_guidance, variant: int, solver: str, callback_fn=None, *, added=None, n_steps=None,
                    alphas=None, xl_form=False, t_of_sigma=None, desc="SD"):
        """THE Euler / DPM++2M loop of both families (CFG: variant 0, CFG++: variant 1, SDXL's 2M CFG++: variant 2 with
        ``xl_form``) on ``sigmas`` from the fp16 start latent ``x``, updated in place (latent_diffusion.py:302-346, 454-503,
        682-723, 830-879; latent_sdxl.py:469-517, 757-808, 860-930).  The UNet input is ``x / sqrt(sigma^2 + 1)``, or with
        ``alphas`` ``x * sqrt(alphas[i])``; ``t_of_sigma``: ``self.timestep`` unless given; ``added``: SDXL's
        ``added_cond_kwargs``.  Returns (denoised, x)."""
        xc, den, old = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        t_of_sigma = t_of_sigma or self.timestep
        have_old = False
        for i in _progress(range(len(self.scheduler.timesteps) if n_steps is None else n_steps), desc):
            sigma = sigmas[i]
            new_t = t_of_sigma(sigma)
            if alphas is None:
                self.engine.kdiff_input(x, xc, K.kdiff_input_scale_sd(sigma, self.scalar_semantics), 0)
            else:
                self.engine.kdiff_input(x, xc, float(alphas[i].clone().sqrt()), 1)
            noise_uc, noise_c = self._predict(xc, new_t, uc, c, added)
            self._eps_from_v(noise_uc, noise_c, xc, sigma)
            first = (solver == "euler") or (not have_old)
            coef, euler = K.kdiff_coeffs(cfg_guidance, sigmas, i, first, xl_form=xl_form, semantics=self.scalar_semantics)
            self.engine.step_kdiff(x, den, old, noise_uc, noise_c, coef, variant, xl_form, euler, solver != "euler")
            have_old = True
            if callback_fn is not None:
                self._run_callback(callback_fn, i, new_t, den, x)
        return den, x

    # ------------------------------------------------------------------ ancestral k-diffusion loops
    def _ancestral_loop(self, uc, c, cfg_guidance, cfgpp: bool, two_stage: bool, callback_fn=None, seeds=None):
        """Euler-ancestral (latent_diffusion.py:349-390 / 726-766) and DPM-Solver++(2S)-ancestral
        (:393-451 / 769-827; two UNet calls per step) on Karras sigmas, fp16 latent.  The injected noise
        is drawn with ``engine.randn_like`` (device RNG on the GPU, like the reference's torch.randn_like)."""
        B = self._batch_of(c, None)
        lam = cfg_guidance
        sigmas = self.tables.karras_sigmas()
        x = self._kdiff_start((B, self.cfg.out_channels) + self.latent_hw, sigmas, seeds)
        xc, den, uden = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        x2, den2, uden2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        # noise="philox": the injected noise comes from the seeded counter-based generator (cfgpp_philox_normal, stream 1, draw =
        # step) into one preallocated buffer - chain b of a batch then equals chain b alone; "torch" (default): randn_like, as ever
        philox = self.noise == "philox"
        if philox:
            job_seeds, nbuf = self._chain_seeds(seeds, B, f"{self._name()} with noise='philox'"), torch.empty_like(x)
        variant = 1 if cfgpp else 0
        sem = self.scalar_semantics
        t_fn = lambda sg: sg.log().neg()       # noqa: E731
        sigma_fn = lambda tt: tt.neg().exp()   # noqa: E731
        first = lambda sc: K._first(K._s(sc), True, sem)   # noqa: E731  scalar written first in `s * fp16`
        n = len(self.scheduler.timesteps)
        for i in _progress(range(n), "SD"):
            sigma = sigmas[i]
            new_t = self.timestep(sigma)
            sigma_down, sigma_up = get_ancestral_step(sigmas[i], sigmas[i + 1])
            self.engine.kdiff_input(x, xc, K.kdiff_input_scale_sd(sigma, self.scalar_semantics), 0)
            noise_uc, noise_c = self.predict_noise(xc, new_t, uc, c)
            self._eps_from_v(noise_uc, noise_c, xc, sigma)
            if (not two_stage) or float(sigma_down) == 0.0:
                # Euler step down to sigma_down: x = den + ((x - d_from)/sigma) * sigma_down
                # (`/ sigma.item()` in to_d, latent_diffusion.py:216-218, is a python-number divisor: K.divisor applies the backend rule)
                coef = [float(lam), float(sigma), 0.0, K.divisor(sigma.item(), sem), float(sigma_down), 0.0, 0.0, 1.0, 0.0]
                self.engine.step_kdiff(x, den, None, noise_uc, noise_c, coef, variant, False, True, False)
            else:
                self.engine.kdiff_denoise(x, noise_uc, noise_c, lam, float(sigma), den, uden)
                t, t_next = t_fn(sigmas[i]), t_fn(K._s(sigma_down))
                r = 1 / 2
                h = t_next - t
                s_mid = t + r * h
                # x_2 = (sigma(s)/sigma(t)) * x - expm1(-h r) * (den | uden)
                self.engine.lincomb(x2, x, uden if cfgpp else den, None, first(sigma_fn(s_mid) / sigma_fn(t)),
                                    first((-h * r).expm1()), 0)
                sigma_s = sigma_fn(s_mid)
                t_2 = self.timestep(sigma_s)
                self.engine.kdiff_input(x2, xc, K.kdiff_input_scale_sd(sigma_s, self.scalar_semantics), 0)
                nuc2, nc2 = self.predict_noise(xc, t_2, uc, c)
                self._eps_from_v(nuc2, nc2, xc, sigma_s)
                self.engine.kdiff_denoise(x2, nuc2, nc2, lam, float(sigma_s), den2, uden2)
                ratio_n = first(sigma_fn(t_next) / sigma_fn(t))
                if cfgpp:   # x = den_2 - exp(-h) * uden_2 + ratio * x
                    self.engine.lincomb(x, x, den2, uden2, ratio_n, first(torch.exp(-h)), 1)
                else:       # x = ratio * x - expm1(-h) * den_2
                    self.engine.lincomb(x, x, den2, None, ratio_n, first((-h).expm1()), 0)
            if sigmas[i + 1] > 0:
                noise = self.engine.philox_normal(nbuf, job_seeds, i, 1) if philox else self.engine.randn_like(x)
                self.engine.lincomb(x, x, noise, None, float(sigma_up), 0.0, 2)
            if callback_fn is not None:
                self._run_callback(callback_fn, i, new_t, den, x)
        return den, x


# ======== plain-CFG solvers (eps_hat used for both the x0 estimate and the renoising) ========
def _sd_prompts(prompt):
    return prompt


@register_solver("ddim")
class BaseDDIM(StableDiffusion):
    """Basic DDIM solver for SD (reference: latent_diffusion.py:247-299)."""
    cfgpp = False
    rescale_ok = True

    @torch.no_grad()
    @controlled
    def sample(self, cfg_guidance=7.5, prompt=["", ""], callback_fn=None, **kwargs):
        uc, c = self._embeds(prompt, kwargs)
        B = int(c.shape[0])
        zt = kwargs.get("latents")
        if zt is None:
            zt = self.initialize_latent(latent_dim=(B, self.cfg.out_channels) + self.latent_hw, seeds=kwargs.get("seeds"))
        z0t, zt = self._ddim_loop(zt.to(self.work_device), uc, c, cfg_guidance, False, self.cfgpp, callback_fn=callback_fn,
                                  update=self._update_hook())
        return self._result(kwargs.get("return_latents"), (z0t, zt), z0t)


@register_solver("euler")
class EulerCFGSolver(StableDiffusion):
    """Karras Euler, VE casted (reference: latent_diffusion.py:302-346)."""
    variant, solver = 0, "euler"
    sigma_solver = True

    @torch.no_grad()
    @controlled
    def sample(self, cfg_guidance, prompt=["", ""], callback_fn=None, **kwargs):
        uc, c = self._embeds(prompt, kwargs)
        sigmas = self.tables.karras_sigmas()
        x = self._kdiff_start((int(c.shape[0]), self.cfg.out_channels) + self.latent_hw, sigmas, kwargs.get("seeds"))
        den, x = self._kdiff_loop(x, sigmas, uc, c, cfg_guidance, self.variant, self.solver, callback_fn)
        # Euler decodes `denoised`, 2M decodes `x`
        return self._result(kwargs.get("return_latents"), (den, x), den if self.solver == "euler" else x)


@register_solver("euler_a")
class EulerAncestralCFGSolver(StableDiffusion):
    """Karras Euler + ancestral sampling (reference: latent_diffusion.py:349-390)."""
    cfgpp, two_stage = False, False
    sigma_solver = True
    ancestral = True

    @torch.no_grad()
    @controlled
    def sample(self, cfg_guidance, prompt=["", ""], callback_fn=None, **kwargs):
        uc, c = self._embeds(prompt, kwargs)
        den, x = self._ancestral_loop(uc, c, cfg_guidance, self.cfgpp, self.two_stage, callback_fn, kwargs.get("seeds"))
        # Euler-a decodes `denoised`, 2S-a decodes `x`
        return self._result(kwargs.get("return_latents"), (den, x), x if self.two_stage else den)


@register_solver("dpm++_2s_a")
class DPMpp2sAncestralCFGSolver(EulerAncestralCFGSolver):
    """DPM-Solver++(2S) ancestral, two UNet calls per step (reference: latent_diffusion.py:393-451)."""
    cfgpp, two_stage = False, True


@register_solver("dpm++_2m")
class DPMpp2mCFGSolver(EulerCFGSolver):
    """DPM-Solver++(2M) with CFG (reference: latent_diffusion.py:454-503)."""
    variant, solver = 0, "dpm2m"


@register_solver("ddim_inversion")
class InversionDDIM(BaseDDIM):
    """Invert with CFG then reconstruct (reference: latent_diffusion.py:506-558)."""
    controllable = False
    rescale_ok = False

    def _invert(self, src_img, uc, c, cfg_guidance, kwargs):
        z0 = kwargs.get("src_latent")
        if z0 is None:
            z0 = self.encode(src_img.to(self.dtype))
        return self.inversion(z0, uc, c, cfg_guidance=cfg_guidance)

    @torch.no_grad()
    @controlled
    def sample(self, src_img=None, cfg_guidance=7.5, prompt=["", "", ""], callback_fn=None, **kwargs):
        uc, c = self._embeds(prompt, kwargs)
        zt = self._invert(src_img, uc, c, cfg_guidance, kwargs)
        z0t, zt = self._ddim_loop(zt, uc, c, cfg_guidance, False, self.cfgpp, callback_fn=callback_fn, update=self._update_hook())
        return self._result(kwargs.get("return_latents"), (z0t, zt), z0t)


@register_solver("ddim_edit")
class EditWordSwapDDIM(InversionDDIM):
    """Invert with the source prompt, regenerate with the target prompt
    (reference: latent_diffusion.py:561-612)."""

    @torch.no_grad()
    @controlled
    def sample(self, src_img=None, cfg_guidance=7.5, prompt=["", "", ""], callback_fn=None, **kwargs):
        uc, src_c, tgt_c = self._embeds(prompt, kwargs, n_cond=2)
        zt = self._invert(src_img, uc, src_c, cfg_guidance, kwargs)
        z0t, zt = self._ddim_loop(zt, uc, tgt_c, cfg_guidance, False, self.cfgpp, callback_fn=callback_fn, desc="DDIM-edit",
                                  update=self._update_hook())
        return self._result(kwargs.get("return_latents"), (z0t, zt), z0t)


# ======== CFG++ solvers (renoise with eps_uc; small-lambda regime) ========
@register_solver("ddim_cfg++")
class BaseDDIMCFGpp(BaseDDIM):
    """DDIM with CFG++: renoise with eps_uc (reference: latent_diffusion.py:621-679)."""
    cfgpp = True


@register_solver("euler_cfg++")
class EulerCFGppSolver(EulerCFGSolver):
    """reference: latent_diffusion.py:682-723 (d from uncond_denoised)."""
    variant, solver = 1, "euler"


@register_solver("euler_a_cfg++")
class EulerAncestralCFGppSolver(EulerAncestralCFGSolver):
    """reference: latent_diffusion.py:726-766 (d from uncond_denoised)."""
    cfgpp, two_stage = True, False


@register_solver("dpm++_2s_a_cfg++")
class DPMpp2sAncestralCFGppSolver(EulerAncestralCFGSolver):
    """reference: latent_diffusion.py:769-827 (x_2 from uncond_denoised; x = D_2 - e^{-h} D_uc,2 + ratio x)."""
    cfgpp, two_stage = True, True


@register_solver("dpm++_2m_cfg++")
class DPMpp2mCFGppSolver(EulerCFGSolver):
    """DPM-Solver++(2M) with CFG++ (reference: latent_diffusion.py:830-879)."""
    variant, solver = 1, "dpm2m"


@register_solver("ddim_inversion_cfg++")
class InversionDDIMCFGpp(InversionDDIM):
    """CFG++ inversion (x0 from eps_uc, renoise eps_hat) + CFG++ reconstruction
    (reference: latent_diffusion.py:882-957)."""
    cfgpp = inversion_cfgpp = True


@register_solver("ddim_edit_cfg++")
class EditWordSwapDDIMCFGpp(EditWordSwapDDIM):
    """reference: latent_diffusion.py:959-1010."""
    cfgpp = inversion_cfgpp = True


if __name__ == "__main__":
    print(f"Possble solvers: {[x for x in __SOLVER__.keys()]}")
