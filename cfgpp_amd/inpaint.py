"""Inpainting solvers: repaint the masked region of an image, keep the rest (DDIM and DDIM-CFG++, SD1.5 and SDXL).

Two model kinds, as in diffusers' ``StableDiffusionInpaintPipeline`` / ``StableDiffusionXLInpaintPipeline``:

* a dedicated inpaint UNet (``unet_config.SD15_INPAINT`` / ``SDXL_INPAINT``: ``conv_in`` takes 9 channels).  The mask and
  the masked image's latent are the step-invariant extra input channels (``engine.image_condition``, once per job: the
  pipelines' per-step ``torch.cat([latents, mask, masked_image_latents], 1)``); the loop is the text-to-image DDIM loop with
  the plain fused step, graph replay included.
* an ordinary 4-channel UNet.  Every step is the fused masked update ``engine.step_ddim_masked``: outside the mask the
  latent is replaced by the source latent, forward-noised to the step's next timestep (``(1, 0)`` - the clean source - on
  the last step), in the same pass as the DDIM update.  Always the eager loop.

These solvers are NOT in the ``latent_diffusion`` / ``latent_sdxl`` registries (those mirror the reference's lists); they
have their own: ``get_inpaint_solver(name, model="sd15" | "sdxl", **get_solver kwargs)``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from . import coeffs as K
from .latent_diffusion import StableDiffusion, controlled
from .latent_sdxl import SDXL
from .registry import Registry

__INPAINT_SOLVER__ = Registry("InpaintSolver")
MODELS = ("sd15", "sdxl")


def register_inpaint_solver(name: str, model: str):
    return __INPAINT_SOLVER__.register(f"{model}/{name}")


def get_inpaint_solver(name: str, model: str = "sd15", **kwargs):
    """``name`` in {"ddim_inpaint", "ddim_inpaint_cfg++"}, ``model`` in {"sd15", "sdxl"}; kwargs as ``get_solver``'s
    (``unet_config=SD15_INPAINT`` / ``SDXL_INPAINT`` or a checkpoint directory's ``solver_kwargs_from_dir`` select the
    9-channel kind)."""
    if model not in MODELS:
        raise ValueError(f"InpaintSolver model {model!r}: one of {MODELS}")
    try:
        cls = __INPAINT_SOLVER__[f"{model}/{name}"]
    except KeyError:
        raise ValueError(f"InpaintSolver {name} does not exist.") from None
    return cls(**kwargs)


def inpaint_solver_names():
    return sorted({k.split("/", 1)[1] for k in __INPAINT_SOLVER__})


# ---------------------------------------------------------------------------------------------------- job preparation (host)
def prepare_mask(mask: torch.Tensor, src_img: torch.Tensor, latent_hw: Tuple[int, int]):
    """diffusers' ``prepare_mask_and_masked_image`` + the latent-size mask of ``prepare_mask_latents``:
    -> (binary pixel mask [Bm,1,8h,8w] fp32, masked image ``src_img * (mask < 0.5)``, latent mask [Bm,1,h,w] fp32).
    The mask is binarized at 0.5 (1 = repaint); the latent mask is the nearest-neighbour downsample, pixel (8i, 8j)."""
    m = (mask.float() >= 0.5).to(torch.float32)
    masked_image = src_img.float() * (m < 0.5)
    lmask = F.interpolate(m, size=tuple(latent_hw))
    return m, masked_image, lmask


def strength_timesteps(timesteps: torch.Tensor, strength: float):
    """diffusers ``get_timesteps``: ``init = min(int(N * strength), N)``; the loop runs ``timesteps[N - init:]``.
    -> (the timesteps the loop runs, index of the first)."""
    N = len(timesteps)
    init = min(int(N * float(strength)), N)
    if init < 1:
        raise ValueError(f"strength={strength} leaves no denoising step of {N}")
    start = N - init
    return timesteps[start:], start


class _InpaintMixin:
    """shared by the SD1.5 and SDXL classes: mask / source preparation, the start latent, the masked update"""

    cfgpp = False
    controllable = False        # ControlNet on inpaint UNets is not supported: sample() refuses control_image
    vpred_ok = False            # the masked update and the forward-noised source are epsilon arithmetic: v-prediction is refused

    @property
    def inpaint_unet(self) -> bool:
        """a 9-channel UNet (mask + masked-image latent as input channels) rather than the masked update"""
        return self.cfg.in_channels > self.cfg.out_channels

    def _graph_loop(self, *args, **kwargs):
        if getattr(self, "_blend", None) is not None:       # the masked update has no graph form: eager loop
            return None
        return super()._graph_loop(*args, **kwargs)

    def _prepare_job(self, src_img, mask, strength, B: int, seeds, wrap: bool):
        """once per job, off the per-step path.  Sets the engine's image condition (9-channel UNet) or ``self._blend``
        (4-channel UNet).  -> (start latent fp32 [B,4,h,w], timesteps of the loop)."""
        if src_img is None or mask is None:
            raise ValueError("inpainting needs src_img and mask")
        h, w = self.latent_hw
        lc = self.cfg.out_channels
        if src_img.dim() != 4 or tuple(src_img.shape[1:]) != (3, 8 * h, 8 * w) or int(src_img.shape[0]) not in (1, B):
            raise ValueError(f"src_img shape {tuple(src_img.shape)}: expected [{B} or 1, 3, {8 * h}, {8 * w}]")
        if mask.dim() != 4 or tuple(mask.shape[1:]) != (1, 8 * h, 8 * w) or int(mask.shape[0]) not in (1, B):
            raise ValueError(f"mask shape {tuple(mask.shape)}: expected [{B} or 1, 1, {8 * h}, {8 * w}]")
        dev = self.work_device
        src_img = src_img.float()
        _, masked_image, lmask = prepare_mask(mask, src_img, (h, w))
        ts, _ = strength_timesteps(self.scheduler.timesteps, strength)
        noise = self._randn((B, lc, h, w), seeds).to(dev)
        z_src = None
        if not self.inpaint_unet or float(strength) < 1.0:
            z_src = self.encode(src_img).to(dev).expand(B, -1, -1, -1).contiguous()          # fp16, like the fp16 pipeline's
        self._blend = None
        if self.inpaint_unet:
            rows = 1 if (int(src_img.shape[0]) == 1 and int(mask.shape[0]) == 1) else B
            ml = self.encode(masked_image).to(dev)
            cond = torch.cat([lmask.to(dev, torch.float16).expand(rows, -1, -1, -1), ml.to(torch.float16).expand(rows, -1, -1, -1)], 1)
            self.engine.image_condition(cond.contiguous())
        else:
            m8 = (lmask > 0.5).to(torch.uint8).expand(B, -1, -1, -1).contiguous().to(dev)
            self._blend = (m8, z_src, noise.contiguous())
        if float(strength) < 1.0:
            c1, c2 = self.tables.ddim_sqrt_coeffs(ts[0], wrap=wrap)[:2]      # sqrt(1 - a_t0), sqrt(a_t0)
            zt = c2 * z_src.float() + c1 * noise
        else:
            zt = noise
        return zt, ts

    def _masked_update(self, zt, z0t, noise_uc, noise_c, lam, sqrt4, tweedie_uc, renoise_uc, device_alpha=None, last=False):
        """``_ddim_update`` with the fused masked update (4-channel UNet; fp32 latent, fp16 eps)"""
        mask, z_src, noise = self._blend
        co = K.ddim_coeffs_pinned(sqrt4, eps_half=True, semantics=self.scalar_semantics, z_half=False, device_alpha=device_alpha)
        # the source forward-noised to this step's target timestep; the clean source after the last step
        a, b = (1.0, 0.0) if last else (sqrt4[2], sqrt4[3])
        self.engine.step_ddim_masked(zt, z0t, noise_uc, noise_c, lam, co, tweedie_uc, renoise_uc, mask, z_src, noise, a, b)

    def _inpaint_loop(self, zt, ts, uc, c, lam, wrap: bool, added=None, callback_fn=None, desc="inpaint"):
        """the DDIM loop over ``ts``: the plain update for a 9-channel UNet, the masked one otherwise; returns (z0t, zt)"""
        return self._ddim_loop(zt, uc, c, lam, False, self.cfgpp, wrap=wrap, added=added, ts=ts, callback_fn=callback_fn, desc=desc,
                               update=None if self._blend is None else self._masked_update)


# ---------------------------------------------------------------------------------------------------- SD1.5
class InpaintDDIM(_InpaintMixin, StableDiffusion):
    """SD1.5 inpainting, DDIM with CFG (eps_hat renoises)."""

    @torch.no_grad()
    @controlled
    def sample(self, cfg_guidance=7.5, prompt=["", ""], src_img=None, mask=None, strength: float = 1.0, callback_fn=None,
               **kwargs):
        """``src_img`` [B or 1,3,8h,8w] in [-1, 1]; ``mask`` [B or 1,1,8h,8w] in [0, 1], 1 = repaint (binarized at 0.5).
        ``strength`` < 1 starts from the source noised to the first of the last ``int(N * strength)`` timesteps.  With an
        all-ones mask on a 4-channel UNet this is image-to-image (SDEdit).  -> the decoded image of the last step's z0t,
        or ``(z0t, zt)`` with ``return_latents=True``."""
        uc, c = self._embeds(prompt, kwargs)
        B = int(c.shape[0])
        zt, ts = self._prepare_job(src_img, mask, strength, B, kwargs.get("seeds"), wrap=False)
        z0t, zt = self._inpaint_loop(zt, ts, uc, c, cfg_guidance, False, callback_fn=callback_fn, desc="SD-inpaint")
        return self._result(kwargs.get("return_latents"), (z0t, zt), z0t)


class InpaintDDIMCFGpp(InpaintDDIM):
    """SD1.5 inpainting, DDIM with CFG++ (renoise with eps_uc)."""
    cfgpp = True


register_inpaint_solver("ddim_inpaint", "sd15")(InpaintDDIM)
register_inpaint_solver("ddim_inpaint_cfg++", "sd15")(InpaintDDIMCFGpp)


# ---------------------------------------------------------------------------------------------------- SDXL
class InpaintDDIMXL(_InpaintMixin, SDXL):
    """SDXL inpainting, DDIM with CFG; the SDXL DDIM loop's index rule (quirk Q3: ``wrap``).  ``sample`` is SDXL's
    (prompt1 / prompt2 or prompt_embeds, size conditioning) plus ``src_img``, ``mask``, ``strength``, ``seeds``; a single
    ``prompt=[null, text]`` is taken for both towers.  ``return_latents=True`` returns the last z0t."""

    @torch.no_grad()
    @controlled
    def sample(self, *args, **kwargs):
        p = kwargs.pop("prompt", None)
        if p is not None:
            kwargs.setdefault("prompt1", p)
            kwargs.setdefault("prompt2", p)
        if "shape" not in kwargs and kwargs.get("target_size") is None:
            h, w = self.latent_hw
            kwargs["target_size"] = (8 * h, 8 * w)
            kwargs.setdefault("original_size", (8 * h, 8 * w))
        return super().sample(*args, **kwargs)

    def reverse_process(self, null_prompt_embeds, prompt_embeds, cfg_guidance, add_cond_kwargs, shape=(1024, 1024),
                        callback_fn=None, src_img=None, mask=None, strength: float = 1.0, seeds=None, **kwargs):
        B = int(prompt_embeds.shape[0])
        zt, ts = self._prepare_job(src_img, mask, strength, B, seeds, wrap=True)
        return self._inpaint_loop(zt, ts, null_prompt_embeds, prompt_embeds, cfg_guidance, True, add_cond_kwargs, callback_fn,
                                  "SDXL-inpaint")[0]


class InpaintDDIMXLCFGpp(InpaintDDIMXL):
    """SDXL inpainting, DDIM with CFG++ (renoise with eps_uc)."""
    cfgpp = True


register_inpaint_solver("ddim_inpaint", "sdxl")(InpaintDDIMXL)
register_inpaint_solver("ddim_inpaint_cfg++", "sdxl")(InpaintDDIMXLCFGpp)


if __name__ == "__main__":
    print(f"inpaint solvers: {inpaint_solver_names()} for models {MODELS}")
