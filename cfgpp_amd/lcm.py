"""Latent-consistency (LCM) sampling: the few-step sampler of the LCM checkpoints (guidance-embedded UNets: ``time_cond_proj_dim``)
and of LCM-LoRA adapters on a plain UNet.  The arithmetic is diffusers' ``LCMScheduler`` / ``LatentConsistencyModelPipeline``
written out; the per-step update is ONE fused launch (include/cfgpp_lcm.h: cfgpp_step_lcm) that draws its renoising noise from a
counter-based generator inside the kernel, keyed by the chain's seed - no launch and no memory traffic of its own, and chain b of a
batch reproduces chain b run alone.

Its own registry (like ``inpaint.py``): the two reference registries mirror the reference's name lists, and the reference has no
LCM.  ``get_lcm_solver("lcm", model="sd15" | "sdxl", **get_solver kwargs)``.

The step at timestep t (next timestep t_prev), model output m (epsilon or v), boundary scalings c_skip / c_out:
    x0  = (z - sqrt(1 - a_t) m) / sqrt(a_t)          (epsilon)       x0 = sqrt(a_t) z - sqrt(1 - a_t) m      (v)
    den = c_out x0 + c_skip z
    z   = sqrt(a_prev) den + sqrt(1 - a_prev) noise                  the last step: z = den
with a_t = abar[t] (diffusers' indexing: no shifted table) from the pinned tables.

Guidance.  An engine with ``time_cond_proj_dim`` runs one conditioning per step - both halves of the engine's batch carry the
positive prompt, as ``predict_noise(uc=None)`` always did - and the guidance scale w goes into the UNet through its embedding
(default 8.5).  Otherwise (an LCM-LoRA on a plain UNet) ``cfg_guidance > 1`` is ordinary CFG on the model output and ``cfg_guidance
<= 1`` the single conditioning.  There is no ``lcm_cfg++``: CFG++ renoises with eps_uc, and this step renoises with FRESH noise, so
there is no eps_uc renoising to define it by.

Refused by name: zero_terminal_snr, inversion / edit / inpaint (``src_img`` / ``mask``), more steps than ``original_inference_steps``,
a sharded run without per-rank ``seeds=``.  Graph replay is never used: the eager loop runs, also under CFGPP_GRAPH=1.
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch

from . import coeffs as K
from .latent_diffusion import StableDiffusion, _progress, controlled
from .latent_sdxl import SDXL
from .registry import Registry

__LCM_SOLVER__ = Registry("LCMSolver")
MODELS = ("sd15", "sdxl")
NUM_TRAIN_TIMESTEPS = 1000
SIGMA_DATA = 0.5
DEFAULT_GUIDANCE_SCALE = 8.5


def register_lcm_solver(name: str, model: str):
    return __LCM_SOLVER__.register(f"{model}/{name}")


def get_lcm_solver(name: str = "lcm", model: str = "sd15", **kwargs):
    """``name``: "lcm"; ``model`` in {"sd15", "sdxl"}; kwargs as ``get_solver``'s plus ``lcm_original_steps`` (50), ``timestep_scaling``
    (10.0) and ``guidance_scale`` (8.5, guidance-embedded UNets).  ``unet_config=SD15_LCM`` / ``SDXL_LCM`` (or a checkpoint directory's
    ``solver_kwargs_from_dir``) selects the guidance-embedded kind."""
    if model not in MODELS:
        raise ValueError(f"LCMSolver model {model!r}: one of {MODELS}")
    try:
        cls = __LCM_SOLVER__[f"{model}/{name}"]
    except KeyError:
        raise ValueError(f"LCMSolver {name} does not exist.") from None
    return cls(**kwargs)


def lcm_solver_names():
    return sorted({k.split("/", 1)[1] for k in __LCM_SOLVER__})


# ---------------------------------------------------------------------------------------------------- schedule (host)
def lcm_timesteps(num_steps: int, original_steps: int = 50) -> List[int]:
    """LCMScheduler.set_timesteps: the ``original_steps`` training-schedule timesteps, reversed, picked at
    floor(linspace(0, original_steps, num_steps, endpoint=False)).  4 steps: 999, 759, 499, 259."""
    n, o = int(num_steps), int(original_steps)
    if not 1 <= o <= NUM_TRAIN_TIMESTEPS:
        raise ValueError(f"lcm_original_steps={o}: 1 .. {NUM_TRAIN_TIMESTEPS}")
    if not 1 <= n <= o:
        raise ValueError(f"solver 'lcm': {n} sampling steps with original_inference_steps={o} (1 .. {o}: the LCM schedule picks its "
                         "timesteps among the original ones)")
    origin = (np.arange(1, o + 1) * (NUM_TRAIN_TIMESTEPS // o) - 1)[::-1]
    idx = np.floor(np.linspace(0, o, n, endpoint=False)).astype(np.int64)
    return [int(t) for t in origin[idx]]


def boundary_scalings(t, timestep_scaling: float = 10.0):
    """(c_skip, c_out) of the consistency parameterisation at timestep t, float64 arithmetic, each rounded once to fp32:
    s = timestep_scaling * t, c_skip = sd^2 / (s^2 + sd^2), c_out = s / sqrt(s^2 + sd^2), sd = 0.5"""
    s = float(timestep_scaling) * float(t)
    c_skip = SIGMA_DATA ** 2 / (s ** 2 + SIGMA_DATA ** 2)
    c_out = s / math.sqrt(s ** 2 + SIGMA_DATA ** 2)
    return float(np.float32(c_skip)), float(np.float32(c_out))


def guidance_scale_embedding(guidance_scale: float, dim: int) -> List[float]:
    """diffusers ``get_guidance_scale_embedding``: w = (guidance_scale - 1) * 1000, f_i = exp(-i ln(10000) / (dim/2 - 1)),
    [sin(w f), cos(w f)]; float64 arithmetic, rounded once to fp32.  ``dim`` even, >= 4."""
    dim = int(dim)
    if dim < 4 or dim % 2:
        raise ValueError(f"guidance_scale_embedding: dim={dim} (an even number >= 4)")
    w = (float(guidance_scale) - 1.0) * 1000.0
    half = dim // 2
    f = np.exp(-np.arange(half, dtype=np.float64) * math.log(10000.0) / (half - 1))
    return [float(v) for v in np.concatenate([np.sin(w * f), np.cos(w * f)]).astype(np.float32)]


def step_coeffs(tables, t: int, t_prev: Optional[int], pred_v: bool, semantics: str, timestep_scaling: float = 10.0):
    """coef6 of cfgpp_step_lcm for the step at ``t`` whose next timestep is ``t_prev`` (None: the last step, c3 = 1, c4 = 0 - the
    kernel's ``last`` flag applies and reads neither).  sqrt(a) / sqrt(1 - a) come from the pinned tables; which of them is
    pre-rounded to fp16 follows ``coeffs.ddim_coeffs_pinned`` (c1, the divisor c2) and ``ddim_v_coeffs_pinned`` (s_v, a_z); c3 / c4
    multiply fp32 values (den, the noise) and stay fp32."""
    i_t = int(t) + 1                                    # abar[k] is entry k + 1 of the shifted tables
    sq_a, sq_1ma = tables._sqrt_a, tables._sqrt_1ma
    if t_prev is None:
        c3, c4 = 1.0, 0.0
    else:
        c3, c4 = float(sq_a[int(t_prev) + 1]), float(sq_1ma[int(t_prev) + 1])
    sqrt4 = (float(sq_1ma[i_t]), float(sq_a[i_t]), c3, c4)
    c_skip, c_out = boundary_scalings(t, timestep_scaling)
    if pred_v:
        cv = K.ddim_v_coeffs_pinned(sqrt4, semantics=semantics, z_half=False)
        return (cv[1], cv[0], c_out, c_skip, c3, c4)    # (s_v, a_z, ..)
    co = K.ddim_coeffs_pinned(sqrt4, eps_half=True, semantics=semantics, z_half=False)
    return (co[0], co[1], c_out, c_skip, c3, c4)        # (c1, c2, ..)


# ---------------------------------------------------------------------------------------------------- the solvers
class _LCMMixin:
    """shared by the SD1.5 and SDXL classes: the schedule, the job's seeds and guidance, the loop"""

    def _lcm_init(self, solver_config, kwargs):
        if kwargs.get("zero_terminal_snr"):
            raise ValueError("solver 'lcm': zero_terminal_snr=True is not supported (LCM checkpoints are distilled on the plain schedule)")
        self.lcm_original_steps = int(kwargs.get("lcm_original_steps") or 50)
        self.timestep_scaling = float(kwargs.get("timestep_scaling") or 10.0)
        self.guidance_scale = float(kwargs.get("guidance_scale") or DEFAULT_GUIDANCE_SCALE)
        self.lcm_ts = lcm_timesteps(solver_config.num_sampling, self.lcm_original_steps)       # refuses N > O before anything is built

    @property
    def guidance_embedded(self) -> bool:
        return int(getattr(self.engine, "time_cond_proj_dim", 0) or 0) > 0

    def _refuse_job(self, kwargs):
        for k in ("src_img", "mask", "strength"):
            if kwargs.get(k) is not None:
                raise ValueError(f"solver 'lcm': {k}=... - inversion, edit and inpaint jobs are not supported by the LCM sampler")

    def inversion(self, *args, **kwargs):
        raise ValueError("solver 'lcm': inversion is not supported (the consistency step is not an invertible DDIM update)")

    def _job_seeds(self, seeds, B: int) -> List[int]:
        """the chains' 64-bit seeds: the caller's (they also made the start latent), else B values from torch's CPU generator"""
        return self._chain_seeds(seeds, B, "solver 'lcm'")

    def _job_guidance(self, cfg_guidance, guidance_scale=None):
        """-> (single conditioning?, lam of the step's guidance mix, guidance scale embedded into the UNet or None)"""
        if self.guidance_embedded:
            w = guidance_scale if guidance_scale is not None else (cfg_guidance if cfg_guidance is not None else self.guidance_scale)
            return True, 1.0, float(w)
        g = 1.0 if cfg_guidance is None else float(cfg_guidance)
        return (g <= 1.0), (1.0 if g <= 1.0 else g), None

    def _lcm_loop(self, zt, uc, c, lam: float, single: bool, w_embed, seeds, *, added=None, callback_fn=None, desc="LCM"):
        """THE LCM loop: per step one UNet call and one cfgpp_step_lcm launch.  Returns (denoised, zt)."""
        zt = self._own_latent(zt.to(torch.float32))
        if w_embed is not None:
            self.engine.set_guidance_embedding(guidance_scale_embedding(w_embed, self.engine.time_cond_proj_dim))
        if single:
            uc = None
        pred_v = self.prediction_type == "v_prediction"
        den = torch.empty_like(zt)
        ts = self.lcm_ts
        n = len(ts)
        for i, t in enumerate(_progress(ts, desc)):
            last = i == n - 1
            coef = step_coeffs(self.tables, t, None if last else ts[i + 1], pred_v, self.scalar_semantics, self.timestep_scaling)
            m_uc, m_c = self._predict(zt, t, uc, c, added)
            self.engine.step_lcm(zt, den, m_uc, m_c, lam, coef, pred_v, last, seeds=seeds, draw=i)
            if callback_fn is not None:
                self._run_callback(callback_fn, i, t, den, zt)
        return den, zt


@register_lcm_solver("lcm", "sd15")
class LCMSolver(_LCMMixin, StableDiffusion):
    """SD1.5 family: ``sample(cfg_guidance=None, prompt=[null, text], seeds=[...], guidance_scale=None, return_latents=False)``"""

    def __init__(self, solver_config, **kwargs):
        self._lcm_init(solver_config, kwargs)
        StableDiffusion.__init__(self, solver_config, **kwargs)

    @torch.no_grad()
    @controlled
    def sample(self, cfg_guidance=None, prompt=["", ""], callback_fn=None, **kwargs):
        self._refuse_job(kwargs)
        single, lam, w = self._job_guidance(cfg_guidance, kwargs.get("guidance_scale"))
        uc, c = self._embeds(prompt, kwargs)
        B = int(c.shape[0])
        zt = kwargs.get("latents")
        if zt is None:
            zt = self.initialize_latent(latent_dim=(B, self.cfg.out_channels) + self.latent_hw, seeds=kwargs.get("seeds"))
        seeds = self._job_seeds(kwargs.get("seeds"), B)
        den, zt = self._lcm_loop(zt.to(self.work_device), uc, c, lam, single, w, seeds, callback_fn=callback_fn)
        return self._result(kwargs.get("return_latents"), (den, zt), den)


@register_lcm_solver("lcm", "sdxl")
class LCMSolverXL(_LCMMixin, SDXL):
    """SDXL family: ``SDXL.sample``'s arguments (prompt1 / prompt2 or prompt_embeds, size conditioning) plus ``seeds``,
    ``guidance_scale``, ``return_latents``"""

    def __init__(self, solver_config, **kwargs):
        self._lcm_init(solver_config, kwargs)
        SDXL.__init__(self, solver_config, **kwargs)

    @torch.no_grad()
    def sample(self, prompt1=["", ""], prompt2=["", ""], cfg_guidance=None, **kwargs):
        self._refuse_job(kwargs)
        ret_lat = kwargs.pop("return_latents", False)
        single, lam, w = self._job_guidance(cfg_guidance, kwargs.pop("guidance_scale", None))
        self._lcm_job = (single, lam, w)
        # SDXL.sample assembles the added conditions for both halves only when it is asked for CFG: 1.0 = the positive rows alone
        den, zt = SDXL.sample(self, prompt1, prompt2, 1.0 if single else lam, return_latents=True, **kwargs)
        return (den, zt) if ret_lat else self._finish(den)

    def reverse_process(self, null_prompt_embeds, prompt_embeds, cfg_guidance, add_cond_kwargs, shape=(1024, 1024), callback_fn=None,
                        **kwargs):
        single, lam, w = self._lcm_job
        zt = kwargs.get("latents")
        if zt is None:
            zt = self.initialize_latent(size=self._latent_size(shape), seeds=kwargs.get("seeds"))
        seeds = self._job_seeds(kwargs.get("seeds"), int(zt.shape[0]))
        return self._lcm_loop(zt.to(self.work_device), null_prompt_embeds, prompt_embeds, lam, single, w, seeds, added=add_cond_kwargs,
                              callback_fn=callback_fn, desc="SDXL LCM")
