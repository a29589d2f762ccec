"""Image-to-image and latent hires fix: start a job from an existing image or latent instead of pure noise, for the DDIM, the
Karras-sigma (Euler, DPM++ 2M) and the SDE (DPM++ 2M / 3M SDE, DPM++ SDE) solvers, SD1.5 and SDXL, CFG and CFG++.

The feature is the START of the job.  ``x = a * resample(z) + s * n`` - the source latent z, upscaled when it is smaller than the
engine's latent, forward-noised to the first timestep / sigma the loop runs - is ONE launch (include/cfgpp_img2img.h:
cfgpp_img2img_start); the existing loops then run the tail of their schedule on it, and no step arithmetic changes.

Its own registry (like ``inpaint.py`` / ``sde.py``; the text-to-image registries and their refusals of ``src_img`` / ``strength``
stay): ``get_img2img_solver(name, model="sd15" | "sdxl", noise="torch" | "philox", **kwargs of the text-to-image getter)``.  Names:
``ddim``, ``ddim_cfg++``, ``euler``, ``euler_cfg++``, ``dpm++_2m``, ``dpm++_2m_cfg++`` (SD1.5; SDXL has no such text-to-image solver to
run), ``dpm++_2m_sde[_cfg++]``, ``dpm++_3m_sde[_cfg++]``, ``dpm++_sde[_cfg++]``.

``sample(<the text-to-image arguments>, src_img= | src_latents=, strength=0.75, upscale="bilinear", seeds=, return_latents=)``:
    src_img      [B or 1, 3, 8h, 8w] in [-1, 1]: encoded by the VAE; the posterior MEAN (nothing is drawn: a chain's source does not
                 depend on its neighbours' noise; the HIP encoder's own bits still vary with its batch size, 4e-4 absolute on the tiny
                 VAE), ``sample_posterior=True`` for the sampled posterior; rounded to the pipeline dtype like every encoded latent
    src_latents  [B or 1, 4, h0, w0], what ``return_latents=True`` hands back (a tuple's first entry), at the engine's latent size or
                 smaller; a smaller one is upscaled by ``upscale`` ("bilinear" | "bicubic" | "nearest-exact") inside the start launch

The strength rule is diffusers' ``get_timesteps`` for every family (``inpaint.strength_timesteps``): ``init = min(int(N * strength),
N)``, the loop runs the last ``init`` steps from index ``i0 = N - init``.  For ``i0 > 0``
    DDIM                         x = sqrt(a_t0) z + sqrt(1 - a_t0) n      fp32       (tables.ddim_sqrt_coeffs(ts[0], wrap))
    Euler / DPM++ 2M             x = z + sigma_i0 n                       fp16
    2M / 3M SDE, DPM++ SDE       x = z + sigma_i0 n                       fp32
and for ``i0 == 0`` (strength 1) the source is dropped, a = 0, and s is the family's own text-to-image start scale (1, sqrt(sigma_0^2
+ 1), sigma_0): with ``noise="torch"`` the job is the text-to-image job bit for bit.

``noise="torch"`` (default): ``_randn(seeds)`` on the host, as everywhere else.  ``noise="philox"``: the normals are drawn inside the
start launch (Philox stream 4, draw 0, keyed by the chains' seeds - ``_chain_seeds``' rule: a sharded run has to pass ``seeds=``).

ControlNet, LoRA, IP-Adapter, FreeU, long prompts, regions and v-models are loop or engine state: they compose wherever the
underlying solver takes them.  Refused by name: no source or both, a source larger than the engine's latent (downscaling is not
built), ``src_img`` of another size than 8h x 8w (pixel-space upscalers are not built), ``strength`` outside (0, 1] or one that leaves
no step, ``mask=`` / ``latents=``, and the ancestral, Lightning, inversion / edit, LCM, inpaint and panorama names.

``hires_fix(first, second, ...)``: an engine has one latent size, so hires fix is two solvers - ``first`` samples small, ``second``
(an img2img solver with a larger ``latent_hw``) denoises the upscaled latent again at partial strength.
"""
from __future__ import annotations

import math

import torch

from . import latent_diffusion as sd
from . import latent_sdxl as xl
from .dpmpp_sde import _DPMppSDESolverSD, _DPMppSDESolverXL
from .inpaint import strength_timesteps
from .latent_diffusion import controlled
from .registry import Registry
from .sde import _SDESolverSD, _SDESolverXL

__IMG2IMG_SOLVER__ = Registry("Img2ImgSolver")
MODELS = ("sd15", "sdxl")
UPSCALERS = ("bilinear", "bicubic", "nearest-exact")
NOISE_STREAM = 4            # stream id of the start's forward noise (include/cfgpp_img2img.h); 0 .. 3 are the step kernels'
DEFAULT_STRENGTH = 0.75


def register_img2img_solver(name: str, model: str):
    def add(cls):
        cls = __IMG2IMG_SOLVER__.register(f"{model}/{name}")(cls)
        cls.solver_name = name
        return cls
    return add


def _refused_name(name: str):
    """why a solver name of another registry has no img2img form, or None"""
    if name in ("euler_a", "euler_a_cfg++", "dpm++_2s_a", "dpm++_2s_a_cfg++"):
        return "img2img for the ancestral solvers is not built"
    if "lightning" in name:
        return "img2img for the Lightning solvers is not built"
    if "inversion" in name or "edit" in name:
        return "the inversion / edit solvers start from their own inverted latent (get_solver)"
    if name.startswith("lcm"):
        return "img2img for the LCM sampler is not built"
    if "inpaint" in name:
        return "the inpaint solvers are get_inpaint_solver's (their strength= is the masked form of this)"
    if "panorama" in name:
        return "img2img for the panorama solvers is not built"
    return None


def get_img2img_solver(name: str, model: str = "sd15", **kwargs):
    """``name``: one of ``img2img_solver_names(model)``; ``model`` in {"sd15", "sdxl"}; kwargs as the corresponding text-to-image
    getter's (``get_solver`` / ``get_sde_solver`` / ``get_dpmpp_sde_solver``) plus ``noise="torch" | "philox"``."""
    if model not in MODELS:
        raise ValueError(f"Img2ImgSolver model {model!r}: one of {MODELS}")
    try:
        cls = __IMG2IMG_SOLVER__[f"{model}/{name}"]
    except KeyError:
        why = _refused_name(str(name))
        if why is not None:
            raise ValueError(f"Img2ImgSolver {name}: {why}") from None
        if f"sd15/{name}" in __IMG2IMG_SOLVER__:
            raise ValueError(f"Img2ImgSolver {name}: model {model!r} has no text-to-image solver of that name to run") from None
        raise ValueError(f"Img2ImgSolver {name} does not exist.") from None
    return cls(**kwargs)


def img2img_solver_names(model: str = "sd15"):
    return sorted(k.split("/", 1)[1] for k in __IMG2IMG_SOLVER__ if k.startswith(model + "/"))


# ---------------------------------------------------------------------------------------------------- the start (shared)
class _Img2ImgMixin:
    """in front of an existing solver class: the source, the strength rule, the start launch.  The loops are the base class's."""

    def __init__(self, *args, **kwargs):
        noise = kwargs.pop("noise", None) or "torch"        # (the base classes' noise= is the ancestral solvers' per-step noise)
        if noise not in ("torch", "philox"):
            raise ValueError(f"{self._name()}: noise={noise!r}: 'torch' or 'philox'")
        self.start_noise = noise
        self.last_start = None              # what the last job's start launch was given (tests, measurements)
        super().__init__(*args, **kwargs)

    def _refuse_job(self, kwargs):
        """(replaces the SDE classes' refusal of src_img / strength)"""
        for k in ("mask", "latents"):
            if kwargs.get(k) is not None:
                raise ValueError(f"{self._name()}: {k}=... is not an img2img argument" +
                                 (" (masked jobs: get_inpaint_solver)" if k == "mask" else " (the start noise is drawn here: seeds=)"))

    def _source(self, B: int, kwargs, load: bool = True):
        """-> (source latent on the engine device [B or 1, C, h0, w0] fp16 / fp32, resample mode name); ``load=False`` (strength 1 drops
        the source): the refusals only, nothing is encoded or moved"""
        who = self._name()
        src_img, src_lat = kwargs.get("src_img"), kwargs.get("src_latents")
        if src_img is None and src_lat is None:
            raise ValueError(f"{who}: img2img needs a source: src_img=[B or 1, 3, 8h, 8w] or src_latents=[B or 1, C, h0, w0]")
        if src_img is not None and src_lat is not None:
            raise ValueError(f"{who}: pass src_img or src_latents, not both")
        upscale = kwargs.get("upscale") or "bilinear"
        if upscale not in UPSCALERS:
            raise ValueError(f"{who}: upscale={upscale!r}: one of {UPSCALERS}")
        h, w = self.latent_hw
        C = self.cfg.out_channels
        dev = self.work_device
        if src_img is not None:
            if not torch.is_tensor(src_img) or src_img.dim() != 4 or int(src_img.shape[1]) != 3 or int(src_img.shape[0]) not in (1, B):
                raise ValueError(f"{who}: src_img shape {tuple(getattr(src_img, 'shape', ()))}: expected [{B} or 1, 3, {8 * h}, {8 * w}]")
            if tuple(src_img.shape[2:]) != (8 * h, 8 * w):
                raise ValueError(f"{who}: src_img of {int(src_img.shape[2])} x {int(src_img.shape[3])} pixels for an engine of {8 * h} x "
                                 f"{8 * w}: pixel-space upscalers are not built (resize the image, or pass a smaller src_latents)")
            if not load:
                return None, "identity"
            vae = self._get_vae()
            if kwargs.get("sample_posterior"):
                z = vae.encode(src_img.float().to(dev))
            else:                           # the posterior mean: nothing is drawn
                z = vae.encode(src_img.float().to(dev), sample=False)
            return z.to(dev, self.dtype).contiguous(), "identity"
        if isinstance(src_lat, (tuple, list)):          # what return_latents=True hands back: (denoised, x)
            src_lat = src_lat[0]
        if not torch.is_tensor(src_lat) or src_lat.dim() != 4 or int(src_lat.shape[1]) != C or int(src_lat.shape[0]) not in (1, B):
            raise ValueError(f"{who}: src_latents shape {tuple(getattr(src_lat, 'shape', ()))}: expected [{B} or 1, {C}, h0 <= {h}, w0 <= {w}]")
        h0, w0 = int(src_lat.shape[2]), int(src_lat.shape[3])
        if h0 > h or w0 > w:
            raise ValueError(f"{who}: src_latents of {h0} x {w0} is larger than the engine's latent {h} x {w}: downscaling is not built")
        if not load:
            return None, "identity"
        dt = src_lat.dtype if src_lat.dtype in (torch.float16, torch.float32) else torch.float32
        return src_lat.detach().to(dev, dt).contiguous(), ("identity" if (h0, w0) == (h, w) else upscale)

    def _strength_index(self, kwargs) -> int:
        """diffusers' get_timesteps on this solver's N steps -> i0, the index of the first step that runs"""
        strength = kwargs.get("strength")
        strength = DEFAULT_STRENGTH if strength is None else float(strength)
        if not (math.isfinite(strength) and 0.0 < strength <= 1.0):
            raise ValueError(f"{self._name()}: strength={strength}: a number in (0, 1]")
        try:
            return int(strength_timesteps(self.scheduler.timesteps, strength)[1])
        except ValueError as e:
            raise ValueError(f"{self._name()}: {e}") from None

    def _start_latent(self, B: int, kwargs, i0: int, coeffs, dtype):
        """the start launch.  ``coeffs``: (a, s) of this family at ``i0``.  -> (x [B, C, h, w] of ``dtype`` on the engine device, the
        seeds the loop's own noise is keyed by: the caller's, or with noise="philox" the ones drawn here)"""
        eng = self.engine
        if not hasattr(eng, "img2img_start"):
            raise ValueError(f"{self._name()}: the engine {type(eng).__name__} has no img2img_start")
        a, s = (float(v) for v in coeffs)
        src, mode = self._source(B, kwargs, load=a != 0.0)          # (the refusals also when strength 1 drops the source)
        size = (B, self.cfg.out_channels) + tuple(self.latent_hw)
        x = torch.empty(size, dtype=dtype, device=self.work_device)
        seeds = kwargs.get("seeds")
        if self.start_noise == "philox":
            seeds = self._chain_seeds(seeds, B, f"{self._name()} with noise='philox'")
            eng.img2img_start(x, src, a, s, mode, seeds=seeds)
        else:
            noise = self._randn(size, seeds).to(self.work_device, torch.float32).contiguous()
            eng.img2img_start(x, src, a, s, mode, noise=noise)
        self.last_start = dict(i0=int(i0), steps=len(self.scheduler.timesteps) - int(i0), a=a, s=s, mode=mode, noise=self.start_noise)
        return x, seeds

    # -- the three families ------------------------------------------------------------------------------------------------
    def _ddim_start(self, B: int, kwargs, wrap: bool):
        """-> (zt fp32, the timesteps the loop runs)"""
        self._refuse_job(kwargs)
        i0 = self._strength_index(kwargs)
        ts = self.scheduler.timesteps[i0:]
        if i0 > 0:
            c1, c2 = self.tables.ddim_sqrt_coeffs(ts[0], wrap=wrap)[:2]      # sqrt(1 - a_t0), sqrt(a_t0)
            coeffs = (c2, c1)
        else:
            coeffs = (0.0, 1.0)
        zt, _ = self._start_latent(B, kwargs, i0, coeffs, torch.float32)
        return zt, ts

    def _sigma_start(self, B: int, kwargs, sigmas, dtype, full_scale: float):
        """-> (x of ``dtype``, i0, seeds); ``full_scale``: the family's text-to-image start scale, used when no step is skipped"""
        self._refuse_job(kwargs)
        i0 = self._strength_index(kwargs)
        coeffs = (1.0, float(sigmas[i0])) if i0 > 0 else (0.0, float(full_scale))
        x, seeds = self._start_latent(B, kwargs, i0, coeffs, dtype)
        return x, i0, seeds

    @staticmethod
    def _kdiff_full_scale(sigmas) -> float:
        """sqrt(sigma_0^2 + 1) as ``initialize_latent("random_kdiffusion")`` forms it: fp32 tensor arithmetic"""
        return float(((sigmas[0].to(torch.float32) ** 2 + 1) ** 0.5))


class _XLPrompts:
    """SDXL: a single ``prompt=[null, text]`` is taken for both towers, and the size conditioning defaults to the engine's size (as
    ``inpaint.InpaintDDIMXL``); ``SDXL.sample`` does the rest"""

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


# ---------------------------------------------------------------------------------------------------- DDIM
class _DDIMImg2Img(_Img2ImgMixin, sd.BaseDDIM):
    @torch.no_grad()
    @controlled
    def sample(self, cfg_guidance=7.5, prompt=["", ""], callback_fn=None, **kwargs):
        uc, c = self._embeds(prompt, kwargs)
        zt, ts = self._ddim_start(int(c.shape[0]), kwargs, wrap=False)
        z0t, zt = self._ddim_loop(zt, uc, c, cfg_guidance, False, self.cfgpp, ts=ts, callback_fn=callback_fn, desc="SD-img2img",
                                  update=self._update_hook())
        return self._result(kwargs.get("return_latents"), (z0t, zt), z0t)


class _DDIMImg2ImgXL(_XLPrompts, _Img2ImgMixin, xl.BaseDDIM):
    def reverse_process(self, null_prompt_embeds, prompt_embeds, cfg_guidance, add_cond_kwargs, shape=(1024, 1024), callback_fn=None,
                        **kwargs):
        zt, ts = self._ddim_start(int(prompt_embeds.shape[0]), kwargs, wrap=True)
        return self._ddim_loop(zt, null_prompt_embeds, prompt_embeds, cfg_guidance, False, self.cfgpp, wrap=True, added=add_cond_kwargs,
                               ts=ts, callback_fn=callback_fn, desc="SDXL-img2img", update=self._update_hook())[0]


# ---------------------------------------------------------------------------------------------------- Euler / DPM++ 2M (fp16 latent)
class _KdiffImg2Img(_Img2ImgMixin, sd.EulerCFGSolver):
    @torch.no_grad()
    @controlled
    def sample(self, cfg_guidance=7.5, prompt=["", ""], callback_fn=None, **kwargs):
        uc, c = self._embeds(prompt, kwargs)
        sigmas = self.tables.karras_sigmas()
        x, i0, _ = self._sigma_start(int(c.shape[0]), kwargs, sigmas, torch.float16, self._kdiff_full_scale(sigmas))
        den, x = self._kdiff_loop(x, sigmas[i0:], uc, c, cfg_guidance, self.variant, self.solver, callback_fn,
                                  n_steps=len(self.scheduler.timesteps) - i0, desc="SD-img2img")
        return self._result(kwargs.get("return_latents"), (den, x), den if self.solver == "euler" else x)


class _EulerImg2ImgXL(_XLPrompts, _Img2ImgMixin, xl.Euler):
    def _xl_sigmas(self):
        return self.tables.karras_sigmas()

    def reverse_process(self, null_prompt_embeds, prompt_embeds, cfg_guidance, add_cond_kwargs, shape=(1024, 1024), callback_fn=None,
                        **kwargs):
        sigmas = self._xl_sigmas()
        x, i0, _ = self._sigma_start(int(prompt_embeds.shape[0]), kwargs, sigmas, torch.float16, self._kdiff_full_scale(sigmas))
        return self._kdiff_loop(x, sigmas[i0:], null_prompt_embeds, prompt_embeds, cfg_guidance, self.variant, "euler", callback_fn,
                                added=add_cond_kwargs, n_steps=len(self.scheduler.timesteps) - i0, desc="SDXL-img2img")[0]


class _EulerCFGppImg2ImgXL(_EulerImg2ImgXL):
    """SDXL's `euler_cfg++` runs on the DDIM-timestep sigmas (latent_sdxl.EulerCFGpp)"""
    variant = 1

    def _xl_sigmas(self):
        total_sigmas = (1 - self.total_alphas).sqrt() / self.total_alphas.sqrt()
        sigmas = total_sigmas[torch.round(self.scheduler.timesteps.float()).int()]
        return torch.cat([sigmas, torch.tensor([0.0])])


# ---------------------------------------------------------------------------------------------------- the SDE solvers (fp32 latent)
class _SDEImg2ImgSD:
    """``sample`` of the SD1.5 SDE classes with the img2img start (2M / 3M SDE and DPM++ SDE: the loop is the class's own)"""

    @torch.no_grad()
    @controlled
    def sample(self, cfg_guidance=7.5, prompt=["", ""], callback_fn=None, **kwargs):
        uc, c = self._embeds(prompt, kwargs)
        B = int(c.shape[0])
        sigmas = self.sde_sigmas()
        x, i0, seeds = self._sigma_start(B, kwargs, sigmas, torch.float32, float(sigmas[0]))
        seeds = self._chain_seeds(seeds, B, self._name())
        den, x = self._sde_loop(x, sigmas[i0:], uc, c, float(cfg_guidance), seeds, callback_fn=callback_fn)
        return self._result(kwargs.get("return_latents"), (den, x), den)


class _SDEImg2ImgXL(_XLPrompts):
    def reverse_process(self, null_prompt_embeds, prompt_embeds, cfg_guidance, add_cond_kwargs, shape=(1024, 1024), callback_fn=None,
                        **kwargs):
        B = int(prompt_embeds.shape[0])
        sigmas = self.sde_sigmas()
        x, i0, seeds = self._sigma_start(B, kwargs, sigmas, torch.float32, float(sigmas[0]))
        seeds = self._chain_seeds(seeds, B, self._name())
        return self._sde_loop(x, sigmas[i0:], null_prompt_embeds, prompt_embeds, float(cfg_guidance), seeds, added=add_cond_kwargs,
                              callback_fn=callback_fn, desc="SDXL SDE img2img")


# ---------------------------------------------------------------------------------------------------- the registry
def _make(name, model, bases, **attrs):
    cls = type(f"Img2Img_{model}_{name}".replace("+", "p").replace("-", "_"), bases, dict(attrs, __doc__=f"img2img `{name}` ({model})",
                                                                                         __module__=__name__))
    return register_img2img_solver(name, model)(cls)


for _cfgpp in (False, True):
    _s = "_cfg++" if _cfgpp else ""
    _make("ddim" + _s, "sd15", (_DDIMImg2Img,), cfgpp=_cfgpp)
    _make("ddim" + _s, "sdxl", (_DDIMImg2ImgXL,), cfgpp=_cfgpp)
    _make("euler" + _s, "sd15", (_KdiffImg2Img,), variant=int(_cfgpp), solver="euler")
    _make("dpm++_2m" + _s, "sd15", (_KdiffImg2Img,), variant=int(_cfgpp), solver="dpm2m")
    _make("euler" + _s, "sdxl", (_EulerCFGppImg2ImgXL if _cfgpp else _EulerImg2ImgXL,))
    for _kind in ("2m", "3m"):
        _make(f"dpm++_{_kind}_sde" + _s, "sd15", (_SDEImg2ImgSD, _Img2ImgMixin, _SDESolverSD), kind=_kind, cfgpp=_cfgpp)
        _make(f"dpm++_{_kind}_sde" + _s, "sdxl", (_SDEImg2ImgXL, _Img2ImgMixin, _SDESolverXL), kind=_kind, cfgpp=_cfgpp)
    _make("dpm++_sde" + _s, "sd15", (_SDEImg2ImgSD, _Img2ImgMixin, _DPMppSDESolverSD), cfgpp=_cfgpp)
    _make("dpm++_sde" + _s, "sdxl", (_SDEImg2ImgXL, _Img2ImgMixin, _DPMppSDESolverXL), cfgpp=_cfgpp)


# ---------------------------------------------------------------------------------------------------- hires fix
def hires_fix(first, second, cfg_guidance, prompt, *, strength: float = 0.5, upscale: str = "bilinear", seeds=None, first_kw=None,
              second_kw=None, **kw):
    """latent hires fix with two solvers: ``first`` (any text-to-image solver; its ``latent_hw`` is the small size) samples, its
    denoised latent goes to ``second`` (an img2img solver with a larger ``latent_hw``), which upscales it inside its start launch and
    denoises again at ``strength``.  ``prompt=[null, text]`` goes to both (both towers of an SDXL solver); ``kw`` goes to both
    ``sample`` calls, ``first_kw`` / ``second_kw`` to one.  -> what ``second.sample`` returns (``return_latents=`` in ``second_kw``)."""
    if not isinstance(second, _Img2ImgMixin):
        raise ValueError(f"hires_fix: second must be an img2img solver (get_img2img_solver), got {type(second).__name__}")

    def prompts(solver):
        if "prompt_embeds" in kw:
            return {}
        if isinstance(solver, xl.SDXL) and not isinstance(solver, _XLPrompts):
            return dict(prompt1=prompt, prompt2=prompt)
        return dict(prompt=prompt)
    lat = first.sample(cfg_guidance=cfg_guidance, seeds=seeds, return_latents=True, **prompts(first), **kw, **(first_kw or {}))
    z = lat[0] if isinstance(lat, (tuple, list)) else lat
    return second.sample(cfg_guidance=cfg_guidance, src_latents=z, strength=strength, upscale=upscale, seeds=seeds, **prompts(second),
                         **kw, **(second_kw or {}))


if __name__ == "__main__":
    print(f"img2img solvers: sd15 {img2img_solver_names('sd15')}; sdxl {img2img_solver_names('sdxl')}")
