"""DPM-Solver++ 2M / 3M SDE sampling (k-diffusion's ``sample_dpmpp_2m_sde`` / ``sample_dpmpp_3m_sde``: "DPM++ 2M SDE Karras", "DPM++ 3M
SDE Exponential") with CFG and with CFG++.  The reference has neither, so there is no fp16 torch arithmetic to mirror: the latent is
fp32 and the per-step update is ONE fused launch (include/cfgpp_sde.h: cfgpp_step_sde) - guidance mix, denoised estimates, the
multistep combination, the noise drawn in registers from the seeded counter-based generator, the history write and the next step's
fp16 UNet input.

Its own registry (like ``lcm.py``): the two reference registries mirror the reference's name lists.
``get_sde_solver(name, model="sd15" | "sdxl", eta=1.0, s_noise=1.0, solver_type="midpoint" | "heun", sigma_schedule="karras" |
"exponential", **get_solver kwargs)``; names: ``dpm++_2m_sde``, ``dpm++_2m_sde_cfg++``, ``dpm++_3m_sde``, ``dpm++_3m_sde_cfg++``.

The update.  With t = -ln sigma_i, s = -ln sigma_{i+1}, h = s - t, h_eta = h (1 + eta), c = exp(-h_eta) and D, D1, D2 the current and
the two previous denoised values:
    both:            x <- c x + (1 - c) D
    2m, history 1:   + 0.5 (1 - c) / r (D - D1)  (midpoint)     + (1 - (1 - c) / h_eta) / r (D - D1)  (heun)        r = h_last / h
    3m, history 1:   + phi2 / r (D - D1)                                                  phi2 = expm1(-h_eta) / h_eta + 1
    3m, history 2:   + phi2 d1 - phi3 d2,  d10 = (D - D1) / r0, d11 = (D1 - D2) / r1, d1 = d10 + (d10 - d11) r0 / (r0 + r1),
                     d2 = (d10 - d11) / (r0 + r1), phi3 = phi2 / h_eta - 0.5, r0 = h_1 / h, r1 = h_2 / h
    noise:           + sigma_{i+1} sqrt(1 - exp(-2 eta h)) s_noise n,   n standard normal;     sigma_{i+1} = 0:  x <- D
All of it is linear: x' = a_x x + a_0 D + a_1 D1 + a_2 D2 + a_n n, and ``sde_coeffs`` makes the row.

CFG++ (the rule the reference uses everywhere: estimate x0 with the guided eps_hat, renoise with eps_uc).  The only place the current
noise enters is a_x x = a_x (den + sigma eps_hat); it becomes a_x (den + sigma eps_uc) = a_x (x - uden + den).  Hence a_d = a_0 + a_x,
a_u = -a_x, and the history holds uden: the current term is den, every history term uden - what the SD1.5 ``dpm++_2m_cfg++`` does.
``dpm++_2m_sde_cfg++`` with eta = 0, midpoint, is that solver in exact arithmetic.

Noise.  The intervals of successive steps do not overlap, so independent standard normals per step have exactly the law of
k-diffusion's Brownian-tree increments; they are keyed by the chains' seeds (stream id 2, draw = step index), so chain b of a batch
reproduces chain b run alone.  ``eta=0`` is a deterministic fp32 DPM++ 2M / 3M.  The two-stage ``dpm++_sde``, whose two noise terms
per step DO overlap, is ``dpmpp_sde.py`` (its own registry; this one keeps refusing the name).

Refused by name: zero_terminal_snr, guidance_rescale, inversion / edit / inpaint (``src_img`` / ``mask`` / ``strength``),
``solver_type`` on 3M, a negative or non-finite ``eta`` / ``s_noise``, a sharded run without per-rank ``seeds=``.  Graph replay is
never used: the eager loop runs, also under CFGPP_GRAPH=1.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .latent_diffusion import StableDiffusion, _progress, controlled
from .latent_sdxl import SDXL
from .registry import Registry

__SDE_SOLVER__ = Registry("SDESolver")
MODELS = ("sd15", "sdxl")
SOLVER_TYPES = ("midpoint", "heun")
SIGMA_SCHEDULES = ("karras", "exponential")
NOISE_STREAM = 2            # stream id of the step noise (include/cfgpp_sde.h); 0 and 1 are the LCM renoise and the ancestral noise


def register_sde_solver(name: str, model: str):
    def add(cls):
        cls = __SDE_SOLVER__.register(f"{model}/{name}")(cls)
        cls.solver_name = name
        return cls
    return add


def get_sde_solver(name: str, model: str = "sd15", **kwargs):
    """``name``: one of ``sde_solver_names()``; ``model`` in {"sd15", "sdxl"}; kwargs as ``get_solver``'s plus ``eta`` (1.0),
    ``s_noise`` (1.0), ``solver_type`` ("midpoint" | "heun", 2M only) and ``sigma_schedule`` ("karras" | "exponential")."""
    if model not in MODELS:
        raise ValueError(f"SDESolver model {model!r}: one of {MODELS}")
    try:
        cls = __SDE_SOLVER__[f"{model}/{name}"]
    except KeyError:
        raise ValueError(f"SDESolver {name} does not exist.") from None
    return cls(**kwargs)


def sde_solver_names():
    return sorted({k.split("/", 1)[1] for k in __SDE_SOLVER__})


# ---------------------------------------------------------------------------------------------------- coefficients (host)
def sde_coeffs(sigmas, i: int, kind: str = "2m", solver_type: str = "midpoint", eta: float = 1.0, s_noise: float = 1.0,
               cfgpp: bool = False, n_hist: int = 0):
    """coef8 of cfgpp_step_sde for step ``i`` of ``sigmas`` (fp32 table with the trailing zero): (sigma, a_x, a_d, a_u, a_1, a_2, a_n,
    s_in_next).  ``n_hist``: how many history values the step uses (at most 1 for "2m", 2 for "3m", and never more than ``i``).
    Python float64 from the fp32 sigmas (``sde_coeffs64``), each entry rounded once to fp32; the step whose next sigma is 0 is the
    kernel's ``last`` (x <- D) and gets zeros.  Independent of ``scalar_semantics``: there is no reference torch arithmetic to imitate."""
    return tuple(float(np.float32(v)) for v in sde_coeffs64(sigmas, i, kind, solver_type, eta, s_noise, cfgpp, n_hist))


def sde_coeffs64(sigmas, i: int, kind: str = "2m", solver_type: str = "midpoint", eta: float = 1.0, s_noise: float = 1.0,
                 cfgpp: bool = False, n_hist: int = 0):
    """``sde_coeffs`` before the rounding to fp32"""
    if kind not in ("2m", "3m"):
        raise ValueError(f"sde_coeffs: kind={kind!r}: '2m' or '3m'")
    if solver_type not in SOLVER_TYPES:
        raise ValueError(f"sde_coeffs: solver_type={solver_type!r}: one of {SOLVER_TYPES}")
    if not 0 <= n_hist <= min(i, 1 if kind == "2m" else 2):
        raise ValueError(f"sde_coeffs: n_hist={n_hist} at step {i} of a {kind} solver")
    sig, sig_n = float(sigmas[i]), float(sigmas[i + 1])
    if sig_n == 0.0:
        return (sig, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    t_of = lambda v: -math.log(float(v))  # noqa: E731
    h = t_of(sig_n) - t_of(sig)
    h_eta = h * (1.0 + eta)
    a_x = math.exp(-h_eta)
    one_c = -math.expm1(-h_eta)                          # 1 - c
    a_0, a_1, a_2 = one_c, 0.0, 0.0
    if n_hist >= 1:
        r0 = (t_of(sig) - t_of(sigmas[i - 1])) / h
        phi2 = math.expm1(-h_eta) / h_eta + 1.0
        if kind == "2m":
            k = 0.5 * one_c / r0 if solver_type == "midpoint" else (1.0 - one_c / h_eta) / r0
            a_0, a_1 = a_0 + k, -k
        elif n_hist == 1:
            k = phi2 / r0
            a_0, a_1 = a_0 + k, -k
        else:
            r1 = (t_of(sigmas[i - 1]) - t_of(sigmas[i - 2])) / h
            phi3 = phi2 / h_eta - 0.5
            R, S = r0 / (r0 + r1), 1.0 / (r0 + r1)
            p = phi2 * (1.0 + R) - phi3 * S              # weight of d10 = (D - D1) / r0
            q = -phi2 * R + phi3 * S                     # weight of d11 = (D1 - D2) / r1
            a_0, a_1, a_2 = a_0 + p / r0, -p / r0 + q / r1, -q / r1
    a_n = sig_n * math.sqrt(-math.expm1(-2.0 * eta * h)) * s_noise if eta > 0.0 else 0.0
    a_d, a_u = (a_0 + a_x, -a_x) if cfgpp else (a_0, 0.0)
    return (sig, a_x, a_d, a_u, a_1, a_2, a_n, 1.0 / math.sqrt(sig_n * sig_n + 1.0))


def input_scale(sigma) -> float:
    """1 / sqrt(sigma^2 + 1) of the UNet input, float64 rounded once to fp32 (what ``sde_coeffs`` puts into s_in_next)"""
    s = float(sigma)
    return float(np.float32(1.0 / math.sqrt(s * s + 1.0)))


# ---------------------------------------------------------------------------------------------------- the solvers
class _SDEMixin:
    """shared by the SD1.5 and SDXL classes: the options, the schedule, the loop"""
    kind, cfgpp = "2m", False
    sigma_solver = True

    def _sde_init(self, kwargs):
        who = self._name()
        if kwargs.get("zero_terminal_snr"):
            raise ValueError(f"{who}: zero_terminal_snr=True is not supported (sigma_max of a zero-terminal-SNR schedule is infinite)")
        if kwargs.get("guidance_rescale"):
            raise ValueError(f"{who}: guidance_rescale={kwargs['guidance_rescale']} is not supported by the SDE solvers")
        st = kwargs.get("solver_type")
        if self.kind == "3m" and st is not None:
            raise ValueError(f"{who}: solver_type={st!r} is an option of the 2M solvers (dpm++_2m_sde*); 3M has one form")
        self.solver_type = st or "midpoint"
        if self.solver_type not in SOLVER_TYPES:
            raise ValueError(f"{who}: solver_type={self.solver_type!r}: one of {SOLVER_TYPES}")
        for k in ("eta", "s_noise"):
            v = kwargs.get(k)
            v = 1.0 if v is None else float(v)
            if not math.isfinite(v) or v < 0.0:
                raise ValueError(f"{who}: {k}={v}: a finite number >= 0")
            setattr(self, k, v)
        self.sigma_schedule = kwargs.get("sigma_schedule") or "karras"
        if self.sigma_schedule not in SIGMA_SCHEDULES:
            raise ValueError(f"{who}: sigma_schedule={self.sigma_schedule!r}: one of {SIGMA_SCHEDULES}")

    def sde_sigmas(self) -> torch.Tensor:
        return self.tables.karras_sigmas() if self.sigma_schedule == "karras" else self.tables.exponential_sigmas()

    def _refuse_job(self, kwargs):
        for k in ("src_img", "mask", "strength"):
            if kwargs.get(k) is not None:
                raise ValueError(f"{self._name()}: {k}=... - inversion, edit and inpaint jobs are not supported by the SDE solvers")

    def inversion(self, *args, **kwargs):
        raise ValueError(f"{self._name()}: inversion is not supported (a stochastic multistep update is not an invertible DDIM update)")

    def _sde_start(self, size, sigmas, seeds, latents=None):
        """the fp32 start latent: standard normals (``latents``, else ``_randn(seeds)``) times sigma_0"""
        z = self._randn(tuple(size), seeds) if latents is None else latents.detach().to("cpu", torch.float32)
        if tuple(z.shape) != tuple(size):
            raise ValueError(f"{self._name()}: latents of shape {tuple(z.shape)} for a job of shape {tuple(size)}")
        return (z.to(torch.float32) * float(sigmas[0])).to(self.work_device).contiguous()

    def _sde_loop(self, x, sigmas, uc, c, lam: float, seeds, *, added=None, callback_fn=None, desc="SDE"):
        """THE SDE loop: one cfgpp_sde_input per job; per step one UNet call (and, for a v-model, one cfgpp_v_to_eps) and one
        cfgpp_step_sde launch.  The history lives in a ring of buffers that is rotated, never copied.  Returns (denoised, x)."""
        eng = self.engine
        depth = 1 if self.kind == "2m" else 2
        den, xc = torch.empty_like(x), torch.empty_like(x, dtype=torch.float16)
        ring = [torch.empty_like(x) for _ in range(depth + 1)]          # most recent first; the last one is written next
        n = len(sigmas) - 1
        have = 0
        eng.sde_input(x, xc, input_scale(sigmas[0]))
        for i in _progress(range(n), desc):
            sigma = sigmas[i]
            last = float(sigmas[i + 1]) == 0.0
            t = self.timestep(sigma)
            m_uc, m_c = self._predict(xc, t, uc, c, added)
            self._eps_from_v(m_uc, m_c, xc, sigma)
            coef = sde_coeffs(sigmas, i, self.kind, self.solver_type, self.eta, self.s_noise, self.cfgpp, have)
            eng.step_sde(x, den, None if last else xc, ring[0] if have >= 1 else None, ring[1] if have == 2 else None,
                         None if last else ring[-1], m_uc, m_c, lam, coef, self.cfgpp, have, last, seeds=seeds, draw=i)
            ring = [ring[-1]] + ring[:-1]
            have = min(have + 1, depth)
            if callback_fn is not None:
                self._run_callback(callback_fn, i, t, den, x)
                if not last:                    # a callback may have replaced x: the next UNet input follows it
                    eng.sde_input(x, xc, coef[7])
        return den, x


class _SDESolverSD(_SDEMixin, StableDiffusion):
    """SD1.5 family: ``sample(cfg_guidance, prompt=[null, text], seeds=[...], latents=None, return_latents=False)``; ``latents``:
    standard-normal start noise [B, 4, h, w] in place of ``_randn(seeds)`` (it is multiplied by sigma_0 here)"""

    def __init__(self, solver_config, **kwargs):
        self._sde_init(kwargs)
        StableDiffusion.__init__(self, solver_config, **kwargs)

    @torch.no_grad()
    @controlled
    def sample(self, cfg_guidance=7.5, prompt=["", ""], callback_fn=None, **kwargs):
        self._refuse_job(kwargs)
        uc, c = self._embeds(prompt, kwargs)
        B = int(c.shape[0])
        sigmas = self.sde_sigmas()
        x = self._sde_start((B, self.cfg.out_channels) + self.latent_hw, sigmas, kwargs.get("seeds"), kwargs.get("latents"))
        seeds = self._chain_seeds(kwargs.get("seeds"), B, self._name())
        den, x = self._sde_loop(x, sigmas, uc, c, float(cfg_guidance), seeds, callback_fn=callback_fn)
        return self._result(kwargs.get("return_latents"), (den, x), den)


class _SDESolverXL(_SDEMixin, SDXL):
    """SDXL family: ``SDXL.sample``'s arguments (prompt1 / prompt2 or prompt_embeds, size conditioning) plus ``seeds``, ``latents``,
    ``return_latents``"""

    def __init__(self, solver_config, **kwargs):
        self._sde_init(kwargs)
        SDXL.__init__(self, solver_config, **kwargs)

    @torch.no_grad()
    def sample(self, prompt1=["", ""], prompt2=["", ""], cfg_guidance=5.0, **kwargs):
        self._refuse_job(kwargs)
        ret_lat = kwargs.pop("return_latents", False)
        den, x = SDXL.sample(self, prompt1, prompt2, cfg_guidance, return_latents=True, **kwargs)
        return (den, x) if ret_lat else self._finish(den)

    def reverse_process(self, null_prompt_embeds, prompt_embeds, cfg_guidance, add_cond_kwargs, shape=(1024, 1024), callback_fn=None,
                        **kwargs):
        sigmas = self.sde_sigmas()
        size = self._latent_size(shape)
        x = self._sde_start(size, sigmas, kwargs.get("seeds"), kwargs.get("latents"))
        seeds = self._chain_seeds(kwargs.get("seeds"), int(size[0]), self._name())
        return self._sde_loop(x, sigmas, null_prompt_embeds, prompt_embeds, float(cfg_guidance), seeds, added=add_cond_kwargs,
                              callback_fn=callback_fn, desc="SDXL SDE")


@register_sde_solver("dpm++_2m_sde", "sd15")
class DPMpp2mSDE(_SDESolverSD):
    """DPM-Solver++(2M) SDE with CFG"""
    kind, cfgpp = "2m", False


@register_sde_solver("dpm++_2m_sde_cfg++", "sd15")
class DPMpp2mSDECFGpp(_SDESolverSD):
    """DPM-Solver++(2M) SDE with CFG++"""
    kind, cfgpp = "2m", True


@register_sde_solver("dpm++_3m_sde", "sd15")
class DPMpp3mSDE(_SDESolverSD):
    """DPM-Solver++(3M) SDE with CFG"""
    kind, cfgpp = "3m", False


@register_sde_solver("dpm++_3m_sde_cfg++", "sd15")
class DPMpp3mSDECFGpp(_SDESolverSD):
    """DPM-Solver++(3M) SDE with CFG++"""
    kind, cfgpp = "3m", True


@register_sde_solver("dpm++_2m_sde", "sdxl")
class DPMpp2mSDEXL(_SDESolverXL):
    """DPM-Solver++(2M) SDE with CFG, SDXL"""
    kind, cfgpp = "2m", False


@register_sde_solver("dpm++_2m_sde_cfg++", "sdxl")
class DPMpp2mSDECFGppXL(_SDESolverXL):
    """DPM-Solver++(2M) SDE with CFG++, SDXL"""
    kind, cfgpp = "2m", True


@register_sde_solver("dpm++_3m_sde", "sdxl")
class DPMpp3mSDEXL(_SDESolverXL):
    """DPM-Solver++(3M) SDE with CFG, SDXL"""
    kind, cfgpp = "3m", False


@register_sde_solver("dpm++_3m_sde_cfg++", "sdxl")
class DPMpp3mSDECFGppXL(_SDESolverXL):
    """DPM-Solver++(3M) SDE with CFG++, SDXL"""
    kind, cfgpp = "3m", True
