"""DPM-Solver++ SDE sampling (k-diffusion's ``sample_dpmpp_sde``: "DPM++ SDE Karras") with CFG and with CFG++: the two-stage,
two-UNet-calls-per-step sibling of the 2M / 3M SDE solvers of ``sde.py``.  The reference has no such sampler, so there is no fp16 torch
arithmetic to mirror: the latent is fp32 and each UNet call is followed by ONE fused launch (include/cfgpp_dpmpp_sde.h:
cfgpp_step_sde_stage) - guidance mix, denoised estimates, the stage's linear combination, the noise drawn in registers and the next
UNet call's fp16 input.  N sampling steps make 2N - 1 UNet calls (the last step has one stage).

Its own registry (like ``sde.py``; ``get_sde_solver("dpm++_sde")`` stays refused):
``get_dpmpp_sde_solver(name, model="sd15" | "sdxl", eta=1.0, s_noise=1.0, sigma_schedule="karras" | "exponential", **get_solver
kwargs)``; names: ``dpm++_sde``, ``dpm++_sde_cfg++``.  k-diffusion's ``r`` is fixed at its default 1/2 and is not an option: at 1/2
``denoised_d`` is ``denoised_2`` alone, which is what makes both stages one linear row each.

The update.  Per step: sigma = sigmas[i], sigma_n = sigmas[i + 1], sigma_mid = sqrt(sigma sigma_n), (sd1, su1) =
get_ancestral_step(sigma, sigma_mid, eta), (sd2, su2) = get_ancestral_step(sigma, sigma_n, eta).  Since -expm1(t - t_fn(sd)) =
1 - sd / sigma (t_fn(0) is never formed; sd = 0 simply gives a_x = 0):
    stage A:  x2 = (sd1 / sigma) x + (1 - sd1 / sigma) D  + su1 s_noise n1,        D  = x  - sigma     eps_hat(x,  sigma)
    stage B:  x' = (sd2 / sigma) x + (1 - sd2 / sigma) D2 + su2 s_noise nB,        D2 = x2 - sigma_mid eps_hat(x2, sigma_mid)
    sigma_n = 0:  one UNet call and x' = D
CFG++ (the reference's two-stage ``dpm++_2s_a_cfg++`` restated: stage A moves along the unconditional estimate, stage B is the
``a_d = a_0 + a_x``, ``a_u = -a_x`` rule of ``sde.py``), with uD = x - sigma eps_uc and uD2 = x2 - sigma_mid eps_uc:
    stage A:  x2 = (sd1 / sigma) x + (1 - sd1 / sigma) uD + noise
    stage B:  x' = (sd2 / sigma) x + D2 - (sd2 / sigma) uD2 + noise
So every stage is one row of  out = a_x x + a_d den + a_u uden + c_1 n1 + c_2 n2  with den / uden taken from a base latent (x in
stage A, x2 in stage B) and ``dpmpp_sde_coeffs`` makes the row.

Noise.  The two noise terms of a step cover overlapping intervals: stage A needs the Brownian increment over [sigma, sigma_mid], stage
B the one over [sigma, sigma_n].  With d1 = sigma - sigma_mid, d2 = sigma_mid - sigma_n and n1, n2 independent standard normals,
    nB = (sqrt(d1) n1 + sqrt(d2) n2) / sqrt(d1 + d2)
and n1 are the normalised increments of ONE path over those two intervals - exactly the law of k-diffusion's
``BrownianTreeNoiseSampler``.  The generator is counter-based (csrc/philox.h, stream id 3), so stage B draws stage A's n1 again
(the same counter: draw 2 i) next to a fresh n2 (draw 2 i + 1) and combines them with c_1 = su2 s_noise sqrt(d1 / (d1 + d2)),
c_2 = su2 s_noise sqrt(d2 / (d1 + d2)): no tensor is kept between the stages and no launch is added.  Keyed by the chains' seeds, so
chain b of a batch reproduces chain b run alone.  ``eta=0`` is a deterministic fp32 DPM-Solver++(2S).  The path is per step count:
runs with different N do not share one path.

Refused by name: zero_terminal_snr, guidance_rescale, solver_type, inversion / edit / inpaint (``src_img`` / ``mask`` /
``strength``), a negative or non-finite ``eta`` / ``s_noise``, a sharded run without per-rank ``seeds=``.  Graph replay is never
used: the eager loop runs, also under CFGPP_GRAPH=1.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

import numpy as np
import torch

from .latent_diffusion import _progress
from .registry import Registry
from .schedule import get_ancestral_step
from .sde import MODELS, _SDEMixin, _SDESolverSD, _SDESolverXL, input_scale

__DPMPP_SDE_SOLVER__ = Registry("DPMppSDESolver")
NOISE_STREAM = 3            # stream id of the path increments (include/cfgpp_dpmpp_sde.h); 0, 1, 2: LCM renoise, ancestral, 2M / 3M SDE
TERM_D, TERM_U, TERM_N1, TERM_N2 = 1, 2, 4, 8       # CFGPP_STAGE_*: which terms of the row are added
STAGES = ("A", "B")


def register_dpmpp_sde_solver(name: str, model: str):
    def add(cls):
        cls = __DPMPP_SDE_SOLVER__.register(f"{model}/{name}")(cls)
        cls.solver_name = name
        return cls
    return add


def get_dpmpp_sde_solver(name: str, model: str = "sd15", **kwargs):
    """``name``: one of ``dpmpp_sde_solver_names()``; ``model`` in {"sd15", "sdxl"}; kwargs as ``get_solver``'s plus ``eta`` (1.0),
    ``s_noise`` (1.0) and ``sigma_schedule`` ("karras" | "exponential")."""
    if model not in MODELS:
        raise ValueError(f"DPMppSDESolver model {model!r}: one of {MODELS}")
    try:
        cls = __DPMPP_SDE_SOLVER__[f"{model}/{name}"]
    except KeyError:
        raise ValueError(f"DPMppSDESolver {name} does not exist.") from None
    return cls(**kwargs)


def dpmpp_sde_solver_names():
    return sorted({k.split("/", 1)[1] for k in __DPMPP_SDE_SOLVER__})


# ---------------------------------------------------------------------------------------------------- coefficients (host)
class StageRow(NamedTuple):
    """one launch of cfgpp_step_sde_stage: ``coef`` = (sigma_b, a_x, a_d, a_u, c_1, c_2, s_in), ``terms`` the mask of TERM_* that are
    added, ``last``: out = den (the step whose next sigma is 0; its coefficients are zeros)"""
    coef: Tuple[float, ...]
    terms: int
    last: bool


def sigma_mid(sigmas, i: int) -> float:
    """sqrt(sigma_i sigma_{i+1}) in float64 from the fp32 table: where step ``i`` makes its second UNet call"""
    return math.sqrt(float(sigmas[i]) * float(sigmas[i + 1]))


def dpmpp_sde_coeffs64(sigmas, i: int, stage: str, eta: float = 1.0, s_noise: float = 1.0, cfgpp: bool = False) -> StageRow:
    """the row of stage ``stage`` ("A" | "B") of step ``i`` of ``sigmas`` (fp32 table with the trailing zero), in Python float64.
    The step whose next sigma is 0 has stage "A" only, with ``last`` set."""
    if stage not in STAGES:
        raise ValueError(f"dpmpp_sde_coeffs: stage={stage!r}: one of {STAGES}")
    sig, sig_n = float(sigmas[i]), float(sigmas[i + 1])
    if sig_n == 0.0:
        if stage == "B":
            raise ValueError(f"dpmpp_sde_coeffs: step {i} ends at sigma 0 and has one stage")
        return StageRow((sig, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0), 0, True)
    mid = sigma_mid(sigmas, i)
    to, sig_b = (mid, sig) if stage == "A" else (sig_n, mid)
    sd, su = get_ancestral_step(sig, to, eta)
    a_x = float(sd) / sig
    a_0 = 1.0 - a_x
    amp = float(su) * s_noise
    if stage == "A":
        a_d, a_u, terms = (0.0, a_0, TERM_U) if cfgpp else (a_0, 0.0, TERM_D)
        c_1, c_2 = amp, 0.0
        if amp != 0.0:
            terms |= TERM_N1
    else:
        a_d, a_u, terms = (a_0 + a_x, -a_x, TERM_D | TERM_U) if cfgpp else (a_0, 0.0, TERM_D)
        d1, d2 = sig - mid, mid - sig_n
        c_1, c_2 = amp * math.sqrt(d1 / (d1 + d2)), amp * math.sqrt(d2 / (d1 + d2))
        if amp != 0.0:
            terms |= TERM_N1 | TERM_N2
    return StageRow((sig_b, a_x, a_d, a_u, c_1, c_2, 1.0 / math.sqrt(to * to + 1.0)), terms, False)


def dpmpp_sde_coeffs(sigmas, i: int, stage: str, eta: float = 1.0, s_noise: float = 1.0, cfgpp: bool = False) -> StageRow:
    """``dpmpp_sde_coeffs64`` with each coefficient rounded once to fp32: what cfgpp_step_sde_stage is given"""
    row = dpmpp_sde_coeffs64(sigmas, i, stage, eta, s_noise, cfgpp)
    return StageRow(tuple(float(np.float32(v)) for v in row.coef), row.terms, row.last)


# ---------------------------------------------------------------------------------------------------- the solvers
class _DPMppSDEMixin(_SDEMixin):
    """``sde.py``'s options, schedule, start latent and refusals; the loop is the two-stage one"""
    cfgpp = False

    def _sde_init(self, kwargs):
        st = kwargs.get("solver_type")
        if st is not None:
            raise ValueError(f"{self._name()}: solver_type={st!r} is an option of the 2M solvers (dpm++_2m_sde*); dpm++_sde has one form")
        super()._sde_init(kwargs)

    def _sde_loop(self, x, sigmas, uc, c, lam: float, seeds, *, added=None, callback_fn=None, desc="DPM++ SDE"):
        """THE loop: one cfgpp_sde_input per job; per step UNet, stage A (x -> x2), UNet at sigma_mid, stage B (in place on x); the last
        step is one UNet call and one launch.  Both stages of step i pass the draws 2 i and 2 i + 1.  Stage B's denoised goes into
        x2, which nothing reads afterwards, so ``den`` is stage A's when the callback runs.  Returns (denoised, x)."""
        eng = self.engine
        x2, den, xc = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x, dtype=torch.float16)
        n = len(sigmas) - 1
        eng.sde_input(x, xc, input_scale(sigmas[0]))
        for i in _progress(range(n), desc):
            sigma = sigmas[i]
            t = self.timestep(sigma)
            draws = dict(seeds=seeds, draw1=2 * i, draw2=2 * i + 1)
            m_uc, m_c = self._predict(xc, t, uc, c, added)
            self._eps_from_v(m_uc, m_c, xc, sigma)
            a = dpmpp_sde_coeffs(sigmas, i, "A", self.eta, self.s_noise, self.cfgpp)
            if a.last:
                eng.step_sde_stage(x, x, x, den, None, m_uc, m_c, lam, a.coef, a.terms, True, **draws)
                s_next = None
            else:
                eng.step_sde_stage(x, x, x2, den, xc, m_uc, m_c, lam, a.coef, a.terms, False, **draws)
                b = dpmpp_sde_coeffs(sigmas, i, "B", self.eta, self.s_noise, self.cfgpp)
                mid = torch.tensor(b.coef[0], dtype=torch.float32)
                m_uc, m_c = self._predict(xc, self.timestep(mid), uc, c, added)
                self._eps_from_v(m_uc, m_c, xc, mid)
                eng.step_sde_stage(x, x2, x, x2, xc, m_uc, m_c, lam, b.coef, b.terms, False, **draws)
                s_next = b.coef[6]
            if callback_fn is not None:
                self._run_callback(callback_fn, i, t, den, x)
                if s_next is not None:          # a callback may have replaced x: the next UNet input follows it
                    eng.sde_input(x, xc, s_next)
        return den, x


class _DPMppSDESolverSD(_DPMppSDEMixin, _SDESolverSD):
    """SD1.5 family: ``sde.py``'s ``sample`` (``seeds``, ``latents``, ``return_latents``)"""


class _DPMppSDESolverXL(_DPMppSDEMixin, _SDESolverXL):
    """SDXL family: ``sde.py``'s ``sample`` / ``reverse_process``"""


@register_dpmpp_sde_solver("dpm++_sde", "sd15")
class DPMppSDE(_DPMppSDESolverSD):
    """DPM-Solver++ SDE with CFG"""
    cfgpp = False


@register_dpmpp_sde_solver("dpm++_sde_cfg++", "sd15")
class DPMppSDECFGpp(_DPMppSDESolverSD):
    """DPM-Solver++ SDE with CFG++"""
    cfgpp = True


@register_dpmpp_sde_solver("dpm++_sde", "sdxl")
class DPMppSDEXL(_DPMppSDESolverXL):
    """DPM-Solver++ SDE with CFG, SDXL"""
    cfgpp = False


@register_dpmpp_sde_solver("dpm++_sde_cfg++", "sdxl")
class DPMppSDECFGppXL(_DPMppSDESolverXL):
    """DPM-Solver++ SDE with CFG++, SDXL"""
    cfgpp = True
