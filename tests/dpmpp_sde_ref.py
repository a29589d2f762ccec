"""The model the DPM++ SDE tests compare against (include/cfgpp_dpmpp_sde.h and cfgpp_amd/dpmpp_sde.py restated): k-diffusion's
``sample_dpmpp_sde`` written literally in float64 with a noise sampler built from ONE explicit Brownian path, the reference's two
2S CFG++ lines written literally, the same chains from expanded rows, and a torch restatement of the header's expression sequence.
The Philox model is tests/lcm_ref.py's.  No product code is imported here."""
from __future__ import annotations

import math

import numpy as np
import torch

import lcm_ref as R

NOISE_STREAM = 3
TERM_D, TERM_U, TERM_N1, TERM_N2 = 1, 2, 4, 8


# ---- k-diffusion, literally -------------------------------------------------------------------------------------------------------
def get_ancestral_step(sigma_from, sigma_to, eta=1.0):
    if not eta:
        return sigma_to, 0.0
    sigma_up = min(sigma_to, eta * (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


class PathNoise:
    """k-diffusion's BrownianTreeNoiseSampler interface on one explicit path in sigma, per step: W(sigma) = 0,
    W(sigma_mid) = sqrt(d1) n1, W(sigma_n) = sqrt(d1) n1 + sqrt(d2) n2;  __call__(s0, s1) = (W(s1) - W(s0)) / sqrt(|s1 - s0|).
    The arguments are the algorithm's own sigma_fn(t) values, a rounding away from the knots: the nearest knot is meant."""

    def __init__(self, sigma, sigma_n, n1, n2):
        mid = math.sqrt(sigma * sigma_n)
        d1, d2 = sigma - mid, mid - sigma_n
        self.knots = np.array([sigma, mid, sigma_n])
        self.W = [0.0 * n1, math.sqrt(d1) * n1, math.sqrt(d1) * n1 + math.sqrt(d2) * n2]

    def _at(self, s):
        return self.W[int(np.abs(self.knots - float(s)).argmin())]

    def __call__(self, s0, s1):
        return (self._at(s1) - self._at(s0)) / np.sqrt(np.abs(s1 - s0))


def literal_chain(denoise, x, sigmas, n1s, n2s, eta=1.0, s_noise=1.0, r=0.5):
    """sample_dpmpp_sde in float64 numpy.  ``denoise(x, sigma) -> (den, uden)``; uden is ignored (plain CFG).  sigma_down = 0
    (eta of about 2 or more) goes through t_fn(0) = inf here, as it does in k-diffusion.  -> list of x_{i+1}"""
    t_fn = lambda sigma: -np.log(np.float64(sigma))  # noqa: E731
    sigma_fn = lambda t: np.exp(-t)  # noqa: E731
    xs = []
    with np.errstate(divide="ignore"):
        for i in range(len(sigmas) - 1):
            denoised, _ = denoise(x, sigmas[i])
            if sigmas[i + 1] == 0:
                d = (x - denoised) / sigmas[i]
                dt = sigmas[i + 1] - sigmas[i]
                x = x + d * dt
            else:
                noise_sampler = PathNoise(sigmas[i], sigmas[i + 1], n1s[i], n2s[i])
                t, t_next = t_fn(sigmas[i]), t_fn(sigmas[i + 1])
                h = t_next - t
                s = t + h * r
                fac = 1 / (2 * r)
                sd, su = get_ancestral_step(sigma_fn(t), sigma_fn(s), eta)
                s_ = t_fn(sd)
                x_2 = (sigma_fn(s_) / sigma_fn(t)) * x - np.expm1(t - s_) * denoised
                x_2 = x_2 + noise_sampler(sigma_fn(t), sigma_fn(s)) * s_noise * su
                denoised_2, _ = denoise(x_2, sigma_fn(s))
                sd, su = get_ancestral_step(sigma_fn(t), sigma_fn(t_next), eta)
                t_next_ = t_fn(sd)
                denoised_d = (1 - fac) * denoised + fac * denoised_2
                x = (sigma_fn(t_next_) / sigma_fn(t)) * x - np.expm1(t - t_next_) * denoised_d
                x = x + noise_sampler(sigma_fn(t), sigma_fn(t_next)) * s_noise * su
            xs.append(x)
    return xs


def literal_2s_cfgpp(denoise, x, sigmas):
    """the reference's deterministic two-stage CFG++ update (its ``dpm++_2s_a_cfg++`` with sigma_down := sigma_{i+1}, no noise
    addition) in float64 numpy.  -> list of x_{i+1}"""
    t_fn = lambda sigma: -np.log(np.float64(sigma))  # noqa: E731
    sigma_fn = lambda t: np.exp(-t)  # noqa: E731
    xs = []
    for i in range(len(sigmas) - 1):
        denoised, uncond_denoised = denoise(x, sigmas[i])
        sigma_down = sigmas[i + 1]
        if sigma_down == 0:
            d = (x - uncond_denoised) / sigmas[i]
            x = denoised + d * sigma_down
        else:
            t, t_next = t_fn(sigmas[i]), t_fn(sigma_down)
            r = 1 / 2
            h = t_next - t
            s = t + r * h
            x_2 = (sigma_fn(s) / sigma_fn(t)) * x - np.expm1(-h * r) * uncond_denoised
            denoised_2, uncond_denoised_2 = denoise(x_2, sigma_fn(s))
            x = denoised_2 - np.exp(-h) * uncond_denoised_2 + (sigma_fn(t_next) / sigma_fn(t)) * x
        xs.append(x)
    return xs


def row_chain(row_fn, denoise, x, sigmas, n1s, n2s, b_n1s=None):
    """the same chains from expanded rows ``row_fn(i, stage) -> ((sigma_b, a_x, a_d, a_u, c_1, c_2, s_in), terms, last)`` in float64.
    ``b_n1s``: a deliberate error - stage B's n1 taken from there instead of being stage A's"""
    def apply(row, x, base, n1, n2):
        (sigma_b, a_x, a_d, a_u, c_1, c_2, _), terms, last = row
        den, uden = denoise(base, sigma_b)
        if last:
            return den
        acc = a_x * x
        if terms & TERM_D:
            acc = acc + a_d * den
        if terms & TERM_U:
            acc = acc + a_u * uden
        if terms & TERM_N1:
            acc = acc + c_1 * n1
        if terms & TERM_N2:
            acc = acc + c_2 * n2
        return acc
    xs = []
    for i in range(len(sigmas) - 1):
        a = row_fn(i, "A")
        if a[2]:
            x = apply(a, x, x, None, None)
        else:
            x2 = apply(a, x, x, n1s[i], n2s[i])
            x = apply(row_fn(i, "B"), x, x2, (b_n1s or n1s)[i], n2s[i])
        xs.append(x)
    return xs


# ---- the stage, in the header's expression sequence -------------------------------------------------------------------------------
def stage(x, base, m_uc, m_c, lam, coef, terms, last, n1, n2, single=None):
    """-> (den, out, xc) on x's device: fp32, fp32, fp16; every operation is one fp32 torch op (one rounding).  ``single`` (default:
    ``m_uc is m_c``): m_hat is m_uc itself.  A term that is off touches neither its tensor nor its coefficient."""
    f, h = torch.float32, torch.float16
    sigma, a_x, a_d, a_u, c_1, c_2, s_in = (torch.tensor(float(v), dtype=f, device=base.device) for v in coef)
    single = (m_uc is m_c) if single is None else single
    hat = m_uc.to(f) if single else R.cfg_mix(m_uc, m_c, lam).to(f)
    den = base - sigma * hat
    if last:
        out = den.clone()
    else:
        acc = a_x * x
        if terms & TERM_D:
            acc = acc + a_d * den
        if terms & TERM_U:
            acc = acc + a_u * (base - sigma * m_uc.to(f))
        if terms & TERM_N1:
            acc = acc + c_1 * n1.to(f)
        if terms & TERM_N2:
            acc = acc + c_2 * n2.to(f)
        out = acc
    return den, out, (out * s_in).to(h)


def noise_rows(B, row_elems, seeds, draw, shape=None):
    """a noise term of cfgpp_step_sde_stage with its tensor NULL: the float64 Philox model (stream 3) rounded to fp32"""
    n = torch.from_numpy(R.normal_rows(B, row_elems, seeds, draw, NOISE_STREAM).astype(np.float32))
    return n if shape is None else n.reshape(shape)


def chain(model_fn, z, seeds, sigmas, row_fn, lam):
    """the whole solver loop on the model's noise: ``z`` standard normals (times sigma_0 here), ``model_fn(xc fp16, sigma fp32
    0-dim tensor) -> (m_uc, m_c)`` fp16 epsilon, ``row_fn(i, stage)`` the launch's fp32 row.  -> (den, x, per-launch record list)"""
    B, row = int(z.shape[0]), int(z[0].numel())
    x = z.to(torch.float32) * float(sigmas[0])
    s0 = float(np.float32(1.0 / math.sqrt(float(sigmas[0]) ** 2 + 1.0)))
    xc = (x * torch.tensor(s0, dtype=torch.float32)).to(torch.float16)
    rec, den = [], None
    for i in range(len(sigmas) - 1):
        n1, n2 = (noise_rows(B, row, seeds, d, z.shape) for d in (2 * i, 2 * i + 1))
        a = row_fn(i, "A")
        m_uc, m_c = model_fn(xc, sigmas[i])
        den, out, xc = stage(x, x, m_uc, m_c, lam, a[0], a[1], a[2], n1, n2)
        rec.append(dict(i=i, stage="A", row=a, sigma=float(sigmas[i]), den=den.clone()))
        if a[2]:
            x = out
            continue
        b = row_fn(i, "B")
        mid = torch.tensor(b[0][0], dtype=torch.float32)
        m_uc, m_c = model_fn(xc, mid)
        _, x, xc = stage(x, out, m_uc, m_c, lam, b[0], b[1], b[2], n1, n2)
        rec.append(dict(i=i, stage="B", row=b, sigma=float(mid)))
    return den, x, rec
