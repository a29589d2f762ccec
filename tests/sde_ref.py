"""The model the SDE-solver tests compare against (include/cfgpp_sde.h and cfgpp_amd/sde.py restated): k-diffusion's two algorithms
written literally in float64 with step-by-step history variables (NOT the expanded coefficients), the CFG++ substitution, and a torch
restatement of the header's expression sequence.  The Philox model is tests/lcm_ref.py's.  No product code is imported here.

``faults``: a set of names; each switches ONE deliberate error into the model so that tests/test_sde_cpu.py can require the assertion
that guards that property to fail (the house style of fault injection)."""
from __future__ import annotations

import math

import numpy as np
import torch

import lcm_ref as R

NOISE_STREAM = 2


# ---- schedules --------------------------------------------------------------------------------------------------------------------
def sigmas_exponential(n, sigma_min, sigma_max):
    """float64: exp(linspace(ln sigma_max, ln sigma_min, n)), then 0"""
    return np.concatenate([np.exp(np.linspace(math.log(sigma_max), math.log(sigma_min), n)), [0.0]])


def sigmas_karras(n, sigma_min, sigma_max, rho=7.0):
    ramp = np.linspace(0, 1, n + 1)[:-1]
    lo, hi = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
    return np.concatenate([(hi + ramp * (lo - hi)) ** rho, [0.0]])


# ---- the two algorithms, literally ------------------------------------------------------------------------------------------------
def _t(sigma):
    return -math.log(sigma)


def literal_chain(kind, denoise, x, sigmas, noises, eta=1.0, s_noise=1.0, solver_type="midpoint", cfgpp=False):
    """k-diffusion's sample_dpmpp_2m_sde / sample_dpmpp_3m_sde in float64.  ``denoise(x, i) -> (den, uden)``: the guided and the
    unconditional denoised estimate at step i; ``noises[i]``: the standard normals of step i.  CFG++: the current noise is eps_uc, so
    the x that the decay term multiplies is den + sigma eps_uc = x - uden + den, and the history holds uden.  -> list of x_{i+1}"""
    xs = []
    old, older = None, None                 # 2m: old_denoised;  3m: denoised_1, denoised_2
    h_1, h_2 = None, None
    for i in range(len(sigmas) - 1):
        den, uden = denoise(x, i)
        keep = uden if cfgpp else den
        if sigmas[i + 1] == 0:
            x = den
        else:
            t, s = _t(sigmas[i]), _t(sigmas[i + 1])
            h = s - t
            eta_h = eta * h
            x_eff = x - uden + den if cfgpp else x
            if kind == "2m":
                x = sigmas[i + 1] / sigmas[i] * math.exp(-eta_h) * x_eff + (-math.expm1(-h - eta_h)) * den
                if old is not None:
                    r = h_1 / h
                    if solver_type == "heun":
                        x = x + ((-math.expm1(-h - eta_h)) / (-h - eta_h) + 1) * (1 / r) * (den - old)
                    else:
                        x = x + 0.5 * (-math.expm1(-h - eta_h)) * (1 / r) * (den - old)
            else:
                h_eta = h * (eta + 1)
                x = math.exp(-h_eta) * x_eff + (-math.expm1(-h_eta)) * den
                if h_2 is not None:
                    r0, r1 = h_1 / h, h_2 / h
                    d1_0, d1_1 = (den - old) / r0, (old - older) / r1
                    d1 = d1_0 + (d1_0 - d1_1) * r0 / (r0 + r1)
                    d2 = (d1_0 - d1_1) / (r0 + r1)
                    phi_2 = math.expm1(-h_eta) / h_eta + 1
                    phi_3 = phi_2 / h_eta - 0.5
                    x = x + phi_2 * d1 - phi_3 * d2
                elif h_1 is not None:
                    r = h_1 / h
                    d = (den - old) / r
                    phi_2 = math.expm1(-h_eta) / h_eta + 1
                    x = x + phi_2 * d
            if eta:
                x = x + noises[i] * sigmas[i + 1] * math.sqrt(-math.expm1(-2 * eta_h)) * s_noise
            h_1, h_2 = h, h_1
        old, older = keep, old
        xs.append(x)
    return xs


def coefficient_chain(coef_fn, kind, denoise, x, sigmas, noises, cfgpp=False):
    """the same chain from expanded coefficients ``coef_fn(i, n_hist) -> (sigma, a_x, a_d, a_u, a_1, a_2, a_n, s_in)`` in float64"""
    xs, hist = [], []
    depth = 1 if kind == "2m" else 2
    for i in range(len(sigmas) - 1):
        den, uden = denoise(x, i)
        n_hist = min(len(hist), depth)
        if sigmas[i + 1] == 0:
            x = den
        else:
            _, a_x, a_d, a_u, a_1, a_2, a_n, _ = coef_fn(i, n_hist)
            acc = a_x * x + a_d * den
            if cfgpp:
                acc = acc + a_u * uden
            if n_hist >= 1:
                acc = acc + a_1 * hist[0]
            if n_hist == 2:
                acc = acc + a_2 * hist[1]
            if a_n != 0:
                acc = acc + a_n * noises[i]
            x = acc
        hist = [uden if cfgpp else den] + hist[:1]
        xs.append(x)
    return xs


# ---- the step, in the header's expression sequence --------------------------------------------------------------------------------
def step_sde(x, hist1, hist2, m_uc, m_c, lam, coef, cfgpp, n_hist, last, noise, single=None, faults=()):
    """-> (den, hist value, x', xc) on x's device: fp32, fp32, fp32, fp16; every operation is one fp32 torch op (one rounding).
    ``single`` (default: ``m_uc is m_c``): m_hat is m_uc itself."""
    f, h = torch.float32, torch.float16
    sigma, a_x, a_d, a_u, a_1, a_2, a_n, s_in = (torch.tensor(float(v), dtype=f, device=x.device) for v in coef)
    if "a_u_sign" in faults:
        a_u = -a_u
    single = (m_uc is m_c) if single is None else single
    hat = m_uc.to(f) if single else R.cfg_mix(m_uc, m_c, lam).to(f)
    den = x - sigma * hat
    uden = x - sigma * m_uc.to(f) if cfgpp else den
    if last:
        xn = den.clone()
        if "noise_on_last" in faults:
            xn = xn + noise.to(f)
    else:
        acc = a_x * x
        acc = acc + a_d * den
        if cfgpp:
            acc = acc + a_u * uden
        if n_hist >= 1:
            acc = acc + a_1 * hist1
        if n_hist == 2:
            acc = acc + a_2 * hist2
        if float(a_n) != 0.0:
            acc = acc + a_n * noise.to(f)
        xn = acc
    keep = den if "cfgpp_hist_den" in faults else uden
    return den, keep.clone(), xn, (xn * s_in).to(h)


def noise_rows(B, row_elems, seeds, draw, shape=None):
    """the step noise of cfgpp_step_sde with noise = NULL: the float64 Philox model (stream 2) rounded to fp32"""
    n = torch.from_numpy(R.normal_rows(B, row_elems, seeds, draw, NOISE_STREAM).astype(np.float32))
    return n if shape is None else n.reshape(shape)


def sde_chain(model_fn, z, seeds, sigmas, coef_fn, kind, lam, cfgpp=False, faults=()):
    """the whole solver loop on the model's noise: ``z`` standard normals (times sigma_0 here), ``model_fn(xc fp16, i) -> (m_uc, m_c)``
    fp16 epsilon, ``coef_fn(i, n_hist)`` the step's coef8.  -> (den, x, per-step record list)"""
    B, row = int(z.shape[0]), int(z[0].numel())
    depth = 1 if kind == "2m" else 2
    x = z.to(torch.float32) * float(sigmas[0])
    s0 = float(np.float32(1.0 / math.sqrt(float(sigmas[0]) ** 2 + 1.0)))
    xc = (x * torch.tensor(s0, dtype=torch.float32)).to(torch.float16)
    hist, rec, den = [], [], None
    n = len(sigmas) - 1
    for i in range(n):
        last = i == n - 1
        n_hist = min(len(hist), depth)
        coef = coef_fn(i, n_hist)
        draw = 0 if "draw_stuck" in faults else i
        noise = noise_rows(B, row, seeds, draw, z.shape).to(z.device)
        m_uc, m_c = model_fn(xc, i)
        den, keep, x, xc = step_sde(x, hist[0] if n_hist >= 1 else None, hist[1] if n_hist == 2 else None, m_uc, m_c, lam, coef, cfgpp,
                                    n_hist, last, noise, faults=faults)
        hist = (hist[:1] + [keep]) if "hist_not_rotated" in faults else ([keep] + hist[:1])
        rec.append(dict(draw=draw, last=last, coef=coef, n_hist=n_hist))
    return den, x, rec
