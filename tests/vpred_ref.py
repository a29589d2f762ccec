"""Restatements of the v-prediction arithmetic (include/cfgpp_vpred.h) the tests compare against - no product code in here.

With a = sqrt(alpha), s = sqrt(1-alpha) a v-prediction model returns v = a*eps - s*x0 at z = a*x0 + s*eps, so
    x0 = a*z - s*v        eps = a*v + s*z

* ``ddim_v_f64`` / ``ddim_eps_f64``: the generalised DDIM update in float64, v form and the eps form of oracle/sampler.py's DDIM
  family (``ddim_step``'s docstring; that function itself casts to fp32, so its formula is restated here in float64).
* ``ddim_v_natural`` / ``v_to_eps_natural``: the update as a torch user writes it - 0-dim fp32 CPU scalars first, tensors of whatever
  dtype and device.  Evaluated by torch-CPU it has the "cpu" scalar semantics of cfgpp_amd/coeffs.py, by torch on a GPU the "cuda"
  ones.
* ``ddim_v_step`` / ``v_to_eps_step``: the same with every rounding spelled out on the oracle's primitives, for both semantics.
* ``rescale_f64`` / ``rescale_f32_two_pass`` / ``rescale_f32_naive``: the guidance-rescale factor.
* whole-loop drivers for the solver tests.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import sampler as O

H, F, D = torch.float16, torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------ float64
def v_from_eps(eps, z, alpha):
    a, s = math.sqrt(alpha), math.sqrt(1.0 - alpha)
    return (eps - s * z) / a


def ddim_eps_f64(z, e_uc, e_c, lam, a_tw, a_rn, tweedie_uc, renoise_uc):
    """oracle/sampler.py ddim_step: z0t = (z - sqrt(1-a_tw)*A)/sqrt(a_tw); z' = sqrt(a_rn)*z0t + sqrt(1-a_rn)*B"""
    hat = e_uc + lam * (e_c - e_uc)
    A = e_uc if tweedie_uc else hat
    B = e_uc if renoise_uc else hat
    z0t = (z - math.sqrt(1 - a_tw) * A) / math.sqrt(a_tw)
    return z0t, math.sqrt(a_rn) * z0t + math.sqrt(1 - a_rn) * B


def ddim_v_f64(z, v_uc, v_c, lam, a_tw, a_rn, tweedie_uc, renoise_uc):
    a, s = math.sqrt(a_tw), math.sqrt(1 - a_tw)
    hat = v_uc + lam * (v_c - v_uc)
    A = v_uc if tweedie_uc else hat
    B = v_uc if renoise_uc else hat
    z0t = a * z - s * A
    epsB = a * B + s * z
    return z0t, math.sqrt(a_rn) * z0t + math.sqrt(1 - a_rn) * epsB


# ------------------------------------------------------------------------------------------------ as a torch user writes it
def _scaled(v_hat, row_scale):
    """our contract for guidance rescale: v_hat <- h(fl(f_b * v_hat)), the factor fp32 [B]"""
    f = row_scale.to(device=v_hat.device, dtype=F).view(-1, *([1] * (v_hat.dim() - 1)))
    return (f * v_hat.to(F)).to(v_hat.dtype)


def ddim_v_natural(zt, v_uc, v_c, lam, sqrt4, tweedie_uc, renoise_uc, row_scale=None):
    """``sqrt4`` = (sqrt(1-a_tw), sqrt(a_tw), sqrt(a_rn), sqrt(1-a_rn)) as 0-dim fp32 CPU tensors; zt / v on any one device"""
    s_t, a_t, a_p, s_p = (torch.as_tensor(x, dtype=F).reshape(()) for x in sqrt4)
    v_hat = v_uc + lam * (v_c - v_uc)
    if row_scale is not None:
        v_hat = _scaled(v_hat, row_scale)
    A = v_uc if tweedie_uc else v_hat
    B = v_uc if renoise_uc else v_hat
    z0t = a_t * zt - s_t * A
    epsB = a_t * B + s_t * zt
    zn = a_p * z0t + s_p * epsB
    return z0t, zn


def v_to_eps_natural(v, x, a, s):
    a, s = (torch.as_tensor(c, dtype=F).reshape(()) for c in (a, s))
    return a * v + s * x


def v_to_eps_scalars(sigma):
    """(a, s) = 1/sqrt(sigma^2+1), sigma/sqrt(sigma^2+1) as 0-dim fp32 tensors"""
    sig = torch.as_tensor(sigma, dtype=F).reshape(())
    den = (sig ** 2 + 1) ** 0.5
    return 1.0 / den, sig / den


# ------------------------------------------------------------------------------------------------ every rounding spelled out
def ddim_v_step(z, v_uc, v_c, lam, sqrt4, tweedie_uc, renoise_uc, semantics="cpu", row_scale=None):
    c1, c2, c3, c4 = sqrt4
    hat = O.cfg_mix(v_uc, v_c, lam)
    if row_scale is not None:
        hat = _scaled(hat, row_scale)
    A = v_uc if tweedie_uc else hat
    B = v_uc if renoise_uc else hat
    m = lambda s, x: O._smul_first(s, x, semantics)  # noqa: E731   fp16 x: one fp16 rounding, scalar per `semantics`; fp32 x: fp32
    z0t = O._sub(m(c2, z), m(c1, A))
    epsB = O._add(m(c2, B), m(c1, z))
    zn = O._add(m(c3, z0t), m(c4, epsB))
    return z0t, zn


def v_to_eps_step(v, x, a, s, semantics="cpu"):
    return O._add(O._smul_first(a, v, semantics), O._smul_first(s, x, semantics))


# ------------------------------------------------------------------------------------------------ guidance rescale
def rescale_f64(v_uc, v_c, lam, phi):
    """f_b in float64 over v_hat with the kernels' fp16 guidance mix; 1 where std(v_hat) == 0"""
    hat = O.cfg_mix(v_uc, v_c, lam).to(D).flatten(1)
    c = v_c.to(D).flatten(1)
    sc, sh = c.std(dim=1, unbiased=True), hat.std(dim=1, unbiased=True)
    return torch.where(sh > 0, phi * sc / sh.clamp_min(1e-300) + (1 - phi), torch.ones_like(sh))


def _pairwise_sum_f32(x: np.ndarray) -> np.float32:
    x = x.astype(np.float32)
    while x.size > 1:
        if x.size % 2:
            x = np.concatenate([x, np.zeros(1, np.float32)])
        x = (x[0::2] + x[1::2]).astype(np.float32)
    return np.float32(x[0])


def _ratio_to_f(r, phi):
    return np.float32(1) + np.float32(phi) * (np.float32(r) - np.float32(1))


def rescale_f32_two_pass(v_uc, v_c, lam, phi):
    """an fp32 model of the kernel's form: mean, then sum of squared deviations, pairwise fp32 sums"""
    hat = O.cfg_mix(v_uc, v_c, lam).float().flatten(1).numpy()
    c = v_c.float().flatten(1).numpy()
    out = []
    for b in range(c.shape[0]):
        n = np.float32(c.shape[1])
        m2 = []
        for x in (c[b], hat[b]):
            mean = _pairwise_sum_f32(x) / n
            d = (x - mean).astype(np.float32)
            m2.append(_pairwise_sum_f32((d * d).astype(np.float32)))
        out.append(1.0 if m2[1] == 0 else float(_ratio_to_f(np.sqrt(m2[0] / m2[1], dtype=np.float32), phi)))
    return torch.tensor(out, dtype=D)


def rescale_f32_naive(v_uc, v_c, lam, phi):
    """what the kernel must NOT do: var = E[x^2] - E[x]^2 in fp32"""
    hat = O.cfg_mix(v_uc, v_c, lam).float().flatten(1).numpy()
    c = v_c.float().flatten(1).numpy()
    out = []
    for b in range(c.shape[0]):
        n = np.float32(c.shape[1])
        var = []
        for x in (c[b], hat[b]):
            mean = _pairwise_sum_f32(x) / n
            ex2 = _pairwise_sum_f32((x * x).astype(np.float32)) / n
            var.append(np.float32(ex2 - mean * mean))
        r = np.sqrt(np.float32(max(var[0], 0)) / var[1], dtype=np.float32) if var[1] > 0 else np.float32(np.inf)
        out.append(float(_ratio_to_f(r, phi)))
    return torch.tensor(out, dtype=D)


def rescale_bound(row_elems: int) -> float:
    """(log2(row_elems) + 8) * 2^-23: the pairwise-summation bound with margin"""
    return (math.log2(row_elems) + 8) * 2.0 ** -23


def cancellation_case(B, row_elems, seed=0):
    """values 8 + 0.01*randn rounded to fp16: |mean| = 800 sigma"""
    g = torch.Generator().manual_seed(seed)
    mk = lambda: (8 + 0.01 * torch.randn((B, row_elems), generator=g)).to(H)  # noqa: E731
    return mk(), mk()


# ------------------------------------------------------------------------------------------------ whole loops (fp32 / fp16 latents)
def sample_ddim_v(unet_fn, zT, tables, lam, cfgpp, wrap=False, inversion=False, semantics="cpu", phi=0.0):
    """DDIM / DDIM-CFG++ (or, with ``inversion``, the inversion over the reversed timesteps) of a v-prediction model:
    unet_fn(z, t) -> (v_uc, v_c).  Returns (z0t, zt)."""
    zt = zT.clone() if zT.dtype == H else zT.clone().to(F)
    z0t = None
    ts = tables.timesteps.flip(0) if inversion else tables.timesteps
    ts = ts.int() if wrap else ts
    for t in ts:
        v_uc, v_c = unet_fn(zt, t)
        rs = rescale_f64(v_uc, v_c, lam, phi).to(F) if phi > 0 else None
        tw, rn = (cfgpp, False) if inversion else (False, cfgpp)
        z0t, zt = ddim_v_step(zt, v_uc, v_c, lam, tables.ddim_sqrt_coeffs(t, wrap=wrap, inversion=inversion), tw, rn, semantics, rs)
    return z0t, zt
