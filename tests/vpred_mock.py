"""``MockEngine`` (tests/mock_engine.py) plus the three v-prediction entry points of include/cfgpp_vpred.h, emulated at the kernels'
INTERFACE: fp32 coefficients in, explicit roundings - so the solvers' coefficient plumbing (cfgpp_amd/coeffs.py) is what the CPU
tests exercise.  Tests only; the product never constructs it."""
from __future__ import annotations

import torch

from mock_engine import MockEngine, _c, _f, _h
from oracle import sampler as O

H = torch.float16


def emulate_step_ddim_v(z, z0t_out, v_uc, v_c, lam, coef6, tweedie_uc, renoise_uc, row_scale=None):
    """what cfgpp_step_ddim_v computes (vpred_kernels.hip: ddim_v_step_kernel)"""
    a_z, s_v, a_v, s_z, c3, c4 = (_c(v) for v in coef6)
    r = lambda t: _f(_h(t))  # noqa: E731
    hat = O.cfg_mix(v_uc, v_c, lam)
    if row_scale is not None:
        f = row_scale.float().view(-1, *([1] * (z.dim() - 1)))
        hat = _h(f * _f(hat))
    A = _f(v_uc if tweedie_uc else hat)
    B = _f(v_uc if renoise_uc else hat)
    sA, aB = r(s_v * A), r(a_v * B)
    zf = _f(z)
    if z.dtype == H:
        z0 = r(r(a_z * zf) - sA)
        eb = r(aB + r(s_z * zf))
        zn = r(r(c3 * z0) + r(c4 * eb))
        z0t_out.copy_(_h(z0))
        z.copy_(_h(zn))
        return
    z0 = a_z * zf - sA
    eb = aB + s_z * zf
    zn = c3 * z0 + c4 * eb
    z0t_out.copy_(z0)
    z.copy_(zn)


def emulate_v_to_eps(eps_uc_out, eps_c_out, v_uc, v_c, x, a, s):
    """what cfgpp_v_to_eps computes; the outputs may be the inputs"""
    r = lambda t: _f(_h(t))  # noqa: E731
    sx = r(_c(s) * _f(x))
    e_uc, e_c = _h(r(_c(a) * _f(v_uc)) + sx), _h(r(_c(a) * _f(v_c)) + sx)
    eps_uc_out.copy_(e_uc)
    eps_c_out.copy_(e_c)


def emulate_cfg_rescale(v_uc, v_c, lam, phi, row_scale_out=None):
    """cfgpp_cfg_rescale's value: float64 statistics rounded once to fp32 (the kernel is within the documented bound of this)"""
    hat = O.cfg_mix(v_uc, v_c, lam).double().flatten(1)
    c = v_c.double().flatten(1)
    sc, sh = c.std(dim=1, unbiased=True), hat.std(dim=1, unbiased=True)
    f = torch.where(sh > 0, phi * sc / sh.clamp_min(1e-300) + (1 - phi), torch.ones_like(sh)).float()
    if row_scale_out is not None:
        row_scale_out.copy_(f)
        return row_scale_out
    return f


class VPredMockEngine(MockEngine):
    """records the v-prediction launches in ``vcalls`` (name, first coefficient) next to MockEngine's ``calls``"""

    def __init__(self, unet_fn, latent_hw=(8, 8)):
        super().__init__(unet_fn, latent_hw)
        self.vcalls = []

    def step_ddim_v(self, z, z0t_out, v_uc, v_c, lam, coef6, tweedie_uc, renoise_uc, row_scale=None):
        self.vcalls.append(("step_ddim_v", tuple(float(v) for v in coef6), row_scale is not None))
        emulate_step_ddim_v(z, z0t_out, v_uc, v_c, lam, coef6, tweedie_uc, renoise_uc, row_scale)

    def v_to_eps(self, eps_uc_out, eps_c_out, v_uc, v_c, x, a, s):
        self.vcalls.append(("v_to_eps", (float(a), float(s)), False))
        emulate_v_to_eps(eps_uc_out, eps_c_out, v_uc, v_c, x, a, s)

    def cfg_rescale(self, v_uc, v_c, lam, phi, row_scale_out=None):
        self.vcalls.append(("cfg_rescale", (float(lam), float(phi)), False))
        return emulate_cfg_rescale(v_uc, v_c, lam, phi, row_scale_out)
