"""CPU stand-in for the inpainting half of ``HipEngine`` (tests only): ``MockEngine`` plus the image condition of a 9-channel
UNet and the masked DDIM update, with the HIP kernels' interface and rounding (step_kernels.hip: ddim_step_masked_kernel)."""
from __future__ import annotations

import torch

from mock_engine import MockEngine, emulate_step_ddim


def emulate_step_ddim_masked(z, z0t_out, eps_uc, eps_c, lam, coeffs, tweedie_uc, renoise_uc, mask, src, noise, a, b):
    """what cfgpp_step_ddim_masked computes: the fp32 / fp16-eps DDIM update, then
    ``z = where(m, z_new, a*src + b*noise)``, ``z0t = where(m, z0t, src)`` (two products, one sum, each rounded to fp32)"""
    zn, z0 = z.clone(), torch.empty_like(z)
    emulate_step_ddim(zn, z0, eps_uc, eps_c, lam, coeffs, tweedie_uc, renoise_uc)
    m = mask.reshape(z.shape[0], 1, z.shape[2], z.shape[3]).bool()
    s = src.float()
    proper = float(a) * s + float(b) * noise.float()
    z0t_out.copy_(torch.where(m, z0, s))
    z.copy_(torch.where(m, zn, proper))


class InpaintMockEngine(MockEngine):
    """``unet_fn`` receives ``cat([z, z])`` with the image condition appended along the channels once one is set
    (the 9-channel input of an inpaint UNet: latent, mask, masked-image latent)."""

    def __init__(self, unet_fn, latent_hw=(8, 8)):
        super().__init__(unet_fn, latent_hw)
        self.cond = None
        self.conds = []

    def image_condition(self, cond):
        self.cond = cond.clone()
        self.conds.append(self.cond)

    def predict(self, z, t):
        if self.cond is None:
            return super().predict(z, t)
        cond = self.cond.to(z.dtype).expand(z.shape[0], -1, -1, -1)
        zz = torch.cat([torch.cat([z, z], 0), torch.cat([cond, cond], 0)], 1)
        eps = self.unet_fn(zz, float(t), self.ehs, self.te, self.ti)
        self.calls.append(dict(t=float(t), z=z.clone(), eps=eps.clone(), z_dtype=z.dtype))
        return eps[: self.B].contiguous(), eps[self.B:].contiguous()

    step_ddim_masked = staticmethod(emulate_step_ddim_masked)
