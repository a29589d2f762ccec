"""``LCMMockEngine`` (tests/lcm_mock.py) plus the two entry points of include/cfgpp_sde.h, emulated at the kernels' INTERFACE with the
model of tests/sde_ref.py: fp32 coefficients in, explicit roundings, the Philox normals of the float64 model (stream 2) rounded to
fp32 - so the solvers' plumbing (cfgpp_amd/sde.py: sigmas, coefficients, seeds, draw indices, the history ring, the ``last`` flag) is
what the CPU tests exercise.  Tests only; the product never constructs it."""
from __future__ import annotations

import torch

import sde_ref as S
from lcm_mock import LCMMockEngine


class SDEMockEngine(LCMMockEngine):
    """records the SDE launches in ``scalls``: ("sde_input", dict) / ("step_sde", dict); the dicts hold the buffers' identities
    (``id``s) so that a test can follow the history ring"""

    def __init__(self, unet_fn, latent_hw=(8, 8)):
        super().__init__(unet_fn, latent_hw)
        self.scalls = []

    def sde_input(self, x, xc_out, s_in):
        assert x.dtype == torch.float32 and xc_out.dtype == torch.float16
        self.scalls.append(("sde_input", dict(s_in=float(s_in), x=id(x), xc=id(xc_out))))
        xc_out.copy_((x * torch.tensor(float(s_in), dtype=torch.float32)).to(torch.float16))

    def step_sde(self, x, den_out, xc_out, hist1, hist2, hist_out, m_uc, m_c, lam, coef8, cfgpp, n_hist, last, seeds=None, draw=0,
                 noise=None):
        ident = lambda t: None if t is None else id(t)  # noqa: E731
        self.scalls.append(("step_sde", dict(coef=tuple(float(v) for v in coef8), lam=float(lam), cfgpp=bool(cfgpp), n_hist=int(n_hist),
                                             last=bool(last), seeds=None if seeds is None else list(seeds), draw=int(draw),
                                             single=m_uc is m_c, noise_given=noise is not None, x=id(x), xc_out=ident(xc_out),
                                             hist1=ident(hist1), hist2=ident(hist2), hist_out=ident(hist_out))))
        assert (n_hist < 1 or hist1 is not None) and (n_hist < 2 or hist2 is not None)
        if noise is None and not last and float(coef8[6]) != 0.0:
            B = int(x.shape[0])
            noise = S.noise_rows(B, x.numel() // B, seeds, draw, x.shape)
        den, keep, xn, xc = S.step_sde(x, hist1, hist2, m_uc, m_c, lam, coef8, cfgpp, n_hist, last, noise)
        den_out.copy_(den)
        x.copy_(xn)
        if hist_out is not None:
            hist_out.copy_(keep)
        if xc_out is not None:
            xc_out.copy_(xc)
