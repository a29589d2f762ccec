"""``SDEMockEngine`` (tests/sde_mock.py) plus the entry point of include/cfgpp_dpmpp_sde.h, emulated at the kernel's INTERFACE with the
model of tests/dpmpp_sde_ref.py: fp32 coefficients in, explicit roundings, the Philox normals of the float64 model (stream 3) rounded
to fp32 - so the solvers' plumbing (cfgpp_amd/dpmpp_sde.py: sigmas, rows, seeds, draw indices, the buffers, the ``last`` flag) is what
the CPU tests exercise.  Tests only; the product never constructs it."""
from __future__ import annotations

import torch

import dpmpp_sde_ref as S
from sde_mock import SDEMockEngine


class DPMppSDEMockEngine(SDEMockEngine):
    """records the stage launches in ``scalls`` next to SDEMockEngine's: ("step_sde_stage", dict); the dicts hold the buffers'
    identities (``id``s) so that a test can follow them"""

    def step_sde_stage(self, x, base, out, den_out, xc_out, m_uc, m_c, lam, coef7, terms, last, seeds=None, draw1=0, draw2=1,
                       noise1=None, noise2=None):
        assert all(t.dtype == torch.float32 for t in (x, base, out, den_out)) and m_uc.dtype == torch.float16 == m_c.dtype
        assert (out is not base or base is x) and den_out is not x and den_out is not out
        self.scalls.append(("step_sde_stage", dict(coef=tuple(float(v) for v in coef7), terms=int(terms), last=bool(last), lam=float(lam),
                                                   seeds=None if seeds is None else list(seeds), draw1=int(draw1), draw2=int(draw2),
                                                   single=m_uc is m_c, noise_given=noise1 is not None or noise2 is not None,
                                                   x=id(x), base=id(base), out=id(out), den_out=id(den_out),
                                                   xc_out=None if xc_out is None else id(xc_out))))
        B = int(x.shape[0])
        if noise1 is None and not last and terms & S.TERM_N1:
            noise1 = S.noise_rows(B, x.numel() // B, seeds, draw1, x.shape)
        if noise2 is None and not last and terms & S.TERM_N2:
            noise2 = S.noise_rows(B, x.numel() // B, seeds, draw2, x.shape)
        den, o, xc = S.stage(x, base, m_uc, m_c, lam, coef7, terms, last, noise1, noise2)
        den_out.copy_(den)
        out.copy_(o)
        if xc_out is not None:
            xc_out.copy_(xc)
