"""``VPredMockEngine`` (tests/vpred_mock.py) plus the LCM entry points of include/cfgpp_lcm.h, emulated at the kernels' INTERFACE with
the model of tests/lcm_ref.py: fp32 coefficients in, explicit roundings, the Philox normals of the float64 model rounded to fp32 - so
the solvers' plumbing (cfgpp_amd/lcm.py: timesteps, coefficients, seeds, draw indices, the ``last`` flag) is what the CPU tests
exercise.  Tests only; the product never constructs it."""
from __future__ import annotations

import numpy as np
import torch

import lcm_ref as R
from vpred_mock import VPredMockEngine


def emulate_philox_normal(out, seeds, draw, stream_id):
    B = int(out.shape[0])
    n = torch.from_numpy(R.normal_rows(B, out.numel() // B, seeds, draw, stream_id).astype(np.float32)).reshape(out.shape)
    out.copy_(n.to(out.dtype))
    return out


class LCMMockEngine(VPredMockEngine):
    """records the LCM launches in ``lcalls``: ("step_lcm", dict) / ("philox_normal", dict) / ("guidance_embedding", values)"""

    def __init__(self, unet_fn, latent_hw=(8, 8), time_cond_proj_dim=0):
        super().__init__(unet_fn, latent_hw)
        self.time_cond_proj_dim = int(time_cond_proj_dim)
        self.lcalls = []

    def set_guidance_embedding(self, w_emb):
        self.lcalls.append(("guidance_embedding", [float(v) for v in w_emb]))

    def philox_normal(self, out, seeds, draw, stream_id):
        self.lcalls.append(("philox_normal", dict(seeds=list(seeds), draw=int(draw), stream_id=int(stream_id), dtype=out.dtype)))
        return emulate_philox_normal(out, seeds, draw, stream_id)

    def step_lcm(self, z, den_out, m_uc, m_c, lam, coef6, pred_v, last, seeds=None, draw=0, noise=None):
        self.lcalls.append(("step_lcm", dict(coef=tuple(float(v) for v in coef6), lam=float(lam), pred_v=bool(pred_v), last=bool(last),
                                             seeds=None if seeds is None else list(seeds), draw=int(draw), single=m_uc is m_c,
                                             noise_given=noise is not None)))
        if noise is None and not last:
            noise = emulate_philox_normal(torch.empty_like(z), seeds, draw, 0)
        den, zn = R.step_lcm(z, m_uc, m_c, lam, coef6, pred_v, last, noise)
        den_out.copy_(den)
        z.copy_(zn)
