"""``MockEngine`` (tests/mock_engine.py) plus the panorama entry points of include/cfgpp_panorama.h, emulated at the kernels' INTERFACE
with the slice model of tests/pano_ref.py: the CPU stand-in the panorama solvers run on in tests."""
from __future__ import annotations

import torch

import pano_ref as R
from mock_engine import MockEngine


def case_of(g):
    return (g.Hp, g.Wp, g.h, g.w, g.stride, int(bool(g.circular)))


class PanoMockEngine(MockEngine):
    def __init__(self, unet_fn, latent_hw=(8, 8)):
        super().__init__(unet_fn, latent_hw)
        self.pcalls = []            # (name, details) of every panorama entry point, in call order

    def predict_into(self, z_chunk, t, eps_chunk):
        assert tuple(eps_chunk.shape) == (2 * self.B, 4, self.H, self.W) and eps_chunk.dtype == torch.float16
        assert int(z_chunk.shape[0]) == self.B and z_chunk.is_contiguous() and eps_chunk.is_contiguous()
        eps = self.unet_fn(torch.cat([z_chunk, z_chunk], 0), float(t), self.ehs, self.te, self.ti)
        self.calls.append(dict(t=float(t), z=z_chunk.clone(), eps=eps.clone(), z_dtype=z_chunk.dtype))
        self.pcalls.append(("predict_into", dict(t=float(t), rows=int(z_chunk.shape[0]))))
        eps_chunk.copy_(eps)

    def gather_views(self, g, z_pano, z_views):
        self.pcalls.append(("gather_views", dict(chunk=g.chunk_views)))
        R.gather(case_of(g), z_pano, int(z_pano.shape[0]), out=z_views)

    def step_ddim_views(self, g, z_pano, z0t_pano, z_views, eps, lam, coeffs, tweedie_uc, renoise_uc):
        B = int(z_pano.shape[0])
        assert tuple(eps.shape) == (g.n_views // g.chunk_views, 2 * g.chunk_views * B, 4, g.h, g.w)
        self.pcalls.append(("step_ddim_views", dict(chunk=g.chunk_views, lam=float(lam), coeffs=tuple(float(c) for c in coeffs),
                                                    tweedie_uc=bool(tweedie_uc), renoise_uc=bool(renoise_uc))))
        z, z0 = R.step(case_of(g), z_pano, z_views, eps, B, g.chunk_views, lam, coeffs, tweedie_uc, renoise_uc)
        z_pano.copy_(z)
        z0t_pano.copy_(z0)
