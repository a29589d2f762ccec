"""CPU stand-in for the ControlNet half of ``HipEngine`` (tests only): ``MockEngine`` plus ``build_controlnet`` /
``set_control`` / ``clear_control``.  Every set_control / clear_control call is recorded; with a control set, ``predict`` asks
``controlled_fn`` (CPU restatement: tests/controlnet_ref.py) instead of ``unet_fn``."""
from __future__ import annotations

import torch

from mock_engine import MockEngine


class ControlMockEngine(MockEngine):
    """``controlled_fn(z_rows, t, ehs, te, ti, cn, image_rows, scale) -> eps``; ``image_rows`` holds one image row per UNet row"""

    def __init__(self, unet_fn, controlled_fn=None, latent_hw=(8, 8), make_controlnet=None):
        super().__init__(unet_fn, latent_hw)
        self.controlled_fn = controlled_fn
        self.make_controlnet = make_controlnet
        self.control = None
        self.control_calls = []

    def build_controlnet(self, spec, seed=0):
        self.control_calls.append(("build", spec, seed))
        return self.make_controlnet(spec, seed) if self.make_controlnet else ("controlnet", spec, seed)

    def set_control(self, cn, image, scale=1.0):
        self.control_calls.append(("set", tuple(image.shape), float(scale)))
        self.control = (cn, image.clone(), float(scale))

    def clear_control(self):
        self.control_calls.append(("clear",))
        self.control = None

    def predict(self, z, t):
        if self.control is None:
            return super().predict(z, t)
        cn, image, scale = self.control
        zz = torch.cat([z, z], 0)
        R = zz.shape[0]
        rows = image[(torch.arange(R) % self.B) % image.shape[0]]
        eps = self.controlled_fn(zz, float(t), self.ehs, self.te, self.ti, cn, rows, scale)
        self.calls.append(dict(t=float(t), z=z.clone(), eps=eps.clone(), z_dtype=z.dtype, control=True))
        return eps[: self.B].contiguous(), eps[self.B:].contiguous()
