"""``DPMppSDEMockEngine`` (tests/dpmpp_sde_mock.py: the DDIM, k-diffusion, v-prediction, LCM and SDE entry points) plus the entry point
of include/cfgpp_img2img.h, emulated at the kernel's INTERFACE with the fp32 restatement of tests/img2img_ref.py - fp32 coefficients in,
one rounding per operation, the Philox normals of the float64 model (stream 4, draw 0) rounded to fp32 - so the solvers' plumbing
(cfgpp_amd/img2img.py: the source, the strength rule, (a, s), the mode, the seeds) is what the CPU tests exercise.  Tests only; the
product never constructs it."""
from __future__ import annotations

import numpy as np
import torch

import img2img_ref as M
from dpmpp_sde_mock import DPMppSDEMockEngine


def emulate_img2img_start(x, src, a, s, mode="identity", noise=None, seeds=None):
    B, C, h, w = (int(v) for v in x.shape)
    mode = M.MODES[mode] if isinstance(mode, str) else int(mode)
    a32, s32 = float(np.float32(a)), float(np.float32(s))
    assert a32 != 0.0 or s32 != 0.0
    if a32 != 0.0:
        assert src.dtype in (torch.float16, torch.float32) and int(src.shape[0]) in (1, B) and int(src.shape[1]) == C
        assert int(src.shape[2]) <= h and int(src.shape[3]) <= w and (mode != 0 or tuple(src.shape[2:]) == (h, w))
    if s32 != 0.0:
        assert (noise is not None and noise.dtype == torch.float32 and noise.shape == x.shape) or (seeds is not None and len(seeds) == B)
    got, _ = M.start(None if a32 == 0.0 else src.double().numpy(), None if noise is None else noise.numpy(), a32, s32, B, h, w, mode,
                     x.dtype == torch.float16, np.float32, seeds=seeds, C=C)
    x.copy_(torch.from_numpy(got).to(x.dtype))
    return x


class Img2ImgMockEngine(DPMppSDEMockEngine):
    """records the start launches in ``icalls``: dicts of what cfgpp_img2img_start was given"""

    def __init__(self, unet_fn, latent_hw=(8, 8)):
        super().__init__(unet_fn, latent_hw)
        self.icalls = []

    def img2img_start(self, x, src, a, s, mode="identity", noise=None, seeds=None):
        self.icalls.append(dict(a=float(a), s=float(s), mode=mode, x_dtype=x.dtype, shape=tuple(x.shape),
                                src=None if src is None else src.clone(), noise_given=noise is not None,
                                seeds=None if seeds is None else list(seeds)))
        out = emulate_img2img_start(x, src, a, s, mode, noise, seeds)
        self.icalls[-1]["x"] = out.clone()
        return out
