"""fp64 references of FreeU (diffusers utils.torch_utils.apply_freeu / fourier_filter, threshold = 1) and the UNet oracle with
FreeU applied.  Two statements of the skip filter: a literal restatement of ``fourier_filter`` (fftn, fftshift, mask, ifftshift,
ifftn, .real) and the closed form the kernel evaluates (tests/test_freeu_cpu.py asserts they agree)."""
from __future__ import annotations

import numpy as np
import torch

from oracle.unet_ref import UNetRef


def fourier_filter_np(x, s, axes=(-2, -1)):
    """diffusers ``fourier_filter(x_in, threshold=1, scale=s)`` on the two spatial axes ``axes`` of a float64 array"""
    x = np.asarray(x, dtype=np.float64)
    f = np.fft.fftshift(np.fft.fftn(x, axes=axes), axes=axes)
    H, W = x.shape[axes[0]], x.shape[axes[1]]
    mask = np.ones(x.shape, dtype=np.float64)
    crow, ccol = H // 2, W // 2
    idx = [slice(None)] * x.ndim
    idx[axes[0] % x.ndim] = slice(crow - 1, crow + 1)
    idx[axes[1] % x.ndim] = slice(ccol - 1, ccol + 1)
    mask[tuple(idx)] = s
    f = np.fft.ifftshift(f * mask, axes=axes)
    return np.fft.ifftn(f, axes=axes).real


def closed_form_np(x, s):
    """the same filter without an FFT, x [..., H, W] float64: four complex sums per plane (seven real ones) and
    out = v + (s - 1) / (H W) * (A + Re(B e^{-i ty}) + Re(C e^{-i tx}) + Re(D e^{-i (ty + tx)}))"""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    ty = 2.0 * np.pi * np.arange(H) / H
    tx = 2.0 * np.pi * np.arange(W) / W
    ey, ex = np.exp(1j * ty)[:, None], np.exp(1j * tx)[None, :]
    A = x.sum((-2, -1), keepdims=True)
    B = (x * ey).sum((-2, -1), keepdims=True)
    C = (x * ex).sum((-2, -1), keepdims=True)
    D = (x * ey * ex).sum((-2, -1), keepdims=True)
    low = A + (B * np.conj(ey)).real + (C * np.conj(ex)).real + (D * np.conj(ey * ex)).real
    return x + (s - 1.0) / (H * W) * low


def freeu_ref64(hidden, skip, b, s):
    """the op on interior NHWC arrays [rows, H, W, C] (fp16 values as float64); b, s as the fp32 values the ABI carries.
    -> (hidden64 | None, skip64 | None), unrounded"""
    b64, s64 = float(np.float32(b)), float(np.float32(s))
    h = k = None
    if hidden is not None:
        h = np.array(hidden, dtype=np.float64)
        h[..., : h.shape[-1] // 2] *= b64
    if skip is not None:
        k = np.moveaxis(closed_form_np(np.moveaxis(np.asarray(skip, dtype=np.float64), -1, 1), s64), 1, -1)
    return h, k


def fourier_filter_t(x, s):
    """``fourier_filter`` in torch fp32 on NCHW (what diffusers runs for sizes that are no power of two)"""
    x = x.float()
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    H, W = x.shape[-2:]
    mask = torch.ones_like(x)
    mask[..., H // 2 - 1: H // 2 + 1, W // 2 - 1: W // 2 + 1] = s
    return torch.fft.ifftn(torch.fft.ifftshift(f * mask, dim=(-2, -1)), dim=(-2, -1)).real


class FreeUUNetRef(UNetRef):
    """UNetRef with diffusers' FreeU: in up_blocks.0 (b1, s1) and up_blocks.1 (b2, s2), before every resnet, the concatenated
    input is split at the hidden / skip boundary the config gives, hidden[:, :C_h // 2] *= b, skip = fourier_filter(skip, 1, s)"""

    def __init__(self, cfg, sd, freeu, round_io: bool = True):
        super().__init__(cfg, sd, round_io)
        self.freeu = None if freeu is None else tuple(float(np.float32(v)) for v in freeu)      # (s1, s2, b1, b2) as the ABI's fp32

    def _resnet(self, p, x, emb):
        if self.freeu is not None and (p.startswith("up_blocks.0.resnets.") or p.startswith("up_blocks.1.resnets.")):
            i, j = int(p.split(".")[1]), int(p.split(".")[3])
            cfg = self.cfg
            L = cfg.num_levels
            co = cfg.block_out_channels[L - 1 - i]
            prev = cfg.block_out_channels[L - 1] if i == 0 else cfg.block_out_channels[L - i]
            c_h = prev if j == 0 else co
            s, b = self.freeu[i], self.freeu[2 + i]
            hidden, skip = x[:, :c_h].clone(), x[:, c_h:]
            hidden[:, : c_h // 2] = hidden[:, : c_h // 2] * b
            x = torch.cat([hidden, fourier_filter_t(skip, s)], dim=1)
        return super()._resnet(p, x, emb)
