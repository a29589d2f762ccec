"""The fp32 CPU oracle of regional prompts: oracle.unet_ref.UNetRef with, for attn2 only, the per-pixel selection - the query at
pixel p of region r attends to the context tokens [77 r, 77 r + 77) alone.  The map of a level is derived from the token count N of
the call: f = sqrt(H0 W0 / N), the level is H0 / f x W0 / f (the latent need not be square), the nearest downsample
id_l[y, x] = id_0[y * f, x * f] (F.interpolate(mode="nearest") for these integer factors).  Everything else is the parent's.

``fault`` makes the three mistakes an engine can make with the map, for the loudness check of tests/test_gpu_regions_net.py:
  swapped         regions 0 and 1 exchanged
  shifted         the map shifted by one pixel along x
  no_downsample   the level-0 map read without its stride at the deeper levels (id_l[y, x] = id_0[y, x])

Shared inputs of the engine tests live here too: the nets, the loud region contexts and the maps."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle.unet_ref import UNetRef

TOK = 77
HW = 16
# standard deviation of region r's context chunk: neighbours differ by a factor of 4 or more, so a misplaced region moves the output
# far more than the engine's tolerance (the three figures of profiles/regional/README.md).  Not louder than 2.0: a chunk drawn at
# 4.0 (four times a CLIP hidden state's spread) makes the cross-attention logits so large that the softmax is one-hot and the
# documented fp16 rounding of the pre-scaled q moves whole rows - measured on the MI355X with (0.25, 2.0, 0.5, 4.0): R = 4 forwards at
# rel-L2 1.4e-3 .. 3.9e-3 on all three nets (kernel 7 and the independent kernel 8 alike) against 1.0e-3 .. 1.3e-3 at R = 2, 3.
REGION_SCALE = (0.25, 2.0, 0.5, 2.0)


class RegionUNetRef(UNetRef):
    def __init__(self, cfg, sd, ids=None, n_regions=0, fault=None):
        super().__init__(cfg, sd)
        self.set_regions(ids, n_regions, fault)

    def set_regions(self, ids, n_regions, fault=None):
        self.ids = None if ids is None else torch.as_tensor(ids).long().reshape(-1, *torch.as_tensor(ids).shape[-2:])
        self.n_regions, self.fault = int(n_regions), fault
        return self

    def level_ids(self, N):
        """the map of the level with N tokens, [map rows, H0 / f, W0 / f]"""
        ids = self.ids
        H0, W0 = ids.shape[-2:]
        f = int(math.isqrt(H0 * W0 // N))
        assert f >= 1 and H0 % f == 0 and W0 % f == 0 and (H0 // f) * (W0 // f) == N
        if self.fault == "swapped":
            ids = torch.where(ids == 0, 1, torch.where(ids == 1, 0, ids))
        if self.fault == "shifted":
            ids = torch.roll(ids, 1, dims=-1)
        return ids[:, :H0 // f, :W0 // f] if self.fault == "no_downsample" else ids[:, ::f, ::f]

    def level_map(self, B, N):
        return self.level_ids(N).reshape(-1, N).expand(B, N)

    def _attn(self, p, x, ctx, heads):
        if self.ids is None or not p.endswith(".attn2"):
            return super()._attn(p, x, ctx, heads)
        q = self._lin(p + ".to_q", x)
        k = self._lin(p + ".to_k", ctx)
        v = self._lin(p + ".to_v", ctx)
        B, N, Cc = q.shape
        assert ctx.shape[1] == TOK * self.n_regions
        d = Cc // heads
        q = q.view(B, N, heads, d).transpose(1, 2)
        k = k.view(B, -1, heads, d).transpose(1, 2)
        v = v.view(B, -1, heads, d).transpose(1, 2)
        m = self.level_map(B, N)
        o = torch.zeros_like(q)
        for r in range(self.n_regions):
            o_r = F.scaled_dot_product_attention(q, k[:, :, TOK * r: TOK * (r + 1)], v[:, :, TOK * r: TOK * (r + 1)])
            o = torch.where((m == r)[:, None, :, None], o_r, o)
        o = o.transpose(1, 2).reshape(B, N, Cc)
        return self._lin(p + ".to_out.0", o)


# ---- shared inputs -------------------------------------------------------------------------------------------------------------
def configs():
    """the nets of tests/test_gpu_long_prompt.py: cross-attention head dims 64 (kernel 7, fp32 denominator), 32 (kernel 8) and 40
    (kernel 7 with the ones row of V^T)"""
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL, UNetConfig
    d40 = UNetConfig(name="tiny_d40", block_out_channels=(320, 320), level_has_attn=(1, 1), transformer_depth=(1, 1), num_heads=(8, 8),
                     cross_attention_dim=64, sample_size=16)
    return {"tiny_xl": (TINY_XL, 2), "tiny_sd": (TINY_SD, 4), "tiny_d40": (d40, 2)}


NETS = ("tiny_xl", "tiny_sd", "tiny_d40")


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).half().float()


def region_context(rows, n_regions, dim, seed=81):
    """[rows, 77 R, dim]: region r's chunk drawn with standard deviation REGION_SCALE[r]"""
    return torch.cat([rnd(rows, TOK, dim, seed=seed + r, scale=REGION_SCALE[r]) for r in range(n_regions)], 1)


def region_ids(kind, n_regions, rows=1, hw=HW):
    """left/right stripes or a checkerboard of n_regions ids -> int64 [rows, h, w] (``hw``: one side, or a pair (h, w)); rows > 1: row
    b's map is rolled by 3 b pixels"""
    h, w = (hw, hw) if isinstance(hw, int) else hw
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if kind == "stripes":
        m = (x * n_regions // w).clamp(max=n_regions - 1)
    elif kind == "checker":
        m = (x + y) % n_regions
    else:
        raise ValueError(kind)
    return torch.stack([torch.roll(m, 3 * b, dims=1) for b in range(rows)])
