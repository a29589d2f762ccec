"""The fp32 CPU oracle of soft regional prompts: oracle.unet_ref.UNetRef with, for attn2 only, the per-pixel BLEND - the query at
pixel p answers with sum_r w_r(p) softmax(q K_r) V_r over the context chunks [77 r, 77 r + 77).  The weights of a level are derived
from the token count N of the call as tests/region_ref.py derives its maps: the nearest downsample w_l[r, y, x] = w_0[r, y f, x f].
Everything else is the parent's.

``fault`` makes the three mistakes an engine can make with the weights, for the loudness check of tests/test_regions_soft_cpu.py:
  swapped         the weights of regions 0 and 1 exchanged
  shifted         the weights shifted by one pixel along x
  no_downsample   the level-0 weights read without their stride at the deeper levels

Shared inputs of the engine tests and the CPU stand-in for ``HipEngine`` with region weights live here too."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import region_ref as RR
from mock_region_engine import RegionMockEngine
from oracle.unet_ref import UNetRef

TOK = RR.TOK
HW = RR.HW


class SoftRegionUNetRef(UNetRef):
    def __init__(self, cfg, sd, w=None, fault=None):
        super().__init__(cfg, sd)
        self.set_region_weights(w, fault)

    def set_region_weights(self, w, fault=None):
        self.w = None if w is None else torch.as_tensor(w).float().reshape(-1, *torch.as_tensor(w).shape[-3:])
        self.fault = fault
        return self

    def level_weights(self, N):
        """[map rows, R, H0 / f, W0 / f]"""
        w = self.w
        H0, W0 = w.shape[-2:]
        f = int(math.isqrt(H0 * W0 // N))
        assert f >= 1 and H0 % f == 0 and W0 % f == 0 and (H0 // f) * (W0 // f) == N
        if self.fault == "swapped":
            w = w[:, [1, 0] + list(range(2, w.shape[1]))]
        if self.fault == "shifted":
            w = torch.roll(w, 1, dims=-1)
        return w[..., :H0 // f, :W0 // f] if self.fault == "no_downsample" else w[..., ::f, ::f]

    def _attn(self, p, x, ctx, heads):
        if self.w is None or not p.endswith(".attn2"):
            return super()._attn(p, x, ctx, heads)
        q = self._lin(p + ".to_q", x)
        k = self._lin(p + ".to_k", ctx)
        v = self._lin(p + ".to_v", ctx)
        B, N, Cc = q.shape
        R = self.w.shape[1]
        assert ctx.shape[1] == TOK * R
        d = Cc // heads
        q = q.view(B, N, heads, d).transpose(1, 2)
        k = k.view(B, -1, heads, d).transpose(1, 2)
        v = v.view(B, -1, heads, d).transpose(1, 2)
        w = self.level_weights(N).reshape(-1, R, N).expand(B, R, N)
        o = torch.zeros_like(q)
        for r in range(R):
            o_r = F.scaled_dot_product_attention(q, k[:, :, TOK * r: TOK * (r + 1)], v[:, :, TOK * r: TOK * (r + 1)])
            o = o + w[:, r][:, None, :, None] * o_r
        o = o.transpose(1, 2).reshape(B, N, Cc)
        return self._lin(p + ".to_out.0", o)


# ---- shared inputs -------------------------------------------------------------------------------------------------------------
def configs():
    """the three nets of region_ref.configs() (cross-attention head dims 64, 32, 40) and a two-level net whose cross-attention head
    dims are 80 and 160 - SD1.5's deeper levels, dp = 96 and 160"""
    from cfgpp_amd.unet_config import UNetConfig
    d80 = UNetConfig(name="tiny_d80_d160", block_out_channels=(320, 640), level_has_attn=(1, 1), transformer_depth=(1, 1), num_heads=(4, 4),
                     cross_attention_dim=64, sample_size=16)
    return {**RR.configs(), "tiny_d80_d160": (d80, 2)}


NETS = RR.NETS + ("tiny_d80_d160",)


def region_weights(kind, n_regions, rows=1, hw=HW, seed=7):
    """float32 [rows, R, h, w] summing to 1 per pixel: "onehot" (the stripes of region_ref.region_ids), "feather" (stripes with linear
    ramps four pixels wide), "mixed" (random, every region everywhere); rows > 1: row b's map is rolled by 3 b pixels"""
    h, w = (hw, hw) if isinstance(hw, int) else hw
    if kind == "onehot":
        out = F.one_hot(RR.region_ids("stripes", n_regions, 1, hw)[0], n_regions).permute(2, 0, 1).float()
    elif kind == "feather":
        x = ((torch.arange(w, dtype=torch.float32) + 0.5) / w * n_regions - 0.5).clamp(0, n_regions - 1)    # region r is centred on x = r
        out = torch.stack([(1.0 - (x - r).abs()).clamp(min=0.0) for r in range(n_regions)])             # hats: a partition of unity
        out = (out / out.sum(0, keepdim=True))[:, None, :].expand(n_regions, h, w).contiguous()
    elif kind == "mixed":
        out = torch.rand((n_regions, h, w), generator=torch.Generator().manual_seed(seed)) + 0.05
        out = out / out.sum(0, keepdim=True)
    else:
        raise ValueError(kind)
    return torch.stack([torch.roll(out, 3 * b, dims=2) for b in range(rows)]).float()


# ---- the CPU stand-in for HipEngine with region weights -----------------------------------------------------------------------
class WeightCalls:
    """mixin for any mock engine (tests/lcm_mock.py, tests/sde_mock.py, ..) next to mock_region_engine.RegionCalls: records
    ``set_region_weights``"""

    def set_region_weights(self, w):
        self.__dict__.setdefault("order", []).append("weights")
        self.__dict__.setdefault("weight_calls", []).append(None if w is None else torch.as_tensor(w).clone())
        self._regions = 0 if w is None else int(torch.as_tensor(w).shape[1])
        return self


class SoftRegionMockEngine(RegionMockEngine):
    """records ``set_region_weights`` next to ``set_regions`` / ``set_context``; with a state dict the UNet is the oracle above (region
    weights set) or that of tests/region_ref.py (a hard map set)"""

    def __init__(self, cfg=None, sd=None, latent_hw=(8, 8)):
        super().__init__(cfg, sd, latent_hw)
        self.soft_ref = SoftRegionUNetRef(cfg, sd) if cfg is not None else None
        self.weight_calls = []          # w or None, in call order
        self._w = None

    def set_regions(self, ids, n_regions=0):
        if ids is None and self._w is not None:
            return self.set_region_weights(None)
        self._w = None
        return super().set_regions(ids, n_regions)

    def set_region_weights(self, w):
        self.order.append("weights")
        self.weight_calls.append(None if w is None else torch.as_tensor(w).clone())
        self._w = None if w is None else torch.as_tensor(w).float()
        self._ids = None
        self._regions = 0 if w is None else int(self._w.shape[1])
        return self

    def _unet(self, z, t, ehs, te, ti):
        if self.soft_ref is None or self._w is None:
            return super()._unet(z, t, ehs, te, ti)
        w = self._w
        if w.shape[0] > 1:
            w = torch.cat([w, w], 0)                        # rows [uc_1..uc_B, c_1..c_B]: both halves use the same weights
        self.soft_ref.set_region_weights(w)
        ack = None if te is None else {"text_embeds": te.float(), "time_ids": ti.float()}
        return self.soft_ref(z.float(), t, ehs.float(), ack)["sample"].half()
