"""CPU restatement of diffusers' IP-Adapter path - ``ImageProjection.forward`` (``unet.encoder_hid_proj``) and
``IPAdapterAttnProcessor2_0.__call__`` for one adapter - TEST INFRASTRUCTURE ONLY, on the primitives of ``oracle.unet_ref.UNetRef``
(fp32 torch ops; the image embeds rounded through fp16 as the fp16 engine's input is)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.unet_ref import UNetRef


class IPUNetRef(UNetRef):
    """``UNetRef`` whose ``.attn2`` adds ``scale * SDPA(q, to_k_ip(tokens), to_v_ip(tokens))`` before ``to_out``.
    ``adapter``: engine keys (cfgpp_amd.ip_adapter.parse_ip_adapter).  ``set_image(embeds [R, E] | None, scale)``."""

    def __init__(self, cfg, sd, adapter, round_io: bool = True):
        super().__init__(cfg, sd, round_io)
        self.ip = {k: v.float() for k, v in adapter.items()}
        self.ip_tokens, self.ip_scale = None, 0.0

    def image_tokens(self, embeds):
        e = embeds.float()
        if self.round_io:
            e = e.half().float()
        cross = self.cfg.cross_attention_dim
        x = F.linear(e, self.ip["image_proj.proj.weight"], self.ip["image_proj.proj.bias"]).reshape(e.shape[0], -1, cross)
        return F.layer_norm(x, (cross,), self.ip["image_proj.norm.weight"], self.ip["image_proj.norm.bias"], 1e-5)

    def set_image(self, embeds, scale=1.0):
        self.ip_tokens = None if embeds is None else self.image_tokens(embeds)
        self.ip_scale = float(scale)
        return self

    def _attn(self, p, x, ctx, heads):
        if not p.endswith(".attn2") or self.ip_tokens is None or self.ip_scale == 0.0:
            return super()._attn(p, x, ctx, heads)
        q = self._lin(p + ".to_q", x)
        B, N, Cc = q.shape
        d = Cc // heads

        def split(t):
            return t.view(B, -1, heads, d).transpose(1, 2)

        q = split(q)
        o = F.scaled_dot_product_attention(q, split(self._lin(p + ".to_k", ctx)), split(self._lin(p + ".to_v", ctx)))
        tok = self.ip_tokens
        ki = F.linear(tok, self.ip[p + ".to_k_ip.weight"])
        vi = F.linear(tok, self.ip[p + ".to_v_ip.weight"])
        o = o + self.ip_scale * F.scaled_dot_product_attention(q, split(ki), split(vi))
        return self._lin(p + ".to_out.0", o.transpose(1, 2).reshape(B, N, Cc))
