"""CPU restatement of the IP-Adapter "plus" image projection - the published ``Resampler`` (``PerceiverAttention`` +
``FeedForward`` layers over learned latents) as ``unet.encoder_hid_proj`` - TEST INFRASTRUCTURE ONLY, on top of
``tests/ip_adapter_ref.IPUNetRef`` (whose decoupled cross-attention it keeps).  fp32 torch ops, an fp64 switch, and a third mode
that keeps fp16 wherever the HIP executor stores an activation (the E_model of tests/test_gpu_ip_plus.py).  The hidden states are
rounded through fp16 as the fp16 engine's input is."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ip_adapter_ref import IPUNetRef

DIM_HEAD = 64
LOG2E_F32 = 1.4426950408889634


def resampler_depth(ip) -> int:
    return len({k.split(".")[2] for k in ip if k.startswith("image_proj.layers.")})


def resampler_tokens(ip, hidden, dtype=torch.float32, storage16=False):
    """tokens [R, n_q, cross] of hidden [R, S, E].  ``ip``: engine keys (image_proj.*) -> tensors.  ``storage16``: every tensor the
    executor writes to memory (GEMM, LayerNorm, attention and GELU outputs; the softmax's P) is rounded to fp16, arithmetic in
    ``dtype`` - the rounding points of csrc/unet.hip cfgpp_unet_image_context_seq and csrc/resampler.hip, nothing else."""
    W = {k[len("image_proj."):]: v.to(dtype) for k, v in ip.items() if k.startswith("image_proj.")}
    r = (lambda t: t.half().to(dtype)) if storage16 else (lambda t: t)
    ln = lambda t, p: r(F.layer_norm(t, (t.shape[-1],), W[p + ".weight"], W[p + ".bias"], 1e-5))       # noqa: E731
    x = r(F.linear(hidden.to(dtype), W["proj_in.weight"], W["proj_in.bias"]))
    R = x.shape[0]
    lat = r(W["latents"].reshape(1, -1, W["latents"].shape[-1]).expand(R, -1, -1))
    for i in range(resampler_depth(ip)):
        p = f"layers.{i}."
        xn, l2 = ln(x, p + "0.norm1"), ln(lat, p + "0.norm2")
        q = r(F.linear(l2, W[p + "0.to_q.weight"]))
        kv = torch.cat([r(F.linear(xn, W[p + "0.to_kv.weight"])), r(F.linear(l2, W[p + "0.to_kv.weight"]))], 1)
        k, v = kv.chunk(2, -1)
        H = q.shape[-1] // DIM_HEAD
        split = lambda t: t.reshape(R, t.shape[1], H, DIM_HEAD).transpose(1, 2)                      # noqa: E731
        qh, kh, vh = split(q), split(k), split(v)
        if storage16:       # the kernel: scores * fp32(1/8 * log2 e), P = exp2(s - max) in fp16, denominator from the rounded P
            sc = float(torch.tensor(0.125, dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32))
            s = (qh @ kh.transpose(-1, -2)) * sc
            pr = r(torch.exp2(s - s.max(-1, keepdim=True).values))
            o = r((pr @ vh) / pr.sum(-1, keepdim=True))
        else:               # the published form: (q * 64^-1/4) (k * 64^-1/4)^T
            s = (qh * DIM_HEAD ** -0.25) @ (kh * DIM_HEAD ** -0.25).transpose(-1, -2)
            o = torch.softmax(s, -1) @ vh
        o = o.transpose(1, 2).reshape(R, -1, H * DIM_HEAD)
        lat = r(F.linear(o, W[p + "0.to_out.weight"]) + lat)
        h = r(F.linear(ln(lat, p + "1.0"), W[p + "1.1.weight"]))
        h = r(h * 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0))))          # nn.GELU(), the erf form
        lat = r(F.linear(h, W[p + "1.3.weight"]) + lat)
    out = r(F.linear(lat, W["proj_out.weight"], W["proj_out.bias"]))
    return r(F.layer_norm(out, (out.shape[-1],), W["norm_out.weight"], W["norm_out.bias"], 1e-5))


class IPPlusUNetRef(IPUNetRef):
    """``IPUNetRef`` whose image tokens come from the Resampler: ``set_image(hidden [R, S, E] | None, scale)``.  ``fp64``: the
    Resampler in double precision (the tokens are handed on in fp32)."""

    def __init__(self, cfg, sd, adapter, round_io: bool = True, fp64: bool = False):
        super().__init__(cfg, sd, adapter, round_io)
        self.fp64 = fp64

    def image_tokens(self, hidden, fp64=None):
        h = hidden.float()
        if self.round_io:
            h = h.half().float()
        if self.fp64 if fp64 is None else fp64:
            return resampler_tokens(self.ip, h, torch.float64).float()
        return resampler_tokens(self.ip, h, torch.float32)
