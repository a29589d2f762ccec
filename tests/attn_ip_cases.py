"""Inputs, references and the error bound of the decoupled cross-attention tests (IP-Adapter; plain torch, no HIP).

Shared by tests/test_ip_adapter_cpu.py (the bound sees the faults it is meant to see) and tests/test_gpu_attention_ip.py
(cfgpp_op_attention_ip of cfgpp_amd/csrc/attn_kernel.hip against the same references).  Builds on tests/attn_cases.py: the text
half of every case IS an attn_cases.Case (same generator, same planted rows / keys), the metric is attn_cases.max_row_err and the
bound of a case is attn_cases.FACTOR x E_model, E_model being the error of ``model_ip`` against ``ref_ip`` on the same inputs,
computed on the CPU by the test that uses it.

Layout contract under test: text keys in slots [0, nk_text), nk_text <= 96; image keys in slots [96, 96 + n_img), n_img <= 32; every
other slot of the 128 is a pad (zero K, zero V) that enters neither softmax.

Image inputs: keys 0.3 * randn - 6u (as the text keys of the ``neg`` kind: every real score strongly negative, so a pad that
enters a softmax with score 0 takes most of its mass), values 8 * sign(randn) with component 0 raised by the key's index + 1 and
component 1 by the (base) head's index % 7 - a wrong key, a wrong head or a wrong batch row moves the output by O(1) per element.

Reference: ``ref_ip`` = softmax(q K_t) V_t + scale * softmax(q K_i) V_i in fp64.
``model_ip``: fp64 arithmetic with the kernels' rounding points and nothing else - q * d^-1/2 * log2(e) rounded to fp16; per key group
its own maximum, P = exp2(s - max) rounded to fp16, the denominator summed from those rounded P; then
  fused (head dim padded to 64)  fp16( O_text + scale * O_img ), one rounding;
  two-pass (other head dims)     O_text rounded to fp16, then fp16( float(O_text) + scale * O_img ).

Kernel / E_model ratios on the MI355X ("attention_ip_case" lines of the parity file): see RATIOS below.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

import attn_cases as A
from attn_cases import FACTOR  # noqa: F401  (the bound's factor is attn_cases' own)

IMG_SLOT = 96                  # first key slot of the image tokens
MAX_IMG = 32

# Kernel / E_model ratios (max_row_err / e_model) measured on the MI355X (profiles/ip_adapter/parity_attention_ip.jsonl; the bound
# is FACTOR = 4): group -> (cases, min, median, max).  Most cases sit at 1.00; the spread (d = 64: 0.97 .. 1.03, d = 40 / 56:
# 0.98 .. 1.07) is fp32 accumulation in the MFMAs' order against the model's fp64.
RATIOS = dict(ip_fused_small=(120, 0.97, 1.00, 1.07), ip_fused_multiblock=(4, 1.00, 1.00, 1.00), ip_fused_remap=(1, 1.00, 1.00, 1.00),
              ip_two_pass=(6, 1.00, 1.01, 1.01))


@dataclass(frozen=True)
class IPCase:
    B: int
    h: int
    Nq: int
    nk_text: int
    n_img: int
    d: int
    scale: float = 1.0
    kind: str = "neg"
    planted: bool = True
    seed: int = 0
    kernel: int = 0            # expected dispatch: 4 xattn64_kernel IP form, 5 attn_ip_add_kernel after a text pass
    xqb: int = 0

    @property
    def id(self):
        return f"B{self.B}h{self.h}q{self.Nq}t{self.nk_text}i{self.n_img}d{self.d}-{self.kind}-s{self.scale:g}"

    @property
    def text(self) -> A.Case:
        return A.Case(self.B, self.h, self.Nq, self.nk_text, self.d, self.kind, planted=self.planted and self.Nq > 1, qscale=2.0,
                      seed=self.seed)

    @property
    def d16(self):
        return (self.d + 15) // 16

    @property
    def ones(self):
        return int(self.d % 32 != 0)

    @property
    def fused(self):
        return (self.d + 31) // 32 == 2

    @property
    def grid(self):
        nqb = (self.Nq + 127) // 128
        return self.B * self.h * (nqb // self.xqb if self.xqb else nqb)


def _seeded(cases, base):
    from dataclasses import replace
    return [replace(c, seed=base + i) for i, c in enumerate(cases)]


def _scale_of(i):
    return (0.6, 1.0)[i % 2]


# ---- GPU case tables: the smallest shapes that reach each branch ----------------------------------------------------------
# 1. the fused kernel: one workgroup per (head, query block), every mask position class of both softmaxes
FUSED_SMALL = _seeded([IPCase(1, 2, nq, nk, ni, d, scale=_scale_of(j), kernel=4, xqb=1)
                       for j, (nq, d, nk, ni) in enumerate((nq, d, nk, ni) for nq in (100, 129) for d in (40, 56, 64)
                                                           for nk in (1, 33, 77, 96) for ni in (1, 4, 16, 31, 32))], 5000)
# 2. the multi-block walk (the launcher needs B * heads * nqb >= 1024 for xqb = 2)
FUSED_MULTIBLOCK = _seeded([IPCase(1, bh, nq, 77, ni, d, scale=sc, kernel=4, xqb=xqb)
                            for (bh, nq, xqb, ni, sc) in ((128, 1000, 2, 4, 0.6), (512, 1024, 8, 16, 1.0)) for d in (40, 64)], 6000)
# 3. the remainder branch of the block -> XCD remap: 13 workgroups
FUSED_REMAP = _seeded([IPCase(1, 13, 100, 77, 4, 64, scale=1.0, kernel=4, xqb=1)], 6100)
# 4. head dims without a fused instance: text pass + image pass
TWO_PASS = _seeded([IPCase(2, 2, 100, 77, ni, d, scale=sc, kernel=5)
                    for d in (32, 80, 160) for (ni, sc) in ((4, 0.6), (16, 1.0))], 6200)

GROUPS = dict(ip_fused_small=FUSED_SMALL, ip_fused_multiblock=FUSED_MULTIBLOCK, ip_fused_remap=FUSED_REMAP, ip_two_pass=TWO_PASS)

# ---- CPU fault-model cases (tests/test_ip_adapter_cpu.py) -----------------------------------------------------------------
FAULT_CASES = _seeded([IPCase(2, 2, 100, nk, ni, d, scale=sc) for nk in (77, 96) for ni in (1, 4, 16, 32)
                       for d in (32, 40, 64, 80, 160) for sc in (0.6, 1.0)], 7000)
FAULTS = ("joint_softmax", "text_pad_leak", "img_pad_leak", "scale_ignored", "img_dropped", "img_other_batch", "img_other_head",
          "img_v_unpermuted", "img_last_dropped")


def fault_applies(fault, c: IPCase):
    """is `fault` a change of the arithmetic at all on case c"""
    if fault == "text_pad_leak":
        return c.nk_text < IMG_SLOT
    if fault == "img_pad_leak":
        return c.n_img < MAX_IMG
    if fault == "scale_ignored":
        return c.scale != 1.0
    if fault == "img_v_unpermuted":
        return c.n_img > 4                     # keys 0 .. 3 keep their columns
    if fault == "img_other_batch":
        return c.B > 1
    if fault == "img_other_head":
        return c.h > 1
    return True


# ---- inputs -------------------------------------------------------------------------------------------------------------
def _build_ip(c: IPCase):
    bld = A._build(c.text)
    P = bld["qb"].shape[0]
    g = torch.Generator().manual_seed(c.seed + 77777)
    d = c.d
    u = torch.full((d,), d ** -0.5)
    ki = 0.3 * torch.randn((P, c.n_img, d), generator=g) - 6 * u
    vi = 8.0 * torch.sign(torch.randn((P, c.n_img, d), generator=g))
    vi[:, :, 0] += torch.arange(1, c.n_img + 1, dtype=torch.float32)
    if d > 1:
        vi[:, :, 1] += (torch.arange(P) % 7).to(torch.float32)[:, None]
    bld.update(kib=ki.half().float(), vib=vi.half().float())
    return bld


def _full_ip(c: IPCase, bld):
    q, k, v = A._full(c.text, bld)
    ki = bld["kib"][bld["base"]]
    vi = bld["vib"][bld["base"]] * bld["vscale"][:, None, None]
    return q, k, v, ki.reshape(c.B, c.h, c.n_img, c.d), vi.reshape(c.B, c.h, c.n_img, c.d)


def make_ip_inputs(c: IPCase):
    """-> q [B, h, Nq, d], k / v [B, h, nk_text, d], ki / vi [B, h, n_img, d] float32 holding fp16 values, info"""
    bld = _build_ip(c)
    return (*_full_ip(c, bld), bld)


# ---- reference and model --------------------------------------------------------------------------------------------------
def _heads_out(x, B, h, Nq, d):
    return x.reshape(B, h, Nq, d).transpose(1, 2).reshape(B, Nq, h * d)


def ref_ip(q, k, v, ki, vi, scale):
    """softmax(q k^T / sqrt(d)) v + scale * softmax(q ki^T / sqrt(d)) vi in fp64 -> [B, Nq, h * d]"""
    return A.ref64(q, k, v) + scale * A.ref64(q, ki, vi)


def _r16(x):
    return x.to(torch.float16).to(torch.float64)


def model_ip(q, k, v, ki, vi, scale, two_pass=False, fault=None):
    """fp64 decoupled attention with the kernels' rounding points -> [B, Nq, h * d] fp64 (holding fp16 values).

    ``fault`` (tests/test_ip_adapter_cpu.py):
      joint_softmax     one softmax over the text and the image keys (image values times scale)
      text_pad_leak     slots nk_text .. 95 (zero K, zero V) enter the text softmax with score 0
      img_pad_leak      slots 96 + n_img .. 127 enter the image softmax with score 0
      scale_ignored     scale = 1
      img_dropped       the text attention alone
      img_other_batch   image K / V of batch row (b + 1) % B
      img_other_head    image K / V of head (h + 1) % heads
      img_v_unpermuted  image V^T stored in key order, read through the bits-2/3 permutation
      img_last_dropped  image key n_img - 1 masked
    """
    B, h, Nq, d = q.shape
    BH = B * h
    nkt, ni = k.shape[2], ki.shape[2]
    sc = torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32) * torch.tensor(A.LOG2E_F32, dtype=torch.float32)
    if fault == "img_other_batch":
        ki, vi = ki.roll(-1, 0), vi.roll(-1, 0)
    if fault == "img_other_head":
        ki, vi = ki.roll(-1, 1), vi.roll(-1, 1)
    qq, kk, vv, kki, vvi = (x.reshape(BH, -1, d).clone() for x in (q, k, v, ki, vi))
    vt, vim = torch.ones(nkt, dtype=torch.bool), torch.ones(ni, dtype=torch.bool)
    if fault == "text_pad_leak":
        n = IMG_SLOT - nkt
        kk, vv = torch.cat([kk, torch.zeros((BH, n, d))], 1), torch.cat([vv, torch.zeros((BH, n, d))], 1)
        vt = torch.ones(IMG_SLOT, dtype=torch.bool)
    if fault == "img_pad_leak":
        n = MAX_IMG - ni
        kki, vvi = torch.cat([kki, torch.zeros((BH, n, d))], 1), torch.cat([vvi, torch.zeros((BH, n, d))], 1)
        vim = torch.ones(MAX_IMG, dtype=torch.bool)
    if fault == "img_last_dropped":
        vim[ni - 1] = False
    if fault == "img_v_unpermuted":
        vp = torch.cat([vvi, torch.zeros((BH, MAX_IMG - ni, d))], 1)
        vvi = vp[:, A.vt_pos(MAX_IMG)][:, :ni]
    if fault == "scale_ignored":
        scale = 1.0
    qs = _r16(qq.float() * sc)

    def group(kx, vx, valid):
        s = qs @ kx.double().transpose(1, 2)
        s[:, :, ~valid] = -math.inf
        m = s.max(-1, keepdim=True).values
        p = _r16(torch.exp2(s - m))
        den = p.sum(-1, keepdim=True)
        return torch.where(den > 0, (p @ vx.double()) / den, torch.zeros((), dtype=torch.float64))

    if fault == "joint_softmax":
        out = _r16(group(torch.cat([kk, kki], 1), torch.cat([vv, scale * vvi], 1), torch.cat([vt, vim])))
    elif fault == "img_dropped" or (fault == "img_last_dropped" and ni == 1):
        out = _r16(group(kk, vv, vt))
    elif two_pass:
        out = _r16(_r16(group(kk, vv, vt)) + scale * group(kki, vvi, vim))
    else:
        out = _r16(group(kk, vv, vt) + scale * group(kki, vvi, vim))
    return _heads_out(out, B, h, Nq, d)


def _assemble_ip(c: IPCase, bld, f):
    """f(q, k, v, ki, vi) of the full inputs, computed on the base heads + the own rows (attn_cases._assemble)"""
    BH, d = c.B * c.h, c.d
    P = bld["qb"].shape[0]
    base = f(bld["qb"][None], bld["kb"][None], bld["vb"][None], bld["kib"][None], bld["vib"][None]).reshape(c.Nq, P, d).transpose(0, 1)
    out = base[bld["base"]] * bld["vscale"].double()[:, None, None]
    if bld["own"] is not None:
        sc = bld["vscale"][:, None, None]
        k, v = bld["kb"][bld["base"]][None], (bld["vb"][bld["base"]] * sc)[None]
        ki, vi = bld["kib"][bld["base"]][None], (bld["vib"][bld["base"]] * sc)[None]
        own = f(bld["q_own"][None, :, None, :], k, v, ki, vi).reshape(BH, d)
        out[torch.arange(BH), bld["own"]] = own
    return out.reshape(c.B, c.h, c.Nq, d).transpose(1, 2).reshape(c.B, c.Nq, c.h * d)


def reference_ip(c: IPCase, full=True):
    """-> (q, k, v, ki, vi), info, ref (fp64), E_model, bound: everything a test of case c needs, computed once"""
    bld = _build_ip(c)
    ins = _full_ip(c, bld) if full else None
    ref = _assemble_ip(c, bld, lambda *a: ref_ip(*a, c.scale))
    mod = _assemble_ip(c, bld, lambda *a: model_ip(*a, c.scale, two_pass=not c.fused))
    e_model = A.max_row_err(mod, ref, c.d)
    return ins, bld, ref, e_model, A.FACTOR * e_model
