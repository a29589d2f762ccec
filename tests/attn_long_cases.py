"""Cases, padded inputs and fault models for xattn64_long_kernel (csrc/attn_kernel.hip): cross-attention over 129 .. 320 keys at
head dims padded to 64, reached through cfgpp_op_attention_cross (dispatch record: kernel 6).

Everything numeric comes from tests/attn_cases.py - Case, the seeded inputs with their planted rows and keys, the fp64 reference,
the model of the kernels' rounding points, the per-row metric and FACTOR.  This file adds the case table, the two faults a
resident multi-tile kernel can have that the older kernels cannot, and the junk that fills the key slots behind the context.

Kernel / E_model ratios measured on the MI355X (max row error of xattn64_long_kernel over the model's, min / median / max per
group; profiles/long_prompt/attention_long_case_parity.jsonl): key counts 0.73 / 1.00 / 1.25 (117 cases), multiblock 0.94 / 1.00 /
1.06, ragged 1.00 / 1.01 / 1.02, late key 1.06 / 1.07 / 1.09, remap 1.00 / 1.00 / 1.00 - against the bound's FACTOR = 4.

Shared by tests/test_attention_long_cases_cpu.py (the bound sees the faults, no GPU) and tests/test_gpu_attention_long.py.
"""
from __future__ import annotations

from dataclasses import replace

import torch

import attn_cases as A
from attn_cases import Case

K_PAD = 320                    # key slots of the buffers the GPU tests launch on: the engine's ck_pad at max_tokens = 308
JUNK = 100.0                   # |value| of what the slots [Nk, K_PAD) hold


def _seeded(cases, base):
    return [replace(c, seed=base + i) for i, c in enumerate(cases)]


def launcher_xqb(c: Case) -> int:
    """128-query blocks per workgroup, by the launcher's rule restated (cfgpp_op_attention_cross: that of xattn64_kernel)"""
    nqb, BH = (c.Nq + 127) // 128, c.B * c.h
    xqb = 1
    while xqb < 8 and nqb % (xqb * 2) == 0 and BH * (nqb // (xqb * 2)) >= 512:
        xqb *= 2
    return xqb


# ---- the case tables -------------------------------------------------------------------------------------------------------
# 1. key counts: both sides of every tile (64) and sub-tile (32) border in range, the chunked prompts (154, 231, 308) and the ends
KEY_COUNTS = _seeded(
    [Case(1, 2, nq, nk, d, kind, planted=planted, qscale=qs, kernel=6, xqb=1)
     for nk in (129, 154, 160, 161, 191, 192, 193, 231, 256, 257, 308, 319, 320) for d in (40, 56, 64)
     for (nq, kind, planted, qs) in ((1, "neg", False, 1.0), (100, "neg", True, 1.0), (129, "rand", True, 2.0))], 2000)

# 2. every xqb the launcher emits, at the smallest B * h * Nq that reaches it; a ragged (1000) and a full (1024) last block
MULTIBLOCK = _seeded([Case(1, bh, nq, nk, d, "neg", planted=True, kernel=6, xqb=xqb)
                      for (bh, nq, xqb) in ((128, 1000, 2), (256, 1000, 4), (512, 1000, 8), (512, 1024, 8))
                      for d in (40, 64) for nk in (154, 308)], 2200)

# 3. ragged batch: a store past Nq would land in batch 1
RAGGED = _seeded([Case(2, 2, 100, 231, d, "neg", planted=True, kernel=6, xqb=1) for d in (40, 64)], 2300)

# 4. a late dominant key: five tiles, the planted key of the second-to-last one (and those of the last) beat the running maximum
#    of peaked rows by far more than RESCALE_THR
LATE_KEY = _seeded([Case(1, 2, 200, 308, d, "rand", planted=True, qscale=4.0, kernel=6, xqb=1) for d in (40, 64)], 2400)

# 5. the remainder branch of the block -> XCD remap
REMAP = _seeded([Case(1, 3, 300, 154, 40, "neg", planted=True, kernel=6, xqb=1),          # 9 = 3 heads x 3 query blocks
                 Case(1, 13, 100, 231, 64, "neg", planted=True, kernel=6, xqb=1)], 2500)  # 13

GROUPS = dict(long_key_counts=KEY_COUNTS, long_multiblock=MULTIBLOCK, long_ragged=RAGGED, long_late_key=LATE_KEY, long_remap=REMAP)
ALL_CASES = [c for g in GROUPS.values() for c in g]


# ---- the slots behind the context -------------------------------------------------------------------------------------------
def junk(c: Case, n: int):
    """-> (K junk [B * h, n, d], V junk [B * h, n, d]): +-JUNK, seeded by the case"""
    g = torch.Generator().manual_seed(c.seed + 7919)
    sign = lambda: torch.where(torch.rand((c.B * c.h, n, c.d), generator=g) < 0.5, -JUNK, JUNK)
    return sign(), sign()


# ---- fault models on top of attn_cases.model --------------------------------------------------------------------------------
def model_tile_alias(c: Case, q, k, v, tile: int):
    """64-key tile `tile` >= 1 answers with tile - 1's K and V^T (a wrong LDS tile offset); the mask still follows the real key count"""
    idx = torch.arange(c.Nk)
    sel = (idx // 64) == tile
    idx[sel] -= 64
    return A.model(q, k[:, :, idx], v[:, :, idx])


def model_stale_slots(c: Case, q, k, v):
    """the junk of slots [Nk, K_PAD) enters the softmax (a mask that follows the buffer, not the context)"""
    n = K_PAD - c.Nk
    jk, jv = junk(c, n)
    k2 = torch.cat([k, jk.reshape(c.B, c.h, n, c.d)], 2)
    v2 = torch.cat([v, jv.reshape(c.B, c.h, n, c.d)], 2)
    return A.model(q, k2, v2)
