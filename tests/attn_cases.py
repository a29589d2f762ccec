"""Inputs, references and the error bound of the attention kernel tests (plain torch, no HIP).

Shared by tests/test_attention_cases_cpu.py (the bound sees the faults it is meant to see: fault models, no GPU) and
tests/test_gpu_attention.py (the kernels of cfgpp_amd/csrc/attn_kernel.hip against the same references).

Inputs (fp16-representable, seeded; q [B, h, Nq, d], k / v [B, h, Nk, d]):
  * ``rand``: gaussian q / k / v, q multiplied by ``qscale`` (peaked rows).
  * ``neg`` : q = 0.3 * randn + 6u, k = 0.3 * randn - 6u with u a unit vector: every real score is strongly negative, so
    a pad key that enters the softmax with score 0 takes most of the probability mass (on gaussian inputs such a leak
    moves the whole-tensor rel-L2 by about 1e-3 and hides below the 1.2e-3 bound).
  * ``planted`` on top of either: chosen query rows get q = w_t and planted key K[t] gets k = c * w_t (one dominant
    score, ~24 nats above every other key) and a V row of large distinctive values, different for every key and head.
    A chosen row's output is its planted V row, or the kernel dropped / misplaced that key.
      rows: 0, Nq - 1, both sides of every multiple of 32 (hence of 128), and one row that no other (batch, head) has;
      keys: 0, Nk - 1, the first key of the last 64-key tile, keys 4 and 8 of one 32-key block (the two that the V^T
            permutation swaps) and, from four tiles on, a key of the second-to-last tile.  Every planted key beats the
            running maximum of the flash loop by far more than RESCALE_THR (attn_kernel.hip) at the tile where it appears.

Reference: ``ref64`` (softmax attention in fp64).  ``model`` is fp64 arithmetic with the kernels' documented rounding
points and nothing else: q * d^-1/2 * log2(e) rounded to fp16, P = exp2(s - max) rounded to fp16, the denominator summed
from those rounded P, the output rounded to fp16.

Metric: per (batch, head, query) row of d outputs ||got - ref|| / (||ref|| + 1e-3 * rms row norm), maximum over rows.
Bound of a case: FACTOR * E_model with E_model the model's own max-row error against ref64, computed on the CPU by the
test that uses it - never taken from a kernel.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import torch

# FACTOR = 2 x 2.  The model's max-row error varies by 1.05x .. 1.7x between five seeds of a case (eleven case families of the
# tables below: neg 1.2x, neg + planted 1.5x, rand + planted 1.7x, rand x 4 1.4x); 2 covers another rounding sample.  The second
# 2 covers what the model leaves out: the fp32 accumulation order of the MFMAs, the hardware exp2, the fp32 (unrounded-P)
# denominator of the d % 32 == 0 kernels and the deferred re-reference of the flash loop, which only scales P up (fewer fp16
# underflows than the model has).  A correct kernel that exceeds it means a rounding point the model lacks: add it, keep the 4.
# Kernel / E_model ratios on the MI355X: NOT MEASURED yet - the tests record e_model, max_row_err and ratio of every case
# ("attention_case" lines of the parity file that record() writes); put min / median / max per group here from the first run.
FACTOR = 4.0

REL_L2_BOUND = 1.2e-3          # the whole-tensor bound of the older attention tests, kept
FP16_MAX = 65504.0
LOG2E_F32 = 1.4426950408889634


@dataclass(frozen=True)
class Case:
    B: int
    h: int
    Nq: int
    Nk: int
    d: int
    kind: str                  # "rand" | "neg"
    planted: bool = False
    qscale: float = 1.0        # rand only
    seed: int = 0
    kernel: int = 0            # expected dispatch: 1 attn_kernel, 2 attn64_kernel, 3 xattn64_kernel (cfgpp_attention_last_launch)
    xqb: int = 0               # expected 128-query blocks per workgroup (xattn64_kernel), 0 for the flash kernels
    dma: int = 1               # cfgpp_attention_set_dma
    cross: int = 1             # cfgpp_attention_set_cross
    period: int = 32           # distinct base heads (see _build)

    @property
    def id(self):
        s = f"B{self.B}h{self.h}q{self.Nq}k{self.Nk}d{self.d}-{self.kind}"
        if self.kind == "rand" and self.qscale != 1.0:
            s += f"{self.qscale:g}"
        if self.planted:
            s += "+planted"
        if not self.dma:
            s += "-dma0"
        if not self.cross:
            s += "-cross0"
        return s

    @property
    def d16(self):
        return (self.d + 15) // 16

    @property
    def ones(self):
        return int(self.d % 32 != 0)

    @property
    def grid(self):
        """workgroups of the launch"""
        nqb = (self.Nq + 127) // 128
        return self.B * self.h * (nqb // self.xqb if self.xqb else nqb)


def _seeded(cases):
    return [replace(c, seed=1000 + i) for i, c in enumerate(cases)]


def _kernel_for(d, Nk, dma=1, cross=1):
    dp64 = (d + 31) // 32 == 2
    if dp64 and dma and cross and Nk <= 128:
        return 3
    return 2 if dp64 and dma else 1


# ---- the case tables (the smallest shapes that reach each path) -------------------------------------------------------
# 1. xattn64_kernel walking xqb > 1 query blocks per workgroup (the launcher needs B * heads * nqb >= 1024 for that)
XATTN_MULTIBLOCK = _seeded([Case(1, bh, nq, 77, d, "neg", planted=True, kernel=3, xqb=xqb)
                            for (bh, nq, xqb) in ((128, 1000, 2), (256, 1000, 4), (512, 1000, 8), (512, 1024, 8))
                            for d in (40, 48, 64)])

# 2. key counts up to 128 through xattn64_kernel (one to four 32-key sub-tiles, every position of the mask)
XATTN_SMALL = _seeded(
    [Case(1, 2, nq, nk, d, kind, planted=nq > 1, qscale=2.0, kernel=3, xqb=1)          # (Nq = 1: a plain neg row, not a planted one)
     for nk in (1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128) for d in (40, 56, 64)
     for (nq, kind) in ((1, "neg"), (100, "neg"), (129, "rand"))]
    + [Case(1, 2, n, n, d, "rand", planted=True, kernel=3, xqb=1) for n in (64, 96, 128) for d in (40, 56, 64)])

# 3. the flash loop of attn64_kernel with a partial last tile; B = 2 with a ragged Nq: a store past Nq would land in batch 1
FLASH_PARTIAL = _seeded(
    [Case(B, h, nq, nk, d, kind, planted=planted, qscale=qs, kernel=2)
     for nk in (129, 144, 191, 193, 4097) for (B, h, nq) in ((2, 2, 100), (1, 3, 257)) for d in (40, 48, 56, 64)
     for (kind, planted, qs) in (("neg", False, 1.0), ("rand", True, 1.0), ("rand", False, 4.0))])

# 4. every head dim: the sixteen that have an instance, and the four that must be refused
HEAD_DIMS_OK = (8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 120, 128, 152, 160)
HEAD_DIMS_REFUSED = (104, 112, 136, 144)
HEAD_DIMS = _seeded([Case(1, 2, 100, 144, d, "neg", planted=True, kernel=_kernel_for(d, 144)) for d in HEAD_DIMS_OK])

# 5. the A/B switches: the register-staged kernel at dp = 64, the flash loop at <= 128 keys, the re-reference branch
SWITCH_DMA0 = _seeded([Case(1, 2, 100 if nk == 144 else 200, nk, d, "neg", planted=True, kernel=1, dma=0)
                       for d in (40, 48, 64) for nk in (144, 1024)])
SWITCH_CROSS0 = _seeded([Case(1, 2, 100, nk, d, "neg", planted=True, kernel=2, cross=0) for nk in (77, 128) for d in (40, 64)])
RESCALE = _seeded([Case(1, 1, 200, 1024, d, "rand", planted=True, kernel=_kernel_for(d, 1024)) for d in (40, 64, 80, 160)])

# 6. the remainder branch of the block -> XCD remap: more than 8 workgroups, not a multiple of 8
REMAP = _seeded([Case(1, 3, 300, 144, 40, "neg", planted=True, kernel=2),          # 9 = 3 heads x 3 query blocks
                 Case(1, 13, 100, 144, 64, "neg", planted=True, kernel=2),        # 13
                 Case(1, 23, 100, 144, 80, "neg", planted=True, kernel=1),        # 23
                 Case(1, 3, 300, 77, 40, "neg", planted=True, kernel=3, xqb=1),   # 9
                 Case(1, 13, 100, 77, 64, "neg", planted=True, kernel=3, xqb=1)])  # 13

GROUPS = dict(xattn_multiblock=XATTN_MULTIBLOCK, xattn_small=XATTN_SMALL, flash_partial=FLASH_PARTIAL, head_dims=HEAD_DIMS,
              switch_dma0=SWITCH_DMA0, switch_cross0=SWITCH_CROSS0, rescale=RESCALE, remap=REMAP)
ALL_CASES = [c for g in GROUPS.values() for c in g]


# ---- inputs -------------------------------------------------------------------------------------------------------------
def vt_pos(n):
    """column of key 0..n-1 in a V^T buffer: bits 2 and 3 of the key index swapped (include/cfgpp.h)"""
    key = torch.arange(n)
    return (key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1)


def planted_keys(Nk):
    keys = [0, Nk - 1, 64 * ((Nk - 1) // 64)]
    if Nk >= 9:
        blk = 32 * ((Nk - 9) // 32)                # the last 32-key block that holds both of its keys 4 and 8
        keys += [blk + 4, blk + 8]
    ntiles = (Nk + 63) // 64
    if ntiles >= 4:
        keys.append(64 * (ntiles - 2) + 21)        # a late tile that is not the last
    out = []
    for k in keys:
        if k not in out:
            out.append(k)
    return out


def planted_rows(Nq):
    rows = {0, Nq - 1}
    for m in range(32, Nq, 32):
        rows.update((m - 1, m))
    return sorted(rows)


def own_row(bh, Nq):
    """the extra planted row of (batch, head) bh: distinct for bh < Nq when 37 does not divide Nq"""
    return (5 + 37 * bh) % Nq


def _build(c: Case):
    """flattened [heads, N, d] tensors of fp16 values.  Heads repeat with period c.period: (batch, head) bh holds the q / k of base
    head bh % period and its v multiplied by 1, 2 or 4 (exact in fp16, and the output scales with it), and differs from every
    other bh in its own planted row - so the references of the 512-head cases cost 32 heads plus one row per head."""
    g = torch.Generator().manual_seed(c.seed)
    BH, d = c.B * c.h, c.d
    P = min(BH, c.period)
    q = torch.randn((P, c.Nq, d), generator=g)
    k = torch.randn((P, c.Nk, d), generator=g)
    v = torch.randn((P, c.Nk, d), generator=g)
    u = torch.full((d,), d ** -0.5)
    if c.kind == "neg":
        q = 0.3 * q + 6 * u
        k = 0.3 * k - 6 * u
    else:
        q = q * c.qscale
    bh = torch.arange(BH)
    out = dict(base=bh % P, vscale=(2.0 ** ((bh // P) % 3)), keys=[], rows=[], own=None, q_own=None, key_of_row=None)
    if c.planted:
        keys, rows = planted_keys(c.Nk), planted_rows(c.Nq)
        nK = len(keys)
        # w_t = a e_t - b u_t (u_t = u without component t): the pair scores c |w_t|^2 / sqrt(d) = 24 .. 60 nats, at least 20 above
        # the row's next key.  neg: b is set so that the OTHER queries (~6u) see a planted key 14 nats below an ordinary one
        # (9 u . w_t = -(36 / sqrt(d) + 14)): the large planted V rows stay out of their outputs, and the pads stay the largest score
        if c.kind == "neg":
            uw = -(36.0 / math.sqrt(d) + 14.0) / 9.0
            a, b, cc = 4.0, (4.0 / math.sqrt(d) - uw) / (1 - 1.0 / d), 1.5 * math.sqrt(d)
        else:
            a, b, cc = 16.0, 0.0, 24.0 * math.sqrt(d) / 256.0
        w = torch.zeros((nK, d))
        for t in range(nK):
            w[t] = -b * u
            w[t, t] = a
        q[:, rows] = w[torch.arange(len(rows)) % nK]
        k[:, keys] = cc * w
        pv = 8.0 * torch.sign(torch.randn((P, nK, d), generator=g))
        pv[:, :, 0] += torch.arange(1, nK + 1, dtype=torch.float32)
        pv[:, :, 1] += (torch.arange(P) % 7).to(torch.float32)[:, None]
        v[:, keys] = pv
        key_of_row = torch.full((BH, c.Nq), -1, dtype=torch.long)
        key_of_row[:, rows] = torch.arange(len(rows)) % nK
        key_of_row[bh, own_row(bh, c.Nq)] = bh % nK
        out.update(keys=keys, rows=rows, own=own_row(bh, c.Nq), q_own=w[bh % nK].half().float(), key_of_row=key_of_row)
    out.update(qb=q.half().float(), kb=k.half().float(), vb=v.half().float())
    return out


def _full(c: Case, bld):
    q = bld["qb"][bld["base"]]
    if bld["own"] is not None:
        q[torch.arange(q.shape[0]), bld["own"]] = bld["q_own"]
    k = bld["kb"][bld["base"]]
    v = bld["vb"][bld["base"]] * bld["vscale"][:, None, None]
    return tuple(x.reshape(c.B, c.h, -1, c.d) for x in (q, k, v))


def make_inputs(c: Case):
    """-> q [B, h, Nq, d], k, v [B, h, Nk, d] float32 holding fp16 values, info (planted rows / keys)"""
    bld = _build(c)
    return (*_full(c, bld), bld)


# ---- reference, model, fault models -----------------------------------------------------------------------------------
def _chunks(BH, per_bh):
    step = max(1, int(2 ** 24 // max(per_bh, 1)))
    return [(i, min(BH, i + step)) for i in range(0, BH, step)]


def ref64(q, k, v):
    """softmax(q k^T / sqrt(d)) v in fp64 -> [B, Nq, h * d]"""
    B, h, Nq, d = q.shape
    Nk = k.shape[2]
    qq, kk, vv = (x.reshape(B * h, -1, d) for x in (q, k, v))
    out = torch.empty((B * h, Nq, d), dtype=torch.float64)
    for i, j in _chunks(B * h, Nq * Nk):
        s = qq[i:j].double() @ kk[i:j].double().transpose(1, 2) / math.sqrt(d)
        out[i:j] = torch.softmax(s, -1) @ vv[i:j].double()
    return out.reshape(B, h, Nq, d).transpose(1, 2).reshape(B, Nq, h * d)


def _r16(x):
    return x.to(torch.float16).to(torch.float64)


def model(q, k, v, fault=None, **fk):
    """fp64 attention with the kernels' rounding points -> [B, Nq, h * d] fp64 (holding fp16 values).

    ``fault`` injects one defect of the kind the GPU tests must catch (tests/test_attention_cases_cpu.py):
      pad_leak        keys Nk .. round_up(Nk, 64) - 1 (zero K, zero V) enter the softmax with score 0
      drop_key        key=j is masked although valid
      v_unpermuted    V^T stored in key order, read through the bits-2/3 permutation
      denom_pads      the denominator also counts the pad keys (an unmasked P meeting the ones row of V^T)
      prev_q_block    query block i of every xqb-block walk answers with block i - 1's queries (a wrong q0n), xqb=
      swap_heads      heads 0 and 1 of the output exchanged
      unwritten       rows=(r0, r1) of the output never stored (left 0)
      no_rereference  the running reference stays the first tile's maximum: P = exp2(s - m_tile0) saturates at the fp16 maximum
                      in the PV product while the fp32 running sum of the d % 32 == 0 kernels keeps the unsaturated value.
                      (Where the denominator comes from the ones row of V^T it saturates with the numerator and the row
                      stays nearly right; the hardware conversion gives inf, not the maximum, which the finiteness check of
                      the GPU tests sees.)
    """
    B, h, Nq, d = q.shape
    Nk = k.shape[2]
    BH = B * h
    scale = torch.tensor(1.0 / math.sqrt(d), dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32)
    qq, kk, vv = (x.reshape(BH, -1, d).clone() for x in (q, k, v))
    valid = torch.ones(Nk, dtype=torch.bool)
    n_pad = (-Nk) % 64
    if fault == "prev_q_block":
        xqb = fk["xqb"]
        src = qq.clone()
        for blk in range(1, (Nq + 127) // 128):
            if blk % xqb:
                n = min(128, Nq - blk * 128)
                qq[:, blk * 128: blk * 128 + n] = src[:, (blk - 1) * 128: (blk - 1) * 128 + n]
    if fault == "pad_leak":
        kk = torch.cat([kk, torch.zeros((BH, n_pad, d))], 1)
        vv = torch.cat([vv, torch.zeros((BH, n_pad, d))], 1)
        valid = torch.ones(Nk + n_pad, dtype=torch.bool)
    if fault == "drop_key":
        valid[fk["key"]] = False
    if fault == "v_unpermuted":
        vp = torch.cat([vv, torch.zeros((BH, (-Nk) % 32, d))], 1)
        vv = vp[:, vt_pos(vp.shape[1])][:, :Nk]
    out = torch.empty((BH, Nq, d), dtype=torch.float64)
    for i, j in _chunks(BH, Nq * kk.shape[1]):
        qs = _r16(qq[i:j].float() * scale)                                  # fp32 product, rounded to fp16 (as the kernels)
        s = qs @ kk[i:j].double().transpose(1, 2)                           # log2 domain
        s[:, :, ~valid] = -math.inf
        if fault == "no_rereference":
            m = s[:, :, :64].max(-1, keepdim=True).values
            p = _r16(torch.exp2(s - m).clamp(max=FP16_MAX))
            den = torch.exp2(s - m).sum(-1, keepdim=True)
        else:
            m = s.max(-1, keepdim=True).values
            p = _r16(torch.exp2(s - m))
            den = p.sum(-1, keepdim=True)
        if fault == "denom_pads":
            den = den + n_pad * _r16(torch.exp2(-m))
        out[i:j] = _r16((p @ vv[i:j].double()) / den)
    out = out.reshape(B, h, Nq, d)
    if fault == "swap_heads":
        out = out[:, [1, 0] + list(range(2, h))]
    if fault == "unwritten":
        r0, r1 = fk["rows"]
        out = out.clone()
        out[:, :, r0:r1] = 0.0
    return out.transpose(1, 2).reshape(B, Nq, h * d)


# ---- metric -------------------------------------------------------------------------------------------------------------
def max_row_err(got, ref, d):
    """max over (batch, query, head) rows of ||got - ref|| / (||ref|| + 1e-3 * rms row norm); NaN / inf in got -> inf"""
    g = got.detach().double().cpu().reshape(-1, d)
    r = ref.detach().double().cpu().reshape(-1, d)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    rn = r.norm(dim=1)
    rms = float(rn.pow(2).mean().sqrt())
    return float(((g - r).norm(dim=1) / (rn + 1e-3 * rms)).max())


def rel_l2(got, ref):
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((g - r).norm() / (r.norm() + 1e-30))


def _assemble(c: Case, bld, f):
    """f (ref64 or model) of the full inputs, computed on the base heads + the own rows (see _build)"""
    BH, d = c.B * c.h, c.d
    P = bld["qb"].shape[0]
    base = f(bld["qb"][None], bld["kb"][None], bld["vb"][None]).reshape(c.Nq, P, d).transpose(0, 1)      # [P, Nq, d]
    out = base[bld["base"]] * bld["vscale"].double()[:, None, None]
    if bld["own"] is not None:
        k = bld["kb"][bld["base"]][None]
        v = (bld["vb"][bld["base"]] * bld["vscale"][:, None, None])[None]
        own = f(bld["q_own"][None, :, None, :], k, v).reshape(BH, d)
        out[torch.arange(BH), bld["own"]] = own
    return out.reshape(c.B, c.h, c.Nq, d).transpose(1, 2).reshape(c.B, c.Nq, c.h * d)


def reference(c: Case, full=True):
    """-> q, k, v, info, ref (fp64), E_model, bound: everything a test of case c needs, computed once (full=False: q = k = v = None)"""
    bld = _build(c)
    q, k, v = _full(c, bld) if full else (None, None, None)
    ref = _assemble(c, bld, ref64)
    e_model = max_row_err(_assemble(c, bld, model), ref, c.d)
    return q, k, v, bld, ref, e_model, FACTOR * e_model
