"""Cases, inputs, references and fault models for the soft regional cross-attention kernel (csrc/attn_kernel.hip:
attn_region_soft_kernel, reached through cfgpp_op_attention_region_soft, dispatch record: kernel 9).

R = 2 .. 4 regions own the key slots [77 r, 77 r + 77); a weight map w [map_rows][R][Nq] (fp32, rows summing to 1) blends them:
    o = sum_r w_r(q) softmax(q K_r) V_r
The reference is that sum in fp64 with every region's softmax over its own 77 keys.  ``model`` is fp64 arithmetic with the kernel's
documented rounding points and nothing else: q * d^-1/2 * log2(e) rounded to fp16, P_r = exp2(s - m_r) rounded to fp16, l_r the sum
of those rounded P_r, the fp32 weights as they are, ONE fp16 rounding of sum_r (w_r / l_r) O_r; terms with w_r == 0 are not
evaluated.  Metric and FACTOR are those of tests/attn_cases.py: a case's bound is FACTOR x the model's own max-row error.

Inputs (fp16-representable, seeded): q = 0.5 randn + 1, k = randn (ordinary scores ~ N(0, 1.25) nats).  Values share a COMMON
component across regions (v = common + offset_r + 0.5 randn, common and offset_r per head) so that a blend does not cancel; offset_r
makes the regions differ, so that a wrong weight is loud.  Local keys 0 and 76 of region r are HEAVY: k = (2.5 + 0.5 r) / sqrt(d) on
every axis (score ~ 2.5 + 0.5 r nats for every query: ~ 10 % of the row's mass each) with V rows of +-8 - a key window that is off
by one slot in either direction loses one and admits the neighbour's; the different strengths make the regions' denominators differ,
which a joint normalisation would mix.  A region whose weight is zero in EVERY row of a case holds keys that would dominate (score
~ +20 nats) and values of +-100; the slots [77 R, k_pad) hold the +-100 junk of attn_long_cases.junk.

Kernel / E_model ratios measured on the MI355X (profiles/regional_soft/attention_region_soft_case_parity.jsonl; min / median / max
per group): soft_hot 1.00 / 1.00 / 1.00 (90 cases), soft_mixed 1.00 / 1.00 / 1.00 (60), soft_skip 1.00 / 1.00 / 1.01 (36), soft_batch
1.00 / 1.00 / 1.00 (18) - against the bound's FACTOR = 4.

What no case can show: whether a zero-weight term of an EVALUATED region is skipped by a select or multiplied by 0.  P <= 1, at most
77 keys and fp32 accumulation keep O_r and l_r finite for every finite fp16 input, so 0 x (O_r / l_r) = 0 and both forms give the
same bits; only a non-finite value slot tells them apart, and that reaches the rows that do weigh the region as well (0 x inf inside
the PV product).  The fault model `zero_evaluated` therefore lives in the CPU test alone.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from types import SimpleNamespace

import torch

import attn_cases as A
import attn_long_cases as L

K_PAD = L.K_PAD
TOK = 77
HEAD_DIMS_REFUSED = A.HEAD_DIMS_REFUSED
LANE_ROW = 77                  # pattern "lane": the one row (wave 2, lane 13 of workgroup 0) that weighs region R - 1


@dataclass(frozen=True)
class SCase:
    B: int
    h: int
    Nq: int
    d: int
    R: int
    pattern: str               # "hot<r>", "uniform", "ramp", "skip<r>", "lane", "random", "pair" (B = 2: two different maps)
    map_rows: int = 1
    seed: int = 0
    k_pad: int = K_PAD
    kernel: int = 9

    @property
    def id(self):
        s = f"B{self.B}h{self.h}q{self.Nq}d{self.d}R{self.R}-{self.pattern}-m{self.map_rows}"
        return s + (f"-kp{self.k_pad}" if self.k_pad != K_PAD else "")

    @property
    def Nk(self):
        return TOK * self.R

    @property
    def d16(self):
        return (self.d + 15) // 16

    @property
    def ones(self):
        return int(self.d % 32 != 0)

    @property
    def grid(self):
        return self.B * self.h * ((self.Nq + 127) // 128)


def _seeded(cases, base):
    return [replace(c, seed=base + i) for i, c in enumerate(cases)]


def min_k_pad(R):
    return (TOK * R + 63) // 64 * 64


D_ALL = (32, 40, 64, 80, 160)          # dp = 32, 64 (ONES and fp32 sum), 96, 160: every padded head dim the engine configs reach

# 1. one-hot: every row in region r, for each r - the hard partition; one query and a ragged block
HOT = _seeded([SCase(1, 2, nq, d, R, f"hot{r}") for R in (2, 3, 4) for r in range(R) for d in D_ALL for nq in (1, 100)], 6000)

# 2. blends at Nq = 129 (two blocks, the second with one row): uniform 1 / R; a ramp inside a 32-row wave slab and one across the
#    128-query block edge; region R - 1 weighed by exactly ONE lane of one wave of workgroup 0 (the workgroup vote); random weights
MIXED = _seeded([SCase(1, 2, 129, d, R, p) for R in (2, 3, 4) for p in ("uniform", "ramp", "lane", "random") for d in D_ALL], 6200)

# 3. a region with zero weight in every row (never evaluated: it holds dominating keys and +-100 values), three blocks, nine
#    workgroups (the remainder branch of the block -> XCD remap); the ramps at three blocks: interior workgroups pay for one region
SKIP = _seeded([SCase(1, 3, 300, d, R, f"skip{r}") for R in (2, 3, 4) for r in (0, R - 1) for d in D_ALL]
               + [SCase(1, 3, 300, d, R, "ramp") for R in (2, 3, 4) for d in (40, 160)], 6400)

# 4. two batch rows, ragged (a store past Nq would land in batch 1): a map per row against one shared map; the buffers have
#    exactly round_up(77 R, 64) key slots
BATCH = _seeded([SCase(2, 1, 100, d, R, p, map_rows=m, k_pad=min_k_pad(R))
                 for R in (2, 3, 4) for (p, m) in (("pair", 2), ("random", 1)) for d in (40, 64, 80)], 6600)

GROUPS = dict(soft_hot=HOT, soft_mixed=MIXED, soft_skip=SKIP, soft_batch=BATCH)
ALL_CASES = [c for g in GROUPS.values() for c in g]


# ---- weight maps ---------------------------------------------------------------------------------------------------------------
def weights(c: SCase) -> torch.Tensor:
    """-> float32 [map_rows, R, Nq], every column summing to 1 up to fp32 rounding"""
    R, Nq = c.R, c.Nq
    q = torch.arange(Nq, dtype=torch.float32)
    g = torch.Generator().manual_seed(c.seed + 104729)

    def rand(nr):
        x = torch.rand((nr, Nq), generator=g) + 0.05
        return x / x.sum(0, keepdim=True)

    def one(p):
        w = torch.zeros((R, Nq))
        if p.startswith("hot"):
            w[int(p[3:])] = 1.0
        elif p == "uniform":
            w[:] = 1.0 / R
        elif p == "ramp":              # region 0 -> 1 over rows 40 .. 56 (inside the slab 32 .. 63), 1 -> R - 1 (R = 2: back to 0) over 120 .. 136
            t1 = ((q - 40) / 16).clamp(0, 1)
            t2 = ((q - 120) / 16).clamp(0, 1)
            last = R - 1 if R > 2 else 0
            w[0] += 1 - t1
            w[1] += t1 * (1 - t2)
            w[last] += t2
        elif p.startswith("skip"):
            s = int(p[4:])
            keep = [r for r in range(R) if r != s]
            w[keep] = rand(len(keep))
        elif p == "lane":
            w[:R - 1] = rand(R - 1)
            if Nq > LANE_ROW:
                w[:R - 1, LANE_ROW] *= 0.5
                w[R - 1, LANE_ROW] = 0.5
        elif p == "random":
            w = rand(R)
        elif p == "random_rev":
            w = rand(R).flip(0).flip(1)
        else:
            raise ValueError(p)
        return w
    if c.pattern == "pair":
        assert c.map_rows == 2 and c.B == 2
        return torch.stack([one("random"), one("random_rev")])
    return torch.stack([one(c.pattern)] * c.map_rows)


def weight_buffer(c: SCase, q_pad: int, w=None) -> torch.Tensor:
    """the fp32 [map_rows][R][q_pad] buffer of the op: the map, pads 0"""
    w = weights(c) if w is None else w
    buf = torch.zeros((c.map_rows, c.R, q_pad), dtype=torch.float32)
    buf[:, :, :c.Nq] = w
    return buf


def dead_regions(c: SCase, w=None):
    """regions whose weight is zero in every row of the case"""
    w = weights(c) if w is None else w
    return [r for r in range(c.R) if not bool((w[:, r] != 0).any())]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
HEAVY_LOCAL = (0, 76)


def build(c: SCase):
    """-> dict: q [B, h, Nq, d], k, v [h, k_pad, d] (fp32 holding fp16 values; junk behind the context and in the dead regions),
    w [B, R, Nq] fp32 (the map of every batch row), wmap [map_rows, R, Nq]"""
    g = torch.Generator().manual_seed(c.seed)
    d, R, Nk, h = c.d, c.R, c.Nk, c.h
    q = 0.5 * torch.randn((c.B, h, c.Nq, d), generator=g) + 1.0
    k = torch.randn((h, Nk, d), generator=g)
    common = torch.randn((h, 1, d), generator=g)
    off = torch.randn((h, R, 1, d), generator=g)
    v = 0.5 * torch.randn((h, Nk, d), generator=g) + common
    v = (v.reshape(h, R, TOK, d) + off).reshape(h, Nk, d)
    for r in range(R):
        for j, loc in enumerate(HEAVY_LOCAL):
            k[:, TOK * r + loc] = (2.5 + 0.5 * r) / math.sqrt(d)
            pv = 8.0 * torch.sign(torch.randn((h, d), generator=g))
            pv[:, 0] += r + 1
            pv[:, 1] += 2 * j + 1
            v[:, TOK * r + loc] = pv
    wmap = weights(c)
    for r in dead_regions(c, wmap):
        k[:, TOK * r: TOK * (r + 1)] = 20.0 / math.sqrt(d)
        v[:, TOK * r: TOK * (r + 1)] = torch.where(torch.rand((h, TOK, d), generator=g) < 0.5, -L.JUNK, L.JUNK)
    jk, jv = L.junk(SimpleNamespace(B=1, h=h, d=d, seed=c.seed), c.k_pad - Nk)
    r16 = lambda x: x.half().float()
    w = wmap if c.map_rows == c.B else wmap.expand(c.B, R, c.Nq)
    return dict(q=r16(q), k=torch.cat([r16(k), jk], 1), v=torch.cat([r16(v), jv], 1), w=w, wmap=wmap)


def full_inputs(c: SCase, bld):
    """-> q [B, h, Nq, d], k, v [B, h, k_pad, d]: what the GPU tests upload"""
    return bld["q"], bld["k"][None].expand(c.B, -1, -1, -1), bld["v"][None].expand(c.B, -1, -1, -1)


# ---- reference, model, fault models ------------------------------------------------------------------------------------------
def _r16(x):
    return x.to(torch.float16).to(torch.float64)


def region_term(c: SCase, bld, r, rounded, lo=None):
    """region r's complete attention over keys [lo, lo + 77) (default 77 r) -> (O_r [B, h, Nq, d], l_r [B, h, Nq, 1]) fp64 with
    softmax = O_r / l_r; rounded: the kernel's rounding points (fp16 scaled q in the log2 domain, fp16 P, l_r summed from them)"""
    lo = TOK * r if lo is None else lo
    idx = torch.arange(lo, lo + TOK).clamp(0, c.k_pad - 1)
    k, v = bld["k"][:, idx].double()[None], bld["v"][:, idx].double()[None]
    if rounded:
        scale = torch.tensor(1.0 / math.sqrt(c.d), dtype=torch.float32) * torch.tensor(A.LOG2E_F32, dtype=torch.float32)
        s = _r16(bld["q"] * scale) @ k.transpose(-1, -2)
        p = _r16(torch.exp2(s - s.max(-1, keepdim=True).values))
    else:
        s = bld["q"].double() @ k.transpose(-1, -2) / math.sqrt(c.d)
        p = torch.exp(s - s.max(-1, keepdim=True).values)
    return p @ v, p.sum(-1, keepdim=True)


def _out(c, x):
    return x.transpose(1, 2).reshape(c.B, c.Nq, c.h * c.d)


def ref64(c: SCase, bld):
    out = torch.zeros((c.B, c.h, c.Nq, c.d), dtype=torch.float64)
    for r in range(c.R):
        w = bld["w"][:, r].double()[:, None, :, None]
        if bool((w != 0).any()):
            o, l = region_term(c, bld, r, False)
            out += torch.where(w != 0, w * o / l, torch.zeros(()).double())
    return _out(c, out)


def model(c: SCase, bld, fault=None, **fk):
    """fp64 with the kernel's rounding points -> [B, Nq, h * d] fp64 (holding fp16 values).

    ``fault`` injects one defect of the kind the GPU tests must catch (tests/test_attention_region_soft_cases_cpu.py):
      swap_weights     the weights of regions a= and b= exchanged
      next_batch_map   batch row b uses row b + 1's map (the last row the first's)
      joint_norm       sum_r w_r O_r / sum_r w_r l_r instead of sum_r w_r O_r / l_r
      off_by_one       every region's key window shifted by shift=+-1 slot
      stride_nq        the region stride of the weight buffer read as Nq instead of q_tok_pad
      lane_skipped     a region is skipped unless at least two rows of the workgroup's 128 weigh it
      zero_evaluated   a term with w_r == 0 is evaluated and multiplied by its zero weight (0 x a non-finite O_r is NaN)
    """
    w = bld["w"].double()                                              # [B, R, Nq]
    if fault == "swap_weights":
        idx = list(range(c.R))
        idx[fk["a"]], idx[fk["b"]] = idx[fk["b"]], idx[fk["a"]]
        w = w[:, idx]
    if fault == "next_batch_map":
        w = w.roll(-1, 0)
    if fault == "stride_nq":
        q_pad = (c.Nq + 127) // 128 * 128
        flat = torch.cat([weight_buffer(c, q_pad, bld["wmap"]).reshape(c.map_rows, -1), torch.zeros((c.map_rows, q_pad))], 1)
        wm = torch.stack([flat[:, r * c.Nq: r * c.Nq + c.Nq] for r in range(c.R)], 1).double()
        w = wm if c.map_rows == c.B else wm.expand(c.B, c.R, c.Nq)
    if fault == "lane_skipped":
        w = w.clone()
        for blk in range(0, c.Nq, 128):
            lone = (w[:, :, blk: blk + 128] != 0).sum(-1, keepdim=True) < 2
            w[:, :, blk: blk + 128] = torch.where(lone, torch.zeros(()).double(), w[:, :, blk: blk + 128])
    num = torch.zeros((c.B, c.h, c.Nq, c.d), dtype=torch.float64)
    den = torch.zeros((c.B, c.h, c.Nq, 1), dtype=torch.float64)
    for r in range(c.R):
        wr = w[:, r][:, None, :, None]
        if fault != "zero_evaluated" and not bool((wr != 0).any()):
            continue
        o, l = region_term(c, bld, r, True, lo=TOK * r + fk["shift"] if fault == "off_by_one" else None)
        if fault == "joint_norm":
            num += wr * o
            den += wr * l
        elif fault == "zero_evaluated":
            num += wr * (o / l)
        else:
            num += torch.where(wr != 0, wr * o / l, torch.zeros(()).double())
    return _out(c, _r16(num / den if fault == "joint_norm" else num))


def model_fp32(c: SCase, bld):
    """an independent model of a correct kernel: fp32 arithmetic, keys in REVERSED order, regions descending"""
    scale = torch.tensor(1.0 / math.sqrt(c.d), dtype=torch.float32) * torch.tensor(A.LOG2E_F32, dtype=torch.float32)
    qs = (bld["q"] * scale).half().float()
    out = torch.zeros((c.B, c.h, c.Nq, c.d), dtype=torch.float32)
    for r in reversed(range(c.R)):
        wr = bld["w"][:, r][:, None, :, None]
        if not bool((wr != 0).any()):
            continue
        idx = torch.arange(TOK * r + TOK - 1, TOK * r - 1, -1)
        k, v = bld["k"][:, idx][None], bld["v"][:, idx][None]
        s = qs @ k.transpose(-1, -2)
        p = torch.exp2(s - s.max(-1, keepdim=True).values).half().float()
        out = torch.where(wr != 0, out + (wr / p.sum(-1, keepdim=True)) * (p @ v), out)
    return _out(c, out.half().double())


def reference(c: SCase):
    """-> bld, ref (fp64), E_model, bound: computed on the CPU, once per case"""
    bld = build(c)
    ref = ref64(c, bld)
    e_model = A.max_row_err(model(c, bld), ref, c.d)
    return bld, ref, e_model, A.FACTOR * e_model
