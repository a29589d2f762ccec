"""Cases, inputs, references and fault models for the regional cross-attention kernels (csrc/attn_kernel.hip), reached through
cfgpp_op_attention_region: xattn64_region_kernel (dispatch record: kernel 7, head dims padded to 64) and attn_region_rows_kernel
(kernel 8: every other head dim, and dp = 64 under cfgpp_attention_set_dma(0) / set_cross(0)).

Everything numeric comes from tests/attn_cases.py - the fp64 reference ``ref64``, the ``model`` of the kernels' rounding points, the
per-row metric ``max_row_err`` and FACTOR.  R = 2 .. 4 regions own the key slots [77 r, 77 r + 77); a region map names the region of
every query; the reference of a row is ``ref64`` over the row's own 77 keys, and the bound of a case is FACTOR x the model's row
error over the same keys.

Inputs (fp16-representable, seeded; "neg" rows of attn_cases: q = 0.3 randn + 6u, k = 0.3 randn - 6u, every ordinary score ~ -36 /
sqrt(d) nats) are built so that a leak is loud:
  * leak keys: local keys 0 and 76 of region r hold k = c e_r (c = 5 sqrt(d)) and a V row of +-8; a query of region rho carries
    +4 on every axis e_r, r != rho, and -4 on e_rho.  A FOREIGN leak key scores ~ +20 nats (~ 37 in the log2 domain, far beyond
    RESCALE_THR = 5, and 2^37 is beyond fp16: an unmasked P is inf), the own ones ~ -15.  They sit at both ends of every region,
    so a key range that is off by one slot in either direction admits one.
  * late keys: local key 70 of region r holds c e_(4+r) - (6 + c / sqrt(d)) u (an ordinary score for ordinary rows) and a V row of
    +-8; the rows q % 8 == 3 of region r carry +4 on e_(4+r): for them it beats every earlier own key by ~ 20 nats, in a LATER
    resident tile than the region's first key - the re-reference branch of a lane that has already seen own keys.
  * slots [77 R, K_PAD) hold the +-100 junk of attn_long_cases.junk.
Heads repeat with period min(h, 8): head i holds the k / v of base head i % period, v multiplied by 1, 2 or 4 (exact in fp16).

Kernel / E_model ratios measured on the MI355X (max row error of the kernel over the model's, min / median / max per group;
profiles/regional/attention_region_case_parity.jsonl): all in one region 0.64 / 1.00 / 1.53 (108 cases), mixed 0.97 / 1.00 / 1.02
(54), batch 0.98 / 1.00 / 1.10 (18), multiblock 0.98 / 1.00 / 1.03 (10), remap 0.98 / 0.98 / 0.99, switches 1.00 / 1.00 / 1.00 -
against the bound's FACTOR = 4.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from types import SimpleNamespace

import torch

import attn_cases as A
import attn_long_cases as L

K_PAD = L.K_PAD                # key slots of the buffers the GPU tests launch on unless a case names fewer
TOK = 77
PERIOD = 8

@dataclass(frozen=True)
class RCase:
    B: int
    h: int
    Nq: int
    d: int
    R: int
    pattern: str               # region map: "all<r>", "alt", "slab", "edge", "pair" (B = 2: two different maps)
    map_rows: int = 1
    seed: int = 0
    kernel: int = 7            # expected dispatch (cfgpp_attention_last_launch): 7 xattn64_region_kernel, 8 attn_region_rows_kernel
    xqb: int = 0               # expected 128-query blocks per workgroup (kernel 7), 0 for kernel 8
    dma: int = 1
    cross: int = 1
    k_pad: int = K_PAD

    @property
    def id(self):
        s = f"B{self.B}h{self.h}q{self.Nq}d{self.d}R{self.R}-{self.pattern}-m{self.map_rows}"
        if self.k_pad != K_PAD:
            s += f"-kp{self.k_pad}"
        if not self.dma:
            s += "-dma0"
        if not self.cross:
            s += "-cross0"
        return s

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
        """workgroups of a kernel-7 launch"""
        nqb = (self.Nq + 127) // 128
        return self.B * self.h * (nqb // self.xqb if self.xqb else nqb)


def expected_kernel(d, dma=1, cross=1):
    return 7 if (d + 31) // 32 == 2 and dma and cross else 8


def launcher_xqb(c: RCase) -> int:
    """128-query blocks per workgroup of kernel 7, by the launcher's rule restated (that of cfgpp_op_attention_cross)"""
    if c.kernel != 7:
        return 0
    return L.launcher_xqb(SimpleNamespace(Nq=c.Nq, B=c.B, h=c.h))


def _mk(B, h, Nq, d, R, pattern, map_rows=1, dma=1, cross=1, k_pad=K_PAD):
    c = RCase(B, h, Nq, d, R, pattern, map_rows=map_rows, kernel=expected_kernel(d, dma, cross), dma=dma, cross=cross, k_pad=k_pad)
    return replace(c, xqb=launcher_xqb(c))


def _seeded(cases, base):
    return [replace(c, seed=base + i) for i, c in enumerate(cases)]


D7, D8 = (40, 56, 64), (32, 80, 160)

# 1. every row in ONE region, for each region: r = R - 1 has no own key in the first resident tile(s) (the hazard of an online
#    softmax that re-references unconditionally at tile 0), r = 0 has only -inf tiles after its own; one query and a ragged block
ALL_IN_ONE = _seeded([_mk(1, 2, nq, d, R, f"all{r}") for R in (2, 3, 4) for r in range(R) for d in D7 + D8 for nq in (1, 100)], 4000)

# 2. mixed maps at Nq = 129 (two blocks, the second with one row): the region alternating per query (every lane of a wave differs),
#    a border inside a 32-row wave slab, a border exactly at the 128-query block edge
MIXED = _seeded([_mk(1, 2, 129, d, R, p) for R in (2, 3, 4) for p in ("alt", "slab", "edge") for d in D7 + D8], 4200)

# 3. two batch rows, ragged (a store past Nq would land in batch 1): a map per row (two different maps), and one map for both;
#    the buffers have exactly round_up(77 R, 64) key slots
BATCH = _seeded([_mk(2, 2, 100, d, R, p, map_rows=m, k_pad=(TOK * R + 63) // 64 * 64)
                 for R in (2, 3, 4) for (p, m) in (("pair", 2), ("alt", 1)) for d in (40, 64, 80)], 4400)

# 4. every xqb the launcher emits, at the smallest B * h * Nq that reaches it, ragged (1000) and full (1024) last block; kernel 8
#    with more than one 256-thread block
MULTIBLOCK = _seeded([_mk(1, bh, nq, d, 2 + (i + j) % 3, ("edge", "alt")[(i + j) % 2])
                      for i, (bh, nq) in enumerate(((128, 1000), (256, 1000), (512, 1000), (512, 1024))) for j, d in enumerate((40, 64))]
                     + [_mk(1, 2, 1000, 80, 3, "edge"), _mk(1, 2, 1024, 32, 4, "alt")], 4600)

# 5. the remainder branch of the block -> XCD remap: more than 8 workgroups, not a multiple of 8
REMAP = _seeded([_mk(1, 3, 300, 40, 2, "edge"),            # 9 = 3 heads x 3 query blocks
                 _mk(1, 13, 100, 64, 4, "slab")], 4700)    # 13

# 6. both A/B switches send dp = 64 to kernel 8
SWITCHES = _seeded([_mk(1, 2, 129, d, R, "slab", dma=dma, cross=cross) for (dma, cross) in ((0, 1), (1, 0)) for d in (40, 64) for R in (2, 4)], 4800)

GROUPS = dict(region_all_in_one=ALL_IN_ONE, region_mixed=MIXED, region_batch=BATCH, region_multiblock=MULTIBLOCK, region_remap=REMAP,
              region_switches=SWITCHES)
ALL_CASES = [c for g in GROUPS.values() for c in g]


# ---- region maps -------------------------------------------------------------------------------------------------------------
def region_map(c: RCase) -> torch.Tensor:
    """-> int64 [map_rows, Nq]"""
    q = torch.arange(c.Nq)
    R = c.R

    def one(p):
        if p.startswith("all"):
            return torch.full((c.Nq,), int(p[3:]), dtype=torch.long)
        if p == "alt":
            return q % R
        if p == "alt_rev":
            return (R - 1) - (q % R)
        if p == "slab":            # borders at 45, 95, 145: inside the 32-row slabs 32 .. 63, 64 .. 95 (its last row), 128 .. 159
            return torch.where(q < 45, 0, ((q - 45) // 50 + 1).clamp(max=R - 1))
        if p == "edge":            # borders at 128, 256, 384: block edges
            return (q // 128).clamp(max=R - 1)
        raise ValueError(p)
    if c.pattern == "pair":
        assert c.map_rows == 2 and c.B == 2
        return torch.stack([one("alt"), one("alt_rev")])
    return torch.stack([one(c.pattern)] * c.map_rows)


def ids_buffer(c: RCase, q_pad: int) -> torch.Tensor:
    """the uint8 [map_rows][q_pad] buffer of the op: the map, pads 0"""
    ids = torch.zeros((c.map_rows, q_pad), dtype=torch.uint8)
    ids[:, :c.Nq] = region_map(c).to(torch.uint8)
    return ids


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
LEAK_LOCAL = (0, 76)
LATE_LOCAL = 70


def build(c: RCase):
    """-> dict: q [B, P, Nq, d] (the queries of batch b for the base heads), k, v [P, K_PAD-or-k_pad slots, d] with the junk behind the
    context, base / vscale per head, maps [B, Nq]"""
    g = torch.Generator().manual_seed(c.seed)
    d, R, Nk = c.d, c.R, c.Nk
    P = min(c.h, PERIOD)
    u = torch.full((d,), d ** -0.5)
    qb = 0.3 * torch.randn((P, c.Nq, d), generator=g) + 6 * u
    k = 0.3 * torch.randn((P, Nk, d), generator=g) - 6 * u
    v = torch.randn((P, Nk, d), generator=g)
    a, cc = 4.0, 5.0 * math.sqrt(d)
    beta = -(6.0 + cc / math.sqrt(d))
    for r in range(R):
        for j, loc in enumerate(LEAK_LOCAL):
            k[:, TOK * r + loc] = 0.0
            k[:, TOK * r + loc, r] = cc
            pv = 8.0 * torch.sign(torch.randn((P, d), generator=g))
            pv[:, 0] += r + 1
            pv[:, 1] += 2 * j + 1
            v[:, TOK * r + loc] = pv
        k[:, TOK * r + LATE_LOCAL] = beta * u
        k[:, TOK * r + LATE_LOCAL, 4 + r] += cc
        pv = 8.0 * torch.sign(torch.randn((P, d), generator=g))
        pv[:, 2] += r + 1
        v[:, TOK * r + LATE_LOCAL] = pv
    maps = region_map(c)
    maps = maps if c.map_rows == c.B else maps.expand(c.B, c.Nq)
    q = qb[None].repeat(c.B, 1, 1, 1)
    rows = torch.arange(c.Nq)
    for b in range(c.B):
        mod = torch.zeros((c.Nq, d))
        mod[:, :R] = a
        mod[rows, maps[b]] = -a
        late = rows % 8 == 3
        mod[rows[late], 4 + maps[b][late]] += a
        q[b] += mod[None]
    jk, jv = L.junk(SimpleNamespace(B=1, h=P, d=d, seed=c.seed), c.k_pad - Nk)
    head = torch.arange(c.h)
    r16 = lambda x: x.half().float()
    return dict(q=r16(q), k=torch.cat([r16(k), jk], 1), v=torch.cat([r16(v), jv], 1), base=head % P, vscale=2.0 ** ((head // P) % 3),
                maps=maps, P=P)


def full_inputs(c: RCase, bld):
    """-> q [B, h, Nq, d], k, v [B, h, k_pad, d] float32 holding fp16 values: what the GPU tests upload (junk slots included)"""
    q = bld["q"][:, bld["base"]]
    k = bld["k"][bld["base"]][None].expand(c.B, -1, -1, -1)
    v = (bld["v"][bld["base"]] * bld["vscale"][:, None, None])[None].expand(c.B, -1, -1, -1)
    return q, k, v


# ---- reference, model, fault models ------------------------------------------------------------------------------------------
def _window(c: RCase, rid: int, fault, fk):
    lo = TOK * rid
    if fault == "mask_ignored":
        return torch.arange(0, c.Nk)
    if fault == "off_by_one":
        s = fk["shift"]
        return torch.arange(max(lo + s, 0), min(lo + TOK + s, c.k_pad))
    if fault == "tail_junk":
        return torch.cat([torch.arange(lo, lo + TOK), torch.arange(c.Nk, c.k_pad)])
    return torch.arange(lo, lo + TOK)


def compute(c: RCase, bld, f, fault=None, **fk):
    """f (A.ref64 or A.model) per row over the row's own keys -> [B, Nq, h * d] fp64.

    ``fault`` injects one defect of the kind the GPU tests must catch (tests/test_attention_region_cases_cpu.py):
      mask_ignored   every row's softmax runs over all 77 R keys
      off_by_one     the key range of every row is shifted by shift=+-1 slot
      neighbour_id   row q takes the region id of row q + 1
      batch0_map     batch row 1 uses batch row 0's map
      tail_junk      the slots [77 R, k_pad) enter every row's softmax
    """
    P, d = bld["P"], c.d
    out = torch.empty((c.B, c.Nq, P, d), dtype=torch.float64)
    for b in range(c.B):
        ids = bld["maps"][0 if fault == "batch0_map" else b]
        if fault == "neighbour_id":
            ids = ids[(torch.arange(c.Nq) + 1).clamp(max=c.Nq - 1)]
        for rid in ids.unique().tolist():
            rows = (ids == rid).nonzero()[:, 0]
            w = _window(c, rid, fault, fk)
            o = f(bld["q"][b][None][:, :, rows], bld["k"][None][:, :, w], bld["v"][None][:, :, w])      # [1, rows, P * d]
            out[b, rows] = o.reshape(len(rows), P, d).double()
    out = out[:, :, bld["base"]] * bld["vscale"].double()[None, None, :, None]
    return out.reshape(c.B, c.Nq, c.h * d)


def reference(c: RCase):
    """-> bld, ref (fp64), E_model, bound: computed on the CPU, once per case"""
    bld = build(c)
    ref = compute(c, bld, A.ref64)
    e_model = A.max_row_err(compute(c, bld, A.model), ref, c.d)
    return bld, ref, e_model, A.FACTOR * e_model


def online_all_masked_first_tile(c: RCase, bld):
    """The long kernel's loop on a row whose first resident tile holds no own key: the tile maximum is -inf, the unconditional
    re-reference of tile 0 takes delta = -inf, alpha = exp2(+inf) = inf, and the zero accumulators become 0 * inf = NaN.  Emulated in
    fp32 for batch 0 -> [B, Nq, h * d] with NaN in every row whose region is not in tile 0 (the honest model elsewhere)."""
    out = compute(c, bld, A.model).reshape(c.B, c.Nq, c.h, c.d).clone()
    ids = bld["maps"][0]
    first_tile_has_own = TOK * ids < 64
    acc = torch.zeros(())
    delta = torch.tensor(-math.inf)
    alpha = torch.exp2(-delta)
    out[0, ~first_tile_has_own] = (acc * alpha).double()
    return out.reshape(c.B, c.Nq, c.h * c.d)
