"""Inputs, references, the error bound and the expected dispatch of the norm / softmax kernel tests (plain torch, no HIP).

Shared by tests/test_norm_cases_cpu.py (the tables reach every instance the launchers can emit, the bound sees the faults it
is meant to see: fault models, no GPU) and tests/test_gpu_norm.py (the kernels of cfgpp_amd/csrc/norm_kernels.hip against the
same references).

Reference: ``ref64``, the op in fp64 from the fp16 inputs (GroupNorm: two-pass, biased variance, affine, optional SiLU).
``model32`` is the same op in fp32 arithmetic, left unrounded, in the kernels' form: exact two-pass statistics (every sum
exact and rounded to fp32 once - no summation order is modelled), ``mean = sum * fl(1 / count)``, ``x * sc + sh`` with ``sc = gamma * rstd`` and ``sh = beta - mean * sc`` (LayerNorm:
``mean = sum / C``, ``(x - mean) * rstd * g + b``), SiLU as ``y / (1 + exp2(-y * log2 e))``.  Every elementary function is
evaluated exactly; only the fp32 roundings of the form remain.

Per-element bound of a case, computed on the CPU by the test that uses it, never from a kernel:

    |got - ref64| <= 0.5 * ulp16(ref64) + FACTOR * A_case,       A_case = max |model32 - ref64| over the case

(ulp16: the fp16 spacing at |ref64|, floor 2^-24 - the one rounding to fp16 the kernels document; the second term covers fp32
effects).  Second statistic, kinds ``rand`` and ``groups`` only: the share of elements with got != fp16(ref64), at most
MISMATCH_CAP; the model alone must stay at or below MODEL_MISMATCH_CAP there.  The whole-tensor rel-L2 bounds of the older
tests are kept as a third assertion.

Input kinds (all values fp16-representable, seeded):
  rand     mean 0.5, sigma 2
  groups   every (sample, group) has its own sigma (0.25 .. 2) and its own mean (both signs, 0.1 .. 0.5 sigma): a chunk credited
           to the wrong group shows.  (Means of a sigma and more put x * sc + sh into cancellation: fp32 arithmetic alone then
           misses the correctly rounded fp16 value on 0.05 .. 0.15 % of the elements, above MODEL_MISMATCH_CAP.)
  offset   |mean| = 100 sigma, a different mean per group (LayerNorm: per row)
  const    constant per group (multiples of 1/4: every partial sum is exact): the variance is exactly 0, the output beta
  big      sigma 8000, near the fp16 maximum
  pivot_outlier  two-launch form only: sigma 0.01 and the value 60 at pixel (0, 0) of each group's first channel, where
           gn_pivot reads
  outlier  LayerNorm: gaussian rows, one row with a single entry of 1000
  dominant / equal / min   softmax: one entry 30 above the rest / all equal / all -65504
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace

import numpy as np
import torch

# FACTOR = 2 x 2: 2 for the kernels' summation trees differing from torch's order, 2 for rsqrtf and the hardware exp2 behind
# silu_f / the softmax, which the model evaluates exactly.  A correct kernel that exceeds it means a rounding point the model
# lacks: add it to the model, keep the 4.
# Kernel ratios (max over elements of (|got - ref64| - 0.5 ulp16) / A_case) on the MI355X, min / median / max per group of
# tests/test_gpu_norm.py (profiles/norm_cases/norm_case_parity.jsonl; <= 0: every element within half an fp16 ulp):
#   slab, cpp 5           0.01 / 0.24 / 0.98       slab, cpp 10 / 15 / 30     0.12 / 0.19 / 0.78
#   slab, two sources     0.08 / 0.21 / 0.54       slab, tokens / remap       0.07 / 0.12 / 0.15
#   form choice           0.03 / 0.16 / 0.24       two launches               0.01 / 0.21 / 0.95   (pivot_outlier 0.008)
#   producer statistics   0.04 / 0.32 / 0.94       LayerNorm                  <= 0 / 0.00 / 0.76   (auto rule 0.30 / 0.31 / 0.33)
#   softmax               <= 0 / 0.00 / 0.003
# Largest mismatch share on rand / groups inputs: 8.8e-4 (two launches), 6.5e-4 (LayerNorm), below 3.7e-4 elsewhere.
# Before the per-block median pivot the two-launch form had ratios up to 2.2 (N = 13, 64x64) and 39 480 on pivot_outlier.
FACTOR = 4.0
MISMATCH_CAP = 5e-3            # share of elements with got != fp16(ref64), kinds rand / groups
MODEL_MISMATCH_CAP = 5e-4      # the same share for fp16(model32): what a correct fp32 implementation gives (measured 0 .. 2e-4)
ORDINARY = ("rand", "groups")
# whole-tensor rel-L2 bounds of the older tests (tests/test_gpu_kernels.py, test_groupnorm_large_mean_small_variance), kept
REL_L2_BOUND = 1.5e-3
REL_L2_BOUND_TIGHT = 6e-4      # offset kinds and the producer-statistics form
LOG2E_F32 = float(np.float32(1.4426950408889634))


# ---- cases ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GN:
    N: int
    C0: int
    C1: int
    H: int
    W: int
    kind: str = "rand"
    G: int = 32
    eps: float = 1e-5
    silu: int = 0
    mode: int = 2              # cfgpp_groupnorm_set_mode: 0 auto, 1 two launches, 2 slab whenever it fits
    tokens: int = 0            # 1: token-major destination [N*H*W][C]
    pre: int = 0               # 1: cfgpp_op_groupnorm_pre (statistics of the producers)
    seed: int = 0

    @property
    def C(self):
        return self.C0 + self.C1

    @property
    def cpg(self):
        return self.C // self.G

    @property
    def id(self):
        s = f"N{self.N}C{self.C0}" + (f"+{self.C1}" if self.C1 else "") + f"x{self.H}x{self.W}-{self.kind}"
        s += f"-G{self.G}" if self.G != 32 else ""
        s += "-silu" if self.silu else ""
        s += "-eps6" if self.eps < 5e-6 else ""
        s += "-tok" if self.tokens else ""
        s += "-pre" if self.pre else f"-m{self.mode}"
        return s


@dataclass(frozen=True)
class LN:
    rows: int
    C: int
    kind: str = "rand"
    seed: int = 0

    @property
    def id(self):
        return f"r{self.rows}C{self.C}-{self.kind}"


@dataclass(frozen=True)
class SM:
    rows: int
    ncols: int
    kind: str = "rand"
    seed: int = 0

    @property
    def id(self):
        return f"r{self.rows}n{self.ncols}-{self.kind}"


_KINDS = ("rand", "groups", "offset", "const", "big")


def _spread(cases, kinds=_KINDS, base=0):
    """kinds, both eps values and SiLU on / off spread over a list of cases; one seed per case"""
    out = []
    for i, c in enumerate(cases):
        kw = dict(seed=base + i)
        if isinstance(c, GN):
            if c.kind == "rand":
                kw["kind"] = kinds[i % len(kinds)]
            kw.update(eps=(1e-5, 1e-6)[(i // 2) % 2], silu=(i + i // 3) % 2)
        out.append(replace(c, **kw))
    return out


_HW7 = ((7, 5), (8, 8), (10, 13), (12, 25), (16, 32), (25, 40), (32, 32))

# ---- GroupNorm, slab kernel (mode 2 unless stated) --------------------------------------------------------------------------
# cpp = 5 (NT 320, R 64): HW < R, MAXCH 2, 4, 8, 8, 16, 16; cpg 10 / 20 (chunks that straddle two groups, gs 4 / 2) and 40
SLAB_CPP5 = _spread([GN(2 if h * w <= 512 else 1, C, 0, h, w) for C in (320, 640, 1280) for (h, w) in _HW7], base=100)
# cpp = 10 (C = 2560): NT 320 with R 32 (MAXCH 16 at 16x32, 2 at 7x5 with a ragged second pass), NT 640 at 32x32
SLAB_CPP10 = _spread([GN(1, 2560, 0, h, w) for (h, w) in ((16, 32), (32, 32), (7, 5))], kinds=("groups", "rand", "offset"), base=200)
# cpp = 15 (NT 960, R 64): C = 960 (cpg 30, gs 4) and 1920 (cpg 60, gs 2); every MAXCH of NT 960
SLAB_CPP15 = _spread([GN(1, C, 0, h, w) for C in (960, 1920) for (h, w) in ((8, 8), (25, 40), (32, 32))]
                     + [GN(2, 960, 0, 10, 13), GN(2, 960, 0, 12, 25)], kinds=("groups", "rand", "offset", "const", "big"), base=300)
# cpp = 30 (G = 8, cpg 240): NT 960, R 32, the last row of s_col
SLAB_CPP30 = _spread([GN(1, 1920, 0, 16, 32, G=8), GN(2, 1920, 0, 7, 5, G=8, kind="groups")], kinds=("groups",), base=400)
# two sources.  320+640, 640+320, 640+1280: the source boundary and the group that straddles it lie inside one workgroup's
# channel range; 1280+1280 (cpg 80, one group per workgroup): the boundary is a workgroup edge, neighbours read different sources
SLAB_CONCAT = _spread([GN(2, a, b, h, w, kind="groups") for (a, b) in ((320, 640), (640, 320), (640, 1280), (1280, 1280))
                       for (h, w) in ((10, 13),)] + [GN(1, 320, 640, 25, 40, kind="groups"), GN(1, 640, 1280, 7, 5, kind="offset")],
                      base=500)
# token-major destination, one case of each cpp
SLAB_TOKENS = _spread([GN(2, 320, 0, 10, 13, kind="groups", tokens=1), GN(1, 2560, 0, 7, 5, kind="groups", tokens=1),
                       GN(2, 960, 0, 7, 5, kind="groups", tokens=1), GN(1, 1920, 0, 10, 13, G=8, kind="groups", tokens=1)], base=600)
# H * W = 1025.  cpp = 15 (C = 960): no slab instance fits (960 threads hold 64 rows x 16), the launcher must take the two-launch
# form even in mode 2.  cpp = 5 (C = 320) divides 640: the launcher still finds NT 640 with R = 128 rows per pass (the shuffle
# tree of block_reduce walks two rounds of 64 rows), MAXCH 16
SLAB_TOO_LARGE = _spread([GN(1, 960, 0, 25, 41, kind="groups")], base=650)
SLAB_R128 = _spread([GN(1, 320, 0, 25, 41, kind="groups")], base=660)
# auto mode: N * (G / gs) = 40 | 48 (C = 320), 32 | 48 (C = 640), 32 | 64 (C = 1280): two launches below 48 workgroups
AUTO_THRESHOLD = _spread([GN(n, C, 0, 8, 8, kind="groups", mode=0) for (C, n) in ((320, 5), (320, 6), (640, 2), (640, 3), (1280, 1), (1280, 2))],
                         base=700)
# 20 workgroups: the remainder branch of the XCD remap (G = 20, cpg 16, cpp 2)
SLAB_REMAP = _spread([GN(1, 320, 0, 10, 13, G=20, kind="groups")], base=750)

# ---- GroupNorm, two-launch form (mode 1, or where the launcher picks it anyway) ----------------------------------------------
# C = 64 and 128+64 (cpg < 8; the source boundary inside group 21), 320 (ppi 6, 16 idle threads), 2048 (256 chunks, ppi 1),
# 2560 (second channel pass).  7x5: 3 blocks, the last of 3 pixels; 4x4: nblk 1; 25x40: a partial last block; 63x65: 256 blocks,
# the last of 15 pixels; 64x64: nblk 256 (N = 2), stats ppb 32 (N = 4), 64 (N = 13, apply ppb 32); 128x128: ppb 64 and nblk 256
TWO_LAUNCH = _spread(
    [GN(2, 64, 0, 7, 5, mode=1), GN(2, 128, 64, 7, 5, mode=1), GN(2, 320, 0, 7, 5, mode=1), GN(1, 2048, 0, 7, 5, mode=1),
     GN(1, 2560, 0, 7, 5, mode=1), GN(1, 2560, 0, 4, 4, mode=1), GN(2, 64, 0, 25, 40, mode=1), GN(2, 320, 0, 25, 40, mode=1),
     GN(1, 2048, 0, 25, 40, mode=1), GN(1, 2560, 0, 25, 40, mode=1), GN(2, 64, 0, 63, 65, mode=1), GN(2, 128, 64, 63, 65, mode=1),
     GN(2, 64, 0, 64, 64, mode=1), GN(2, 320, 0, 64, 64, mode=1), GN(4, 64, 0, 64, 64, mode=1), GN(13, 64, 0, 64, 64, mode=1),
     GN(1, 64, 0, 128, 128, mode=1)], base=800)
# auto mode with cpg = 1: N * H * W = 65536 pixels, the smallest tensor with apply ppb 64
TWO_LAUNCH_APB64 = _spread([GN(16, 32, 0, 64, 64, kind="groups", mode=0)], base=850)
TWO_LAUNCH_TOKENS = _spread([GN(2, 320, 0, 25, 40, kind="groups", mode=1, tokens=1), GN(2, 128, 64, 7, 5, kind="groups", mode=1, tokens=1)],
                            base=870)
PIVOT_OUTLIER = [GN(1, 64, 0, 128, 128, kind="pivot_outlier", mode=1, seed=890)]

# ---- GroupNorm from producer statistics: HW = 32 (one block, fewer pairs than threads), 256, 1024; cpg 2, 10, 30 -------------
PRESTATS = _spread([GN(2, a, b, h, w, kind=k, pre=1) for (a, b) in ((64, 0), (320, 0), (320, 640))
                    for ((h, w), k) in (((4, 8), "groups"), ((16, 16), "offset"), ((32, 32), "const"))]
                   + [GN(2, 320, 0, 4, 8, kind="offset", pre=1), GN(2, 320, 640, 16, 16, kind="groups", pre=1),
                      GN(1, 64, 0, 32, 32, kind="groups", pre=1), GN(2, 320, 640, 4, 8, kind="const", pre=1)], base=900)

GN_GROUPS = dict(slab_cpp5=SLAB_CPP5, slab_cpp10=SLAB_CPP10, slab_cpp15=SLAB_CPP15, slab_cpp30=SLAB_CPP30, slab_concat=SLAB_CONCAT,
                 slab_tokens=SLAB_TOKENS, slab_too_large=SLAB_TOO_LARGE, slab_r128=SLAB_R128, auto_threshold=AUTO_THRESHOLD, slab_remap=SLAB_REMAP,
                 two_launch=TWO_LAUNCH, two_launch_apb64=TWO_LAUNCH_APB64, two_launch_tokens=TWO_LAUNCH_TOKENS,
                 pivot_outlier=PIVOT_OUTLIER, prestats=PRESTATS)
GN_CASES = [c for g in GN_GROUPS.values() for c in g]

# ---- LayerNorm: every case runs with rows-per-wave forced to 1, 2 and 4 ------------------------------------------------------
LN_C = (8, 64, 320, 512, 520, 1024, 1032, 1280, 1536, 1544, 2048)
LN_ROWS = (1, 3, 4, 5, 37)
LN_KINDS = ("rand", "offset", "const", "outlier")
# (seeds from 2100: in a `rand` case of a few thousand elements ONE element where fp16(model32) != fp16(ref64) is above
# MODEL_MISMATCH_CAP; with these seeds the small cases have none)
LN_TABLE = [LN(r, C, LN_KINDS[(i + j) % 4], seed=2100 + 10 * i + j) for i, C in enumerate(LN_C) for j, r in enumerate(LN_ROWS)]
LN_RPW = (1, 2, 4)
# the automatic rule: two rows per wave for C <= 320 with at least 8192 rows
LN_AUTO = [LN(8192, 320, "rand", seed=2900), LN(8191, 320, "rand", seed=2901), LN(8192, 328, "rand", seed=2902)]
LN_REFUSED = (12, 2056)

# ---- row softmax -------------------------------------------------------------------------------------------------------------
SM_NCOLS = (8, 256, 2048, 4096, 4104, 16384)
SM_KINDS = ("rand", "dominant", "equal", "min")
SM_TABLE = [SM(r, n, k, seed=3000 + 100 * i + 10 * j + m) for i, n in enumerate(SM_NCOLS) for j, r in enumerate((1, 37))
            for m, k in enumerate(SM_KINDS)]
SM_REFUSED = (12, 16392)


# ---- the launchers' dispatch rules, restated -----------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def slab_instance(cpp, HW):
    """(NT, MAXCH) of gn_slab_kernel for cpp 16-byte chunks per pixel segment and HW pixels, None when no instance fits"""
    if not (0 < cpp <= 32):
        return None
    for nt in (320, 640, 960):
        if nt % cpp == 0 and cdiv(HW, nt // cpp) <= 16:
            cpt = cdiv(HW, nt // cpp)
            return nt, 2 if cpt <= 2 else 4 if cpt <= 4 else 8 if cpt <= 8 else 16
    return None


def slab_split(c: GN):
    """(gs, cpp) of the slab kernel: the smallest gs in 1, 2, 4 whose channel range is whole chunks; (0, 0) when there is none"""
    for t in (1, 2, 4):
        if c.G % t == 0 and (t * c.cpg) % 8 == 0:
            return t, t * c.cpg // 8
    return 0, 0


def apply_ppb(N, HW):
    apb = 64
    while apb > 16 and N * cdiv(HW, apb) < 1024:
        apb >>= 1
    return apb


def stats_ppb(N, HW):
    nblk_max = max(64, min(256, cdiv(768, N)))
    ppb = 16
    while cdiv(HW, ppb) > nblk_max:
        ppb <<= 1
    return ppb, cdiv(HW, ppb)


def expected_launch_gn(c: GN):
    """cfgpp_groupnorm_last_launch after case c: (form, NT, MAXCH, gs, cpp, stats ppb, stats nblk, apply ppb)"""
    HW = c.H * c.W
    if c.pre:
        return (3, 0, 0, 0, 0, 0, 0, apply_ppb(c.N, HW))
    if c.mode != 1 and c.cpg >= 8:
        gs, cpp = slab_split(c)
        inst = slab_instance(cpp, HW) if gs else None
        if inst and (c.mode == 2 or c.N * (c.G // gs) >= 48):
            return (1, inst[0], inst[1], gs, cpp, 0, 0, 0)
    ppb, nblk = stats_ppb(c.N, HW)
    return (2, 0, 0, 0, 0, ppb, nblk, apply_ppb(c.N, HW))


def expected_launch_ln(c: LN, rpw=0):
    """cfgpp_layernorm_last_launch: (MAXV, RPW) with cfgpp_layernorm_set_rows_per_wave(rpw)"""
    need = cdiv(c.C // 8, 64)
    if need > 3:
        return (4, 1)
    r = rpw if rpw in (1, 2, 4) else (2 if c.C <= 320 and c.rows >= 8192 else 1)
    return (need, r)


def expected_launch_sm(c: SM):
    return (2 if cdiv(c.ncols // 8, 256) <= 2 else 8,)


def expected_launch(case, rpw=0):
    if isinstance(case, GN):
        return expected_launch_gn(case)
    if isinstance(case, LN):
        return expected_launch_ln(case, rpw)
    return expected_launch_sm(case)


def two_launch_loops(c: GN, ppb):
    """(the 4-unrolled pixel loop runs, its tail loop runs) for gn_stats_kernel / gn_apply_kernel with ppb pixels per block"""
    HW, chunks = c.H * c.W, c.C // 8
    ppi = max(1, 256 // chunks)
    unrolled = tail = False
    for p0 in range(0, HW, ppb):
        p1 = min(p0 + ppb, HW)
        for psub in range(ppi if chunks <= 256 else 1):
            p = p0 + psub
            while p + 3 * ppi < p1:
                unrolled = True
                p += 4 * ppi
            tail |= p < p1
    return unrolled, tail


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _h(x):
    return x.half().float()


def gn_inputs(c: GN):
    """-> x [N, H*W, C] (NHWC, both sources concatenated), gamma [C], beta [C]: fp32 tensors, x holding fp16 values"""
    g = torch.Generator().manual_seed(c.seed)
    N, HW, G, cpg = c.N, c.H * c.W, c.G, c.cpg
    z = torch.randn((N, HW, G, cpg), generator=g)
    sign = torch.where(torch.rand((N, 1, G, 1), generator=g) < 0.5, -1.0, 1.0)
    if c.kind == "rand":
        x = z * 2 + 0.5
    elif c.kind == "groups":
        sigma = 0.25 * 8.0 ** torch.rand((N, 1, G, 1), generator=g)
        x = (z + sign * (0.1 + 0.4 * torch.rand((N, 1, G, 1), generator=g))) * sigma
    elif c.kind == "offset":
        mean = sign * (20.0 + 2.0 * (torch.arange(G) % 32).float().reshape(1, 1, G, 1))
        x = z * (mean.abs() / 100) + mean
    elif c.kind == "const":
        x = (sign * torch.randint(1, 17, (N, 1, G, 1), generator=g).float() / 4).expand(N, HW, G, cpg)
    elif c.kind == "big":
        x = (z * 8000).clamp(-60000, 60000)
    elif c.kind == "pivot_outlier":
        x = z * 0.01
        x[:, 0, :, 0] = 60.0
    else:
        raise ValueError(c.kind)
    gamma = 1 + 0.3 * torch.randn(c.C, generator=g)
    beta = 0.3 * torch.randn(c.C, generator=g)
    return _h(x.reshape(N, HW, c.C)).contiguous(), gamma, beta


def ln_inputs(c: LN):
    g = torch.Generator().manual_seed(c.seed)
    z = torch.randn((c.rows, c.C), generator=g)
    if c.kind in ("rand", "outlier"):
        x = z * 2 + 0.5
        if c.kind == "outlier":
            x[c.rows // 2, (5 * c.C) // 7] = 1000.0
    elif c.kind == "offset":
        mean = (20.0 + 3.0 * (torch.arange(c.rows) % 20).float()) * torch.where(torch.arange(c.rows) % 2 == 0, 1.0, -1.0)
        x = z * (mean.abs()[:, None] / 100) + mean[:, None]
    elif c.kind == "const":
        x = (torch.randint(-16, 17, (c.rows, 1), generator=g).float() / 4).expand(c.rows, c.C)
    else:
        raise ValueError(c.kind)
    return _h(x).contiguous(), 1 + 0.3 * torch.randn(c.C, generator=g), 0.3 * torch.randn(c.C, generator=g)


def sm_inputs(c: SM):
    g = torch.Generator().manual_seed(c.seed)
    x = torch.randn((c.rows, c.ncols), generator=g) * 3
    if c.kind == "dominant":
        x[torch.arange(c.rows), (torch.arange(c.rows) * 977 + c.ncols - 1) % c.ncols] = 30.0
    elif c.kind == "equal":
        x = torch.full((c.rows, c.ncols), 1.5)
    elif c.kind == "min":
        x = torch.full((c.rows, c.ncols), -65504.0)
    return _h(x).contiguous()


def producer_stats(c: GN, x):
    """{mean, M2} per 32-pixel block and channel of x [N, HW, C], in fp64, stored as fp32 -> one [N * HW / 32, Cs, 2] per source"""
    b = x.double().reshape(c.N * c.H * c.W // 32, 32, c.C)
    mean = b.mean(1)
    st = torch.stack([mean, ((b - mean[:, None]) ** 2).sum(1)], -1).float()
    return st[:, :c.C0].contiguous(), (st[:, c.C0:].contiguous() if c.C1 else None)


# ---- reference, model, fault models --------------------------------------------------------------------------------------------
def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _silu64(y):
    return y / (1 + torch.exp(-y))


def gn_ref64(c: GN, x, gamma, beta):
    """GroupNorm(+SiLU) in fp64 -> [N, HW, C] fp64"""
    N, HW = c.N, c.H * c.W
    xg = x.double().reshape(N, HW, c.G, c.cpg)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + float(_f32(c.eps)))).reshape(N, HW, c.C) * gamma.double() + beta.double()
    return _silu64(y) if c.silu else y


def gn_model32(c: GN, x, gamma, beta, fault=None, **fk):
    """the kernels' form in fp32 arithmetic, unrounded -> [N, HW, C] fp32.

    ``fault`` injects one defect of the kind the GPU tests must catch (tests/test_norm_cases_cpu.py):
      count_off_by_one_pixel   the variance divides by cpg * (HW - 1)
      straddle_lower_group     every element of a 16-byte chunk that straddles two groups gets the lower group's statistics
      tail_in_pass2            the zero-filled pixel slots p >= HW of the slab (pad=) enter the sum of squared deviations
      rstd_rel                 rstd multiplied by 1 + rel=
    """
    N, HW, G, cpg = c.N, c.H * c.W, c.G, c.cpg
    xg = x.double().reshape(N, HW, G, cpg)
    inv_cnt = _f32(1.0) / _f32(float(cpg * HW))
    # exact two-pass statistics: every sum is exact (fp64) and rounded to fp32 once, the deviations are taken from the fp32 mean
    mean = xg.sum((1, 3), keepdim=True).float() * inv_cnt
    m2 = ((xg - mean.double()) ** 2).sum((1, 3), keepdim=True).float()
    if fault == "tail_in_pass2":
        m2 = m2 + float(fk["pad"] * cpg) * mean * mean
    if fault == "count_off_by_one_pixel":
        inv_cnt = _f32(1.0) / _f32(float(cpg * (HW - 1)))
    rstd = torch.rsqrt((m2 * inv_cnt + _f32(c.eps)).double()).float()
    if fault == "rstd_rel":
        rstd = rstd * _f32(1.0 + fk["rel"])
    mean, rstd = (t.expand(N, 1, G, cpg).reshape(N, 1, c.C) for t in (mean, rstd))
    if fault == "straddle_lower_group":
        ch = torch.arange(c.C)
        gs, _ = slab_split(c)
        base = ch - ch % (gs * cpg)                                       # first channel of the workgroup's range
        lower = (base + ((ch - base) // 8 * 8) // cpg * cpg)              # first channel of the chunk's lower group
        mean, rstd = mean[:, :, lower], rstd[:, :, lower]
    sc = gamma.float() * rstd
    sh = beta.float() - mean * sc
    y = x.float() * sc + sh
    if c.silu:
        e = torch.exp2((-y * _f32(LOG2E_F32)).double()).float()
        y = y / (1 + e)
    return y


def ln_ref64(x, gamma, beta, eps=1e-5):
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    return (xd - mean) / torch.sqrt(var + float(_f32(eps))) * gamma.double() + beta.double()


def ln_model32(x, gamma, beta, eps=1e-5, fault=None):
    """fault ``tail_row_duplicate``: the last-but-one row stored from the clamped duplicate of the last row"""
    xf = x.float()
    C = _f32(float(x.shape[1]))
    mean = x.double().sum(1, keepdim=True).float() / C                      # exact sums rounded to fp32 once, as in gn_model32
    d = xf - mean
    m2 = ((x.double() - mean.double()) ** 2).sum(1, keepdim=True).float()
    rstd = torch.rsqrt((m2 / C + _f32(eps)).double()).float()
    y = d * rstd * gamma.float() + beta.float()
    if fault == "tail_row_duplicate":
        y = y.clone()
        y[-2] = y[-1]
    return y


def sm_ref64(x):
    return torch.softmax(x.double(), -1)


def sm_model32(x):
    v = x.float() * _f32(LOG2E_F32)
    e = torch.exp2((v - v.max(1, keepdim=True).values).double()).float()
    return e * (_f32(1.0) / e.double().sum(1, keepdim=True).float())


# ---- metric ------------------------------------------------------------------------------------------------------------------
def ulp16(ref):
    """fp16 spacing at |ref| (fp64 tensor), floor 2^-24"""
    _, e = torch.frexp(ref.abs().double())
    return torch.ldexp(torch.ones_like(ref, dtype=torch.float64), (e - 11).clamp(min=-24))


def to_half(ref):
    """fp64 -> fp16 in ONE correct rounding (a conversion through fp32 rounds twice)"""
    return torch.from_numpy(ref.double().numpy().astype(np.float16))


def excess(got, ref):
    """max over elements of |got - ref64| - 0.5 ulp16(ref64); inf when got is not finite"""
    g = got.detach().double().cpu().reshape(ref.shape)
    if not bool(torch.isfinite(g).all()):
        return math.inf
    return float(((g - ref).abs() - 0.5 * ulp16(ref)).max())


def within_bound(got, ref, a_case):
    return excess(got, ref) <= FACTOR * a_case


def mismatch_share(got, ref):
    """share of elements where fp16(got) != fp16(ref64) (got: fp16 kernel output, or an unrounded model)"""
    g = got.detach().cpu().reshape(ref.shape)
    g = g if g.dtype == torch.float16 else to_half(g)
    return float((g != to_half(ref)).double().mean())


def rel_l2(got, ref):
    g, r = got.detach().double().cpu().reshape(ref.shape), ref.double()
    return float((g - r).norm() / (r.norm() + 1e-30))


def rel_l2_bound(case):
    return REL_L2_BOUND_TIGHT if isinstance(case, GN) and (case.pre or case.kind == "offset") else REL_L2_BOUND


@dataclass
class Ref:
    inputs: tuple              # GN: (x [N, HW, C], gamma, beta); LN: (x, gamma, beta); SM: (x,)
    ref: torch.Tensor          # fp64
    a_case: float              # max |model32 - ref64|
    model_mismatch: float      # share of elements with fp16(model32) != fp16(ref64)

    @property
    def slack(self):
        return FACTOR * self.a_case


@functools.lru_cache(maxsize=4)
def reference(case) -> Ref:
    """everything a test of `case` needs, computed once and shared; the tensors must be left unchanged"""
    if isinstance(case, GN):
        inp = gn_inputs(case)
        ref, mod = gn_ref64(case, *inp), gn_model32(case, *inp)
    elif isinstance(case, LN):
        inp = ln_inputs(case)
        ref, mod = ln_ref64(*inp), ln_model32(*inp)
    else:
        inp = (sm_inputs(case),)
        ref, mod = sm_ref64(*inp), sm_model32(*inp)
    return Ref(inp, ref, float((mod.double() - ref).abs().max()), mismatch_share(mod, ref))
