"""Cases, inputs, fp64 references, the per-element error bound and the expected dispatch of the implicit-GEMM tests (numpy /
torch on the CPU, no HIP).

Shared by tests/test_igemm_cases_cpu.py (the tables reach every tile and epilogue variant the launcher can emit, the fp32 model of
a correct kernel passes every condition, fault models do not: no GPU) and tests/test_gpu_igemm.py (the kernels of
csrc/igemm_kernel.hip, big4_kernel.hip and big4p_kernel.hip against the same references).

Reference: the ORIGINAL operation in fp64 from fp16-representable inputs - torch's conv2d over the (concatenated, strided, shifted,
upsampled) NCHW map with the OIHW weight, a plain matmul, ``v * gelu_erf(g)``, the head-major scatter (cfgpp_vt_pos from
hip_ops.vt_pos).  What the device reads - halo-padded NHWC sources, weights in the kernels' K order (channel-block major, tap
minor) - is built from the same arrays by device_buffers(); im2col() restates the kernels' gather over those buffers for the fp32
model, and the CPU test holds that model against the conv2d reference, so a mistake in the packing shows without a GPU.

Bound, per output element (derived; nothing here is measured but E):

    store / heads:  |got - ref64| <= 0.5 ulp16(got) + (K + ksplit + 8) 2^-23 T  [+ 0.5 ulp16(|ref64 - resid| + acc term)]
                    T = |out_scale| sum_k |a_k| |w_k| + |bias| + |temb| + |resid|          (fp64)

  0.5 ulp16(got): the rounding of the result to fp16, in the binade of the stored value.  (K + ksplit + 8) 2^-23 T: K fp32
  additions of the accumulation, ksplit of the K-split reduce, at most 8 of the epilogue (scale, bias, time embedding, residual,
  and the conversions), each relative 2^-24, with a factor 2 for the unknown order inside an MFMA.  The bracketed term exists only
  for the LDS-staged store epilogues WITH a residual: they round acc * scale + bias + temb to fp16 BEFORE the residual is added
  (torch's `conv(x) + residual` on fp16 tensors, igemm_device.h igemm_epilogue_staged) and round the sum again; that first
  rounding is half an fp16 ulp of the pre-residual value u, |u| <= |ref64 - resid| + acc term.  The generic epilogue and the
  K-split reduce add the residual in fp32 and round once: no such term.

    GEGLU:  |got - ref64| <= 0.5 ulp16(got) + |gelu(g)| dv + (|v| + dv)(1.13 dg + E) + 2^-23 |v gelu(g)|

  dv, dg: the accumulation term of the value and of the gate column; 1.13 >= max |gelu'|; E = gelu_pk_max_error(), the maximum
  absolute error of common.h's gelu_erf_pk (ported to numpy fp32 below) against the erf form on a dense grid over [-8, 8].
"""
from __future__ import annotations

import functools
import os
import re
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL_L2_BOUND = 1.5e-3          # the whole-tensor bound of the older tests (tests/test_gpu_kernels.py), kept
EPI_STORE, EPI_GEGLU, EPI_HEADS = 0, 1, 2
LDS = 160 * 1024
PAR_NB = 5
WS_BYTES = 128 << 20


def cdiv(a, b):
    return (a + b - 1) // b


def round_up(a, b):
    return cdiv(a, b) * b


# ---- B1: cases ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Problem:
    """one operation on one shape: everything the inputs and the reference depend on"""
    op: str = "store"          # store | geglu | heads
    amode: int = 0             # 0 token rows, 1 padded NHWC, 2 stride 2, 3 fused nearest-2x upsample
    taps: int = 1
    B: int = 1                 # samples (amode >= 1, padded token destinations, heads)
    H: int = 0                 # OUTPUT map (amode >= 1; amode 0 with H > 0: token rows into a padded destination)
    W: int = 0
    Hs: int = 0                # amode 2: the true source size (odd sizes leave the buffer's last row / column zero)
    Ws: int = 0
    M: int = 0                 # rows of a plain token GEMM (H == 0)
    C0: int = 64
    C1: int = 0
    N: int = 64
    bias: int = 0
    temb: int = 0
    resid: int = 0
    ashift: int = 0
    out_scale: float = 1.0
    tokens: int = 0            # heads: tokens per sample
    head_dim: int = 0
    nheads: int = 0
    part0: int = 1             # heads: part of column 0 (0 Q, 1 K); parts part0 .. 2
    vt_linear: int = 0
    seed: int = 0

    @property
    def rows(self):
        if self.op == "heads":
            return self.B * self.tokens
        return self.B * self.H * self.W if self.H else self.M

    @property
    def Cin(self):
        return self.C0 + self.C1

    @property
    def K(self):
        return self.taps * self.Cin

    @property
    def padded(self):
        return self.H > 0

    @property
    def part_width(self):
        return self.nheads * self.head_dim

    @property
    def n_out(self):
        return self.N // 2 if self.op == "geglu" else self.N

    @property
    def epi(self):
        return {"store": EPI_STORE, "geglu": EPI_GEGLU, "heads": EPI_HEADS}[self.op]

    @property
    def id(self):
        if self.op == "heads":
            s = f"heads{self.B}x{self.tokens}t-d{self.head_dim}h{self.nheads}p{self.part0}" + ("-lin" if self.vt_linear else "")
        elif self.H:
            s = f"a{self.amode}t{self.taps}-{self.B}x{self.H}x{self.W}"
            s += f"-src{self.Hs}x{self.Ws}s{self.ashift}" if self.amode == 2 else ""
        else:
            s = f"{'geglu' if self.op == 'geglu' else 'lin'}-M{self.M}"
        s += f"-N{self.N}-C{self.C0}" + (f"+{self.C1}" if self.C1 else "")
        s += "".join(t for t, on in (("b", self.bias), ("t", self.temb), ("r", self.resid)) if on)
        s += f"-s{self.out_scale:g}" if self.out_scale != 1.0 else ""
        return s


@dataclass(frozen=True)
class Case:
    """a problem and the launcher switches it runs under"""
    group: str
    p: Problem
    cfg: int = 0               # cfgpp_igemm_force_config (0: the heuristic)
    split: int = 0             # cfgpp_igemm_force_split
    staging: int = 1           # cfgpp_igemm_set_staging
    staged_epi: int = 1        # cfgpp_igemm_set_staged_epilogue
    n_major: int = -1          # cfgpp_igemm_set_n_major
    blocked: int = 1           # cfgpp_igemm_set_blocked_walk
    tail_split: int = 1        # cfgpp_igemm_set_tail_split
    hint: int = 0              # IGemmArgs::cfg_hint
    gstat: int = 0             # 1: a statistics buffer is offered (cfgpp_op_igemm_set_gstat)

    @property
    def id(self):
        s = f"{self.group}-{self.p.id}-c{self.cfg}"
        s += f"-S{self.split}" if self.split else ""
        s += "-reg" if not self.staging else ""
        s += "-gen" if not self.staged_epi else ""
        s += f"-nm{self.n_major}" if self.n_major >= 0 else ""
        s += "-1d" if not self.blocked else ""
        s += "-nots" if not self.tail_split else ""
        s += f"-h{self.hint}" if self.hint else ""
        s += "-gst" if self.gstat else ""
        return s


# cfg -> (family, WM, WN, WTM, WTN, stages): the table of launch_config's switch (igemm_kernel.hip).  Family 1 igemm_kernel (64-deep
# K-tiles), 2 tile32_kernel (32-deep), 3 igemm16_kernel, 4 big4_kernel, 5 big4p_kernel.  Fifth entry of family 2: waves per SIMD.
TILES = {
    1: (1, 2, 2, 64, 64, 2), 2: (1, 4, 1, 64, 64, 2), 3: (1, 2, 2, 32, 32, 2), 4: (1, 2, 4, 128, 64, 2), 5: (1, 4, 2, 64, 160, 2),
    6: (1, 4, 2, 64, 64, 2), 7: (1, 4, 1, 32, 160, 2), 8: (1, 4, 2, 32, 160, 2), 9: (1, 4, 1, 32, 160, 3), 10: (1, 8, 1, 32, 320, 2),
    11: (1, 4, 1, 32, 160, 4), 12: (1, 2, 2, 64, 64, 3), 14: (1, 4, 2, 64, 64, 3),
    13: (2, 2, 4, 128, 64, 4), 15: (2, 4, 2, 64, 64, 3), 16: (2, 2, 2, 64, 64, 3), 17: (2, 4, 1, 64, 64, 3), 20: (2, 4, 2, 64, 160, 4),
    27: (2, 2, 2, 64, 160, 2),
    18: (3, 4, 2, 32, 80, 3), 19: (3, 4, 2, 32, 80, 4),
    24: (4, 2, 2, 128, 128, 2), 25: (4, 2, 2, 64, 160, 2), 26: (4, 2, 2, 64, 128, 2), 28: (5, 2, 4, 128, 64, 2),
}
T32_WPE = {13: 2, 15: 4, 16: 3, 17: 2, 20: 2, 27: 2}
STORE_CONFIGS = tuple(range(1, 21)) + (24, 25, 26, 27, 28)


def tile_bm_bn(cfg):
    _, WM, WN, WTM, WTN, _ = TILES[cfg]
    return WM * WTM, WN * WTN


def _tiles_store():
    out = []
    for cfg in STORE_CONFIGS:
        BM, BN = tile_bm_bn(cfg)
        nst = TILES[cfg][5]
        n = 320 if cfg in (18, 19) else BN + 64                    # ragged N where the tile admits it
        for kt in sorted({1, 2, nst, nst + 1}):                      # 64-channel blocks: 2 kt K-tiles on the 32-deep rings
            p = Problem(M=BM + 44, N=n, C0=64 * kt, bias=1, resid=1, seed=1)
            out.append(Case("tiles_store", p, cfg=cfg))
            if cfg != 1:
                out.append(Case("tiles_store", p, cfg=1))             # the bits every whole-tile config must reproduce
    # conv3x3 + bias + time embedding + padded residual, 12 x 10 map (W no power of two), two samples: a tile straddles them
    p = Problem(amode=1, taps=9, B=2, H=12, W=10, C0=64, N=320, bias=1, temb=1, resid=1, seed=2)
    out += [Case("tiles_store", p, cfg=cfg) for cfg in STORE_CONFIGS]
    seen, uniq = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq


def _tiles_fallback():
    out = []
    lin = Problem(M=172, N=192, C0=128, bias=1, resid=1, seed=3)
    out += [Case("tiles_fallback", lin, cfg=c) for c in (18, 19)]                          # N % 160 != 0 -> 4-wave 128 x 160
    out += [Case("tiles_fallback", lin, cfg=c, staged_epi=0) for c in (24, 25, 26, 28)]  # no staged epilogue -> 128 x 128
    conv = Problem(amode=1, taps=9, B=2, H=12, W=10, C0=64, N=320, bias=1, temb=1, resid=1, seed=2)
    out.append(Case("tiles_fallback", conv, cfg=28))                                      # not a token-major linear -> 128 x 128
    gg = Problem(op="geglu", M=172, N=256, C0=128, bias=1, seed=4)
    out += [Case("tiles_fallback", gg, cfg=c) for c in (27, 20, 25)]                      # 32-deep 128 x 128 / 256 x 256; no GEGLU pairs
    # time-embedding rows of a tile that do not fit the LDS (feature maps under 8 x 8): 64 x 64 or 128 x 128 runs instead
    for (b, h, w) in ((40, 4, 4), (70, 2, 2)):
        p = Problem(amode=1, taps=9, B=b, H=h, W=w, C0=64, N=320, bias=1, temb=1, resid=1, seed=5)
        out += [Case("tiles_fallback", p, cfg=c) for c in (1, 3, 4, 5, 6, 7, 11, 13, 14, 15, 16, 17, 19, 20, 24)]
    return out


_AMODE_CFGS = (1, 3, 16, 19, 24)


def _amodes():
    ps = []
    for (hs, ws) in ((12, 10), (11, 9)):
        for sh in (0, 1):
            h = (hs + (1 if sh else 2) - 3) // 2 + 1
            w = (ws + (1 if sh else 2) - 3) // 2 + 1
            ps.append(Problem(amode=2, taps=9, B=5, H=h, W=w, Hs=hs, Ws=ws, ashift=sh, C0=64, N=160, bias=1, resid=1, seed=6))
    ps.append(Problem(amode=3, taps=9, B=2, H=12, W=10, C0=64, N=160, bias=1, seed=7))
    ps.append(Problem(amode=1, taps=1, B=2, H=12, W=10, C0=64, C1=128, N=160, bias=1, seed=8))
    ps.append(Problem(amode=1, taps=9, B=2, H=12, W=10, C0=64, C1=128, N=160, bias=1, temb=1, seed=9))
    ps.append(Problem(amode=0, B=2, H=12, W=10, C0=128, N=160, bias=1, resid=1, seed=10))      # token rows into a padded map
    return [Case("amodes", p, cfg=c) for p in ps for c in _AMODE_CFGS]


def _heads(tokens, d, h, part0=1, lin=0, seed=11):
    return Problem(op="heads", B=2, tokens=tokens, head_dim=d, nheads=h, part0=part0, vt_linear=lin, C0=128,
                   N=(3 - part0) * d * h, bias=1, seed=seed)


def _epilogues_generic():
    out = []
    for cfg in (1, 6, 16):
        out.append(Case("epilogues_generic", Problem(M=300, N=192, C0=128, bias=1, resid=1, seed=12), cfg=cfg, staged_epi=0))
        out.append(Case("epilogues_generic", Problem(amode=1, taps=9, B=2, H=12, W=10, C0=64, N=192, bias=1, temb=1, resid=1, seed=13),
                        cfg=cfg, staged_epi=0))
        for n in (68, 132):
            out.append(Case("epilogues_generic", Problem(M=172, N=n, C0=128, bias=1, resid=1, seed=14), cfg=cfg))
        for n in (192, 320):
            out.append(Case("epilogues_generic", Problem(op="geglu", M=172, N=n, C0=128, bias=1, seed=15), cfg=cfg))
        out.append(Case("epilogues_generic", Problem(op="geglu", M=172, N=256, C0=128, bias=1, seed=4), cfg=cfg, staged_epi=0))
        for (d, h) in ((40, 2), (64, 2), (160, 2)):
            for lin in (0, 1):
                out.append(Case("epilogues_generic", _heads(77, d, h, lin=lin), cfg=cfg))
        out.append(Case("epilogues_generic", _heads(64, 64, 2, part0=0), cfg=cfg, staged_epi=0))
        out.append(Case("epilogues_generic", _heads(64, 40, 2), cfg=cfg))                 # part_width % 32 != 0 alone
        out.append(Case("epilogues_generic", _heads(64, 36, 8), cfg=cfg))                 # head_dim % 8 != 0 alone
        out.append(Case("epilogues_generic", Problem(M=172, N=192, C0=128, bias=1, out_scale=0.125, seed=16), cfg=cfg, staged_epi=0))
    return out


def _epilogues_staged():
    out = []
    for cfg in (1, 6, 16, 24, 28):
        out.append(Case("epilogues_staged", Problem(M=300, N=192, C0=128, bias=1, resid=1, seed=12), cfg=cfg))
        out.append(Case("epilogues_staged", Problem(M=320, N=192, C0=128, bias=1, resid=1, seed=17), cfg=cfg, gstat=1))
        out.append(Case("epilogues_staged", Problem(amode=1, taps=9, B=2, H=12, W=10, C0=64, N=192, bias=1, temb=1, resid=1, seed=13), cfg=cfg))
        for n in (256, 384):
            out.append(Case("epilogues_staged", Problem(op="geglu", M=172, N=n, C0=128, bias=1, seed=4 if n == 256 else 18), cfg=cfg))
        for (d, h) in ((40, 4), (64, 2), (160, 2)):
            for lin in (0, 1):
                out.append(Case("epilogues_staged", _heads(64, d, h, lin=lin), cfg=cfg))
        out.append(Case("epilogues_staged", _heads(64, 64, 2, part0=0), cfg=cfg))
        out.append(Case("epilogues_staged", Problem(M=172, N=192, C0=128, bias=1, out_scale=0.125, seed=16), cfg=cfg))
    for cfg in (18, 19):                                                                  # 16x16x32 tile: N % 160 == 0
        out.append(Case("epilogues_staged", Problem(M=172, N=320, C0=128, bias=1, out_scale=0.125, seed=19), cfg=cfg))
        out.append(Case("epilogues_staged", Problem(M=320, N=320, C0=128, bias=1, resid=1, seed=20), cfg=cfg, gstat=1))
        for lin in (0, 1):
            out.append(Case("epilogues_staged", _heads(64, 160, 2, lin=lin), cfg=cfg))
        out.append(Case("epilogues_staged", _heads(64, 40, 4, part0=0), cfg=cfg))
    return out


def _staging():
    lin = Problem(M=172, N=192, C0=192, bias=1, resid=1, seed=21)
    conv = Problem(amode=1, taps=9, B=2, H=12, W=10, C0=64, N=192, bias=1, temb=1, resid=1, seed=13)
    s2 = Problem(amode=2, taps=9, B=5, H=6, W=5, Hs=11, Ws=9, ashift=0, C0=64, N=160, bias=1, resid=1, seed=6)
    gg = Problem(op="geglu", M=172, N=256, C0=128, bias=1, seed=4)
    out = []
    for p in (lin, conv, s2, gg, _heads(77, 40, 2)):
        out += [Case("staging", p, cfg=c) for c in (21, 22, 23) if not (p.op == "geglu" and c == 23)]
        out += [Case("staging", p, cfg=c, staging=0) for c in (1, 2, 3) if not (p.op == "geglu" and c == 3)]
        out.append(Case("staging", p, cfg=1))
    return out


def _ksplit():
    out = []
    for cfg in (1, 12, 14, 8):
        BM, BN = tile_bm_bn(cfg)
        p = Problem(M=BM + 44, N=BN + 64, C0=384, bias=1, resid=1, seed=22)
        out += [Case("ksplit", p, cfg=cfg, split=s) for s in (2, 3, 6)]
        out.append(Case("ksplit", p, cfg=cfg, split=2, gstat=1))                          # a K-split launch writes no statistics
        conv = Problem(amode=1, taps=9, B=2, H=12, W=10, C0=64, N=192, bias=1, temb=1, resid=1, seed=13)
        out.append(Case("ksplit", conv, cfg=cfg, split=3))
        # the tail rule (few tiles, K >= 2048 on the 64 x 64 wave tiles): 2 slices at K = 2048, 5 at K = 4096; config 8 never splits
        for k in (2048, 4096):
            t = Problem(M=BM + 44, N=BN + 64, C0=k, bias=1, resid=1, seed=23)
            out.append(Case("ksplit", t, cfg=cfg))
        out.append(Case("ksplit", Problem(M=BM + 44, N=BN + 64, C0=2048, bias=1, resid=1, seed=23), cfg=cfg, tail_split=0))
    return out


WALK_SHAPE = Problem(M=500, N=512, C0=128, bias=1, seed=24)       # 8 x 8 tiles of 64 x 64 (config 3): T = 64, ragged last M-tile


def _walks():
    p = WALK_SHAPE
    return [Case("walks", p, cfg=3, blocked=0, n_major=0), Case("walks", p, cfg=3, blocked=0, n_major=1), Case("walks", p, cfg=3),
            Case("walks", p, cfg=3, n_major=1), Case("walks", p, cfg=1)]


def _heuristic():
    small = Problem(M=100, N=64, C0=64, bias=1, seed=25)                                   # -> 64 x 64 (config 3)
    gg = Problem(op="geglu", M=100, N=128, C0=64, bias=1, seed=26)                        # -> 3, then 1: GEGLU needs 64-wide wave tiles
    tail = Problem(M=300, N=384, C0=2048, bias=1, resid=1, seed=27)                       # 9 tiles of 128 x 128, KT = 32 -> 14, K-split
    lin = Problem(M=300, N=192, C0=128, bias=1, resid=1, seed=12)
    return [Case("heuristic", small), Case("heuristic", gg), Case("heuristic", tail), Case("heuristic", tail, tail_split=0),
            Case("heuristic", lin, hint=6), Case("heuristic", lin, hint=16), Case("heuristic", lin, hint=6 | (2 << 6)),
            Case("heuristic", lin, hint=28), Case("heuristic", tail, hint=1),              # the rule splits: the hint does not run
            Case("heuristic", gg, hint=5), Case("heuristic", gg, hint=10),                 # 5: invalid for GEGLU; 10: valid
            Case("heuristic", lin, hint=10)]                                               # 10: invalid for a plain store


GROUPS = {
    "tiles_store": _tiles_store(), "tiles_fallback": _tiles_fallback(), "amodes": _amodes(), "epilogues_generic": _epilogues_generic(),
    "epilogues_staged": _epilogues_staged(), "staging": _staging(), "ksplit": _ksplit(), "walks": _walks(), "heuristic": _heuristic(),
}


def all_cases():
    return [c for g in GROUPS.values() for c in g]


# ---- B2: inputs ----------------------------------------------------------------------------------------------------------------
def _h(a):
    """round to fp16, keep as fp64"""
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


@functools.lru_cache(maxsize=None)
def inputs(p: Problem):
    """fp16-representable values as fp64: sources (NCHW or [rows, K]), the weight in checkpoint order (OIHW / [N, K]; GEGLU and
    heads: the kernels' column order), bias [N], temb [B, N], resid [rows, N] in output row order (sample, y, x)"""
    g = np.random.default_rng(1000 + p.seed)
    r = SimpleNamespace()
    if p.amode == 0:
        r.a = _h(g.standard_normal((p.rows, p.K)))
        r.w = _h(g.standard_normal((p.N, p.K)) * p.K ** -0.5 * (1.5 if p.op == "geglu" else 1.0))
    else:
        hs, ws = (p.Hs, p.Ws) if p.amode == 2 else (p.H // 2, p.W // 2) if p.amode == 3 else (p.H, p.W)
        r.x = [_h(g.standard_normal((p.B, c, hs, ws))) for c in (p.C0, p.C1) if c]
        kk = 3 if p.taps == 9 else 1
        r.w = _h(g.standard_normal((p.N, p.Cin, kk, kk)) * p.K ** -0.5)
    r.bias = _h(g.standard_normal(p.N) * 0.1) if p.bias else None
    r.temb = _h(g.standard_normal((p.B, p.N)) * 0.5) if p.temb else None
    r.resid = _h(g.standard_normal((p.rows, p.N))) if p.resid else None
    return r


def pack_weight(p: Problem, w):
    """checkpoint order -> [N, K] in the kernels' K order: k = (cb * taps + tap) * 64 + c, cb = 64-channel block of the concatenated
    input (cfgpp_debug.h)"""
    if p.amode == 0:
        return w
    n, cin, kh, kw = w.shape
    return w.transpose(0, 2, 3, 1).reshape(n, kh * kw, cin // 64, 64).transpose(0, 2, 1, 3).reshape(n, kh * kw * cin)


@functools.lru_cache(maxsize=None)
def device_buffers(p: Problem):
    """what the device reads, as numpy fp16: `src` (one or two halo-padded NHWC maps with ZERO halos, or the token rows), `w` [N, K]
    packed, `resid` in the destination's layout (padded: zero halo), bias / temb fp32"""
    i = inputs(p)
    d = SimpleNamespace(bias=None, temb=None, resid=None)
    if p.amode == 0:
        d.src = [i.a.astype(np.float16)]
    else:
        d.src = []
        for x in i.x:
            b, c, hs, ws = x.shape
            hb, wb = (2 * p.H + 2, 2 * p.W + 2) if p.amode == 2 else (hs + 2, ws + 2)
            buf = np.zeros((b, hb, wb, c), dtype=np.float16)
            buf[:, 1:1 + hs, 1:1 + ws] = x.transpose(0, 2, 3, 1)
            d.src.append(buf)
    d.w = np.ascontiguousarray(pack_weight(p, i.w)).astype(np.float16)
    if p.bias:
        d.bias = i.bias.astype(np.float32)
    if p.temb:
        d.temb = i.temb.astype(np.float32)
    if p.resid:
        if p.padded:
            d.resid = np.zeros((p.B, p.H + 2, p.W + 2, p.N), dtype=np.float16)
            d.resid[:, 1:-1, 1:-1] = i.resid.reshape(p.B, p.H, p.W, p.N)
        else:
            d.resid = i.resid.astype(np.float16)
    return d


def im2col(p: Problem, ashift=None):
    """[rows, K] fp32: the kernels' gather (igemm_device.h a_row_map / a_gather / a_gather_pix) over device_buffers(p).src, K-tile by K-tile"""
    d = device_buffers(p)
    ashift = p.ashift if ashift is None else ashift
    flat = [s.reshape(-1, s.shape[-1]).astype(np.float32) for s in d.src]
    if p.amode == 0:
        return flat[0]
    m = np.arange(p.rows)
    b, q = np.divmod(m, p.H * p.W)
    y, x = np.divmod(q, p.W)
    a = np.empty((p.rows, p.K), dtype=np.float32)
    for kt in range(p.K // 64):
        cb, tap = divmod(kt, 9) if p.taps == 9 else (kt, 0)
        cc = cb * 64
        src, cs = (flat[0], cc) if cc < p.C0 else (flat[1], cc - p.C0)
        dy, dx = (tap // 3 - 1, tap % 3 - 1) if p.taps == 9 else (0, 0)
        if p.amode == 1:
            pix = (b * (p.H + 2) + y + 1) * (p.W + 2) + x + 1 + dy * (p.W + 2) + dx
        elif p.amode == 2:
            pix = (b * (2 * p.H + 2) + 2 * y + 1 + ashift) * (2 * p.W + 2) + 2 * x + 1 + ashift + dy * (2 * p.W + 2) + dx
        else:
            pix = (b * (p.H // 2 + 2) + ((y + dy) >> 1) + 1) * (p.W // 2 + 2) + ((x + dx) >> 1) + 1
        a[:, kt * 64:(kt + 1) * 64] = src[pix, cs:cs + 64]
    return a


# ---- the GELU of the GEGLU epilogues ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gelu_consts():
    src = open(os.path.join(ROOT, "cfgpp_amd", "csrc", "common.h")).read()
    c = np.float32(re.search(r"#define CFGPP_GELU_C ([0-9.]+)f", src).group(1))
    body = re.search(r"#define CFGPP_GELU_POLY \{(.*?)\}", src, re.S).group(1).replace("\\", " ")
    return c, tuple(np.float32(v.strip().rstrip("f")) for v in body.split(","))


def gelu_erf_pk(x):
    """common.h gelu_erf_pk in numpy fp32: clamp, centred variable (one fma), Horner with one rounding per fma, |x| * p, one fma"""
    c, k = _gelu_consts()
    x = np.asarray(x, dtype=np.float32)
    a = np.minimum(np.abs(x), c)
    t = (a.astype(np.float64) * np.float64(np.float32(2.0) / c) - 1.0).astype(np.float32)
    pp = np.full_like(t, k[12])
    for kk in k[11::-1]:
        pp = (pp.astype(np.float64) * t + np.float64(kk)).astype(np.float32)
    mm = np.abs(x) * pp
    return (x.astype(np.float64) * 0.5 + mm).astype(np.float32)


def gelu64(g):
    from scipy.special import erf
    g = np.asarray(g, dtype=np.float64)
    return g * 0.5 * (1.0 + erf(g / np.sqrt(2.0)))


@functools.lru_cache(maxsize=None)
def gelu_pk_max_error():
    """E: max |gelu_erf_pk(x) - x Phi(x)| over fp32 x on a grid of step 2^-17 over [-8, 8] and around the breakpoint c = 4.75"""
    c, _ = _gelu_consts()
    x = np.arange(-8 * 2 ** 17, 8 * 2 ** 17 + 1, dtype=np.float64) * 2.0 ** -17
    near = float(c) + np.arange(-4096, 4097) * 2.0 ** -21
    x = np.concatenate([x, near, -near]).astype(np.float32)
    return float(np.abs(gelu_erf_pk(x).astype(np.float64) - gelu64(x.astype(np.float64))).max())


# ---- B3: reference -------------------------------------------------------------------------------------------------------------
def vt_pos(n):
    import hip_ops
    return hip_ops.vt_pos(n).numpy()


def _gemm64(p: Problem, absolute=False):
    """[rows, N] fp64: the convolution / matmul alone, of the values or of their magnitudes"""
    i = inputs(p)
    f = np.abs if absolute else (lambda v: v)
    if p.amode == 0:
        return f(i.a) @ f(i.w).T
    x = torch.from_numpy(f(np.concatenate(i.x, axis=1)))
    w = torch.from_numpy(f(i.w))
    if p.amode == 1:
        y = F.conv2d(x, w, padding=1 if p.taps == 9 else 0)
    elif p.amode == 2:
        y = F.conv2d(F.pad(x, (0, 1, 0, 1) if p.ashift else (1, 1, 1, 1)), w, stride=2)
    else:
        y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    assert tuple(y.shape) == (p.B, p.N, p.H, p.W), (p, tuple(y.shape))
    return y.permute(0, 2, 3, 1).reshape(p.rows, p.N).numpy()


def _batch_of_rows(p: Problem):
    return np.arange(p.rows) // (p.H * p.W if p.H else p.rows)


@functools.lru_cache(maxsize=None)
def reference(p: Problem):
    """fp64: ref [rows, n_out] of the original operation; T (store / heads) or v, g, Tv, Tg (GEGLU) for the bound; pre = ref before the
    residual"""
    i = inputs(p)
    r = SimpleNamespace()
    y = _gemm64(p) * (p.out_scale if p.op == "store" else 1.0)
    t = _gemm64(p, absolute=True) * (abs(p.out_scale) if p.op == "store" else 1.0)
    if p.bias:
        y = y + i.bias
        t = t + np.abs(i.bias)
    if p.op == "geglu":
        f = np.arange(p.N // 2)
        pv = (f // 32) * 64 + f % 32                                    # feature f: value column pv, gate column pv + 32
        r.v, r.g, r.Tv, r.Tg = y[:, pv], y[:, pv + 32], t[:, pv], t[:, pv + 32]
        r.ref = r.v * gelu64(r.g)
        return r
    if p.temb:
        tb = i.temb[_batch_of_rows(p)]
        y = y + tb
        t = t + np.abs(tb)
    r.pre = y
    if p.resid:
        y = y + i.resid
        t = t + np.abs(i.resid)
    r.ref, r.T = y, t
    return r


def heads_layout(p: Problem):
    """the head-major destinations of p (include/cfgpp.h): shapes of hq / hk / hvt and, per (row, column) of the [rows, N] projection,
    the buffer (part 0 / 1 / 2) and the flat offset inside it.  V^T key positions: hip_ops.vt_pos, or the identity with vt_linear"""
    d, h, c = p.head_dim, p.nheads, p.part_width
    dp, qp, kp = round_up(d, 32), round_up(p.tokens, 128), round_up(p.tokens, 64)
    m, n = np.meshgrid(np.arange(p.rows), np.arange(p.N), indexing="ij")
    b, tok = np.divmod(m, p.tokens)
    part = n // c + p.part0
    head, dd = np.divmod(n % c, d)
    bh = b * h + head
    pos = np.arange(kp) if p.vt_linear else vt_pos(kp)
    off = np.where(part == 2, (bh * dp + dd) * kp + pos[tok], (bh * np.where(part == 0, qp, kp) + tok) * dp + dd)
    shapes = {0: (p.B * h, qp, dp), 1: (p.B * h, kp, dp), 2: (p.B * h, dp, kp)}
    return SimpleNamespace(shapes=shapes, part=part, off=off, parts=tuple(range(p.part0, 3)))


# ---- B4: bound -----------------------------------------------------------------------------------------------------------------
def ulp16(v):
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def bound(c: Case, got):
    """per element of got [rows, n_out] (module docstring)"""
    p, r = c.p, reference(c.p)
    rep = expected_launch(c)
    ksplit, variant = rep[7], rep[13]
    k = (p.K + ksplit + 8) * 2.0 ** -23
    if p.op == "geglu":
        dv, dg = k * r.Tv, k * r.Tg
        gl = np.abs(gelu64(r.g))
        return 0.5 * ulp16(got) + gl * dv + (np.abs(r.v) + dv) * (1.13 * dg + gelu_pk_max_error()) + 2.0 ** -23 * np.abs(r.v) * gl
    b = 0.5 * ulp16(got) + k * r.T
    if p.op == "store" and p.resid and variant == 1:
        b = b + 0.5 * ulp16(np.abs(r.pre) + k * r.T)                   # the staged epilogue's fp16 rounding before the residual
    return b


def rel_l2(got, ref):
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))


# ---- B5: the launcher's dispatch, restated (igemm_kernel.hip igemm_launch .. launch_*) ----------------------------------------------
def par_bnp(BN):
    return (BN + 63) // 64 * 64


def par_bytes(BN, nb=PAR_NB):
    return par_bnp(BN) * 4 * (1 + nb)


def _args(c: Case):
    p = c.p
    a = SimpleNamespace(M=p.rows, N=p.N, K=p.K, C0=p.C0, C1=p.C1, taps=p.taps, amode=p.amode, H=p.H, W=p.W, epi=p.epi,
                        bias=bool(p.bias), temb=bool(p.temb), resid=bool(p.resid), omode=1 if p.padded else 0,
                        rpb=p.tokens if p.op == "heads" else p.H * p.W, part_width=p.part_width, head_dim=p.head_dim,
                        gstat=bool(c.gstat) and p.op != "heads", cfg_hint=c.hint, split=0, allow_split=1, walk_hint=0,
                        n_main=0, ksplit=1, n_major=0, walk_bn=0, par_nb=0, staged_epi=1)
    return a


def _par_slots(a, BM):
    if not a.temb or a.rpb <= 0:
        return 0
    span = (BM + a.rpb - 1) // a.rpb + 1
    return min(span, cdiv(a.M, a.rpb))


def _a_traffic(a):
    return 4.0 if a.amode == 2 else 0.25 if a.amode == 3 else 1.0


def _n_major(a, c, ntn, a_bytes=None):
    w_bytes = 2.0 * a.N * a.K
    a_bytes = 2.0 * a.M * (a.C0 + a.C1) * _a_traffic(a) if a_bytes is None else a_bytes
    nm = 1 if (c.n_major == 1 or (c.n_major < 0 and w_bytes > 1.5 * a_bytes and ntn >= 8)) else 0
    if c.n_major < 0 and a.walk_hint:
        nm = 1 if a.walk_hint == 2 else 0
    return nm


def walk_plan(M, N, K, Cin, BM, BN, smem, n_major, traffic=1.0):
    """igemm_kernel.hip walk_plan for whole-tile launches without a pinned walk -> (walk_bn, tmb, tnb, n_major)"""
    ntm, ntn = cdiv(M, BM), cdiv(N, BN)
    T = ntm * ntn
    if (T & 7) or T < 64 or ntm > 512 or ntn > 512:
        return 0, 0, 0, n_major
    per = T >> 3
    wpc = min(max(LDS // smem if smem > 0 else 1, 1), 4)
    R = 32 * wpc
    a_row, w_col = 2.0 * BM * Cin * traffic, 2.0 * BN * K

    def cost(tile_at):
        tot = 0.0
        for r0 in range(0, per, R):
            tiles = [tile_at(i) for i in range(r0, min(per, r0 + R))]
            tot += len({t[0] for t in tiles}) * a_row + len({t[1] for t in tiles}) * w_col
        return tot

    div1 = ntm if n_major else ntn
    now = cost(lambda i: (i % div1, i // div1) if n_major else (i // div1, i % div1))
    best, pick = now, None
    for bn in (4, 2):
        bm = 8 // bn
        if ntm % bm or ntn % bn:
            continue
        tmb, tnb = ntm // bm, ntn // bn
        for inner in (0, 1):
            cst = cost((lambda i: (i % tmb, i // tmb)) if inner else (lambda i: (i // tnb, i % tnb)))
            if cst < best:
                best, pick = cst, (bn, tmb, tnb, inner)
    if pick and best <= 0.85 * now:
        return pick
    return 0, 0, 0, n_major


def _walk(a, c, BM, BN, smem):
    a.walk_bn = 0
    T = cdiv(a.M, BM) * cdiv(a.N, BN)
    if not c.blocked or a.walk_hint or a.ksplit > 1 or a.n_main != T:
        return
    a.walk_bn, _, _, a.n_major = walk_plan(a.M, a.N, a.K, a.C0 + a.C1, BM, BN, smem, a.n_major, _a_traffic(a))


def _stats(a, staged_store):
    a.gstat = bool(a.gstat and staged_store and a.epi == EPI_STORE and a.N % 8 == 0 and a.M % 32 == 0 and a.ksplit <= 1 and a.n_main > 0)


def _epi_variant(a, WM, WN, WTM, WTN, ring_bytes):
    if a.ksplit > 1:
        return 0
    NW, MT, NT = WM * WN, WTM // 32, WTN // 32
    if NW * 32 * (WTN * 2 + 16) <= ring_bytes and a.epi == EPI_STORE and a.N % 8 == 0 and a.staged_epi:
        return 1
    if NT % 2 == 0 and a.epi == EPI_GEGLU and a.N % 128 == 0 and a.staged_epi and a.omode == 0:
        return 2
    if (NW * NT * 2560 <= ring_bytes and MT * NT <= 8 and a.epi == EPI_HEADS and a.staged_epi and a.rpb % 32 == 0 and
            a.part_width % 32 == 0 and a.head_dim % 8 == 0 and a.N % 32 == 0 and a.M % 32 == 0):
        return 3
    return 0


def _report(family, BM, BN, nst, amode, dma, grid, a, smem, variant, WM, WN):
    return (family, BM, BN, nst, amode, dma, grid, a.ksplit, a.n_major, a.walk_bn, a.par_nb, smem, int(a.gstat), variant, WM, WN)


def _launch_cfg(a, c, st, tile, glds):
    _, WM, WN, WTM, WTN, nst = tile
    BM, BN = WM * WTM, WN * WTN
    assert not (a.epi == EPI_GEGLU and (WTN // 32) % 2), "refused by the launcher: no GEGLU pairs in these wave tiles"
    smem_std = nst * (BM + BN) * 128 + (par_bytes(BN) if glds else 0)
    slots = 256 * min(LDS // smem_std, 8)
    a = SimpleNamespace(**vars(a))
    ntm, ntn = cdiv(a.M, BM), cdiv(a.N, BN)
    a.par_nb = _par_slots(a, BM)
    smem = nst * (BM + BN) * 128 + (par_bytes(BN, max(a.par_nb, PAR_NB)) if glds else 0)
    if smem > LDS:
        assert BM > 64 or BN > 64 or nst != 2, "the case table holds no refused launch"
        st.hint_applied = 0
        return _launch_cfg(a, c, st, (1, 2, 2, 32, 32, 2), glds)
    T, KT = ntm * ntn, a.K >> 6
    a.n_main, a.ksplit, a.staged_epi = T, 1, c.staged_epi
    a.n_major = _n_major(a, c, ntn)
    S = 0
    if a.split >= 2 and a.epi == EPI_STORE:
        S = min(a.split, KT)
    elif c.tail_split and a.allow_split and WTM == 64 and WTN == 64 and a.epi == EPI_STORE and T * 2 <= slots and KT >= 32:
        S = cdiv(slots, T) if c.tail_split == 2 else slots // T
        if KT // S < 12:
            S = KT // 12
        S = min(S, 16)
    if S >= 2 and T * S * BM * BN * 4 <= WS_BYTES:
        a.n_main, a.ksplit = 0, S
    n_tail = T - a.n_main
    _stats(a, WM * WN * 32 * (WTN * 2 + 16) <= nst * (BM + BN) * 128 and a.staged_epi and n_tail == 0)
    if n_tail > 0:
        a.n_major = 0
    _walk(a, c, BM, BN, smem)
    return _report(1, BM, BN, nst, a.amode, int(glds), a.n_main + n_tail * a.ksplit, a, smem,
                   _epi_variant(a, WM, WN, WTM, WTN, nst * (BM + BN) * 128), WM, WN)


def _launch_tile32(a, c, st, tile, wpe):
    _, WM, WN, WTM, WTN, nst = tile
    BM, BN = WM * WTM, WN * WTN
    wgs = wpe * 4 // (WM * WN)
    a = SimpleNamespace(**vars(a))
    a.par_nb = _par_slots(a, BM)
    smem = nst * (BM + BN) * 64 + par_bytes(BN, max(a.par_nb, PAR_NB) if a.temb else 0)
    if smem > LDS:
        st.hint_applied = 0
        return _launch_cfg(a, c, st, (1, 2, 2, 32, 32, 2), True)
    if wgs > 1 and smem * wgs > LDS:
        st.hint_applied = 0
        return _launch_cfg(a, c, st, TILES[1], True)
    ntm, ntn = cdiv(a.M, BM), cdiv(a.N, BN)
    a.n_main, a.ksplit, a.staged_epi = ntm * ntn, 1, c.staged_epi
    a.n_major = _n_major(a, c, ntn)
    _walk(a, c, BM, BN, smem)
    _stats(a, WM * WN * 32 * (WTN * 2 + 16) <= nst * (BM + BN) * 64 and a.staged_epi)
    return _report(2, BM, BN, nst, a.amode, 1, a.n_main, a, smem, _epi_variant(a, WM, WN, WTM, WTN, nst * (BM + BN) * 64), WM, WN)


def _variant_staged_only(a):
    return 1 if a.epi == EPI_STORE else 2 if a.epi == EPI_GEGLU else 3


def _mf16_supports(a, c):
    if a.N % 160 or not c.staged_epi or a.K < 64:
        return False
    if a.epi == EPI_STORE:
        return True
    return a.epi == EPI_HEADS and a.rpb % 32 == 0 and a.M % 32 == 0 and a.part_width % 16 == 0 and a.head_dim % 8 == 0


def _launch_mf16(a, c, st, nst):
    a = SimpleNamespace(**vars(a))
    a.par_nb = _par_slots(a, 128)
    smem = nst * 288 * 128 + par_bytes(160, max(a.par_nb, PAR_NB))
    if smem > LDS:
        st.hint_applied = 0
        return _launch_cfg(a, c, st, TILES[7], True)
    ntm, ntn = cdiv(a.M, 128), a.N // 160
    a.n_main, a.ksplit, a.staged_epi = ntm * ntn, 1, 1
    a.n_major = _n_major(a, c, ntn)
    _walk(a, c, 128, 160, smem)
    _stats(a, True)
    return _report(3, 128, 160, nst, a.amode, 1, a.n_main, a, smem, _variant_staged_only(a), 4, 2)


def _big4_supports(cfg, a, staged):
    if cfg < 24 or cfg > 26 or not staged or a.K < 64 or a.amode == 4:
        return False
    if a.epi == EPI_STORE:                                             # (operand sizes: every case here is far below the 4-GiB limits)
        return a.N % 8 == 0
    if a.epi == EPI_GEGLU:
        return cfg != 25 and a.N % 128 == 0 and a.omode == 0
    return a.rpb % 32 == 0 and a.part_width % 32 == 0 and a.head_dim % 8 == 0 and a.N % 32 == 0 and a.M % 32 == 0


def _big4_smem(cfg, a):
    BM, BN = tile_bm_bn(cfg)
    nb = _par_slots(a, BM) if a.temb else 0
    return 2 * (BM + BN) * 128 + par_bytes(BN, max(nb, PAR_NB))


def _launch_big4(a, c, cfg):
    BM, BN = tile_bm_bn(cfg)
    a = SimpleNamespace(**vars(a))
    a.par_nb = _par_slots(a, BM)
    smem = _big4_smem(cfg, a)
    ntm, ntn = cdiv(a.M, BM), cdiv(a.N, BN)
    a.n_main, a.ksplit, a.staged_epi = ntm * ntn, 1, 1
    a.n_major = _n_major(a, c, ntn)
    _walk(a, c, BM, BN, smem)
    _stats(a, True)
    return _report(4, BM, BN, 2, a.amode, 1, a.n_main, a, smem, _variant_staged_only(a), 2, 2)


def _big4p_ok(a, c):
    return a.amode == 0 and a.C1 == 0 and a.taps == 1 and not a.temb and _big4_supports(24, a, c.staged_epi) and a.K * 2 < (1 << 24)


def _launch_big4p(a, c):
    a = SimpleNamespace(**vars(a))
    a.par_nb = 0
    smem = 2 * 512 * 128 + 2 * par_bytes(256, PAR_NB)
    ntm, ntn = cdiv(a.M, 256), cdiv(a.N, 256)
    a.n_main, a.ksplit, a.staged_epi = ntm * ntn, 1, 1
    a.n_major = _n_major(a, c, ntn, a_bytes=2.0 * a.M * a.C0)
    _walk(a, c, 256, 256, smem)
    _stats(a, True)
    return _report(5, 256, 256, 2, 0, 1, min(a.n_main, 256), a, smem, _variant_staged_only(a), 2, 4)


def _launch_config(cfg, a, c, st):
    glds = c.staging != 0
    if 20 < cfg < 24:
        cfg, glds = cfg - 20, False
    if cfg in (1, 2, 3):
        return _launch_cfg(a, c, st, TILES[cfg], glds)
    if cfg in (4, 5, 6, 7, 8, 9, 10, 11, 12, 14):
        return _launch_cfg(a, c, st, TILES[cfg], True)
    if cfg in (13, 15, 16, 17):
        return _launch_tile32(a, c, st, TILES[cfg], T32_WPE[cfg])
    if cfg == 27:
        t = 16 if a.epi != EPI_STORE else 27
        st.hint_applied = 0 if t != cfg else st.hint_applied
        return _launch_tile32(a, c, st, TILES[t], T32_WPE[t])
    if cfg == 20:
        t = 13 if a.epi == EPI_GEGLU else 20
        st.hint_applied = 0 if t != cfg else st.hint_applied
        return _launch_tile32(a, c, st, TILES[t], T32_WPE[t])
    if cfg in (18, 19):
        if _mf16_supports(a, c):
            return _launch_mf16(a, c, st, TILES[cfg][5])
        st.hint_applied = 0
        return _launch_cfg(a, c, st, TILES[7], True)
    if cfg in (24, 25, 26):
        if _big4_supports(cfg, a, c.staged_epi) and _big4_smem(cfg, a) <= LDS:
            return _launch_big4(a, c, cfg)
        st.hint_applied = 0
        return _launch_cfg(a, c, st, TILES[1], True)
    if cfg == 28:
        if _big4p_ok(a, c):
            return _launch_big4p(a, c)
        st.hint_applied = 0
        return _launch_cfg(a, c, st, TILES[1], True)
    raise ValueError(cfg)


def _dispatch(c: Case):
    a = _args(c)
    st = SimpleNamespace(hint_applied=1 if (c.hint & 63) == 0 else 0)
    p = c.p
    assert a.C0 > 0 and a.C0 % 64 == 0 and a.C1 % 64 == 0 and a.N % 4 == 0 and a.taps in (1, 9) and 0 <= a.amode <= 3, c.id
    assert a.epi != EPI_GEGLU or a.N % 64 == 0, c.id
    assert a.epi != EPI_HEADS or (a.head_dim % 4 == 0 and a.part_width % 4 == 0), c.id
    cfg = c.cfg
    KT = a.K >> 6
    t128 = cdiv(a.M, 128) * cdiv(a.N, 128)
    if cfg == 0:
        t256x64 = cdiv(a.M, 256) * cdiv(a.N, 64)
        n_odd64 = a.N % 128 != 0
        t5 = cdiv(a.M, 256) * (a.N // 320) if a.N % 320 == 0 else 0
        t4 = cdiv(a.M, 256) * (a.N // 256) if a.N % 256 == 0 else 0

        def fills(t):
            return t >= 224 and (t % 256 == 0 or t % 256 >= 160 or t >= 1024)
        if a.epi != EPI_GEGLU and a.K >= 1280 and fills(t5):
            cfg = 5
        elif t4 >= 192 and (t4 % 256 == 0 or t4 % 256 >= 128 or t4 >= 512):
            cfg = 4
        elif t128 >= 256 and not n_odd64:
            cfg = 1
        elif t256x64 >= 256 and (n_odd64 or a.N <= 64):
            cfg = 2
        elif t128 >= 200:
            cfg = 1
        elif c.tail_split and KT >= 32 and t128 >= 8 and a.epi == EPI_STORE:
            cfg = 14
        else:
            cfg = 3
        if a.epi == EPI_GEGLU and cfg == 3:
            cfg = 1
    a.split = c.split if c.cfg != 0 else 0
    if c.cfg == 0 and c.staging and _mf16_supports(a, c):
        t7 = cdiv(a.M, 128) * (a.N // 160)
        if 200 <= t7 <= 256 or (t7 > 256 and t7 % 256 == 0 and t7 // 256 <= 2):
            return _launch_config(19, a, c, st), st.hint_applied
    if c.cfg == 0 and a.cfg_hint > 0 and c.staging:
        t_rule = cdiv(a.M, 256) * cdiv(a.N, 128) if cfg == 14 else t128
        rule_splits = (cfg in (1, 12, 14) and c.tail_split and a.epi == EPI_STORE and KT >= 32 and
                       t_rule * 2 <= (512 if cfg == 1 else 256))
        h = a.cfg_hint & 63
        valid = (h in (1, 4, 6, 12, 14, 13, 15, 16, 17) or (h == 10 and a.epi == EPI_GEGLU) or
                 (h in (5, 7, 8, 9, 11, 20) and a.epi != EPI_GEGLU) or (h == 27 and a.epi == EPI_STORE) or
                 (24 <= h <= 26 and _big4_supports(h, a, c.staged_epi) and _big4_smem(h, a) <= LDS) or (h == 28 and _big4p_ok(a, c)))
        if not rule_splits and valid:
            cfg, a.allow_split, st.hint_applied = h, 0, 1
    a.walk_hint = (a.cfg_hint >> 6) & 3 if (c.cfg == 0 and c.staging) else 0
    return _launch_config(cfg, a, c, st), st.hint_applied


@functools.lru_cache(maxsize=None)
def expected_launch(c: Case):
    """what cfgpp_igemm_last_launch must report after case c (slot order: igemm_kernel.hip, beside report_launch)"""
    return _dispatch(c)[0]


def expected_config_ran(c: Case):
    """cfgpp_igemm_last_config_ran() after case c"""
    return _dispatch(c)[1]


REPORT_FIELDS = ("family", "BM", "BN", "stages", "amode", "dma", "grid", "ksplit", "n_major", "walk_bn", "par_nb", "smem", "stats",
                 "epilogue", "WM", "WN")


# ---- the fp32 model of a correct kernel, and faults applied to it (tests/test_igemm_cases_cpu.py) ------------------------------------
def _f16(v32):
    return v32.astype(np.float16).astype(np.float32)


def model(c: Case, fault=None):
    """[rows, n_out] fp64: fp32 accumulation in the kernels' k order (channel-block major, tap minor; K-split slices summed as
    igemm_reduce_kernel does), the epilogue the launch report names, one rounding to fp16 (two on the staged store epilogues with a
    residual).  fault: one of FAULTS - what a subtly wrong kernel would compute instead.  An element a fault leaves unwritten is NaN"""
    p, i = c.p, inputs(c.p)
    rep = expected_launch(c)
    BM, ksplit, variant = rep[1], rep[7], rep[13]
    a = im2col(p, ashift=0 if fault == "ashift_ignored" else None)
    w = device_buffers(p).w.astype(np.float32)
    if fault == "tap_skipped":                                        # K-tile (channel block 0, tap 4): never accumulated
        a = a.copy()
        a[:, 4 * 64:5 * 64] = 0
    KT = p.K // 64
    slices = [(s * KT // ksplit, (s + 1) * KT // ksplit) for s in range(ksplit)]
    if fault == "slice_dropped":
        slices = slices[:-1]
    parts = []
    for (k0, k1) in slices:
        acc = np.zeros((p.rows, p.N), dtype=np.float32)
        for k in range(k0 * 64, k1 * 64):
            acc += np.outer(a[:, k], w[:, k])
        parts.append(acc)
    if ksplit == 1:
        acc = parts[0]
    else:                                                            # igemm_reduce_kernel: pairs, then the odd one
        acc = np.zeros((p.rows, p.N), dtype=np.float32)
        for s in range(0, len(parts) - 1, 2):
            acc += parts[s] + parts[s + 1]
        if len(parts) % 2:
            acc += parts[-1]
    bias = None if i.bias is None else i.bias.astype(np.float32)
    if p.op == "geglu":
        y = acc + bias if p.bias else acc
        f = np.arange(p.N // 2)
        pv = (f // 32) * 64 + f % 32
        pg = pv + 32
        if fault == "value_gate_swapped":                            # in the second 64-column group
            sw = (pv >= 64) & (pv < 128)
            pv, pg = np.where(sw, pg, pv), np.where(sw, pv, pg)
        return _f16(y[:, pv] * gelu_erf_pk(y[:, pg])).astype(np.float64)
    scale = np.float32(p.out_scale) if p.op == "store" else np.float32(1.0)
    if fault == "scale_after_bias":
        v = (acc + bias) * scale
    else:
        v = acc * scale
        if p.bias:
            bb = np.broadcast_to(bias, v.shape).copy()
            if fault == "bias_shifted":                               # columns [32, 64): the bias of 4 columns further
                bb[:, 32:64] = bias[36:68]
            v = v + bb
    if p.temb:
        b = _batch_of_rows(p)
        if fault == "temb_neighbour":                                # rows of sample 1 inside the first tile take sample 0's row
            b = np.where(np.arange(p.rows) < BM, 0, b)
        v = v + i.temb.astype(np.float32)[b]
    if p.resid:
        rr = i.resid.astype(np.float32)
        if fault == "resid_left":                                    # first 32-row block: the pixel one to the left
            rr = rr.copy()
            rr[1:32] = i.resid.astype(np.float32)[0:31]
        v = _f16(_f16(v) + rr) if variant == 1 else _f16(v + rr)
    else:
        v = _f16(v)
    out = v.astype(np.float64)
    if fault == "last_row_unwritten":
        out[p.rows - 1] = np.nan
    if fault == "last_columns_unwritten":
        out[:, p.N - 4:] = np.nan
    if fault == "vt_identity":                                       # V columns land at key position tok instead of cfgpp_vt_pos(tok)
        assert p.op == "heads" and not p.vt_linear
        lay = heads_layout(p)
        wrong = heads_layout(replace(p, vt_linear=1))
        out = scatter_gather_heads(p, out, wrong, lay)
    return out


def scatter_gather_heads(p: Problem, y, write, read):
    """write y [rows, N] into zeroed head-major buffers with layout `write`, read it back with layout `read`; slots nothing wrote: NaN
    where the live region is expected (as the GPU test's NaN fill)"""
    out = np.empty_like(y)
    for part in read.parts:
        buf = np.full(int(np.prod(read.shapes[part])), np.nan)
        sel = write.part == part
        buf[write.off[sel]] = y[sel]
        out[read.part == part] = buf[read.off[read.part == part]]
    return out


FAULTS = ("last_row_unwritten", "last_columns_unwritten", "bias_shifted", "resid_left", "tap_skipped", "value_gate_swapped", "vt_identity",
          "ashift_ignored", "scale_after_bias", "slice_dropped", "temb_neighbour")
