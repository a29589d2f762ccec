"""Inputs, references and the error bound of the perceiver-attention tests (IP-Adapter Plus Resampler; plain torch, no HIP).

Shared by tests/test_perceiver_cases_cpu.py (the bound sees the faults it is meant to see) and tests/test_gpu_perceiver.py
(cfgpp_op_perceiver_attention of cfgpp_amd/csrc/resampler.hip against the same references).  Metric and factor are those of
tests/attn_cases.py: attn_cases.max_row_err, bound of a case = attn_cases.FACTOR x E_model, E_model being the error of ``model``
against ``ref`` on the same inputs, computed on the CPU by the test that uses it.

Contract under test: head dim 64; per (row, head) n_q <= 32 queries attend, in ONE softmax, to S image-token keys followed by n_q
latent keys; operands token-major as the to_q / to_kv GEMMs leave them (q [rows, n_q, heads * 64], kv_x [rows, S, 2 * heads * 64]
and kv_l [rows, n_q, 2 * heads * 64] with K in the first half of the columns and V in the second); the kernel walks the joint key
axis in tiles of KEY_TILE = 32 keys, and keys past S + n_q / queries past n_q are pads that enter nothing.

Inputs (fp16-representable, seeded): q = 0.3 * randn + 6u, k = 0.3 * randn - 6u with u a unit vector - every real score is about -4.5
nats, so a pad key that enters with score 0 takes the mass of ~90 real keys; v = 8 * sign(randn) with component 0 raised by the joint
key index + 1, component 1 by the head index and component 2 by the row index.  On top, PLANTED queries: query j of (row r, head h)
has plant kind (j + r + h) % 4 - 0: the last key (a latent key), 1: key 0 (an image key), 2: key 4 (one of the two columns the V^T
staging swaps; the last key when there are at most 4 keys), 3: not planted.  A planted query is q = w and its key k = 3w with |w| = 8:
one score ~23 nats above every other, so that row's output IS the planted key's V row - a dropped, misplaced or foreign key moves it
by O(1), however many keys there are.  Every case of the tables has all four kinds.

Reference: ``ref`` = softmax(q k^T / 8) v in fp64 over the joint keys.  ``model``: fp64 arithmetic with the kernel's rounding points
and nothing else - fp32 scores times fp32(1/8 * log2 e) (q is NOT rounded again: the scale is applied once, on the scores), one
maximum over all keys, P = exp2(s - max) rounded to fp16, the denominator summed from the rounded P, one output rounding.

Kernel / E_model ratios on the MI355X ("perceiver_case" lines of the parity file): see RATIOS below.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

import attn_cases as A
from attn_cases import FACTOR, max_row_err  # noqa: F401  (the metric and the bound's factor are attn_cases' own)

D = 64                         # dim_head of every published Resampler
KEY_TILE = 32                  # keys per tile of perceiver_attn_kernel
MAX_Q = 32
MAX_S = 1024

# Kernel / E_model ratios (max_row_err / e_model) measured on the MI355X ("perceiver_case" lines of the parity file; the bound is
# FACTOR = 4): group -> (cases, min, median, max).  Most cases sit at 1.00 - the row that sets the maximum is one whose error is the
# output rounding alone; the rest is fp32 accumulation in the MFMAs' order and the tile-by-tile rescale against the model's fp64.
RATIOS = dict(perceiver_small=(10, 0.95, 1.00, 1.00), perceiver_tile_edges=(24, 0.87, 1.00, 1.00), perceiver_real=(5, 0.98, 1.00, 1.00))


@dataclass(frozen=True)
class PCase:
    rows: int
    heads: int
    nq: int
    S: int
    seed: int = 0

    @property
    def id(self):
        return f"r{self.rows}h{self.heads}q{self.nq}S{self.S}"

    @property
    def nk(self):
        return self.S + self.nq

    @property
    def tiles(self):
        return (self.nk + KEY_TILE - 1) // KEY_TILE


def _rh(i, nq):
    """rows, heads of the i-th case of a table: a single query needs 3 x 3 (row, head) pairs to see every plant kind"""
    return (3, 3) if nq < 4 else ((1, 1), (3, 1), (1, 3), (3, 3))[i % 4]


def _table(shapes, base):
    return [PCase(*_rh(i, nq), nq, S, seed=base + i) for i, (nq, S) in enumerate(shapes)]


NQS = (1, 4, 16, 17, 32)
T = KEY_TILE
# 1. one and two image keys under every query count
SMALL = _table([(nq, S) for nq in NQS for S in (1, 2)], 9000)
# 2. S + n_q at T - 1, T, T + 1, 2T and 2T + 1: the tile boundary inside the image keys (n_q = 1, 4: S > T), exactly between the
#    two sources (S = T: n_q = 1 at T + 1, n_q = 32 at 2T) and inside the latent keys (n_q = 16, 17, 32 at T + 1 and 2T + 1)
TILE_EDGES = _table([(nq, tot - nq) for nq in NQS for tot in (T - 1, T, T + 1, 2 * T, 2 * T + 1) if tot - nq >= 3]      # (S = 1, 2: table 1)
                    + [(32, 16), (32, 48)], 9100)       # ... and 16 latent keys on either side of the boundary at T / at 2T
# 3. the towers' sequence lengths (ViT-H/14, ViT-bigG/14: 257; ViT-L/14@336: 577) and the longest supported
REAL = _table([(16, 257), (16, 577), (1, 257), (32, 577), (32, MAX_S)], 9200)

GROUPS = dict(perceiver_small=SMALL, perceiver_tile_edges=TILE_EDGES, perceiver_real=REAL)
ALL_CASES = [c for g in GROUPS.values() for c in g]

FAULTS = ("latent_dropped", "image_dropped", "two_softmaxes", "pad_leak", "last_dropped", "other_row_latents", "other_head_k",
          "v_unpermuted", "scale_once")


def fault_applies(fault, c: PCase):
    """is `fault` a change of the arithmetic at all on case c"""
    if fault == "pad_leak":
        return c.nk % KEY_TILE != 0
    if fault == "other_row_latents":
        return c.rows > 1
    if fault == "other_head_k":
        return c.heads > 1
    if fault == "v_unpermuted":
        return c.nk > 4                        # keys 0 .. 3 keep their columns
    return True


# ---- inputs -------------------------------------------------------------------------------------------------------------
def plant_kind(c: PCase):
    """[rows, heads, nq] int: 0 last key, 1 key 0, 2 key 4 (the last key when nk <= 4), 3 none"""
    r = torch.arange(c.rows)[:, None, None]
    h = torch.arange(c.heads)[None, :, None]
    j = torch.arange(c.nq)[None, None, :]
    return (j + r + h) % 4


def plant_targets(c: PCase):
    """joint key index of plant kinds 0, 1, 2"""
    return (c.nk - 1, 0, 4 if c.nk > 4 else c.nk - 1)


def make_inputs(c: PCase):
    """-> q [rows, heads, nq, 64], k / v [rows, heads, S + nq, 64] (joint key axis: image keys, then latent keys) float32 holding
    fp16 values"""
    g = torch.Generator().manual_seed(c.seed)
    R, H, nq, nk = c.rows, c.heads, c.nq, c.nk
    u = torch.full((D,), D ** -0.5)
    q = 0.3 * torch.randn((R, H, nq, D), generator=g) + 6 * u
    k = 0.3 * torch.randn((R, H, nk, D), generator=g) - 6 * u
    v = 8.0 * torch.sign(torch.randn((R, H, nk, D), generator=g))
    v[..., 0] += torch.arange(1, nk + 1, dtype=torch.float32)
    v[..., 1] += torch.arange(H, dtype=torch.float32)[None, :, None]
    v[..., 2] += torch.arange(R, dtype=torch.float32)[:, None, None]
    w = torch.randn((R, H, 3, D), generator=g)
    w = 8.0 * w / w.norm(dim=-1, keepdim=True)
    tg = plant_targets(c)
    if tg[2] == tg[0]:
        w[:, :, 2] = w[:, :, 0]
    kind = plant_kind(c)
    for p in range(3):
        sel = kind == p                                         # [R, H, nq]
        q = torch.where(sel[..., None], w[:, :, p][:, :, None, :].expand(R, H, nq, D), q)
        k[:, :, tg[p]] = 3.0 * w[:, :, p]
    return tuple(x.half().float() for x in (q, k, v))


def to_kernel_layout(c: PCase, q, k, v):
    """-> q [rows, nq, inner], kv_x [rows, S, 2 * inner], kv_l [rows, nq, 2 * inner] (fp32 holding fp16 values)"""
    R, H, nq, S = c.rows, c.heads, c.nq, c.S
    tok = lambda x: x.transpose(1, 2).reshape(R, x.shape[2], H * D)     # noqa: E731
    kv = torch.cat([tok(k), tok(v)], -1)
    return tok(q).contiguous(), kv[:, :S].contiguous(), kv[:, S:].contiguous()


# ---- reference and model --------------------------------------------------------------------------------------------------
def _tok_out(o):
    R, H, nq, d = o.shape
    return o.transpose(1, 2).reshape(R, nq, H * d)


def ref(q, k, v):
    """softmax(q k^T / 8) v in fp64 -> [rows, nq, heads * 64]"""
    s = q.double() @ k.double().transpose(-1, -2) / 8.0
    return _tok_out(torch.softmax(s, -1) @ v.double())


def _r16(x):
    return x.to(torch.float16).to(torch.float64)


def vt_pos(n):
    """column of key i in the kernel's V^T staging, i < n (n a multiple of 32): bits 2 and 3 of the index swapped"""
    i = torch.arange(n)
    return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1)


def model(q, k, v, S, fault=None):
    """fp64 perceiver attention with the kernel's rounding points -> [rows, nq, heads * 64] fp64 (holding fp16 values).

    ``fault`` (tests/test_perceiver_cases_cpu.py):
      latent_dropped     the latent keys S .. S + n_q - 1 masked
      image_dropped      the image keys 0 .. S - 1 masked
      two_softmaxes      one softmax per source, the two outputs added
      pad_leak           keys S + n_q .. round_up(S + n_q, 32) - 1 (zero K, zero V) enter with score 0
      last_dropped       key S + n_q - 1 masked
      other_row_latents  latent K / V of row (r + 1) % rows
      other_head_k       K of head (h + 1) % heads (V of the right head)
      v_unpermuted       V staged in key order, read through the bits-2/3 permutation (per 32-key tile)
      scale_once         scores times 64^-1/4 (the scale applied to one operand only) instead of 1/8
    """
    R, H, nq, d = q.shape
    nk = k.shape[2]
    k, v = k.clone(), v.clone()
    if fault == "other_row_latents":
        k[:, :, S:], v[:, :, S:] = k[:, :, S:].roll(-1, 0), v[:, :, S:].roll(-1, 0)
    if fault == "other_head_k":
        k = k.roll(-1, 1)
    valid = torch.ones(nk, dtype=torch.bool)
    n_pad = (-nk) % KEY_TILE
    if fault in ("pad_leak", "v_unpermuted") and n_pad:
        k = torch.cat([k, torch.zeros((R, H, n_pad, d))], 2)
        v = torch.cat([v, torch.zeros((R, H, n_pad, d))], 2)
        valid = torch.cat([valid, torch.full((n_pad,), fault == "pad_leak")])
    if fault == "v_unpermuted":
        v = v[:, :, vt_pos(v.shape[2])]
    if fault == "latent_dropped":
        valid[S:nk] = False
    if fault == "image_dropped":
        valid[:S] = False
    if fault == "last_dropped":
        valid[nk - 1] = False
    scale = 64.0 ** -0.25 if fault == "scale_once" else 0.125
    sc = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(A.LOG2E_F32, dtype=torch.float32))
    s = (q.double() @ k.double().transpose(-1, -2)) * sc                # log2 domain

    def group(mask):
        t = s.clone()
        t[..., ~mask] = -math.inf
        m = t.max(-1, keepdim=True).values
        p = _r16(torch.exp2(t - m))
        return (p @ v.double()) / p.sum(-1, keepdim=True)

    if fault == "two_softmaxes":
        mx, ml = valid.clone(), valid.clone()
        mx[S:] = False
        ml[:S] = False
        return _tok_out(_r16(group(mx) + group(ml)))
    return _tok_out(_r16(group(valid)))


def reference(c: PCase):
    """-> (q, k, v), ref (fp64), E_model, bound: everything a test of case c needs, computed once"""
    ins = make_inputs(c)
    r = ref(*ins)
    e_model = max_row_err(model(*ins, c.S), r, D)
    return ins, r, e_model, FACTOR * e_model
