"""Inputs, references and the error bound of the image tower's attention kernel (plain torch, no HIP).

Shared by tests/test_vit_attn_cases_cpu.py (the bound sees the faults it is meant to see: fault models, no GPU) and
tests/test_gpu_vit_attention.py (vit_attn_kernel of cfgpp_amd/csrc/vision.hip through cfgpp_op_attention_vit).

Layout, as the kernel reads it: qkv [rows, T, 3 * hidden] fp16, hidden = heads * d, Q | K | V column blocks, head h at columns h * d of
each; output [rows, T, hidden].

Inputs (fp16-representable, seeded), built so that a fault moves a row by about 1:
  * background: q = 0.3 randn + 8u, k = 0.3 randn - 8u (u the unit vector): every real score is about -64 / sqrt(d), so a pad key that
    enters the softmax with score 0 takes most of the probability mass;
  * k dims 0 .. 7 carry +-4 and v dims 0 .. 7 +-8, signs per (row, head, key, dim): what a d = 104 kernel reads as "dims 104 .. 111" when
    it does not zero-fill its seventh k-step are the NEXT head's (or the next column block's) dims 0 .. 7, and those then reweigh
    every key by about e^+-1;
  * planted pairs: chosen query rows get q = w_t, planted key keys[t] gets k = 1.5 sqrt(d) w_t - one dominant score, ~30 nats above
    every other key - and a V row of large distinctive values; w_t = 4 e_dim(t) - b u with dim(t) = d - 8 + t: for d = 104 the
    planted directions are dims 96 .. 103, the lower half of the seventh k-step.  Which planted key a row asks for depends on the
    head, the batch row and the row's 32-query block ((i + row // 32 + 3 h + r) mod nK), so an answer from another head or row is a different V row.
      rows: 0, T - 1, both sides of every multiple of 32, every i = 2 mod 5;
      keys: 0, T - 1, the first key of the last (partial) 32-key tile, keys 4 and 8 of the last block that holds both (the two the V^T
            permutation swaps), key 40 when T > 64.

Reference: ``ref64`` (softmax attention in fp64).  ``model`` restates vit_attn_kernel in fp64 with its rounding points and nothing else:
fp16 operands, scores rounded to fp32 and multiplied by the fp32 constant d^-1/2 log2(e) in fp32, the online softmax over 32-key tiles
with P = exp2(s - running max) rounded to fp16, the denominator summed from the ROUNDED P, the output rounded to fp16.

Metric and bound are the project's (tests/attn_cases.py): per (row, token, head) row of d outputs ||got - ref|| / (||ref|| + 1e-3 rms row
norm), maximum over rows; bound of a case = FACTOR * E_model, E_model the model's own error against ref64, computed on the CPU.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

from attn_cases import FACTOR, max_row_err  # noqa: F401  (the project's bound and metric, not restated)

LOG2E = 1.4426950408889634
KT = 32
HEAD_DIMS = (64, 80, 104)
MAX_TOKENS = 320


@dataclass(frozen=True)
class Case:
    d: int
    T: int
    heads: int
    rows: int
    seed: int = 0

    @property
    def id(self):
        return f"d{self.d}T{self.T}h{self.heads}r{self.rows}"

    @property
    def launch(self):
        """what cfgpp_vit_attention_last_launch must report: head dim, query blocks, key tiles"""
        return [self.d, (self.T + 31) // 32, (self.T + KT - 1) // KT]


def _table():
    out = []
    for T in (1, 5, 31, 32, 33, 37, 64, 65, 257):           # one partial tile, exact tiles, a tile + a few keys, the real size
        out += [Case(104, T, 1, 1), Case(104, T, 2, 2)]
    out += [Case(104, 37, 2, 1), Case(104, 37, 1, 2)]
    for d in (64, 80):
        out += [Case(d, T, 2, 2) for T in (5, 33, 64, 257)] + [Case(d, 33, 1, 1), Case(d, 37, 1, 2)]
    return [Case(c.d, c.T, c.heads, c.rows, seed=2000 + i) for i, c in enumerate(out)]


ALL_CASES = _table()


def planted_keys(T):
    keys = [0, T - 1, KT * ((T - 1) // KT)]
    if T >= 9:
        blk = 32 * ((T - 9) // 32)
        keys += [blk + 4, blk + 8]
    if T > 64:
        keys.append(40)
    out = []
    for k in keys:
        if k not in out:
            out.append(k)
    return out


def planted_rows(T):
    rows = {0, T - 1} | {i for i in range(T) if i % 5 == 2}
    for m in range(32, T, 32):
        rows.update((m - 1, m))
    return sorted(rows)


def make_qkv(c: Case):
    """-> qkv [rows, T, 3 * hidden] float32 holding fp16 values"""
    g = torch.Generator().manual_seed(c.seed)
    R, h, T, d = c.rows, c.heads, c.T, c.d
    q = 0.3 * torch.randn((R, h, T, d), generator=g)
    k = 0.3 * torch.randn((R, h, T, d), generator=g)
    v = torch.randn((R, h, T, d), generator=g)
    u = torch.full((d,), d ** -0.5)
    q, k = q + 8 * u, k - 8 * u
    k[..., :8] += 4.0 * torch.sign(torch.randn((R, h, T, 8), generator=g))
    v[..., :8] = 8.0 * torch.sign(torch.randn((R, h, T, 8), generator=g))
    keys, rows = planted_keys(T), planted_rows(T)
    nK = len(keys)
    uw = -(64.0 / math.sqrt(d) + 14.0) / 12.0               # other queries (~8u) see a planted key 14 nats below an ordinary one
    a, cc = 4.0, 1.5 * math.sqrt(d)
    b = (a / math.sqrt(d) - uw) / (1 - 1.0 / d)
    w = torch.zeros((nK, d))
    for t in range(nK):
        w[t] = -b * u
        w[t, d - 8 + t] = a
    pv = 8.0 * torch.sign(torch.randn((R, h, nK, d), generator=g))
    pv[..., 0] += torch.arange(1, nK + 1, dtype=torch.float32)
    ri = torch.arange(len(rows))
    blk = torch.tensor(rows) // 32                          # ... and on the row's 32-query block: a block answering for its neighbour shows
    for r in range(R):
        for hh in range(h):
            q[r, hh, rows] = w[(ri + blk + 3 * hh + r) % nK]
            k[r, hh, keys] = cc * w
            pv[r, hh, :, 1] += float(2 * hh + r)
            v[r, hh, keys] = pv[r, hh]
    parts = [x.permute(0, 2, 1, 3).reshape(R, T, h * d) for x in (q, k, v)]
    return torch.cat(parts, -1).half().float()


def split(qkv, heads, d):
    """qkv [rows, T, 3 hidden] -> q, k, v [rows, heads, T, d]"""
    R, T, _ = qkv.shape
    hid = heads * d
    return tuple(qkv[..., i * hid:(i + 1) * hid].reshape(R, T, heads, d).permute(0, 2, 1, 3) for i in range(3))


def ref64(qkv, heads, d):
    """softmax(q k^T / sqrt(d)) v in fp64 -> [rows, T, hidden]"""
    q, k, v = (x.double() for x in split(qkv, heads, d))
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    o = torch.softmax(s, -1) @ v
    return o.permute(0, 2, 1, 3).reshape(qkv.shape[0], qkv.shape[1], heads * d)


def _r16(x):
    return x.to(torch.float16).to(torch.float64)


FAULTS = ("pad_leak", "drop_last_tile", "no_zero_fill", "head_stride", "kv_swap", "qblock_off")


def model(qkv, heads, d, fault=None):
    """vit_attn_kernel in fp64 with its rounding points -> [rows, T, hidden] fp64 (holding fp16 values).

    ``fault`` injects one defect of the kind the GPU test must catch (tests/test_vit_attn_cases_cpu.py):
      pad_leak        the pad keys T .. 32 ceil(T / 32) - 1 of the last tile (zero K, zero V, as the kernel stages them) enter the softmax
      drop_last_tile  the last, partial key tile is not walked (T % 32 != 0, T > 32)
      no_zero_fill    d = 104: dims 104 .. 111 of Q and K are read from memory - the next head's, or the next column block's, dims 0 .. 7
      head_stride     head h answers with head (h + 1) mod heads' operands
      kv_swap         the K and V column blocks exchanged
      qblock_off      query block i >= 1 answers with the queries of block i - 1 (a base off by 32)
    """
    R, T, _ = qkv.shape
    hid = heads * d
    q, k, v = (x.double().clone() for x in split(qkv, heads, d))
    if fault == "kv_swap":
        k, v = v, k
    if fault == "head_stride":
        idx = [(i + 1) % heads for i in range(heads)]
        q, k, v = q[:, idx], k[:, idx], v[:, idx]
    if fault == "qblock_off":
        q = torch.cat([q[:, :, :32], q[:, :, :-32]], 2) if T > 32 else q
    if fault == "no_zero_fill":
        assert d == 104
        ext = [torch.stack([qkv[..., sec * hid + hh * d + 104: sec * hid + hh * d + 112] for hh in range(heads)], 1).double() for sec in (0, 1)]
        q, k = torch.cat([q, ext[0]], -1), torch.cat([k, ext[1]], -1)
    Tp = (T + KT - 1) // KT * KT
    scale = torch.tensor(LOG2E / math.sqrt(d), dtype=torch.float32)
    s = ((q @ k.transpose(-1, -2)).float() * scale).double()                    # fp32 scores x the fp32 constant, in fp32
    s = torch.cat([s, torch.zeros((R, heads, T, Tp - T), dtype=torch.float64)], -1)
    vv = torch.cat([v, torch.zeros((R, heads, Tp - T, v.shape[-1]), dtype=torch.float64)], 2)
    valid = torch.arange(Tp) < T
    if fault == "pad_leak":
        valid[:] = True
    ntiles = Tp // KT
    if fault == "drop_last_tile" and T % KT != 0 and T > KT:
        ntiles -= 1
    s[..., ~valid] = -math.inf
    m = torch.full((R, heads, T, 1), -math.inf, dtype=torch.float64)
    l = torch.zeros((R, heads, T, 1), dtype=torch.float64)
    o = torch.zeros((R, heads, T, v.shape[-1]), dtype=torch.float64)
    for t in range(ntiles):
        st = s[..., t * KT:(t + 1) * KT]
        mn = torch.maximum(m, st.max(-1, keepdim=True).values)
        alpha = torch.exp2(m - mn)
        p = _r16(torch.exp2(st - mn))
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p @ vv[:, :, t * KT:(t + 1) * KT]
        m = mn
    out = _r16(o / l)
    return out.permute(0, 2, 1, 3).reshape(R, T, heads * d)


@functools.lru_cache(maxsize=None)
def reference(c: Case):
    """-> qkv, ref (fp64), E_model, bound: everything a test of case c needs, computed once and shared (do not modify)"""
    qkv = make_qkv(c)
    ref = ref64(qkv, c.heads, c.d)
    e_model = max_row_err(model(qkv, c.heads, c.d), ref, c.d)
    return qkv, ref, e_model, FACTOR * e_model
