"""Cases, inputs, fp64 references, models, fault models and bounds of the kernels the text and image towers add beside the implicit
GEMM and the LayerNorm (numpy / torch on the CPU, no HIP): csrc/text.hip (text_embed, text_attn, text_pool), csrc/vision.hip
(vit_assemble, vit_cls_rows), csrc/resampler.hip (broadcast_rows, gelu_inplace) and act_inplace of csrc/small_kernels.hip.

Shared by tests/test_tower_cases_cpu.py (the tables reach every launcher branch and refusal, the model of a correct kernel passes
every condition, every fault model fails one: no GPU) and tests/test_gpu_tower_kernels.py (the kernels, through the hooks of
csrc/cfgpp_debug.h, which call the launchers the towers' plans call).

Every model returns the WHOLE destination as fp64 with NaN where the kernel stores nothing.  Every batch row, head, token and channel
carries its own scale or sign, so a value credited to the wrong place shows.

Causal text attention (text_attn_kernel; T = 77 tokens and d = 64 are the kernel's).  Layout as tests/vit_attn_cases.py: qkv
[B, 77, 3 H], H = 64 heads, Q | K | V column blocks; out [B, 77, H].  Inputs follow vit_attn_cases.make_qkv - a background of
q = 0.3 randn + 1, k = 0.3 randn - 1 per component (every ordinary score about -8), K dims 0 .. 7 carrying +-4 and V dims 0 .. 7 +-8
decoys in EVERY head, so the next head's columns are never neutral - with three kinds of head, (head + batch row) mod 3 when a case
has more than one head:
  planted   query rows 0, 1, 31, 32, 63, 64, 75, 76 are q = 16 e_(56 + t), t the row's rank in that list.  The keys j = i (the
            diagonal: must be in), j = i + 1 and j = 76 (the future: must be out) and j = 0 carry, per row that asks for them,
            c_j e_(56 + t) with c_j = 23.625 / (1 - n_j / 64), n_j the number of rows asking for key j, and -(112 + n_j c_j) / 64 on
            every component: the planted rows score their own keys about +42, everything else about -2 .. -12, and ordinary rows
            (components about 1) score a planted key about 14 nats below an ordinary one.  A planted row's answer is a mix of
            V[i] and V[0] of comparable weights; the planted keys' V rows are large and carry the key's rank, head and batch row.
  rising    k_j += 2 j on every component: every query's scores rise by about 16 nats per key, the running maximum rises and acc / l
            are rescaled at EVERY key; the answer is V[i], the diagonal.  Scores reach 1.2e3.
  falling   k_j -= 2 j: the maximum is set at key 0 and never moves; the answer is V[0].
The `big` case multiplies q by 32 (all heads planted): planted scores of 1.3e3.
Exact properties: row 0 of every head equals V[0] bit for bit (p = 1, l = 1, acc = V).
Metric and bound are the project's (tests/attn_cases.py): max over (batch row, token, head) rows of ||got - ref|| / (||ref|| + 1e-3
rms row norm) <= FACTOR x E_model, E_model the error of `attn_model` against `attn_ref64`, computed on the CPU.  The model restates
the kernel's rounding points and nothing else: fp16 operands, q x 0.125 in fp32 (exact), the 64-term dot product as an fp32 FMA
chain, the per-key online softmax in fp32 (m, corr = exp(m - m'), p = exp(s - m'), l = l corr + p, acc = acc corr + p v, every
operation rounded once, the exponentials evaluated exactly), acc / l by a reciprocal, the output rounded to fp16.

embed, assemble, pool, cls_rows, broadcast_rows: bit-exact against the torch restatement, e.g. (tok[id].float() + pos[t].float())
.half(): one fp32 addition of two fp16 values and one conversion are IEEE operations.  Row widths H: 64 (only 8 of the 128 threads
work), 768, 1024 (exactly one pass of 128 threads x 8 values), 1088, 1280, 1664 (a partial second pass).  Ids outside [0, vocab) and
EOS positions outside [0, 77) are clamped: that is what the kernels promise, so the references clamp.

Activations, per element, (|got - ref64| - rounding) / rest <= 1 with rounding = 0.5 ulp16(ref64), on all 63488 finite fp16 values.
EPS = 2^-23.
  act 0, quick_gelu: ref = x sigmoid(c x), c the VALUE of the fp32 constant 1.702f.  The kernel evaluates f / (1 + __expf(-(c f)))
      with y' = fl(c f), |y' - y| <= dy = 2^-24 |y|.  It is silu(y) / c but for the numerator, which is the exact x:
      x sigmoid(y') = silu-like evaluation at y' (error E_silu(y; dy) / c, small_cases.e_silu: the exponential, the addition and the
      division) plus x (sigmoid(y') - sigmoid(y)), at most |x| dy sigmoid(-(|y| - dy)) since sigmoid' <= sigmoid(-|.|):
          rest = E_silu(y, dy) / c + |x| dy sigmoid(-(|y| - dy)).
  act 1, erf GELU: ref = x / 2 (1 + erf(x / sqrt 2)), evaluated as x / 2 erfc(-x / sqrt 2) (the same function without the
      cancellation).  The kernel: a = fl(f k), k = fl32(1 / sqrt 2): relative 1.5 x 2^-24, which moves erf by at most max_a |a erf'(a)|
      1.5 x 2^-24 < 0.5 EPS; erff within 16 ulp (the ROCm installation documents no limit; OpenCL's full-profile limit for erf is
      used, as small_cases.py does for exp / sin / cos): 16 EPS |erf|; the addition 1 + erf, |1 + erf| <= 2: 1 EPS; the product
      with fl(0.5 f) (exact): 2^-24 |1 + erf| <= 1 EPS.  Hence
          rest = |x| / 2 (16 EPS |erf(x / sqrt 2)| + 3 EPS).
      It is an ABSOLUTE bound of about 1e-6 |x|: for x < -4 the fp32 sum 1 + erff cancels to 0 and the kernel returns -0 where the
      true value is -1e-6 or less; that is inside the bound, and it is what `transformers`' fp32 GELU does as well.
  Signed zeros: where the fp64 reference is +-0 or underflows fp16 (|ref| < 2^-25) the stored zero must carry the reference's sign -
  large negative x gives -0 in both activations.
  gelu_inplace (the Resampler's own kernel, common.h gelu_erf_f: erfc by Abramowitz-Stegun 7.1.26, |abs err| <= 1.5e-7, hardware rcp
  and exp2): the same reference, rest = |x| (1.5e-7 + 8 EPS) - the polynomial's documented limit on erfc / 2 .. erfc, plus 1 ulp
  each for rcp and exp2 entering erfc (<= 1) with factors below 2, the Horner chain and the final product.  It is NOT act 1 (another
  erf), which is why it keeps its own kernel and hook.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

import vit_attn_cases as V
from attn_cases import FACTOR, max_row_err  # noqa: F401  (the project's bound and metric, not restated)
from igemm_cases import ulp16
from small_cases import EPS, F32, F64, _scales, cdiv, e_silu, fma32, h16, ratio, violations  # noqa: F401

# Kernel figures on the MI355X (profiles/tower_cases/tower_case_parity.jsonl), min / median / max per group of
# tests/test_gpu_tower_kernels.py:
#   text attention, max row error / E_model   1.000 / 1.000 / 1.000   (E_model 2.5e-4 .. 3.5e-4 over the five cases: in every case the
#       worst row of the kernel is the worst row of the model, to the last digit - the fp16 rounding of the output; row 0 == V[0])
#   act_inplace, (|got - ref64| - rounding) / rest over the 63488 values:   act 0   0.174      act 1   0.133      (the fp32 models: the same)
#   gelu_inplace                                                                    0.065
#   the tails n = 8, 2040, 2048, 2056 of all three: the bits of the full launch.
#   embed, assemble, pool, cls_rows, broadcast_rows: exact, 68 cases.
# Nothing is above 1; the activations stay below a fifth of `rest` because `rest` carries the 16 ulp of erf / the worst-case exponential
# term, of which the device functions use about one ulp.
T = 77
D = 64
H_VALUES = (64, 768, 1024, 1088, 1280, 1664)


def row_passes(H, threads=128, per_thread=8):
    """(threads that work in the first pass, passes of the `for (c = tid * 8; c < H; c += 1024)` loop, the last pass is partial)"""
    span = threads * per_thread
    return min(threads, cdiv(H, per_thread)), cdiv(H, span), H % span != 0


# =================================================================================================================================
# causal text attention
# =================================================================================================================================
@dataclass(frozen=True)
class AT:
    heads: int
    B: int
    big: int = 0
    seed: int = 0

    @property
    def id(self):
        return f"h{self.heads}B{self.B}" + ("-big" if self.big else "")

    @property
    def H(self):
        return self.heads * D


ATTN = [AT(1, 1, seed=3000), AT(2, 3, seed=3001), AT(12, 1, seed=3002), AT(20, 2, seed=3003), AT(2, 3, big=1, seed=3004)]
ATTN_REFUSED = ("H%8", "H!=64heads", "B0", "null_qkv", "null_out")
PLANT_ROWS = (0, 1, 31, 32, 63, 64, 75, 76)
KINDS = ("planted", "rising", "falling")


def head_kind(c: AT, b, h):
    return "planted" if c.heads == 1 or c.big else KINDS[(h + b) % 3]


def plant_keys(i):
    """the keys planted for query row i: the diagonal, the two future keys i + 1 and 76, key 0"""
    return sorted({i, min(i + 1, T - 1), T - 1, 0})


def planted_key_set():
    return sorted({j for i in PLANT_ROWS for j in plant_keys(i)})


def attn_qkv(c: AT):
    """-> qkv [B, 77, 3 H] float32 holding fp16 values"""
    g = torch.Generator().manual_seed(c.seed)
    R, h = c.B, c.heads
    q = 0.3 * torch.randn((R, h, T, D), generator=g) + 1.0
    k = 0.3 * torch.randn((R, h, T, D), generator=g) - 1.0
    v = torch.randn((R, h, T, D), generator=g)
    k[..., :8] += 4.0 * torch.sign(torch.randn((R, h, T, 8), generator=g))
    v[..., :8] = 8.0 * torch.sign(torch.randn((R, h, T, 8), generator=g))
    keys = planted_key_set()
    asks = {j: [t for t, i in enumerate(PLANT_ROWS) if j in plant_keys(i)] for j in keys}
    pv = 8.0 * torch.sign(torch.randn((R, h, len(keys), D), generator=g))
    pv[..., 0] = 8.0 + torch.arange(1, len(keys) + 1, dtype=torch.float32)
    ramp = 2.0 * torch.arange(T, dtype=torch.float32)[:, None]
    for r in range(R):
        for hh in range(h):
            kind = head_kind(c, r, hh)
            if kind == "rising":
                k[r, hh] += ramp
            elif kind == "falling":
                k[r, hh] -= ramp
            else:
                for t, i in enumerate(PLANT_ROWS):
                    q[r, hh, i] = 0.0
                    q[r, hh, i, 56 + t] = 16.0
                for n, j in enumerate(keys):
                    cj = 23.625 / (1.0 - len(asks[j]) / 64.0)
                    k[r, hh, j] -= (112.0 + len(asks[j]) * cj) / 64.0
                    for t in asks[j]:
                        k[r, hh, j, 56 + t] += cj
                    v[r, hh, j] = pv[r, hh, n]
                    v[r, hh, j, 1] = 8.0 + 2 * hh + r
    if c.big:
        q = q * 32.0
    parts = [x.permute(0, 2, 1, 3).reshape(R, T, h * D) for x in (q, k, v)]
    return torch.cat(parts, -1).half().float()


def attn_scores64(qkv, heads):
    """q k^T / 8 in fp64 -> [B, heads, 77, 77] (unmasked)"""
    q, k, _ = (x.double() for x in V.split(qkv, heads, D))
    return q @ k.transpose(-1, -2) * 0.125


def attn_ref64(qkv, heads):
    """causal softmax(q k^T / 8) v in fp64 -> [B, 77, H]"""
    _, _, v = (x.double() for x in V.split(qkv, heads, D))
    s = attn_scores64(qkv, heads)
    future = torch.triu(torch.ones((T, T), dtype=torch.bool), 1)
    o = torch.softmax(s.masked_fill(future, -math.inf), -1) @ v
    return o.permute(0, 2, 1, 3).reshape(qkv.shape[0], T, heads * D)


ATTN_FAULTS = ("future_key", "no_diagonal", "scale1", "acc_not_rescaled", "l_not_rescaled", "next_head_k", "kv_swap", "last_row_dropped")


def attn_model(qkv, heads, fault=None):
    """text_attn_kernel in fp32 with its rounding points -> [B, 77, H] fp64 (holding fp16 values; NaN where nothing is stored).
    fault: future_key (j <= i + 1), no_diagonal (j < i), scale1 (q not scaled), acc_not_rescaled (acc += p v when the maximum rises),
    l_not_rescaled (l += p), next_head_k (head h reads K of head (h + 1) mod heads), kv_swap (K and V column blocks exchanged),
    last_row_dropped (query 76 stores nothing)"""
    q, k, v = (x.numpy().astype(F32) for x in V.split(qkv, heads, D))
    if fault == "kv_swap":
        k, v = v, k
    if fault == "next_head_k":
        k = k[:, [(i + 1) % heads for i in range(heads)]]
    qs = q * F32(1.0 if fault == "scale1" else 0.125)
    R = q.shape[0]
    s = np.zeros((R, heads, T, T), F32)
    for d in range(D):
        s = fma32(s, qs[..., :, None, d], k[..., None, :, d])
    i = np.arange(T)
    last = i + 1 if fault == "future_key" else (i - 1 if fault == "no_diagonal" else i)
    m = np.full((R, heads, T), -np.inf, F32)
    l = np.zeros((R, heads, T), F32)
    acc = np.zeros((R, heads, T, D), F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(T):
            live = j <= last
            sj = s[..., j]
            mn = np.maximum(m, sj)
            corr = np.where(np.isneginf(m), 0.0, np.exp((m - mn).astype(F64))).astype(F32)
            p = np.exp((sj - mn).astype(F64)).astype(F32)
            ln = (l + p).astype(F32) if fault == "l_not_rescaled" else fma32(p, l, corr)
            ca = np.ones_like(corr) if fault == "acc_not_rescaled" else corr
            an = fma32((acc * ca[..., None]).astype(F32), p[..., None], v[..., j, None, :])
            m = np.where(live, mn, m)
            l = np.where(live, ln, l)
            acc = np.where(live[:, None], an, acc)
        inv = (F32(1.0) / l).astype(F32)
        out = (acc * inv[..., None]).astype(F32).astype(np.float16).astype(F64)
    if fault == "last_row_dropped":
        out[:, :, T - 1] = np.nan
    return torch.from_numpy(np.ascontiguousarray(out.transpose(0, 2, 1, 3).reshape(R, T, heads * D)))


@functools.lru_cache(maxsize=None)
def attn_reference(c: AT):
    """-> qkv, ref (fp64), E_model, bound: computed once and shared (do not modify)"""
    qkv = attn_qkv(c)
    ref = attn_ref64(qkv, c.heads)
    e_model = max_row_err(attn_model(qkv, c.heads), ref, D)
    return qkv, ref, e_model, FACTOR * e_model


# =================================================================================================================================
# embed, assemble, pool, cls_rows, broadcast_rows: exact
# =================================================================================================================================
@dataclass(frozen=True)
class GL:
    H: int
    N: int                     # batch rows (embed, pool: B; assemble, cls_rows: images; broadcast_rows: rows)
    Tk: int = T                # tokens per row (assemble, cls_rows)
    seed: int = 0

    @property
    def id(self):
        return f"H{self.H}N{self.N}" + (f"T{self.Tk}" if self.Tk != T else "")


VOCAB = 11
EDGE_IDS = (-5, 0, VOCAB - 1, VOCAB, VOCAB + 7, 3, 3, 0)
EDGE_EOS = (-1, 0, 76, 77, 200)
ASSEMBLE_T = (2, 5, 50, 257)
_HN = [(H, N) for H in H_VALUES for N in (1, 3)]
EMBED = [GL(H, N, seed=3100 + i) for i, (H, N) in enumerate(_HN)]
POOL = [GL(H, N, seed=3200 + i) for i, (H, N) in enumerate(_HN)]
ASSEMBLE = [GL(H, N, ASSEMBLE_T[(i + i // 4) % 4], seed=3300 + i) for i, (H, N) in enumerate(_HN)] + [GL(64, 3, 257, seed=3320), GL(1664, 3, 257, seed=3321)]
CLS_ROWS = [GL(c.H, c.N, c.Tk, seed=c.seed + 100) for c in ASSEMBLE]
BROADCAST = [GL(H, N, seed=3500 + i) for i, (H, N) in enumerate(_HN)] + [GL(8, 3, seed=3520), GL(8 * 257, 3, seed=3521), GL(16 * 768, 3, seed=3522), GL(8, 1, seed=3523)]
GLUE_REFUSED = dict(embed=("H%8", "B0", "vocab0", "null_ids", "null_x"), pool=("H0", "B0", "null_eos", "null_out"),
                    assemble=("H%8", "T1", "N0", "null_cls", "null_x"), cls_rows=("H%8", "T0", "N0", "null_dst"),
                    broadcast_rows=("n%8", "rows0", "null_src", "null_dst"), act_inplace=("n%8", "n0", "act2", "null_x"),
                    gelu_inplace=("n%8", "n0", "null_x"))


def _table(rng, rows, H):
    """[rows, H] fp16 values, every row with its own scale and sign"""
    return h16(rng.standard_normal((rows, H)) * _scales(rng, (rows, 1)))


def _h(a):
    return np.asarray(a, dtype=F64).astype(np.float16)


def _sum16(a, b):
    """(a.float() + b.float()).half() as fp64"""
    return (torch.from_numpy(_h(a)).float() + torch.from_numpy(_h(b)).float()).half().double().numpy()


def embed_inputs(c: GL):
    rng = np.random.default_rng(c.seed)
    ids = rng.integers(-2, VOCAB + 3, (c.N, T)).astype(np.int32)
    ids[:, :len(EDGE_IDS)] = EDGE_IDS
    ids[-1, T - 1] = VOCAB + 7                                  # the last row of the launch holds an edge id too
    return dict(ids=ids, tok=_table(rng, VOCAB, c.H), pos=_table(rng, T, c.H))


def embed_model(c: GL, fault=None):
    """text_embed_kernel -> x [N * 77, H].  fault: pos_row (position row `row`, not row % 77: rows past the table read nothing the
    test owns, NaN), no_clamp (modelled as id mod vocab)"""
    i = embed_inputs(c)
    ids = i["ids"].reshape(-1)
    idc = ids % VOCAB if fault == "no_clamp" else np.clip(ids, 0, VOCAB - 1)
    row = np.arange(c.N * T)
    pos = np.concatenate([i["pos"], np.full(((c.N - 1) * T, c.H), np.nan)]) if fault == "pos_row" else i["pos"]
    return _sum16(i["tok"][idc], pos[row if fault == "pos_row" else row % T])


def assemble_inputs(c: GL):
    rng = np.random.default_rng(c.seed)
    return dict(patch=_table(rng, c.N * (c.Tk - 1), c.H), cls=_table(rng, 1, c.H)[0], pos=_table(rng, c.Tk, c.H))


def assemble_model(c: GL, fault=None):
    """vit_assemble_kernel -> x [N * T, H].  fault: pos_row (pos[row]), patch_stride (image n's patches start at n T), t_not_minus_1
    (token t takes patch t), cls_pos1 (the class row takes pos[1]); a read past a table is NaN"""
    i = assemble_inputs(c)
    Tk = c.Tk
    row = np.arange(c.N * Tk)
    t, n = row % Tk, row // Tk
    pad = np.full((c.N * Tk + 1, c.H), np.nan)
    patch, pos = np.concatenate([i["patch"], pad]), np.concatenate([i["pos"], pad])
    pi = n * (Tk if fault == "patch_stride" else Tk - 1) + (t if fault == "t_not_minus_1" else t - 1)
    src = np.where((t == 0)[:, None], i["cls"][None, :], patch[np.maximum(pi, 0)])
    prow = row if fault == "pos_row" else t
    if fault == "cls_pos1":
        prow = np.where(t == 0, 1, prow)
    return _sum16(src, pos[prow])


def pool_inputs(c: GL):
    """every row of a case has another EOS position; the 12 cases walk EDGE_EOS, and one of the three-row ones holds an ordinary 40"""
    rng = np.random.default_rng(c.seed)
    k = c.seed % 100
    eos = np.array([EDGE_EOS[(k + 2 * b) % 5] for b in range(c.N)], dtype=np.int32)
    if c.N == 3 and k % 4 == 3:
        eos[1] = 40
    return dict(h=_table(rng, c.N * T, c.H).reshape(c.N, T, c.H), eos=eos)


def pool_model(c: GL, fault=None):
    """text_pool_kernel -> out [N, H] (fp32 holding fp16 values).  fault: one_eos (eos[0] for every row), no_clamp (position mod 77)"""
    i = pool_inputs(c)
    e = i["eos"].copy()
    if fault == "one_eos":
        e[:] = e[0]
    e = e % T if fault == "no_clamp" else np.clip(e, 0, T - 1)
    return i["h"][np.arange(c.N), e].copy()


def cls_inputs(c: GL):
    rng = np.random.default_rng(c.seed)
    return dict(x=_table(rng, c.N * c.Tk, c.H).reshape(c.N, c.Tk, c.H))


def cls_model(c: GL, fault=None):
    """vit_cls_rows_kernel -> dst [N, H].  fault: row_stride (image n read at row n, not n T)"""
    x = cls_inputs(c)["x"].reshape(c.N * c.Tk, c.H)
    return x[np.arange(c.N) * (1 if fault == "row_stride" else c.Tk)].copy()


def broadcast_inputs(c: GL):
    rng = np.random.default_rng(c.seed)
    return dict(src=(rng.standard_normal(c.H) * _scales(rng, c.H) * 3).astype(F32))            # fp32 values: the kernel rounds


def broadcast_model(c: GL, fault=None):
    """broadcast_rows_kernel -> dst [rows, n] = fp16(src).  fault: first_row_only"""
    out = np.broadcast_to(broadcast_inputs(c)["src"].astype(np.float16).astype(F64), (c.N, c.H)).copy()
    if fault == "first_row_only":
        out[1:] = np.nan
    return out


GLUE = dict(embed=(EMBED, embed_model, ("pos_row", "no_clamp")),
            assemble=(ASSEMBLE, assemble_model, ("pos_row", "patch_stride", "t_not_minus_1", "cls_pos1")),
            pool=(POOL, pool_model, ("one_eos", "no_clamp")),
            cls_rows=(CLS_ROWS, cls_model, ("row_stride",)),
            broadcast_rows=(BROADCAST, broadcast_model, ("first_row_only",)))


def same_bits(got, want):
    """exact equality of fp16 / fp32 values held in fp64 arrays, signed zeros included; a NaN in `got` (nothing stored) never matches"""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    return got.shape == want.shape and bool(np.isfinite(got).all()) and bool(((got == want) & (np.signbit(got) == np.signbit(want))).all())


# =================================================================================================================================
# activations
# =================================================================================================================================
C_QG = float(F32(1.702))
K_SQRT_HALF = F32(0.70710678118654752)
ACT_TAIL_N = (8, 8 * 255, 8 * 256, 8 * 257)
ACT_FAULTS = ("const_1.7", "sigmoid_of_x", "tanh_gelu", "act_inverted")


def all_fp16():
    """all 63488 finite fp16 values, in a seeded shuffle (so every launch tail holds values of every magnitude)"""
    v = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    v = v[np.isfinite(v)]
    return v[np.random.default_rng(3600).permutation(v.size)]


def _erf64(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, dtype=F64))).numpy()


def act_ref64(x, act):
    """x sigmoid(c x) (act 0) / x / 2 (1 + erf(x / sqrt 2)) (act 1) in fp64; -0 where the value underflows"""
    x = np.asarray(x, dtype=F64)
    with np.errstate(over="ignore"):
        if act == 0:
            return x / (1.0 + np.exp(-C_QG * x))
        return 0.5 * x * torch.erfc(torch.from_numpy(-x / math.sqrt(2.0))).numpy()


def act_bound(x, act, kernel="act_inplace"):
    """-> (rounding, rest) per element (module docstring)"""
    x = np.asarray(x, dtype=F64)
    ref = act_ref64(x, act)
    rounding = 0.5 * ulp16(ref)
    if kernel == "gelu_inplace":
        return rounding, np.abs(x) * (1.5e-7 + 8 * EPS)
    if act == 0:
        y = C_QG * x
        dy = np.abs(y) * 2.0 ** -24
        with np.errstate(over="ignore"):
            return rounding, e_silu(y, dy) / C_QG + np.abs(x) * dy / (1.0 + np.exp(np.abs(y) - dy))
    return rounding, np.abs(x) / 2 * (16 * EPS * np.abs(_erf64(x / math.sqrt(2.0))) + 3 * EPS)


def act_model32(x, act, fault=None):
    """act_inplace_kernel in fp32, every operation rounded once and exp / erf evaluated exactly -> fp64 holding fp16 values.
    fault: const_1.7, sigmoid_of_x (x sigmoid(x)), tanh_gelu (act 1 by the tanh form), act_inverted"""
    f = np.asarray(x, dtype=np.float16).astype(F32)
    if fault == "act_inverted":
        act = 1 - act
    with np.errstate(over="ignore"):
        if act == 0:
            c = F32(1.7) if fault == "const_1.7" else (F32(1.0) if fault == "sigmoid_of_x" else F32(1.702))
            e = np.exp(-((c * f).astype(F32)).astype(F64)).astype(F32)
            r = (f / (F32(1.0) + e).astype(F32)).astype(F32)
        elif fault == "tanh_gelu":
            f64 = f.astype(F64)
            r = (0.5 * f64 * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (f64 + 0.044715 * f64 ** 3)))).astype(F32)
        else:
            a = (f * K_SQRT_HALF).astype(F32)
            s = (F32(1.0) + _erf64(a.astype(F64)).astype(F32)).astype(F32)
            r = ((F32(0.5) * f).astype(F32) * s).astype(F32)
    return r.astype(np.float16).astype(F64)


def gelu_model32(x):
    """common.h gelu_erf_f in fp32 (rcp and exp2 evaluated exactly, fp contraction ignored) -> fp64 holding fp16 values"""
    f = np.asarray(x, dtype=np.float16).astype(F32)
    ax = (np.abs(f) * K_SQRT_HALF).astype(F32)
    t = (1.0 / (F32(1.0) + (F32(0.3275911) * ax).astype(F32)).astype(F64)).astype(F32)
    poly = F32(1.061405429) * t
    for k in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        poly = (t * (F32(k) + poly).astype(F32)).astype(F32)
    with np.errstate(under="ignore"):
        ex = np.exp2(((-ax * ax).astype(F32) * F32(1.4426950408889634)).astype(F32).astype(F64)).astype(F32)
    erfc = (poly * ex).astype(F32)
    cdf = np.where(f >= 0, (F32(1.0) - (F32(0.5) * erfc).astype(F32)).astype(F32), (F32(0.5) * erfc).astype(F32))
    return (f * cdf).astype(F32).astype(np.float16).astype(F64)


def act_ratio(got, x, act, kernel="act_inplace"):
    """max (|got - ref64| - rounding) / rest; inf when a stored zero carries the wrong sign or an element is not finite"""
    got = np.asarray(got, dtype=F64)
    ref = act_ref64(x, act)
    zero = got == 0
    if bool((np.signbit(got[zero]) != np.signbit(ref[zero])).any()):
        return math.inf
    return ratio(got, ref, *act_bound(x, act, kernel))
