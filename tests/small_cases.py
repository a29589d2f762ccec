"""Cases, inputs, fp64 references, fp32 models, per-element bounds and the expected dispatch of the tests of
cfgpp_amd/csrc/small_kernels.hip (numpy / torch on the CPU, no HIP).

Shared by tests/test_small_cases_cpu.py (the tables reach every instance and branch the launchers can emit, the fp32 model of a
correct kernel passes every condition, fault models do not: no GPU) and tests/test_gpu_small.py (the kernels against the same
references).

References restate the ORIGINAL operation in fp64 from seeded inputs: torch's conv2d on the concatenated NCHW input (conv_in,
conv_out), diffusers' get_timestep_embedding (flip_sin_to_cos=True, downscale_freq_shift=0), ``act(x) @ W.T + bias + addend``,
DiagonalGaussianDistribution.  Every sample and channel has its own scale and sign, so a row, channel or tap credited to the wrong
place shows.  ``*_model32`` are numpy fp32 ports of the kernels' arithmetic in the kernels' own order (lanes, chunks, shuffle tree),
every fp32 operation rounded once and every elementary function evaluated exactly; they read what the device reads (halo-padded
NHWC, the packed weights), so holding them against the conv2d references holds the tests' packing too.

Bounds, per element.  EPS = 2^-23.  ``rounding`` is the rounding of the stored value, ``rest`` everything else; the recorded ratio is
max (|got - ref64| - rounding) / rest and must not exceed 1.

  conv_in, conv_out (both kernels) - the store bound of tests/igemm_cases.py:
      rounding = 0.5 ulp16(got) for an fp16 output, 2^-24 |ref64| for an fp32 output
      rest     = (K + 8) EPS T,   T = |post_scale| sum |a| |w| + |bias| + |shift|  (fp64; conv_in: + |addend|),  K = 9 Cin
    K fp32 additions of the accumulation and at most 8 operations of the shuffle tree / epilogue, each relative 2^-24, with the
    factor 2 for FMA contraction and the dot2 instruction's inner order.  The clamp to [0, 1] is applied in the reference; it is
    1-Lipschitz, so the bound of the unclamped value holds.
    conv_in with an addend rounds conv + bias to fp16 BEFORE the addend is added (diffusers' `sample + controlnet_cond` on fp16
    tensors) and rounds the sum again; the reference adds in fp64 and rounds nowhere, so `rounding` gains the first rounding,
    0.5 ulp16(|ref64 - addend| + rest), exactly as the staged-residual epilogue does in igemm_cases.bound.
    fp32 `z * in_scale` followed by the rounding to fp16 is one IEEE multiplication and one IEEE conversion: the reference restates
    it in numpy float32, nothing of it is in the bound.  The folded 1x1 pre-conv (pre_w, pre_b) is not bit-reproducible (FMA
    contraction).  Kind `exact`: z, pre_w, pre_b short dyadic values and in_scale a power of two make every partial sum and the
    fp16 rounding of the pre-conv exact - the plain bound.  Kind `real` (in_scale = 1 / 0.18215, gaussian pre_w): the reference
    keeps the pre-conv v_k unrounded and `rest` gains sum_k |w_k| ulp16(v_k): half an ulp of the fp16 rounding of v_k, the other
    half for its fp32 accumulation.

  skinny GEMM (fp32 output):
      rounding = 2^-24 |ref64|
      dv   = (K + 8) EPS T + [silu_in] sum_k |w_k| E_silu(x_k),     T = sum |act(x_k)| |w_k| + |bias| + |addend|
      rest = dv                                                     without silu_out
           = 1.1 dv + E_silu(v; dv)                                 with silu_out (1.1 >= max |silu'| = 1.0998)
    E_silu is derived next to silu_f32 below.

  sinusoid (values rounded to fp16, stored as fp32):
      rounding = 0.5 ulp16(ref64),    rest = |darg| + E_trig
    x_j = -ln(10000) j / half.  The kernel evaluates q = fl(fl(c j) / half) with c = fl32(-ln 10000): relative 2^-24 for the
    constant, 2^-24 for the product, 2.5 ulp = 2.5 EPS for the division (j and half are exact in fp32): q = x (1 + d), |d| <= 3.5 EPS.
    e = expf(q) = exp(x) (1 + |x| d) within expf's own 3 ulp: relative (3.5 |x| + 3) EPS.  arg = fl(v e): another 2^-24.  So
    |darg| <= |v exp(x_j)| (3.5 |x_j| + 3.5) EPS, and |cos a - cos b|, |sin a - sin b| <= |a - b|.  E_trig = 4 EPS: 4 ulp of a
    result of magnitude at most 1.  expf, cosf, sinf are the device library's; the ROCm installation carries no document that
    states their ulp limits (only headers), so the OpenCL full-profile limits are used: 3 ulp for exp, 4 ulp for sin and cos, 2.5
    ulp for the division.

  posterior:
      moments: the store bound with K = 8 on the quant conv of the fp16-rounded encoder output (the rounding restated in the
               reference), the clamp of logvar to [-30, 20] applied in the reference.  They are fp16 values stored as fp32:
               rounding = 0.5 ulp16(got), rest = 16 EPS (sum |qw| |x| + |qb|).
      z:       against (mean + exp(logvar / 2) noise) scale in fp64 on THE MOMENTS THE SAME CALL RETURNED (scale = the fp32 value
               the kernel received).  h = logvar / 2 is exact; e = __expf(h) is relative (|h| + 1) EPS (derivation at silu_f32);
               e n, the sum and the product with scale are one fp32 rounding each:
               rounding = 2^-24 |ref64|,  rest = |scale| (|e n| (|h| + 2) EPS + (|mean| + |e n|) EPS).
      moments == null: z equals the z of the call that returned them, bit for bit.

  f16_to_f32_rows, fan-out: exact equality.

Untouched memory: every model here returns the whole destination with NaN where the kernel stores nothing; the GPU test prefills
the destination and guard regions with a NaN bit pattern and compares bits outside the write set.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from igemm_cases import REL_L2_BOUND, rel_l2, ulp16  # noqa: F401  (the store bound's pieces, reused)

# Kernel ratios on the MI355X, max over elements of (|got - ref64| - rounding) / rest, min / median / max per group of
# tests/test_gpu_small.py (profiles/small_cases/small_case_parity.jsonl; <= 0: every element within the rounding term alone):
#   conv_in                 -12.6 / 0.000 / 0.302   (the `real` pre-conv case; 0.010 without it)
#   conv_out, wave kernel   -24.3 / 0.000 / 0.005       conv_out, tiled kernel   0.000 / 0.001 / 0.004   (switch off: 0.000)
#   sinusoid                -0.15 / 0.033 / 0.078       skinny GEMM              0.000 / 0.001 / 0.021
#   posterior moments       -9.15 / -0.01 / 0.004       posterior z              -0.27 / 0.006 / 0.313
#   f16_to_f32_rows, fan-out: exact.
# No ratio is above 1 and none above 0.5: the accumulation term (K + 8) EPS T is a worst case over K roundings of one sign, a
# kernel's roundings cancel; the two largest are cases where `rest` is dominated by an fp16-ulp term (the pre-conv's rounding) and by
# the exp term (exp(logvar / 2) noise), which the kernels do come within a third of.
EPS = 2.0 ** -23
LOG2E_F32 = np.float32(1.4426950408889634)
F32, F64 = np.float32, np.float64


def cdiv(a, b):
    return -(-a // b)


def h16(a):
    """round to fp16, returned as fp64"""
    return np.asarray(a, dtype=F64).astype(np.float16).astype(F64)


def fma32(acc, a, b):
    """fl32(acc + a b): the product of two fp32 values is exact in fp64"""
    return (acc.astype(F64) + np.asarray(a, dtype=F64) * np.asarray(b, dtype=F64)).astype(F32)


def butterfly(acc):
    """`for s in 32 .. 1: acc += __shfl_xor(acc, s)` over the last axis (64 lanes) -> lane 0"""
    lane = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[..., lane ^ s]).astype(F32)
    return acc[..., 0]


def _scales(rng, shape):
    """one sign and one scale in 0.5 .. 2 per entry"""
    return np.where(rng.random(shape) < 0.5, -1.0, 1.0) * 2.0 ** rng.uniform(-1, 1, shape)


def ratio(got, ref, rounding, rest):
    """max over elements of (|got - ref| - rounding) / rest; inf when got is not finite everywhere"""
    got = np.asarray(got, dtype=F64)
    if not np.isfinite(got).all():
        return math.inf
    exc = np.abs(got - ref) - rounding
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(rest > 0, exc / rest, np.where(exc <= 0, 0.0, np.inf))
    return float(q.max())


def violations(got, ref, rounding, rest):
    """number of elements unwritten (not finite) or outside the bound"""
    got = np.asarray(got, dtype=F64)
    bad = ~np.isfinite(got)
    return int(bad.sum() + ((np.abs(np.nan_to_num(got) - ref) > rounding + rest) & ~bad).sum())


# =================================================================================================================================
# conv_in
# =================================================================================================================================
@dataclass(frozen=True)
class CI:
    H: int
    W: int
    Cout: int
    Cz: int = 4
    Cc: int = 0                # condition channels (0: cond == null)
    R: int = 1
    zB: int = 1
    cond_rows: int = 1
    add_rows: int = 0          # 0: addend == null
    z_half: int = 0
    bias: int = 1
    pre: int = 0               # 0 no pre-conv, 1 pre_w, 2 pre_w and pre_b (cfgpp_op_conv_in_ex)
    kind: str = "rand"         # rand | exact | real | scaled (no pre-conv, in_scale = 1 / 0.18215)
    seed: int = 0

    @property
    def Cin(self):
        return self.Cz + self.Cc

    @property
    def in_scale(self):
        return {"rand": 1.0, "exact": 2.0 if self.seed % 2 else 0.5, "real": 1 / 0.18215, "scaled": 1 / 0.18215}[self.kind]

    @property
    def entry(self):
        return "ex" if self.pre or self.kind != "rand" else "add"

    @property
    def id(self):
        s = f"{self.H}x{self.W}-Co{self.Cout}-Cz{self.Cz}" + (f"+{self.Cc}" if self.Cc else "")
        s += f"-R{self.R}z{self.zB}c{self.cond_rows}a{self.add_rows}" + ("-h" if self.z_half else "-f") + ("" if self.bias else "-nob")
        return s + (f"-pre{self.pre}" if self.pre else "") + (f"-{self.kind}" if self.kind != "rand" else "")


_RZ = ((1, 1, 1, 1), (4, 2, 1, 2), (3, 3, 3, 1), (6, 3, 2, 3), (8, 4, 2, 2))          # (R, zB, cond_rows, add_rows)


def _ci(hw, Cout, Cz, Cc, rz, add, **kw):
    R, zB, cr, ar = _RZ[rz]
    return CI(hw[0], hw[1], Cout, Cz, Cc, R, zB, cr if Cc else 1, ar if add else 0, **kw)


CONV_IN = [
    _ci((1, 1), 1, 1, 0, 0, 0, seed=10),
    _ci((3, 1), 24, 3, 0, 1, 1, z_half=1, seed=11),
    _ci((1, 5), 128, 4, 5, 2, 0, seed=12),
    _ci((5, 7), 320, 4, 5, 3, 1, z_half=1, seed=13),          # second Cout pass, pixel tail, cond_rows < zB with the addend
    _ci((16, 12), 320, 4, 0, 4, 1, seed=14),                  # SD's shape class: 12 full blocks of 16 pixels
    _ci((5, 7), 24, 8, 8, 1, 0, bias=0, seed=15),             # Cz + Cc = 16: the width of patch[][9 * 16]
    _ci((5, 7), 128, 8, 0, 0, 0, bias=0, z_half=1, seed=16),
    _ci((3, 1), 1, 1, 8, 2, 1, seed=17),
    _ci((16, 12), 24, 3, 5, 4, 1, z_half=1, seed=18),
    _ci((1, 5), 320, 4, 8, 3, 1, bias=0, seed=19),
    _ci((1, 1), 320, 8, 5, 4, 0, z_half=1, seed=20),
    _ci((16, 12), 128, 1, 0, 3, 0, seed=21),
    _ci((5, 7), 128, 4, 0, 1, 0, pre=2, kind="exact", seed=30),
    _ci((16, 12), 24, 4, 0, 1, 0, pre=1, kind="exact", z_half=1, seed=31),
    _ci((1, 1), 24, 8, 0, 0, 0, pre=2, kind="exact", seed=32),
    _ci((3, 1), 128, 3, 0, 2, 0, pre=1, kind="exact", bias=0, seed=33),
    _ci((5, 7), 320, 4, 0, 1, 0, pre=2, kind="real", seed=34),             # the VAE's post_quant_conv fold as it ships
    _ci((5, 7), 24, 4, 0, 1, 0, kind="scaled", seed=35),
]
CONV_IN_REFUSED = ("Cz9", "Cin17", "add_rows0", "null_z")


def ci_inputs(c: CI):
    rng = np.random.default_rng(c.seed)
    i = SimpleNamespace(cond=None, add=None, bias=None, pre_w=None, pre_b=None)
    if c.kind == "exact":
        i.z = rng.integers(-8, 9, (c.zB, c.Cz, c.H, c.W)).astype(F64) / 4
        i.pre_w = (rng.integers(-4, 5, (c.Cz, c.Cz)).astype(F64) / 4).astype(F32)
        i.pre_b = (rng.integers(-8, 9, c.Cz).astype(F64) / 8).astype(F32) if c.pre == 2 else None
    else:
        zs = 0.18215 if c.kind in ("real", "scaled") else 1.0
        i.z = h16(rng.standard_normal((c.zB, c.Cz, c.H, c.W)) * _scales(rng, (c.zB, c.Cz, 1, 1)) * zs)
        if c.pre:
            i.pre_w = (rng.standard_normal((c.Cz, c.Cz)) * 0.5).astype(F32)
            i.pre_b = (rng.standard_normal(c.Cz) * 0.3).astype(F32) if c.pre == 2 else None
    if c.Cc:
        i.cond = h16(rng.standard_normal((c.cond_rows, c.Cc, c.H, c.W)) * _scales(rng, (c.cond_rows, c.Cc, 1, 1)))
    i.w = h16(rng.standard_normal((c.Cout, c.Cin, 3, 3)) * _scales(rng, (1, c.Cin, 1, 1)) / math.sqrt(9 * c.Cin))
    if c.bias:
        i.bias = h16(rng.standard_normal(c.Cout) * 0.5)
    if c.add_rows:
        i.add = h16(rng.standard_normal((c.add_rows, c.H, c.W, c.Cout)) * _scales(rng, (c.add_rows, 1, 1, 1)))
    return i


def ci_scaled_z(c: CI, i):
    """fp16(fp32(z) * fp32(in_scale)): IEEE-exact, what both the reference's fp16 VAE and the kernel feed the (pre-)conv"""
    return (i.z.astype(F32) * F32(c.in_scale)).astype(np.float16).astype(F64)


def ci_nchw(c: CI, i, zc):
    """the concatenated NCHW input [R, Cin, H, W]: latent rows r % zB (zc: their channels), condition rows (r % zB) % cond_rows"""
    r = np.arange(c.R) % c.zB
    x = zc[r]
    return np.concatenate([x, i.cond[r % c.cond_rows]], axis=1) if c.Cc else x


def _conv(x, w):
    return F.conv2d(torch.from_numpy(np.ascontiguousarray(x, dtype=F64)), torch.from_numpy(np.ascontiguousarray(w, dtype=F64)), padding=1).numpy()


@functools.lru_cache(maxsize=None)
def ci_reference(c: CI):
    """ref [R, H, W, Cout] fp64 (the output's NHWC interior), pre = ref before the addend, rest of the bound"""
    i = ci_inputs(c)
    v = ci_scaled_z(c, i)
    extra = 0.0
    if c.pre:
        u = np.einsum("oj,bjhw->bohw", i.pre_w.astype(F64), v) + (i.pre_b.astype(F64)[None, :, None, None] if c.pre == 2 else 0.0)
        if c.kind == "real":
            extra = _conv(ulp16(u)[np.arange(c.R) % c.zB], np.abs(i.w))          # (a pre-conv case has no condition channels)
        v = u
    x = ci_nchw(c, i, v)
    y, t = _conv(x, i.w), _conv(np.abs(x), np.abs(i.w))
    if c.bias:
        y, t = y + i.bias[None, :, None, None], t + np.abs(i.bias)[None, :, None, None]
    y, t, extra = (a.transpose(0, 2, 3, 1) if isinstance(a, np.ndarray) else a for a in (y, t, extra))
    pre = y
    if c.add_rows:
        a = i.add[(np.arange(c.R) % c.zB) % c.add_rows]
        y, t = y + a, t + np.abs(a)
    return SimpleNamespace(inputs=i, ref=y, pre=pre, rest=(9 * c.Cin + 8) * EPS * t + extra)


def ci_bound(c: CI, got):
    """-> (rounding, rest) per element of got [R, H, W, Cout]"""
    r = ci_reference(c)
    rounding = 0.5 * ulp16(np.nan_to_num(got))
    if c.add_rows:
        rounding = rounding + 0.5 * ulp16(np.abs(r.pre) + r.rest)
    return rounding, r.rest


def ci_pack_w(w):
    """OIHW -> [9 * Cin][Cout] fp32, k = tap * Cin + ci"""
    O, I = w.shape[:2]
    return np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(9 * I, O)).astype(F32)


def ci_model32(c: CI, fault=None):
    """conv_in_kernel in fp32 -> [R, H, W, Cout] fp64 holding fp16 values, NaN where the kernel stores nothing.
    fault: row_div (r / zB for r % zB), tail (the last, partial block of 16 pixels is not written), second_pass (outputs >= 256
    not written), cond_off (condition channel + 1)"""
    i = ci_inputs(c)
    v = ci_scaled_z(c, i).astype(F32)
    if c.pre:
        acc = np.broadcast_to((i.pre_b if c.pre == 2 else np.zeros(c.Cz, F32))[None, :, None, None], v.shape).astype(F32)
        for j in range(c.Cz):
            acc = fma32(acc, i.pre_w[None, :, j, None, None], v[:, j:j + 1])
        v = acc.astype(np.float16).astype(F32)
    r = np.arange(c.R)
    zb = np.minimum(r // c.zB, c.zB - 1) if fault == "row_div" else r % c.zB
    x = v[zb]
    if c.Cc:
        cond = i.cond[zb % c.cond_rows].astype(F32)
        x = np.concatenate([x, np.roll(cond, -1, axis=1) if fault == "cond_off" else cond], axis=1)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    wk = ci_pack_w(i.w)
    acc = np.broadcast_to(i.bias.astype(F32) if c.bias else np.zeros(c.Cout, F32), (c.R, c.H, c.W, c.Cout)).astype(F32)
    for k in range(9 * c.Cin):
        tap, ci = divmod(k, c.Cin)
        dy, dx = tap // 3, tap % 3
        acc = fma32(acc, xp[:, ci, dy:dy + c.H, dx:dx + c.W, None], wk[k])
    out = acc.astype(np.float16)
    if c.add_rows:
        out = (out.astype(F32) + i.add[zb % c.add_rows].astype(F32)).astype(np.float16)
    out = out.astype(F64)
    if fault == "tail":
        out.reshape(c.R, c.H * c.W, c.Cout)[:, (c.H * c.W) // 16 * 16:] = np.nan
    if fault == "second_pass":
        out[..., 256:] = np.nan
    return out


def ci_branches(c: CI):
    """what of conv_in_kernel and its two launchers case c runs"""
    return dict(entry=c.entry, z_half=c.z_half, tail=(c.H * c.W) % 16 != 0, blocks=cdiv(c.H * c.W, 16) > 1, second_pass=c.Cout > 256,
                cond=c.Cc > 0, add=c.add_rows > 0, bias=c.bias, pre=c.pre, full_patch=c.Cin == 16,
                cond_and_add_rows_below_zB=c.Cc > 0 and c.add_rows > 0 and c.cond_rows < c.zB)


# =================================================================================================================================
# conv_out
# =================================================================================================================================
@dataclass(frozen=True)
class CO:
    C: int
    Cout: int
    R: int
    H: int
    W: int
    out_half: int
    post: int = 0              # 1: post_scale 0.5, post_shift 0.5, clamp to [0, 1]
    bias: int = 1
    seed: int = 0

    @property
    def id(self):
        return f"C{self.C}-Co{self.Cout}-{self.R}x{self.H}x{self.W}-" + ("h" if self.out_half else "f") + ("-post" if self.post else "") + ("" if self.bias else "-nob")

    @property
    def post_op(self):
        return (0.5, 0.5, 1) if self.post else (1.0, 0.0, 0)


_PIX = {1: (1, 1, 1), 9: (1, 3, 3), 35: (1, 5, 7), 240: (2, 10, 12)}


def _co(C, Cout, pix, half, **kw):
    return CO(C, Cout, *_PIX[pix], half, **kw)


CONV_OUT_WAVE = [
    _co(8, 1, 1, 1, seed=40), _co(8, 4, 9, 0, seed=41), _co(8, 3, 35, 1, seed=42), _co(8, 2, 240, 0, bias=0, seed=43),
    _co(24, 2, 35, 1, seed=44), _co(24, 4, 240, 1, post=1, seed=45), _co(24, 8, 9, 0, seed=46), _co(24, 1, 1, 0, seed=47),
    _co(64, 3, 35, 0, post=1, seed=48), _co(64, 4, 9, 1, seed=49), _co(64, 5, 240, 0, seed=50), _co(64, 1, 240, 1, seed=51),
    _co(64, 2, 1, 0, seed=52), _co(128, 2, 35, 1, bias=0, seed=53), _co(128, 8, 35, 0, post=1, seed=54), _co(128, 3, 240, 1, seed=55),
    _co(128, 4, 1, 0, seed=56), _co(512, 4, 9, 0, seed=57), _co(512, 1, 35, 1, seed=58), _co(512, 2, 1, 0, seed=59),
    _co(512, 5, 9, 0, seed=60), _co(512, 3, 35, 0, seed=61), _co(8, 8, 35, 0, seed=62), _co(128, 1, 9, 0, seed=63),
]
# H * W >= 16384 and C % 64 == 0; (4, 4096) and (2048, 8): tiles of which the halo guard and the store guard leave a sliver
CONV_OUT_TILED = [
    CO(64, 4, 1, 128, 128, 1, seed=70), CO(64, 3, 1, 129, 161, 0, post=1, seed=71), CO(64, 1, 1, 4, 4096, 0, seed=72),
    CO(64, 2, 1, 2048, 8, 1, seed=73), CO(128, 4, 1, 136, 152, 0, seed=74), CO(128, 3, 1, 4, 4096, 1, seed=75),
    CO(64, 4, 1, 2048, 8, 0, seed=76), CO(128, 2, 1, 129, 161, 0, bias=0, seed=77), CO(64, 1, 2, 128, 128, 1, seed=78),
]
CONV_OUT_REFUSED = ("Cout9", "C12", "Cout8_half")


def expected_launch_co(c: CO, tiled=1):
    """cfgpp_conv_out_last_launch after case c: (kernel 0 wave / 1 tiled, CO, out_is_half, workgroups)"""
    if c.Cout <= 4 and c.C % 64 == 0 and c.H * c.W >= 128 * 128 and tiled:
        return (1, 4 if c.out_half or c.Cout > 3 else 3, c.out_half, c.R * cdiv(c.H, 8) * cdiv(c.W, 32))
    return (0, 8 if c.Cout > 4 else 4, c.out_half, cdiv(c.R * c.H * c.W, 4))


def co_inputs(c: CO):
    rng = np.random.default_rng(c.seed)
    x = h16(rng.standard_normal((c.R, c.C, c.H, c.W)) * _scales(rng, (c.R, c.C, 1, 1)))
    w = h16(rng.standard_normal((c.Cout, c.C, 3, 3)) * _scales(rng, (c.Cout, c.C, 1, 1)) * (2.0 / math.sqrt(9 * c.C)))
    bias = h16(rng.standard_normal(c.Cout) * 0.5) if c.bias else None
    return SimpleNamespace(x=x, w=w, bias=bias)


@functools.lru_cache(maxsize=4)
def co_reference(c: CO):
    """ref [R, Cout, H, W] fp64 and T of the bound"""
    i = co_inputs(c)
    ps, sh, clamp = c.post_op
    y, t = _conv(i.x, i.w), _conv(np.abs(i.x), np.abs(i.w)) * abs(ps)
    if c.bias:
        y, t = y + i.bias[None, :, None, None], t + np.abs(i.bias)[None, :, None, None]
    y, t = y * ps + sh, t + abs(sh)
    unclamped = y
    if clamp:
        y = np.clip(y, 0.0, 1.0)
    return SimpleNamespace(inputs=i, ref=y, unclamped=unclamped, rest=(9 * c.C + 8) * EPS * t)


def co_bound(c: CO, got):
    r = co_reference(c)
    return (0.5 * ulp16(np.nan_to_num(got)) if c.out_half else 2.0 ** -24 * np.abs(r.ref)), r.rest


def co_device_layout(i):
    """what the device reads: x halo-padded NHWC [R, H+2, W+2, C], w [Cout][9][C]"""
    xp = np.pad(i.x.transpose(0, 2, 3, 1), ((0, 0), (1, 1), (1, 1), (0, 0)))
    return np.ascontiguousarray(xp), np.ascontiguousarray(i.w.transpose(0, 2, 3, 1).reshape(i.w.shape[0], 9, i.w.shape[1]))


def co_model32(c: CO, kernel, fault=None):
    """conv_out_kernel (kernel 0) / conv_out_tile_kernel (1) in fp32 -> [R, Cout, H, W] fp64, NaN where nothing is stored.
    fault: dx_mirrored (tap 5 reads dx = -1), stride_co (the output's channel stride is the instance's CO, not Cout),
    last_block (the last 64-channel block is skipped), last_row (the store guard drops row H - 1)"""
    i = co_inputs(c)
    xp, wk = (a.astype(F32) for a in co_device_layout(i))
    R, H, W, C, Co = c.R, c.H, c.W, c.C, c.Cout

    def window(tap, ch):
        dy, dx = tap // 3, tap % 3
        if fault == "dx_mirrored" and tap == 5:
            dx = 0
        return xp[:, dy:dy + H, dx:dx + W, ch, None]

    if kernel == 0:
        acc = np.zeros((R, H, W, Co, 64), F32)
        cpt = C // 8
        for ch in range(9 * cpt):
            tap, cc = ch // cpt, (ch % cpt) * 8
            for k in range(8):
                acc[..., ch % 64] = fma32(acc[..., ch % 64], window(tap, cc + k), wk[:, tap, cc + k])
        acc = butterfly(acc)
    else:
        acc = np.zeros((R, H, W, Co), F32)
        for cb in range(0, C - 64 if fault == "last_block" else C, 64):
            for tap in range(9):
                for k in range(cb, cb + 64, 2):               # v_dot2_f32_f16: two exact products and the accumulator, rounded once
                    acc = (acc.astype(F64) + window(tap, k).astype(F64) * wk[:, tap, k] + window(tap, k + 1).astype(F64) * wk[:, tap, k + 1]).astype(F32)
    ps, sh, clamp = c.post_op
    v = acc + (i.bias.astype(F32) if c.bias else F32(0))
    v = (v * F32(ps) + F32(sh)).astype(F32)
    if clamp:
        v = np.clip(v, F32(0), F32(1))
    v = (v.astype(np.float16) if c.out_half else v).astype(F64).transpose(0, 3, 1, 2)
    if fault == "last_row":
        v[:, :, H - 1] = np.nan
    if fault == "stride_co":
        co_inst = expected_launch_co(c, kernel)[1]
        flat = np.full(R * co_inst * H * W, np.nan)
        flat.reshape(R, co_inst, H, W)[:, :Co] = v
        v = flat[:R * Co * H * W].reshape(R, Co, H, W)
    return np.ascontiguousarray(v)


# =================================================================================================================================
# sinusoid
# =================================================================================================================================
@dataclass(frozen=True)
class SN:
    dim: int
    vals: tuple                # the timesteps; scalar form (vals == null): ONE value, written to `count` rows
    count: int
    scalar: int = 0
    out_ld: int = 0            # 0: dim
    out_off: int = 0

    @property
    def ld(self):
        return self.out_ld or self.dim

    @property
    def id(self):
        return f"d{self.dim}-n{self.count}-" + ("s" if self.scalar else "v") + "_".join(f"{v:g}" for v in self.vals) + (f"-ld{self.out_ld}+{self.out_off}" if self.out_ld else "")


_SV = (0.0, 1.0, 0.5, 499.25, 981.0, 999.0, 1024.0, 2048.0)
SINUSOID = [
    SN(2, _SV[:5], 5), SN(8, _SV[2:8], 6), SN(256, _SV[:6], 6, out_ld=2816, out_off=1280), SN(256, _SV[2:8], 6, out_ld=2816, out_off=2560),
    SN(320, _SV[3:8], 5), SN(320, (981.0,), 1, scalar=1), SN(320, (499.25,), 5, scalar=1), SN(2, (2048.0,), 6, scalar=1),
    SN(8, (0.0,), 1), SN(256, (999.0,), 1, scalar=1, out_ld=2816, out_off=1280), SN(8, (1.0,), 5, scalar=1, out_ld=2816, out_off=2560),
    SN(320, _SV[:2] + _SV[5:], 5),
]
SINUSOID_REFUSED = ("odd_dim", "count0")


def sn_values(c: SN):
    return np.array(c.vals * c.count if c.scalar else c.vals, dtype=F64)


def sn_ref64(c: SN):
    """diffusers get_timestep_embedding(t, dim, flip_sin_to_cos=True, downscale_freq_shift=0) in fp64 -> [count, dim]"""
    half = c.dim // 2
    exponent = -math.log(10000) * np.arange(half, dtype=F64) / (half - 0.0)
    emb = sn_values(c)[:, None] * np.exp(exponent)[None, :]
    emb = np.concatenate([np.sin(emb), np.cos(emb)], axis=-1)
    return np.concatenate([emb[:, half:], emb[:, :half]], axis=-1)            # flip_sin_to_cos


def sn_bound(c: SN):
    half = c.dim // 2
    x = -math.log(10000) * np.arange(half, dtype=F64) / half
    darg = np.abs(sn_values(c)[:, None] * np.exp(x)[None, :]) * (3.5 * np.abs(x)[None, :] + 3.5) * EPS
    return 0.5 * ulp16(sn_ref64(c)), np.concatenate([darg, darg], axis=-1) + 4 * EPS


def sn_model32(c: SN, fault=None):
    """sinusoid_kernel in fp32 -> the destination [count, out_ld] fp64, NaN where nothing is stored.
    fault: swapped (sin first), off_ignored (out_off = 0), half_minus_one (j / (half - 1))"""
    half = c.dim // 2
    j = np.arange(half, dtype=F32)
    den = F32(half - 1 if fault == "half_minus_one" and half > 1 else half)
    q = ((F32(-9.210340371976184) * j).astype(F32) / den).astype(F32)
    e = np.exp(q.astype(F64)).astype(F32)
    arg = (sn_values(c).astype(F32)[:, None] * e[None, :]).astype(F32).astype(F64)
    cs, sn = (f(arg).astype(F32).astype(np.float16).astype(F64) for f in (np.cos, np.sin))
    out = np.full((c.count, c.ld), np.nan)
    off = 0 if fault == "off_ignored" else c.out_off
    out[:, off:off + c.dim] = np.concatenate([sn, cs] if fault == "swapped" else [cs, sn], axis=-1)
    return out


# =================================================================================================================================
# skinny GEMM
# =================================================================================================================================
def silu_f32(x):
    """common.h silu_f, x / (1 + __expf(-x)), in fp32 with the exponential evaluated exactly.

    __expf(-x) is the hardware exp2 of t = fl(-x L), L = fl32(log2 e): |L - log2 e| <= 2^-25 |L| and the product's rounding 2^-24 |t|
    give |dt| <= 2^-23 |t|; exp2 turns that into the relative error ln 2 |dt| <= 2^-23 |x| (|t| ln 2 = |x|), and the instruction
    itself is good to one ulp, 2^-23: e = exp(-x) (1 + (|x| + 1) EPS).  silu = x / (1 + e) depends on e with the relative sensitivity
    e / (1 + e) = sigmoid(-x); the addition 1 + e is one rounding (2^-24), the division at most 2.5 ulp (OpenCL's limit; HIP's
    default division is correctly rounded).  Hence
        E_silu(x) = |silu(x)| (sigmoid(-x) (|x| + 1) + 3) EPS."""
    x = np.asarray(x, dtype=F32)
    e = np.exp2((-x * LOG2E_F32).astype(F32).astype(F64)).astype(F32)
    return (x / (F32(1) + e).astype(F32)).astype(F32)


def silu64(x):
    return x / (1 + np.exp(-x))


def e_silu(x, dx=0.0):
    """E_silu at any point within dx of x (fp64): |silu| grows by at most 1.1 dx, sigmoid(-x) is largest at the low end"""
    return (np.abs(silu64(x)) + 1.1 * dx) * (1 / (1 + np.exp(x - dx)) * (np.abs(x) + dx + 1) + 3) * EPS


@dataclass(frozen=True)
class SK:
    M: int
    N: int
    K: int
    ldx: str = "K"             # "K", "0" (one row for every m), "K+8"
    add: str = ""              # "" no addend, "N", "N+4": add_ld
    ldo: int = 0               # extra columns of the destination
    silu_in: int = 0
    silu_out: int = 0
    bias: int = 1
    seed: int = 0

    @property
    def ldx_v(self):
        return {"K": self.K, "0": 0, "K+8": self.K + 8}[self.ldx]

    @property
    def add_ld(self):
        return {"": 0, "N": self.N, "N+4": self.N + 4}[self.add]

    @property
    def id(self):
        return (f"M{self.M}N{self.N}K{self.K}-ldx{self.ldx}" + (f"-add{self.add}" if self.add else "") + (f"-ldo+{self.ldo}" if self.ldo else "")
                + f"-s{self.silu_in}{self.silu_out}" + ("" if self.bias else "-nob"))


SKINNY = [
    SK(1, 1280, 320, silu_out=1, seed=80), SK(5, 1280, 320, silu_in=1, silu_out=1, seed=81), SK(1, 7, 8, add="N", seed=82),
    SK(2, 1, 64, ldx="0", add="N+4", ldo=3, silu_in=1, seed=83), SK(4, 2, 512, ldx="K+8", seed=84), SK(5, 9, 520, ldx="0", add="N", bias=0, silu_out=1, seed=85),
    SK(8, 64, 2816, ldx="K+8", ldo=3, silu_out=1, seed=86), SK(64, 7, 320, add="N+4", silu_in=1, silu_out=1, seed=87),
    SK(64, 1280, 64, ldx="0", add="N", seed=88), SK(2, 9, 2816, silu_in=1, bias=0, seed=89), SK(1, 64, 520, ldx="K+8", add="N+4", ldo=3, silu_in=1, silu_out=1, seed=90),
    SK(4, 7, 8, ldx="0", silu_out=1, seed=91), SK(8, 2, 8, add="N", silu_in=1, seed=92), SK(1, 1, 512, bias=0, seed=93),
    SK(1, 2, 2816, silu_in=1, ldo=3, seed=94), SK(8, 1280, 512, silu_in=1, add="N+4", seed=95), SK(4, 64, 64, ldo=3, silu_in=1, silu_out=1, bias=0, seed=96),
    SK(2, 1280, 520, ldx="K+8", silu_out=1, seed=97), SK(5, 1, 8, silu_in=1, seed=98), SK(64, 9, 512, ldx="K+8", add="N", ldo=3, seed=99),
    SK(5, 2, 320, ldx="0", silu_in=1, silu_out=1, seed=100), SK(8, 9, 64, add="N+4", silu_out=1, seed=101),
]
SKINNY_REFUSED = ("K12", "M0")


def expected_launch_sk(c: SK):
    """(MB of the skinny_gemm_kernel<MB, 2> instance, grid.x, grid.y)"""
    return (1, cdiv(c.N, 8), 1) if c.M == 1 else (4, cdiv(c.N, 8), cdiv(c.M, 4))


def sk_inputs(c: SK):
    rng = np.random.default_rng(c.seed)
    rows = 1 if c.ldx == "0" else c.M
    x = rng.standard_normal((rows, c.K)) * 2 * _scales(rng, (rows, 1))
    hit = rng.random((rows, c.K)) < 0.02
    x = h16(np.where(hit, np.where(rng.random((rows, c.K)) < 0.5, -20.0, 20.0), x))          # SiLU saturates on both sides
    x[0, :2] = (20.0, -20.0)
    w = h16(rng.standard_normal((c.N, c.K)) * _scales(rng, (c.N, 1)) / math.sqrt(c.K))
    bias = h16(rng.standard_normal(c.N) * (8.0 if c.silu_out else 0.5)) if c.bias else None
    add = h16(rng.standard_normal((c.M, c.N)) * _scales(rng, (c.M, 1)) * (4.0 if c.silu_out else 1.0)) if c.add else None
    return SimpleNamespace(x=x, w=w, bias=bias, add=add)


@functools.lru_cache(maxsize=None)
def sk_reference(c: SK):
    i = sk_inputs(c)
    x = np.broadcast_to(i.x, (c.M, c.K))
    a = silu64(x) if c.silu_in else x
    v, t = a @ i.w.T, np.abs(a) @ np.abs(i.w).T
    if c.bias:
        v, t = v + i.bias, t + np.abs(i.bias)
    if c.add:
        v, t = v + i.add, t + np.abs(i.add)
    dv = (c.K + 8) * EPS * t + (e_silu(x) @ np.abs(i.w).T if c.silu_in else 0.0)
    ref = silu64(v) if c.silu_out else v
    rest = 1.1 * dv + e_silu(v, dv) if c.silu_out else dv
    return SimpleNamespace(inputs=i, ref=ref, rounding=2.0 ** -24 * np.abs(ref), rest=rest)


def sk_model32(c: SK, fault=None):
    """skinny_gemm_kernel in fp32 -> the destination [M, N + ldo] fp64, NaN where nothing is stored.
    fault: last_chunk (the last 8 values of K are dropped), ldx0_as_K (a broadcast x read with row stride K: rows m > 0 read past the
    row - modelled as zeros), add_row0 (addend row 0 for every m), silu_before_add"""
    i = sk_inputs(c)
    x = i.x.astype(F32)
    if c.ldx == "0":
        x = np.concatenate([x, np.zeros((c.M - 1, c.K), F32)]) if fault == "ldx0_as_K" else np.broadcast_to(x, (c.M, c.K))
    if c.silu_in:
        x = silu_f32(x)
    w = i.w.astype(F32)
    acc = np.zeros((c.M, c.N, 64), F32)
    nchunk = c.K // 8 - (1 if fault == "last_chunk" else 0)
    for ch in range(nchunk):
        for k in range(ch * 8, ch * 8 + 8):
            acc[..., ch % 64] = fma32(acc[..., ch % 64], x[:, None, k], w[None, :, k])
    v = butterfly(acc)
    if c.bias:
        v = (v + i.bias.astype(F32)).astype(F32)
    if fault == "silu_before_add" and c.silu_out:
        v = silu_f32(v)
    if c.add:
        v = (v + (i.add[:1] if fault == "add_row0" else i.add).astype(F32)).astype(F32)
    if c.silu_out and fault != "silu_before_add":
        v = silu_f32(v)
    out = np.full((c.M, c.N + c.ldo), np.nan)
    out[:, :c.N] = v
    return out


# =================================================================================================================================
# f16_to_f32_rows, fan-out
# =================================================================================================================================
@dataclass(frozen=True)
class RW:
    rows: int
    cols: int
    out_ld: int = 0
    out_off: int = 0

    @property
    def ld(self):
        return self.out_ld or self.cols

    @property
    def id(self):
        return f"{self.rows}x{self.cols}" + (f"-ld{self.out_ld}+{self.out_off}" if self.out_ld else "")


# 300 x 1024 elements: more than the 1024 blocks x 256 threads of the capped grid, the grid stride runs
ROWS = [RW(1, 1), RW(3, 7), RW(2, 1280), RW(300, 1024), RW(3, 7, 2816, 1280), RW(2, 1280, 2816, 1280), RW(1, 1, 2816, 2560), RW(2, 256, 2816, 2560),
        RW(300, 1024, 2816, 1280)]


def rw_input(c: RW):
    return np.random.default_rng(c.rows * 131 + c.cols).standard_normal((c.rows, c.cols)).astype(np.float16)


def rw_grid(c: RW):
    """(blocks, the grid-stride loop runs a second time)"""
    g = min(cdiv(c.rows * c.cols, 256), 1024)
    return g, c.rows * c.cols > g * 256


def rw_expected(c: RW):
    out = np.full((c.rows, c.ld), np.nan)
    out[:, c.out_off:c.out_off + c.cols] = rw_input(c).astype(F64)
    return out


@dataclass(frozen=True)
class FO:
    n16: tuple                 # 16-byte units per ROW of each segment (row_elems / 8)
    h: int = 1

    @property
    def units(self):
        return tuple(self.h * n for n in self.n16)

    @property
    def id(self):
        return f"h{self.h}-" + "_".join(str(n) for n in self.n16)


FANOUT_CAP = 2048
# units per segment that choose the loop path.  T = 256 * min(cdiv(most, 1024), 2048) threads per segment: 4 T >= n unless the cap
# holds, so 4 T - 1 is met at n = 4095 (T = 1024) and 4 T + 1 only under the cap (n = 2048 * 1024 + 1, 32 MiB per half)
FANOUT = [FO((1,)), FO((255,)), FO((1024,)), FO((1025,)), FO((4095,)), FO((FANOUT_CAP * 1024 + 1,)), FO((512, 3), h=2), FO((1, 5000, 300000)),
          FO((1025, 1024), h=2), FO((7, 4095, 1), h=1)]
FANOUT_REFUSED = ("row_elems", "alignment", "nseg4")


def fo_grid(c: FO):
    return min(cdiv(max(c.units), 1024), FANOUT_CAP)


def fo_copied(n, T, fault=None):
    """which of the n units of a segment fanout_rows_kernel copies with T threads; fault `tail`: the loop after the unrolled one is
    missing.  Unit i belongs to the pass that starts at (i / 4T) 4T + i % T; the unrolled loop takes it iff that start + 3 T < n."""
    i = np.arange(n)
    unrolled = (i // (4 * T)) * 4 * T + i % T + 3 * T < n
    return (unrolled if fault == "tail" else np.ones(n, dtype=bool)), unrolled


def fo_paths(c: FO):
    """per segment (the unrolled loop runs, the tail loop runs), and whether the block cap holds"""
    T = 256 * fo_grid(c)
    paths = []
    for n in c.units:
        _, unrolled = fo_copied(n, T)
        paths.append((bool(unrolled.any()), bool((~unrolled).any())))
    return paths, cdiv(max(c.units), 1024) > FANOUT_CAP


# =================================================================================================================================
# VAE posterior
# =================================================================================================================================
@dataclass(frozen=True)
class PO:
    B: int
    HW: int
    noise: int = 1
    clamp: int = 0             # 1: qb drives logvar channels above 20 and below -30
    scale: float = 0.18215
    seed: int = 0

    @property
    def id(self):
        return f"B{self.B}x{self.HW}-" + ("n" if self.noise else "mean") + ("-clamp" if self.clamp else "") + f"-{self.scale:g}"


POSTERIOR = [PO(1, 1, seed=110), PO(3, 35, noise=0, scale=0.13025, seed=111), PO(2, 256, clamp=1, seed=112), PO(1, 300, scale=0.13025, seed=113),
             PO(3, 35, clamp=1, scale=0.13025, seed=114), PO(1, 300, noise=0, clamp=1, seed=115), PO(2, 256, noise=0, seed=116), PO(1, 1, clamp=1, noise=0, seed=117)]


def po_inputs(c: PO):
    rng = np.random.default_rng(c.seed)
    co = (rng.standard_normal((c.B, 8, c.HW)) * 3 * _scales(rng, (c.B, 8, 1))).astype(F32)
    qw = (rng.standard_normal((8, 8)) * 0.4).astype(F32)
    qb = (rng.standard_normal(8) * 0.5).astype(F32)
    if c.clamp:
        qb[4:] = (45.0, -70.0, 30.0, -40.0)
    noise = rng.standard_normal((c.B, 4, c.HW)).astype(F32) if c.noise else None
    return SimpleNamespace(co=co, qw=qw, qb=qb, noise=noise)


def po_moments_ref(c: PO):
    """quant_conv on the fp16-rounded encoder output, logvar clamped -> ref [B, 8, HW] fp64, the unclamped value, rest of the bound"""
    i = po_inputs(c)
    x = i.co.astype(np.float16).astype(F64)
    m = np.einsum("oj,bjp->bop", i.qw.astype(F64), x) + i.qb.astype(F64)[None, :, None]
    t = np.einsum("oj,bjp->bop", np.abs(i.qw).astype(F64), np.abs(x)) + np.abs(i.qb).astype(F64)[None, :, None]
    ref = m.copy()
    ref[:, 4:] = np.clip(m[:, 4:], -30.0, 20.0)
    return SimpleNamespace(ref=ref, unclamped=m, rest=16 * EPS * t)


def po_z_ref(c: PO, moments):
    """DiagonalGaussianDistribution.sample() * scale in fp64 on the returned moments -> ref, rounding, rest"""
    i = po_inputs(c)
    m = np.asarray(moments, dtype=F64)
    s = float(F32(c.scale))
    h = 0.5 * m[:, 4:]
    en = np.exp(h) * (i.noise.astype(F64) if c.noise else 0.0)
    ref = (m[:, :4] + en) * s
    return ref, 2.0 ** -24 * np.abs(ref), abs(s) * (np.abs(en) * (np.abs(h) + 2) + np.abs(m[:, :4]) + np.abs(en)) * EPS


def po_model32(c: PO, fault=None):
    """vae_posterior_kernel in fp32 -> (z [B, 4, HW], moments [B, 8, HW]) fp64.  fault: no_clamp, logvar_not_halved"""
    i = po_inputs(c)
    x = i.co.astype(np.float16).astype(F32)
    acc = np.broadcast_to(i.qb[None, :, None], (c.B, 8, c.HW)).astype(F32)
    for j in range(8):
        acc = fma32(acc, i.qw[None, :, j, None], x[:, j:j + 1])
    m = acc.astype(np.float16).astype(F32)
    lv = m[:, 4:] if fault == "no_clamp" else np.clip(m[:, 4:], F32(-30), F32(20))
    h = lv if fault == "logvar_not_halved" else (F32(0.5) * lv).astype(F32)
    e = np.exp2((h * LOG2E_F32).astype(F32).astype(F64)).astype(F32)
    n = i.noise if c.noise else np.zeros((c.B, 4, c.HW), F32)
    z = (fma32(m[:, :4], e, n) * F32(c.scale)).astype(F32)
    return z.astype(F64), np.concatenate([m[:, :4], lv], axis=1).astype(F64)


GROUPS = dict(conv_in=CONV_IN, conv_out_wave=CONV_OUT_WAVE, conv_out_tiled=CONV_OUT_TILED, sinusoid=SINUSOID, skinny=SKINNY, rows=ROWS,
              fanout=FANOUT, posterior=POSTERIOR)
