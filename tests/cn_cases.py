"""Cases, inputs, fp64 references, fp32 models, fault models and per-element bounds of the ControlNet kernels of
cfgpp_amd/csrc/controlnet_kernels.hip that had no test of their own: cn_conv3x3_kernel (three input layouts, two strides, two output
layouts, optional SiLU and bias) and cn_residual_nchw_kernel (numpy / torch on the CPU, no HIP).

Shared by tests/test_cn_cases_cpu.py (the table reaches every launcher branch, the fp32 model of a correct kernel passes, every fault
model fails: no GPU) and tests/test_gpu_cn_kernels.py (the kernels against the same references).

cn_conv3x3.  Reference: torch's conv2d(padding=1, stride) in fp64 of the fp16-ROUNDED input (in_kind 2 hands the kernel fp32 values
that are not fp16 numbers: the kernel rounds them, as the pipeline hands the net an fp16 image) with fp32 weights and bias, then,
with silu, SiLU in fp64 of the fp16-rounded convolution (torch's conv2d then F.silu on fp16 tensors).  Weights are gaussian, so not
symmetric in ky / kx; every batch row and input channel has its own scale and sign.  Ho = (Hi - 1) / stride + 1.
Bounds, per element; EPS = 2^-23, the recorded ratio is max (|got - ref64| - rounding) / rest and must not exceed 1.
    T = sum |x| |w| + |bias| (fp64),  K = 9 Ci,  dconv = (K + 8) EPS T        the store bound of tests/small_cases.py: K additions and K
                                                                             products (no contraction: 2^-24 each), and the epilogue
  silu = 0:  rounding = 0.5 ulp16(got),  rest = dconv
  silu = 1:  the kernel's fp16 convolution h lies within dv = dconv + ulp16(|conv64| + dconv) of the reference's v = fp16(conv64)
             (rounding is monotone: the two fp16 values differ by at most the distance of their arguments plus one spacing), and
             |silu(h) - silu(v)| <= 1.1 dv (1.1 >= max |silu'|):
             rounding = 0.5 ulp16(got) + 1.1 ulp16(|conv64| + dconv)         the output's rounding and the second, inner one
             rest     = 1.1 dconv + E_silu(v; dv)                            small_cases.e_silu: exponential, addition, division
             (the kernel calls expf, not __expf; E_silu's exponential term (|x| + 1) EPS covers a 1-ulp expf as well)
With out_pad = 1 the destination is halo-padded; the halo (and every guard) is prefilled with a NaN pattern and must hold the same
bits afterwards.  The model returns the whole destination with NaN where nothing is stored.
The grid of the launch is capped at 2^20 blocks of 256 threads; 2^28 outputs are out of reach of a test that takes seconds (512 MiB of
fp16 output alone), so the grid-stride loop's second trip is NOT covered here.

residual_nchw: bit-exact against ((v.float() * scale).half()).float() read from the interior of a halo-padded NHWC tensor whose halo
holds NaN, written as dense NCHW fp32.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from igemm_cases import ulp16
from small_cases import EPS, F32, F64, _scales, e_silu, h16, ratio, silu64, violations  # noqa: F401

# Kernel ratios on the MI355X (profiles/tower_cases/tower_case_parity.jsonl), max over elements of (|got - ref64| - rounding) / rest,
# min / median / max over the cases of tests/test_gpu_cn_kernels.py (<= 0: every element within the rounding term alone):
#   cn_conv3x3, silu = 0 (15 cases)   -26.3 / -0.002 / 0.003        cn_conv3x3, silu = 1 (13 cases)   -152 / -0.032 / -0.001
#   residual_nchw: exact.
# No ratio is above 0.003: with at most 2304 terms the accumulation stays far inside (K + 8) EPS T, the fp16 rounding of the output
# is the whole error; the fp32 model gives the same maximum.
SIZES = ((1, 1), (1, 6), (5, 7), (8, 8), (9, 4))
CHANNELS = ((1, 1), (3, 16), (16, 96), (96, 32))


@dataclass(frozen=True)
class CV:
    Ci: int
    Co: int
    Hi: int
    Wi: int
    stride: int
    in_kind: int               # 0 NHWC fp16, 1 NCHW fp16, 2 NCHW fp32
    silu: int
    bias: int
    out_pad: int
    R: int
    seed: int = 0

    @property
    def Ho(self):
        return (self.Hi - 1) // self.stride + 1

    @property
    def Wo(self):
        return (self.Wi - 1) // self.stride + 1

    @property
    def id(self):
        return (f"C{self.Ci}-{self.Co}-{self.Hi}x{self.Wi}-s{self.stride}-k{self.in_kind}" + ("-silu" if self.silu else "") + ("" if self.bias else "-nob")
                + ("-pad" if self.out_pad else "") + f"-R{self.R}")


def _conv_table():
    """every size x every channel pair, the flags walking their values with co-prime periods; (256, 256) at 5 x 7 only"""
    out = []
    n = 0
    for hw in SIZES:
        for ch in CHANNELS:
            out.append(CV(ch[0], ch[1], hw[0], hw[1], 1 + n % 2, (n // 2) % 3, (n // 3) % 2, (n // 5) % 2, (n // 7 + n) % 2, 1 if n % 3 else 3, seed=3700 + n))
            n += 1
    out += [CV(256, 256, 5, 7, 1, 1, 0, 0, 0, 1, seed=3730), CV(256, 256, 5, 7, 2, 2, 1, 1, 1, 3, seed=3731),
            CV(3, 16, 9, 4, 2, 1, 0, 0, 0, 3, seed=3732), CV(16, 96, 5, 7, 2, 0, 0, 1, 1, 3, seed=3733), CV(3, 16, 1, 6, 2, 2, 1, 0, 0, 1, seed=3734),
            CV(96, 32, 1, 1, 2, 0, 1, 0, 1, 1, seed=3735), CV(1, 1, 9, 4, 1, 2, 0, 0, 0, 3, seed=3736), CV(16, 96, 8, 8, 2, 1, 1, 1, 0, 1, seed=3737)]
    return out


CONV = _conv_table()
CONV_REFUSED = ("Ci257", "Co0", "stride3", "in_kind3", "null_in", "null_out", "null_w", "R0")
CONV_FAULTS = ("ho_floor", "kykx_swapped", "plane_hi_hi", "pad0", "no_halo_offset", "bias_co_minus_1")


def cv_inputs(c: CV):
    """x: the NCHW map as the caller holds it (fp64; in_kind 2: fp32 values that are not fp16 numbers), x16: what the convolution
    sees, dev: the array in the device's layout and dtype, w OIHW fp32, wk [9][Ci][Co] fp32, bias fp32 or None"""
    rng = np.random.default_rng(c.seed)
    x = (rng.standard_normal((c.R, c.Ci, c.Hi, c.Wi)) * _scales(rng, (c.R, c.Ci, 1, 1))).astype(F32)
    if c.in_kind != 2:
        x = x.astype(np.float16).astype(F32)
    x16 = x.astype(np.float16)
    dev = np.ascontiguousarray(x16.transpose(0, 2, 3, 1)) if c.in_kind == 0 else (x16 if c.in_kind == 1 else x)
    w = (rng.standard_normal((c.Co, c.Ci, 3, 3)) * _scales(rng, (1, c.Ci, 1, 1)) / math.sqrt(9 * c.Ci)).astype(F32)
    bias = (rng.standard_normal(c.Co) * 0.5).astype(F32) if c.bias else None
    wk = np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(9, c.Ci, c.Co))
    return SimpleNamespace(x=x.astype(F64), x16=x16.astype(F64), dev=dev, w=w, wk=wk, bias=bias)


def _conv64(x, w, stride):
    return F.conv2d(torch.from_numpy(np.ascontiguousarray(x, dtype=F64)), torch.from_numpy(np.ascontiguousarray(w, dtype=F64)), padding=1, stride=stride).numpy()


@functools.lru_cache(maxsize=None)
def cv_reference(c: CV):
    """ref [R, Ho, Wo, Co] fp64 (the output's NHWC interior), conv (before SiLU), dconv"""
    i = cv_inputs(c)
    y, t = _conv64(i.x16, i.w, c.stride), _conv64(np.abs(i.x16), np.abs(i.w), c.stride)
    if c.bias:
        y, t = y + i.bias.astype(F64)[None, :, None, None], t + np.abs(i.bias).astype(F64)[None, :, None, None]
    y, t = y.transpose(0, 2, 3, 1), t.transpose(0, 2, 3, 1)
    dconv = (9 * c.Ci + 8) * EPS * t
    ref = silu64(h16(y)) if c.silu else y
    return SimpleNamespace(inputs=i, ref=ref, conv=y, dconv=dconv)


def cv_bound(c: CV, got):
    """-> (rounding, rest) per element of got [R, Ho, Wo, Co] (module docstring)"""
    r = cv_reference(c)
    rounding = 0.5 * ulp16(np.nan_to_num(got))
    if not c.silu:
        return rounding, r.dconv
    inner = ulp16(np.abs(r.conv) + r.dconv)
    return rounding + 1.1 * inner, 1.1 * r.dconv + e_silu(h16(r.conv), r.dconv + inner)


def cv_dest_shape(c: CV):
    p = 2 * c.out_pad
    return (c.R, c.Ho + p, c.Wo + p, c.Co)


def cv_interior(c: CV, dest):
    return dest[:, 1:c.Ho + 1, 1:c.Wo + 1] if c.out_pad else dest


def cv_model32(c: CV, fault=None):
    """cn_conv3x3_kernel in fp32 by the kernel's own index arithmetic (no fp contraction: product and sum rounded separately; the
    exponential evaluated exactly) -> the whole destination as fp64, NaN where nothing is stored; a read outside the input is NaN.
    fault: ho_floor (Ho = Hi / stride), kykx_swapped (tap (ky, kx) takes the weight of (kx, ky)), plane_hi_hi (NCHW plane stride Hi Hi),
    pad0 (taps start at the output pixel), no_halo_offset (a padded destination written from its corner), bias_co_minus_1"""
    i = cv_inputs(c)
    R, Ci, Co, Hi, Wi, s = c.R, c.Ci, c.Co, c.Hi, c.Wi, c.stride
    Ho, Wo = (Hi // s, Wi // s) if fault == "ho_floor" else (c.Ho, c.Wo)
    dest = np.full(int(np.prod(cv_dest_shape(c))), np.nan)
    if Ho == 0 or Wo == 0:
        return dest.reshape(cv_dest_shape(c))
    src = i.dev.astype(np.float16).astype(F64).reshape(-1)
    flat = np.concatenate([src, np.full(src.size * max(Hi, Wi) + 1, np.nan)])
    r, yo, xo = np.arange(R)[:, None, None], np.arange(Ho)[None, :, None], np.arange(Wo)[None, None, :]
    bias = np.zeros(Co, F32) if i.bias is None else (np.roll(i.bias, 1) if fault == "bias_co_minus_1" else i.bias)
    acc = np.broadcast_to(bias, (R, Ho, Wo, Co)).astype(F32)
    off = 0 if fault == "pad0" else 1
    plane = Hi * Hi if fault == "plane_hi_hi" else Hi * Wi
    for ky in range(3):
        for kx in range(3):
            y, x = yo * s + ky - off, xo * s + kx - off
            valid = np.broadcast_to((y >= 0) & (y < Hi) & (x >= 0) & (x < Wi), (R, Ho, Wo))
            wt = i.wk[kx * 3 + ky if fault == "kykx_swapped" else ky * 3 + kx]
            for ci in range(Ci):
                idx = ((r * Hi + y) * Wi + x) * Ci + ci if c.in_kind == 0 else r * Ci * plane + y * Wi + x + ci * plane
                v = np.where(valid, flat[np.clip(idx, 0, flat.size - 1)], 0.0)
                prod = (wt[ci].astype(F64)[None, None, None, :] * v[..., None]).astype(F32)
                acc = (acc + prod).astype(F32)
    h = acc.astype(np.float16)
    if c.silu:
        v = h.astype(F32)
        with np.errstate(over="ignore"):
            e = np.exp(-v.astype(F64)).astype(F32)
        h = (v / (F32(1.0) + e).astype(F32)).astype(F32).astype(np.float16)
    p = c.out_pad
    q = 0 if fault == "no_halo_offset" else p
    o = ((r * (Ho + 2 * p) + yo + q) * (Wo + 2 * p) + xo + q) * Co
    o = np.broadcast_to(o[..., None] + np.arange(Co), (R, Ho, Wo, Co))
    dest[o.reshape(-1)] = h.astype(F64).reshape(-1)
    return dest.reshape(cv_dest_shape(c))


def cv_ratio(c: CV, dest):
    """the recorded ratio of a whole destination; inf when an element of the write set is not finite or the halo was written"""
    dest = np.asarray(dest, dtype=F64)
    if c.out_pad:
        halo = np.ones(dest.shape, dtype=bool)
        halo[:, 1:c.Ho + 1, 1:c.Wo + 1] = False
        if not np.isnan(dest[halo]).all():
            return math.inf
    got = cv_interior(c, dest)
    return ratio(got, cv_reference(c).ref, *cv_bound(c, got))


def cv_branches(c: CV):
    return dict(odd_stride2=c.stride == 2 and (c.Hi % 2 == 1 or c.Wi % 2 == 1), non_square=c.Hi != c.Wi, blocks=c.R * c.Ho * c.Wo * c.Co > 256,
                tail=(c.R * c.Ho * c.Wo * c.Co) % 256 != 0)


# =================================================================================================================================
# residual_nchw
# =================================================================================================================================
@dataclass(frozen=True)
class RN:
    rows: int
    H: int
    W: int
    C: int
    scale: float
    seed: int = 0

    @property
    def id(self):
        return f"{self.rows}x{self.H}x{self.W}x{self.C}-s{self.scale:g}"


RESIDUAL_NCHW = [RN(3, 5, 7, 64, 1.0, seed=3800), RN(3, 5, 7, 64, 0.7, seed=3801), RN(1, 1, 1, 8, 1.0, seed=3802), RN(1, 1, 1, 8, 0.7, seed=3803)]
RESIDUAL_NCHW_REFUSED = ("rows0", "C0", "null_src", "null_out")


def rn_input(c: RN):
    """halo-padded NHWC fp16 [rows, H + 2, W + 2, C], NaN in the halo"""
    rng = np.random.default_rng(c.seed)
    x = np.full((c.rows, c.H + 2, c.W + 2, c.C), np.nan, dtype=np.float16)
    x[:, 1:c.H + 1, 1:c.W + 1] = (rng.standard_normal((c.rows, c.H, c.W, c.C)) * 3 * _scales(rng, (c.rows, 1, 1, c.C))).astype(np.float16)
    return x


def rn_model(c: RN, fault=None):
    """((v.float() * scale).half()).float() as dense NCHW -> [rows, C, H, W] fp64.  fault: no_halo_offset, nhwc_order"""
    x = torch.from_numpy(rn_input(c))
    v = x[:, :c.H, :c.W] if fault == "no_halo_offset" else x[:, 1:c.H + 1, 1:c.W + 1]
    out = (v.float() * c.scale).half().float()
    out = out.reshape(c.rows, c.C, c.H, c.W) if fault == "nhwc_order" else out.permute(0, 3, 1, 2)
    return out.double().numpy()
