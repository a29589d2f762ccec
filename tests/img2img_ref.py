"""The model the img2img tests compare against (include/cfgpp_img2img.h restated in plain numpy): the resample on exact
integer-rational coordinates (python ``Fraction``), the separable sum in the header's order, the forward-noise combination and the
Philox normals of tests/lcm_ref.py on stream 4, draw 0.  ``dtype=np.float64`` is the model (weights and sums unrounded beyond fp64);
``dtype=np.float32`` is the restatement of a correct kernel: each weight rounded once to fp32, one fp32 rounding per operation.  No
product code is imported here.

``faults``: a set of names; each switches ONE deliberate error into the model so that tests/test_img2img_cases_cpu.py can require
the bound to notice it (the house style of fault injection):
    align_corners         the align_corners=True coordinate d (in - 1) / (out - 1)
    no_half_pixel         the coordinate d in / out (the half-pixel offset is missing)
    swap_scales           each axis uses the other axis's in / out ratio
    clamp_wrong_edge      a tap outside [0, in) goes to the opposite edge
    tap_off_by_one        every tap index is one too large
    bilinear_for_bicubic  mode 3 evaluates mode 2
    broadcast_row_b       a one-row source is read at row b (what lies behind the source: ``src_parent``)
    noise_per_image_row   the Philox group index restarts at every image row instead of running along the chain's row
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import lcm_ref as R

MODES = {"identity": 0, "nearest-exact": 1, "bilinear": 2, "bicubic": 3}
CUBIC_A = -0.75
NOISE_STREAM, NOISE_DRAW = 4, 0
# Rounding points of the contract between the exact value and x', per source term: the two axis weights (2), wx * v (1), the row's
# adds (<= 3), wy * row (1), the column's adds (<= 3), a * r (1), the final add (1) = 12; the noise term has s * n and the final add
# (2 <= 12).  (1 + u)^12 - 1 <= 13 u for u = 2^-24, which takes in the second-order terms: c = 13.
C_ROUNDINGS = 13
U32 = 2.0 ** -24


def _cubic1(u):
    return ((CUBIC_A + 2.0) * u - (CUBIC_A + 3.0)) * u * u + 1.0


def _cubic2(u):
    return ((CUBIC_A * u - 5.0 * CUBIC_A) * u + 8.0 * CUBIC_A) * u - 4.0 * CUBIC_A


def axis_taps(d, n_in, n_out, mode, faults=(), other=None):
    """the taps of output index ``d`` of an axis of ``n_out`` elements over ``n_in``: ([indices], [float64 weights]); ``other``: the
    other axis's (in, out), which only the swap_scales fault reads"""
    if mode == 3 and "bilinear_for_bicubic" in faults:
        mode = 2
    if mode == 0:
        return [d], [1.0]
    s_in, s_out = other if ("swap_scales" in faults and other is not None) else (n_in, n_out)
    if "align_corners" in faults:
        coord = Fraction(d * (s_in - 1), s_out - 1) if s_out > 1 else Fraction(0)
    elif "no_half_pixel" in faults:
        coord = Fraction(d * s_in, s_out)
    else:
        coord = Fraction((2 * d + 1) * s_in - s_out, 2 * s_out)
    off = 1 if "tap_off_by_one" in faults else 0

    def cl(i):
        i += off
        if "clamp_wrong_edge" in faults:
            return n_in - 1 if i < 0 else (0 if i > n_in - 1 else i)
        return min(max(i, 0), n_in - 1)
    if mode == 1:
        return [cl(math.floor(coord + Fraction(1, 2)))], [1.0]
    if mode == 2:
        coord = max(coord, Fraction(0))
        q = math.floor(coord)
        t = coord - q
        return [cl(q), cl(q + 1)], [float(1 - t), float(t)]
    q = math.floor(coord)
    t, omt = float(coord - q), float(1 - (coord - q))
    return [cl(q - 1 + k) for k in range(4)], [_cubic2(t + 1.0), _cubic1(t), _cubic1(omt), _cubic2(omt + 1.0)]


def tap_tables(n_in, n_out, mode, faults=(), other=None):
    taps = [axis_taps(d, n_in, n_out, mode, faults, other) for d in range(n_out)]
    return np.array([t[0] for t in taps], np.int64), np.array([t[1] for t in taps], np.float64)


def resample(v, h, w, mode, dtype=np.float64, faults=(), absolute=False):
    """``v`` [R, C, h0, w0] (float64 array of the source values) -> r [R, C, h, w] by the header's expression sequence in ``dtype``;
    ``absolute``: sum |wy| |wx| |v| instead (the bound's magnitude)"""
    h0, w0 = v.shape[2:]
    iy, wy = tap_tables(h0, h, mode, faults, (w0, w))
    ix, wx = tap_tables(w0, w, mode, faults, (h0, h))
    v = v.astype(dtype)
    if iy.shape[1] == 1:
        out = v[:, :, iy[:, 0], :][:, :, :, ix[:, 0]]
        return np.abs(out) if absolute else out
    wy, wx = wy.astype(dtype), wx.astype(dtype)           # one rounding per weight in the fp32 restatement
    if absolute:
        v, wy, wx = np.abs(v), np.abs(wy), np.abs(wx)
    r = None
    for j in range(iy.shape[1]):
        vy = v[:, :, iy[:, j], :]
        row = wx[:, 0] * vy[..., ix[:, 0]]
        for k in range(1, ix.shape[1]):
            row = row + wx[:, k] * vy[..., ix[:, k]]
        term = wy[:, j][:, None] * row
        r = term if r is None else r + term
    return r


def noise_rows(B, C, h, w, seeds, faults=()):
    """the fp32 values of the in-kernel draw: the float64 normals of stream 4, draw 0, rounded to fp32, [B, C, h, w]"""
    if "noise_per_image_row" in faults:
        w4 = 4 * ((w + 3) // 4)
        rows = np.stack([np.tile(R.normals(w4, s, NOISE_DRAW, NOISE_STREAM)[:w], C * h) for s in seeds])
        return rows.reshape(B, C, h, w).astype(np.float32)
    return R.normal_rows(B, C * h * w, seeds, NOISE_DRAW, NOISE_STREAM).reshape(B, C, h, w).astype(np.float32)


def start(src, noise, a, s, B, h, w, mode, x_half=False, dtype=np.float64, faults=(), src_parent=None, seeds=None, C=4):
    """x [B, C, h, w] of cfgpp_img2img_start.  ``src`` [1 or B, C, h0, w0] array or None (a == 0); ``noise`` fp32 array, or None: drawn
    from ``seeds``; float64: the exact value of the contract's expression (no storage rounding); float32: a correct kernel's, stored
    dtype included (returned as float64 for comparison).  -> (x, magnitude |a| sum |w| |v| + |s n|)"""
    a32, s32 = np.float32(a), np.float32(s)
    x = mag = None
    if float(a32) != 0.0:
        v = np.asarray(src, np.float64)
        if v.shape[0] == 1 and B > 1:
            v = np.asarray(src_parent, np.float64)[:B] if "broadcast_row_b" in faults else np.broadcast_to(v, (B,) + v.shape[1:])
        r = resample(v, h, w, mode, dtype, faults)
        x = dtype(a32) * r
        mag = abs(float(a32)) * resample(v, h, w, mode, np.float64, faults, absolute=True)
    if float(s32) != 0.0:
        n = noise_rows(B, C, h, w, seeds, faults) if noise is None else np.asarray(noise, np.float32)
        sn = dtype(s32) * n.astype(dtype)
        x = sn if x is None else x + sn
        m2 = np.abs(float(s32) * n.astype(np.float64))
        mag = m2 if mag is None else mag + m2
    if dtype == np.float32:
        x = x.astype(np.float16) if x_half else x
    return x.astype(np.float64), mag


def bound(ref, mag, x_half):
    """the per-element bound of the issue: 0.5 ulp of the stored dtype at the model's value (taken at |ref| + the arithmetic term, so
    that a result just across a binade is covered) + C_ROUNDINGS 2^-24 (|a| sum |w| |v| + |s n|)"""
    arith = C_ROUNDINGS * U32 * mag
    store = np.float16 if x_half else np.float32
    top = np.minimum(np.abs(ref) + arith, float(np.finfo(store).max)).astype(store)
    return 0.5 * np.spacing(top).astype(np.float64) + arith
