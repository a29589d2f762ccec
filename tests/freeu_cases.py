"""Case table, inputs, fp32 kernel model, planted faults and the per-element bound of the FreeU op (csrc/freeu_kernel.hip), shared by
tests/test_freeu_cpu.py (no GPU) and tests/test_gpu_freeu.py.

Bound (derived from the number formats, not from the kernel's output), per element:
  skip:   |got - ref64| <= 0.5 ulp16(got) + (H W + 8) 2^-23 T,   T = |v| + 4 |s - 1| mean|v| over the plane
          - one fp16 rounding of the result, plus fp32 accumulation of H W terms in ANY order (<= H W 2^-24 sum|v| per sum, four sums
            scaled by |s - 1| / (H W), twice that for slack) and a few fp32 roundings of twiddles, products and the final add;
  hidden: |got - ref64| <= 0.5 ulp16(got) + 2^-23 |h b|          - one fp32 rounding of the product, one fp16 rounding
and at most MISMATCH_CAP of the scaled hidden elements may differ from the correctly rounded fp16 of the exact product."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

import freeu_ref as R

MISMATCH_CAP = 5e-3
LDS_PLANE_CAP = 64 * 1024          # csrc/freeu_kernel.hip: FREEU_LDS_PLANE_CAP
F32 = np.float32


@dataclasses.dataclass(frozen=True)
class Case:
    H: int
    W: int
    C_h: int
    C_s: int
    rows: int
    s: float
    b: float
    half: str = "both"              # "both" | "hidden" | "skip": which pointers the call passes
    seed: int = 0

    @property
    def id(self):
        return f"{self.H}x{self.W}-h{self.C_h}-s{self.C_s}-r{self.rows}-s{self.s}-b{self.b}-{self.half}"


def _table():
    out, k = [], 0
    planes = [(4, 4), (8, 8), (8, 16), (6, 10), (16, 16), (32, 32), (64, 64)]
    chs = [(64, 64), (128, 128), (192, 320), (1280, 640)]
    scales = [(0.2, 1.5), (0.9, 1.0), (0.0, 1.5), (1.0, 1.0)]
    for i, (H, W) in enumerate(planes):
        big = H * W >= 1024
        for j in range(2):
            C_h, C_s = chs[(i + j) % 4] if not big else chs[j]      # the large planes with the narrow tensors: quick references
            s, b = scales[(i + 2 * j) % 4]
            out.append(Case(H, W, C_h, C_s, 1 + 2 * ((i + j) % 2), s, b, seed=100 + k)); k += 1
    # wide tensors on a mid-size plane, every scale pair once more on 8 x 8
    out.append(Case(16, 16, 1280, 640, 1, 0.2, 1.5, seed=150))
    for n, (s, b) in enumerate(scales):
        out.append(Case(8, 8, 192, 320, 3, s, b, seed=160 + n))
    # half jobs
    out += [Case(8, 16, 128, 128, 3, 0.2, 1.5, "hidden", 170), Case(6, 10, 192, 320, 3, 0.2, 1.5, "skip", 171),
            Case(64, 64, 64, 64, 1, 0.9, 1.5, "skip", 172), Case(4, 4, 1280, 64, 1, 0.2, 1.6, "hidden", 173)]
    # slab widths 64 / 32 / 16 channels: chosen once rows * C_s / width reaches 256 workgroups - small planes, many rows
    out += [Case(4, 4, 64, 1280, 16, 0.2, 1.5, seed=180), Case(4, 4, 64, 320, 26, 0.2, 1.5, seed=181),
            Case(6, 10, 64, 320, 13, 0.9, 1.5, seed=182), Case(8, 8, 64, 1280, 16, 0.2, 1.0, "skip", 183)]
    # beyond the resident limit (H W * 8 channels * 2 bytes > 64 KiB): the two-phase path; and exactly at it
    out += [Case(64, 66, 64, 64, 1, 0.2, 1.5, seed=190), Case(72, 64, 128, 128, 1, 0.9, 1.5, "skip", 191),
            Case(32, 128, 64, 64, 1, 0.2, 1.5, "skip", 192)]
    return out


CASES = _table()
REFUSED = [dict(H=1, W=8, C_h=64, C_s=64, word="one-pixel axis"), dict(H=8, W=1, C_h=64, C_s=64, word="one-pixel axis"),
           dict(H=8, W=8, C_h=72, C_s=64, word="C_h=72"), dict(H=8, W=8, C_h=64, C_s=68, word="C_s=68"),
           dict(H=8, W=8, C_h=64, C_s=64, b=math.inf, word="non-finite"), dict(H=8, W=8, C_h=64, C_s=64, s=math.nan, word="non-finite")]


def expected_launch(c: Case):
    """what cfgpp_freeu_last_launch reports for case c: {path, channels per slab, skip workgroups, hidden workgroups}"""
    HW = c.H * c.W
    cs = nskip = 0
    resident = HW * 8 * 2 <= LDS_PLANE_CAP
    if c.half != "hidden":
        for w in (64, 32, 16, 8):
            if c.C_s % w or (resident and HW * w * 2 > LDS_PLANE_CAP):
                continue
            cs = w
            if c.rows * (c.C_s // w) >= 256:
                break
        nskip = c.rows * (c.C_s // cs)
    nhid = 0 if c.half == "skip" else min(max(-(-(c.rows * HW * (c.C_h // 16)) // 256), 1), 2048)
    path = 3 if c.half == "hidden" else (1 if resident else 2)
    return [path, cs, nskip, nhid]


# ---- inputs: a fault moves elements by about the size of the signal -------------------------------------------------------------
def make_inputs(c: Case):
    """(hidden, skip): interior NHWC fp16 arrays [rows, H, W, C].  Every plane has its own DC offset and planted cosines at
    frequency 1 along y, along x and on the diagonal (a real cosine holds +1 and -1), with plane-dependent phase, on noise."""
    rng = np.random.RandomState(c.seed)
    y = (2 * np.pi * np.arange(c.H) / c.H)[None, :, None, None]
    x = (2 * np.pi * np.arange(c.W) / c.W)[None, None, :, None]

    def tensor(C):
        pl = (c.rows, 1, 1, C)
        dc = rng.uniform(-1.0, 1.0, pl) + np.arange(C)[None, None, None, :] % 7 * 0.125
        p1, p2, p3 = (rng.uniform(0, 2 * np.pi, pl) for _ in range(3))
        a1, a2, a3 = (rng.uniform(0.4, 0.9, pl) for _ in range(3))
        v = dc + a1 * np.cos(y + p1) + a2 * np.cos(x + p2) + a3 * np.cos(y + x + p3) + 0.5 * rng.randn(c.rows, c.H, c.W, C)
        return v.astype(np.float16)
    return tensor(c.C_h), tensor(c.C_s)


def reference(c: Case, hidden, skip):
    """fp64 reference of what the call leaves in the two tensors (a tensor the call does not pass stays as it is)"""
    h, k = R.freeu_ref64(hidden if c.half != "skip" else None, skip if c.half != "hidden" else None, c.b, c.s)
    return (h if h is not None else hidden.astype(np.float64)), (k if k is not None else skip.astype(np.float64))


# ---- metric ---------------------------------------------------------------------------------------------------------------------
def ulp16(v):
    _, e = np.frexp(np.abs(np.asarray(v, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 11, -24))


def bound_skip(c: Case, got, skip_in):
    v = np.abs(skip_in.astype(np.float64))
    T = v + 4.0 * abs(float(F32(c.s)) - 1.0) * v.mean(axis=(1, 2), keepdims=True)
    return 0.5 * ulp16(got) + (c.H * c.W + 8) * 2.0 ** -23 * T


def bound_hidden(c: Case, got, hidden_in):
    return 0.5 * ulp16(got) + 2.0 ** -23 * np.abs(hidden_in.astype(np.float64) * float(F32(c.b)))


def worst_ratio(c: Case, got_h, got_k, hidden, skip, ref_h, ref_k):
    """max over elements of |got - ref| / bound for the two tensors (inf when something is not finite).  A tensor or a part of one
    the call must leave alone has to be bit-identical: any change there counts as inf."""
    gh, gk = np.asarray(got_h, dtype=np.float64), np.asarray(got_k, dtype=np.float64)
    if not (np.isfinite(gh).all() and np.isfinite(gk).all()):
        return math.inf, math.inf
    half = c.C_h // 2
    rh = rk = 0.0
    if c.half == "skip":
        rh = 0.0 if np.array_equal(gh, hidden.astype(np.float64)) else math.inf
    else:
        rh = float((np.abs(gh - ref_h)[..., :half] / bound_hidden(c, gh, hidden)[..., :half]).max())
        if not np.array_equal(gh[..., half:], hidden.astype(np.float64)[..., half:]):
            rh = math.inf
    if c.half == "hidden":
        rk = 0.0 if np.array_equal(gk, skip.astype(np.float64)) else math.inf
    else:
        rk = float((np.abs(gk - ref_k) / bound_skip(c, gk, skip)).max())
    return rh, rk


def hidden_mismatch_share(c: Case, got_h, ref_h):
    """share of the scaled hidden elements whose fp16 value is not the correctly rounded exact product"""
    half = c.C_h // 2
    g = np.asarray(got_h)[..., :half].astype(np.float16)
    return float((g != ref_h[..., :half].astype(np.float16)).mean())


# ---- fp32 model of the kernel, with planted faults ----------------------------------------------------------------------------------
FAULTS = ("swap_hw_twiddles", "phase_sign", "both_pm1", "drop_d", "padded_coords", "second_half", "half_slab64", "rows_mixed",
          "b_on_skip", "s_on_hidden")


def _twiddles(n, padded=False):
    t = 2.0 * np.pi * (np.arange(n) + (1 if padded else 0)) / n
    return np.cos(t).astype(F32), np.sin(t).astype(F32)         # double on the host, rounded to fp32: the kernel's table


def _sum(a, order):
    """sum over axes (1, 2) of an fp32 array [rows, H, W, C] in fp32: numpy's pairwise order, or strictly sequential"""
    if order == "pairwise":
        t = np.ascontiguousarray(a.reshape(a.shape[0], -1, a.shape[-1]).transpose(0, 2, 1))      # the summed axis last and contiguous
        return t.sum(axis=-1, dtype=F32)[:, None, None, :]
    acc = np.zeros((a.shape[0], a.shape[-1]), dtype=F32)
    for p in a.reshape(a.shape[0], -1, a.shape[-1]).transpose(1, 0, 2):
        acc = acc + p
    return acc[:, None, None, :]


def model32(c: Case, hidden, skip, order="pairwise", fault=None):
    """what a correct fp32 implementation stores (fp16 arrays), or a faulty one.  -> (hidden, skip)"""
    b, s = F32(c.b), F32(c.s)
    H, W = c.H, c.W
    h, k = hidden.copy(), skip.copy()
    if c.half != "skip":
        half = c.C_h // 2
        lo, hi = 0, half
        if fault == "second_half":
            lo, hi = half, c.C_h
        elif fault == "half_slab64":
            hi = min((half + 63) // 64 * 64, c.C_h)      # the boundary moved up to a 64-channel slab edge (halves 32 and 96 change)
        scale = s if fault == "s_on_hidden" else b
        h[..., lo:hi] = (hidden[..., lo:hi].astype(F32) * scale).astype(np.float16)
    if c.half != "hidden":
        v = skip.astype(F32)
        sw = fault == "swap_hw_twiddles"

        def tw(padded):
            cy, sy = _twiddles(W if sw else H, padded)
            cx, sx = _twiddles(H if sw else W, padded)
            cy, sy = np.resize(cy, H)[None, :, None, None], np.resize(sy, H)[None, :, None, None]
            cx, sx = np.resize(cx, W)[None, None, :, None], np.resize(sx, W)[None, None, :, None]
            return cy, sy, cx, sx, cy * cx - sy * sx, sy * cx + cy * sx
        # padded_coords: the reduce indexes the twiddles with the halo-padded coordinate (y + 1, x + 1), the apply with the interior
        # one (in BOTH places the shift would cancel)
        A = _sum(v, order)
        Bc, Bs, Cc, Cs, Dc, Ds = (_sum(v * w, order) for w in tw(fault == "padded_coords"))
        cy, sy, cx, sx, cd, sd = tw(False)
        if fault == "rows_mixed":
            A, Bc, Bs, Cc, Cs, Dc, Ds = (np.roll(t, 1, axis=0) if c.rows > 1 else np.roll(t, 1, axis=-1) for t in (A, Bc, Bs, Cc, Cs, Dc, Ds))
        sg = F32(-1.0) if fault == "phase_sign" else F32(1.0)
        low = A + (Bc * cy + sg * Bs * sy) + (Cc * cx + sg * Cs * sx)
        if fault != "drop_d":
            low = low + (Dc * cd + sg * Ds * sd)
        if fault == "both_pm1":         # frequencies +1 scaled as well: the conjugate terms (minus the doubly counted DC row / column)
            low = low + (Bc * cy + Bs * sy) + (Cc * cx + Cs * sx) + (Dc * cd + Ds * sd)
        kk = ((b if fault == "b_on_skip" else s) - F32(1.0)) / F32(H * W)
        k = (v + kk * low).astype(np.float16)
        if kk == 0:
            k = skip.copy()
    return h, k
