"""The model the LCM tests compare against (include/cfgpp_lcm.h and cfgpp_amd/lcm.py restated in plain numpy / torch): Philox4x32-10,
the Box-Muller normals in float64 and in numpy-float32, the LCM timesteps and boundary scalings in float64, the guidance-scale
embedding, and the step's expression sequence.  No product code is imported here.

``faults``: a set of names; each switches ONE deliberate error into the model so that tests/test_lcm_cpu.py can require the
assertion that guards that property to fail (the house style of fault injection)."""
from __future__ import annotations

import math

import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(ctr, key):
    """one block, python integers"""
    c0, c1, c2, c3 = (int(v) & MASK for v in ctr)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_words(n_groups, seed, draw, stream_id, c0_start=0, c1=0):
    """[n_groups, 4] uint32: the blocks of counters (c0_start + q, c1, draw, stream_id) under the key of ``seed``, vectorised"""
    u = np.uint64
    c = [(np.arange(n_groups, dtype=np.uint64) + u(c0_start)) & u(MASK), np.full(n_groups, c1, np.uint64),
         np.full(n_groups, draw, np.uint64), np.full(n_groups, stream_id, np.uint64)]
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        p0, p1 = u(M0) * c[0], u(M1) * c[2]
        c = [((p1 >> u(32)) ^ c[1] ^ u(k0)) & u(MASK), p1 & u(MASK), ((p0 >> u(32)) ^ c[3] ^ u(k1)) & u(MASK), p0 & u(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, 1).astype(np.uint32)


def uniforms(words):
    """(u1 in (0, 1], u2 in [0, 1)) float64 [n, 2] each, from words [n, 4]: columns (r0, r2) and (r1, r3)"""
    w = words.astype(np.uint64)
    u1 = ((w[:, 0::2] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (w[:, 1::2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normals(row_elems, seed, draw, stream_id, dtype=np.float64, faults=()):
    """the row of ``row_elems`` normals of one chain.  float64: the model; float32: the numpy-float32 restatement whose error against
    the model sizes the GPU test's bound."""
    assert row_elems % 4 == 0
    n = row_elems // 4
    if "stream_ignored" in faults:
        stream_id = 0
    words = philox_words(n, seed, draw, stream_id)
    u1, u2 = uniforms(words)
    u1, u2 = u1.astype(dtype), u2.astype(dtype)
    rho = np.sqrt(dtype(-2.0) * np.log(u1))
    ang = dtype(2.0) * u2                  # exact in fp32; sin / cos of pi * ang, as sincospif takes it
    if dtype == np.float64:
        c, s = np.cos(np.pi * ang), np.sin(np.pi * ang)
    else:                                  # fp32 restatement: the argument reduced exactly first, as sincospi does
        r = ang - np.floor(ang)            # [0, 1)
        sgn = np.where(ang >= 1.0, dtype(-1.0), dtype(1.0))
        pr = (dtype(np.pi) * r).astype(dtype)
        c, s = sgn * np.cos(pr, dtype=dtype), sgn * np.sin(pr, dtype=dtype)
    if "sincos_swapped" in faults:
        c, s = s, c
    out = np.empty((n, 4), dtype)
    out[:, 0::2] = rho * c
    out[:, 1::2] = rho * s
    if "last_group_skipped" in faults:
        out[-1] = 0
    return out.reshape(-1)


def normal_rows(B, row_elems, seeds, draw, stream_id, dtype=np.float64, faults=()):
    rows = []
    for b in range(B):
        seed = seeds[0] if "row0_seed" in faults else seeds[b]
        rows.append(normals(row_elems, seed, draw, stream_id, dtype, faults))
    return np.stack(rows)


# ---- schedule -------------------------------------------------------------------------------------------------------------------
def lcm_timesteps(n, original_steps=50, train=1000):
    origin = (np.arange(1, original_steps + 1) * (train // original_steps) - 1)[::-1]
    idx = np.floor(np.linspace(0, original_steps, n, endpoint=False)).astype(np.int64)
    return origin[idx].tolist()


def boundary_scalings(t, timestep_scaling=10.0, sigma_data=0.5, faults=()):
    """(c_skip, c_out) in float64"""
    s = timestep_scaling * float(t)
    c_skip = sigma_data ** 2 / (s ** 2 + sigma_data ** 2)
    c_out = s / math.sqrt(s ** 2 + sigma_data ** 2)
    return (c_out, c_skip) if "skip_out_swapped" in faults else (c_skip, c_out)


def guidance_embedding(guidance_scale, dim):
    """diffusers get_guidance_scale_embedding in float64: w = (scale - 1) * 1000, [sin(w f), cos(w f)]"""
    w = (float(guidance_scale) - 1.0) * 1000.0
    half = dim // 2
    f = np.exp(-np.arange(half, dtype=np.float64) * math.log(10000.0) / (half - 1))
    return np.concatenate([np.sin(w * f), np.cos(w * f)])


# ---- the step, in the header's expression sequence --------------------------------------------------------------------------------
def cfg_mix(m_uc, m_c, lam):
    """h(m_uc + h(lam * h(m_c - m_uc))) on fp16 tensors, each operation computed in fp32 and rounded to fp16"""
    f, h = torch.float32, torch.float16
    d = (m_c.to(f) - m_uc.to(f)).to(h)
    e = (d.to(f) * torch.tensor(float(lam), dtype=f, device=d.device)).to(h)
    return (m_uc.to(f) + e.to(f)).to(h)


def step_lcm(z, m_uc, m_c, lam, coef, pred_v, last, noise, faults=()):
    """-> (den, z_next), fp32 tensors on z's device; every operation is one fp32 torch op (one rounding), products with the fp16 model
    output rounded to fp16 after their fp32 rounding"""
    f, h = torch.float32, torch.float16
    k0, k1, c_out, c_skip, c3, c4 = (torch.tensor(float(v), dtype=f, device=z.device) for v in coef[:6])
    hat = cfg_mix(m_uc, m_c, lam).to(f)
    if pred_v:
        x0 = k1 * z - (k0 * hat).to(h).to(f)
    else:
        num = z - (hat * k0).to(h).to(f)
        x0 = num * (-k1) if float(k1) < 0 else num / k1
    den = c_out * x0 + c_skip * z
    if last:      # (the fault: the renoise runs on the last step too, at full noise weight)
        return den, (den + noise.to(f) if "noise_on_last" in faults else den.clone())
    return den, c3 * den + c4 * noise.to(f)


def pinned_sqrt_tables(path):
    """(sqrt(abar), sqrt(1 - abar)) fp32 [1000] from the package's pinned data file (data, not code): entry k + 1 of the shifted
    tables is abar[k]"""
    d = np.load(path)
    return d["sqrt_a"].astype(np.float32)[1:], d["sqrt_1ma"].astype(np.float32)[1:]


def chain_coeffs(sqrt_a, sqrt_1ma, t, t_prev, pred_v, semantics, scaling=10.0, faults=()):
    """coef6 of one step, restating the scalar rules: a scalar that multiplies the fp16 model output is pre-rounded to fp16 under
    "cpu" semantics and stays fp32 under "cuda"; the divisor sqrt(a_t) is an IEEE division under "cpu" and the multiplication by
    the fp32 reciprocal (passed negated) under "cuda"; everything that multiplies fp32 values stays fp32"""
    f32 = np.float32
    h = (lambda v: float(f32(np.float16(v)))) if semantics == "cpu" else float
    c_skip, c_out = boundary_scalings(t, scaling, faults=faults)
    c3, c4 = (1.0, 0.0) if t_prev is None else (float(sqrt_a[t_prev]), float(sqrt_1ma[t_prev]))
    k0 = h(sqrt_1ma[t])
    if pred_v:
        k1 = float(sqrt_a[t])
    else:
        k1 = float(sqrt_a[t]) if semantics == "cpu" else -float(f32(1.0) / f32(sqrt_a[t]))
    return (k0, k1, float(f32(c_out)), float(f32(c_skip)), c3, c4)


def lcm_chain(model_fn, z, seeds, ts, sqrt_a, sqrt_1ma, lam, pred_v=False, semantics="cuda", scaling=10.0, faults=()):
    """the whole LCM loop on the model's noise: ``model_fn(z, t) -> (m_uc, m_c)`` fp16.  -> (den, z, per-step record list)"""
    B, row = int(z.shape[0]), int(z[0].numel())
    rec = []
    den = None
    z = z.clone()
    for i, t in enumerate(ts):
        last = i == len(ts) - 1
        coef = chain_coeffs(sqrt_a, sqrt_1ma, t, None if last else ts[i + 1], pred_v, semantics, scaling, faults)
        draw = 0 if "draw_stuck" in faults else i
        noise = torch.from_numpy(normal_rows(B, row, seeds, draw, 0, np.float64, faults).astype(np.float32)).reshape(z.shape).to(z.device)
        m_uc, m_c = model_fn(z, t)
        den, z = step_lcm(z, m_uc, m_c, lam, coef, pred_v, last, noise, faults)
        rec.append(dict(t=t, draw=draw, last=last, coef=coef))
    return den, z, rec
