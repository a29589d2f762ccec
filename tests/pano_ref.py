"""The model the panorama tests compare against: the loop of diffusers' ``StableDiffusionPanoramaPipeline`` written with slices, in
torch on the CPU.  Per view, in view order, the step's expression sequence (``mock_engine.emulate_step_ddim``) runs on a copy of the
view's slice of the panorama; ``value[slice] += result; count[slice] += 1``; a view that wraps around the width is two pieces; at
the end ``z = value / count``.

``faults``: deliberate errors a test switches into the model to show that its assertions can fail (tests/test_pano_cpu.py)."""
from __future__ import annotations

import torch

from mock_engine import emulate_step_ddim

FAULTS = ("start_off_by_stride", "no_wrap", "div_max_count", "wrong_batch_row", "eps_next_view", "swap_halves", "no_wrapped_scatter")


def views(case, faults=()):
    """``(y0, x0)`` per view, diffusers' ``get_views`` in latent units (circular: the views also start in the last columns)"""
    Hp, Wp, h, w, stride, circ = case
    nbh = (Hp - h) // stride + 1 if Hp > h else 1
    nbw = (Wp // stride if circ else (Wp - w) // stride + 1) if Wp > w else 1
    out = [((i // nbw) * stride, (i % nbw) * stride) for i in range(nbh * nbw)]
    if "start_off_by_stride" in faults and len(out) > 1:
        y0, x0 = out[-1]
        out[-1] = (y0, x0 - stride) if x0 >= stride else (y0 - stride, x0)
    return out


def pieces(case, x0, faults=()):
    """the view's columns as (panorama columns, window columns) slices: one piece, or two when the view wraps"""
    _, Wp, _, w, _, _ = case
    if x0 + w <= Wp:
        return [(slice(x0, x0 + w), slice(0, w))]
    first = [(slice(x0, Wp), slice(0, Wp - x0))]
    return first if "no_wrap" in faults else first + [(slice(0, x0 + w - Wp), slice(Wp - x0, w))]


def coverage(case) -> torch.Tensor:
    """[Hp, Wp] int: how many views cover each latent pixel"""
    Hp, Wp, h, _, _, _ = case
    cnt = torch.zeros(Hp, Wp, dtype=torch.int64)
    for y0, x0 in views(case):
        for ps, _ in pieces(case, x0):
            cnt[y0:y0 + h, ps] += 1
    return cnt


def gather(case, z_pano, B, faults=(), out=None):
    """z_views [V * B, C, h, w], row v * B + b: the windows of ``z_pano`` [B, C, Hp, Wp]"""
    _, _, h, w, _, _ = case
    vs = views(case)
    if out is None:
        out = torch.empty((len(vs) * B, z_pano.shape[1], h, w), dtype=z_pano.dtype)
    for v, (y0, x0) in enumerate(vs):
        for i, (ps, ws) in enumerate(pieces(case, x0)):
            if i == 1 and "no_wrapped_scatter" in faults:
                continue
            out[v * B:(v + 1) * B, :, :, ws] = z_pano[:, :, y0:y0 + h, ps]
    return out


def step(case, z_pano, z_views, eps, B, Vc, lam, coeffs, tweedie_uc, renoise_uc, faults=()):
    """one MultiDiffusion step.  ``eps`` [V / Vc, 2 * Vc * B, C, h, w] fp16: chunk k holds the eps of views k * Vc .. (k + 1) * Vc - 1, the
    Vc * B unconditional rows (row vi * B + b) first, then the conditional rows.  -> the new (z_pano, z0t_pano); ``z_views`` is
    updated in place with the new latent's windows."""
    _, _, h, _, _, _ = case
    vs = views(case, faults)
    V = len(vs)
    value, value0, count = torch.zeros_like(z_pano), torch.zeros_like(z_pano), torch.zeros_like(z_pano)
    for v, (y0, x0) in enumerate(vs):
        ev = v + 1 if ("eps_next_view" in faults and v + 1 < V) else v
        k, vi = divmod(ev, Vc)
        for b in range(B):
            eb = (b + 1) % B if "wrong_batch_row" in faults else b
            e_uc, e_c = eps[k, vi * B + eb], eps[k, Vc * B + vi * B + eb]
            if "swap_halves" in faults:
                e_uc, e_c = e_c, e_uc
            for ps, ws in pieces(case, x0, faults):
                zc = z_pano[b, :, y0:y0 + h, ps].clone()          # the view's slice of the OLD panorama
                z0 = torch.empty_like(zc)
                emulate_step_ddim(zc, z0, e_uc[:, :, ws], e_c[:, :, ws], lam, coeffs, tweedie_uc, renoise_uc)
                value[b, :, y0:y0 + h, ps] += zc
                value0[b, :, y0:y0 + h, ps] += z0
                count[b, :, y0:y0 + h, ps] += 1
    if "div_max_count" in faults:
        count = torch.full_like(count, float(count.max()))
    z_new, z0t_new = value / count, value0 / count
    gather(case, z_new, B, faults, out=z_views)
    return z_new, z0t_new


def loop(case, unet_pair, z, ts, step_coeffs, B, lam, tweedie_uc, renoise_uc, faults=()):
    """the plain loop: per timestep, per view, ONE forward of that view's slices (``unet_pair(z_view [B, C, h, w], t) -> (eps_uc,
    eps_c)``), then :func:`step` with one view per chunk.  ``step_coeffs(t)`` -> (c1, c2, c3, c4).  -> (z0t, zt) of the panorama."""
    z = z.clone()
    z0t = torch.empty_like(z)
    z_views = gather(case, z, B)
    V = z_views.shape[0] // B
    for t in ts:
        eps = torch.stack([torch.cat(unet_pair(z_views[v * B:(v + 1) * B], t), 0) for v in range(V)], 0)
        z, z0t = step(case, z, z_views, eps, B, 1, lam, step_coeffs(t), tweedie_uc, renoise_uc, faults)
    return z0t, z
