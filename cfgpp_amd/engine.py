"""Python face of the HIP engine: PyTorch-ROCm tensors in, raw HIP kernels
underneath (ctypes -> libcfgpp_hip.so).  Torch is plumbing only (device
memory, streams); no torch op computes anything on the hot path.

``HipUNet``      replaces ``pipe.unet`` of the reference
                 (latent_diffusion.py:63-67,146-156; latent_sdxl.py:40,50,170-183).
``step_ddim`` /  replace the per-step sampler arithmetic
``step_kdiff``   (latent_diffusion.py:660-666 etc.).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional, Tuple

import torch

from . import _lib
from ._lib import CfgppError, UNetConfigC, check
from .unet_config import UNetConfig


def _require_cuda(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise CfgppError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if not t.is_contiguous():
        raise CfgppError(f"{name} must be contiguous")


def _stream_ptr(t: Optional[torch.Tensor] = None) -> int:
    """the current torch stream of the device the tensor lives on (not of whatever device is current)"""
    if t is not None and t.is_cuda:
        return torch.cuda.current_stream(t.device).cuda_stream
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ----------------------------------------------------------------------------
# sampler step kernels
# ----------------------------------------------------------------------------
def step_ddim(z: torch.Tensor, z0t_out: torch.Tensor, eps_uc: torch.Tensor, eps_c: torch.Tensor,
              lam: float, coeffs: Tuple[float, float, float, float], tweedie_uc: bool, renoise_uc: bool):
    """In-place generalised DDIM update (see include/cfgpp.h: cfgpp_step_ddim)."""
    lib = _lib.load()
    for n, t in (("z", z), ("z0t_out", z0t_out), ("eps_uc", eps_uc), ("eps_c", eps_c)):
        _require_cuda(t, n)
    if z.dtype != z0t_out.dtype or z.dtype not in (torch.float16, torch.float32):
        raise CfgppError("step_ddim: z and z0t_out must both be fp32 or both fp16")
    if eps_uc.dtype != eps_c.dtype or eps_uc.dtype not in (torch.float16, torch.float32):
        raise CfgppError("step_ddim: eps must both be fp16 or both fp32")
    if not (z.numel() == z0t_out.numel() == eps_uc.numel() == eps_c.numel()):
        raise CfgppError("step_ddim: size mismatch")
    c1, c2, c3, c4 = (float(x) for x in coeffs)
    if z.dtype == torch.float16:          # fp16 latent (inversion / edit paths): every op rounds to fp16
        if eps_uc.dtype != torch.float16:
            raise CfgppError("step_ddim: an fp16 latent needs fp16 eps")
        check(lib.cfgpp_step_ddim_h(z.data_ptr(), z0t_out.data_ptr(), eps_uc.data_ptr(), eps_c.data_ptr(), float(lam),
                                    c1, c2, c3, c4, int(bool(tweedie_uc)), int(bool(renoise_uc)), z.numel(), _stream_ptr(z)),
              "cfgpp_step_ddim_h")
        return
    check(lib.cfgpp_step_ddim(z.data_ptr(), z0t_out.data_ptr(), eps_uc.data_ptr(), eps_c.data_ptr(),
                              1 if eps_uc.dtype == torch.float16 else 0, float(lam), c1, c2, c3, c4,
                              int(bool(tweedie_uc)), int(bool(renoise_uc)), z.numel(), _stream_ptr(z)),
          "cfgpp_step_ddim")


def step_ddim_masked(z: torch.Tensor, z0t_out: torch.Tensor, eps_uc: torch.Tensor, eps_c: torch.Tensor, lam: float,
                     coeffs: Tuple[float, float, float, float], tweedie_uc: bool, renoise_uc: bool, mask: torch.Tensor,
                     src: torch.Tensor, noise: torch.Tensor, a: float, b: float):
    """:func:`step_ddim` on an fp32 latent with fp16 eps, blended in the same pass with the forward-noised source
    (include/cfgpp.h: cfgpp_step_ddim_masked): ``z = where(mask, z_new, a*src + b*noise)``, ``z0t_out = where(mask, z0t, src)``.
    z / z0t_out / noise fp32 [B,4,h,w], eps / src fp16 [B,4,h,w], mask bool or uint8 [B,1,h,w] (or [B,h,w]), nonzero = repaint."""
    lib = _lib.load()
    for n, t in (("z", z), ("z0t_out", z0t_out), ("eps_uc", eps_uc), ("eps_c", eps_c), ("mask", mask), ("src", src),
                 ("noise", noise)):
        _require_cuda(t, n)
    if z.dtype != torch.float32 or z0t_out.dtype != torch.float32 or noise.dtype != torch.float32:
        raise CfgppError("step_ddim_masked: z, z0t_out and noise must be fp32")
    if eps_uc.dtype != torch.float16 or eps_c.dtype != torch.float16 or src.dtype != torch.float16:
        raise CfgppError("step_ddim_masked: eps and src must be fp16")
    if mask.dtype not in (torch.bool, torch.uint8):
        raise CfgppError("step_ddim_masked: mask must be bool or uint8 (binarized)")
    if z.dim() != 4 or tuple(z.shape[1:2]) != (4,):
        raise CfgppError(f"step_ddim_masked: z shape {tuple(z.shape)} is not [B, 4, h, w]")
    B, hw = int(z.shape[0]), int(z.shape[2]) * int(z.shape[3])
    for n, t in (("z0t_out", z0t_out), ("eps_uc", eps_uc), ("eps_c", eps_c), ("src", src), ("noise", noise)):
        if tuple(t.shape) != tuple(z.shape):
            raise CfgppError(f"step_ddim_masked: {n} shape {tuple(t.shape)} != z shape {tuple(z.shape)}")
    if mask.numel() != B * hw:
        raise CfgppError(f"step_ddim_masked: mask has {mask.numel()} elements for B={B} x hw={hw}")
    c1, c2, c3, c4 = (float(x) for x in coeffs)
    check(lib.cfgpp_step_ddim_masked(z.data_ptr(), z0t_out.data_ptr(), eps_uc.data_ptr(), eps_c.data_ptr(), float(lam), c1, c2, c3, c4,
                                     int(bool(tweedie_uc)), int(bool(renoise_uc)), mask.data_ptr(), src.data_ptr(), noise.data_ptr(),
                                     float(a), float(b), B, hw, _stream_ptr(z)), "cfgpp_step_ddim_masked")


def kdiff_input(x: torch.Tensor, xc_out: torch.Tensor, s: float, mode: int):
    lib = _lib.load()
    _require_cuda(x, "x")
    _require_cuda(xc_out, "xc_out")
    if x.dtype != torch.float16 or xc_out.dtype != torch.float16:
        raise CfgppError("kdiff_input: fp16 latents expected")
    check(lib.cfgpp_kdiff_input(x.data_ptr(), xc_out.data_ptr(), float(s), int(mode), x.numel(), _stream_ptr(x)),
          "cfgpp_kdiff_input")


def step_kdiff(x: torch.Tensor, den_out: torch.Tensor, old: Optional[torch.Tensor], eps_uc: torch.Tensor,
               eps_c: torch.Tensor, coef9, variant: int, xl_form: bool, euler_branch: bool, write_old: bool):
    lib = _lib.load()
    for n, t in (("x", x), ("den_out", den_out), ("eps_uc", eps_uc), ("eps_c", eps_c)):
        _require_cuda(t, n)
        if t.dtype != torch.float16:
            raise CfgppError(f"step_kdiff: {n} must be fp16")
    if old is not None:
        _require_cuda(old, "old")
    arr = (C.c_float * 9)(*[float(v) for v in coef9])
    check(lib.cfgpp_step_kdiff(x.data_ptr(), den_out.data_ptr(), _ptr(old), eps_uc.data_ptr(), eps_c.data_ptr(),
                               arr, int(variant), int(bool(xl_form)), int(bool(euler_branch)), int(bool(write_old)),
                               x.numel(), _stream_ptr(x)), "cfgpp_step_kdiff")


def kdiff_denoise(x, eps_uc, eps_c, lam: float, sigma: float, den_out, uden_out):
    lib = _lib.load()
    for n, t in (("x", x), ("eps_uc", eps_uc), ("eps_c", eps_c), ("den_out", den_out), ("uden_out", uden_out)):
        _require_cuda(t, n)
        if t.dtype != torch.float16:
            raise CfgppError(f"kdiff_denoise: {n} must be fp16")
    check(lib.cfgpp_kdiff_denoise(x.data_ptr(), eps_uc.data_ptr(), eps_c.data_ptr(), float(lam), float(sigma),
                                  den_out.data_ptr(), uden_out.data_ptr(), x.numel(), _stream_ptr(x)), "cfgpp_kdiff_denoise")


def lincomb(out, x, y, z, a: float, b: float, mode: int):
    lib = _lib.load()
    for n, t in (("out", out), ("x", x), ("y", y)) + ((("z", z),) if z is not None else ()):
        _require_cuda(t, n)
        if t.dtype != torch.float16:
            raise CfgppError(f"lincomb: {n} must be fp16")
    check(lib.cfgpp_lincomb(out.data_ptr(), x.data_ptr(), y.data_ptr(), _ptr(z), float(a), float(b), int(mode), x.numel(),
                            _stream_ptr(x)), "cfgpp_lincomb")


# ----------------------------------------------------------------------------
# v-prediction (include/cfgpp_vpred.h)
# ----------------------------------------------------------------------------
def step_ddim_v(z: torch.Tensor, z0t_out: torch.Tensor, v_uc: torch.Tensor, v_c: torch.Tensor, lam: float, coef6,
                tweedie_uc: bool, renoise_uc: bool, row_scale: Optional[torch.Tensor] = None):
    """In-place generalised DDIM update of a v-prediction model (cfgpp_step_ddim_v): ``coef6`` = (a_z, s_v, a_v, s_z, c3, c4) from
    ``coeffs.ddim_v_coeffs_pinned``; z / z0t_out both fp32 or both fp16, v fp16.  ``row_scale``: fp32 [B] from :func:`cfg_rescale`
    (z is then [B, ...]), or None."""
    lib = _lib.load()
    for n, t in (("z", z), ("z0t_out", z0t_out), ("v_uc", v_uc), ("v_c", v_c)):
        _require_cuda(t, n)
    if z.dtype != z0t_out.dtype or z.dtype not in (torch.float16, torch.float32):
        raise CfgppError("step_ddim_v: z and z0t_out must both be fp32 or both fp16")
    if v_uc.dtype != torch.float16 or v_c.dtype != torch.float16:
        raise CfgppError("step_ddim_v: v must be fp16")
    if not (z.numel() == z0t_out.numel() == v_uc.numel() == v_c.numel()):
        raise CfgppError("step_ddim_v: size mismatch")
    if len(coef6) != 6:
        raise CfgppError("step_ddim_v: coef6 = (a_z, s_v, a_v, s_z, c3, c4)")
    row_elems = 0
    if row_scale is not None:
        _require_cuda(row_scale, "row_scale")
        if row_scale.dtype != torch.float32 or row_scale.numel() != int(z.shape[0]):
            raise CfgppError(f"step_ddim_v: row_scale must be fp32 [{int(z.shape[0])}]")
        row_elems = z.numel() // int(z.shape[0])
    arr = (C.c_float * 6)(*[float(v) for v in coef6])
    check(lib.cfgpp_step_ddim_v(z.data_ptr(), z0t_out.data_ptr(), v_uc.data_ptr(), v_c.data_ptr(), 1 if z.dtype == torch.float16 else 0,
                                float(lam), arr, int(bool(tweedie_uc)), int(bool(renoise_uc)), _ptr(row_scale), row_elems, z.numel(),
                                _stream_ptr(z)), "cfgpp_step_ddim_v")


def v_to_eps(eps_uc_out: torch.Tensor, eps_c_out: torch.Tensor, v_uc: torch.Tensor, v_c: torch.Tensor, x: torch.Tensor, a: float, s: float):
    """eps = a*v + s*x for both CFG halves in one launch (cfgpp_v_to_eps), all fp16; the outputs may be the inputs."""
    lib = _lib.load()
    for n, t in (("eps_uc_out", eps_uc_out), ("eps_c_out", eps_c_out), ("v_uc", v_uc), ("v_c", v_c), ("x", x)):
        _require_cuda(t, n)
        if t.dtype != torch.float16:
            raise CfgppError(f"v_to_eps: {n} must be fp16")
        if t.numel() != x.numel():
            raise CfgppError("v_to_eps: size mismatch")
    check(lib.cfgpp_v_to_eps(eps_uc_out.data_ptr(), eps_c_out.data_ptr(), v_uc.data_ptr(), v_c.data_ptr(), x.data_ptr(), 1, float(a),
                             float(s), x.numel(), _stream_ptr(x)), "cfgpp_v_to_eps")


def cfg_rescale(v_uc: torch.Tensor, v_c: torch.Tensor, lam: float, phi: float, row_scale_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [B]: the per-sample factor of diffusers' ``rescale_noise_cfg`` (cfgpp_cfg_rescale); v_uc / v_c fp16 [B, ...]."""
    lib = _lib.load()
    for n, t in (("v_uc", v_uc), ("v_c", v_c)):
        _require_cuda(t, n)
        if t.dtype != torch.float16:
            raise CfgppError(f"cfg_rescale: {n} must be fp16")
    if v_uc.shape != v_c.shape or v_uc.dim() < 2:
        raise CfgppError("cfg_rescale: v_uc / v_c must be [B, ...] of one shape")
    B = int(v_uc.shape[0])
    if row_scale_out is None:
        row_scale_out = torch.empty((B,), dtype=torch.float32, device=v_uc.device)
    _require_cuda(row_scale_out, "row_scale_out")
    if row_scale_out.dtype != torch.float32 or row_scale_out.numel() != B:
        raise CfgppError(f"cfg_rescale: row_scale_out must be fp32 [{B}]")
    check(lib.cfgpp_cfg_rescale(v_uc.data_ptr(), v_c.data_ptr(), float(lam), float(phi), row_scale_out.data_ptr(), B, v_uc.numel() // B,
                                _stream_ptr(v_uc)), "cfgpp_cfg_rescale")
    return row_scale_out


# ----------------------------------------------------------------------------
# LCM (include/cfgpp_lcm.h)
# ----------------------------------------------------------------------------
def _seed_array(seeds, B: int, who: str):
    if len(seeds) != B:
        raise CfgppError(f"{who}: {len(seeds)} seeds for {B} chains")
    return (C.c_ulonglong * B)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds])


def philox_normal(out: torch.Tensor, seeds, draw: int, stream_id: int) -> torch.Tensor:
    """fill ``out`` [B, ...] (fp32 or fp16) with the seeded normals of cfgpp_philox_normal: chain b's row from ``seeds[b]``, draw index
    ``draw``, ``stream_id`` 0 (LCM renoise) / 1 (ancestral noise)"""
    lib = _lib.load()
    _require_cuda(out, "out")
    if out.dtype not in (torch.float16, torch.float32) or out.dim() < 2:
        raise CfgppError("philox_normal: out must be fp32 or fp16 [B, ...]")
    B = int(out.shape[0])
    check(lib.cfgpp_philox_normal(out.data_ptr(), 1 if out.dtype == torch.float16 else 0, _seed_array(seeds, B, "philox_normal"), B,
                                  out.numel() // B, int(draw), int(stream_id), _stream_ptr(out)), "cfgpp_philox_normal")
    return out


def step_lcm(z: torch.Tensor, den_out: torch.Tensor, m_uc: torch.Tensor, m_c: torch.Tensor, lam: float, coef6, pred_v: bool, last: bool,
             seeds=None, draw: int = 0, noise: Optional[torch.Tensor] = None):
    """one fused LCM step in place on the fp32 latent ``z`` [B, ...] (cfgpp_step_lcm); ``coef6`` from ``lcm.step_coeffs``; the
    renoising noise is ``noise`` (fp32, z's shape) or, with None, drawn in the kernel from ``seeds`` / ``draw``"""
    lib = _lib.load()
    for n, t in (("z", z), ("den_out", den_out), ("m_uc", m_uc), ("m_c", m_c)) + ((("noise", noise),) if noise is not None else ()):
        _require_cuda(t, n)
        if t.numel() != z.numel():
            raise CfgppError("step_lcm: size mismatch")
    if z.dtype != torch.float32 or den_out.dtype != torch.float32 or (noise is not None and noise.dtype != torch.float32):
        raise CfgppError("step_lcm: z, den_out and noise must be fp32")
    if m_uc.dtype != torch.float16 or m_c.dtype != torch.float16:
        raise CfgppError("step_lcm: the model output must be fp16")
    if len(coef6) != 6:
        raise CfgppError("step_lcm: coef6 = (c1 | s_v, c2 | a_z, c_out, c_skip, c3, c4)")
    B = int(z.shape[0])
    sd = None
    if not last and noise is None:
        if seeds is None:
            raise CfgppError("step_lcm: a step that is not the last needs seeds or noise")
        sd = _seed_array(seeds, B, "step_lcm")
    arr = (C.c_float * 8)(*[float(v) for v in coef6], 0.0, 0.0)
    check(lib.cfgpp_step_lcm(z.data_ptr(), den_out.data_ptr(), m_uc.data_ptr(), m_c.data_ptr(), float(lam), arr, int(bool(pred_v)),
                             int(bool(last)), _ptr(noise), sd, B, z.numel() // B, int(draw), _stream_ptr(z)), "cfgpp_step_lcm")


def philox_raw(ctr4, key2, n: int, device=None) -> torch.Tensor:
    """test hook (cfgpp_debug.h: cfgpp_op_philox_raw): [n, 4] int32 holding the uint32 words of counters (ctr4[0] + i, ctr4[1..3])"""
    lib = _lib.load()
    out = torch.empty((int(n), 4), dtype=torch.int32, device=device or "cuda")
    check(lib.cfgpp_op_philox_raw(out.data_ptr(), (C.c_uint * 4)(*[int(v) & 0xFFFFFFFF for v in ctr4]),
                                  (C.c_uint * 2)(*[int(v) & 0xFFFFFFFF for v in key2]), int(n), _stream_ptr(out)), "cfgpp_op_philox_raw")
    return out


# ----------------------------------------------------------------------------
# DPM++ 2M / 3M SDE (include/cfgpp_sde.h)
# ----------------------------------------------------------------------------
def sde_input(x: torch.Tensor, xc_out: torch.Tensor, s_in: float):
    """``xc_out = h(x * s_in)``: the fp16 UNet input of step 0 of an SDE job from the fp32 latent (cfgpp_sde_input)"""
    lib = _lib.load()
    _require_cuda(x, "x")
    _require_cuda(xc_out, "xc_out")
    if x.dtype != torch.float32 or xc_out.dtype != torch.float16:
        raise CfgppError("sde_input: x must be fp32 and xc_out fp16")
    if x.numel() != xc_out.numel():
        raise CfgppError("sde_input: size mismatch")
    check(lib.cfgpp_sde_input(x.data_ptr(), xc_out.data_ptr(), float(s_in), x.numel(), _stream_ptr(x)), "cfgpp_sde_input")


def step_sde(x: torch.Tensor, den_out: torch.Tensor, xc_out: Optional[torch.Tensor], hist1: Optional[torch.Tensor],
             hist2: Optional[torch.Tensor], hist_out: Optional[torch.Tensor], m_uc: torch.Tensor, m_c: torch.Tensor, lam: float, coef8,
             cfgpp: bool, n_hist: int, last: bool, seeds=None, draw: int = 0, noise: Optional[torch.Tensor] = None):
    """one fused DPM++ 2M / 3M SDE step in place on the fp32 latent ``x`` [B, ...] (cfgpp_step_sde); ``coef8`` from ``sde.sde_coeffs``;
    the step noise is ``noise`` (fp32, x's shape) or, with None, drawn in the kernel from ``seeds`` / ``draw``.  ``hist_out`` may be
    ``hist2``; ``xc_out`` / ``hist_out`` may be None."""
    lib = _lib.load()
    f32 = (("x", x), ("den_out", den_out)) + tuple((n, t) for n, t in (("hist1", hist1), ("hist2", hist2), ("hist_out", hist_out),
                                                                        ("noise", noise)) if t is not None)
    f16 = (("m_uc", m_uc), ("m_c", m_c)) + ((("xc_out", xc_out),) if xc_out is not None else ())
    for n, t in f32 + f16:
        _require_cuda(t, n)
        if t.numel() != x.numel():
            raise CfgppError(f"step_sde: size mismatch ({n})")
    if any(t.dtype != torch.float32 for _, t in f32):
        raise CfgppError("step_sde: x, den_out, the history and noise must be fp32")
    if any(t.dtype != torch.float16 for _, t in f16):
        raise CfgppError("step_sde: the model output and xc_out must be fp16")
    if len(coef8) != 8:
        raise CfgppError("step_sde: coef8 = (sigma, a_x, a_d, a_u, a_1, a_2, a_n, s_in_next)")
    if x.dim() < 2:
        raise CfgppError("step_sde: x must be [B, ...]")
    B = int(x.shape[0])
    sd = None
    if not last and float(coef8[6]) != 0.0 and noise is None:
        if seeds is None:
            raise CfgppError("step_sde: a step with a noise term needs seeds or noise")
        sd = _seed_array(seeds, B, "step_sde")
    arr = (C.c_float * 8)(*[float(v) for v in coef8])
    check(lib.cfgpp_step_sde(x.data_ptr(), den_out.data_ptr(), _ptr(xc_out), _ptr(hist1), _ptr(hist2), _ptr(hist_out), m_uc.data_ptr(),
                             m_c.data_ptr(), float(lam), arr, int(bool(cfgpp)), int(n_hist), int(bool(last)), _ptr(noise), sd, B,
                             x.numel() // B, int(draw), _stream_ptr(x)), "cfgpp_step_sde")


# ----------------------------------------------------------------------------
# DPM++ SDE (include/cfgpp_dpmpp_sde.h)
# ----------------------------------------------------------------------------
STAGE_D, STAGE_U, STAGE_N1, STAGE_N2 = 1, 2, 4, 8       # the bits of ``terms`` (CFGPP_STAGE_*)


def step_sde_stage(x: torch.Tensor, base: torch.Tensor, out: torch.Tensor, den_out: torch.Tensor, xc_out: Optional[torch.Tensor],
                   m_uc: torch.Tensor, m_c: torch.Tensor, lam: float, coef7, terms: int, last: bool, seeds=None, draw1: int = 0,
                   draw2: int = 1, noise1: Optional[torch.Tensor] = None, noise2: Optional[torch.Tensor] = None):
    """one stage of a DPM++ SDE step on the fp32 latents ``x`` / ``base`` [B, ...] -> ``out`` (cfgpp_step_sde_stage); ``coef7`` and
    ``terms`` from ``dpmpp_sde.dpmpp_sde_coeffs``; each noise term that is on is ``noise1`` / ``noise2`` (fp32, x's shape) or, with
    None, drawn in the kernel from ``seeds`` and ``draw1`` / ``draw2``.  ``base`` may be ``x``, ``out`` may be ``x``; ``xc_out`` may
    be None."""
    lib = _lib.load()
    f32 = (("x", x), ("base", base), ("out", out), ("den_out", den_out)) + tuple((n, t) for n, t in (("noise1", noise1), ("noise2", noise2))
                                                                                 if t is not None)
    f16 = (("m_uc", m_uc), ("m_c", m_c)) + ((("xc_out", xc_out),) if xc_out is not None else ())
    for n, t in f32 + f16:
        _require_cuda(t, n)
        if t.numel() != x.numel():
            raise CfgppError(f"step_sde_stage: size mismatch ({n})")
    if any(t.dtype != torch.float32 for _, t in f32):
        raise CfgppError("step_sde_stage: x, base, out, den_out and the noise must be fp32")
    if any(t.dtype != torch.float16 for _, t in f16):
        raise CfgppError("step_sde_stage: the model output and xc_out must be fp16")
    if len(coef7) != 7:
        raise CfgppError("step_sde_stage: coef7 = (sigma_b, a_x, a_d, a_u, c_1, c_2, s_in)")
    if x.dim() < 2:
        raise CfgppError("step_sde_stage: x must be [B, ...]")
    B = int(x.shape[0])
    terms = int(terms)
    sd = None
    if not last and ((terms & STAGE_N1 and noise1 is None) or (terms & STAGE_N2 and noise2 is None)):
        if seeds is None:
            raise CfgppError("step_sde_stage: a noise term needs seeds or its noise tensor")
        sd = _seed_array(seeds, B, "step_sde_stage")
    arr = (C.c_float * 7)(*[float(v) for v in coef7])
    check(lib.cfgpp_step_sde_stage(x.data_ptr(), base.data_ptr(), out.data_ptr(), den_out.data_ptr(), _ptr(xc_out), m_uc.data_ptr(),
                                   m_c.data_ptr(), float(lam), arr, terms, int(bool(last)), _ptr(noise1), _ptr(noise2), sd, B,
                                   x.numel() // B, int(draw1), int(draw2), _stream_ptr(x)), "cfgpp_step_sde_stage")


# ----------------------------------------------------------------------------
# img2img / latent hires fix (include/cfgpp_img2img.h)
# ----------------------------------------------------------------------------
RESAMPLE_MODES = {"identity": 0, "nearest-exact": 1, "bilinear": 2, "bicubic": 3}
START_NOISE_STREAM = 4      # stream id of the start's forward noise (draw 0); 0 .. 3: LCM renoise, ancestral, 2M / 3M SDE, DPM++ SDE


def img2img_start(x: torch.Tensor, src: Optional[torch.Tensor], a: float, s: float, mode="identity", noise: Optional[torch.Tensor] = None,
                  seeds=None):
    """``x = a * resample(src) + s * n`` in one launch (cfgpp_img2img_start): ``x`` [B, C, h, w] fp32 or fp16 is written; ``src``
    [1 or B, C, h0, w0] fp32 or fp16 (not read, and may be None, when ``a == 0``); ``mode``: a key of ``RESAMPLE_MODES`` or its number;
    the normals are ``noise`` (fp32, x's shape) or, with None, drawn in the kernel from ``seeds`` (one per chain); ``s == 0`` needs
    neither."""
    lib = _lib.load()
    _require_cuda(x, "x")
    if x.dim() != 4 or x.dtype not in (torch.float16, torch.float32):
        raise CfgppError("img2img_start: x must be fp32 or fp16 [B, C, h, w]")
    B, C_, h, w = (int(v) for v in x.shape)
    a, s = float(a), float(s)
    mode = RESAMPLE_MODES[mode] if isinstance(mode, str) else int(mode)
    rows, h0, w0, src_half = 1, h, w, 0
    if a != 0.0:
        if src is None:
            raise CfgppError("img2img_start: a != 0 needs src")
        _require_cuda(src, "src")
        if src.dim() != 4 or src.dtype not in (torch.float16, torch.float32) or int(src.shape[1]) != C_ or int(src.shape[0]) not in (1, B):
            raise CfgppError(f"img2img_start: src must be fp32 or fp16 [1 or {B}, {C_}, h0, w0], got {src.dtype} {list(src.shape)}")
        rows, h0, w0, src_half = int(src.shape[0]), int(src.shape[2]), int(src.shape[3]), int(src.dtype == torch.float16)
    else:                       # the source plays no part: the identity geometry of x
        src, mode = None, 0
    sd = None
    if s != 0.0:
        if noise is not None:
            _require_cuda(noise, "noise")
            if noise.dtype != torch.float32 or tuple(noise.shape) != tuple(x.shape):
                raise CfgppError("img2img_start: noise must be fp32 of x's shape")
        elif seeds is None:
            raise CfgppError("img2img_start: s != 0 needs noise or seeds")
        else:
            sd = _seed_array(seeds, B, "img2img_start")
    else:
        noise = None
    check(lib.cfgpp_img2img_start(x.data_ptr(), _ptr(src), _ptr(noise), sd, a, s, B, rows, C_, h0, w0, h, w, mode,
                                  int(x.dtype == torch.float16), src_half, _stream_ptr(x)), "cfgpp_img2img_start")
    return x


# ----------------------------------------------------------------------------
# MultiDiffusion panoramas (include/cfgpp_panorama.h)
# ----------------------------------------------------------------------------
def _pano_views_c(g, B: int, C_: int, name: str, z_pano: torch.Tensor, z_views: torch.Tensor):
    """the C struct of ``g`` (``panorama.ViewGeometry``: Hp, Wp, h, w, stride, circular, n_views, chunk_views) for B chains, after
    checking the two latent buffers against it"""
    for n, t in (("z_pano", z_pano), ("z_views", z_views)):
        _require_cuda(t, n)
        if t.dtype != torch.float32:
            raise CfgppError(f"{name}: {n} must be fp32")
    if tuple(z_pano.shape) != (B, C_, g.Hp, g.Wp):
        raise CfgppError(f"{name}: z_pano shape {tuple(z_pano.shape)} != [{B}, {C_}, {g.Hp}, {g.Wp}]")
    if tuple(z_views.shape) != (g.n_views * B, C_, g.h, g.w):
        raise CfgppError(f"{name}: z_views shape {tuple(z_views.shape)} != [{g.n_views} * {B}, {C_}, {g.h}, {g.w}]")
    return _lib.PanoViewsC(B, C_, g.Hp, g.Wp, g.h, g.w, g.stride, int(bool(g.circular)), int(g.chunk_views))


def gather_views(g, z_pano: torch.Tensor, z_views: torch.Tensor):
    """``z_views`` [V * B, C, h, w] (row v * B + b) = the windows of ``z_pano`` [B, C, Hp, Wp], one launch (cfgpp_views_gather)"""
    lib = _lib.load()
    B, C_ = int(z_pano.shape[0]), int(z_pano.shape[1])
    vc = _pano_views_c(g, B, C_, "gather_views", z_pano, z_views)
    check(lib.cfgpp_views_gather(C.byref(vc), z_pano.data_ptr(), z_views.data_ptr(), _stream_ptr(z_pano)), "cfgpp_views_gather")


def step_ddim_views(g, z_pano: torch.Tensor, z0t_pano: torch.Tensor, z_views: torch.Tensor, eps: torch.Tensor, lam: float,
                    coeffs: Tuple[float, float, float, float], tweedie_uc: bool, renoise_uc: bool):
    """one MultiDiffusion step in one launch (cfgpp_step_ddim_views): every view's :func:`step_ddim` from ``z_pano`` and its rows of
    ``eps`` [V / Vc, 2 * Vc * B, C, h, w] fp16, the overlap average into ``z_pano`` (in place) / ``z0t_pano``, and the new latent
    scattered into ``z_views``"""
    lib = _lib.load()
    B, C_ = int(z_pano.shape[0]), int(z_pano.shape[1])
    vc = _pano_views_c(g, B, C_, "step_ddim_views", z_pano, z_views)
    _require_cuda(z0t_pano, "z0t_pano")
    _require_cuda(eps, "eps")
    if z0t_pano.dtype != torch.float32 or z0t_pano.shape != z_pano.shape:
        raise CfgppError("step_ddim_views: z0t_pano must be fp32 of z_pano's shape")
    want = (g.n_views // g.chunk_views, 2 * g.chunk_views * B, C_, g.h, g.w)
    if eps.dtype != torch.float16 or tuple(eps.shape) != want:
        raise CfgppError(f"step_ddim_views: eps must be fp16 {list(want)}, got {eps.dtype} {list(eps.shape)}")
    c1, c2, c3, c4 = (float(x) for x in coeffs)
    check(lib.cfgpp_step_ddim_views(C.byref(vc), z_pano.data_ptr(), z0t_pano.data_ptr(), z_views.data_ptr(), eps.data_ptr(), float(lam),
                                    c1, c2, c3, c4, int(bool(tweedie_uc)), int(bool(renoise_uc)), _stream_ptr(z_pano)),
          "cfgpp_step_ddim_views")


# ----------------------------------------------------------------------------
# UNet engine
# ----------------------------------------------------------------------------
def unet_config_c(cfg: UNetConfig, H: int, W: int, max_rows: int, out_channels: Optional[int] = None) -> UNetConfigC:
    """the C struct of include/cfgpp.h for ``cfg`` at latent H x W; ``out_channels=0`` makes a ControlNet"""
    cc = UNetConfigC()
    cc.in_channels = cfg.in_channels
    cc.out_channels = cfg.out_channels if out_channels is None else int(out_channels)
    cc.num_levels = cfg.num_levels
    for i in range(cfg.num_levels):
        cc.block_out_channels[i] = cfg.block_out_channels[i]
        cc.level_has_attn[i] = cfg.level_has_attn[i]
        cc.transformer_depth[i] = cfg.transformer_depth[i]
        cc.num_heads[i] = cfg.num_heads[i]
    cc.layers_per_block = cfg.layers_per_block
    cc.cross_attention_dim = cfg.cross_attention_dim
    cc.addition_embed = cfg.addition_embed
    cc.addition_time_embed_dim = cfg.addition_time_embed_dim
    cc.addition_pooled_dim = cfg.addition_pooled_dim
    cc.norm_groups = cfg.norm_groups
    cc.sample_h, cc.sample_w = int(H), int(W)
    cc.max_rows = int(max_rows)
    return cc


class HipUNet:
    """Hand-written HIP UNet behind the C ABI.  One instance per device."""

    def __init__(self, cfg: UNetConfig, max_rows: int, sample_hw: Optional[Tuple[int, int]] = None,
                 device: int = 0, max_tokens: int = 77, soft_regions: bool = False):
        """``max_tokens``: the longest text context ``set_context`` will take, 77 * j with j <= 4 (include/cfgpp_long_prompt.h:
        cfgpp_unet_set_max_tokens).  ``soft_regions``: also allocate the region-weight buffers (``enable_region_weights``)"""
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise CfgppError("HipUNet needs a ROCm GPU (torch.cuda.is_available() is False); "
                             "there is no CPU fallback for the HIP path")
        self.cfg = cfg
        self.device = int(device)
        self.max_rows = int(max_rows)
        H, W = sample_hw if sample_hw is not None else (cfg.sample_size, cfg.sample_size)
        self.H, self.W = int(H), int(W)
        cc = unet_config_c(cfg, self.H, self.W, self.max_rows)
        self._h = self.lib.cfgpp_unet_create(C.byref(cc), self.device)
        if not self._h:
            raise CfgppError("cfgpp_unet_create failed: " + _lib.last_error())
        self._keep = {}          # tensors the engine holds raw pointers to
        self.finalized = False
        self.max_tokens = 77
        if int(max_tokens) != 77:
            self.set_max_tokens(max_tokens)
        self.soft_regions_enabled = False
        self.soft_regions = 0                        # n_regions while region weights are set (set_region_weights)
        if soft_regions:
            self.enable_region_weights()
        self.time_cond = 0                           # time_cond_proj_dim of a guidance-embedded UNet (include/cfgpp_lcm.h)
        if int(getattr(cfg, "time_cond_proj_dim", 0)):
            self.set_time_cond(cfg.time_cond_proj_dim)
        self.freeu = None                            # (s1, s2, b1, b2) while FreeU is on (set_freeu)
        self.latent_channels = cfg.out_channels     # z carries these; an inpaint UNet's other inputs come from image_condition
        self.cond_channels = cfg.in_channels - cfg.out_channels

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                torch.cuda.synchronize()
            except Exception:
                pass
            self.lib.cfgpp_unet_destroy(h)
            self._h = None

    # -- weights ---------------------------------------------------------------
    def load_tensor(self, key: str, t: torch.Tensor):
        t = t.detach().cpu().contiguous()
        if t.dtype == torch.float16:
            dt = 1
        else:
            t = t.to(torch.float32)
            dt = 0
        shape = (C.c_long * t.dim())(*t.shape)
        check(self.lib.cfgpp_unet_load_tensor(self._h, key.encode(), t.data_ptr(), dt, shape, t.dim()),
              f"cfgpp_unet_load_tensor({key})")

    def load_state_dict(self, items: Iterable[Tuple[str, torch.Tensor]]):
        if isinstance(items, dict):
            items = items.items()
        for k, v in items:
            self.load_tensor(k, v)
        return self

    def set_max_tokens(self, max_tokens: int):
        """before ``finalize``: size the cross-attention buffers for contexts of up to ``max_tokens`` = 77, 154, 231 or 308 tokens"""
        check(self.lib.cfgpp_unet_set_max_tokens(self._h, int(max_tokens)), "cfgpp_unet_set_max_tokens")
        self.max_tokens = int(max_tokens)
        return self

    def set_time_cond(self, dim: int):
        """before ``finalize``: the UNet has ``time_embedding.cond_proj`` [c0, dim] (include/cfgpp_lcm.h: cfgpp_unet_set_time_cond)"""
        check(self.lib.cfgpp_unet_set_time_cond(self._h, int(dim)), "cfgpp_unet_set_time_cond")
        self.time_cond = int(dim)
        return self

    def guidance_embedding(self, w_emb):
        """once per job on a guidance-embedded UNet: ``w_emb`` [time_cond] (``lcm.guidance_scale_embedding``), host values"""
        w = [float(v) for v in w_emb]
        if len(w) != self.time_cond or not self.time_cond:
            raise CfgppError(f"guidance_embedding: {len(w)} values for time_cond_proj_dim={self.time_cond}")
        check(self.lib.cfgpp_unet_guidance_embedding(self._h, (C.c_float * len(w))(*w), _stream_ptr()), "cfgpp_unet_guidance_embedding")
        return self

    def finalize(self):
        check(self.lib.cfgpp_unet_finalize(self._h), "cfgpp_unet_finalize")
        self.finalized = True
        return self

    # -- conditioning ------------------------------------------------------------
    def set_context(self, ehs: torch.Tensor, text_embeds: Optional[torch.Tensor] = None,
                    time_ids: Optional[torch.Tensor] = None):
        """ehs [rows,77 * j,D] with 77 * j <= max_tokens (uc rows first, then c rows).  SDXL: text_embeds [rows|1,1280], time_ids [rows|1,6]."""
        dev = torch.device("cuda", self.device)
        ehs = ehs.to(device=dev, dtype=torch.float16).contiguous()
        rows, tokens = int(ehs.shape[0]), int(ehs.shape[1])
        te = ti = None
        cond_rows = 0
        if self.cfg.addition_embed:
            if text_embeds is None or time_ids is None:
                raise CfgppError("set_context: SDXL needs text_embeds and time_ids")
            te = text_embeds.to(device=dev, dtype=torch.float16).contiguous()
            ti = time_ids.to(device=dev, dtype=torch.float32).contiguous()
            cond_rows = int(te.shape[0])
            if int(ti.shape[0]) != cond_rows:
                raise CfgppError("set_context: text_embeds / time_ids row mismatch")
        self._keep["ctx"] = (ehs, te, ti)
        self.rows = rows
        check(self.lib.cfgpp_unet_set_context(self._h, ehs.data_ptr(), rows, tokens, _ptr(te), _ptr(ti), cond_rows,
                                              _stream_ptr(ehs)), "cfgpp_unet_set_context")

    def set_regions(self, ids: Optional[torch.Tensor], n_regions: int = 0):
        """regional prompts on the finalized engine (include/cfgpp_regions.h: cfgpp_unet_set_regions): ``ids`` is an integer region
        map [1 or rows, H, W] with ids < ``n_regions`` = 2 .. 4, and the context to follow holds ``n_regions`` chunks of 77 tokens.
        ``None`` turns regions off: the plain engine.  The map is copied into the engine's own buffers, once per call."""
        if ids is None:
            check(self.lib.cfgpp_unet_set_regions(self._h, None, 0, 0), "cfgpp_unet_set_regions")
            self.regions = 0
            return self
        ids = torch.as_tensor(ids)
        if ids.dim() == 2:
            ids = ids[None]
        if ids.dim() != 3 or tuple(ids.shape[1:]) != (self.H, self.W):
            raise CfgppError(f"set_regions: region map of shape {tuple(ids.shape)}, expected [1 or rows, {self.H}, {self.W}]")
        if ids.is_floating_point() or int(ids.min()) < 0 or int(ids.max()) > 255:
            raise CfgppError("set_regions: the region map must hold integer ids 0 .. n_regions - 1")
        host = ids.detach().to("cpu", torch.uint8).contiguous()
        check(self.lib.cfgpp_unet_set_regions(self._h, host.data_ptr(), int(host.shape[0]), int(n_regions)), "cfgpp_unet_set_regions")
        self.regions = int(n_regions)
        self.soft_regions = 0            # exclusive: the engine cleared its region weights
        return self

    def enable_region_weights(self):
        """before ``finalize``, after ``set_max_tokens`` (> 77): allocate the per-level fp32 region-weight buffers at finalize
        (include/cfgpp_regions_soft.h: cfgpp_unet_enable_region_weights)"""
        check(self.lib.cfgpp_unet_enable_region_weights(self._h), "cfgpp_unet_enable_region_weights")
        self.soft_regions_enabled = True
        return self

    def set_region_weights(self, w: Optional[torch.Tensor]):
        """soft regional prompts on the finalized engine (include/cfgpp_regions_soft.h: cfgpp_unet_set_region_weights): ``w`` is a
        float map [1 or rows, R, H, W], R = 2 .. 4, every pixel's weights summing to 1, and the context to follow holds R chunks of
        77 tokens.  ``None`` turns the weights off.  Setting weights clears a hard region map and the reverse."""
        if w is None:
            check(self.lib.cfgpp_unet_set_region_weights(self._h, None, 0, 0), "cfgpp_unet_set_region_weights")
            self.soft_regions = 0
            return self
        w = torch.as_tensor(w)
        if w.dim() == 3:
            w = w[None]
        if w.dim() != 4 or tuple(w.shape[2:]) != (self.H, self.W) or not w.is_floating_point():
            raise CfgppError(f"set_region_weights: weights of shape {tuple(w.shape)}, expected a float [1 or rows, R, {self.H}, {self.W}]")
        host = w.detach().to("cpu", torch.float32).contiguous()
        check(self.lib.cfgpp_unet_set_region_weights(self._h, host.data_ptr(), int(host.shape[0]), int(host.shape[1])),
              "cfgpp_unet_set_region_weights")
        self.soft_regions = int(host.shape[1])
        self.regions = 0
        return self

    def image_condition(self, cond: torch.Tensor):
        """inpaint UNets only: the step-invariant extra input channels ``cond`` [1 or z_rows, in - out, H, W] (mask, masked-image
        latent: diffusers' channel order), copied into the engine (include/cfgpp.h: cfgpp_unet_image_condition)."""
        if self.cond_channels <= 0:
            raise CfgppError(f"image_condition: {self.cfg.name} takes no image condition (in_channels == out_channels)")
        dev = torch.device("cuda", self.device)
        cond = cond.to(device=dev, dtype=torch.float16).contiguous()
        if cond.dim() != 4 or tuple(cond.shape[1:]) != (self.cond_channels, self.H, self.W):
            raise CfgppError(f"image_condition: cond shape {tuple(cond.shape)} != [*, {self.cond_channels}, {self.H}, {self.W}]")
        check(self.lib.cfgpp_unet_image_condition(self._h, cond.data_ptr(), int(cond.shape[0]), _stream_ptr(cond)),
              "cfgpp_unet_image_condition")
        self._keep["cond"] = cond          # the copy is asynchronous on the current stream: keep the source alive

    # -- forward -----------------------------------------------------------------
    def forward(self, z: torch.Tensor, t: float, eps_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """eps[rows,4,H,W] fp16 = UNet(z[row % z_rows], t); rows were fixed by set_context."""
        _require_cuda(z, "z")
        if z.dtype not in (torch.float16, torch.float32):
            raise CfgppError("forward: z must be fp16 or fp32")
        zr = int(z.shape[0])
        if tuple(z.shape[1:]) != (self.latent_channels, self.H, self.W):
            raise CfgppError(f"forward: z shape {tuple(z.shape)} != [*, {self.latent_channels}, {self.H}, {self.W}]")
        rows = self.rows
        if rows % zr != 0:
            raise CfgppError(f"forward: rows={rows} is not a multiple of z rows={zr}")
        if eps_out is None:
            eps_out = torch.empty((rows, self.cfg.out_channels, self.H, self.W), dtype=torch.float16, device=z.device)
        check(self.lib.cfgpp_unet_forward(self._h, z.data_ptr(), 1 if z.dtype == torch.float16 else 0, zr, float(t),
                                          eps_out.data_ptr(), rows, _stream_ptr(z)), "cfgpp_unet_forward")
        return eps_out

    # -- LoRA ----------------------------------------------------------------------
    def _matrix_shape(self, key: str):
        from .unet_config import param_shapes
        shapes = getattr(self, "_shapes", None)
        if shapes is None:
            shapes = self._shapes = dict(param_shapes(self.cfg))
        return shapes.get(key)

    def lora(self, key: str, up: Optional[torch.Tensor], down: Optional[torch.Tensor]):
        """weight ``key`` = fp16(base + up @ down) in place on the device (include/cfgpp.h: cfgpp_unet_lora).  ``up`` [O, rank],
        ``down`` [rank, I*kh*kw] (OIHW flattening), any float dtype / device: they are made fp32 on the engine's device.
        ``up is None`` (or rank 0) restores the base bit for bit.  After a change of attn2.to_k / to_v call ``set_context`` again."""
        dev = torch.device("cuda", self.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        if up is None or int(up.shape[1]) == 0:
            check(self.lib.cfgpp_unet_lora(self._h, key.encode(), None, None, 0, stream), f"cfgpp_unet_lora({key})")
            return
        shape = self._matrix_shape(key)
        if shape is not None and len(shape) in (2, 4):         # (anything else: the engine's own refusal names the key)
            O, K = int(shape[0]), 1
            for d in shape[1:]:
                K *= int(d)
            if up.dim() != 2 or down.dim() != 2 or int(up.shape[0]) != O or int(down.shape[1]) != K or int(up.shape[1]) != int(down.shape[0]):
                raise CfgppError(f"lora({key}): up {tuple(up.shape)} / down {tuple(down.shape)} do not fit the weight {tuple(shape)} "
                                 f"(up [{O}, rank], down [rank, {K}])")
        up = up.to(device=dev, dtype=torch.float32).contiguous()
        down = down.to(device=dev, dtype=torch.float32).contiguous()
        check(self.lib.cfgpp_unet_lora(self._h, key.encode(), up.data_ptr(), down.data_ptr(), int(up.shape[1]), stream),
              f"cfgpp_unet_lora({key})")
        # up / down are released here: the merge is enqueued on the stream torch's caching allocator orders their memory by, so a
        # later allocation cannot reuse it before the kernel ran, and no adapter copy stays resident on the device

    def read_weight(self, key: str) -> torch.Tensor:
        """the current weight of ``key`` in checkpoint order, fp16 on the host (cfgpp_debug.h: cfgpp_unet_read_weight)"""
        shape = self._matrix_shape(key)
        if shape is None:
            raise CfgppError(f"read_weight: unknown key {key}")
        out = torch.empty(tuple(shape), dtype=torch.float16)
        check(self.lib.cfgpp_unet_read_weight(self._h, key.encode(), out.data_ptr()), f"cfgpp_unet_read_weight({key})")
        return out

    # -- IP-Adapter --------------------------------------------------------------------
    def ip_load(self, key: Optional[str], t: Optional[torch.Tensor] = None):
        """one adapter tensor by its engine key (include/cfgpp_ip_adapter.h: cfgpp_unet_ip_load); ``key is None`` drops the adapter"""
        if key is None:
            check(self.lib.cfgpp_unet_ip_load(self._h, None, None, 0, None, 0), "cfgpp_unet_ip_load(NULL)")
            self._keep.pop("ip_embeds", None)
            return
        t = t.detach().cpu().contiguous()
        if t.dtype == torch.float16:
            dt = 1
        else:
            t = t.to(torch.float32)
            dt = 0
        shape = (C.c_long * t.dim())(*t.shape)
        check(self.lib.cfgpp_unet_ip_load(self._h, key.encode(), t.data_ptr(), dt, shape, t.dim()), f"cfgpp_unet_ip_load({key})")

    def set_image_context(self, image_embeds: Optional[torch.Tensor], scale: float = 1.0):
        """image_embeds [rows, embed_dim] (uc rows first, then c rows; rows of the current text context); None or scale 0
        deactivates (include/cfgpp_ip_adapter.h: cfgpp_unet_image_context).  A 3-D tensor [rows, seq, embed_dim] is the image tower's
        hidden states for a Resampler ("plus") adapter (include/cfgpp_ip_plus.h: cfgpp_unet_image_context_seq); the engine refuses
        the form that does not fit the loaded adapter's kind.  The engine identifies the embeds by address, so the tensor of the
        last call is kept alive here and an equal tensor is not copied again."""
        dev = torch.device("cuda", self.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        if image_embeds is None or float(scale) == 0.0:
            check(self.lib.cfgpp_unet_image_context(self._h, None, 0, 0, 0.0, stream), "cfgpp_unet_image_context")
            return
        e = image_embeds.to(device=dev, dtype=torch.float16).contiguous()
        if e.dim() not in (2, 3):
            raise CfgppError(f"set_image_context: image_embeds shape {tuple(e.shape)}, expected [rows, embed_dim] (Linear adapters) or "
                             "[rows, seq, embed_dim] (Resampler adapters)")
        old = self._keep.get("ip_embeds")
        if old is not None and old.shape == e.shape and bool(torch.equal(old, e)):
            e = old                         # the same values: only the scale changes, nothing is projected again
        else:
            e = e.clone()                   # a private copy (the old one is still alive: a new address), safe from in-place edits
        if e.dim() == 3:                    # hidden states for a Resampler adapter (include/cfgpp_ip_plus.h)
            check(self.lib.cfgpp_unet_image_context_seq(self._h, e.data_ptr(), int(e.shape[0]), int(e.shape[1]), int(e.shape[2]), float(scale),
                                                        stream), "cfgpp_unet_image_context_seq")
        else:
            check(self.lib.cfgpp_unet_image_context(self._h, e.data_ptr(), int(e.shape[0]), int(e.shape[1]), float(scale), stream),
                  "cfgpp_unet_image_context")
        self._keep["ip_embeds"] = e

    def ip_tokens(self, rows: int, n_img: int) -> torch.Tensor:
        """the [rows, n_img, cross_attention_dim] fp16 image tokens of the last image context (csrc/cfgpp_debug.h: cfgpp_unet_ip_tokens)"""
        out = torch.empty((int(rows), int(n_img), self.cfg.cross_attention_dim), dtype=torch.float16)
        check(self.lib.cfgpp_unet_ip_tokens(self._h, out.data_ptr(), int(rows)), "cfgpp_unet_ip_tokens")
        return out

    def set_freeu(self, spec):
        """diffusers' ``enable_freeu(s1, s2, b1, b2)`` (``spec`` = that tuple, or a mapping with those keys) / ``disable_freeu()``
        (None) on the finalized engine (include/cfgpp_freeu.h: cfgpp_unet_set_freeu).  Host state only; the next forward sees it."""
        from .freeu import parse_freeu
        v = parse_freeu(spec)
        s1, s2, b1, b2 = v if v is not None else (1.0, 1.0, 1.0, 1.0)
        check(self.lib.cfgpp_unet_set_freeu(self._h, s1, s2, b1, b2, 0 if v is None else 1), "cfgpp_unet_set_freeu")
        self.freeu = v
        return self

    def attach_control(self, cn, scale: float):
        """attach ControlNet ``cn`` (a finalized :class:`cfgpp_amd.controlnet.HipControlNet`; None detaches) with
        ``conditioning_scale`` (include/cfgpp.h: cfgpp_unet_attach_control).  Synchronises the device."""
        check(self.lib.cfgpp_unet_attach_control(self._h, None if cn is None else cn._h, float(scale)), "cfgpp_unet_attach_control")
        self._keep["control"] = cn          # the engine holds cn's raw handle

    def sample_graph_ddim(self, z: torch.Tensor, z0t: torch.Tensor, eps: torch.Tensor, eps_uc: torch.Tensor, eps_c: torch.Tensor,
                          steps, lam: float, tweedie_uc: bool, renoise_uc: bool):
        """the whole DDIM loop as hipGraph replays (include/cfgpp.h: cfgpp_sample_graph_ddim).  ``steps``: per step
        ``(t, c1, c2, c3, c4)`` - what the eager loop passes to ``forward`` and ``step_ddim``; z is updated in place."""
        for n, t in (("z", z), ("z0t", z0t), ("eps", eps)):
            _require_cuda(t, n)
        if z.dtype != z0t.dtype or z.dtype not in (torch.float16, torch.float32) or eps.dtype != torch.float16:
            raise CfgppError("sample_graph_ddim: z / z0t must both be fp32 or both fp16, eps fp16")
        if tuple(z.shape[1:]) != (self.latent_channels, self.H, self.W) or z.shape != z0t.shape:
            raise CfgppError(f"sample_graph_ddim: z shape {tuple(z.shape)}")
        if int(eps.shape[0]) != self.rows or self.rows % int(z.shape[0]) != 0:
            raise CfgppError(f"sample_graph_ddim: eps rows {int(eps.shape[0])} / z rows {int(z.shape[0])} vs context rows {self.rows}")
        flat = [float(v) for st in steps for v in st]
        if len(flat) != 5 * len(steps) or not steps:
            raise CfgppError("sample_graph_ddim: steps must be a non-empty list of (t, c1, c2, c3, c4)")
        arr = (C.c_float * len(flat))(*flat)
        check(self.lib.cfgpp_sample_graph_ddim(self._h, z.data_ptr(), z0t.data_ptr(), 1 if z.dtype == torch.float16 else 0, int(z.shape[0]),
                                               eps.data_ptr(), eps_uc.data_ptr(), eps_c.data_ptr(), self.rows, arr, len(steps), float(lam),
                                               int(bool(tweedie_uc)), int(bool(renoise_uc)), _stream_ptr(z)), "cfgpp_sample_graph_ddim")

    def profile(self, z: torch.Tensor, t: float, detail: bool = False) -> dict:
        """One forward with HIP events between launches: per kernel family ms / algorithmic flops / launches."""
        _require_cuda(z, "z")
        rows = self.rows
        eps = torch.empty((rows, self.cfg.out_channels, self.H, self.W), dtype=torch.float16, device=z.device)
        ms, fl, ln = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_int * 4)()
        buf = C.create_string_buffer(1 << 20) if detail else None
        check(self.lib.cfgpp_unet_profile(self._h, z.data_ptr(), 1 if z.dtype == torch.float16 else 0, int(z.shape[0]),
                                          float(t), eps.data_ptr(), rows, _stream_ptr(z), ms, fl, ln, buf, (1 << 20) if detail else 0),
              "cfgpp_unet_profile")
        names = ("igemm", "attention", "norm", "small")
        out = {n: dict(ms=ms[i], flops=fl[i], launches=ln[i]) for i, n in enumerate(names)}
        if detail:
            out["detail"] = buf.value.decode()
        return out

    def export_tuning(self, rows: Optional[int] = None):
        """tile config pinned per igemm launch by the in-situ tuning at this batch (list of ints, plan order)"""
        rows = self.rows if rows is None else int(rows)
        buf = (C.c_int * 4096)()
        n = self.lib.cfgpp_unet_tuning(self._h, rows, buf, 4096, 0)
        if n < 0:
            raise CfgppError("cfgpp_unet_tuning: " + _lib.last_error())
        return [int(buf[i]) for i in range(n)]

    def import_tuning(self, hints, rows: int):
        buf = (C.c_int * len(hints))(*[int(h) for h in hints])
        n = self.lib.cfgpp_unet_tuning(self._h, int(rows), buf, len(hints), 1)
        if n < 0:
            raise CfgppError("cfgpp_unet_tuning: " + _lib.last_error())

    def flops(self, rows: int) -> float:
        """algorithmic FLOPs of one forward at ``rows``; the shared CFG prefix counts once when the most recent forward shared it"""
        return float(self.lib.cfgpp_unet_flops(self._h, int(rows)))

    def shared_prefix_ops(self, rows: int, z_rows: int) -> int:
        """plan ops a forward at (rows, z_rows) runs at rows / 2 (0: it does not share; cfgpp_debug.h)"""
        return int(self.lib.cfgpp_unet_shared_prefix_ops(self._h, int(rows), int(z_rows)))

    def device_bytes(self) -> float:
        return float(self.lib.cfgpp_unet_device_bytes(self._h))


def set_share_prefix(on: bool):
    """process-global A/B switch of the shared CFG prefix (default on; cfgpp_debug.h: cfgpp_unet_set_share_prefix)"""
    _lib.load().cfgpp_unet_set_share_prefix(1 if on else 0)


def share_prefix_enabled() -> bool:
    return bool(_lib.load().cfgpp_unet_share_prefix_enabled())
