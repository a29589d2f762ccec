"""Thin test-side wrappers that call the single-op C-ABI entry points of
libcfgpp_hip.so on torch CUDA tensors, plus layout helpers (halo-padded NHWC,
head-major Q/K/V^T) and the repacking the engine does at finalize()."""
from __future__ import annotations

import torch

from cfgpp_amd import _lib
from cfgpp_amd._lib import check

DEV = "cuda"


def lib():
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def round_up(a, b):
    return (a + b - 1) // b * b


# ---- layouts ----------------------------------------------------------------
def to_pn(x_nchw: torch.Tensor) -> torch.Tensor:
    """NCHW (any float) -> halo-padded NHWC fp16 on the GPU."""
    N, C, H, W = x_nchw.shape
    out = torch.zeros((N, H + 2, W + 2, C), dtype=torch.float16, device=DEV)
    out[:, 1:H + 1, 1:W + 1, :] = x_nchw.permute(0, 2, 3, 1).to(DEV, torch.float16)
    return out


def empty_pn(N, H, W, C) -> torch.Tensor:
    return torch.zeros((N, H + 2, W + 2, C), dtype=torch.float16, device=DEV)


def from_pn(pn: torch.Tensor) -> torch.Tensor:
    """halo-padded NHWC -> NCHW fp32 CPU (interior only)."""
    N, Hp, Wp, C = pn.shape
    return pn[:, 1:Hp - 1, 1:Wp - 1, :].permute(0, 3, 1, 2).float().cpu()


def halo_is_zero(pn: torch.Tensor) -> bool:
    a = pn.float()
    return bool((a[:, 0].abs().sum() + a[:, -1].abs().sum() + a[:, :, 0].abs().sum() + a[:, :, -1].abs().sum()) == 0)


def pack_conv3(w_oihw: torch.Tensor) -> torch.Tensor:
    """OIHW -> [O][I/64][9][64] fp16 (k = (cb*9 + tap)*64 + c: channel-block major, tap minor)."""
    O, I, kh, kw = w_oihw.shape
    return (w_oihw.permute(0, 2, 3, 1).reshape(O, kh * kw, I // 64, 64).permute(0, 2, 1, 3)
            .reshape(O, kh * kw * I).to(DEV, torch.float16).contiguous())


def pack_geglu(w: torch.Tensor, b: torch.Tensor):
    """[8C, C] -> packed rows: per 64 packed rows, [0,32) value features, [32,64) gate features."""
    F4 = w.shape[0] // 2
    f = torch.arange(F4)
    pv = (f // 32) * 64 + (f % 32)
    wp = torch.empty_like(w)
    bp = torch.empty_like(b)
    wp[pv] = w[:F4]
    wp[pv + 32] = w[F4:]
    bp[pv] = b[:F4]
    bp[pv + 32] = b[F4:]
    return wp.to(DEV, torch.float16).contiguous(), bp.to(DEV, torch.float32).contiguous()


# ---- ops ----------------------------------------------------------------------
def igemm(a0, a1, C0, C1, taps, amode, H, W, w, M, N, bias=None, temb=None, temb_ld=0, resid=None, rmode=0, rld=0,
          out=None, omode=0, old=0, epi=0):
    check(lib().cfgpp_op_igemm(P(a0), P(a1), C0, C1, taps, amode, H, W, P(w), M, N, P(bias), P(temb), temb_ld,
                               P(resid), rmode, rld, P(out), omode, old, epi, stream()), "cfgpp_op_igemm")
    return out


def igemm_ex(a0, a1, C0, C1, taps, amode, H, W, w, M, N, bias=None, temb=None, temb_ld=0, resid=None, rmode=0, rld=0,
             out=None, omode=0, old=0, epi=0, ashift=0, out_scale=1.0, cfg_hint=0):
    """cfgpp_op_igemm plus ashift, out_scale and the tuner's cfg_hint (cfgpp_debug.h)"""
    check(lib().cfgpp_op_igemm_ex(P(a0), P(a1), C0, C1, taps, amode, H, W, P(w), M, N, P(bias), P(temb), temb_ld,
                                  P(resid), rmode, rld, P(out), omode, old, epi, ashift, float(out_scale), cfg_hint, stream()),
          "cfgpp_op_igemm_ex")
    return out


def igemm_last_launch():
    """what the last implicit-GEMM launch issued, 16 slots (cfgpp_debug.h: cfgpp_igemm_last_launch)"""
    return _last_launch("cfgpp_igemm_last_launch", 16)


def linear(a, w, bias=None, resid=None, epi=0):
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty((M, N // 2 if epi == 1 else N), dtype=torch.float16, device=DEV)
    igemm(a, None, K, 0, 1, 0, 0, 0, w, M, N, bias=bias, resid=resid, rmode=0, rld=N, out=out, omode=0,
          old=out.shape[1], epi=epi)
    return out


def conv3x3(x_pn, w_packed, bias, Hout, Wout, amode=1, temb=None, temb_ld=0, resid_pn=None):
    N = x_pn.shape[0]
    Cin = x_pn.shape[3]
    Cout = w_packed.shape[0]
    out = empty_pn(N, Hout, Wout, Cout)
    igemm(x_pn, None, Cin, 0, 9, amode, Hout, Wout, w_packed, N * Hout * Wout, Cout, bias=bias, temb=temb,
          temb_ld=temb_ld, resid=resid_pn, rmode=1, rld=Cout, out=out, omode=1, old=Cout, epi=0)
    return out


def conv1x1_2src(x0_pn, x1_pn, w, bias):
    N, Hp, Wp, C0 = x0_pn.shape
    H, W = Hp - 2, Wp - 2
    C1 = 0 if x1_pn is None else x1_pn.shape[3]
    Cout = w.shape[0]
    out = empty_pn(N, H, W, Cout)
    igemm(x0_pn, x1_pn, C0, C1, 1, 1, H, W, w, N * H * W, Cout, bias=bias, out=out, omode=1, old=Cout)
    return out


def _norm_dst(out, N, H, W, C, dst_padded):
    """the destination of a GroupNorm: a fresh one, or `out` - a contiguous fp16 device tensor [N, H+2, W+2, C] (halo-padded) or
    [N*H*W, C] (token-major) to write into (tests that watch what the kernel leaves untouched)"""
    shape = (N, H + 2, W + 2, C) if dst_padded else (N * H * W, C)
    if out is None:
        return empty_pn(N, H, W, C) if dst_padded else torch.empty(shape, dtype=torch.float16, device=DEV)
    assert out.is_contiguous() and out.dtype == torch.float16 and tuple(out.shape) == shape
    return out


def groupnorm(x0_pn, x1_pn, gamma, beta, G, eps, silu, dst_padded=True, out=None):
    N, Hp, Wp, C0 = x0_pn.shape
    H, W = Hp - 2, Wp - 2
    C1 = 0 if x1_pn is None else x1_pn.shape[3]
    C = C0 + C1
    stats = torch.zeros(N * (1024 * G * 2 + G * 2), dtype=torch.float32, device=DEV)
    dst = _norm_dst(out, N, H, W, C, dst_padded)
    check(lib().cfgpp_op_groupnorm(P(x0_pn), P(x1_pn), P(dst), P(gamma), P(beta), P(stats), N, H, W, C0, C1, G,
                                   float(eps), int(silu), int(dst_padded), stream()), "cfgpp_op_groupnorm")
    return dst


def groupnorm_pre(x0_pn, x1_pn, gst0, gst1, gamma, beta, G, eps, silu, dst_padded=True, out=None):
    """GroupNorm with the statistics its inputs' producers left behind (cfgpp_op_igemm_set_gstat)"""
    N, Hp, Wp, C0 = x0_pn.shape
    H, W = Hp - 2, Wp - 2
    C1 = 0 if x1_pn is None else x1_pn.shape[3]
    stats = torch.zeros(N * G * 2, dtype=torch.float32, device=DEV)
    dst = _norm_dst(out, N, H, W, C0 + C1, dst_padded)
    check(lib().cfgpp_op_groupnorm_pre(P(x0_pn), P(x1_pn), P(dst), P(gamma), P(beta), P(gst0), P(gst1), P(stats), N, H, W, C0, C1, G,
                                       float(eps), int(silu), int(dst_padded), stream()), "cfgpp_op_groupnorm_pre")
    return dst


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    y = torch.empty_like(x) if out is None else out
    assert y.is_contiguous() and y.dtype == torch.float16 and y.shape == x.shape
    check(lib().cfgpp_op_layernorm(P(x), P(y), P(gamma), P(beta), x.shape[0], x.shape[1], float(eps), stream()),
          "cfgpp_op_layernorm")
    return y


def softmax_rows(s):
    """row softmax of the contiguous fp16 device tensor s [rows, ncols], in place"""
    assert s.is_contiguous() and s.dtype == torch.float16 and s.dim() == 2
    check(lib().cfgpp_op_softmax_rows(P(s), s.shape[0], s.shape[1], stream()), "cfgpp_op_softmax_rows")
    return s


def _last_launch(name, n):
    import ctypes
    out = (ctypes.c_int * n)()
    getattr(lib(), name)(out)
    return tuple(out)


def groupnorm_last_launch():
    """(form, NT, MAXCH, gs, cpp, stats pix_per_block, stats nblk, apply pix_per_block) of the last GroupNorm call (cfgpp_debug.h)"""
    return _last_launch("cfgpp_groupnorm_last_launch", 8)


def layernorm_last_launch():
    """(MAXV, RPW) of the last cfgpp_op_layernorm call"""
    return _last_launch("cfgpp_layernorm_last_launch", 2)


def softmax_last_launch():
    """(MAXC,) of the last cfgpp_op_softmax_rows call"""
    return _last_launch("cfgpp_softmax_last_launch", 1)


def heads_project(a, w, B, tokens, C, nheads, part0, nparts, q_pad, k_pad):
    """a [B*tokens, K] x w [nparts*C, K] -> head-major buffers (zero initialised)."""
    d = C // nheads
    dp = round_up(d, 32)
    hq = torch.zeros((B * nheads, q_pad, dp), dtype=torch.float16, device=DEV)
    hk = torch.zeros((B * nheads, k_pad, dp), dtype=torch.float16, device=DEV)
    hvt = torch.zeros((B * nheads, dp, k_pad), dtype=torch.float16, device=DEV)
    check(lib().cfgpp_op_attention_prepare_vt(P(hvt), B * nheads, d, k_pad, stream()), "cfgpp_op_attention_prepare_vt")
    check(lib().cfgpp_op_igemm_heads(P(a), a.shape[1], P(w), a.shape[0], w.shape[0], None, tokens, P(hq), P(hk),
                                     P(hvt), part0, C, d, nheads, q_pad, k_pad, stream()), "cfgpp_op_igemm_heads")
    return hq, hk, hvt


def vt_pos(n):
    """column of key 0..n-1 in a V^T buffer (bits 2 and 3 of the key index swapped; include/cfgpp.h)"""
    key = torch.arange(n)
    return (key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1)


def make_heads(q, k, v):
    """q [B,h,Nq,d], k/v [B,h,Nk,d] (cpu float) -> padded head-major device buffers."""
    B, h, Nq, d = q.shape
    Nk = k.shape[2]
    dp = round_up(d, 32)
    q_pad, k_pad = round_up(Nq, 128), round_up(Nk, 64)
    hq = torch.zeros((B * h, q_pad, dp), dtype=torch.float16, device=DEV)
    hk = torch.zeros((B * h, k_pad, dp), dtype=torch.float16, device=DEV)
    hvt = torch.zeros((B * h, dp, k_pad), dtype=torch.float16, device=DEV)
    hq[:, :Nq, :d] = q.reshape(B * h, Nq, d).to(DEV, torch.float16)
    hk[:, :Nk, :d] = k.reshape(B * h, Nk, d).to(DEV, torch.float16)
    # V^T contract: within every 32-key block the key index has bits 2 and 3 swapped (include/cfgpp.h)
    hvt[:, :d, vt_pos(Nk).to(DEV)] = v.reshape(B * h, Nk, d).transpose(1, 2).to(DEV, torch.float16)
    check(lib().cfgpp_op_attention_prepare_vt(P(hvt), B * h, d, k_pad, stream()), "cfgpp_op_attention_prepare_vt")   # ones row when d % 32 != 0
    return hq, hk, hvt, q_pad, k_pad


def attention(hq, hk, hvt, B, nheads, d, nq, nk, q_pad, k_pad, out=None):
    """out: a contiguous [B, nq, nheads * d] fp16 device tensor to write into (tests that watch what the kernel leaves untouched)"""
    o = torch.empty((B, nq, nheads * d), dtype=torch.float16, device=DEV) if out is None else out
    assert o.is_contiguous() and o.dtype == torch.float16 and tuple(o.shape) == (B, nq, nheads * d)
    check(lib().cfgpp_op_attention(P(hq), P(hk), P(hvt), P(o), B, nheads, d, nq, nk, q_pad, k_pad, stream()),
          "cfgpp_op_attention")
    return o


def attention_last_launch():
    """(kernel, D16, ONES, xqb) of the last cfgpp_op_attention call (cfgpp_debug.h: cfgpp_attention_last_launch)"""
    import ctypes
    out4 = (ctypes.c_int * 4)()
    lib().cfgpp_attention_last_launch(out4)
    return tuple(out4)


def conv_in(z, w_oihw, bias, R):
    zB, Cin, H, W = z.shape
    Cout = w_oihw.shape[0]
    wk = w_oihw.permute(2, 3, 1, 0).reshape(9 * Cin, Cout).to(DEV, torch.float32).contiguous()
    out = empty_pn(R, H, W, Cout)
    check(lib().cfgpp_op_conv_in(P(z), int(z.dtype == torch.float16), P(out), P(wk), P(bias), R, zB, Cin, H, W, Cout,
                                 stream()), "cfgpp_op_conv_in")
    return out


def conv_out(x_pn, w_oihw, bias, out_half=True):
    R, Hp, Wp, C = x_pn.shape
    H, W = Hp - 2, Wp - 2
    Co = w_oihw.shape[0]
    wk = w_oihw.permute(0, 2, 3, 1).reshape(Co, 9, C).to(DEV, torch.float16).contiguous()
    out = torch.empty((R, Co, H, W), dtype=torch.float16 if out_half else torch.float32, device=DEV)
    check(lib().cfgpp_op_conv_out(P(x_pn), P(out), int(out_half), P(wk), P(bias), R, H, W, C, Co, stream()),
          "cfgpp_op_conv_out")
    return out


def sinusoid(vals, dim):
    out = torch.empty((vals.numel(), dim), dtype=torch.float32, device=DEV)
    check(lib().cfgpp_op_sinusoid(P(vals), 0.0, P(out), vals.numel(), dim, dim, 0, stream()), "cfgpp_op_sinusoid")
    return out


def skinny(x, w, bias, silu_in=False, silu_out=False, addend=None):
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=DEV)
    check(lib().cfgpp_op_skinny_gemm(P(x), K, P(w), P(bias), P(addend), N if addend is not None else 0, P(out), N, M, N,
                                     K, int(silu_in), int(silu_out), stream()), "cfgpp_op_skinny_gemm")
    return out


def err_stats(got: torch.Tensor, ref: torch.Tensor) -> dict:
    g = got.detach().float().cpu()
    r = ref.detach().float().cpu()
    diff = (g - r)
    return dict(rel_l2=float(diff.norm() / (r.norm() + 1e-30)), max_abs=float(diff.abs().max()),
                ref_max=float(r.abs().max()), finite=bool(torch.isfinite(g).all()))


# ---- small kernels (csrc/small_kernels.hip), every argument of the C entry points; `out=`: a contiguous device tensor to write into
# (tests that watch what the kernel leaves untouched) ---------------------------------------------------------------------------------
def _dst(out, shape, dtype):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=DEV)
    assert out.is_contiguous() and out.dtype == dtype and tuple(out.shape) == tuple(shape), (tuple(out.shape), shape, out.dtype)
    return out


def conv_in_add(z, wk, bias, R, Cout, cond=None, addend=None, out=None):
    """z [zB, Cz, H, W] fp32 / fp16, wk [9 * Cin, Cout] fp32, cond [cond_rows, Cc, H, W] fp16, addend [add_rows, H+2, W+2, Cout] fp16"""
    zB, Cz, H, W = z.shape
    o = empty_pn(R, H, W, Cout) if out is None else _dst(out, (R, H + 2, W + 2, Cout), torch.float16)
    check(lib().cfgpp_op_conv_in_add(P(z), int(z.dtype == torch.float16), P(cond), 0 if cond is None else cond.shape[0],
                                     0 if cond is None else cond.shape[1], P(addend), 0 if addend is None else addend.shape[0], P(o), P(wk),
                                     P(bias), R, zB, Cz, H, W, Cout, stream()), "cfgpp_op_conv_in_add")
    return o


def conv_in_ex(z, wk, bias, R, Cout, pre_w=None, pre_b=None, in_scale=1.0, out=None):
    zB, Cz, H, W = z.shape
    o = empty_pn(R, H, W, Cout) if out is None else _dst(out, (R, H + 2, W + 2, Cout), torch.float16)
    check(lib().cfgpp_op_conv_in_ex(P(z), int(z.dtype == torch.float16), P(o), P(wk), P(bias), R, zB, Cz, H, W, Cout, P(pre_w), P(pre_b),
                                    float(in_scale), stream()), "cfgpp_op_conv_in_ex")
    return o


def conv_out_ex(x_pn, wk, bias, out_half=True, post_scale=1.0, post_shift=0.0, clamp01=0, out=None):
    """x_pn halo-padded NHWC fp16, wk [Cout, 9, C] fp16 -> NCHW [R, Cout, H, W]"""
    R, Hp, Wp, C = x_pn.shape
    H, W, Co = Hp - 2, Wp - 2, wk.shape[0]
    o = _dst(out, (R, Co, H, W), torch.float16 if out_half else torch.float32)
    check(lib().cfgpp_op_conv_out_ex(P(x_pn), P(o), int(out_half), P(wk), P(bias), R, H, W, C, Co, float(post_scale), float(post_shift),
                                     int(clamp01), stream()), "cfgpp_op_conv_out_ex")
    return o


def conv_out_last_launch():
    """(kernel 0 wave per pixel / 1 tiled, CO, out_is_half, workgroups) of the last conv_out call (cfgpp_debug.h)"""
    return _last_launch("cfgpp_conv_out_last_launch", 4)


def sinusoid_ex(vals, dim, count=None, scalar=0.0, out_ld=None, out_off=0, out=None):
    """vals: device fp32 tensor or None (the scalar form: `count` rows of `scalar`); out [count, out_ld] fp32"""
    count = vals.numel() if count is None else count
    ld = dim if out_ld is None else out_ld
    o = _dst(out, (count, ld), torch.float32)
    check(lib().cfgpp_op_sinusoid(P(vals), float(scalar), P(o), count, dim, ld, out_off, stream()), "cfgpp_op_sinusoid")
    return o


def skinny_ex(x, ldx, w, bias, M, addend=None, add_ld=0, ldo=None, silu_in=False, silu_out=False, out=None):
    """x: fp32 device tensor read as rows of stride ldx (0: one row), w [N, K] fp16; out [M, ldo] fp32"""
    N, K = w.shape
    ldo = N if ldo is None else ldo
    o = _dst(out, (M, ldo), torch.float32)
    check(lib().cfgpp_op_skinny_gemm(P(x), ldx, P(w), P(bias), P(addend), add_ld, P(o), ldo, M, N, K, int(silu_in), int(silu_out), stream()),
          "cfgpp_op_skinny_gemm")
    return o


def f16_to_f32_rows(x, out_ld=None, out_off=0, out=None):
    rows, cols = x.shape
    ld = cols if out_ld is None else out_ld
    o = _dst(out, (rows, ld), torch.float32)
    check(lib().cfgpp_op_f16_to_f32_rows(P(x), P(o), rows, cols, ld, out_off, stream()), "cfgpp_op_f16_to_f32_rows")
    return o


def fanout_rows(bufs, h, row_elems=None, ptrs=None):
    """rows [0, h) of every fp16 device tensor in bufs ([>= 2h, row_elems]) copied onto rows [h, 2h), in place, one launch"""
    import ctypes
    n = len(bufs)
    p = (ctypes.c_void_p * n)(*(ptrs if ptrs is not None else [b.data_ptr() for b in bufs]))
    e = (ctypes.c_long * n)(*(row_elems if row_elems is not None else [b.shape[1] for b in bufs]))
    check(lib().cfgpp_op_fanout_rows(p, e, n, h, stream()), "cfgpp_op_fanout_rows")
    return bufs


def vae_posterior(conv_out, qw, qb, noise, scale, moments=True, out=None, out_moments=None):
    """conv_out [B, 8, HW] fp32 -> (z [B, 4, HW], moments [B, 8, HW] or None)"""
    B, _, HW = conv_out.shape
    z = _dst(out, (B, 4, HW), torch.float32)
    m = _dst(out_moments, (B, 8, HW), torch.float32) if moments else None
    check(lib().cfgpp_op_vae_posterior(P(conv_out), P(qw), P(qb), P(noise), P(z), P(m), B, HW, float(scale), stream()), "cfgpp_op_vae_posterior")
    return z, m


# ---- the towers' small kernels (csrc/text.hip, csrc/vision.hip, csrc/resampler.hip, act_inplace of csrc/small_kernels.hip) and the
# ControlNet kernels, every argument of the C entry points; destinations are the caller's (guarded) tensors -----------------------------
def text_embed(ids, tok, pos, x, B, H, vocab):
    """ids: device int32 [B, 77]; tok [vocab, H], pos [77, H], x [B * 77, H] fp16"""
    check(lib().cfgpp_op_text_embed(P(ids), P(tok), P(pos), P(x), B, H, vocab, stream()), "cfgpp_op_text_embed")
    return x


def text_attention(qkv, out, B, heads, H):
    check(lib().cfgpp_op_text_attention(P(qkv), P(out), B, heads, H, stream()), "cfgpp_op_text_attention")
    return out


def text_pool(h, eos, out, B, H):
    """h [B, 77, H] fp16, eos: device int32 [B], out [B, H] fp32"""
    check(lib().cfgpp_op_text_pool(P(h), P(eos), P(out), B, H, stream()), "cfgpp_op_text_pool")
    return out


def act_inplace(x, n, act):
    check(lib().cfgpp_op_act_inplace(P(x), n, act, stream()), "cfgpp_op_act_inplace")
    return x


def gelu_inplace(x, n):
    check(lib().cfgpp_op_gelu_inplace(P(x), n, stream()), "cfgpp_op_gelu_inplace")
    return x


def vit_assemble(patch, cls, pos, x, N, T, H):
    check(lib().cfgpp_op_vit_assemble(P(patch), P(cls), P(pos), P(x), N, T, H, stream()), "cfgpp_op_vit_assemble")
    return x


def vit_cls_rows(x, dst, N, T, H):
    check(lib().cfgpp_op_vit_cls_rows(P(x), P(dst), N, T, H, stream()), "cfgpp_op_vit_cls_rows")
    return dst


def broadcast_rows(src, dst, n, rows):
    check(lib().cfgpp_op_broadcast_rows(P(src), P(dst), n, rows, stream()), "cfgpp_op_broadcast_rows")
    return dst


def cn_conv3x3(x, in_kind, out, out_pad, wk, bias, R, Ci, Co, Hi, Wi, stride, silu):
    check(lib().cfgpp_op_cn_conv3x3(P(x), in_kind, P(out), out_pad, P(wk), P(bias), R, Ci, Co, Hi, Wi, stride, silu, stream()), "cfgpp_op_cn_conv3x3")
    return out


def residual_nchw(src, out, rows, H, W, C, scale):
    check(lib().cfgpp_op_residual_nchw(P(src), P(out), rows, H, W, C, float(scale), stream()), "cfgpp_op_residual_nchw")
    return out
