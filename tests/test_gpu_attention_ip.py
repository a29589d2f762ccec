"""-m gpu: cfgpp_op_attention_ip (decoupled cross-attention of an IP-Adapter, csrc/attn_kernel.hip) against the fp64 two-softmax
reference of tests/attn_ip_cases.py, with the harness of tests/test_gpu_attention.py: NaN-filled output between sentinel guard
rows, a second launch bit-identical, the dispatch the case is named after (cfgpp_attention_last_launch: 4 = xattn64_kernel IP
form, one launch; 5 = text pass + attn_ip_add_kernel) and a per-row bound of attn_cases.FACTOR x the error of the CPU model of the
kernels' rounding points on the same inputs.  tests/test_ip_adapter_cpu.py shows which faults that bound catches."""
import ctypes

import pytest
import torch

import attn_cases as A
import attn_ip_cases as I
from test_gpu_attention import guarded, guards_intact
from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu

ids = dict(ids=lambda c: c.id)
K_PAD = 128


@pytest.fixture(autouse=True)
def _one_cpu_thread():
    """the references are many tiny fp64 matmuls: torch's intra-op thread pool costs ~100x its benefit there"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def make_heads_ip(q, k, v, ki, vi, k_pad=K_PAD, poison_pads=False):
    """-> head-major device buffers with the text keys in slots [0, nk_text) and the image keys in [96, 96 + n_img) of k_pad slots"""
    import hip_ops as H
    B, h, Nq, d = q.shape
    nkt, ni = k.shape[2], ki.shape[2]
    dp = H.round_up(d, 32)
    q_pad = H.round_up(Nq, 128)
    hq = torch.zeros((B * h, q_pad, dp), dtype=torch.float16, device=H.DEV)
    hk = torch.zeros((B * h, k_pad, dp), dtype=torch.float16, device=H.DEV)
    hvt = torch.zeros((B * h, dp, k_pad), dtype=torch.float16, device=H.DEV)
    hq[:, :Nq, :d] = q.reshape(B * h, Nq, d).to(H.DEV, torch.float16)
    hk[:, :nkt, :d] = k.reshape(B * h, nkt, d).to(H.DEV, torch.float16)
    hk[:, I.IMG_SLOT:I.IMG_SLOT + ni, :d] = ki.reshape(B * h, ni, d).to(H.DEV, torch.float16)
    hvt[:, :d, H.vt_pos(nkt).to(H.DEV)] = v.reshape(B * h, nkt, d).transpose(1, 2).to(H.DEV, torch.float16)
    hvt[:, :d, (I.IMG_SLOT + H.vt_pos(ni)).to(H.DEV)] = vi.reshape(B * h, ni, d).transpose(1, 2).to(H.DEV, torch.float16)
    H.check(H.lib().cfgpp_op_attention_prepare_vt(H.P(hvt), B * h, d, k_pad, H.stream()), "cfgpp_op_attention_prepare_vt")
    return hq, hk, hvt, q_pad, k_pad


def attention_ip(hq, hk, hvt, B, h, d, nq, nk_text, n_img, scale, q_pad, k_pad, out):
    import hip_ops as H
    H.check(H.lib().cfgpp_op_attention_ip(H.P(hq), H.P(hk), H.P(hvt), H.P(out), B, h, d, nq, nk_text, n_img, ctypes.c_float(scale),
                                          q_pad, k_pad, H.stream()), "cfgpp_op_attention_ip")
    return out


def launch(c, ins):
    import hip_ops as H
    hq, hk, hvt, qp, kp = make_heads_ip(*ins)
    outs, paths = [], []
    for _ in range(2):
        buf, o = guarded(c.B, c.Nq, c.h * c.d)
        attention_ip(hq, hk, hvt, c.B, c.h, c.d, c.Nq, c.nk_text, c.n_img, c.scale, qp, kp, o)
        paths.append(H.attention_last_launch())
        torch.cuda.synchronize()
        outs.append((buf, o))
    problems = []
    want = (c.kernel, c.d16, c.ones, c.xqb)
    if paths[0] != want or paths[1] != want:
        problems.append(f"dispatched {paths[0]} (kernel, D16, ONES, xqb), the case is for {want}")
    if not all(guards_intact(buf, c.h * c.d) for buf, _ in outs):
        problems.append("guard rows written")
    if not bool(torch.isfinite(outs[0][1]).all()):
        problems.append(f"{int((~torch.isfinite(outs[0][1])).sum())} output elements not finite (unwritten or NaN)")
    if not torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16)):
        problems.append("second launch differs")
    return outs[0][1].cpu(), problems


def check_case(c, group):
    need_gpu()
    ins, info, ref, e_model, bound = I.reference_ip(c)
    got, problems = launch(c, ins)
    err, rel = A.max_row_err(got, ref, c.d), A.rel_l2(got, ref)
    record("attention_ip_case", group=group, case=c.id, grid=c.grid, e_model=e_model, max_row_err=err,
           ratio=(err / e_model if e_model else None), rel_l2=rel, problems=problems)
    print(f"{group} {c.id}: E_model {e_model:.3e} kernel {err:.3e} bound {bound:.3e} rel_l2 {rel:.3e} {problems}")
    assert not problems, (c.id, problems)
    assert err <= bound, f"{c.id}: max row error {err:.3e} > {A.FACTOR:g} x E_model = {bound:.3e}"


@pytest.mark.parametrize("c", I.FUSED_SMALL, **ids)
def test_fused_one_workgroup_per_block(c):
    """xattn64_kernel IP form: 1 .. 96 text keys and 1 .. 32 image keys, every class of mask position of both softmaxes"""
    check_case(c, "ip_fused_small")


@pytest.mark.parametrize("c", I.FUSED_MULTIBLOCK, **ids)
def test_fused_walks_several_query_blocks(c):
    """xqb = 2 (ragged last block) and 8 query blocks per workgroup"""
    check_case(c, "ip_fused_multiblock")


@pytest.mark.parametrize("c", I.FUSED_REMAP, **ids)
def test_fused_xcd_remap_remainder(c):
    assert c.grid > 8 and c.grid % 8 != 0
    check_case(c, "ip_fused_remap")


@pytest.mark.parametrize("c", I.TWO_PASS, **ids)
def test_two_pass_head_dims(c):
    """d = 32, 80, 160: the text pass of the flash kernel, then attn_ip_add_kernel"""
    check_case(c, "ip_two_pass")


@pytest.mark.parametrize("d", (64, 40, 80))
def test_scale_zero_is_the_text_attention(d):
    """ip_scale = 0 gives the bits of cfgpp_op_attention over the text keys"""
    need_gpu()
    import hip_ops as H
    c = I.IPCase(1, 2, 100, 77, 16, d, scale=0.0, seed=8100 + d)
    ins = I.make_ip_inputs(c)[:5]
    hq, hk, hvt, qp, kp = make_heads_ip(*ins)
    buf, o = guarded(c.B, c.Nq, c.h * d)
    attention_ip(hq, hk, hvt, c.B, c.h, d, c.Nq, 77, 16, 0.0, qp, kp, o)
    want = H.attention(hq, hk, hvt, c.B, c.h, d, c.Nq, 77, qp, kp)
    torch.cuda.synchronize()
    assert guards_intact(buf, c.h * d)
    assert torch.equal(o.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("nk_text,n_img,k_pad,msg", [(97, 4, 128, "nk_text=97"), (77, 33, 128, "n_img=33"), (77, 0, 128, "n_img=0"),
                                                     (33, 4, 64, "k_tok_pad=64")])
def test_refusals_launch_nothing(nk_text, n_img, k_pad, msg):
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    d, B, h, Nq = 64, 1, 2, 100
    hq = torch.zeros((B * h, 128, 64), dtype=torch.float16, device=H.DEV)
    hk = torch.zeros((B * h, 128, 64), dtype=torch.float16, device=H.DEV)
    hvt = torch.zeros((B * h, 64, 128), dtype=torch.float16, device=H.DEV)
    buf, o = guarded(B, Nq, h * d)
    with pytest.raises(CfgppError, match=msg):
        attention_ip(hq, hk, hvt, B, h, d, Nq, nk_text, n_img, 1.0, 128, k_pad, o)
    torch.cuda.synchronize()
    assert H.attention_last_launch() == (0, 0, 0, 0)
    assert bool(torch.isnan(o).all()) and guards_intact(buf, h * d)


@pytest.mark.parametrize("d,slot0,n", [(40, 96, 32), (56, 96, 32), (64, 96, 32), (80, 96, 32), (32, 96, 8), (160, 64, 64)])
def test_clear_slots_zeroes_the_image_slots_and_nothing_else(d, slot0, n):
    """cfgpp_op_attention_clear_slots: K slots [slot0, slot0 + n) (all dp columns) and columns [slot0, slot0 + n) of rows < d of
    V^T become zero; every other element - the text slots, the ones row d of V^T and the pad rows above it, the guard heads before
    and after - keeps its bits"""
    need_gpu()
    import hip_ops as H
    BH, dp = 5, H.round_up(d, 32)
    g = torch.Generator().manual_seed(d + n)
    k = (torch.rand((BH + 2, K_PAD, dp), generator=g) + 1).half().to(H.DEV)         # nonzero everywhere; heads 0 and BH + 1 are guards
    vt = (torch.rand((BH + 2, dp, K_PAD), generator=g) + 1).half().to(H.DEV)
    k0, vt0 = k.clone(), vt.clone()
    H.check(H.lib().cfgpp_op_attention_clear_slots(H.P(k[1:]), H.P(vt[1:]), BH, d, K_PAD, slot0, n, H.stream()), "cfgpp_op_attention_clear_slots")
    torch.cuda.synchronize()
    wk, wvt = k0.clone(), vt0.clone()
    wk[1:BH + 1, slot0:slot0 + n, :] = 0
    wvt[1:BH + 1, :d, slot0:slot0 + n] = 0
    assert torch.equal(k.view(torch.int16), wk.view(torch.int16))
    assert torch.equal(vt.view(torch.int16), wvt.view(torch.int16))
