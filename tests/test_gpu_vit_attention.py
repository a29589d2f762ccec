"""-m gpu: cfgpp_op_attention_vit (the CLIP image tower's self-attention, vit_attn_kernel of csrc/vision.hip) against the fp64
reference of tests/vit_attn_cases.py, with the harness of tests/test_gpu_attention.py: NaN-filled output between sentinel guard
rows, the reported launch path asserted, a second launch bit-identical, and a per-row bound of attn_cases.FACTOR x the error of the
CPU model of the kernel's rounding points on the same inputs.  tests/test_vit_attn_cases_cpu.py shows which faults that bound catches."""
import ctypes as C

import pytest
import torch

import attn_cases as A
import vit_attn_cases as V
from test_gpu_attention import guarded, guards_intact
from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu

ids = dict(ids=lambda c: c.id)


def last_launch():
    import hip_ops as H
    out = (C.c_int * 3)()
    H.lib().cfgpp_vit_attention_last_launch(out)
    return list(out)


def vit_attention(qkv, out, rows, heads, d, T):
    import hip_ops as H
    H.check(H.lib().cfgpp_op_attention_vit(H.P(qkv), H.P(out), rows, heads, d, T, H.stream()), "cfgpp_op_attention_vit")
    return out


def launch(c, qkv):
    import hip_ops as H
    dq = qkv.to(H.DEV, torch.float16).contiguous()
    width = c.heads * c.d
    outs, paths = [], []
    for _ in range(2):
        buf, o = guarded(c.rows, c.T, width)
        vit_attention(dq, o, c.rows, c.heads, c.d, c.T)
        paths.append(last_launch())
        torch.cuda.synchronize()
        outs.append((buf, o))
    problems = []
    if not all(guards_intact(buf, width) for buf, _ in outs):
        problems.append("guard rows written")
    if not bool(torch.isfinite(outs[0][1]).all()):
        problems.append(f"{int((~torch.isfinite(outs[0][1])).sum())} output elements not finite (unwritten or NaN)")
    if not torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16)):
        problems.append("second launch differs")
    if paths != [c.launch, c.launch]:
        problems.append(f"launch {paths}, expected {c.launch}")
    return outs[0][1].cpu(), problems


@pytest.mark.parametrize("c", V.ALL_CASES, **ids)
def test_case(c):
    need_gpu()
    qkv, ref, e_model, bound = V.reference(c)
    got, problems = launch(c, qkv)
    err = A.max_row_err(got, ref, c.d)
    record("vit_attention_case", case=c.id, launch=c.launch, e_model=e_model, max_row_err=err,
           ratio=(err / e_model if e_model else None), problems=problems)
    print(f"{c.id}: E_model {e_model:.3e} kernel {err:.3e} bound {bound:.3e} {problems}")
    assert not problems, (c.id, problems)
    assert err <= bound, f"{c.id}: max row error {err:.3e} > {A.FACTOR:g} x E_model = {bound:.3e}"


@pytest.mark.parametrize("d,T,msg", [(96, 37, "head dim 96"), (112, 37, "head dim 112"), (104, 0, "T=0"), (104, 321, "T=321")])
def test_refusals_launch_nothing(d, T, msg):
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    rows, heads = 1, 2
    qkv = torch.zeros((rows, 321, 3 * heads * d), dtype=torch.float16, device=H.DEV)
    buf, o = guarded(rows, 321, heads * d)
    with pytest.raises(CfgppError, match=msg):
        vit_attention(qkv, o, rows, heads, d, T)
    torch.cuda.synchronize()
    assert last_launch() == [0, 0, 0]
    assert bool(torch.isnan(o).all()) and guards_intact(buf, heads * d)


def test_general_attention_op_still_refuses_head_dim_104():
    """cfgpp_op_attention has no instance for d = 104 and the image tower did not add one: restates the pin of
    tests/test_gpu_attention.py (attn_cases.HEAD_DIMS_REFUSED) next to the kernel that does take 104"""
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    assert 104 in A.HEAD_DIMS_REFUSED
    c = A.Case(1, 2, 37, 37, 104, "rand", seed=104)
    q, k, v, _ = A.make_inputs(c)
    hq, hk, hvt, qp, kp = H.make_heads(q, k, v)
    buf, o = guarded(c.B, c.Nq, c.h * 104)
    with pytest.raises(CfgppError, match="no kernel instance for head dim 104"):
        H.attention(hq, hk, hvt, c.B, c.h, 104, c.Nq, c.Nk, qp, kp, out=o)
    torch.cuda.synchronize()
    assert H.attention_last_launch() == (0, 0, 0, 0)
    assert bool(torch.isnan(o).all()) and guards_intact(buf, c.h * 104)
