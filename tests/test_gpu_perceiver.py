"""-m gpu: cfgpp_op_perceiver_attention (the IP-Adapter Plus Resampler's attention, csrc/resampler.hip) against the fp64 reference
of tests/perceiver_cases.py, with the harness of tests/test_gpu_attention.py: NaN-filled output between sentinel guard rows, a
second launch bit-identical, and a per-row bound of attn_cases.FACTOR x the error of the CPU model of the kernel's rounding
points on the same inputs.  tests/test_perceiver_cases_cpu.py shows which faults that bound catches."""
import pytest
import torch

import attn_cases as A
import perceiver_cases as P
from test_gpu_attention import guarded, guards_intact
from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu

ids = dict(ids=lambda c: c.id)


@pytest.fixture(autouse=True)
def _one_cpu_thread():
    """the references are many tiny fp64 matmuls: torch's intra-op thread pool costs more than it gives there"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def perceiver(q, kvx, kvl, out, rows, heads, nq, S):
    import hip_ops as H
    H.check(H.lib().cfgpp_op_perceiver_attention(H.P(q), H.P(kvx), H.P(kvl), H.P(out), rows, heads, nq, S, H.stream()),
            "cfgpp_op_perceiver_attention")
    return out


def launch(c, ins):
    import hip_ops as H
    q, kvx, kvl = (x.to(H.DEV, torch.float16).contiguous() for x in P.to_kernel_layout(c, *ins))
    outs = []
    for _ in range(2):
        buf, o = guarded(c.rows, c.nq, c.heads * P.D)
        perceiver(q, kvx, kvl, o, c.rows, c.heads, c.nq, c.S)
        torch.cuda.synchronize()
        outs.append((buf, o))
    problems = []
    if not all(guards_intact(buf, c.heads * P.D) for buf, _ in outs):
        problems.append("guard rows written")
    if not bool(torch.isfinite(outs[0][1]).all()):
        problems.append(f"{int((~torch.isfinite(outs[0][1])).sum())} output elements not finite (unwritten or NaN)")
    if not torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16)):
        problems.append("second launch differs")
    return outs[0][1].cpu(), problems


def check_case(c, group):
    need_gpu()
    ins, ref, e_model, bound = P.reference(c)
    got, problems = launch(c, ins)
    err = A.max_row_err(got, ref, P.D)
    record("perceiver_case", group=group, case=c.id, tiles=c.tiles, e_model=e_model, max_row_err=err,
           ratio=(err / e_model if e_model else None), problems=problems)
    print(f"{group} {c.id}: E_model {e_model:.3e} kernel {err:.3e} bound {bound:.3e} {problems}")
    assert not problems, (c.id, problems)
    assert err <= bound, f"{c.id}: max row error {err:.3e} > {A.FACTOR:g} x E_model = {bound:.3e}"


@pytest.mark.parametrize("c", P.SMALL, **ids)
def test_one_and_two_image_keys(c):
    check_case(c, "perceiver_small")


@pytest.mark.parametrize("c", P.TILE_EDGES, **ids)
def test_key_tile_edges_in_both_sources(c):
    """S + n_q around one and two 32-key tiles, the boundary in the image keys, between the sources and in the latent keys"""
    check_case(c, "perceiver_tile_edges")


@pytest.mark.parametrize("c", P.REAL, **ids)
def test_tower_sequence_lengths(c):
    """S = 257 (ViT-H/14, ViT-bigG/14), 577 (ViT-L/14@336) and 1024, the longest supported"""
    check_case(c, "perceiver_real")


@pytest.mark.parametrize("nq,S,msg", [(0, 5, "n_q=0"), (33, 5, "n_q=33"), (4, 0, "S=0"), (4, 1025, "S=1025")])
def test_refusals_launch_nothing(nq, S, msg):
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    rows, heads = 1, 2
    q = torch.zeros((rows, 32, heads * 64), dtype=torch.float16, device=H.DEV)
    kvx = torch.zeros((rows, 1025, 2 * heads * 64), dtype=torch.float16, device=H.DEV)
    kvl = torch.zeros((rows, 33, 2 * heads * 64), dtype=torch.float16, device=H.DEV)
    buf, o = guarded(rows, 32, heads * 64)
    with pytest.raises(CfgppError, match=msg):
        perceiver(q, kvx, kvl, o, rows, heads, nq, S)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and guards_intact(buf, heads * 64)
