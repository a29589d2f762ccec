"""-m gpu: the three attention kernels of csrc/attn_kernel.hip (attn_kernel, attn64_kernel, xattn64_kernel) at the edge
shapes of every dispatch path, against the fp64 reference of tests/attn_cases.py with a per-row bound.

Every launch writes into a NaN-filled buffer with sentinel guard rows before and after the [B][Nq][heads * d] region:
the output must be finite everywhere (a row the kernel never stores stays NaN), the guards untouched (a store outside
the tensor), a second launch bit-identical, and the launcher must have taken the path the case is named after
(cfgpp_attention_last_launch).  The bound of a case is attn_cases.FACTOR x the error of the CPU model of the kernels'
rounding points on the same inputs; tests/test_attention_cases_cpu.py shows which faults that bound catches."""
import pytest
import torch

import attn_cases as A
from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu

GUARD_ROWS = 4
SENTINEL = -1234.0
ids = dict(ids=lambda c: c.id)


def guarded(B, Nq, width):
    """-> (whole buffer, the [B, Nq, width] view the kernel writes): NaN inside, SENTINEL in the guard rows around it"""
    import hip_ops as H
    g = GUARD_ROWS * width
    buf = torch.full((2 * g + B * Nq * width,), float("nan"), dtype=torch.float16, device=H.DEV)
    buf[:g] = SENTINEL
    buf[-g:] = SENTINEL
    return buf, buf[g:-g].view(B, Nq, width)


def guards_intact(buf, width):
    g = GUARD_ROWS * width
    return bool((buf[:g] == SENTINEL).all()) and bool((buf[-g:] == SENTINEL).all())


def launch(c, q, k, v):
    """two guarded launches of case c under its switches -> (output of the first, problems found by the harness)"""
    import hip_ops as H
    hq, hk, hvt, qp, kp = H.make_heads(q, k, v)
    lib = H.lib()
    lib.cfgpp_attention_set_dma(c.dma)
    lib.cfgpp_attention_set_cross(c.cross)
    try:
        outs, paths = [], []
        for _ in range(2):
            buf, o = guarded(c.B, c.Nq, c.h * c.d)
            H.attention(hq, hk, hvt, c.B, c.h, c.d, c.Nq, c.Nk, qp, kp, out=o)
            paths.append(H.attention_last_launch())
            torch.cuda.synchronize()
            outs.append((buf, o))
    finally:
        lib.cfgpp_attention_set_dma(1)
        lib.cfgpp_attention_set_cross(1)
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
    q, k, v, info, ref, e_model, bound = A.reference(c)
    got, problems = launch(c, q, k, v)
    err, rel = A.max_row_err(got, ref, c.d), A.rel_l2(got, ref)
    record("attention_case", group=group, case=c.id, grid=c.grid, e_model=e_model, max_row_err=err,
           ratio=(err / e_model if e_model else None), rel_l2=rel, problems=problems)
    print(f"{group} {c.id}: E_model {e_model:.3e} kernel {err:.3e} bound {bound:.3e} rel_l2 {rel:.3e} {problems}")
    assert not problems, (c.id, problems)
    assert err <= bound, f"{c.id}: max row error {err:.3e} > {A.FACTOR:g} x E_model = {bound:.3e}"
    assert rel < A.REL_L2_BOUND, f"{c.id}: rel-L2 {rel:.3e}"


@pytest.mark.parametrize("c", A.XATTN_MULTIBLOCK, **ids)
def test_cross_attention_walks_several_query_blocks(c):
    """xattn64_kernel with xqb = 2, 4, 8 blocks of 128 queries per workgroup and the prefetch of the next block's Q, with a
    ragged (Nq = 1000) and a full (1024) last block"""
    check_case(c, "xattn_multiblock")


@pytest.mark.parametrize("c", A.XATTN_SMALL, **ids)
def test_cross_attention_small_key_counts(c):
    """1 .. 128 keys through xattn64_kernel: one to four 32-key sub-tiles, the mask at every position of the last one"""
    check_case(c, "xattn_small")


@pytest.mark.parametrize("c", A.FLASH_PARTIAL, **ids)
def test_flash_loop_partial_last_tile(c):
    """attn64_kernel with nk > 128 and nk % 64 != 0: the key mask of the last tile (1, 16, 63 valid keys; 4097 = 64 tiles + 1)"""
    check_case(c, "flash_partial")


@pytest.mark.parametrize("c", A.HEAD_DIMS, **ids)
def test_every_head_dim_with_an_instance(c):
    """d = 8 .. 160: every (D16, DT, ONES) instance, the denominator read from accumulator register 4 * g for g = 0 .. 3"""
    check_case(c, "head_dims")


@pytest.mark.parametrize("d", A.HEAD_DIMS_REFUSED)
def test_head_dims_without_an_instance_are_refused(d):
    """d16 = 7 and 9 have no instance: the call fails with that message and launches nothing"""
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    c = A.Case(1, 2, 100, 144, d, "rand", seed=d)
    q, k, v, _ = A.make_inputs(c)
    hq, hk, hvt, qp, kp = H.make_heads(q, k, v)
    buf, o = guarded(c.B, c.Nq, c.h * d)
    with pytest.raises(CfgppError, match=f"no kernel instance for head dim {d}"):
        H.attention(hq, hk, hvt, c.B, c.h, d, c.Nq, c.Nk, qp, kp, out=o)
    torch.cuda.synchronize()
    assert H.attention_last_launch() == (0, 0, 0, 0)
    assert bool(torch.isnan(o).all()) and guards_intact(buf, c.h * d)


@pytest.mark.parametrize("c", A.SWITCH_DMA0, **ids)
def test_register_staged_kernel_at_dp64(c):
    """cfgpp_attention_set_dma(0): the dp = 64 instances of attn_kernel, partial last tile and a late dominant key"""
    check_case(c, "switch_dma0")


@pytest.mark.parametrize("c", A.SWITCH_CROSS0, **ids)
def test_flash_loop_at_cross_attention_key_counts(c):
    """cfgpp_attention_set_cross(0): 77 and 128 keys through attn64_kernel"""
    check_case(c, "switch_cross0")


@pytest.mark.parametrize("c", A.RESCALE, **ids)
def test_rereference_branch(c):
    """keys in late tiles that beat the running maximum by ~35 (log2 domain): the re-reference branch of both flash kernels"""
    check_case(c, "rescale")


@pytest.mark.parametrize("c", A.REMAP, **ids)
def test_xcd_remap_remainder_branch(c):
    """grids of 9, 13 and 23 workgroups: more than 8 and not a multiple of 8"""
    assert c.grid > 8 and c.grid % 8 != 0
    check_case(c, "remap")
