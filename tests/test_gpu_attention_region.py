"""-m gpu: the regional cross-attention kernels (csrc/attn_kernel.hip) through cfgpp_op_attention_region - xattn64_region_kernel
(record: kernel 7) at head dims padded to 64, attn_region_rows_kernel (kernel 8) at every other head dim and under the A/B
switches - against the fp64 reference of tests/attn_region_cases.py (a row's reference is attn_cases.ref64 over the row's own 77
keys) with the per-row bound of tests/attn_cases.py, by the method of tests/test_gpu_attention_long.py: the dispatch record
asserted, the output written into a NaN-filled buffer between guard rows, a second launch bit-identical.  Foreign regions hold
keys that would dominate a row, and the slots behind the context hold +-100; tests/test_attention_region_cases_cpu.py shows the
faults the bound catches.  Kernel / E_model ratios are recorded per case ("attention_case" lines, groups region_*)."""
import pytest
import torch

import attn_cases as A
import attn_region_cases as RC
from test_gpu_attention import guarded, guards_intact
from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu
ids = dict(ids=lambda c: c.id)


def make_buffers(c, bld):
    """head-major Q / K / V^T buffers of case c with c.k_pad key slots (junk behind the context) and the uint8 region map"""
    import hip_ops as H
    q, k, v = RC.full_inputs(c, bld)
    BH, d, dp = c.B * c.h, c.d, H.round_up(c.d, 32)
    q_pad, k_pad = H.round_up(c.Nq, 128), c.k_pad
    hq = torch.zeros((BH, q_pad, dp), dtype=torch.float16, device=H.DEV)
    hk = torch.zeros((BH, k_pad, dp), dtype=torch.float16, device=H.DEV)
    hvt = torch.zeros((BH, dp, k_pad), dtype=torch.float16, device=H.DEV)
    hq[:, :c.Nq, :d] = q.reshape(BH, c.Nq, d).to(H.DEV, torch.float16)
    hk[:, :, :d] = k.reshape(BH, k_pad, d).to(H.DEV, torch.float16)
    pos = H.vt_pos(k_pad).to(H.DEV)
    hvt[:, :d, pos] = v.reshape(BH, k_pad, d).transpose(1, 2).to(H.DEV, torch.float16)
    H.check(H.lib().cfgpp_op_attention_prepare_vt(H.P(hvt), BH, d, k_pad, H.stream()), "cfgpp_op_attention_prepare_vt")
    ids_dev = RC.ids_buffer(c, q_pad).to(H.DEV)
    return hq, hk, hvt, ids_dev, q_pad, k_pad


def attention_region(hq, hk, hvt, ids_dev, c, q_pad, k_pad, out, n_regions=None, map_rows=None, null_ids=False):
    import hip_ops as H
    H.check(H.lib().cfgpp_op_attention_region(H.P(hq), H.P(hk), H.P(hvt), H.P(out), c.B, c.h, c.d, c.Nq, c.R if n_regions is None else n_regions,
                                              None if null_ids else H.P(ids_dev), c.map_rows if map_rows is None else map_rows, q_pad, k_pad,
                                              H.stream()), "cfgpp_op_attention_region")
    return out


def launch(c, bld):
    """two guarded launches of case c under its switches -> (output of the first, problems found by the harness)"""
    import hip_ops as H
    hq, hk, hvt, ids_dev, qp, kp = make_buffers(c, bld)
    lib = H.lib()
    lib.cfgpp_attention_set_dma(c.dma)
    lib.cfgpp_attention_set_cross(c.cross)
    try:
        outs, paths = [], []
        for _ in range(2):
            buf, o = guarded(c.B, c.Nq, c.h * c.d)
            attention_region(hq, hk, hvt, ids_dev, c, qp, kp, o)
            paths.append(H.attention_last_launch())
            torch.cuda.synchronize()
            outs.append((buf, o))
    finally:
        lib.cfgpp_attention_set_dma(1)
        lib.cfgpp_attention_set_cross(1)
    want = (c.kernel, c.d16, c.ones, c.xqb)
    problems = []
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
    bld, ref, e_model, bound = RC.reference(c)
    got, problems = launch(c, bld)
    err, rel = A.max_row_err(got, ref, c.d), A.rel_l2(got, ref)
    record("attention_case", group=group, case=c.id, grid=c.grid, e_model=e_model, max_row_err=err,
           ratio=(err / e_model if e_model else None), rel_l2=rel, problems=problems)
    print(f"{group} {c.id}: E_model {e_model:.3e} kernel {err:.3e} bound {bound:.3e} rel_l2 {rel:.3e} {problems}")
    assert not problems, (c.id, problems)
    assert err <= bound, f"{c.id}: max row error {err:.3e} > {A.FACTOR:g} x E_model = {bound:.3e}"
    return got          # (rel-L2 is recorded, not bounded: on the two rows of an Nq = 1 case it is the model's own row error)


@pytest.mark.parametrize("c", RC.ALL_IN_ONE, **ids)
def test_every_row_in_one_region(c):
    """r = R - 1: no own key in the first resident tile(s); r = 0: only foreign tiles after the own ones"""
    check_case(c, "region_all_in_one")


@pytest.mark.parametrize("c", RC.MIXED, **ids)
def test_mixed_maps(c):
    """the region alternating per query, a border inside a 32-row wave slab, a border at the 128-query block edge"""
    check_case(c, "region_mixed")


@pytest.mark.parametrize("c", RC.BATCH, **ids)
def test_ragged_batch_with_one_map_and_with_a_map_per_row(c):
    check_case(c, "region_batch")


@pytest.mark.parametrize("c", RC.MULTIBLOCK, **ids)
def test_walks_several_query_blocks(c):
    check_case(c, "region_multiblock")


@pytest.mark.parametrize("c", RC.REMAP, **ids)
def test_xcd_remap_remainder_branch(c):
    assert c.grid > 8 and c.grid % 8 != 0
    check_case(c, "region_remap")


@pytest.mark.parametrize("c", RC.SWITCHES, **ids)
def test_switches_send_dp64_to_the_row_kernel(c):
    assert c.kernel == 8 and (c.d + 31) // 32 == 2
    check_case(c, "region_switches")


def test_identical_regions_equal_the_plain_cross_attention():
    """every region holding the same 77 keys: any map gives the plain 77-key cross-attention, within the bound of that case"""
    need_gpu()
    import hip_ops as H
    c = RC.MIXED[0]
    bld = RC.build(c)
    hq, hk, hvt, ids_dev, qp, kp = make_buffers(c, bld)
    pos = H.vt_pos(kp).to(H.DEV)
    for r in range(1, c.R):
        hk[:, RC.TOK * r: RC.TOK * (r + 1)] = hk[:, :RC.TOK]
        hvt[:, :, pos[RC.TOK * r: RC.TOK * (r + 1)]] = hvt[:, :, pos[:RC.TOK]]
    _, o = guarded(c.B, c.Nq, c.h * c.d)
    attention_region(hq, hk, hvt, ids_dev, c, qp, kp, o)
    plain = H.attention(hq, hk, hvt, c.B, c.h, c.d, c.Nq, RC.TOK, qp, kp)
    torch.cuda.synchronize()
    q, k, v = RC.full_inputs(c, bld)
    ref = A.ref64(q, k[:, :, :RC.TOK], v[:, :, :RC.TOK])
    e_model = A.max_row_err(A.model(q, k[:, :, :RC.TOK], v[:, :, :RC.TOK]), ref, c.d)
    assert A.max_row_err(o.cpu(), ref, c.d) <= A.FACTOR * e_model and A.max_row_err(plain.cpu(), ref, c.d) <= A.FACTOR * e_model


# ---- refusals: by name, nothing launched ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [(dict(n_regions=1), "n_regions=1"), (dict(n_regions=5), "n_regions=5"), (dict(map_rows=3), "map_rows=3"),
                                      (dict(null_ids=True), "null ids"), (dict(n_regions=4), "k_tok_pad=192")])
def test_refusals(kw, match):
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    c = next(c for c in RC.BATCH if c.R == 2 and c.map_rows == 2 and c.d == 64)
    assert c.k_pad == 192
    bld = RC.build(c)
    hq, hk, hvt, ids_dev, qp, kp = make_buffers(c, bld)
    buf, o = guarded(c.B, c.Nq, c.h * c.d)
    with pytest.raises(CfgppError, match=match):
        attention_region(hq, hk, hvt, ids_dev, c, qp, kp, o, **kw)
    torch.cuda.synchronize()
    assert H.attention_last_launch() == (0, 0, 0, 0)
    assert bool(torch.isnan(o).all()) and guards_intact(buf, c.h * c.d)
