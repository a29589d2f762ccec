"""-m gpu: the soft regional cross-attention kernel (csrc/attn_kernel.hip: attn_region_soft_kernel, record: kernel 9) through
cfgpp_op_attention_region_soft against the fp64 reference of tests/attn_region_soft_cases.py (sum_r w_r softmax(q K_r) V_r, every
softmax over its region's own 77 keys) with the per-row bound of tests/attn_cases.py, by the method of
tests/test_gpu_attention_region.py: the dispatch record asserted, the output written into a NaN-filled buffer between guard rows,
a second launch bit-identical.  Regions no row weighs hold keys that would dominate and +-100 values, the slots behind the context
hold +-100; tests/test_attention_region_soft_cases_cpu.py shows the faults the bound catches.  Kernel / E_model ratios are recorded
per case ("attention_case" lines, groups soft_*)."""
import pytest
import torch

import attn_cases as A
import attn_region_soft_cases as SC
from test_gpu_attention import guarded, guards_intact
from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu
ids = dict(ids=lambda c: c.id)


def make_buffers(c, bld):
    """head-major Q / K / V^T buffers of case c with c.k_pad key slots and the fp32 weight buffer [map_rows][R][q_pad]"""
    import hip_ops as H
    q, k, v = SC.full_inputs(c, bld)
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
    w_dev = SC.weight_buffer(c, q_pad, bld["wmap"]).to(H.DEV).contiguous()
    return hq, hk, hvt, w_dev, q_pad, k_pad


def attention_soft(hq, hk, hvt, w_dev, c, q_pad, k_pad, out, n_regions=None, map_rows=None, null_w=False, d=None):
    import hip_ops as H
    H.check(H.lib().cfgpp_op_attention_region_soft(H.P(hq), H.P(hk), H.P(hvt), H.P(out), c.B, c.h, c.d if d is None else d, c.Nq,
                                                   c.R if n_regions is None else n_regions, None if null_w else H.P(w_dev),
                                                   c.map_rows if map_rows is None else map_rows, q_pad, k_pad, H.stream()),
            "cfgpp_op_attention_region_soft")
    return out


def launch(c, bld):
    """two guarded launches of case c -> (output of the first, problems found by the harness)"""
    import hip_ops as H
    hq, hk, hvt, w_dev, qp, kp = make_buffers(c, bld)
    outs, paths = [], []
    for _ in range(2):
        buf, o = guarded(c.B, c.Nq, c.h * c.d)
        attention_soft(hq, hk, hvt, w_dev, c, qp, kp, o)
        paths.append(H.attention_last_launch())
        torch.cuda.synchronize()
        outs.append((buf, o))
    want = (9, c.d16, c.ones, 0)
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
    bld, ref, e_model, bound = SC.reference(c)
    got, problems = launch(c, bld)
    err, rel = A.max_row_err(got, ref, c.d), A.rel_l2(got, ref)
    record("attention_case", group=group, case=c.id, grid=c.grid, e_model=e_model, max_row_err=err,
           ratio=(err / e_model if e_model else None), rel_l2=rel, problems=problems)
    print(f"{group} {c.id}: E_model {e_model:.3e} kernel {err:.3e} bound {bound:.3e} rel_l2 {rel:.3e} {problems}")
    assert not problems, (c.id, problems)
    assert err <= bound, f"{c.id}: max row error {err:.3e} > {A.FACTOR:g} x E_model = {bound:.3e}"


@pytest.mark.parametrize("c", SC.HOT, **ids)
def test_one_hot_weights(c):
    """every row in one region: the other regions are never evaluated (they hold dominating keys and +-100 values)"""
    check_case(c, "soft_hot")


@pytest.mark.parametrize("c", SC.MIXED, **ids)
def test_blends(c):
    """uniform 1 / R, a ramp inside a wave slab and across the block edge, a region weighed by one lane, random weights"""
    check_case(c, "soft_mixed")


@pytest.mark.parametrize("c", SC.SKIP, **ids)
def test_region_nobody_weighs_and_three_blocks(c):
    assert c.grid > 8 and c.grid % 8 != 0
    check_case(c, "soft_skip")


@pytest.mark.parametrize("c", SC.BATCH, **ids)
def test_ragged_batch_with_one_map_and_with_a_map_per_row(c):
    check_case(c, "soft_batch")


@pytest.mark.parametrize("c", [c for c in SC.HOT if c.Nq == 100 and c.R == 3 and c.d in (40, 64, 80, 160)], **ids)
def test_one_hot_weights_against_the_hard_region_op(c):
    """the same buffers through cfgpp_op_attention_region with the map the one-hot weights name: both inside their bound of the
    same fp64 reference"""
    need_gpu()
    import hip_ops as H
    bld, ref, e_model, bound = SC.reference(c)
    hq, hk, hvt, w_dev, qp, kp = make_buffers(c, bld)
    _, soft = guarded(c.B, c.Nq, c.h * c.d)
    attention_soft(hq, hk, hvt, w_dev, c, qp, kp, soft)
    ids_dev = w_dev.argmax(1).to(torch.uint8).contiguous()                     # [map_rows][q_pad]; pads (all-zero columns) -> 0
    _, hard = guarded(c.B, c.Nq, c.h * c.d)
    H.check(H.lib().cfgpp_op_attention_region(H.P(hq), H.P(hk), H.P(hvt), H.P(hard), c.B, c.h, c.d, c.Nq, c.R, H.P(ids_dev), c.map_rows,
                                              qp, kp, H.stream()), "cfgpp_op_attention_region")
    assert H.attention_last_launch()[0] in (7, 8)
    torch.cuda.synchronize()
    e_soft, e_hard = A.max_row_err(soft.cpu(), ref, c.d), A.max_row_err(hard.cpu(), ref, c.d)
    print(f"{c.id}: soft {e_soft:.3e} hard {e_hard:.3e} bound {bound:.3e}")
    assert e_soft <= bound and e_hard <= bound


@pytest.mark.parametrize("c", [c for c in SC.MIXED if c.pattern == "random" and c.R == 4 and c.d in (40, 160)], **ids)
def test_identical_regions_equal_the_plain_cross_attention(c):
    """every region holding the same 77 keys: any weights give the plain 77-key cross-attention, within the bound of that case"""
    need_gpu()
    import hip_ops as H
    bld = SC.build(c)
    hq, hk, hvt, w_dev, qp, kp = make_buffers(c, bld)
    pos = H.vt_pos(kp).to(H.DEV)
    for r in range(1, c.R):
        hk[:, SC.TOK * r: SC.TOK * (r + 1)] = hk[:, :SC.TOK]
        hvt[:, :, pos[SC.TOK * r: SC.TOK * (r + 1)]] = hvt[:, :, pos[:SC.TOK]]
    _, o = guarded(c.B, c.Nq, c.h * c.d)
    attention_soft(hq, hk, hvt, w_dev, c, qp, kp, o)
    plain = H.attention(hq, hk, hvt, c.B, c.h, c.d, c.Nq, SC.TOK, qp, kp)
    torch.cuda.synchronize()
    q, k, v = SC.full_inputs(c, bld)
    ref = A.ref64(q, k[:, :, :SC.TOK], v[:, :, :SC.TOK])
    e_model = A.max_row_err(A.model(q, k[:, :, :SC.TOK], v[:, :, :SC.TOK]), ref, c.d)
    assert A.max_row_err(o.cpu(), ref, c.d) <= A.FACTOR * e_model and A.max_row_err(plain.cpu(), ref, c.d) <= A.FACTOR * e_model


# ---- refusals: by name, nothing launched ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,match", [(dict(n_regions=1), "n_regions=1"), (dict(n_regions=5), "n_regions=5"), (dict(map_rows=3), "map_rows=3"),
                                      (dict(null_w=True), "null weights"), (dict(n_regions=4), "k_tok_pad=192")])
def test_refusals(kw, match):
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    c = next(c for c in SC.BATCH if c.R == 2 and c.map_rows == 2 and c.d == 64)
    assert c.k_pad == 192
    bld = SC.build(c)
    hq, hk, hvt, w_dev, qp, kp = make_buffers(c, bld)
    buf, o = guarded(c.B, c.Nq, c.h * c.d)
    with pytest.raises(CfgppError, match=match):
        attention_soft(hq, hk, hvt, w_dev, c, qp, kp, o, **kw)
    torch.cuda.synchronize()
    assert H.attention_last_launch() == (0, 0, 0, 0)
    assert bool(torch.isnan(o).all()) and guards_intact(buf, c.h * c.d)


@pytest.mark.parametrize("d", SC.HEAD_DIMS_REFUSED)
def test_head_dims_without_an_instance_are_refused(d):
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    c = SC.SCase(1, 2, 100, d, 2, "uniform")
    dp, qp, kp = H.round_up(d, 32), 128, c.k_pad
    hq = torch.zeros((2, qp, dp), dtype=torch.float16, device=H.DEV)
    hk = torch.zeros((2, kp, dp), dtype=torch.float16, device=H.DEV)
    hvt = torch.zeros((2, dp, kp), dtype=torch.float16, device=H.DEV)
    w_dev = SC.weight_buffer(c, qp).to(H.DEV)
    buf, o = guarded(c.B, c.Nq, c.h * d)
    with pytest.raises(CfgppError, match=f"no kernel instance for head dim {d}"):
        attention_soft(hq, hk, hvt, w_dev, c, qp, kp, o)
    torch.cuda.synchronize()
    assert H.attention_last_launch() == (0, 0, 0, 0)
    assert bool(torch.isnan(o).all()) and guards_intact(buf, c.h * d)
