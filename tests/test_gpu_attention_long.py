"""-m gpu: xattn64_long_kernel (csrc/attn_kernel.hip) through cfgpp_op_attention_cross - the UNet's cross-attention op at 129 ..
320 keys and head dims padded to 64 - against the fp64 reference of tests/attn_cases.py with its per-row bound, by the method
of tests/test_gpu_attention.py: the dispatch record asserted, the output written into a NaN-filled buffer between guard rows,
a second launch bit-identical.  The K / V^T buffers have attn_long_cases.K_PAD = 320 key slots, and the slots [Nk, 320) hold
+-100 (the ones row of V^T kept): what a longer, earlier context leaves behind in the engine.  The bound of a case is
attn_cases.FACTOR x the error of the CPU model on the same inputs; tests/test_attention_long_cases_cpu.py shows the faults it
catches.  Kernel / E_model ratios are recorded per case ("attention_case" lines, groups long_*).

The kernel's cases run under cfgpp_attention_set_cross_long(2) - its whole scope.  What the default (1) ships is the part of that
scope where it measured >= 3 % faster than the flash loop: test_default_dispatch_ships_the_measured_classes."""
from dataclasses import replace

import pytest
import torch

import attn_cases as A
import attn_long_cases as L
from test_gpu_attention import guarded, guards_intact
from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu
ids = dict(ids=lambda c: c.id)


@pytest.fixture(autouse=True)
def whole_scope():
    """every test of this file starts with the kernel taking its whole scope and leaves the default behind"""
    if not torch.cuda.is_available():
        yield
        return
    import hip_ops as H
    H.lib().cfgpp_attention_set_cross_long(2)
    try:
        yield
    finally:
        H.lib().cfgpp_attention_set_cross_long(1)


def make_heads_padded(c, q, k, v, k_pad=L.K_PAD):
    """hip_ops.make_heads with k_pad key slots, the slots behind the context filled with junk"""
    import hip_ops as H
    BH, d, dp = c.B * c.h, c.d, H.round_up(c.d, 32)
    q_pad = H.round_up(c.Nq, 128)
    hq = torch.zeros((BH, q_pad, dp), dtype=torch.float16, device=H.DEV)
    hk = torch.zeros((BH, k_pad, dp), dtype=torch.float16, device=H.DEV)
    hvt = torch.zeros((BH, dp, k_pad), dtype=torch.float16, device=H.DEV)
    hq[:, :c.Nq, :d] = q.reshape(BH, c.Nq, d).to(H.DEV, torch.float16)
    hk[:, :c.Nk, :d] = k.reshape(BH, c.Nk, d).to(H.DEV, torch.float16)
    pos = H.vt_pos(k_pad).to(H.DEV)
    hvt[:, :d, pos[:c.Nk]] = v.reshape(BH, c.Nk, d).transpose(1, 2).to(H.DEV, torch.float16)
    if k_pad > c.Nk:
        jk, jv = L.junk(c, k_pad - c.Nk)
        hk[:, c.Nk:, :d] = jk.to(H.DEV, torch.float16)
        hvt[:, :d, pos[c.Nk:]] = jv.transpose(1, 2).to(H.DEV, torch.float16)
    H.check(H.lib().cfgpp_op_attention_prepare_vt(H.P(hvt), BH, d, k_pad, H.stream()), "cfgpp_op_attention_prepare_vt")
    return hq, hk, hvt, q_pad, k_pad


def attention_cross(hq, hk, hvt, c, q_pad, k_pad, out, nk=None):
    import hip_ops as H
    H.check(H.lib().cfgpp_op_attention_cross(H.P(hq), H.P(hk), H.P(hvt), H.P(out), c.B, c.h, c.d, c.Nq, c.Nk if nk is None else nk,
                                             q_pad, k_pad, H.stream()), "cfgpp_op_attention_cross")
    return out


def launch(c, q, k, v, want, k_pad=L.K_PAD):
    """two guarded launches of case c -> (output of the first, problems found by the harness)"""
    import hip_ops as H
    hq, hk, hvt, qp, kp = make_heads_padded(c, q, k, v, k_pad)
    outs, paths = [], []
    for _ in range(2):
        buf, o = guarded(c.B, c.Nq, c.h * c.d)
        attention_cross(hq, hk, hvt, c, qp, kp, o)
        paths.append(H.attention_last_launch())
        torch.cuda.synchronize()
        outs.append((buf, o))
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


def check_case(c, group, want=None, k_pad=L.K_PAD):
    need_gpu()
    q, k, v, info, ref, e_model, bound = A.reference(c)
    got, problems = launch(c, q, k, v, want or (c.kernel, c.d16, c.ones, c.xqb), k_pad)
    err, rel = A.max_row_err(got, ref, c.d), A.rel_l2(got, ref)
    record("attention_case", group=group, case=c.id, grid=c.grid, e_model=e_model, max_row_err=err,
           ratio=(err / e_model if e_model else None), rel_l2=rel, problems=problems)
    print(f"{group} {c.id}: E_model {e_model:.3e} kernel {err:.3e} bound {bound:.3e} rel_l2 {rel:.3e} {problems}")
    assert not problems, (c.id, problems)
    assert err <= bound, f"{c.id}: max row error {err:.3e} > {A.FACTOR:g} x E_model = {bound:.3e}"
    assert rel < A.REL_L2_BOUND, f"{c.id}: rel-L2 {rel:.3e}"
    return got


@pytest.mark.parametrize("c", L.KEY_COUNTS, **ids)
def test_key_counts(c):
    """129 .. 320 keys: three to five resident tiles, the last sub-tile full, partial or absent, the mask at its positions"""
    check_case(c, "long_key_counts")


@pytest.mark.parametrize("c", L.MULTIBLOCK, **ids)
def test_walks_several_query_blocks(c):
    """xqb = 2, 4, 8 blocks of 128 queries per workgroup with the prefetch of the next block's Q; ragged and full last block"""
    check_case(c, "long_multiblock")


@pytest.mark.parametrize("c", L.RAGGED, **ids)
def test_ragged_batch(c):
    check_case(c, "long_ragged")


@pytest.mark.parametrize("c", L.LATE_KEY, **ids)
def test_late_dominant_key(c):
    """the re-reference branch inside the resident walk: planted keys of tiles 3 and 4 on peaked rows"""
    check_case(c, "long_late_key")


@pytest.mark.parametrize("c", L.REMAP, **ids)
def test_xcd_remap_remainder_branch(c):
    assert c.grid > 8 and c.grid % 8 != 0
    check_case(c, "long_remap")


# ---- the borders of the dispatch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (40, 64))
def test_128_keys_are_the_plain_op(d):
    """nk = 128 is forwarded: record 3 (xattn64_kernel) and the bits of cfgpp_op_attention on the same buffers"""
    need_gpu()
    import hip_ops as H
    c = A.Case(1, 2, 100, 128, d, "neg", planted=True, seed=2600 + d, kernel=3, xqb=1)
    got = check_case(c, "long_border")
    q, k, v, _ = A.make_inputs(c)
    hq, hk, hvt, qp, kp = make_heads_padded(c, q, k, v)
    plain = H.attention(hq, hk, hvt, c.B, c.h, c.d, c.Nq, c.Nk, qp, kp)
    assert H.attention_last_launch() == (3, c.d16, c.ones, 1)
    assert torch.equal(plain.cpu().view(torch.int16), got.view(torch.int16))


@pytest.mark.parametrize("nk", (321, 384))
def test_more_than_320_keys_take_the_flash_loop(nk):
    c = A.Case(1, 2, 100, nk, 64, "neg", planted=True, seed=2700 + nk, kernel=2)
    check_case(c, "long_border", k_pad=384)


def test_other_head_dims_take_their_kernel():
    c = A.Case(1, 2, 100, 154, 80, "neg", planted=True, seed=2800, kernel=1)
    check_case(c, "long_border")


def test_switch_off_takes_the_flash_loop():
    """cfgpp_attention_set_cross_long(0): the A/B partner of the measurements, same inputs, record 2"""
    need_gpu()
    import hip_ops as H
    c = A.Case(1, 2, 100, 154, 40, "neg", planted=True, seed=2900, kernel=2)
    H.lib().cfgpp_attention_set_cross_long(0)
    try:
        check_case(c, "long_border")
    finally:
        H.lib().cfgpp_attention_set_cross_long(2)
    check_case(replace(c, kernel=6, xqb=1), "long_border")


@pytest.mark.parametrize("d,nk,kernel", [(40, 154, 6), (48, 193, 6), (40, 308, 6), (56, 154, 6), (64, 192, 6), (64, 193, 2), (56, 308, 2), (64, 308, 2)])
def test_default_dispatch_ships_the_measured_classes(d, nk, kernel):
    """cfgpp_attention_set_cross_long(1), the default: the kernel where it measured >= 3 % faster (d = 40 / 48 at every key
    count, d = 56 / 64 at up to three resident tiles), the flash loop in the rest of its scope"""
    need_gpu()
    import hip_ops as H
    c = A.Case(1, 2, 100, nk, d, "neg", planted=True, seed=3100 + d + nk, kernel=kernel, xqb=1 if kernel == 6 else 0)
    H.lib().cfgpp_attention_set_cross_long(1)
    check_case(c, "long_default")


def test_short_key_buffer_is_refused():
    """k_tok_pad < nk: refused before anything is launched"""
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    c = A.Case(1, 2, 100, 154, 64, "rand", seed=3000)
    q, k, v, _ = A.make_inputs(c)
    hq, hk, hvt, qp, kp = make_heads_padded(c, q, k, v, k_pad=192)
    buf, o = guarded(c.B, c.Nq, c.h * c.d)
    with pytest.raises(CfgppError, match="k_tok_pad=192"):
        attention_cross(hq, hk, hvt, c, qp, kp, o, nk=200)
    torch.cuda.synchronize()
    assert H.attention_last_launch() == (0, 0, 0, 0)
    assert bool(torch.isnan(o).all()) and guards_intact(buf, c.h * c.d)
