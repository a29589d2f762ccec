"""The tables of tests/norm_cases.py reach every kernel instance the launchers of csrc/norm_kernels.hip can emit, the
references alone satisfy the conditions the GPU tests put on the kernels, and the per-element bound catches faults that the
whole-tensor rel-L2 of the older tests lets through - every fault is applied to the fp32 model (no GPU)."""
import math
from dataclasses import replace

import numpy as np
import pytest
import torch

import norm_cases as NC
from norm_cases import GN, LN

ids = dict(ids=lambda c: c.id)


# ---- the tables reach every instance ---------------------------------------------------------------------------------------
def test_case_ids_are_unique():
    for table in (NC.GN_CASES, NC.LN_TABLE + NC.LN_AUTO, NC.SM_TABLE):
        assert len(table) == len(set(c.id for c in table))


def test_slab_table_reaches_every_instance_the_launcher_can_emit():
    """every (NT, MAXCH) the launcher's rule yields for any chunk count 1 .. 32 and any pixel count: NT 320 and 960 with MAXCH
    2 / 4 / 8 / 16, NT 640 with MAXCH 16 only (640 is tried after 320 failed, i.e. with more than 8 chunks per thread)"""
    emit = {NC.slab_instance(cpp, hw) for cpp in range(1, 33) for hw in range(1, 16 * 960 + 2)} - {None}
    assert emit == {(nt, m) for nt in (320, 960) for m in (2, 4, 8, 16)} | {(640, 16)}
    got = {NC.expected_launch(c)[1:3] for c in NC.GN_CASES if NC.expected_launch(c)[0] == 1}
    assert got == emit
    assert {NC.expected_launch(c)[0] for c in NC.GN_CASES} == {1, 2, 3}
    # chunks per pixel segment 2, 5, 10, 15, 30 and groups per workgroup 1, 2, 4
    assert {NC.expected_launch(c)[4] for c in NC.GN_CASES} >= {2, 5, 10, 15, 30}
    assert {NC.expected_launch(c)[3] for c in NC.GN_CASES if NC.expected_launch(c)[0] == 1} == {1, 2, 4}


def test_slab_table_details():
    E = NC.expected_launch
    by = {c.id.split("-")[0]: E(c) for c in NC.SLAB_CPP5 + NC.SLAB_CPP10 + NC.SLAB_CPP15 + NC.SLAB_CPP30}
    assert [by[f"N{n}C320x{h}x{w}"][2] for n, (h, w) in zip((2, 2, 2, 2, 2, 1, 1), NC._HW7)] == [2, 2, 4, 8, 8, 16, 16]
    assert by["N1C2560x16x32"][:5] == (1, 320, 16, 1, 10) and by["N1C2560x32x32"][:5] == (1, 640, 16, 1, 10)
    assert by["N1C2560x7x5"][:5] == (1, 320, 2, 1, 10)
    assert all(E(c)[1] == 960 and E(c)[4] == 15 for c in NC.SLAB_CPP15)
    assert {E(c)[2] for c in NC.SLAB_CPP15} == {2, 4, 8, 16}
    assert E(NC.SLAB_CPP30[0])[:5] == (1, 960, 16, 1, 30)
    # chunks that straddle two groups: cpg 10, 20, 30, 60
    assert {c.cpg for c in NC.GN_CASES if E(c)[0] == 1 and c.cpg % 8} >= {10, 20, 30, 60}
    c = NC.SLAB_TOO_LARGE[0]
    assert E(c)[0] == 2 and c.mode == 2 and c.H * c.W == 1025 and c.cpg >= 8
    assert E(NC.SLAB_R128[0])[:5] == (1, 640, 16, 4, 5) and NC.SLAB_R128[0].H * NC.SLAB_R128[0].W == 1025
    assert [E(c)[0] for c in NC.AUTO_THRESHOLD] == [2, 1, 2, 1, 2, 1]
    assert [c.N * (c.G // NC.slab_split(c)[0]) for c in NC.AUTO_THRESHOLD] == [40, 48, 32, 48, 32, 64]
    c = NC.SLAB_REMAP[0]
    wgs = c.N * (c.G // NC.slab_split(c)[0])
    assert E(c)[0] == 1 and wgs == 20 and wgs > 8 and wgs % 8
    assert {E(c)[4] for c in NC.SLAB_TOKENS} == {5, 10, 15, 30} and all(c.tokens and E(c)[0] == 1 for c in NC.SLAB_TOKENS)
    # a ragged last pass (some thread's pixel slot lies beyond H * W) and H * W below one pass
    ragged = [c for c in NC.GN_CASES if E(c)[0] == 1 and (c.H * c.W) % (E(c)[1] // E(c)[4])]
    assert len(ragged) >= 10 and any(c.H * c.W < E(c)[1] // E(c)[4] for c in ragged)
    for c in NC.SLAB_CONCAT:
        gs, _ = NC.slab_split(c)
        chw, inside, straddled = gs * c.cpg, c.C0 % (gs * c.cpg) != 0, c.C0 % c.cpg != 0
        assert E(c)[0] == 1
        # 1280+1280: cpg 80 divides 1280, the boundary is a workgroup edge; every other pair has it inside a range and a group
        assert (inside and straddled) or (c.C0, c.C1) == (1280, 1280), c.id
        if straddled:                                  # the straddling group lies in the range that holds the boundary
            g = c.C0 // c.cpg
            assert g * c.cpg // chw == ((g + 1) * c.cpg - 1) // chw == c.C0 // chw


def test_two_launch_table_reaches_every_path():
    E = NC.expected_launch
    tl = [c for c in NC.GN_CASES if E(c)[0] == 2]
    assert {E(c)[5] for c in tl} == {16, 32, 64}                      # stats pixels per block
    assert {1, 256} <= {E(c)[6] for c in tl}
    assert {E(c)[7] for c in tl} == {16, 32, 64}                      # apply pixels per block
    assert any(E(c)[5] == 64 and E(c)[6] == 256 for c in tl) and any(E(c)[5] == 64 and c.N == 13 for c in tl)
    assert any((c.H * c.W) % E(c)[5] for c in tl) and any((c.H * c.W) % E(c)[7] for c in tl)          # a partial last block
    for k in (5, 7):
        loops = [NC.two_launch_loops(c, E(c)[k]) for c in tl]
        assert any(u for u, _ in loops) and any(t for _, t in loops) and any(u and t for u, t in loops)
    assert {c.C for c in tl} >= {64, 192, 320, 2048, 2560}
    assert any(c.tokens for c in tl) and any(c.C1 and c.C0 % c.cpg for c in tl)
    assert any(c.C // 8 > 256 and c.H * c.W == 16 for c in tl)          # second channel pass, one block
    c = NC.PIVOT_OUTLIER[0]
    assert (c.N, c.C, c.H, c.W, E(c)[0]) == (1, 64, 128, 128, 2)
    x, _, _ = NC.gn_inputs(c)
    assert bool((x[:, 0, ::c.cpg] == 60).all()) and float(x[:, 1:].abs().max()) < 0.1
    pre = [c for c in NC.GN_CASES if c.pre]
    assert {c.H * c.W for c in pre} == {32, 256, 1024} and {c.cpg for c in pre} == {2, 10, 30}
    assert {c.kind for c in pre} == {"groups", "offset", "const"} and all((c.H * c.W) % 32 == 0 for c in pre)
    assert any(c.C1 for c in pre) and any(c.cpg * c.H * c.W // 32 < 256 for c in pre)


def test_layernorm_and_softmax_tables_reach_every_instance():
    got = {NC.expected_launch(c, rpw) for c in NC.LN_TABLE for rpw in NC.LN_RPW}
    assert got == {(mv, r) for mv in (1, 2, 3) for r in (1, 2, 4)} | {(4, 1)}
    assert [NC.expected_launch(c) for c in NC.LN_AUTO] == [(1, 2), (1, 1), (1, 1)]
    assert {c.C for c in NC.LN_TABLE} == set(NC.LN_C) and {c.rows for c in NC.LN_TABLE} == set(NC.LN_ROWS)
    assert {(c.kind, NC.expected_launch(c)[0]) for c in NC.LN_TABLE} >= {(k, mv) for k in NC.LN_KINDS for mv in (1, 2, 3, 4)}
    assert {NC.expected_launch(c) for c in NC.SM_TABLE} == {(2,), (8,)}
    assert {c.ncols for c in NC.SM_TABLE} == set(NC.SM_NCOLS) and {c.kind for c in NC.SM_TABLE} == set(NC.SM_KINDS)
    assert all(C % 8 or C > 2048 for C in NC.LN_REFUSED) and all(n % 8 or n > 16384 for n in NC.SM_REFUSED)


# ---- the references alone -------------------------------------------------------------------------------------------------
def _check_reference(c):
    r = NC.reference(c)
    x = r.inputs[0]
    assert torch.equal(x, x.half().float()) and bool(torch.isfinite(x).all()), c.id
    assert bool(torch.isfinite(r.ref).all()) and math.isfinite(r.a_case), c.id
    # fp32 arithmetic on these inputs: A_case is a few fp32 ulps of the largest intermediate, far below the fp16 spacing.
    # `const`: rstd = eps^-1/2, and x * sc + sh cancels two terms of size |x gamma| eps^-1/2 - beta is met to an fp32 ulp of THAT
    if c.kind == "const" and not isinstance(c, NC.SM):
        cap = 2.0 ** -22 * float(x.abs().max() * r.inputs[1].abs().max()) * getattr(c, "eps", 1e-5) ** -0.5
    else:
        cap = 2.0 ** -11 * float(r.ref.abs().max()) / 8 + 2.0 ** -26
    assert 0 <= r.a_case <= cap, (c.id, r.a_case, cap)
    if c.kind in NC.ORDINARY:
        assert r.model_mismatch <= NC.MODEL_MISMATCH_CAP, (c.id, r.model_mismatch)
    return r


@pytest.mark.parametrize("group", list(NC.GN_GROUPS))
def test_groupnorm_references(group):
    for c in NC.GN_GROUPS[group]:
        r = _check_reference(c)
        x, gamma, beta = r.inputs
        model = NC.gn_model32(c, x, gamma, beta)
        assert NC.within_bound(NC.to_half(model), r.ref, r.a_case), c.id
        assert NC.rel_l2(NC.to_half(model), r.ref) < NC.rel_l2_bound(c) / 2, c.id
        if c.kind == "const":                        # the variance is exactly 0: the output is beta, or SiLU(beta)
            b = beta.double().expand(r.ref.shape)
            assert float((r.ref - (NC._silu64(b) if c.silu else b)).abs().max()) < 1e-12, c.id
        if c.kind == "offset":
            xg = x.double().reshape(c.N, -1, c.G, c.cpg)
            ratio = xg.mean((1, 3)).abs() / xg.std((1, 3))
            assert 80 < float(ratio.min()) and float(ratio.max()) < 125, c.id
        if c.pre:                                    # the pairs fold back to the group statistics (Chan, in fp64)
            g0, g1 = NC.producer_stats(c, x)
            st = (torch.cat([g0, g1], 1) if c.C1 else g0).double().reshape(c.N, -1, c.G, c.cpg, 2)
            mean = st[..., 0].mean((1, 3))
            m2 = st[..., 1].sum((1, 3)) + 32 * ((st[..., 0] - mean[:, None, :, None]) ** 2).sum((1, 3))
            xg = x.double().reshape(c.N, -1, c.G, c.cpg)
            assert float((mean - xg.mean((1, 3))).abs().max()) < 1e-5 * max(1.0, float(mean.abs().max()))
            var = ((xg - xg.mean((1, 3), keepdim=True)) ** 2).sum((1, 3))
            assert float((m2 - var).abs().max()) <= 1e-5 * float(var.max()) + 1e-9


def test_layernorm_and_softmax_references():
    for c in NC.LN_TABLE + NC.LN_AUTO:
        r = _check_reference(c)
        x, gamma, beta = r.inputs
        assert NC.within_bound(NC.to_half(NC.ln_model32(x, gamma, beta)), r.ref, r.a_case), c.id
        if c.kind == "const":
            assert float((r.ref - beta.double()).abs().max()) < 1e-12, c.id
    for c in NC.SM_TABLE:
        r = _check_reference(c)
        assert NC.within_bound(NC.to_half(NC.sm_model32(*r.inputs)), r.ref, r.a_case), c.id
        assert float((r.ref.sum(1) - 1).abs().max()) < 1e-12
        if c.kind in ("equal", "min"):
            assert float((r.ref - 1.0 / c.ncols).abs().max()) < 1e-15


# ---- fault models: the bound catches them, the whole-tensor rel-L2 of the older tests does not -----------------------------
def _fault(c, fault, **fk):
    """-> (excess over 0.5 ulp16 / (FACTOR * A_case), mismatch share, rel-L2) of the faulty model rounded to fp16"""
    r = NC.reference(c)
    bad = NC.to_half(NC.gn_model32(c, *r.inputs, fault=fault, **fk))
    return NC.excess(bad, r.ref) / r.slack, NC.mismatch_share(bad, r.ref), NC.rel_l2(bad, r.ref)


FAULT_64 = GN(2, 320, 0, 64, 64, kind="rand", silu=1, mode=1, seed=4001)
FAULT_STRADDLE = [GN(2, C, 0, 16, 16, kind="rand", seed=4002 + C) for C in (320, 640, 960, 1920)]
FAULT_TAIL = GN(1, 320, 0, 25, 40, kind="rand", silu=1, seed=4003)


def test_variance_count_off_by_one_pixel_at_64x64():
    over, share, rel = _fault(FAULT_64, "count_off_by_one_pixel")
    assert over >= 10 and share > 4 * NC.MISMATCH_CAP and rel < NC.REL_L2_BOUND, (over, share, rel)


@pytest.mark.parametrize("c", FAULT_STRADDLE, **ids)
def test_straddling_chunk_takes_the_lower_groups_statistics(c):
    """cpg 10, 20, 30, 60.  Even on `rand` inputs, where neighbouring groups differ only by their sampling noise, the fault is
    three orders beyond the bound; there rel-L2 is 2e-3 .. 1.5e-2, so the old bound would have seen it too - had any test run a
    straddling chunk through the slab kernel.  On `groups` inputs (what the GPU cases use) it is far beyond everything."""
    over, share, rel = _fault(c, "straddle_lower_group")
    assert over >= 1000 and share > 4 * NC.MISMATCH_CAP and rel < 2e-2, (over, share, rel)
    over, share, rel = _fault(replace(c, kind="groups"), "straddle_lower_group")
    assert over >= 1e5 and share > 4 * NC.MISMATCH_CAP and rel > 0.1, (over, share, rel)


def test_slab_tail_pixels_enter_pass_2():
    nt, maxch = NC.expected_launch(FAULT_TAIL)[1:3]
    pad = maxch * (nt // 5) - 1000
    assert pad == 24
    over, share, rel = _fault(FAULT_TAIL, "tail_in_pass2", pad=pad)
    assert over >= 10 and share > 4 * NC.MISMATCH_CAP and rel < NC.REL_L2_BOUND, (over, share, rel)


@pytest.mark.parametrize("c", [FAULT_64, FAULT_TAIL, FAULT_STRADDLE[0]], **ids)
def test_rstd_off_by_2e_4_relative(c):
    over, share, rel = _fault(c, "rstd_rel", rel=2e-4)
    assert over >= 10 and share > 4 * NC.MISMATCH_CAP and rel < NC.REL_L2_BOUND, (over, share, rel)


@pytest.mark.parametrize("c", [c for c in NC.LN_TABLE if c.rows >= 3 and c.kind in ("rand", "offset", "outlier")][::3], **ids)
def test_layernorm_tail_row_stored_from_the_clamped_duplicate(c):
    """a whole wrong row: on `rand` rows rel-L2 sees it as well; on `offset` rows (every row normalises to the same
    distribution) and on the bound's own terms it is far beyond the per-element bound"""
    r = NC.reference(c)
    bad = NC.to_half(NC.ln_model32(*r.inputs, fault="tail_row_duplicate"))
    assert NC.excess(bad, r.ref) / r.slack >= 1000


# ---- the pixel-row computation of the GroupNorm kernels ---------------------------------------------------------------------
def test_float_division_of_the_pixel_index_is_exact():
    """(int)((p + 0.5f) * (1.0f / W)) == p / W in fp32 for every W <= 1024 and every p < H * W <= 2^20 (H <= 1024): the claim of
    the comment above poff in gn_stats_kernel / gn_apply_kernel / gn_slab_kernel"""
    half, one = np.float32(0.5), np.float32(1.0)
    p = np.arange(1 << 20, dtype=np.int32)
    pf = p.astype(np.float32) + half
    assert np.array_equal(pf.astype(np.float64), p.astype(np.float64) + 0.5)            # p + 0.5 is exact below 2^23
    for W in range(1, 1025):
        n = 1024 * W
        inv = one / np.float32(W)
        q = (pf[:n] * inv).astype(np.int32)
        assert np.array_equal(q, p[:n] // W), W
