"""The case table of tests/attn_region_soft_cases.py covers the soft regional cross-attention kernel and would catch its real
faults: an independent fp32 model of a correct kernel (another summation order) stays inside every bound, and every fault below,
applied to the fp64 model of the kernel (no GPU), pushes at least one case past its bound - the bound
tests/test_gpu_attention_region_soft.py asserts for kernel 9 - at least tenfold."""
import math

import pytest
import torch

import attn_cases as A
import attn_region_soft_cases as SC

ids = dict(ids=lambda c: c.id)
SMALL = [c for c in SC.ALL_CASES if c.Nq <= 129]


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = SC.reference(c)
        return cache[c]
    return get


def over_bound(refs, c, fault, **fk):
    bld, ref, e_model, bound = refs(c)
    assert bound > 0, c.id
    return A.max_row_err(SC.model(c, bld, fault, **fk), ref, c.d) / bound


def test_table_coverage():
    """every instance (dp = 32, 64 with and without the ones row, 96, 160), every pattern, every R; B * heads of 2 .. 3"""
    assert len(SC.ALL_CASES) == len(set(c.id for c in SC.ALL_CASES))
    assert {(c.d16, c.ones) for c in SC.ALL_CASES} >= {(2, 0), (3, 1), (4, 0), (5, 1), (10, 0)}
    assert {c.Nq for c in SC.ALL_CASES} == {1, 100, 129, 300}
    assert all(2 <= c.B * c.h <= 3 and c.kernel == 9 for c in SC.ALL_CASES)
    for R in (2, 3, 4):
        pats = {c.pattern for c in SC.ALL_CASES if c.R == R}
        assert pats >= {f"hot{r}" for r in range(R)} | {"uniform", "ramp", "lane", "random", "pair", "skip0", f"skip{R - 1}"}
        for p in ("uniform", "ramp", "lane", "random") + tuple(f"hot{r}" for r in range(R)):
            assert {c.d for c in SC.ALL_CASES if c.R == R and c.pattern == p} >= set(SC.D_ALL), (R, p)
        assert {c.k_pad for c in SC.ALL_CASES if c.R == R} == {SC.min_k_pad(R), SC.K_PAD} or SC.min_k_pad(R) == SC.K_PAD
    assert {c.map_rows for c in SC.BATCH} == {1, 2} and all(c.B == 2 and c.Nq % 128 for c in SC.BATCH)
    assert all(c.grid == 9 for c in SC.SKIP)                                   # > 8 workgroups, not a multiple of 8
    assert set(SC.HEAD_DIMS_REFUSED) == {104, 112, 136, 144}


def test_weight_patterns():
    for c in SC.ALL_CASES:
        w = SC.weights(c)
        assert w.shape == (c.map_rows, c.R, c.Nq) and w.dtype == torch.float32
        assert bool((w >= 0).all()) and float((w.sum(1) - 1).abs().max()) < 1e-6, c.id
    ramp = SC.weights(next(c for c in SC.MIXED if c.pattern == "ramp" and c.R == 4))[0]
    assert ramp[0, 40] == 1 and 0 < ramp[0, 48] < 1 and ramp[1, 56] == 1               # a ramp inside the slab 32 .. 63
    assert 0 < ramp[3, 127] < 1 and 0 < ramp[3, 128] < 1 and ramp[3, 128] > ramp[3, 127]     # ... and one across the block edge
    lane = SC.weights(next(c for c in SC.MIXED if c.pattern == "lane" and c.R == 3))[0]
    assert (lane[2] != 0).nonzero().flatten().tolist() == [SC.LANE_ROW] and SC.LANE_ROW // 32 == 2 and SC.LANE_ROW < 128
    skip = next(c for c in SC.SKIP if c.pattern == "skip0")
    assert SC.dead_regions(skip) == [0]
    bld = SC.build(skip)
    assert float(bld["v"][:, :SC.TOK].abs().min()) == SC.L.JUNK and float(bld["k"][:, skip.Nk:].abs().min()) == SC.L.JUNK
    s_dead = (bld["q"][0].double() @ bld["k"][:, :SC.TOK].double().transpose(1, 2)) / math.sqrt(skip.d)
    s_live = (bld["q"][0].double() @ bld["k"][:, SC.TOK: 2 * SC.TOK].double().transpose(1, 2)) / math.sqrt(skip.d)
    assert float(s_dead.min()) > float(s_live.max()) + 5                               # the dead region's keys would dominate
    pair = SC.weights(SC.BATCH[0])
    assert pair.shape[0] == 2 and not torch.equal(pair[0], pair[1])
    hot = next(c for c in SC.HOT if c.pattern == "hot1" and c.R == 3)
    assert SC.dead_regions(hot) == [0, 2]


def test_honest_models_are_inside_every_bound():
    """the fp64 model within a quarter of its bound by construction, and an independent fp32 model with reversed key order and
    descending regions inside it; the model's error is a rounding error, not a blend that cancelled"""
    for c in SC.ALL_CASES:
        bld, ref, e_model, bound = SC.reference(c)
        assert ref.shape == (c.B, c.Nq, c.h * c.d) and bool(torch.isfinite(ref).all())
        assert math.isfinite(e_model) and 2.0 ** -14 < e_model < 2e-3, (c.id, e_model)
        e32 = A.max_row_err(SC.model_fp32(c, bld), ref, c.d)
        assert e32 <= bound, (c.id, e32, bound)


def test_one_hot_weights_are_the_hard_partition():
    """with one-hot weights the reference is tests/attn_cases.ref64 over the row's own 77 keys"""
    c = next(c for c in SC.HOT if c.pattern == "hot2" and c.R == 3 and c.d == 80 and c.Nq == 100)
    bld = SC.build(c)
    q, k, v = SC.full_inputs(c, bld)
    own = slice(2 * SC.TOK, 3 * SC.TOK)
    assert torch.allclose(SC.ref64(c, bld), A.ref64(q, k[:, :, own], v[:, :, own]), rtol=1e-12, atol=1e-12)


def _worst(refs, cases, fault, **fk):
    return max(over_bound(refs, c, fault, **fk) for c in cases)


def test_fault_weights_of_two_regions_swapped(refs):
    for c in [c for c in SMALL if c.pattern in ("ramp", "lane", "random", "pair") or c.pattern.startswith("hot")]:
        a = int(c.pattern[3:]) if c.pattern.startswith("hot") else 0
        b = (a + 1) % c.R if c.pattern.startswith("hot") else c.R - 1
        assert over_bound(refs, c, "swap_weights", a=a, b=b) >= 10, c.id


def test_fault_row_b_uses_row_b_plus_1_map(refs):
    for c in [c for c in SC.BATCH if c.pattern == "pair"]:
        assert over_bound(refs, c, "next_batch_map") >= 10, c.id


def test_fault_joint_normalisation(refs):
    cases = [c for c in SMALL if c.pattern in ("uniform", "random", "pair")]
    assert min(over_bound(refs, c, "joint_norm") for c in cases) >= 10


@pytest.mark.parametrize("shift", [1, -1])
def test_fault_key_window_off_by_one(refs, shift):
    for c in [c for c in SMALL if c.Nq > 1]:
        assert over_bound(refs, c, "off_by_one", shift=shift) >= 10, (c.id, shift)


def test_fault_weight_region_stride_read_as_nq(refs):
    for c in [c for c in SMALL if c.Nq % 128 and c.pattern in ("uniform", "ramp", "random", "pair", "lane")]:
        assert over_bound(refs, c, "stride_nq") >= 10, c.id


def test_fault_single_lane_region_skipped(refs):
    for c in [c for c in SC.MIXED if c.pattern == "lane"]:
        assert over_bound(refs, c, "lane_skipped") >= 10, c.id


def test_fault_zero_weight_region_evaluated_with_junk_that_overflows():
    """a kernel that evaluates a zero-weight term and multiplies it by 0: finite junk passes through it unseen, junk that overflows
    (here: value slots beyond the fp16 range, held as inf) makes 0 x inf = NaN, which the metric maps to inf.  The honest model does
    not read the region at all."""
    for c in [c for c in SC.SKIP if c.pattern.startswith("skip") and c.d in (40, 160)]:
        bld, ref, e_model, bound = SC.reference(c)
        dead = SC.dead_regions(c)[0]
        bld["v"][:, SC.TOK * dead: SC.TOK * (dead + 1)] = math.inf
        assert A.max_row_err(SC.model(c, bld), ref, c.d) == e_model
        assert A.max_row_err(SC.model(c, bld, "zero_evaluated"), ref, c.d) == math.inf > 10 * bound
