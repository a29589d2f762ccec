"""The case table of tests/attn_region_cases.py would catch real faults of a region-masked cross-attention kernel: every fault below
is applied to the fp64 model of the kernels (no GPU) and must push its designated cases past their bound - the bound
tests/test_gpu_attention_region.py asserts for kernels 7 and 8 - at least tenfold, as tests/test_attention_cases_cpu.py requires of
the older tables."""
import math

import pytest
import torch

import attn_cases as A
import attn_region_cases as RC

ids = dict(ids=lambda c: c.id)
SMALL = [c for c in RC.ALL_CASES if c.Nq <= 129 and c.h <= 4]
HAS_LOWER_REGION = [c for c in SMALL if c.pattern != f"all{c.R - 1}"]
HAS_BORDER = [c for c in SMALL if c.pattern in ("alt", "slab", "edge", "pair") and c.Nq > 1]
HAS_UPPER_REGION = [c for c in SMALL if c.pattern != "all0"]
TWO_MAPS = [c for c in RC.ALL_CASES if c.pattern == "pair"]


@pytest.fixture(scope="module")
def refs():
    """reference(case), computed once per case and shared by the faults that use it"""
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = RC.reference(c)
        return cache[c]
    return get


def over_bound(refs, c, fault, **fk):
    bld, ref, e_model, bound = refs(c)
    assert bound > 0, c.id
    return A.max_row_err(RC.compute(c, bld, A.model, fault, **fk), ref, c.d) / bound


@pytest.mark.parametrize("c", SMALL, **ids)
def test_mask_ignored(refs, c):
    assert over_bound(refs, c, "mask_ignored") >= 10


@pytest.mark.parametrize("c", HAS_LOWER_REGION, **ids)
def test_key_range_one_slot_late(refs, c):
    """[77 r + 1, 77 r + 78): the next region's first key (a case needs a row of a region < R - 1 for it: behind the last region
    lies one junk slot, whose sign is luck - test_tail_junk_admitted covers those slots)"""
    assert over_bound(refs, c, "off_by_one", shift=1) >= 10


@pytest.mark.parametrize("c", HAS_UPPER_REGION, **ids)
def test_key_range_one_slot_early(refs, c):
    """[77 r - 1, 77 r + 76): the previous region's last key (a case needs a row of a region >= 1 for it)"""
    assert over_bound(refs, c, "off_by_one", shift=-1) >= 10


@pytest.mark.parametrize("c", HAS_BORDER, **ids)
def test_id_taken_from_the_neighbouring_query(refs, c):
    assert over_bound(refs, c, "neighbour_id") >= 10


@pytest.mark.parametrize("c", TWO_MAPS, **ids)
def test_batch_0_map_used_for_batch_1(refs, c):
    assert over_bound(refs, c, "batch0_map") >= 10


@pytest.mark.parametrize("c", SMALL, **ids)
def test_tail_junk_admitted(refs, c):
    assert over_bound(refs, c, "tail_junk") >= 10


@pytest.mark.parametrize("c", [c for c in RC.ALL_IN_ONE if c.Nq == 100 and c.d == 64], **ids)
def test_all_masked_first_tile_is_not_finite_and_the_bound_sees_it(refs, c):
    """the hazard the region kernel's per-lane start removes: rows with no own key in tile 0 come out NaN, which the metric maps
    to inf; rows of region 0 (own keys in tile 0) are untouched"""
    bld, ref, e_model, bound = refs(c)
    got = RC.online_all_masked_first_tile(c, bld)
    rid = int(c.pattern[3:])
    if rid == 0:
        assert bool(torch.isfinite(got).all()) and A.max_row_err(got, ref, c.d) <= bound
    else:
        assert bool(torch.isnan(got).any())
        assert A.max_row_err(got, ref, c.d) == math.inf > 10 * bound


def test_honest_model_is_within_a_quarter_of_every_bound():
    assert len(RC.ALL_CASES) == len(set(c.id for c in RC.ALL_CASES))
    for c in SMALL:
        bld, ref, e_model, bound = RC.reference(c)
        assert math.isfinite(e_model) and 2.0 ** -14 < e_model <= bound / A.FACTOR and e_model < 2e-2, (c.id, e_model)
        assert ref.shape == (c.B, c.Nq, c.h * c.d) and bool(torch.isfinite(ref).all())


def test_inputs_make_a_leak_loud():
    """a foreign leak key beats the row's own maximum by far more than RESCALE_THR = 5 (log2 domain); a late own key beats every
    earlier own key of its rows by as much, and sits in a later 64-key tile than the region's first key"""
    for c in (RC.MIXED[0], RC.MIXED[-1], RC.BATCH[0]):
        bld = RC.build(c)
        q, k = bld["q"][0].double(), bld["k"].double()
        s = (q @ k.transpose(1, 2)) / math.sqrt(c.d) * A.LOG2E_F32             # [P, Nq, k_pad], log2 domain
        ids = bld["maps"][0]
        for r in range(c.R):
            rows = ids == r
            if not bool(rows.any()):
                continue
            own = s[:, rows, RC.TOK * r: RC.TOK * (r + 1)]
            for f in range(c.R):
                if f != r:
                    for loc in RC.LEAK_LOCAL:
                        lead = s[:, rows, RC.TOK * f + loc] - own.max(-1).values
                        late = (torch.arange(c.Nq) % 8 == 3)[rows]               # their own maximum is the late key, itself ~ +29:
                        assert float(lead[:, ~late].min()) > 4 * 5.0 and float(lead.min()) > 0.0, (c.id, r, f)      # the leak still leads
            late_rows = rows & (torch.arange(c.Nq) % 8 == 3)
            if bool(late_rows.any()):
                sl = s[:, late_rows]
                before = sl[:, :, RC.TOK * r: RC.TOK * r + RC.LATE_LOCAL].max(-1).values
                assert float((sl[:, :, RC.TOK * r + RC.LATE_LOCAL] - before).min()) > 4 * 5.0, (c.id, r)
            assert (RC.TOK * r + RC.LATE_LOCAL) // 64 > (RC.TOK * r) // 64
        assert float(bld["k"][:, c.Nk:].abs().min()) == RC.L.JUNK and c.k_pad > c.Nk


def test_expected_dispatch_of_the_table():
    """kernel 7 at head dims padded to 64 with both switches on, kernel 8 otherwise; the xqb of every case is the launcher's"""
    for c in RC.ALL_CASES:
        assert c.kernel == RC.expected_kernel(c.d, c.dma, c.cross) and c.xqb == RC.launcher_xqb(c), c.id
        assert c.k_pad % 64 == 0 and c.k_pad >= (c.Nk + 63) // 64 * 64
    assert sorted(set(c.xqb for c in RC.MULTIBLOCK if c.kernel == 7)) == [2, 4, 8]
    assert [c.grid for c in RC.REMAP] == [9, 13]
    assert all(c.kernel == 8 for c in RC.SWITCHES) and {(c.dma, c.cross) for c in RC.SWITCHES} == {(0, 1), (1, 0)}
    for R in (2, 3, 4):
        assert {c.pattern for c in RC.ALL_IN_ONE if c.R == R} == {f"all{r}" for r in range(R)}
        for kern, dims in ((7, RC.D7), (8, RC.D8)):
            assert {c.d for c in RC.ALL_CASES if c.R == R and c.kernel == kern and c.dma and c.cross} >= set(dims)
    m = RC.region_map(RC.MIXED[0])
    assert m.shape == (1, 129)
    slab = RC.region_map(next(c for c in RC.MIXED if c.pattern == "slab" and c.R == 4))[0]
    assert slab[44] == 0 and slab[45] == 1 and slab[95] == 2                     # borders inside 32-row slabs
    edge = RC.region_map(next(c for c in RC.MIXED if c.pattern == "edge"))[0]
    assert edge[127] == 0 and edge[128] == 1                                     # a border at the 128-query block edge
    pair = RC.region_map(RC.BATCH[0])
    assert pair.shape[0] == 2 and not torch.equal(pair[0], pair[1])
