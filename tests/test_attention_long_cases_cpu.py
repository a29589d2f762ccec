"""The case table of tests/attn_long_cases.py would catch real faults of a resident multi-tile cross-attention kernel: every fault
below is applied to the fp64 model of the kernels (no GPU) and must push its designated cases past their bound - the bound
tests/test_gpu_attention_long.py asserts for xattn64_long_kernel - at least tenfold, as tests/test_attention_cases_cpu.py requires
of the older table."""
import math
from dataclasses import replace

import pytest
import torch

import attn_cases as A
import attn_long_cases as L


def pick(group, **kw):
    out = [c for c in L.GROUPS[group] if all(getattr(c, a) == b for a, b in kw.items())]
    assert out, (group, kw)
    return out


@pytest.fixture(scope="module")
def refs():
    """reference(case), computed once per case and shared by the faults that use it"""
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = A.reference(c)
        return cache[c]
    return get


def over_bound(refs, c, fault, **fk):
    q, k, v, info, ref, e_model, bound = refs(c)
    assert bound > 0, c.id
    if fault == "tile_alias":
        got = L.model_tile_alias(c, q, k, v, **fk)
    elif fault == "stale_slots":
        got = L.model_stale_slots(c, q, k, v)
    else:
        got = A.model(q, k, v, fault, **fk)
    return A.max_row_err(got, ref, c.d) / bound


ids = dict(ids=lambda c: c.id)
# neg rows: every real score is strongly negative, a pad / stale key that enters takes the probability mass
NEG_WITH_PADS = [c for c in pick("long_key_counts", kind="neg", Nq=100) if c.Nk % 64] + pick("long_ragged")
NEG_ALL = pick("long_key_counts", kind="neg", Nq=100) + pick("long_ragged") + pick("long_remap")
PLANTED = pick("long_key_counts", Nq=129) + pick("long_late_key")
STALE = [c for c in NEG_ALL + PLANTED if c.Nk < L.K_PAD]


@pytest.mark.parametrize("c", NEG_WITH_PADS, **ids)
def test_pad_keys_admitted_with_score_zero(refs, c):
    assert over_bound(refs, c, "pad_leak") >= 10


@pytest.mark.parametrize("c", NEG_WITH_PADS, **ids)
def test_denominator_counts_pad_keys(refs, c):
    assert over_bound(refs, c, "denom_pads") >= 10


@pytest.mark.parametrize("c", PLANTED + NEG_ALL, **ids)
def test_last_valid_key_dropped(refs, c):
    assert over_bound(refs, c, "drop_key", key=c.Nk - 1) >= 10


@pytest.mark.parametrize("c", NEG_ALL, **ids)
def test_first_key_of_every_tile_dropped(refs, c):
    for t in range((c.Nk + 63) // 64):
        assert over_bound(refs, c, "drop_key", key=64 * t) >= 10, t


@pytest.mark.parametrize("c", PLANTED, **ids)
def test_vt_without_the_permutation(refs, c):
    assert over_bound(refs, c, "v_unpermuted") >= 10


@pytest.mark.parametrize("c", pick("long_multiblock", h=128) + pick("long_multiblock", Nq=1024), **ids)
def test_query_block_answers_with_previous_blocks_queries(refs, c):
    c = replace(c, h=c.h // 16)                        # the walk of one workgroup: the head count does not matter to the model
    assert over_bound(refs, c, "prev_q_block", xqb=c.xqb) >= 10


@pytest.mark.parametrize("c", pick("long_late_key", d=64) + pick("long_key_counts", Nq=129, d=64, Nk=308), **ids)
def test_rereference_skipped(refs, c):
    assert c.d % 32 == 0 and over_bound(refs, c, "no_rereference") >= 10


@pytest.mark.parametrize("c", NEG_ALL + PLANTED, **ids)
def test_tile_reads_the_previous_tiles_k_and_vt(refs, c):
    """every tile t >= 1 on its own, the middle ones included"""
    for t in range(1, (c.Nk + 63) // 64):
        assert over_bound(refs, c, "tile_alias", tile=t) >= 10, t


@pytest.mark.parametrize("c", STALE, **ids)
def test_stale_slots_enter_the_softmax(refs, c):
    assert over_bound(refs, c, "stale_slots") >= 10


def test_honest_model_is_within_a_quarter_of_every_bound():
    assert len(L.ALL_CASES) == len(set(c.id for c in L.ALL_CASES))
    assert not set(c.id for c in L.ALL_CASES) & set(c.id for c in A.ALL_CASES)
    for c in L.ALL_CASES:
        _, _, _, info, ref, e_model, bound = A.reference(c, full=False)
        assert math.isfinite(e_model) and 2.0 ** -14 < e_model <= bound / A.FACTOR and e_model < 2e-2, (c.id, e_model)
        assert ref.shape == (c.B, c.Nq, c.h * c.d) and bool(torch.isfinite(ref).all())


def test_expected_dispatch_of_the_table():
    """129 .. 320 keys at dp = 64, and the xqb of every case is the launcher's"""
    for c in L.ALL_CASES:
        assert c.kernel == 6 and 129 <= c.Nk <= 320 and (c.d + 31) // 32 == 2 and c.xqb == L.launcher_xqb(c), c.id
    assert sorted(set(c.xqb for c in L.MULTIBLOCK)) == [2, 4, 8]
    assert [c.grid for c in L.REMAP] == [9, 13]
    for c in L.LATE_KEY:                               # five tiles: a planted key in the second-to-last one
        assert 64 * 3 + 21 in A.planted_keys(c.Nk)
