"""The case table of tests/attn_cases.py would catch real faults: every fault below is applied to the fp64 model of the
kernels (no GPU) and must push its designated cases past their bound - the bound tests/test_gpu_attention.py asserts for
the kernels - at least tenfold.  The honest model stays under bound / FACTOR on every case of the table."""
import math
from dataclasses import replace

import pytest
import torch

import attn_cases as A


def pick(group, **kw):
    out = [c for c in A.GROUPS[group] if all(getattr(c, a) == b for a, b in kw.items())]
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
    return A.max_row_err(A.model(q, k, v, fault, **fk), ref, c.d) / bound


NEG_WITH_PADS = (pick("flash_partial", kind="neg", Nq=100)[::3] + pick("xattn_small", kind="neg", Nq=100, Nk=33)
                 + pick("xattn_small", kind="neg", Nq=100, Nk=97) + pick("switch_cross0", Nk=77) + pick("head_dims", d=8)
                 + pick("head_dims", d=160) + pick("switch_dma0", Nk=144) + pick("xattn_multiblock", h=128, d=48))
PLANTED = (pick("flash_partial", planted=True, Nq=257)[::3] + pick("xattn_small", Nq=129, d=56)[1:] + pick("head_dims")[::3]
           + pick("switch_dma0", d=48) + pick("switch_cross0", d=40))
ids = dict(ids=lambda c: c.id)


@pytest.mark.parametrize("c", NEG_WITH_PADS, **ids)
def test_pad_keys_admitted_with_score_zero(refs, c):
    assert over_bound(refs, c, "pad_leak") >= 10


@pytest.mark.parametrize("c", NEG_WITH_PADS, **ids)
def test_denominator_counts_pad_keys(refs, c):
    assert over_bound(refs, c, "denom_pads") >= 10


@pytest.mark.parametrize("c", PLANTED, **ids)
def test_last_valid_key_dropped(refs, c):
    assert over_bound(refs, c, "drop_key", key=c.Nk - 1) >= 10


@pytest.mark.parametrize("c", PLANTED, **ids)
def test_first_key_of_last_tile_dropped(refs, c):
    assert over_bound(refs, c, "drop_key", key=64 * ((c.Nk - 1) // 64)) >= 10


@pytest.mark.parametrize("c", PLANTED, **ids)
def test_vt_without_the_permutation(refs, c):
    assert over_bound(refs, c, "v_unpermuted") >= 10


@pytest.mark.parametrize("c", pick("xattn_multiblock", d=40, Nq=1000, h=128) + pick("xattn_multiblock", d=64, Nq=1024), **ids)
def test_query_block_answers_with_previous_blocks_queries(refs, c):
    c = replace(c, h=c.h // 16)                        # the walk of one workgroup: the head count does not matter to the model
    assert over_bound(refs, c, "prev_q_block", xqb=c.xqb) >= 10


@pytest.mark.parametrize("c", PLANTED + NEG_WITH_PADS[:3], **ids)
def test_two_heads_swapped(refs, c):
    assert c.h >= 2 and over_bound(refs, c, "swap_heads") >= 10


@pytest.mark.parametrize("c", PLANTED, **ids)
def test_one_query_slice_unwritten(refs, c):
    last = 32 * ((c.Nq - 1) // 32)
    assert over_bound(refs, c, "unwritten", rows=(32, 64)) >= 10 and over_bound(refs, c, "unwritten", rows=(last, c.Nq)) >= 10


@pytest.mark.parametrize("c", pick("rescale", d=64) + pick("rescale", d=160) + pick("switch_dma0", d=64, Nk=1024), **ids)
def test_rereference_skipped(refs, c):
    assert c.d % 32 == 0 and over_bound(refs, c, "no_rereference") >= 10


def test_honest_model_is_within_a_quarter_of_every_bound():
    """by construction (bound = FACTOR * E_model): guards the table and the metric against edits.  E_model itself is bounded by
    the formats: three roundings of relative size 2^-11 (q, P, output); the q rounding moves a score of up to ~60 (log2
    domain, the planted pairs) by 60 * 2^-11 * ln 2 = 2 % in P, on rows that own ~half of a planted V row's weight at most"""
    assert len(A.ALL_CASES) == len(set(c.id for c in A.ALL_CASES))
    for c in A.ALL_CASES:
        _, _, _, info, ref, e_model, bound = A.reference(c, full=False)
        assert math.isfinite(e_model) and 0 <= e_model <= bound / A.FACTOR and e_model < 2e-2, (c.id, e_model)
        if c.Nk > 1:
            assert e_model > 2.0 ** -14, (c.id, e_model)                # (one key: the output is that key's V row, exactly)
        assert ref.shape == (c.B, c.Nq, c.h * c.d) and bool(torch.isfinite(ref).all())
        for x in (info["qb"], info["kb"], info["vb"]):                  # finite fp16 values (x 1, 2, 4 for v: still fp16)
            assert torch.equal(x, x.half().float()) and bool(torch.isfinite(x).all()) and float(x.abs().max()) < 1024


def test_assembled_reference_equals_the_direct_one():
    """the references of the many-head cases are assembled from the base heads (attn_cases._build): same numbers as the direct form"""
    c = replace(A.XATTN_MULTIBLOCK[0], h=10, Nq=300, period=4)
    q, k, v, info, ref, e_model, bound = A.reference(c)
    assert float((A.ref64(q, k, v) - ref).abs().max()) < 1e-12
    direct = A.max_row_err(A.model(q, k, v), ref, c.d)
    assert abs(direct - e_model) <= 1e-6 * e_model
    assert len(set(info["own"].tolist())) == c.h                        # every head has a planted row of its own


def test_expected_dispatch_of_the_table():
    """the shapes reach the paths their group is named after, by the launcher's own rule restated (xqb: cfgpp_op_attention)"""
    for c in A.ALL_CASES:
        nqb, BH = (c.Nq + 127) // 128, c.B * c.h
        xqb = 1
        while xqb < 8 and nqb % (xqb * 2) == 0 and BH * (nqb // (xqb * 2)) >= 512:
            xqb *= 2
        assert c.kernel == A._kernel_for(c.d, c.Nk, c.dma, c.cross) and c.xqb == (xqb if c.kernel == 3 else 0), c.id
    assert sorted(c.xqb for c in A.XATTN_MULTIBLOCK) == [2] * 3 + [4] * 3 + [8] * 6
    assert [c.grid for c in A.REMAP] == [9, 13, 23, 9, 13]
    assert any(c.grid > 8 and c.grid % 8 for c in A.FLASH_PARTIAL)
    assert sorted(A.HEAD_DIMS_OK + A.HEAD_DIMS_REFUSED) == list(range(8, 161, 8))
