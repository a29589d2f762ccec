"""The case table of tests/vit_attn_cases.py would catch real faults: every fault below is applied to the fp64 model of
vit_attn_kernel (no GPU) and must push its designated cases past their bound - the bound tests/test_gpu_vit_attention.py asserts
for the kernel - at least tenfold.  The honest model stays under bound / FACTOR on every case of the table."""
import pytest
import torch

import vit_attn_cases as V

ids = dict(ids=lambda c: c.id)


def over_bound(c, fault):
    qkv, ref, e_model, bound = V.reference(c)
    assert bound > 0, c.id
    return V.max_row_err(V.model(qkv, c.heads, c.d, fault), ref, c.d) / bound


WITH_PADS = [c for c in V.ALL_CASES if c.T % 32 != 0 and c.T > 1]
PARTIAL_LAST = [c for c in V.ALL_CASES if c.T % 32 != 0 and c.T > 32]
D104 = [c for c in V.ALL_CASES if c.d == 104 and c.T > 1]
MULTI_HEAD = [c for c in V.ALL_CASES if c.heads > 1 and c.T > 1]
MULTI_BLOCK = [c for c in V.ALL_CASES if c.T > 32]
ANY = [c for c in V.ALL_CASES if c.T > 1]


def test_table_covers_what_the_issue_names():
    ts = {c.T for c in V.ALL_CASES if c.d == 104}
    assert ts == {1, 5, 31, 32, 33, 37, 64, 65, 257}
    assert {c.d for c in V.ALL_CASES} == {64, 80, 104}
    for d in (64, 80, 104):
        assert {(c.heads, c.rows) for c in V.ALL_CASES if c.d == d} >= {(1, 1), (2, 2)}
    assert {(c.heads, c.rows) for c in V.ALL_CASES if c.d == 104} == {(1, 1), (2, 2), (2, 1), (1, 2)}
    assert all(c.T <= V.MAX_TOKENS for c in V.ALL_CASES)
    for c in V.ALL_CASES:                                   # a planted key in the last (partial) tile, planted dims 96 .. 103 at d = 104
        assert 32 * ((c.T - 1) // 32) in V.planted_keys(c.T) and c.T - 1 in V.planted_keys(c.T)


@pytest.mark.parametrize("c", V.ALL_CASES, **ids)
def test_honest_model_is_inside_its_own_bound(c):
    qkv, ref, e_model, bound = V.reference(c)
    assert qkv.shape == (c.rows, c.T, 3 * c.heads * c.d) and bool((qkv.half().float() == qkv).all())
    assert 0 <= e_model < 5e-3 and bound == V.FACTOR * e_model
    assert e_model > 0 or c.T == 1          # one token: softmax = 1, the output IS the V row, exactly, in the model and in the kernel


@pytest.mark.parametrize("c", WITH_PADS, **ids)
def test_pad_keys_not_masked(c):
    assert over_bound(c, "pad_leak") >= 10


@pytest.mark.parametrize("c", PARTIAL_LAST, **ids)
def test_last_partial_key_tile_dropped(c):
    assert over_bound(c, "drop_last_tile") >= 10


@pytest.mark.parametrize("c", D104, **ids)
def test_seventh_k_step_not_zero_filled(c):
    assert over_bound(c, "no_zero_fill") >= 10


@pytest.mark.parametrize("c", MULTI_HEAD, **ids)
def test_head_stride_off_by_one_head(c):
    assert over_bound(c, "head_stride") >= 10


@pytest.mark.parametrize("c", ANY, **ids)
def test_k_and_v_columns_swapped(c):
    assert over_bound(c, "kv_swap") >= 10


@pytest.mark.parametrize("c", MULTI_BLOCK, **ids)
def test_query_block_base_off_by_32(c):
    assert over_bound(c, "qblock_off") >= 10


def test_planted_rows_answer_with_their_planted_value_row():
    """the design the faults rely on: a planted row's reference output IS the V row of the key it asks for (which depends on head and
    batch row), to within 1e-6 of the probability mass"""
    c = next(c for c in V.ALL_CASES if c.d == 104 and c.T == 257 and c.heads == 2)
    qkv, ref, _, _ = V.reference(c)
    q, k, v = V.split(qkv, c.heads, c.d)
    keys, rows = V.planted_keys(c.T), V.planted_rows(c.T)
    out = ref.reshape(c.rows, c.T, c.heads, c.d)
    for r in range(c.rows):
        for h in range(c.heads):
            for i, row in enumerate(rows):
                key = keys[(i + row // 32 + 3 * h + r) % len(keys)]
                assert torch.allclose(out[r, row, h], v[r, h, key].double(), atol=1e-3), (r, h, row, key)
