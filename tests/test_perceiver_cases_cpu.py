"""CPU: the perceiver-attention case tables of tests/perceiver_cases.py cover what they claim, the model of the kernel's rounding
points stays inside its own bound, and every fault the GPU test must catch breaks that bound tenfold on every case where the
fault changes the arithmetic at all.  No HIP."""
import pytest
import torch

import attn_cases as A
import perceiver_cases as P

ids = dict(ids=lambda c: c.id)


@pytest.fixture(autouse=True)
def _one_cpu_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


_REF = {}


def reference(c):
    """one reference per case for the whole module, never modified"""
    if c.id not in _REF:
        _REF[c.id] = P.reference(c)
    return _REF[c.id]


def test_table_coverage():
    T = P.KEY_TILE
    cases = P.ALL_CASES
    assert len({c.id for c in cases}) == len(cases)
    assert {c.rows for c in cases} == {1, 3} and {c.heads for c in cases} == {1, 3}
    assert {c.nq for c in cases} == {1, 4, 16, 17, 32}
    assert all(1 <= c.nq <= P.MAX_Q and 1 <= c.S <= P.MAX_S for c in cases)
    for nq in (1, 4, 16, 17, 32):
        assert {c.S for c in P.SMALL if c.nq == nq} == {1, 2}
    totals = {c.nk for c in P.TILE_EDGES}
    assert totals >= {T - 1, T, T + 1, 2 * T, 2 * T + 1}
    # the tile boundary at key T: inside the image keys, exactly between the sources, inside the latent keys
    assert any(c.S > T and c.nk > T for c in P.TILE_EDGES)
    assert any(c.S == T for c in P.TILE_EDGES)
    assert any(c.S < T < c.nk for c in P.TILE_EDGES) and any(c.S + 8 <= T <= c.nk - 8 for c in P.TILE_EDGES)
    # ... and the one at 2T inside the latent keys
    assert any(c.S < 2 * T < c.nk for c in P.TILE_EDGES)
    assert {257, 577, P.MAX_S} <= {c.S for c in P.REAL}
    for c in cases:                                                  # every case has every plant kind
        assert set(P.plant_kind(c).flatten().tolist()) == {0, 1, 2, 3}, c.id


@pytest.mark.parametrize("c", P.ALL_CASES, **ids)
def test_planted_rows_answer_with_their_key(c):
    (q, k, v), ref, _, _ = reference(c)
    kind = P.plant_kind(c)
    out = ref.reshape(c.rows, c.nq, c.heads, P.D).transpose(1, 2)          # [rows, heads, nq, d]
    for p, t in enumerate(P.plant_targets(c)):
        sel = kind == p
        want = v[:, :, t][:, :, None, :].expand(c.rows, c.heads, c.nq, P.D)[sel].double()
        assert float((out[sel] - want).abs().max()) < 1e-3 * float(want.abs().max()), (c.id, p)


@pytest.mark.parametrize("c", P.ALL_CASES, **ids)
def test_model_within_its_bound(c):
    ins, ref, e_model, bound = reference(c)
    assert 0 < e_model < 5e-3, (c.id, e_model)                 # fp16 output rounding (2^-11) and the rounded P, nothing else
    assert A.max_row_err(P.model(*ins, c.S), ref, P.D) <= bound


def test_layout_round_trip():
    c = P.PCase(3, 3, 4, 5, seed=1)
    q, k, v = P.make_inputs(c)
    tq, kvx, kvl = P.to_kernel_layout(c, q, k, v)
    inner = c.heads * P.D
    assert tq.shape == (3, 4, inner) and kvx.shape == (3, 5, 2 * inner) and kvl.shape == (3, 4, 2 * inner)
    assert torch.equal(tq[2, 1, 64:128], q[2, 1, 1])
    assert torch.equal(kvx[1, 4, 128:192], k[1, 2, 4]) and torch.equal(kvx[1, 4, inner:inner + 64], v[1, 0, 4])
    assert torch.equal(kvl[0, 3, :64], k[0, 0, 5 + 3]) and torch.equal(kvl[0, 3, inner + 64:inner + 128], v[0, 1, 5 + 3])


@pytest.mark.parametrize("fault", P.FAULTS)
def test_faults_break_the_bound_tenfold(fault):
    seen = 0
    for c in P.ALL_CASES:
        if not P.fault_applies(fault, c):
            continue
        ins, ref, e_model, bound = reference(c)
        err = A.max_row_err(P.model(*ins, c.S, fault=fault), ref, P.D)
        assert err > 10 * bound, f"{fault} on {c.id}: error {err:.3e} is not above 10 x bound = {10 * bound:.3e}"
        seen += 1
    assert seen >= 5, fault
