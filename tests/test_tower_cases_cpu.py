"""No GPU: what tests/tower_cases.py claims, and what the conditions of tests/test_gpu_tower_kernels.py can see.

D1  the tables hold every value the issue lists and reach every branch of the launchers (threads idle, one pass, a partial second
    pass; every head kind; every edge id and EOS position); the inputs have the properties the docstring claims.
D2  the model of a correct kernel passes its own condition on every case.
D3  every fault model fails on at least one case; the test names the cases (a fault that no case sees fails the test by name).
D4  refusals return the error code with the launcher's name before anything could be launched."""
import ctypes
import math

import numpy as np
import pytest
import torch

import tower_cases as W

ids = dict(ids=lambda c: c.id)


# ---- D1 -----------------------------------------------------------------------------------------------------------------------
def test_tables():
    for cases in (W.ATTN, W.EMBED, W.POOL, W.ASSEMBLE, W.CLS_ROWS, W.BROADCAST):
        assert len({c.id for c in cases}) == len(cases)
    assert {(c.heads, c.B) for c in W.ATTN} == {(1, 1), (2, 3), (12, 1), (20, 2)} and sum(c.big for c in W.ATTN) == 1
    for c in W.ATTN:
        kinds = {W.head_kind(c, b, h) for b in range(c.B) for h in range(c.heads)}
        assert kinds == ({"planted"} if c.heads == 1 or c.big else set(W.KINDS)), c.id
    for cases in (W.EMBED, W.POOL, W.ASSEMBLE, W.CLS_ROWS):
        assert {c.H for c in cases} == set(W.H_VALUES) and {c.N for c in cases} == {1, 3}
        assert {(c.H, c.N) for c in cases} >= {(H, N) for H in W.H_VALUES for N in (1, 3)}
    assert {c.H for c in W.BROADCAST} >= set(W.H_VALUES) and {c.N for c in W.BROADCAST} == {1, 3}
    # 64: 8 of 128 threads work; 1024: exactly one full pass; 1088 / 1280 / 1664: a partial second pass
    assert W.row_passes(64) == (8, 1, True) and W.row_passes(768) == (96, 1, True) and W.row_passes(1024) == (128, 1, False)
    assert [W.row_passes(H)[1:] for H in (1088, 1280, 1664)] == [(2, True)] * 3
    assert {c.Tk for c in W.ASSEMBLE} == set(W.ASSEMBLE_T) and {(c.Tk, c.N) for c in W.ASSEMBLE} >= {(257, 3), (2, 1), (2, 3)}
    # broadcast_rows / act: one thread, a block less one thread, exactly a block, a block and one thread
    assert {n // 8 for n in W.ACT_TAIL_N} == {1, 255, 256, 257}
    assert {c.H * c.N // 8 for c in W.BROADCAST} >= {1, 3, 3 * 257}


def test_embed_and_pool_inputs_hold_every_edge():
    seen = set()
    for c in W.EMBED:
        i = W.embed_inputs(c)["ids"]
        assert set(W.EDGE_IDS) <= set(i.reshape(-1).tolist()) and i[-1, -1] == W.VOCAB + 7
        assert (i[:, 5] == i[:, 6]).all()                                      # a repeat
    for c in W.POOL:
        e = W.pool_inputs(c)["eos"].tolist()
        assert len(set(e)) == len(e)
        seen |= set(e)
    assert seen == set(W.EDGE_EOS) | {40}
    assert {-5, 0, W.VOCAB - 1, W.VOCAB, W.VOCAB + 7} == set(W.EDGE_IDS) - {3}


@pytest.mark.parametrize("c", W.ATTN, **ids)
def test_attention_inputs_have_the_planted_structure(c):
    qkv, ref, e_model, bound = W.attn_reference(c)
    q, k, v = W.V.split(qkv, c.heads, W.D)
    s = W.attn_scores64(qkv, c.heads)
    ordinary = [j for j in range(W.T) if j not in W.planted_key_set()]
    assert bool(((k[..., :8] - k[..., 8:56].mean(-1, keepdim=True)).abs() > 2.0).all()) and bool((v[..., :8].abs() >= 7.0).all())          # the decoys, in EVERY head's columns
    for b in range(c.B):
        for h in range(c.heads):
            kind, sh = W.head_kind(c, b, h), s[b, h]
            if kind == "planted":
                for t, r in enumerate(W.PLANT_ROWS):
                    mine = W.plant_keys(r)
                    assert float(sh[r, mine].min()) > float(sh[r, [j for j in range(W.T) if j not in mine]].max()) + 25, (c.id, b, h, r)
                    assert r in mine and 0 in mine and 76 in mine and min(r + 1, 76) in mine
                rows = [r for r in range(W.T) if r not in W.PLANT_ROWS]
                gap = sh[rows][:, ordinary].median() - sh[rows][:, W.planted_key_set()].median()
                assert 10 * (32 if c.big else 1) < float(gap) < 18 * (32 if c.big else 1), (c.id, float(gap))
            else:
                d = sh[:, 1:] - sh[:, :-1]
                assert bool((d > 2).all() if kind == "rising" else (d < -2).all()), (c.id, b, h, float(d.abs().min()))
                assert float(sh.abs().max()) > 1e3
    if c.big:
        assert float(s[:, :, list(W.PLANT_ROWS)].abs().max()) > 1e3
    assert math.isfinite(e_model) and 0 < e_model < 2e-3, e_model
    # row 0 sees key 0 alone: V[0] bit for bit, in the reference's rounding and in the model
    v0 = v[:, :, 0].reshape(c.B, c.H)
    assert torch.equal(W.attn_model(qkv, c.heads)[:, 0].float(), v0)
    assert torch.equal(ref[:, 0].float(), v0)
    # the reference is causal: another V row at the last key moves row 76 and no other
    qkv2 = qkv.clone()
    qkv2[:, W.T - 1, 2 * c.H:] += 1.0
    moved = (W.attn_ref64(qkv2, c.heads) != ref).reshape(c.B, W.T, -1).any(-1)
    assert bool(moved[:, W.T - 1].all()) and not bool(moved[:, :W.T - 1].any())


# ---- D2 / D3 --------------------------------------------------------------------------------------------------------------------
def test_attention_model_passes_and_every_fault_is_seen():
    seen = {f: [] for f in W.ATTN_FAULTS}
    for c in W.ATTN:
        qkv, ref, e_model, bound = W.attn_reference(c)
        assert W.max_row_err(W.attn_model(qkv, c.heads), ref, W.D) <= bound
        for f in W.ATTN_FAULTS:
            err = W.max_row_err(W.attn_model(qkv, c.heads, f), ref, W.D)
            if err > bound:
                seen[f].append(c.id)
    print("attention faults seen by:", seen)
    assert all(seen.values()), {f: v for f, v in seen.items() if not v}
    # the faults that do not depend on a second head are seen by every case
    for f in ("future_key", "no_diagonal", "scale1", "acc_not_rescaled", "l_not_rescaled", "kv_swap", "last_row_dropped"):
        assert len(seen[f]) == len(W.ATTN), (f, seen[f])
    assert set(seen["next_head_k"]) == {c.id for c in W.ATTN if c.heads > 1}


@pytest.mark.parametrize("op", sorted(W.GLUE))
def test_exact_models_and_their_faults(op):
    cases, model, faults = W.GLUE[op]
    seen = {f: [] for f in faults}
    for c in cases:
        want = model(c)
        assert W.same_bits(want, want) and want.shape[-1] == c.H
        for f in faults:
            if not W.same_bits(model(c, f), want):
                seen[f].append(c.id)
    print(op, "faults seen by:", seen)
    assert all(seen.values()), {f: v for f, v in seen.items() if not v}
    if op == "embed":
        assert len(seen["no_clamp"]) == len(cases) and set(seen["pos_row"]) == {c.id for c in cases if c.N > 1}
    if op == "assemble":
        assert len(seen["t_not_minus_1"]) == len(cases) and len(seen["cls_pos1"]) == len(cases)
        assert set(seen["patch_stride"]) == set(seen["pos_row"]) == {c.id for c in cases if c.N > 1}
    if op == "pool":
        assert set(seen["one_eos"]) == {c.id for c in cases if c.N > 1}


def test_same_bits_sees_signed_zeros_and_unwritten_elements():
    a = np.array([0.0, 1.0])
    assert W.same_bits(a, a) and not W.same_bits(np.array([-0.0, 1.0]), a) and not W.same_bits(np.array([0.0, np.nan]), a)


def test_activation_models_pass_and_every_fault_is_seen():
    x = W.all_fp16()
    assert x.size == 63488 and x.size % 8 == 0 and len(set(x.view(np.uint16).tolist())) == 63488
    for act in (0, 1):
        q = W.act_ratio(W.act_model32(x, act), x, act)
        print(f"act {act}: model ratio {q:.3f}")
        assert q <= 1.0, (act, q)
        for n in W.ACT_TAIL_N:
            assert W.act_ratio(W.act_model32(x[:n], act), x[:n], act) <= 1.0
    seen = {}
    for f, acts in (("const_1.7", (0,)), ("sigmoid_of_x", (0,)), ("tanh_gelu", (1,)), ("act_inverted", (0, 1))):
        seen[f] = [act for act in acts if W.act_ratio(W.act_model32(x, act, f), x, act) > 1.0]
        assert seen[f] == list(acts), (f, seen[f])
    assert set(seen) == set(W.ACT_FAULTS)
    # the Resampler's GELU is another function in the last bits: inside its own bound, outside act 1's bits
    g = W.gelu_model32(x)
    q = W.act_ratio(g, x, 1, "gelu_inplace")
    print(f"gelu_inplace: model ratio {q:.3f}")
    assert q <= 1.0
    assert not W.same_bits(g, W.act_model32(x, 1))
    # ... and that bound discriminates: the tanh form and quick_gelu in its place fail it
    for f in ("tanh_gelu", "act_inverted"):
        qf = W.act_ratio(W.act_model32(x, 1, f), x, 1, "gelu_inplace")
        print(f"gelu_inplace bound, fault {f}: ratio {qf:.1f}")
        assert qf > 1.0, (f, qf)


def test_activation_reference_signs_and_tails():
    x = np.array([-65504.0, -100.0, -20.0, -0.0, 0.0, 6e-8, 65504.0])
    for act in (0, 1):
        r = W.act_ref64(x, act)
        assert np.signbit(r[:4]).all() and not np.signbit(r[4:]).any() and r[0] == 0 and r[-1] == 65504.0
        m = W.act_model32(x, act)
        assert np.signbit(m[:4]).all() and (m[:3] == 0).all() and m[-1] == 65504.0
    # a zero of the wrong sign is a failure
    bad = W.act_model32(x, 0)
    bad[0] = 0.0
    assert W.act_ratio(bad, x, 0) == math.inf


# ---- D4 -----------------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_error_code_before_any_launch():
    """none of these calls may touch the device: the pointers are small integers no kernel could read"""
    from cfgpp_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)

    def refused(rc, word):
        msg = lib.cfgpp_last_error()
        assert rc != 0 and word in msg, (rc, msg)

    R = W.GLUE_REFUSED
    calls = dict(
        embed={"H%8": (p, p, p, p, 1, 12, 5), "B0": (p, p, p, p, 0, 64, 5), "vocab0": (p, p, p, p, 1, 64, 0), "null_ids": (None, p, p, p, 1, 64, 5),
               "null_x": (p, p, p, None, 1, 64, 5)},
        pool={"H0": (p, p, p, 1, 0), "B0": (p, p, p, 0, 64), "null_eos": (p, None, p, 1, 64), "null_out": (p, p, None, 1, 64)},
        assemble={"H%8": (p, p, p, p, 1, 5, 12), "T1": (p, p, p, p, 1, 1, 64), "N0": (p, p, p, p, 0, 5, 64), "null_cls": (p, None, p, p, 1, 5, 64),
                  "null_x": (p, p, p, None, 1, 5, 64)},
        cls_rows={"H%8": (p, p, 1, 5, 12), "T0": (p, p, 1, 0, 64), "N0": (p, p, 0, 5, 64), "null_dst": (p, None, 1, 5, 64)},
        broadcast_rows={"n%8": (p, p, 12, 1), "rows0": (p, p, 8, 0), "null_src": (None, p, 8, 1), "null_dst": (p, None, 8, 1)},
        act_inplace={"n%8": (p, 12, 0), "n0": (p, 0, 0), "act2": (p, 8, 2), "null_x": (None, 8, 0)},
        gelu_inplace={"n%8": (p, 12), "n0": (p, 0), "null_x": (None, 8)})
    fn = dict(embed=(lib.cfgpp_op_text_embed, b"text_embed"), pool=(lib.cfgpp_op_text_pool, b"text_pool"),
              assemble=(lib.cfgpp_op_vit_assemble, b"vit_assemble"), cls_rows=(lib.cfgpp_op_vit_cls_rows, b"vit_cls_rows"),
              broadcast_rows=(lib.cfgpp_op_broadcast_rows, b"broadcast_rows"), act_inplace=(lib.cfgpp_op_act_inplace, b"act_inplace"),
              gelu_inplace=(lib.cfgpp_op_gelu_inplace, b"gelu"))
    assert set(calls) == set(R) == set(fn)
    for op, table in calls.items():
        assert set(table) == set(R[op]), op
        for name, args in table.items():
            refused(fn[op][0](*args, None), fn[op][1])
    attn = {"H%8": (p, p, 1, 1, 68), "H!=64heads": (p, p, 1, 2, 64), "B0": (p, p, 0, 1, 64), "null_qkv": (None, p, 1, 1, 64), "null_out": (p, None, 1, 1, 64)}
    assert set(attn) == set(W.ATTN_REFUSED)
    for name, args in attn.items():
        refused(lib.cfgpp_op_text_attention(*args, None), b"text_attention")
