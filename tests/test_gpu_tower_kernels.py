"""-m gpu: the small kernels of the text tower, the image tower and the Resampler - text_embed, text_attn, text_pool (csrc/text.hip),
vit_assemble, vit_cls_rows (csrc/vision.hip), broadcast_rows, gelu_inplace (csrc/resampler.hip) and act_inplace
(csrc/small_kernels.hip) - through the hooks that call the launchers the towers' plans call, against the references of
tests/tower_cases.py, with the harness of tests/test_gpu_vit_attention.py: every destination is NaN-filled between sentinel guard
rows, the guards are checked, a second launch must be bit-identical, a refusal raises by name and leaves the destination untouched.
tests/test_tower_cases_cpu.py shows which faults these conditions catch."""
import numpy as np
import pytest
import torch

import tower_cases as W
from test_gpu_attention import GUARD_ROWS, SENTINEL, guarded, guards_intact
from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu

ids = dict(ids=lambda c: c.id)


def dev(a, dtype):
    import hip_ops as H
    return torch.from_numpy(np.ascontiguousarray(a)).to(H.DEV, dtype).contiguous()


def guarded32(rows, width):
    """test_gpu_attention.guarded for an fp32 destination [rows, width]"""
    import hip_ops as H
    g = GUARD_ROWS * width
    buf = torch.full((2 * g + rows * width,), float("nan"), dtype=torch.float32, device=H.DEV)
    buf[:g] = SENTINEL
    buf[-g:] = SENTINEL
    return buf, buf[g:-g].view(rows, width)


def twice(make, call):
    """two launches into fresh guarded destinations -> (the first destination on the CPU as fp64, problems)"""
    outs = []
    for _ in range(2):
        buf, o, width = make()
        call(o)
        torch.cuda.synchronize()
        outs.append((buf, o, width))
    problems = []
    if not all(guards_intact(buf, width) for buf, _, width in outs):
        problems.append("guard rows written")
    a, b = outs[0][1], outs[1][1]
    it = torch.int16 if a.dtype == torch.float16 else torch.int32
    if not torch.equal(a.view(it), b.view(it)):
        problems.append("second launch differs")
    return a.double().cpu().numpy(), problems


def exact(group, c, got, want, problems):
    ok = W.same_bits(got.reshape(want.shape), want)
    record("tower_case", group=group, case=c.id, exact=ok, problems=problems)
    print(f"{group} {c.id}: exact {ok} {problems}")
    assert not problems, (c.id, problems)
    assert np.isfinite(got).all(), f"{c.id}: {int((~np.isfinite(got)).sum())} elements not finite (unwritten or NaN)"
    assert ok, f"{c.id}: {int((got.reshape(want.shape) != want).sum())} elements differ from the torch restatement"


# ---- causal text attention ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.ATTN, **ids)
def test_text_attention(c):
    need_gpu()
    import hip_ops as H
    qkv, ref, e_model, bound = W.attn_reference(c)
    dq = qkv.to(H.DEV, torch.float16).contiguous()
    got, problems = twice(lambda: guarded(c.B, W.T, c.H) + (c.H,), lambda o: H.text_attention(dq, o, c.B, c.heads, c.H))
    got = torch.from_numpy(got)
    if not bool(torch.isfinite(got).all()):
        problems.append(f"{int((~torch.isfinite(got)).sum())} output elements not finite (unwritten or NaN)")
    err = W.max_row_err(got, ref, W.D)
    _, _, v = W.V.split(qkv, c.heads, W.D)
    row0 = torch.equal(got[:, 0].float(), v[:, :, 0].reshape(c.B, c.H))
    record("tower_case", group="text_attention", case=c.id, e_model=e_model, max_row_err=err, ratio=(err / e_model if e_model else None),
           row0_exact=row0, problems=problems)
    print(f"{c.id}: E_model {e_model:.3e} kernel {err:.3e} bound {bound:.3e} row 0 exact {row0} {problems}")
    assert not problems, (c.id, problems)
    assert err <= bound, f"{c.id}: max row error {err:.3e} > {W.FACTOR:g} x E_model = {bound:.3e}"
    assert row0, f"{c.id}: row 0 is not V[0] bit for bit"


@pytest.mark.parametrize("heads,H,qkv_null,out_null,msg", [(1, 68, 0, 0, "H=68"), (2, 64, 0, 0, "H=64 must be heads=2 x 64"), (3, 128, 0, 0, "must be heads=3"),
                                                           (1, 64, 1, 0, "null operand"), (1, 64, 0, 1, "null operand")])
def test_text_attention_refusals_launch_nothing(heads, H, qkv_null, out_null, msg):
    need_gpu()
    import hip_ops as HO
    from cfgpp_amd._lib import CfgppError
    qkv = torch.zeros((1, W.T, 3 * 192), dtype=torch.float16, device=HO.DEV)
    buf, o = guarded(1, W.T, 192)
    with pytest.raises(CfgppError, match="text_attention.*" + msg):
        HO.text_attention(None if qkv_null else qkv, None if out_null else o, 1, heads, H)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and guards_intact(buf, 192)


# ---- embed, pool, assemble, cls_rows, broadcast_rows: exact ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.EMBED, **ids)
def test_text_embed(c):
    """ids below 0 and at or above vocab (clamped), repeats, 8 .. 128 working threads, one pass and a partial second pass"""
    need_gpu()
    import hip_ops as H
    i = W.embed_inputs(c)
    idd, tok, pos = dev(i["ids"], torch.int32), dev(i["tok"], torch.float16), dev(i["pos"], torch.float16)
    got, problems = twice(lambda: guarded(c.N, W.T, c.H) + (c.H,), lambda o: H.text_embed(idd, tok, pos, o, c.N, c.H, W.VOCAB))
    exact("text_embed", c, got, W.embed_model(c), problems)


@pytest.mark.parametrize("c", W.POOL, **ids)
def test_text_pool(c):
    """EOS positions -1, 0, 76, 77 and 200 (clamped), another one in every batch row"""
    need_gpu()
    import hip_ops as H
    i = W.pool_inputs(c)
    h, eos = dev(i["h"], torch.float16), dev(i["eos"], torch.int32)
    got, problems = twice(lambda: guarded32(c.N, c.H) + (c.H,), lambda o: H.text_pool(h, eos, o, c.N, c.H))
    exact("text_pool", c, got, W.pool_model(c), problems)


@pytest.mark.parametrize("c", W.ASSEMBLE, **ids)
def test_vit_assemble(c):
    need_gpu()
    import hip_ops as H
    i = W.assemble_inputs(c)
    patch, cls, pos = dev(i["patch"], torch.float16), dev(i["cls"], torch.float16), dev(i["pos"], torch.float16)
    got, problems = twice(lambda: guarded(c.N, c.Tk, c.H) + (c.H,), lambda o: H.vit_assemble(patch, cls, pos, o, c.N, c.Tk, c.H))
    exact("vit_assemble", c, got, W.assemble_model(c), problems)


@pytest.mark.parametrize("c", W.CLS_ROWS, **ids)
def test_vit_cls_rows(c):
    need_gpu()
    import hip_ops as H
    x = dev(W.cls_inputs(c)["x"], torch.float16)
    got, problems = twice(lambda: guarded(1, c.N, c.H) + (c.H,), lambda o: H.vit_cls_rows(x, o, c.N, c.Tk, c.H))
    exact("vit_cls_rows", c, got, W.cls_model(c), problems)


@pytest.mark.parametrize("c", W.BROADCAST, **ids)
def test_broadcast_rows(c):
    """one thread, blocks with a tail, fp32 sources that are not fp16 numbers"""
    need_gpu()
    import hip_ops as H
    src = dev(W.broadcast_inputs(c)["src"], torch.float32)
    got, problems = twice(lambda: guarded(1, c.N, c.H) + (c.H,), lambda o: H.broadcast_rows(src, o, c.H, c.N))
    exact("broadcast_rows", c, got, W.broadcast_model(c), problems)


def _refusal_cases():
    """(op, name, message, call(H, ops, dest)) - ops: a dict of valid device operands, dest: the guarded destination"""
    return [
        ("embed", "H%8", "text_embed.*H=12", lambda H, a, o: H.text_embed(a["ids"], a["h16"], a["h16"], o, 1, 12, 5)),
        ("embed", "B0", "text_embed.*B=0", lambda H, a, o: H.text_embed(a["ids"], a["h16"], a["h16"], o, 0, 64, 5)),
        ("embed", "null", "text_embed: null", lambda H, a, o: H.text_embed(None, a["h16"], a["h16"], o, 1, 64, 5)),
        ("assemble", "H%8", "vit_assemble.*H=12", lambda H, a, o: H.vit_assemble(a["h16"], a["h16"], a["h16"], o, 1, 5, 12)),
        ("assemble", "T1", "vit_assemble.*T=1", lambda H, a, o: H.vit_assemble(a["h16"], a["h16"], a["h16"], o, 1, 1, 64)),
        ("assemble", "null", "vit_assemble: null", lambda H, a, o: H.vit_assemble(a["h16"], None, a["h16"], o, 1, 5, 64)),
        ("cls_rows", "H%8", "vit_cls_rows.*H=12", lambda H, a, o: H.vit_cls_rows(a["h16"], o, 1, 5, 12)),
        ("cls_rows", "null", "vit_cls_rows: null", lambda H, a, o: H.vit_cls_rows(None, o, 1, 5, 64)),
        ("broadcast_rows", "n%8", "broadcast_rows: n=12", lambda H, a, o: H.broadcast_rows(a["f32"], o, 12, 1)),
        ("broadcast_rows", "null", "broadcast_rows", lambda H, a, o: H.broadcast_rows(None, o, 8, 1)),
        ("act_inplace", "n%8", "act_inplace: n=12", lambda H, a, o: H.act_inplace(o, 12, 0)),
        ("act_inplace", "act2", "act_inplace: activation 2", lambda H, a, o: H.act_inplace(o, 8, 2)),
        ("act_inplace", "null", "act_inplace: null", lambda H, a, o: H.act_inplace(None, 8, 0)),
        ("gelu_inplace", "n%8", "gelu: n=12", lambda H, a, o: H.gelu_inplace(o, 12)),
    ]


@pytest.mark.parametrize("op,name,msg,call", _refusal_cases(), ids=[f"{r[0]}-{r[1]}" for r in _refusal_cases()])
def test_refusals_launch_nothing(op, name, msg, call):
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    a = dict(ids=torch.zeros((3, W.T), dtype=torch.int32, device=H.DEV), h16=torch.ones((3 * W.T, 64), dtype=torch.float16, device=H.DEV),
             f32=torch.ones(64, dtype=torch.float32, device=H.DEV))
    buf, o = guarded(1, 3 * W.T, 64)
    with pytest.raises(CfgppError, match=msg):
        call(H, a, o)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and guards_intact(buf, 64)


def test_text_pool_refusals_launch_nothing():
    need_gpu()
    import hip_ops as H
    from cfgpp_amd._lib import CfgppError
    h = torch.ones((1, W.T, 64), dtype=torch.float16, device=H.DEV)
    eos = torch.zeros(1, dtype=torch.int32, device=H.DEV)
    buf, o = guarded32(1, 64)
    for args, msg in (((h, None, o, 1, 64), "text_pool: null"), ((h, eos, o, 0, 64), "text_pool: B=0"), ((h, eos, o, 1, 0), "text_pool: B=1 H=0")):
        with pytest.raises(CfgppError, match=msg):
            H.text_pool(*args)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and guards_intact(buf, 64)


# ---- activations -------------------------------------------------------------------------------------------------------------------
def run_act(x, kernel, act):
    """x: fp16 numpy values, n % 8 == 0 -> (the kernel's output as fp64, problems): in place inside a guarded buffer, twice"""
    import hip_ops as H
    n = x.size
    xd = dev(x, torch.float16)

    def make():
        buf, o = guarded(1, n // 8, 8)
        o.view(-1).copy_(xd)
        return buf, o, 8
    got, problems = twice(make, (lambda o: H.act_inplace(o, n, act)) if kernel == "act_inplace" else (lambda o: H.gelu_inplace(o, n)))
    return got.reshape(-1), problems


@pytest.mark.parametrize("kernel,act", [("act_inplace", 0), ("act_inplace", 1), ("gelu_inplace", 1)])
def test_activation_on_every_fp16_value(kernel, act):
    """all 63488 finite fp16 values in one launch (248 blocks), then the launch tails: 1, 255, 256 and 257 threads, whose outputs must
    be the bits the big launch gave for the same inputs"""
    need_gpu()
    x = W.all_fp16()
    got, problems = run_act(x, kernel, act)
    q = W.act_ratio(got, x, act, kernel)
    tails = {}
    for n in W.ACT_TAIL_N:
        g, p = run_act(x[:n], kernel, act)
        problems += [f"n={n}: {m}" for m in p]
        tails[n] = W.same_bits(g, got[:n])
    record("tower_case", group=kernel, case=f"act{act}", ratio=q, tails_exact=tails, problems=problems)
    print(f"{kernel} act {act}: ratio {q:.3f} tails {tails} {problems}")
    assert not problems, problems
    assert np.isfinite(got).all()
    assert q <= 1.0, f"{kernel} act {act}: (|got - ref64| - rounding) / rest = {q:.3f} > 1, " \
                     f"{W.violations(got, W.act_ref64(x, act), *W.act_bound(x, act, kernel))} elements outside the bound"
    assert all(tails.values()), tails
