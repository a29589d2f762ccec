"""IP-Adapter without a GPU: (1) the CPU model of the decoupled cross-attention (tests/attn_ip_cases.py) and the bound the GPU
tests use - every fault model must exceed 10 x FACTOR x E_model; (2) the checkpoint parser (cfgpp_amd/ip_adapter.py); (3) the solver
interface on the mock engine with image tokens (tests/ip_adapter_mock.py)."""
import types

import pytest
import torch

import attn_cases as A
import attn_ip_cases as I
from mock_engine import StubVAE

ids = dict(ids=lambda c: c.id)


@pytest.fixture(autouse=True)
def _one_cpu_thread():
    """the references are many tiny fp64 matmuls: torch's intra-op thread pool costs ~100x its benefit there"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# ---- (1) the attention model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", I.FAULT_CASES, **ids)
def test_bound_sees_every_fault(c):
    """neg-kind inputs with planted keys: each fault that changes the arithmetic of case c is more than tenfold the bound"""
    q, k, v, ki, vi, _ = I.make_ip_inputs(c)
    ref = I.ref_ip(q, k, v, ki, vi, c.scale)
    e_model = A.max_row_err(I.model_ip(q, k, v, ki, vi, c.scale, two_pass=not c.fused), ref, c.d)
    assert 0 < e_model < 2e-3, e_model                  # a handful of fp16 roundings
    bound = A.FACTOR * e_model
    seen = 0
    for fault in I.FAULTS:
        if not I.fault_applies(fault, c):
            continue
        err = A.max_row_err(I.model_ip(q, k, v, ki, vi, c.scale, two_pass=not c.fused, fault=fault), ref, c.d)
        assert err > 10 * bound, f"{c.id} {fault}: {err:.3e} is only {err / bound:.1f} x the bound {bound:.3e}"
        seen += 1
    assert seen >= 4


def test_every_fault_is_exercised():
    for fault in I.FAULTS:
        assert any(I.fault_applies(fault, c) for c in I.FAULT_CASES), fault


def test_model_without_image_branch_is_the_text_model():
    """scale 0: model_ip is attn_cases.model on the text keys"""
    c = I.FAULT_CASES[0]
    q, k, v, ki, vi, _ = I.make_ip_inputs(c)
    assert torch.equal(I.model_ip(q, k, v, ki, vi, 0.0), A.model(q, k, v))
    assert torch.equal(I.model_ip(q, k, v, ki, vi, c.scale, fault="img_dropped"), A.model(q, k, v))


def test_assembled_reference_equals_the_direct_one():
    """reference_ip computes base heads + own rows (as attn_cases.reference): same numbers as the direct evaluation"""
    c = I.IPCase(1, 40, 100, 77, 4, 40, scale=0.6, seed=9)           # 40 heads on 32 base heads
    ins, info, ref, e_model, bound = I.reference_ip(c)
    direct = I.ref_ip(*ins, c.scale)
    assert A.max_row_err(direct, ref, c.d) < 1e-12


def test_gpu_case_tables_cover_the_branches():
    assert {c.d for c in I.FUSED_SMALL} == {40, 56, 64} and {c.n_img for c in I.FUSED_SMALL} == {1, 4, 16, 31, 32}
    assert {c.nk_text for c in I.FUSED_SMALL} == {1, 33, 77, 96} and {c.scale for c in I.FUSED_SMALL} == {0.6, 1.0}
    assert {(c.B * c.h, c.Nq, c.xqb) for c in I.FUSED_MULTIBLOCK} == {(128, 1000, 2), (512, 1024, 8)}
    assert all(c.grid > 8 and c.grid % 8 for c in I.FUSED_REMAP)
    assert {c.d for c in I.TWO_PASS} == {32, 80, 160} and all(not c.fused for c in I.TWO_PASS)
    assert all(c.fused for g in (I.FUSED_SMALL, I.FUSED_MULTIBLOCK, I.FUSED_REMAP) for c in g)


# ---- (2) the parser ---------------------------------------------------------------------------------------------------------
def test_block_table_sd15_and_sdxl():
    from cfgpp_amd.ip_adapter import block_table
    from cfgpp_amd.unet_config import SD15, SDXL
    t = block_table(SD15)
    assert [i for i, _ in t] == list(range(1, 32, 2)) and len(t) == 16
    assert t[0] == (1, "down_blocks.0.attentions.0.transformer_blocks.0")
    assert t[5] == (11, "down_blocks.2.attentions.1.transformer_blocks.0")
    assert t[6] == (13, "up_blocks.1.attentions.0.transformer_blocks.0")
    assert t[14] == (29, "up_blocks.3.attentions.2.transformer_blocks.0")
    assert t[15] == (31, "mid_block.attentions.0.transformer_blocks.0")          # the mid block LAST
    x = block_table(SDXL)
    assert [i for i, _ in x] == list(range(1, 140, 2)) and len(x) == 70
    assert x[0] == (1, "down_blocks.1.attentions.0.transformer_blocks.0")
    assert x[24] == (49, "up_blocks.0.attentions.0.transformer_blocks.0")
    assert x[59] == (119, "up_blocks.1.attentions.2.transformer_blocks.1")
    assert [n for _, n in x[60:]] == [f"mid_block.attentions.0.transformer_blocks.{k}" for k in range(10)] and x[60][0] == 121


def _synthetic(cfg_name="tiny_sd", **kw):
    from cfgpp_amd.ip_adapter import synthetic_ip_adapter
    from cfgpp_amd.unet_config import CONFIGS
    return CONFIGS[cfg_name], synthetic_ip_adapter(CONFIGS[cfg_name], **kw)


def test_parse_nested_flat_and_safetensors(tmp_path):
    from safetensors.torch import save_file
    from cfgpp_amd.ip_adapter import block_table, parse_ip_adapter
    cfg, nested = _synthetic(n_img=4, embed_dim=128)
    flat = {f"{g}.{k}": v for g in nested for k, v in nested[g].items()}
    a, b = parse_ip_adapter(nested, cfg), parse_ip_adapter(flat, cfg)
    path = str(tmp_path / "ip.safetensors")
    save_file({k: v.contiguous() for k, v in flat.items()}, path)
    c = parse_ip_adapter(path, cfg)
    for p in (a, b, c):
        assert (p.n_img, p.embed_dim) == (4, 128)
        assert set(p) == set(a) and all(torch.equal(p[k], a[k]) for k in a)
    table = block_table(cfg)
    assert len(a) == 4 + 2 * len(table)
    i, name = table[-1]
    assert name.startswith("mid_block") and torch.equal(a[name + ".attn2.to_v_ip.weight"], nested["ip_adapter"][f"{i}.to_v_ip.weight"])
    i, name = table[2]
    assert torch.equal(a[name + ".attn2.to_k_ip.weight"], nested["ip_adapter"][f"{i}.to_k_ip.weight"])


def test_parser_refusals():
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.ip_adapter import parse_ip_adapter
    from cfgpp_amd.unet_config import TINY_XL
    cfg, nested = _synthetic()
    plus = {"image_proj": dict(nested["image_proj"], latents=torch.zeros(1, 16, 64)), "ip_adapter": nested["ip_adapter"]}
    with pytest.raises(CfgppError, match=r"Resampler.*image_proj\.latents"):
        parse_ip_adapter(plus, cfg)
    face = {"image_proj": {"proj.0.weight": torch.zeros(8, 8)}, "ip_adapter": nested["ip_adapter"]}
    with pytest.raises(CfgppError, match=r"FaceID.*image_proj\.proj\.0\.weight"):
        parse_ip_adapter(face, cfg)
    fewer = {"image_proj": nested["image_proj"], "ip_adapter": {k: v for k, v in nested["ip_adapter"].items() if not k.startswith("1.")}}
    with pytest.raises(CfgppError, match="block count"):
        parse_ip_adapter(fewer, cfg)
    with pytest.raises(CfgppError, match="cross_dim|cross_attention_dim|block count"):
        parse_ip_adapter(nested, TINY_XL)               # another UNet: cross_dim 64 vs 128
    _, wrong = _synthetic("tiny_xl")
    with pytest.raises(CfgppError, match="cross_attention_dim 64"):
        parse_ip_adapter(wrong, cfg)
    _, many = _synthetic(n_img=32)
    many["image_proj"]["proj.weight"] = torch.zeros(33 * 64, 64)
    with pytest.raises(CfgppError, match="33 image tokens"):
        parse_ip_adapter(many, cfg)


def test_assemble_embeds_rows():
    from cfgpp_amd.ip_adapter import assemble_embeds
    e = torch.randn(1, 8)
    r = assemble_embeds(e, None, 3)
    assert r.shape == (6, 8) and r.dtype == torch.float16
    assert bool((r[:3] == 0).all()) and all(torch.equal(r[3 + i], e[0].half()) for i in range(3))      # zeros first, then B copies
    n = torch.randn(2, 8)
    r = assemble_embeds(torch.randn(2, 8), n, 2)
    assert torch.equal(r[:2], n.half())


def test_preprocess_image_geometry():
    from cfgpp_amd.ip_adapter import CLIP_MEAN, CLIP_STD, preprocess_image
    x = preprocess_image(torch.full((1, 3, 300, 500), 0.5))
    assert x.shape == (1, 3, 224, 224)
    for ch in range(3):
        assert torch.allclose(x[0, ch], torch.full((224, 224), (0.5 - CLIP_MEAN[ch]) / CLIP_STD[ch]), atol=1e-5)


# ---- (3) the solvers on the mock engine -------------------------------------------------------------------------------------
def _solver(name, model="sd15", adapter="synthetic", **kw):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    from cfgpp_amd.weights import synth_state_dict
    from ip_adapter_mock import IPMockEngine
    if model == "sd15":
        from cfgpp_amd.latent_diffusion import get_solver
        cfg = TINY_SD
    else:
        from cfgpp_amd.latent_sdxl import get_solver
        cfg = TINY_XL
    eng = IPMockEngine(cfg, synth_state_dict(cfg, 0), (8, 8))
    s = get_solver(name, solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", unet_config=cfg, max_batch=2,
                   latent_hw=(8, 8), engine=eng, vae=StubVAE(cfg.vae_scale), ip_adapter=adapter, **kw)
    return s, eng, cfg


def _kw(model):
    if model == "sd15":
        return dict(cfg_guidance=0.6, prompt=["", ["a cat", "a dog"]], seeds=[1, 2], return_latents=True)
    return dict(prompt1=["", ["a cat", "a dog"]], prompt2=["", ["a cat", "a dog"]], cfg_guidance=0.6, target_size=(64, 64),
                original_size=(64, 64), seeds=[1, 2], return_latents=True)


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_ddim_cfgpp_with_image_prompt(model):
    s, eng, cfg = _solver("ddim_cfg++", model)
    E = eng.ip_adapter.embed_dim
    emb = torch.randn(1, E, generator=torch.Generator().manual_seed(5))
    plain = s.sample(**_kw(model))
    assert eng.image_calls in ([], [(None, 0.0)])
    n = len(eng.image_calls)
    zero = s.sample(ip_adapter_image_embeds=emb, ip_adapter_scale=0, **_kw(model))
    for x, y in zip(plain, zero):
        assert torch.equal(x, y)                        # scale 0: the no-adapter latents, bit for bit
    with_ip = s.sample(ip_adapter_image_embeds=emb, ip_adapter_scale=0.8, **_kw(model))
    rows, scale = [c for c in eng.image_calls[n:] if c[0] is not None][-1]
    assert scale == 0.8 and rows.shape == (4, E)
    assert bool((rows[:2] == 0).all())                  # default negative embeds: zeros
    assert torch.equal(rows[2], emb[0].half()) and torch.equal(rows[3], emb[0].half())       # B = 1 broadcasts to both chains
    assert not torch.equal(with_ip[0], plain[0])
    again = s.sample(**_kw(model))                      # the next call without an image prompt: adapter off
    assert eng.image_calls[-1] == (None, 0.0)
    for x, y in zip(plain, again):
        assert torch.equal(x, y)
    neg = torch.randn(1, E, generator=torch.Generator().manual_seed(6))
    s.sample(ip_adapter_image_embeds=emb, negative_ip_adapter_image_embeds=neg, **_kw(model))
    rows, scale = [c for c in eng.image_calls if c[0] is not None][-1]
    assert scale == 1.0 and torch.equal(rows[0], neg[0].half()) and torch.equal(rows[1], neg[0].half())


def test_image_prompt_without_adapter_is_an_error():
    s, eng, cfg = _solver("ddim_cfg++", adapter=None)
    with pytest.raises(ValueError, match="no IP-Adapter"):
        s.sample(ip_adapter_image_embeds=torch.zeros(1, 64), **_kw("sd15"))


def test_set_ip_adapter_none_drops_it():
    s, eng, cfg = _solver("ddim_cfg++")
    s.set_ip_adapter(None)
    assert eng.ip_adapter is None
    with pytest.raises(ValueError, match="no IP-Adapter"):
        s.sample(ip_adapter_image_embeds=torch.zeros(1, 64), **_kw("sd15"))


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_sharded_runs_refuse_image_prompts(model, monkeypatch):
    """world size > 1 (dist.py): the per-chain embeds are not sharded, so the call is refused before anything reaches the engine;
    an initialised group of one process is not a sharded run"""
    import torch.distributed as dist
    s, eng, cfg = _solver("ddim_cfg++", model)
    emb = torch.zeros(1, eng.ip_adapter.embed_dim)
    monkeypatch.setattr(dist, "is_available", lambda: True)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    n = len(eng.image_calls)
    with pytest.raises(ValueError, match=r"not supported in sharded runs \(world size > 1\)"):
        s.sample(ip_adapter_image_embeds=emb, **_kw(model))
    assert not [c for c in eng.image_calls[n:] if c[0] is not None]
    s.sample(**_kw(model))                              # no image prompt: a sharded run is served as before
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 1)
    s.sample(ip_adapter_image_embeds=emb, **_kw(model))
    assert [c for c in eng.image_calls[n:] if c[0] is not None]


@pytest.mark.parametrize("model,name", [("sd15", "ddim_inversion_cfg++"), ("sd15", "ddim_edit"), ("sdxl", "ddim_edit_cfg++"),
                                        ("sdxl", "ddim_inversion_cfg++")])
def test_inversion_and_edit_refuse_image_prompts(model, name):
    s, eng, cfg = _solver(name, model)
    with pytest.raises(ValueError, match="does not take ip_adapter_image_embeds"):
        s.sample(ip_adapter_image_embeds=torch.zeros(1, eng.ip_adapter.embed_dim))
    assert not [c for c in eng.image_calls if c[0] is not None]


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_inpaint_refuses_image_prompts(model):
    from cfgpp_amd.inpaint import get_inpaint_solver
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    from cfgpp_amd.weights import synth_state_dict
    from ip_adapter_mock import IPMockEngine
    cfg = TINY_SD if model == "sd15" else TINY_XL
    s = get_inpaint_solver("ddim_inpaint_cfg++", model, solver_config=types.SimpleNamespace(num_sampling=2), device="cpu",
                           unet_config=cfg, latent_hw=(8, 8), engine=IPMockEngine(cfg, synth_state_dict(cfg, 0), (8, 8)),
                           vae=StubVAE(cfg.vae_scale))
    with pytest.raises(ValueError, match="does not take ip_adapter_image_embeds"):
        s.sample(prompt=["", "a cat"], src_img=torch.zeros(1, 3, 64, 64), mask=torch.ones(1, 1, 64, 64),
                 ip_adapter_image_embeds=torch.zeros(1, 64))


# ---- (4) the extension header ------------------------------------------------------------------------------------------------
def test_extension_header_is_exported_and_bound():
    """include/cfgpp_ip_adapter.h: every declaration is exported by the library and has a ctypes prototype in its own table"""
    import os
    import re
    from cfgpp_amd import _lib
    from cfgpp_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cfgpp_ip_adapter.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cfgpp_[a-z0-9_]+)\s*\(", code))
    assert declared == {"cfgpp_unet_ip_load", "cfgpp_unet_image_context"} == set(_lib.IP_ADAPTER_PROTOTYPES)
    assert all(hasattr(lib, n) for n in declared)
    for word in ("IPAdapterAttnProcessor2_0.__call__", "ImageProjection.forward", "unet.encoder_hid_proj", "No reference counterpart"):
        assert word in hdr, word


# ---- (5) the command line -----------------------------------------------------------------------------------------------------
def test_text_to_img_cli_with_ip_adapter(tmp_path):
    import os
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import text_to_img
    from cfgpp_amd.unet_config import TINY_SD
    from cfgpp_amd.weights import synth_state_dict
    from ip_adapter_mock import IPMockEngine
    eng = IPMockEngine(TINY_SD, synth_state_dict(TINY_SD, 0), (8, 8))
    emb = np.random.RandomState(0).randn(1, 64).astype(np.float32)
    np.save(tmp_path / "e.npy", emb)
    common = ["--method", "ddim_cfg++", "--cfg_guidance", "0.6", "--NFE", "2", "--prompt", "a cat", "--device", "cpu", "--workdir", str(tmp_path)]
    kw = dict(engine=eng, vae=StubVAE(0.18215), latent_hw=(8, 8), unet_config=TINY_SD)
    text_to_img.main(common + ["--ip_adapter", "synthetic:0.5", "--ip_embeds", str(tmp_path / "e.npy")], solver_kwargs=kw)
    rows, scale = [c for c in eng.image_calls if c[0] is not None][-1]
    assert scale == 0.5 and rows.shape == (2, 64) and torch.equal(rows[1], torch.from_numpy(emb[0]).half())
    assert (tmp_path / "result" / "generated.png").exists()
    with pytest.raises(SystemExit, match="need --ip_adapter"):
        text_to_img.main(common + ["--ip_embeds", str(tmp_path / "e.npy")], solver_kwargs=kw)
    with pytest.raises(SystemExit, match="exactly one of"):
        text_to_img.main(common + ["--ip_adapter", "synthetic"], solver_kwargs=kw)
    with pytest.raises(SystemExit, match="--ip_adapter_dir"):
        text_to_img.main(common + ["--ip_adapter", "synthetic", "--ip_image", "x.png"], solver_kwargs=kw)
