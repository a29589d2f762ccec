"""IP-Adapter Plus (Resampler image projection) without a GPU: the checkpoint parser and its refusals, the 3-D embeds assembly,
the image tower's hidden states, the solver interface on the mock engine (tests/ip_plus_mock.py), the extension header and the
command line."""
import types

import pytest
import torch

from mock_engine import StubVAE


def _plus(cfg_name="tiny_sd", **kw):
    from cfgpp_amd.ip_adapter import synthetic_ip_adapter
    from cfgpp_amd.unet_config import CONFIGS
    return CONFIGS[cfg_name], synthetic_ip_adapter(CONFIGS[cfg_name], kind="plus", **kw)


# ---- (1) the parser ---------------------------------------------------------------------------------------------------------
def test_parse_nested_flat_and_safetensors(tmp_path):
    from safetensors.torch import save_file
    from cfgpp_amd.ip_adapter import block_table, parse_ip_adapter
    cfg, nested = _plus()
    flat = {f"{g}.{k}": v for g in nested for k, v in nested[g].items()}
    a, b = parse_ip_adapter(nested, cfg), parse_ip_adapter(flat, cfg)
    path = str(tmp_path / "plus.safetensors")
    save_file({k: v.contiguous() for k, v in flat.items()}, path)
    c = parse_ip_adapter(path, cfg)
    for p in (a, b, c):
        assert (p.kind, p.seq_input, p.n_img, p.embed_dim, p.hidden_dim, p.heads, p.depth, p.ff_inner) == ("resampler", True, 16, 128, 128, 2, 2, 512)
        assert set(p) == set(a) and all(torch.equal(p[k], a[k]) for k in a)
    assert len(a) == 7 + 11 * 2 + 2 * len(block_table(cfg))
    assert torch.equal(a["image_proj.layers.1.0.to_kv.weight"], nested["image_proj"]["layers.1.0.to_kv.weight"])
    assert a["image_proj.latents"].shape == (1, 16, 128)
    lat = a["image_proj.latents"]
    assert 0.5 < float(lat.std()) * 128 ** 0.5 < 2.0            # latents ~ D^-1/2


@pytest.mark.parametrize("geo", [dict(n_img=16, embed_dim=1280, hidden_dim=768, heads=12, depth=4, cross=768),
                                 dict(n_img=16, embed_dim=1280, hidden_dim=1280, heads=20, depth=4, cross=2048),
                                 dict(n_img=1, embed_dim=64, hidden_dim=64, heads=1, depth=1, cross=None),
                                 dict(n_img=32, embed_dim=192, hidden_dim=256, heads=3, depth=8, cross=None)])
def test_geometry_is_read_from_the_checkpoint(geo):
    """the shipped plus geometries (SD1.5: D 768, 12 heads; SDXL vit-h: D 1280, 20 heads, cross 2048) and the extremes"""
    import dataclasses
    from cfgpp_amd.ip_adapter import parse_ip_adapter, synthetic_ip_adapter
    from cfgpp_amd.unet_config import TINY_SD
    geo = dict(geo)
    cross = geo.pop("cross")
    cfg = TINY_SD if cross is None else dataclasses.replace(TINY_SD, cross_attention_dim=cross)
    p = parse_ip_adapter(synthetic_ip_adapter(cfg, kind="plus", **geo), cfg)
    assert (p.n_img, p.embed_dim, p.hidden_dim, p.heads, p.depth) == (geo["n_img"], geo["embed_dim"], geo["hidden_dim"], geo["heads"], geo["depth"])
    assert p.ff_inner == 4 * geo["hidden_dim"] and p.kind == "resampler"
    assert p["image_proj.norm_out.weight"].shape == (cfg.cross_attention_dim,)


def test_linear_adapters_parse_exactly_as_before():
    from cfgpp_amd.ip_adapter import block_table, parse_ip_adapter, resolve, synthetic_ip_adapter
    from cfgpp_amd.unet_config import TINY_SD
    nested = synthetic_ip_adapter(TINY_SD, n_img=4, embed_dim=128, seed=2)
    p = parse_ip_adapter(nested, TINY_SD)
    assert (p.kind, p.seq_input, p.n_img, p.embed_dim, p.hidden_dim, p.heads, p.depth) == ("linear", False, 4, 128, 0, 0, 0)
    table = block_table(TINY_SD)
    assert len(p) == 4 + 2 * len(table)
    assert list(p)[:4] == ["image_proj.proj.weight", "image_proj.proj.bias", "image_proj.norm.weight", "image_proj.norm.bias"]
    assert list(p)[4:6] == [table[0][1] + ".attn2.to_k_ip.weight", table[0][1] + ".attn2.to_v_ip.weight"]
    assert torch.equal(synthetic_ip_adapter(TINY_SD)["image_proj"]["proj.weight"], synthetic_ip_adapter(TINY_SD, 4, None, 0)["image_proj"]["proj.weight"])
    assert resolve("synthetic", TINY_SD).kind == "linear" and resolve("synthetic_plus", TINY_SD).kind == "resampler"


def _edit(nested, **changes):
    out = {"image_proj": dict(nested["image_proj"]), "ip_adapter": dict(nested["ip_adapter"])}
    for k, v in changes.items():
        k = k.replace("__", ".")
        if v is None:
            del out["image_proj"][k]
        else:
            out["image_proj"][k] = v
    return out


def test_parser_refusals_by_message():
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.ip_adapter import parse_ip_adapter
    from cfgpp_amd.unet_config import TINY_XL
    cfg, nested = _plus()
    Z = torch.zeros

    def refused(match, spec, c=cfg):
        with pytest.raises(CfgppError, match=match):
            parse_ip_adapter(spec, c)

    parse_ip_adapter(_edit(nested), cfg)                                         # the unedited copy parses
    refused(r"Resampler.*image_proj\.latents.*image_proj\.proj_in\.weight is missing", _edit(nested, proj_in__weight=None))
    refused(r"image_proj\.layers\.1\.1\.3\.weight is missing", _edit(nested, layers__1__1__3__weight=None))
    # inner, D, E, ff_inner not multiples of 64
    refused(r"inner = 96 is not a multiple of 64", _edit(nested, layers__0__0__to_q__weight=Z(96, 128)))
    refused(r"E = 100 is not a multiple of 64", _edit(nested, proj_in__weight=Z(128, 100)))
    refused(r"ff_inner = 200 is not a multiple of 64", _edit(nested, layers__0__1__1__weight=Z(200, 128)))
    d96 = _edit(nested, latents=Z(1, 16, 96), proj_in__weight=Z(96, 128))
    refused(r"D = 96 is not a multiple of 64", d96)
    # n_q outside 1 .. 32
    refused(r"n_q = 33 image tokens", _edit(nested, latents=Z(1, 33, 128)))
    refused(r"n_q = 0 image tokens", _edit(nested, latents=Z(1, 0, 128)))
    # depth outside 1 .. 8
    none = _edit(nested, **{k.replace(".", "__"): None for k in nested["image_proj"] if k.startswith("layers.")})
    refused(r"depth 0", none)
    _, deep = _plus(depth=9)
    refused(r"depth 9", deep)
    gap = _edit(nested, **{k.replace(".", "__"): None for k in nested["image_proj"] if k.startswith("layers.0.")})
    refused(r"depth 1 \(layers \[1\]\)", gap)
    # to_kv rows != 2 * inner
    refused(r"to_kv\.weight has 192 rows, expected 2 \* inner = 256", _edit(nested, layers__0__0__to_kv__weight=Z(192, 128)))
    # norm_out length != the UNet's cross_attention_dim
    refused(r"norm_out length 128 does not match the UNet's cross_attention_dim 64", _plus("tiny_xl")[1])
    refused(r"norm_out length 64 does not match the UNet's cross_attention_dim 128", nested, TINY_XL)
    # a layer that disagrees with layer 0
    refused(r"image_proj\.layers\.1\.0\.to_q\.weight has shape \(64, 128\), layer 0 fixes \(128, 128\)", _edit(nested, layers__1__0__to_q__weight=Z(64, 128)))
    refused(r"image_proj\.layers\.1\.1\.3\.weight has shape \(128, 256\), layer 0 fixes \(128, 512\)", _edit(nested, layers__1__1__3__weight=Z(128, 256)))
    # FaceID / MLP projection keeps its refusal, also beside latents
    face = {"image_proj": {"proj.0.weight": Z(8, 8), "latents": Z(1, 4, 64)}, "ip_adapter": nested["ip_adapter"]}
    refused(r"FaceID.*image_proj\.proj\.0\.weight", face)
    # the cross-attention half is checked as for Linear adapters
    fewer = {"image_proj": nested["image_proj"], "ip_adapter": {k: v for k, v in nested["ip_adapter"].items() if not k.startswith("1.")}}
    refused("block count", fewer)


def test_synthetic_kind_is_checked():
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.ip_adapter import synthetic_ip_adapter
    from cfgpp_amd.unet_config import TINY_SD
    with pytest.raises(CfgppError, match="kind 'mlp'"):
        synthetic_ip_adapter(TINY_SD, kind="mlp")


# ---- (2) embeds ---------------------------------------------------------------------------------------------------------------
def test_assemble_hidden_rows():
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.ip_adapter import assemble_embeds, assemble_hidden
    h = torch.randn(1, 5, 8)
    r = assemble_hidden(h, None, 3)
    assert r.shape == (6, 5, 8) and r.dtype == torch.float16 and r.is_contiguous()
    assert bool((r[:3] == 0).all()) and all(torch.equal(r[3 + i], h[0].half()) for i in range(3))      # zeros first, then B copies
    n, p = torch.randn(2, 5, 8), torch.randn(2, 5, 8)
    r = assemble_hidden(p, n, 2)
    assert torch.equal(r[:2], n.half()) and torch.equal(r[2:], p.half())
    with pytest.raises(CfgppError, match=r"shape \(1, 8\).*\[1 or 3, seq, embed_dim\]"):
        assemble_hidden(torch.randn(1, 8), None, 3)
    with pytest.raises(CfgppError, match="negative_ip_adapter_image_embeds"):
        assemble_hidden(h, torch.randn(1, 4, 8), 3)
    assert assemble_embeds(torch.randn(2, 1, 8), None, 2).shape == (4, 8)       # the 2-D form keeps its [B, 1, E] squeeze
    with pytest.raises(CfgppError, match=r"expected \[1 or 2, embed_dim\]"):
        assemble_embeds(torch.randn(2, 5, 8), None, 2)


def test_image_encoder_hidden_states(tmp_path):
    transformers = pytest.importorskip("transformers")
    from cfgpp_amd.ip_adapter import ImageEncoder, preprocess_image
    cfgv = transformers.CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=3, num_attention_heads=2, image_size=224,
                                         patch_size=32, projection_dim=16)
    torch.manual_seed(0)
    transformers.CLIPVisionModelWithProjection(cfgv).save_pretrained(str(tmp_path / "image_encoder"))
    enc = ImageEncoder(str(tmp_path), device="cpu")
    enc.model = enc.model.float()                                               # (fp16 LayerNorm / conv on the CPU is not everywhere)
    img = torch.rand(2, 3, 240, 300, generator=torch.Generator().manual_seed(1))
    h = enc(img, hidden=True)
    assert h.shape == (2, 1 + (224 // 32) ** 2, 32)
    want = enc.model(pixel_values=preprocess_image(img), output_hidden_states=True).hidden_states[-2]
    assert torch.equal(h, want)
    assert enc(img).shape == (2, 16)                                            # the pooled embeds, as before
    neg = enc.negative_hidden(img)
    zero_pixels = enc.model(pixel_values=torch.zeros(2, 3, 224, 224), output_hidden_states=True).hidden_states[-2]
    assert torch.equal(neg, zero_pixels) and float(neg.abs().max()) > 0        # the tower on zero PIXELS, not zero hidden states
    assert "zeros_like" in ImageEncoder.negative_hidden.__doc__


# ---- (3) the solvers on the mock engine -------------------------------------------------------------------------------------
def _solver(name, model="sd15", adapter="synthetic_plus", **kw):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    from cfgpp_amd.weights import synth_state_dict
    from ip_plus_mock import IPPlusMockEngine
    if model == "sd15":
        from cfgpp_amd.latent_diffusion import get_solver
        cfg = TINY_SD
    else:
        from cfgpp_amd.latent_sdxl import get_solver
        cfg = TINY_XL
    eng = IPPlusMockEngine(cfg, synth_state_dict(cfg, 0), (8, 8))
    s = get_solver(name, solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", unet_config=cfg, max_batch=2,
                   latent_hw=(8, 8), engine=eng, vae=StubVAE(cfg.vae_scale), ip_adapter=adapter, **kw)
    return s, eng, cfg


def _kw(model):
    if model == "sd15":
        return dict(cfg_guidance=0.6, prompt=["", ["a cat", "a dog"]], seeds=[1, 2], return_latents=True)
    return dict(prompt1=["", ["a cat", "a dog"]], prompt2=["", ["a cat", "a dog"]], cfg_guidance=0.6, target_size=(64, 64),
                original_size=(64, 64), seeds=[1, 2], return_latents=True)


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_ddim_cfgpp_with_a_plus_adapter(model):
    s, eng, cfg = _solver("ddim_cfg++", model)
    E = eng.ip_adapter.embed_dim
    hid = torch.randn(1, 5, E, generator=torch.Generator().manual_seed(5))
    plain = s.sample(**_kw(model))
    n = len(eng.image_calls)
    zero = s.sample(ip_adapter_image_embeds=hid, ip_adapter_scale=0, **_kw(model))
    for x, y in zip(plain, zero):
        assert torch.equal(x, y)                        # scale 0: the plain chain, bit for bit
    with_ip = s.sample(ip_adapter_image_embeds=hid, ip_adapter_scale=0.8, **_kw(model))
    rows, scale = [c for c in eng.image_calls[n:] if c[0] is not None][-1]
    assert scale == 0.8 and rows.shape == (4, 5, E)
    assert bool((rows[:2] == 0).all())                  # default negative: zeros of the same shape
    assert torch.equal(rows[2], hid[0].half()) and torch.equal(rows[3], hid[0].half())
    assert float((with_ip[0].float() - plain[0].float()).abs().max()) > 1e-2        # the image prompt moves the chain
    other = s.sample(ip_adapter_image_embeds=-hid, ip_adapter_scale=0.8, **_kw(model))
    assert not torch.equal(other[0], with_ip[0])        # ... and the chain depends on the hidden states, not on the latents alone
    from cfgpp_amd._lib import CfgppError
    with pytest.raises(CfgppError, match=r"Resampler.*\[1 or 2, seq, embed_dim\]"):
        s.sample(ip_adapter_image_embeds=torch.zeros(1, E), **_kw(model))


def test_solver_asks_the_tower_for_hidden_states():
    """ip_adapter_image= with a Resampler adapter: hidden=True, and the default negative is the tower on zero pixels"""
    s, eng, cfg = _solver("ddim_cfg++")
    E = eng.ip_adapter.embed_dim
    calls = []

    class Tower:
        def __call__(self, image, hidden=False):
            calls.append(("pos", hidden))
            return torch.full((1, 3, E), 0.5)

        def negative_hidden(self, image):
            calls.append(("neg", True))
            return torch.full((1, 3, E), -0.25)

    s.image_encoder = Tower()
    s.sample(ip_adapter_image=torch.rand(1, 3, 32, 32), **_kw("sd15"))
    assert calls == [("pos", True), ("neg", True)]
    rows, _ = [c for c in eng.image_calls if c[0] is not None][-1]
    assert rows.shape == (4, 3, E) and bool((rows[:2] == -0.25).all()) and bool((rows[2:] == 0.5).all())
    s.set_ip_adapter("synthetic")                       # a Linear adapter on the same solver: the pooled embeds, zeros as negative
    calls.clear()

    class Pooled:
        def __call__(self, image, hidden=False):
            calls.append(("pos", hidden))
            return torch.full((1, eng.ip_adapter.embed_dim), 0.5)

    s.image_encoder = Pooled()
    s.sample(ip_adapter_image=torch.rand(1, 3, 32, 32), **_kw("sd15"))
    assert calls == [("pos", False)]


@pytest.mark.parametrize("name", ["ddim_inversion_cfg++", "ddim_edit"])
def test_inversion_and_edit_still_refuse(name):
    s, eng, cfg = _solver(name)
    with pytest.raises(ValueError, match="does not take ip_adapter_image_embeds"):
        s.sample(ip_adapter_image_embeds=torch.zeros(1, 5, eng.ip_adapter.embed_dim))


def test_reference_resampler_matches_its_fp64_and_fp16_storage_forms():
    """tests/ip_plus_ref.py: the fp32 form, the fp64 form and the fp16-storage model agree to their precisions, the published
    scaling (q and k times 64^-1/4) equals scores / 8, and the tokens depend on the hidden states"""
    from cfgpp_amd.ip_adapter import parse_ip_adapter
    from ip_plus_ref import resampler_tokens
    cfg, nested = _plus()
    ad = parse_ip_adapter(nested, cfg)
    h = torch.randn(2, 7, 128, generator=torch.Generator().manual_seed(3)).half().float()
    t64 = resampler_tokens(ad, h, torch.float64)
    t32 = resampler_tokens(ad, h, torch.float32)
    t16 = resampler_tokens(ad, h, torch.float64, storage16=True)
    assert t64.shape == (2, 16, cfg.cross_attention_dim)
    assert float((t32 - t64).abs().max()) < 1e-4
    assert 0 < float((t16 - t64).abs().max()) < 3e-2
    assert float((resampler_tokens(ad, -h, torch.float64) - t64).abs().max()) > 0.1


# ---- (4) the extension header ------------------------------------------------------------------------------------------------
def test_extension_header_is_exported_and_bound():
    import os
    import re
    from cfgpp_amd import _lib
    from cfgpp_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "cfgpp_ip_plus.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cfgpp_[a-z0-9_]+)\s*\(", code))
    assert declared == {"cfgpp_unet_image_context_seq"} == set(_lib.IP_PLUS_PROTOTYPES)
    assert all(hasattr(lib, n) for n in declared)
    for name in ("cfgpp_op_perceiver_attention", "cfgpp_unet_ip_tokens"):
        assert name in _lib.DEBUG_PROTOTYPES and hasattr(lib, name)
    for word in ("Resampler", "no counterpart in the reference", "cfgpp_unet_image_context", "proj_in", "to_kv"):
        assert word in hdr, word


# ---- (5) the command line -----------------------------------------------------------------------------------------------------
def test_text_to_img_cli_with_a_plus_adapter(tmp_path):
    import os
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import text_to_img
    from cfgpp_amd.unet_config import TINY_SD
    from cfgpp_amd.weights import synth_state_dict
    from ip_plus_mock import IPPlusMockEngine
    eng = IPPlusMockEngine(TINY_SD, synth_state_dict(TINY_SD, 0), (8, 8))
    hid = np.random.RandomState(0).randn(5, 128).astype(np.float32)             # [S, E]: one image
    np.save(tmp_path / "h.npy", hid)
    common = ["--method", "ddim_cfg++", "--cfg_guidance", "0.6", "--NFE", "2", "--prompt", "a cat", "--device", "cpu", "--workdir", str(tmp_path)]
    kw = dict(engine=eng, vae=StubVAE(0.18215), latent_hw=(8, 8), unet_config=TINY_SD)
    text_to_img.main(common + ["--ip_adapter", "synthetic_plus:0.5", "--ip_embeds", str(tmp_path / "h.npy")], solver_kwargs=kw)
    rows, scale = [c for c in eng.image_calls if c[0] is not None][-1]
    assert scale == 0.5 and rows.shape == (2, 5, 128) and torch.equal(rows[1], torch.from_numpy(hid).half())
    assert (tmp_path / "result" / "generated.png").exists()
    np.save(tmp_path / "h3.npy", hid[None])                                     # [B, S, E]
    text_to_img.main(common + ["--ip_adapter", "synthetic_plus", "--ip_embeds", str(tmp_path / "h3.npy")], solver_kwargs=kw)
    rows, scale = [c for c in eng.image_calls if c[0] is not None][-1]
    assert scale == 1.0 and rows.shape == (2, 5, 128)
