"""CPU: ControlNet plumbing - the diffusers ControlNetModel key table, the solvers' control_image / scale path on a mock
engine (tests/controlnet_mock.py), refusals of the non-text-to-image solvers, the controlnet/ folder loader and the
text_to_img CLI flags."""
import json
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

from controlnet_mock import ControlMockEngine      # noqa: E402
from mock_engine import MockEngine, StubVAE        # noqa: E402


def _unet(z, t, ehs, te, ti):
    return (0.1 * z + 0.01 * ehs.float().mean(dim=(1, 2)).view(-1, 1, 1, 1)).half()


def _controlled(z, t, ehs, te, ti, cn, rows, scale):
    # a stand-in whose output depends on the image rows and the scale
    return (_unet(z, t, ehs, te, ti).float() + scale * 0.05 * rows.float().mean(dim=(1, 2, 3)).view(-1, 1, 1, 1)).half()


def test_controlnet_param_totals_and_residual_counts():
    from cfgpp_amd.controlnet import controlnet_param_count, controlnet_param_shapes, num_down_residuals
    from cfgpp_amd.unet_config import SD15, SDXL
    assert controlnet_param_count(SD15) == 361_279_120 and num_down_residuals(SD15) == 12
    assert controlnet_param_count(SDXL) == 1_251_014_160 and num_down_residuals(SDXL) == 9
    P = controlnet_param_shapes(SD15)
    assert P["controlnet_cond_embedding.conv_in.weight"] == (16, 3, 3, 3)
    assert P["controlnet_cond_embedding.blocks.5.weight"] == (256, 96, 3, 3)
    assert P["controlnet_cond_embedding.conv_out.weight"] == (320, 256, 3, 3)
    assert P["controlnet_down_blocks.11.weight"] == (1280, 1280, 1, 1) and "controlnet_down_blocks.12.weight" not in P
    assert P["controlnet_mid_block.weight"] == (1280, 1280, 1, 1)
    assert not any(k.startswith(("up_blocks.", "conv_out.", "conv_norm_out.")) for k in P)
    assert sum(k.startswith("controlnet_down_blocks.") for k in controlnet_param_shapes(SDXL)) == 2 * 9


def test_synthetic_zero_convolutions_are_not_zero():
    from cfgpp_amd.controlnet import synth_controlnet_state_dict
    from cfgpp_amd.unet_config import TINY_SD
    sd = synth_controlnet_state_dict(TINY_SD)
    for k, v in sd.items():
        if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block")) and k.endswith("weight"):
            assert float(v.abs().mean()) > 1e-3, k


def _solver(name, engine, model="sd15", **kw):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    if model == "sd15":
        from cfgpp_amd.latent_diffusion import get_solver
        cfg = TINY_SD
    else:
        from cfgpp_amd.latent_sdxl import get_solver
        cfg = TINY_XL
    return get_solver(name, solver_config=types.SimpleNamespace(num_sampling=4), device="cpu", unet_config=cfg, max_batch=2,
                      latent_hw=(8, 8), engine=engine, vae=StubVAE(cfg.vae_scale), **kw)


@pytest.mark.parametrize("name", ["ddim_cfg++", "ddim", "euler_cfg++", "euler_a_cfg++", "dpm++_2m_cfg++", "dpm++_2s_a"])
def test_sample_with_control_image_drives_the_engine(name):
    eng = ControlMockEngine(_unet, _controlled, (8, 8))
    s = _solver(name, eng, controlnet="synthetic")
    assert eng.control_calls == [("build", "synthetic", 0)]
    img = torch.rand(1, 3, 64, 64)
    kw = dict(cfg_guidance=0.6, prompt=["", ["a cat", "a dog"]], seeds=[1, 2], return_latents=True)
    a = s.sample(control_image=img, controlnet_conditioning_scale=0.7, **kw)
    assert eng.control_calls[1:] == [("set", (1, 3, 64, 64), 0.7), ("clear",)]
    assert all(c.get("control") for c in eng.calls)
    n = len(eng.calls)
    torch.manual_seed(0)                               # the ancestral samplers' noise
    b = s.sample(**kw)                                 # no control image: the plain engine, nothing attached
    assert eng.control is None and not any(c.get("control") for c in eng.calls[n:])
    torch.manual_seed(0)
    ref = _solver(name, MockEngine(_unet, (8, 8))).sample(**kw)      # a solver built without a ControlNet
    for x, y in zip(b, ref):
        assert torch.equal(x, y)
    assert not all(torch.equal(x, y) for x, y in zip(a, b))


def test_sdxl_sample_with_control_image():
    eng = ControlMockEngine(_unet, _controlled, (8, 8))
    s = _solver("ddim_cfg++", eng, model="sdxl", controlnet="synthetic")
    s.sample(prompt1=["", "a cat"], prompt2=["", "a cat"], cfg_guidance=0.6, target_size=(64, 64), original_size=(64, 64),
             control_image=torch.rand(1, 3, 64, 64), controlnet_conditioning_scale=1.0, return_latents=True)
    assert eng.control_calls[1:] == [("set", (1, 3, 64, 64), 1.0), ("clear",)]


def test_control_image_without_controlnet_is_an_error():
    s = _solver("ddim_cfg++", ControlMockEngine(_unet, _controlled, (8, 8)))
    with pytest.raises(ValueError, match="no ControlNet"):
        s.sample(cfg_guidance=0.6, prompt=["", "a cat"], control_image=torch.rand(1, 3, 64, 64))


@pytest.mark.parametrize("model,name", [("sd15", "ddim_inversion_cfg++"), ("sd15", "ddim_edit"), ("sdxl", "ddim_edit_cfg++"),
                                        ("sdxl", "ddim_inversion_cfg++")])
def test_inversion_and_edit_refuse_control_image(model, name):
    eng = ControlMockEngine(_unet, _controlled, (8, 8))
    s = _solver(name, eng, model=model, controlnet="synthetic")
    with pytest.raises(ValueError, match="does not take control_image"):
        s.sample(control_image=torch.rand(1, 3, 64, 64))
    assert eng.control is None


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_inpaint_refuses_control_image(model):
    from cfgpp_amd.inpaint import get_inpaint_solver
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    cfg = TINY_SD if model == "sd15" else TINY_XL
    s = get_inpaint_solver("ddim_inpaint_cfg++", model, solver_config=types.SimpleNamespace(num_sampling=2), device="cpu",
                           unet_config=cfg, latent_hw=(8, 8), engine=ControlMockEngine(_unet, _controlled, (8, 8)), vae=StubVAE(cfg.vae_scale))
    with pytest.raises(ValueError, match="does not take control_image"):
        s.sample(prompt=["", "a cat"], src_img=torch.zeros(1, 3, 64, 64), mask=torch.ones(1, 1, 64, 64),
                 control_image=torch.rand(1, 3, 64, 64))


def _write_controlnet_dir(folder, cfg, **extra):
    from safetensors.torch import save_file
    from cfgpp_amd.controlnet import synth_controlnet_state_dict
    os.makedirs(folder, exist_ok=True)
    conf = {"_class_name": "ControlNetModel", "in_channels": 4, "block_out_channels": list(cfg.block_out_channels),
            "layers_per_block": cfg.layers_per_block,
            "down_block_types": ["CrossAttnDownBlock2D" if a else "DownBlock2D" for a in cfg.level_has_attn],
            "attention_head_dim": list(cfg.num_heads), "cross_attention_dim": cfg.cross_attention_dim,
            "transformer_layers_per_block": list(cfg.transformer_depth), "conditioning_embedding_out_channels": [16, 32, 96, 256],
            "global_pool_conditions": False, "controlnet_conditioning_channel_order": "rgb", "norm_num_groups": 32}
    conf.update(extra)
    with open(os.path.join(folder, "config.json"), "w") as f:
        json.dump(conf, f)
    save_file({k: v.half() for k, v in synth_controlnet_state_dict(cfg).items()}, os.path.join(folder, "diffusion_pytorch_model.safetensors"))


def test_controlnet_folder_loader(tmp_path):
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.checkpoint import controlnet_from_dir
    from cfgpp_amd.controlnet import controlnet_param_shapes
    from cfgpp_amd.unet_config import TINY_SD
    d = str(tmp_path / "controlnet")
    _write_controlnet_dir(d, TINY_SD)
    cfg, items = controlnet_from_dir(d, TINY_SD)
    assert (cfg.block_out_channels, cfg.level_has_attn, cfg.num_heads, cfg.transformer_depth) == \
        (TINY_SD.block_out_channels, TINY_SD.level_has_attn, TINY_SD.num_heads, TINY_SD.transformer_depth)
    sd = dict(items)
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(controlnet_param_shapes(TINY_SD))
    for field, value in (("global_pool_conditions", True), ("controlnet_conditioning_channel_order", "bgr"),
                         ("conditioning_embedding_out_channels", [16, 32, 96, 128])):
        bad = str(tmp_path / field)
        _write_controlnet_dir(bad, TINY_SD, **{field: value})
        with pytest.raises(CfgppError, match=field):
            controlnet_from_dir(bad, TINY_SD)


def test_text_to_img_cli_with_controlnet(tmp_path):
    from PIL import Image
    import text_to_img
    from cfgpp_amd.checkpoint import controlnet_from_dir
    from cfgpp_amd.unet_config import SD15
    d = str(tmp_path / "controlnet")
    _write_controlnet_dir(d, SD15.__class__(**{**SD15.__dict__, "name": "tiny_cli", "block_out_channels": (64, 128), "level_has_attn": (1, 0),
                                                "transformer_depth": (1, 1), "num_heads": (2, 2), "cross_attention_dim": 64}))
    loaded = []

    def make(spec, seed):
        cfg, items = controlnet_from_dir(spec, SD15)
        loaded.append((cfg.block_out_channels, len(dict(items))))
        return "cn"
    eng = ControlMockEngine(_unet, _controlled, (8, 8), make_controlnet=make)
    edges = tmp_path / "edges.png"
    Image.fromarray((torch.rand(40, 50, 3) * 255).byte().numpy()).save(edges)
    text_to_img.main(["--method", "ddim_cfg++", "--cfg_guidance", "0.6", "--NFE", "2", "--prompt", "a cat", "--device", "cpu",
                      "--workdir", str(tmp_path), "--controlnet_dir", d, "--control_image", str(edges)],
                     solver_kwargs=dict(engine=eng, vae=StubVAE(0.18215), latent_hw=(8, 8)))
    assert loaded and loaded[0][0] == (64, 128)
    sets = [c for c in eng.control_calls if c[0] == "set"]
    assert sets == [("set", (1, 3, 64, 64), 1.0)]                  # resized to the target size, RGB
    assert Image.open(tmp_path / "result" / "generated.png").size == (64, 64)
