"""Inpainting host logic without a GPU: the inpaint UNet configs, mask preparation, the strength rule, the checkpoint
loader's 9-channel detection, the solver registry, and whole chains on the CPU mock (tests/inpaint_mock.py) against
restatements written here."""
import json
import os
import types

import pytest
import torch

from inpaint_mock import InpaintMockEngine
from mock_engine import MockEngine, StubVAE
from oracle import sampler as O

import cfgpp_amd.latent_diffusion as sd
import cfgpp_amd.latent_sdxl as xl
from cfgpp_amd import inpaint as IP
from cfgpp_amd.schedule import SchedulerTables
from cfgpp_amd.unet_config import (CONFIGS, SD15, SD15_INPAINT, SDXL, SDXL_INPAINT, TINY_SD, TINY_SD_INPAINT, TINY_XL,
                                   TINY_XL_INPAINT, param_count)
from cfgpp_amd.weights import synth_state_dict

HW = 16


def cfgn(n):
    return types.SimpleNamespace(num_sampling=n)


def test_inpaint_config_parameter_totals():
    assert param_count(SD15_INPAINT) == 859_535_364 and param_count(SDXL_INPAINT) == 2_567_478_084
    assert param_count(SD15_INPAINT) - param_count(SD15) == 14_400 and param_count(SDXL_INPAINT) - param_count(SDXL) == 14_400
    for base, inp in ((SD15, SD15_INPAINT), (SDXL, SDXL_INPAINT), (TINY_SD, TINY_SD_INPAINT), (TINY_XL, TINY_XL_INPAINT)):
        assert inp.in_channels == 9 and inp.out_channels == 4 and CONFIGS[inp.name] is inp
        assert inp.block_out_channels == base.block_out_channels and inp.cross_attention_dim == base.cross_attention_dim


def test_mask_preparation_binarizes_picks_pixel_8i_8j_and_masks_the_image():
    g = torch.Generator().manual_seed(0)
    mask = torch.rand(2, 1, 8 * 4, 8 * 3, generator=g)
    mask[0, 0, 0, 0], mask[0, 0, 8, 0], mask[0, 0, 0, 8] = 0.5, 0.49999, 1.0
    img = torch.rand(2, 3, 32, 24, generator=g) * 2 - 1
    m, masked, lm = IP.prepare_mask(mask, img, (4, 3))
    assert set(m.unique().tolist()) <= {0.0, 1.0} and torch.equal(m, (mask >= 0.5).float())
    assert m[0, 0, 0, 0] == 1 and m[0, 0, 8, 0] == 0
    assert lm.shape == (2, 1, 4, 3) and torch.equal(lm, m[:, :, ::8, ::8])
    assert torch.equal(masked, img * (mask < 0.5))
    assert (masked[m.expand_as(img) == 1] == 0).all()


@pytest.mark.parametrize("n,strength", [(10, 1.0), (10, 0.5), (10, 0.75), (7, 0.3), (50, 0.999)])
def test_strength_slices_timesteps_like_get_timesteps(n, strength):
    ts = SchedulerTables(n).timesteps
    got, start = IP.strength_timesteps(ts, strength)
    init = min(int(n * strength), n)
    assert start == max(n - init, 0) and torch.equal(got, ts[n - init:])
    with pytest.raises(ValueError):
        IP.strength_timesteps(ts, 0.01)


def test_checkpoint_dir_with_9_input_channels_selects_the_inpaint_config(tmp_path):
    from cfgpp_amd.checkpoint import solver_kwargs_from_dir
    for sub in ("unet", "vae"):
        (tmp_path / sub).mkdir()
        (tmp_path / sub / "diffusion_pytorch_model.safetensors").write_bytes(b"")
    before = solver_kwargs_from_dir(tmp_path, sdxl=False, device="cpu")
    (tmp_path / "unet" / "config.json").write_text(json.dumps({"in_channels": 4, "out_channels": 4}))
    assert solver_kwargs_from_dir(tmp_path, sdxl=False, device="cpu") == before
    (tmp_path / "unet" / "config.json").write_text(json.dumps({"in_channels": 9, "out_channels": 4}))
    kw, missing = solver_kwargs_from_dir(tmp_path, sdxl=False, device="cpu")
    assert kw.pop("unet_config") is SD15_INPAINT and (kw, missing) == before
    kw, _ = solver_kwargs_from_dir(tmp_path, sdxl=True, device="cpu")
    assert kw["unet_config"] is SDXL_INPAINT


def test_inpaint_solvers_have_their_own_registry():
    assert IP.inpaint_solver_names() == ["ddim_inpaint", "ddim_inpaint_cfg++"]
    for name in IP.inpaint_solver_names():
        assert name not in sd.__SOLVER__ and name not in xl.__SOLVER__
        assert issubclass(IP.__INPAINT_SOLVER__[f"sd15/{name}"], sd.StableDiffusion)
        assert issubclass(IP.__INPAINT_SOLVER__[f"sdxl/{name}"], xl.SDXL)
    with pytest.raises(ValueError):
        IP.get_inpaint_solver("ddim_inpaint", model="sd20")
    with pytest.raises(ValueError):
        IP.get_inpaint_solver("ddim", model="sd15")


# ---------------------------------------------------------------------------------------------------- chains on the CPU mock
_NETS = {}


def _net(cfg):
    from oracle.unet_ref import UNetRef
    if cfg.name not in _NETS:
        _NETS[cfg.name] = UNetRef(cfg, synth_state_dict(cfg, 0))
    return _NETS[cfg.name]


def _unet_fn(cfg):
    net = _net(cfg)
    return lambda z, t, ehs, te, ti: net(z.float(), t, ehs.float())["sample"].half()


def _inputs(B=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(B, 3, 8 * HW, 8 * HW, generator=g) * 2 - 1
    mask = torch.zeros(1, 1, 8 * HW, 8 * HW)
    mask[..., 24:88, 40:104] = 1.0
    return img, mask


def _solver(name, cfg, nfe=4, B=2, model="sd15"):
    eng = InpaintMockEngine(_unet_fn(cfg), (HW, HW))
    kw = dict(solver_config=cfgn(nfe), device="cpu", unet_config=cfg, max_batch=B, latent_hw=(HW, HW), engine=eng,
              vae=StubVAE(cfg.vae_scale))
    return IP.get_inpaint_solver(name, model=model, **kw), eng


def test_all_ones_mask_is_ddim_cfgpp_bit_for_bit():
    s, _ = _solver("ddim_inpaint_cfg++", TINY_SD)
    uc, c = s.get_text_embed("bad", ["a cat", "a dog"])
    img, mask = _inputs()
    a = s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), src_img=img, mask=torch.ones_like(mask), seeds=[1, 2], return_latents=True)
    ref = sd.get_solver("ddim_cfg++", solver_config=cfgn(4), device="cpu", unet_config=TINY_SD, max_batch=2, latent_hw=(HW, HW),
                        engine=MockEngine(_unet_fn(TINY_SD), (HW, HW)), vae=StubVAE(TINY_SD.vae_scale))
    b = ref.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), latents=ref._randn((2, 4, HW, HW), [1, 2]), return_latents=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name", ["ddim_inpaint", "ddim_inpaint_cfg++"])
def test_all_zeros_mask_ends_on_the_source_latent(name):
    s, _ = _solver(name, TINY_SD)
    uc, c = s.get_text_embed("bad", ["a cat", "a dog"])
    img, mask = _inputs()
    z0t, _ = s.sample(cfg_guidance=0.6 if "++" in name else 7.5, prompt_embeds=(uc, c), src_img=img, mask=torch.zeros_like(mask),
                      seeds=[1, 2], return_latents=True)
    assert torch.equal(z0t, s.encode(img).float())


def _masked_restatement(cfg, uc, c, img, mask, lam, cfgpp, nfe, seeds, strength=1.0, wrap=False):
    """diffusers' 4-channel inpaint loop with the oracle's DDIM step: blend with the source noised to t_next after every step"""
    net = _net(cfg)
    tb = SchedulerTables(nfe)
    vae = StubVAE(cfg.vae_scale)
    z_src = vae.encode(img).half().float()
    m = (torch.nn.functional.interpolate((mask >= 0.5).float(), size=(HW, HW)) >= 0.5).expand(z_src.shape[0], 1, HW, HW)
    noise = sd.StableDiffusion._randn((z_src.shape[0], 4, HW, HW), seeds)
    n = len(tb.timesteps)
    init = min(int(n * strength), n)
    ts = tb.timesteps[n - init:]
    if strength < 1:
        c1, c2 = tb.ddim_sqrt_coeffs(ts[0], wrap=wrap)[:2]
        zt = c2 * z_src + c1 * noise
    else:
        zt = noise.clone()
    ehs = torch.cat([uc.expand(c.shape[0], -1, -1), c]).float()
    ts = ts.int() if wrap else ts
    for i, t in enumerate(ts):
        eps = net(torch.cat([zt, zt]).float(), float(t), ehs)["sample"].half()
        B = zt.shape[0]
        sq = tb.ddim_sqrt_coeffs(t, wrap=wrap)
        z0t, zn = O.ddim_step(zt, eps[:B], eps[B:], lam, None, None, tweedie_uc=False, renoise_uc=cfgpp, sqrt4=sq)
        a, b = (sq[2], sq[3]) if i < len(ts) - 1 else (1.0, 0.0)
        zt = torch.where(m, zn, a * z_src + b * noise)
        z0t = torch.where(m, z0t, z_src)
    return z0t, zt


@pytest.mark.parametrize("name,lam,strength", [("ddim_inpaint_cfg++", 0.6, 1.0), ("ddim_inpaint", 7.5, 0.5)])
def test_masked_chain_vs_restatement(name, lam, strength):
    s, eng = _solver(name, TINY_SD, nfe=6)
    uc, c = s.get_text_embed("bad", ["a cat", "a dog"])
    img, mask = _inputs()
    z0t, zt = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), src_img=img, mask=mask, strength=strength, seeds=[3, 4],
                       return_latents=True)
    r0, rt = _masked_restatement(TINY_SD, uc, c, img, mask, lam, "++" in name, 6, [3, 4], strength)
    assert len(eng.calls) == min(int(6 * strength), 6)
    assert torch.equal(z0t, r0) and torch.equal(zt, rt)


def test_strength_start_latent_is_the_noised_source():
    s, eng = _solver("ddim_inpaint_cfg++", TINY_SD, nfe=10)
    uc, c = s.get_text_embed("bad", ["a cat", "a dog"])
    img, mask = _inputs()
    s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), src_img=img, mask=mask, strength=0.5, seeds=[3, 4], return_latents=True)
    ts = SchedulerTables(10).timesteps
    assert [cl["t"] for cl in eng.calls] == [float(t) for t in ts[5:]]
    c1, c2 = SchedulerTables(10).ddim_sqrt_coeffs(ts[5])[:2]
    start = c2 * s.encode(img).float() + c1 * s._randn((2, 4, HW, HW), [3, 4])
    assert torch.equal(eng.calls[0]["z"], start)


@pytest.mark.parametrize("name,lam", [("ddim_inpaint_cfg++", 0.6), ("ddim_inpaint", 7.5)])
def test_9_channel_chain_vs_restatement(name, lam):
    """the inpaint UNet's chain: the oracle UNet on cat(z, mask, masked-image latent) inside the oracle's DDIM loop"""
    s, eng = _solver(name, TINY_SD_INPAINT, nfe=5)
    uc, c = s.get_text_embed("bad", ["a cat", "a dog"])
    img, mask = _inputs()
    z0t, _ = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), src_img=img, mask=mask, seeds=[7, 8], return_latents=True)
    assert len(eng.conds) == 1 and eng.conds[0].shape == (2, 5, HW, HW) and eng.conds[0].dtype == torch.float16

    net = _net(TINY_SD_INPAINT)
    lm = (torch.nn.functional.interpolate((mask >= 0.5).float(), size=(HW, HW))).expand(2, -1, -1, -1)
    ml = StubVAE(TINY_SD_INPAINT.vae_scale).encode(img * (mask < 0.5)).half().float()
    cond = torch.cat([lm, ml], 1)
    ehs = torch.cat([uc.expand(2, -1, -1), c]).float()

    def unet(z, t):
        x = torch.cat([z.float(), cond], 1)
        eps = net(torch.cat([x, x]), float(t), ehs)["sample"].half()
        return eps[:2], eps[2:]
    zT = sd.StableDiffusion._randn((2, 4, HW, HW), [7, 8])
    r0, _ = O.sample_ddim(unet, zT, SchedulerTables(5), lam, cfgpp="++" in name)
    assert torch.equal(z0t, r0)


def test_sdxl_masked_and_9_channel_solvers_run_on_the_mock():
    img, mask = _inputs(B=1)
    for cfg in (TINY_XL, TINY_XL_INPAINT):
        eng = InpaintMockEngine(lambda z, t, ehs, te, ti, cfg=cfg: _net(cfg)(z.float(), t, ehs.float(),
                                                                             {"text_embeds": te.float(), "time_ids": ti.float()})["sample"].half(),
                                (HW, HW))
        s = IP.get_inpaint_solver("ddim_inpaint_cfg++", model="sdxl", solver_config=cfgn(3), device="cpu", unet_config=cfg, max_batch=1,
                                  latent_hw=(HW, HW), engine=eng, vae=StubVAE(cfg.vae_scale))
        z0t = s.sample(prompt=["bad", "a cat"], cfg_guidance=0.6, src_img=img, mask=mask, seeds=[1], return_latents=True)
        assert z0t.shape == (1, 4, HW, HW) and torch.isfinite(z0t).all() and len(eng.calls) == 3
        assert (len(eng.conds) == 1) == (cfg is TINY_XL_INPAINT)
        if cfg is TINY_XL:
            keep = (torch.nn.functional.interpolate(mask, size=(HW, HW)) < 0.5).expand_as(z0t)
            assert torch.equal(z0t[keep], s.encode(img).float()[keep])


def test_inpaint_cli_writes_an_image_on_the_cpu_mock(tmp_path):
    import sys
    from PIL import Image
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import inpaint as cli
    Image.fromarray((torch.rand(128, 128, 3) * 255).to(torch.uint8).numpy()).save(tmp_path / "src.png")
    m = torch.zeros(128, 128, dtype=torch.uint8)
    m[32:96, 16:80] = 255
    Image.fromarray(m.numpy()).save(tmp_path / "mask.png")
    for cfg in (TINY_SD, TINY_SD_INPAINT):
        eng = InpaintMockEngine(_unet_fn(cfg), (HW, HW))
        cli.main(["--img_path", str(tmp_path / "src.png"), "--mask_path", str(tmp_path / "mask.png"), "--img_size", "128", "--NFE", "2",
                  "--device", "cpu", "--workdir", str(tmp_path / cfg.name), "--prompt", "a dog", "--cfg_guidance", "0.6"],
                 solver_kwargs=dict(engine=eng, unet_config=cfg, vae=StubVAE(cfg.vae_scale)))
        assert (tmp_path / cfg.name / "result" / "inpaint.png").exists() and len(eng.calls) == 2
        assert (len(eng.conds) == 1) == (cfg is TINY_SD_INPAINT)
