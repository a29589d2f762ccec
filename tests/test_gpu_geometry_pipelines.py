"""-m gpu: whole jobs at a non-square latent, (8, 24) = a 64 x 192 image, NFE 4 each (the hires job: 5 steps at strength 0.6, of which 3
run, as every job of tests/test_gpu_img2img_net.py) - what strings the engines of
tests/test_gpu_geometry_engines.py to the step kernels, the VAE, the graph replay and the img2img start, all of which take H and W from
the solver's ``latent_hw``.

  * `ddim_cfg++` on tiny SD and on tiny SDXL (target_size = original_size = (64, 192)) against the MockEngine + UNetRef loop, exactly as
    test_gpu_unet.py::test_sd_chain_vs_oracle and test_gpu_configs.py::test_sdxl_solver_chain_vs_oracle do.
  * the solver's latent into the VAE: HipVAE takes H * W in multiples of 128 only and refuses 8 x 24 = 192 by name (asserted), so the
    tiny SD chain runs once more at (16, 24), the nearest latent it accepts, and its result is decoded by HipVAE against VAERef at
    tests/test_gpu_vae.py's 1e-2: shape (B, 3, 128, 192).
  * the tiny SD loop under CFGPP_GRAPH=1: the eager loop's bits (the `_both` pattern of tests/test_gpu_graph.py).
  * hires fix: source latents (4, 12) upscaled bilinear to (8, 24) inside the start launch, through test_gpu_img2img_net.py's entry
    point against its mock.

Chain tolerances: twice the rel-L2 the same job measures at (16, 16) on the MI355X (CHAIN_16, the convention of those tests), under the
project's chain bar.  Measured at (8, 24): next to each entry; profiles/latent_geometry/README.md."""
import types

import pytest
import torch

import test_gpu_img2img_net as I2I
from test_gpu_graph import _both, _same

pytestmark = pytest.mark.gpu

HW, SMALL = (8, 24), (4, 12)
VAE_HW = (16, 24)           # H * W = 384 = 3 x 128: the VAE engine accepts it, (8, 24) it does not
NFE = 4
CHAIN_BAR = 7.5e-3          # the project's chain bar (tests/test_gpu_pano_net.py)
# rel-L2 of the same job at (16, 16), measured on the MI355X (sd, sdxl: record("sd_chain") / record("sdxl_chain") at NFE 4; hires:
# test_gpu_img2img_net.CHAIN_MEASURED["ddim_cfgpp"]) -> asserted at twice the value.
CHAIN_16 = {"sd": 4.890e-4,                                # at (8, 24): 4.646e-4; at (16, 24): 4.769e-4
            "sdxl": 3.636e-4,                              # at (8, 24): 3.560e-4
            "hires": I2I.CHAIN_MEASURED["ddim_cfgpp"]}     # 3.849e-4; from (4, 12) to (8, 24): 3.816e-4


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def sd_pair(hw, nfe=NFE):
    """(hip solver, the same solver on MockEngine + UNetRef) of `ddim_cfg++` on tiny SD at ``hw``"""
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD as cfg
    from cfgpp_amd.weights import synth_state_dict
    from mock_engine import MockEngine
    from oracle.unet_ref import UNetRef
    sc = types.SimpleNamespace(num_sampling=nfe)
    hip = get_solver("ddim_cfg++", solver_config=sc, device="cuda", unet_config=cfg, max_batch=2, latent_hw=hw)
    net = UNetRef(cfg, synth_state_dict(cfg, 0))
    ref = get_solver("ddim_cfg++", solver_config=sc, device="cpu", unet_config=cfg, max_batch=2, latent_hw=hw, text_encoder=hip.text_encoder,
                     engine=MockEngine(lambda z, t, ehs, te, ti: net(z, t, ehs.float())["sample"].half(), hw))
    return hip, ref, cfg


def sd_chain(hw, nfe=NFE):
    hip, ref, cfg = sd_pair(hw, nfe)
    uc, c = hip.get_text_embed("bad", ["a cat", "a dog"])
    kw = dict(cfg_guidance=0.6, seeds=[11, 12], return_latents=True)
    a = hip.sample(prompt_embeds=(uc, c), **kw)[0].clone()
    b = ref.sample(prompt_embeds=(uc.cpu(), c.cpu()), **kw)[0].float()
    return a, b, cfg


def sdxl_chain(hw, nfe=NFE):
    from cfgpp_amd.latent_sdxl import get_solver
    from cfgpp_amd.unet_config import TINY_XL as cfg
    from cfgpp_amd.weights import synth_state_dict
    from mock_engine import MockEngine
    from oracle.unet_ref import UNetRef
    sc = types.SimpleNamespace(num_sampling=nfe)
    hip = get_solver("ddim_cfg++", solver_config=sc, device="cuda", unet_config=cfg, max_batch=2, latent_hw=hw, scalar_semantics="cuda")
    net = UNetRef(cfg, synth_state_dict(cfg, 0))

    def unet(z, t, ehs, te, ti):
        return net(z.float(), t, ehs.float(), {"text_embeds": te.float(), "time_ids": ti.float()})["sample"].half()
    ref = get_solver("ddim_cfg++", solver_config=sc, device="cpu", unet_config=cfg, max_batch=2, latent_hw=hw, text_encoder=hip.text_encoder,
                     engine=MockEngine(unet, hw), scalar_semantics="cuda")
    p = ["a cat", "a dog"]
    pe = hip.get_text_embed("bad", p, "bad", p)
    size = (8 * hw[0], 8 * hw[1])
    kw = dict(cfg_guidance=0.6, target_size=size, original_size=size, seeds=[21, 22], return_latents=True)
    a = hip.sample(prompt_embeds=pe, **kw).clone()
    b = ref.sample(prompt_embeds=tuple(x.cpu() for x in pe), **kw).float()
    # the sizes reached the UNet: the added-condition rows hold them
    assert ref.engine.contexts[-1]["ti"].float().cpu()[0].tolist() == [size[0], size[1], 0, 0, size[0], size[1]]
    return a, b, cfg


def hires_chain(hw, small):
    """a 5-step `ddim_cfg++` job on tiny SDXL at strength 0.6 from ``small`` source latents, upscaled bilinear in the start launch"""
    from cfgpp_amd.weights import synth_state_dict
    model, name, opts, lam = I2I.CASES["ddim_cfgpp"]
    cfg = I2I._cfg(model)
    hip = I2I._solver(model, name, hw=hw, device="cuda", **opts)
    eng = I2I.OracleMock(cfg, synth_state_dict(cfg, 0), hw=hw)
    ref = I2I._solver(model, name, hw=hw, device="cpu", text_encoder=hip.text_encoder, engine=eng, **opts)
    pe = I2I._embeds(hip, model)
    src = I2I._source("ddim_cfgpp", hw=hw, small=small)
    size = dict(target_size=(8 * hw[0], 8 * hw[1]), original_size=(8 * hw[0], 8 * hw[1]))
    a = I2I._sample(hip, model, pe, [11, 12], lam, strength=0.6, **size, **src)
    b = I2I._sample(ref, model, tuple(x.cpu() for x in pe), [11, 12], lam, strength=0.6, **size, **src)
    assert hip.last_start == ref.last_start and hip.last_start["mode"] == "bilinear" and hip.last_start["steps"] == 3
    assert len(eng.icalls) == 1 and eng.icalls[0]["shape"] == (2, 4) + tuple(hw) and tuple(eng.icalls[0]["src"].shape[2:]) == tuple(small)
    full = I2I._sample(hip, model, pe, [11, 12], lam, strength=1.0, **size, **src)
    return a, b, full


def chain_check(name, a, b, shape):
    from test_gpu_configs import record
    rel = rel_l2(a, b)
    record("latent_geometry", case=f"{name}-chain-{shape[2]}x{shape[3]}", rel_l2=rel)
    print(f"{name} chain at {shape[2]} x {shape[3]}: rel-L2 {rel:.3e} (tolerance {2 * CHAIN_16[name]:.3e})")
    assert tuple(a.shape) == tuple(b.shape) == shape and bool(torch.isfinite(a.float()).all())
    assert rel < CHAIN_BAR and rel < 2 * CHAIN_16[name], f"{name}: chain rel-L2 {rel:.3e}"
    return rel


def test_sd_chain_at_8x24_and_the_vae_names_the_latent_it_refuses():
    """HipVAE takes latents with H * W a multiple of 128 only, and 8 x 24 = 192 is none: the chain's result cannot be decoded on the
    HIP path, and the refusal says so with the size (the VAE's own non-square decodes: tests/test_gpu_vae.py)"""
    need_gpu()
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.vae import HipVAE, synth_vae_state_dict
    a, b, cfg = sd_chain(HW)
    chain_check("sd", a, b, (2, 4) + HW)
    with pytest.raises(CfgppError, match=r"vae_create: latent 8x24 unsupported \(H\*W must be a multiple of 128"):
        HipVAE(cfg.vae_scale, HW, max_batch=2, state_dict=synth_vae_state_dict(0))


def test_sd_chain_and_vae_decode_at_16x24():
    """the solver's non-square latent handed to the HIP VAE: the chain against the oracle loop, its result decoded against VAERef"""
    need_gpu()
    from cfgpp_amd.vae import HipVAE, synth_vae_state_dict
    from oracle.vae_ref import VAERef
    from test_gpu_configs import record
    a, b, cfg = sd_chain(VAE_HW)
    chain_check("sd", a, b, (2, 4) + VAE_HW)
    vsd = synth_vae_state_dict(0)
    img = HipVAE(cfg.vae_scale, VAE_HW, max_batch=2, state_dict=vsd).decode(a).float().cpu()
    ref = VAERef(cfg.vae_scale, device="cpu", dtype=torch.float32, state_dict=vsd).decode(a.float().cpu())
    rel = rel_l2(img, ref)
    record("latent_geometry", case="vae-decode-16x24", rel_l2=rel)
    print(f"VAE decode of the chain's result at 16 x 24: rel-L2 {rel:.3e}")
    assert img.shape == ref.shape == (2, 3, 8 * VAE_HW[0], 8 * VAE_HW[1]) == (2, 3, 128, 192)
    assert torch.isfinite(img).all() and rel < 1e-2, f"VAE decode rel-L2 {rel:.3e}"
    # a transposed hand-off would be loud: the oracle's image of the transposed-and-refilled latent is far from it
    wrong = VAERef(cfg.vae_scale, device="cpu", dtype=torch.float32, state_dict=vsd).decode(a.float().cpu().transpose(-1, -2).reshape(a.shape))
    assert rel_l2(wrong, ref) > 10 * 1e-2


def test_sdxl_chain_at_8x24():
    need_gpu()
    a, b, _ = sdxl_chain(HW)
    chain_check("sdxl", a, b, (2, 4) + HW)


def test_graph_replay_is_bit_identical_at_8x24(monkeypatch):
    need_gpu()
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD as cfg
    s = get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=NFE), device="cuda", unet_config=cfg, max_batch=2, latent_hw=HW)
    uc, c = s.get_text_embed("bad", ["a cat", "a dog"])

    def run():
        return [t.clone() for t in s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), seeds=[5, 6], return_latents=True)]
    eager, graph, again = _both(monkeypatch, run)
    assert eager[0].shape == (2, 4) + HW and eager[0].dtype == torch.float32 and torch.isfinite(eager[0]).all()
    assert _same(eager, graph) and _same(eager, again)


def test_hires_fix_from_4x12_to_8x24():
    need_gpu()
    a, b, full = hires_chain(HW, SMALL)
    rel = chain_check("hires", a, b, (2, 4) + HW)
    assert rel_l2(a, full) > 10 * 2 * CHAIN_16["hires"], rel_l2(a, full)         # the source was used
