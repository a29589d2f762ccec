"""-m gpu: img2img / latent hires fix on the HIP engine (cfgpp_amd/img2img.py) - 5-step jobs at strength 0.6 (3 steps run) on tiny SD
and tiny SDXL, 16 x 16 latents, 2 chains, from an 8 x 8 ``src_latents`` upscaled bilinear inside the start launch, against the same
solver on a mock engine (tests/img2img_mock.py) whose UNet is the oracle and whose start and steps are the models of tests/img2img_ref.py
/ sde_ref.py / dpmpp_sde_ref.py: the same seeds, therefore the same noise.  One ``src_img`` job through the tiny VAE, a plain
`ddim_cfg++` job on the same engine before and after an img2img job, strength 0.6 against strength 1.

Chain tolerances (the convention of tests/test_gpu_sde_net.py): the final denoised by rel-L2 against the oracle loop, under the project's
chain bar of 7.5e-3 and under twice the value measured on the MI355X (CHAIN_MEASURED below; profiles/img2img/README.md).  Measured: tiny
SDXL `ddim_cfg++` at 0.6 3.849e-4, tiny SD `dpm++_2m_cfg++` at 0.6 1.009e-3, tiny SD `dpm++_2m_sde_cfg++` with noise="philox" 5.359e-4,
tiny SDXL `dpm++_sde` at 7.5 3.162e-3, tiny SD `ddim_cfg++` from ``src_img`` through the tiny VAE 5.601e-4; strength 0.6 against
strength 1 moves the result by 0.78 .. 0.87."""
import types

import pytest
import torch

from img2img_mock import Img2ImgMockEngine

pytestmark = pytest.mark.gpu

CHAIN_BAR = 7.5e-3          # the project's chain bar (tests/test_gpu_pano_net.py)
HW, SMALL = (16, 16), (8, 8)
# (model, solver, options, cfg_guidance)
CASES = {
    "ddim_cfgpp": ("sdxl", "ddim_cfg++", {}, 0.6),
    "2m_cfgpp": ("sd15", "dpm++_2m_cfg++", {}, 0.6),
    "2m_sde_cfgpp_philox": ("sd15", "dpm++_2m_sde_cfg++", dict(noise="philox"), 0.6),
    "dpmpp_sde": ("sdxl", "dpm++_sde", {}, 7.5),
    "ddim_cfgpp_src_img": ("sd15", "ddim_cfg++", {}, 0.6),
}
# measured rel-L2 of the jobs below against the oracle loop -> asserted at twice the value (and under CHAIN_BAR)
CHAIN_MEASURED = {"ddim_cfgpp": 3.849e-4, "2m_cfgpp": 1.009e-3, "2m_sde_cfgpp_philox": 5.359e-4, "dpmpp_sde": 3.162e-3,
                  "ddim_cfgpp_src_img": 5.601e-4}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def _cfg(model):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    return TINY_SD if model == "sd15" else TINY_XL


def _solver(model, name, hw=HW, **kw):
    from cfgpp_amd.img2img import get_img2img_solver
    return get_img2img_solver(name, model=model, solver_config=types.SimpleNamespace(num_sampling=5), unet_config=_cfg(model), max_batch=2,
                              latent_hw=hw, scalar_semantics="cuda", **kw)


def _embeds(s, model):
    if model == "sd15":
        return s.get_text_embed("bad", ["a cat", "a dog"])
    return s.get_text_embed("bad", ["a cat", "a dog"], "bad", ["a cat", "a dog"])


def _sample(s, model, pe, seeds, lam, **kw):
    if model == "sdxl":
        kw = dict(dict(target_size=(128, 128), original_size=(128, 128)), **kw)
    out = s.sample(cfg_guidance=lam, prompt_embeds=pe, seeds=seeds, return_latents=True, **kw)
    return (out[0] if isinstance(out, (tuple, list)) else out).clone()


class OracleMock(Img2ImgMockEngine):
    """the mock engine whose UNet is the oracle"""

    def __init__(self, cfg, sd, hw=HW):
        from oracle.unet_ref import UNetRef
        self.net = UNetRef(cfg, sd)
        super().__init__(self._unet, hw)

    def _unet(self, z, t, ehs, te, ti):
        ack = None if te is None else {"text_embeds": te.float(), "time_ids": ti.float()}
        return self.net(z.float(), t, ehs.float(), ack)["sample"].half()


class MeanVAE:
    """the posterior mean of the tiny VAE, on the HIP encoder or on the CPU restatement (oracle/vae_ref.py)"""

    def __init__(self, kind, scale, sd):
        self.kind, self.scale = kind, scale
        if kind == "hip":
            from cfgpp_amd.vae import HipVAE
            self.v = HipVAE(scale, HW, max_batch=2, state_dict=sd)
        else:
            from oracle.vae_ref import VAERef
            self.v = VAERef(scale, device="cpu", dtype=torch.float32, state_dict=sd)

    def encode(self, x, sample=True):
        assert sample is False, "img2img encodes the posterior mean"
        if self.kind == "hip":
            return self.v.encode(x, sample=False)
        return self.v.encode_moments(x.float().cpu())[0] * self.scale

    def decode(self, z):
        return self.v.decode(z)


def _source(case, hw=HW, small=SMALL):
    g = torch.Generator().manual_seed(31)
    if case.endswith("src_img"):
        return dict(src_img=torch.rand((2, 3, 8 * hw[0], 8 * hw[1]), generator=g) * 2 - 1)
    return dict(src_latents=torch.randn((2, 4) + small, generator=g), upscale="bilinear")


@pytest.mark.parametrize("case", list(CASES))
def test_job_vs_oracle_loop(case):
    need_gpu()
    from cfgpp_amd.vae import synth_vae_state_dict
    from cfgpp_amd.weights import synth_state_dict
    model, name, opts, lam = CASES[case]
    cfg = _cfg(model)
    hip = _solver(model, name, device="cuda", **opts)
    eng = OracleMock(cfg, synth_state_dict(cfg, 0))
    ref = _solver(model, name, device="cpu", text_encoder=hip.text_encoder, engine=eng, **opts)
    if case.endswith("src_img"):
        vsd = synth_vae_state_dict(0)
        hip.vae, ref.vae = MeanVAE("hip", cfg.vae_scale, vsd), MeanVAE("cpu", cfg.vae_scale, vsd)
    pe = _embeds(hip, model)
    seeds, src = [11, 12], _source(case)
    a = _sample(hip, model, pe, seeds, lam, strength=0.6, **src)
    b = _sample(ref, model, tuple(x.cpu() for x in pe), seeds, lam, strength=0.6, **src)
    assert hip.last_start == ref.last_start and hip.last_start["i0"] == 2 and hip.last_start["steps"] == 3
    assert hip.last_start["mode"] == ("identity" if case.endswith("src_img") else "bilinear")
    assert len(eng.icalls) == 1 and len(eng.calls) == (5 if name == "dpm++_sde" else 3)
    rel = rel_l2(a, b)
    full = _sample(hip, model, pe, seeds, lam, strength=1.0, **src)          # strength 1: the text-to-image job
    moved = rel_l2(a, full)
    print(f"{case}: img2img job rel-L2 {rel:.3e}; strength 0.6 vs 1 {moved:.3e}")
    assert a.shape == (2, 4) + HW and torch.isfinite(a).all() and float(a.float().std()) > 0
    assert rel < CHAIN_BAR, rel
    tol = 2 * CHAIN_MEASURED[case]
    assert rel < tol, rel
    assert moved > 10 * tol, moved
    # batched chains equal independent runs, bit for bit; the same seeds again: the same bits
    for b_ in range(2):
        pe_b = tuple(x[b_:b_ + 1] if x.shape[0] == 2 else x for x in pe)
        src_b = {k: (v[b_:b_ + 1] if torch.is_tensor(v) else v) for k, v in src.items()}
        if "src_img" in src:
            # the posterior mean draws nothing, so a chain's source does not depend on its neighbours' noise; whether the encoder's own
            # bits depend on its batch size is the VAE's business (its tiles are chosen by the row count): where they do, chain b alone is
            # started from the batch's latent for chain b
            zb = hip.vae.encode(src["src_img"].cuda(), sample=False)[b_:b_ + 1]
            z1 = hip.vae.encode(src_b["src_img"].cuda(), sample=False)
            print(f"{case}: VAE posterior mean of image {b_}, batch of 2 vs alone: max abs difference {float((zb - z1).abs().max()):.3e}")
            if not torch.equal(zb, z1):
                src_b = dict(src_latents=zb.to(hip.dtype))
        one = _sample(hip, model, pe_b, seeds[b_:b_ + 1], lam, strength=0.6, **src_b)
        assert torch.equal(one[0], a[b_]), f"chain {b_} alone differs from chain {b_} of the batch"
    assert torch.equal(_sample(hip, model, pe, seeds, lam, strength=0.6, **src), a)
    assert not torch.equal(_sample(hip, model, pe, [11, 13], lam, strength=0.6, **src)[1], a[1])


def test_plain_engine_gives_the_same_bits_around_an_img2img_job():
    need_gpu()
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    mk = lambda: get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=5), device="cuda", unet_config=TINY_SD,  # noqa: E731
                            max_batch=2, latent_hw=HW, scalar_semantics="cuda")
    s = mk()
    pe = s.get_text_embed("bad", ["a cat", "a dog"])
    run = lambda sv: [t.clone() for t in sv.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=[5, 6], return_latents=True)]  # noqa: E731
    before = run(s)
    i2i = _solver("sd15", "dpm++_2m_sde_cfg++", device="cuda", engine=s.engine, text_encoder=s.text_encoder, noise="philox")
    den = _sample(i2i, "sd15", pe, [5, 6], 0.6, strength=0.6, **_source("x"))
    assert torch.isfinite(den).all()
    s._ctx_key = None                                                # the img2img job set the engine's context: the next job sets its own
    after = run(s)
    fresh = run(mk())
    for a, b, w in zip(before, after, fresh):
        assert torch.equal(a, b) and torch.equal(a, w)


def test_hires_fix_on_two_engines():
    """a 8 x 8 `ddim_cfg++` job, its latent upscaled bicubic into a 16 x 16 `dpm++_2m_cfg++` job at strength 0.6: equal to the two calls
    made by hand, and decodable"""
    need_gpu()
    from cfgpp_amd.img2img import hires_fix
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    first = get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=4), device="cuda", unet_config=TINY_SD, max_batch=2,
                       latent_hw=SMALL, scalar_semantics="cuda")
    second = _solver("sd15", "dpm++_2m_cfg++", device="cuda", text_encoder=first.text_encoder)
    pe = first.get_text_embed("bad", ["a cat", "a dog"])
    out = hires_fix(first, second, 0.6, None, strength=0.6, upscale="bicubic", seeds=[7, 8], prompt_embeds=pe, second_kw=dict(return_latents=True))
    z = first.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=[7, 8], return_latents=True)[0]
    first._ctx_key = None
    want = second.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=[7, 8], src_latents=z, strength=0.6, upscale="bicubic", return_latents=True)
    assert tuple(z.shape) == (2, 4) + SMALL and all(torch.equal(a, b) for a, b in zip(out, want))
    assert second.last_start["mode"] == "bicubic" and out[0].shape == (2, 4) + HW and torch.isfinite(out[0].float()).all()
