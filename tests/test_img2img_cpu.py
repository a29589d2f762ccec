"""cfgpp_amd/img2img.py without a GPU, on the mock engine of tests/img2img_mock.py: the registry and its refusals, strength 1 against the
text-to-image solvers bit for bit, the strength rule, the (a, s) and schedule tail handed to the start and the loop, the DDIM job against
the all-ones-mask inpaint job, every refusal by name, ``hires_fix``' call order, the two command lines."""
import math
import os
import types

import numpy as np
import pytest
import torch

from img2img_mock import Img2ImgMockEngine
from inpaint_mock import InpaintMockEngine
from mock_engine import StubVAE

import cfgpp_amd.latent_diffusion as sd
import cfgpp_amd.latent_sdxl as xl
from cfgpp_amd import img2img as I2I
from cfgpp_amd.dpmpp_sde import get_dpmpp_sde_solver
from cfgpp_amd.inpaint import get_inpaint_solver, strength_timesteps
from cfgpp_amd.sde import get_sde_solver
from cfgpp_amd.unet_config import TINY_SD, TINY_XL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = torch.float16
HW = (8, 8)
SD_NAMES = ["ddim", "ddim_cfg++", "euler", "euler_cfg++", "dpm++_2m", "dpm++_2m_cfg++", "dpm++_2m_sde", "dpm++_2m_sde_cfg++",
            "dpm++_3m_sde", "dpm++_3m_sde_cfg++", "dpm++_sde", "dpm++_sde_cfg++"]
XL_NAMES = [n for n in SD_NAMES if not n.startswith("dpm++_2m") or "sde" in n]
ALL = [("sd15", n) for n in SD_NAMES] + [("sdxl", n) for n in XL_NAMES]


def cfgn(n):
    return types.SimpleNamespace(num_sampling=n)


def _rand(shape, seed, dtype=torch.float32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _unet(z, t, ehs, te, ti):
    v = 0.3 * z.float() * math.cos(0.004 * t) + 0.05 * ehs.float().mean(dim=(1, 2)).view(-1, 1, 1, 1) + 0.02 * math.sin(0.01 * t)
    if te is not None:
        v = v + 0.01 * te.float().mean(dim=1).view(-1, 1, 1, 1)
    return v.half()


def _cfg(model):
    return TINY_SD if model == "sd15" else TINY_XL


def _kw(model, nfe, eng, hw=HW, **kw):
    cfg = _cfg(model)
    return dict(solver_config=cfgn(nfe), device="cpu", unet_config=cfg, max_batch=3, latent_hw=hw, engine=eng, vae=StubVAE(cfg.vae_scale), **kw)


def _i2i(name, model="sd15", nfe=5, hw=HW, eng=None, **kw):
    eng = eng or Img2ImgMockEngine(_unet, hw)
    return I2I.get_img2img_solver(name, model=model, **_kw(model, nfe, eng, hw, **kw)), eng


def _t2i(name, model, nfe, eng, **kw):
    if "sde" in name:
        get = get_dpmpp_sde_solver if name.startswith("dpm++_sde") else get_sde_solver
        return get(name, model=model, **_kw(model, nfe, eng, **kw))
    return (sd if model == "sd15" else xl).get_solver(name, **_kw(model, nfe, eng, **kw))


def _pe(model, B=2, seed=5):
    cfg = _cfg(model)
    uc, c = _rand((B, 77, cfg.cross_attention_dim), seed, H), _rand((B, 77, cfg.cross_attention_dim), seed + 1, H)
    if model == "sd15":
        return (uc, c)
    return (uc, c, _rand((B, cfg.addition_pooled_dim), seed + 2, H), _rand((B, cfg.addition_pooled_dim), seed + 3, H))


def _run(s, model, pe, seeds, lam=0.6, **kw):
    if model == "sdxl":
        kw = dict(dict(target_size=(8 * HW[0], 8 * HW[1]), original_size=(8 * HW[0], 8 * HW[1])), **kw)
    out = s.sample(cfg_guidance=lam, prompt_embeds=pe, seeds=seeds, return_latents=True, **kw)
    return [t.clone() for t in (out if isinstance(out, (tuple, list)) else (out,))]


def _lat(B=2, hw=HW, seed=9, dtype=torch.float32):
    return _rand((B, 4) + tuple(hw), seed, dtype)


# ---- the registry ---------------------------------------------------------------------------------------------------------------
def test_registry_of_its_own():
    assert I2I.img2img_solver_names("sd15") == sorted(SD_NAMES) and I2I.img2img_solver_names("sdxl") == sorted(XL_NAMES)
    for model, name in ALL:
        cls = I2I.__IMG2IMG_SOLVER__[f"{model}/{name}"]
        assert issubclass(cls, I2I._Img2ImgMixin) and issubclass(cls, xl.SDXL if model == "sdxl" else sd.StableDiffusion)
        assert (issubclass(cls, xl.SDXL)) == (model == "sdxl") and cls.solver_name == name
    # the text-to-image registries are untouched: no new name, and their classes are not the img2img ones
    assert not any(issubclass(c, I2I._Img2ImgMixin) for c in list(sd.__SOLVER__.values()) + list(xl.__SOLVER__.values()))
    with pytest.raises(ValueError, match="Img2ImgSolver model 'sd3'"):
        I2I.get_img2img_solver("ddim", model="sd3")
    with pytest.raises(ValueError, match="Img2ImgSolver nope does not exist"):
        I2I.get_img2img_solver("nope")
    with pytest.raises(ValueError, match=r"dpm\+\+_2m_cfg\+\+: model 'sdxl' has no text-to-image solver"):
        I2I.get_img2img_solver("dpm++_2m_cfg++", model="sdxl")


@pytest.mark.parametrize("name,word", [("euler_a", "ancestral"), ("dpm++_2s_a_cfg++", "ancestral"), ("euler_lightning", "Lightning"),
                                       ("ddim_cfg++_lightning", "Lightning"), ("ddim_inversion", "inversion / edit"),
                                       ("ddim_edit_cfg++", "inversion / edit"), ("lcm", "LCM"), ("ddim_inpaint", "get_inpaint_solver"),
                                       ("ddim_panorama_cfg++", "panorama")])
def test_names_of_other_registries_are_refused_by_name(name, word):
    for model in I2I.MODELS:
        with pytest.raises(ValueError, match=f"Img2ImgSolver {name.replace('+', chr(92) + '+')}: .*{word}"):
            I2I.get_img2img_solver(name, model=model)


def test_the_text_to_image_solvers_keep_refusing():
    eng = Img2ImgMockEngine(_unet, HW)
    for get, name in ((get_sde_solver, "dpm++_2m_sde"), (get_dpmpp_sde_solver, "dpm++_sde")):
        s = get(name, **_kw("sd15", 3, eng))
        with pytest.raises(ValueError, match="strength=... - inversion, edit and inpaint jobs are not supported"):
            s.sample(cfg_guidance=0.6, prompt_embeds=_pe("sd15"), seeds=[1, 2], strength=0.5)


# ---- strength 1 is the text-to-image job ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,name", ALL)
def test_strength_1_is_the_text_to_image_job_bit_for_bit(model, name):
    s, eng = _i2i(name, model)
    ref = _t2i(name, model, 5, Img2ImgMockEngine(_unet, HW))
    pe, seeds = _pe(model), [11, 12]
    got = _run(s, model, pe, seeds, src_latents=_lat(), strength=1.0)
    want = _run(ref, model, pe, seeds)
    assert len(got) == len(want) and all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    (call,) = eng.icalls
    assert call["a"] == 0.0 and call["src"] is None and call["noise_given"] and call["mode"] == "identity"
    assert s.last_start["i0"] == 0 and s.last_start["steps"] == 5
    # ... and the source plays no part
    assert all(torch.equal(a, b) for a, b in zip(_run(s, model, pe, seeds, src_latents=_lat(seed=10), strength=1.0), want))


# ---- the strength rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 20, 50])
def test_strength_rule_is_get_timesteps(n):
    from cfgpp_amd.schedule import SchedulerTables
    ts = SchedulerTables(n).timesteps
    for name in ("ddim_cfg++", "dpm++_2m", "dpm++_3m_sde_cfg++", "dpm++_sde"):
        s, eng = _i2i(name, nfe=n)
        for strength in (0.21, 0.5, 0.6, 0.75, 0.999, 1.0):
            want_ts, i0 = strength_timesteps(ts, strength)
            assert s._strength_index(dict(strength=strength)) == i0 == n - min(int(n * strength), n) and len(want_ts) == n - i0
        assert s._strength_index({}) == n - int(n * 0.75)             # the default strength
        with pytest.raises(ValueError, match=f"'{name.replace('+', chr(92) + '+')}': strength=0.01 leaves no denoising step of {n}"):
            s._strength_index(dict(strength=0.01))


@pytest.mark.parametrize("model,name", ALL)
def test_start_and_tail_are_the_tables(model, name):
    """the (a, s) of the start launch, the first sigma / timestep of the loop and its step count, for N = 5 at strength 0.6 (i0 = 2)"""
    s, eng = _i2i(name, model)
    pe, seeds = _pe(model), [3, 4]
    z = _lat(hw=(4, 4), dtype=H)
    _run(s, model, pe, seeds, src_latents=z, strength=0.6, upscale="bicubic")
    (call,) = eng.icalls
    assert s.last_start == dict(i0=2, steps=3, a=call["a"], s=call["s"], mode="bicubic", noise="torch")
    assert call["mode"] == "bicubic" and torch.equal(call["src"], z) and call["shape"] == (2, 4, 8, 8)
    t_first = eng.calls[0]["t"]
    if name.startswith("ddim"):
        ts = s.scheduler.timesteps[2:]
        c1, c2 = s.tables.ddim_sqrt_coeffs(ts[0], wrap=(model == "sdxl"))[:2]
        assert (call["a"], call["s"]) == (c2, c1) and call["x_dtype"] == torch.float32
        assert [c["t"] for c in eng.calls] == [float(t) for t in (ts.int() if model == "sdxl" else ts)]
    else:
        if "sde" in name:
            sigmas = s.sde_sigmas()
        elif model == "sdxl" and name == "euler_cfg++":
            sigmas = s._xl_sigmas()
        else:
            sigmas = s.tables.karras_sigmas()
        assert len(sigmas) == 6 and (call["a"], call["s"]) == (1.0, float(sigmas[2]))
        assert call["x_dtype"] == (torch.float32 if "sde" in name else H)
        assert t_first == float(s.timestep(sigmas[2]))
        n_unet = 3 if not name.startswith("dpm++_sde") else 2 * 3 - 1
        assert len(eng.calls) == n_unet
        if "sde" in name:                                  # the loop got the tail: its first input scale is sigma_2's
            from cfgpp_amd.sde import input_scale
            assert eng.scalls[0] == ("sde_input", dict(eng.scalls[0][1], s_in=input_scale(sigmas[2])))
    # the start is the model's: a * bicubic(z) + s * n
    import img2img_ref as M
    n = s._randn((2, 4, 8, 8), seeds).numpy()
    want, _ = M.start(z.double().numpy(), n, call["a"], call["s"], 2, 8, 8, 3, call["x_dtype"] == H, np.float32)
    assert np.array_equal(call["x"].double().numpy(), want)


def test_philox_start_keys_the_chains_and_needs_seeds_when_sharded(monkeypatch):
    s, eng = _i2i("dpm++_2m_sde_cfg++", noise="philox")
    pe = _pe("sd15")
    a = _run(s, "sd15", pe, [7, 8], src_latents=_lat(), strength=0.6)[0]
    (call,) = eng.icalls
    assert call["seeds"] == [7, 8] and not call["noise_given"] and s.last_start["noise"] == "philox"
    assert all(k["seeds"] == [7, 8] for nm, k in eng.scalls if nm == "step_sde")
    for b in range(2):                                     # chain b of the batch is chain b alone
        one = _run(s, "sd15", tuple(t[b:b + 1] for t in pe), [7 + b], src_latents=_lat()[b:b + 1], strength=0.6)[0]
        assert torch.equal(one[0], a[b])
    assert not torch.equal(_run(s, "sd15", pe, [7, 9], src_latents=_lat(), strength=0.6)[0][1], a[1])
    with pytest.raises(ValueError, match="noise='gauss'"):
        _i2i("ddim", noise="gauss")
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(ValueError, match="noise='philox' in a sharded run .* needs seeds"):
        _i2i("ddim_cfg++", noise="philox")[0].sample(cfg_guidance=0.6, prompt_embeds=pe, src_latents=_lat(), strength=0.6)


# ---- DDIM img2img is the all-ones-mask inpaint job -----------------------------------------------------------------------------
@pytest.mark.parametrize("model,name", [("sd15", "ddim"), ("sd15", "ddim_cfg++"), ("sdxl", "ddim_cfg++")])
def test_ddim_job_is_the_all_ones_mask_inpaint_job(model, name):
    """``get_inpaint_solver`` with an all-ones mask on a 4-channel UNet is the documented DDIM img2img.  Same seeds, same strength: the
    start latents and every state of the loop agree bit for bit - the last step included: its clean-source blend replaces the elements
    OUTSIDE the mask, and an all-ones mask has none."""
    cfg = _cfg(model)
    hw = (16, 16)
    ieng = InpaintMockEngine(_unet, hw)
    inp = get_inpaint_solver(name.replace("ddim", "ddim_inpaint"), model=model, **_kw(model, 5, ieng, hw))
    s, eng = _i2i(name, model, hw=hw)
    g = torch.Generator().manual_seed(3)
    img = torch.rand(2, 3, 128, 128, generator=g) * 2 - 1
    pe, seeds = _pe(model), [21, 22]
    xlkw = dict(target_size=(128, 128), original_size=(128, 128)) if model == "sdxl" else {}
    seen_a, seen_b = [], []
    cb = lambda store: (lambda i, t, kw: (store.append((int(i), kw["z0t"].clone(), kw["zt"].clone())), kw)[1])  # noqa: E731
    a = inp.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=seeds, src_img=img, mask=torch.ones(1, 1, 128, 128), strength=0.6,
                   return_latents=True, callback_fn=cb(seen_a), **xlkw)
    b = s.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=seeds, src_img=img, strength=0.6, return_latents=True, callback_fn=cb(seen_b),
                 **xlkw)
    assert len(seen_a) == len(seen_b) == 3
    for (i, z0a, za), (j, z0b, zb) in zip(seen_a, seen_b):
        assert i == j and torch.equal(z0a, z0b) and torch.equal(za, zb)
    a, b = (a[0] if isinstance(a, tuple) else a), (b[0] if isinstance(b, tuple) else b)
    assert torch.equal(a, b)
    # the source went through the VAE's posterior mean, rounded to the pipeline dtype
    (call,) = eng.icalls
    assert call["mode"] == "identity" and call["src"].dtype == H and torch.equal(call["src"], StubVAE(cfg.vae_scale).encode(img).to(H))
    assert call["a"] != 0.0 and torch.equal(ieng.calls[0]["z"], eng.calls[0]["z"])


def test_src_img_uses_the_posterior_mean_unless_asked():
    class Vae(StubVAE):
        seen = []

        def encode(self, x, **kw):
            self.seen.append(kw)
            return super().encode(x)
    s, eng = _i2i("ddim_cfg++", hw=(8, 8))
    s.vae = Vae(TINY_SD.vae_scale)
    img = torch.rand(1, 3, 64, 64) * 2 - 1
    pe = _pe("sd15")
    _run(s, "sd15", pe, [1, 2], src_img=img, strength=0.6)
    _run(s, "sd15", pe, [1, 2], src_img=img, strength=0.6, sample_posterior=True)
    assert Vae.seen == [dict(sample=False), {}]
    assert eng.icalls[0]["src"].shape == (1, 4, 8, 8)           # one source row, broadcast to both chains by the kernel
    _run(s, "sd15", pe, [1, 2], src_img=img, strength=1.0)        # strength 1 drops the source: nothing is encoded
    assert len(Vae.seen) == 2


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,name", [("sd15", "ddim_cfg++"), ("sd15", "euler"), ("sdxl", "dpm++_2m_sde_cfg++"), ("sdxl", "dpm++_sde")])
def test_every_refusal_is_raised_by_name(model, name):
    s, eng = _i2i(name, model)
    pe = _pe(model)
    nm = f"'{name}'".replace("+", "\\+")
    run = lambda **kw: _run(s, model, pe, [1, 2], **kw)  # noqa: E731
    z = _lat()
    for kw, msg in ((dict(), "needs a source"),
                    (dict(src_latents=z, src_img=torch.zeros(2, 3, 64, 64)), "src_img or src_latents, not both"),
                    (dict(src_latents=_lat(hw=(9, 8))), "larger than the engine's latent 8 x 8: downscaling is not built"),
                    (dict(src_latents=_lat(hw=(4, 16))), "larger than the engine's latent"),
                    (dict(src_img=torch.zeros(2, 3, 32, 32)), "pixel-space upscalers are not built"),
                    (dict(src_img=torch.zeros(3, 3, 64, 64)), r"src_img shape \(3, 3, 64, 64\)"),
                    (dict(src_latents=_lat()[:, :3]), "src_latents shape"),
                    (dict(src_latents=z, strength=0.0), r"strength=0.0: a number in \(0, 1\]"),
                    (dict(src_latents=z, strength=1.5), r"strength=1.5: a number in \(0, 1\]"),
                    (dict(src_latents=z, strength=float("nan")), r"strength=nan"),
                    (dict(src_latents=z, strength=0.1), "strength=0.1 leaves no denoising step of 5"),
                    (dict(src_latents=z, upscale="lanczos"), "upscale='lanczos'"),
                    (dict(src_latents=z, mask=torch.ones(1, 1, 64, 64)), "mask=... is not an img2img argument"),
                    (dict(src_latents=z, latents=z), "latents=... is not an img2img argument")):
        with pytest.raises(ValueError, match=f"{nm}: .*{msg}"):
            run(**kw)
    assert eng.icalls == [] and eng.calls == []              # refused before anything ran
    # the refusals hold when strength 1 would drop the source
    with pytest.raises(ValueError, match="downscaling is not built"):
        run(src_latents=_lat(hw=(9, 8)), strength=1.0)


def test_an_engine_without_the_start_is_refused():
    from dpmpp_sde_mock import DPMppSDEMockEngine
    s, _ = _i2i("ddim", eng=DPMppSDEMockEngine(_unet, HW))
    with pytest.raises(ValueError, match="the engine DPMppSDEMockEngine has no img2img_start"):
        _run(s, "sd15", _pe("sd15"), [1, 2], src_latents=_lat())


# ---- hires fix ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_hires_fix_calls_first_then_second_with_the_firsts_latent(model):
    small, big = (4, 4), (8, 8)
    e1, e2 = Img2ImgMockEngine(_unet, small), Img2ImgMockEngine(_unet, big)
    first = (sd if model == "sd15" else xl).get_solver("ddim_cfg++", **_kw(model, 4, e1, small))
    second, _ = _i2i("dpm++_2m_sde_cfg++", model, nfe=5, hw=big, eng=e2)
    order = []
    f_sample, s_sample = first.sample, second.sample
    first.sample = lambda *a, **k: (order.append(("first", k)), f_sample(*a, **k))[1]
    second.sample = lambda *a, **k: (order.append(("second", k)), s_sample(*a, **k))[1]
    pe = _pe(model)
    fkw = dict(target_size=(32, 32), original_size=(32, 32)) if model == "sdxl" else {}
    out = I2I.hires_fix(first, second, 0.6, ["", "a cat"], strength=0.6, upscale="bicubic", seeds=[5, 6], prompt_embeds=pe, first_kw=fkw,
                        second_kw=dict(return_latents=True))
    assert [o[0] for o in order] == ["first", "second"]
    assert order[0][1]["return_latents"] is True and order[0][1]["seeds"] == [5, 6]
    k2 = order[1][1]
    lat = f_sample(cfg_guidance=0.6, seeds=[5, 6], return_latents=True, prompt_embeds=pe, **fkw)
    z = lat[0] if isinstance(lat, tuple) else lat
    assert torch.equal(k2["src_latents"], z) and tuple(z.shape) == (2, 4, 4, 4)
    assert k2["strength"] == 0.6 and k2["upscale"] == "bicubic" and k2["seeds"] == [5, 6]
    (call,) = e2.icalls
    assert call["mode"] == "bicubic" and torch.equal(call["src"], z.to(call["src"].dtype)) and call["shape"] == (2, 4, 8, 8)
    den = out[0]
    assert den.shape == (2, 4, 8, 8) and torch.isfinite(den).all()
    with pytest.raises(ValueError, match="second must be an img2img solver"):
        I2I.hires_fix(first, first, 0.6, ["", "a cat"])


def test_hires_fix_takes_prompts_for_both_families():
    """without prompt_embeds: ``prompt`` goes to an SD1.5 solver as prompt=, to both towers of an SDXL one"""
    seen = []

    class Fake:
        latent_hw = (4, 4)

        def sample(self, **k):
            seen.append(k)
            return (torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4))
    second, _ = _i2i("ddim", "sdxl")
    second.sample = lambda **k: seen.append(k)
    I2I.hires_fix(Fake(), second, 5.0, ["", "a fox"])
    assert seen[0]["prompt"] == ["", "a fox"] and seen[1]["prompt"] == ["", "a fox"] and seen[1]["strength"] == 0.5
    assert seen[1]["upscale"] == "bilinear" and seen[1]["src_latents"].shape == (1, 4, 4, 4)


# ---- the command lines ----------------------------------------------------------------------------------------------------------------
def _examples():
    import sys
    p = os.path.join(ROOT, "examples")
    if p not in sys.path:
        sys.path.insert(0, p)


@pytest.mark.parametrize("model,method", [("sd15", "ddim_cfg++"), ("sdxl", "dpm++_sde_cfg++")])
def test_img2img_command_line(tmp_path, model, method):
    from PIL import Image
    _examples()
    import img2img as cli
    src = tmp_path / "src.png"
    Image.fromarray((np.random.default_rng(0).random((40, 56, 3)) * 255).astype(np.uint8)).save(src)
    cfg = _cfg(model)
    eng = Img2ImgMockEngine(_unet, HW)
    cli.main(["--src_img", str(src), "--strength", "0.6", "--method", method, "--model", model, "--NFE", "5", "--cfg_guidance", "0.6",
              "--prompt", "a cat", "--device", "cpu", "--workdir", str(tmp_path), "--seed", "4", "--batch", "2", "--noise", "philox",
              "--eta", "0.5"], solver_kwargs=dict(engine=eng, vae=StubVAE(cfg.vae_scale), latent_hw=HW, unet_config=cfg))
    (call,) = eng.icalls
    assert call["seeds"] == [4, 5] and call["mode"] == "identity" and call["src"].shape == (1, 4, 8, 8) and call["a"] != 0.0
    assert sorted(p.name for p in (tmp_path / "result").glob("*.png")) == ["img2img_0.png", "img2img_1.png"]
    assert Image.open(tmp_path / "result" / "img2img_0.png").size == (64, 64)
    with pytest.raises(SystemExit):
        cli.main(["--method", method, "--model", model, "--device", "cpu", "--workdir", str(tmp_path)])      # no --src_img


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_hires_fix_command_line(tmp_path, model):
    from PIL import Image
    _examples()
    import hires_fix as cli
    cfg = _cfg(model)
    e1, e2 = Img2ImgMockEngine(_unet, (4, 4)), Img2ImgMockEngine(_unet, (6, 6))
    mk = lambda e, hw: dict(engine=e, vae=StubVAE(cfg.vae_scale), unet_config=cfg)  # noqa: E731
    z0ts, step = [], e1.step_ddim
    e1.step_ddim = lambda z, z0t_out, *a, **k: (step(z, z0t_out, *a, **k), z0ts.append(z0t_out.clone()))[0]   # the first pass's z0t
    cli.main(["--method", "ddim_cfg++", "--hires_method", "dpm++_2m_sde_cfg++", "--model", model, "--NFE", "4", "--hires_NFE", "5",
              "--cfg_guidance", "0.6", "--prompt", "a cat", "--device", "cpu", "--workdir", str(tmp_path), "--seed", "4", "--img_size", "32",
              "--hires_scale", "1.5", "--hires_strength", "0.6", "--hires_upscaler", "bicubic"],
             solver_kwargs=mk(e1, (4, 4)), hires_solver_kwargs=mk(e2, (6, 6)))
    assert e1.icalls == [] and len(e1.calls) == 4
    (call,) = e2.icalls
    assert call["mode"] == "bicubic" and call["src"].shape == (1, 4, 4, 4) and call["shape"] == (1, 4, 6, 6) and len(e2.calls) == 3
    assert len(z0ts) == 4 and torch.equal(call["src"].float(), z0ts[-1].float())
    assert Image.open(tmp_path / "result" / "hires.png").size == (48, 48)
    with pytest.raises(SystemExit):
        cli.main(["--hires_upscaler", "lanczos", "--device", "cpu", "--workdir", str(tmp_path)])
    with pytest.raises(SystemExit):
        cli.main(["--hires_scale", "0.5", "--device", "cpu", "--workdir", str(tmp_path)])
