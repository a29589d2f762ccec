"""CPU: LCM sampling - the Philox / Box-Muller generator against known answers, the LCM schedule and boundary scalings against
float64, the guidance-scale embedding, the solvers' plumbing on a mock engine (tests/lcm_mock.py) against the model of
tests/lcm_ref.py, the refusals, the checkpoint reader, the library's LCM header, the seeded ancestral noise, and fault injection:
each deliberate error switched into the model has to break the assertion that guards it."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import lcm_ref as R
from lcm_mock import LCMMockEngine
from mock_engine import StubVAE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, F, D = torch.float16, torch.float32, torch.float64
SQRT_FILE = os.path.join(ROOT, "cfgpp_amd", "data", "ddim_sqrt_tables.npz")


def _rand(shape, seed, scale=1.0, dtype=F):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=D) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------ the generator
def test_philox_known_answers():
    for ctr, key, want in R.KNOWN_ANSWERS:
        assert R.philox4x32_10(ctr, key) == want
    # the vectorised form the other tests use is the scalar one
    ctr, key, want = R.KNOWN_ANSWERS[2]
    w = R.philox_words(3, (key[1] << 32) | key[0], ctr[2], ctr[3], c0_start=ctr[0], c1=ctr[1])
    assert tuple(int(v) for v in w[0]) == want
    assert tuple(int(v) for v in w[2]) == R.philox4x32_10((ctr[0] + 2, ctr[1], ctr[2], ctr[3]), key)
    w = R.philox_words(5, 0x0123456789ABCDEF, 7, 1)
    for q in range(5):
        assert tuple(int(v) for v in w[q]) == R.philox4x32_10((q, 0, 7, 1), (0x89ABCDEF, 0x01234567))


def test_box_muller_model_statistics_and_range():
    n = 1 << 16
    z = R.normals(n, seed=20240601, draw=3, stream_id=0)
    se_mean, se_var = 1.0 / math.sqrt(n), math.sqrt(2.0 / n)
    assert abs(z.mean()) <= 5 * se_mean and abs(z.var() - 1.0) <= 5 * se_var
    u1, u2 = R.uniforms(R.philox_words(n // 4, 20240601, 3, 0))
    assert u1.min() >= 2.0 ** -24 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0      # u1 never reaches 0
    assert np.abs(z).max() <= 5.78
    # the extreme word: u1 = 2^-24 gives the largest magnitude the generator can produce, below the bound
    assert math.sqrt(-2.0 * math.log(2.0 ** -24)) < 5.78
    # both uniforms are exact in fp32
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1) and np.array_equal(u2.astype(np.float32).astype(np.float64), u2)
    # the float32 restatement that sizes the GPU bound stays close to the model
    assert np.abs(R.normals(4096, 5, 0, 0, np.float32).astype(np.float64) - R.normals(4096, 5, 0, 0)).max() < 4e-6


# ------------------------------------------------------------------------------------------------ schedule
def test_timestep_pins_and_refusal():
    from cfgpp_amd.lcm import lcm_timesteps
    assert lcm_timesteps(4) == [999, 759, 499, 259] == R.lcm_timesteps(4)
    assert lcm_timesteps(8) == [999, 879, 759, 639, 499, 379, 259, 139]
    assert lcm_timesteps(2) == [999, 499] and lcm_timesteps(1) == [999]
    for n in (1, 3, 5, 7, 50):
        assert lcm_timesteps(n) == R.lcm_timesteps(n)
    assert lcm_timesteps(4, 25) == R.lcm_timesteps(4, 25)
    with pytest.raises(ValueError, match="original_inference_steps=50"):
        lcm_timesteps(51)
    with pytest.raises(ValueError, match="original_inference_steps=8"):
        lcm_timesteps(9, 8)


def test_boundary_scalings_against_float64():
    from cfgpp_amd.lcm import boundary_scalings
    for t in (999, 759, 499, 259, 139, 19, 0):
        c_skip, c_out = boundary_scalings(t)
        w_skip, w_out = R.boundary_scalings(t)
        assert c_skip == float(np.float32(w_skip)) and c_out == float(np.float32(w_out))
        s = 10.0 * t
        assert abs(w_skip - 0.25 / (s * s + 0.25)) < 1e-18 and abs(w_out - s / math.sqrt(s * s + 0.25)) < 1e-15
    assert boundary_scalings(0) == (1.0, 0.0)                       # the boundary condition: f(x, 0) = x
    assert boundary_scalings(999)[0] < 3e-9 and boundary_scalings(999)[1] == 1.0
    assert boundary_scalings(100, 1.0) == tuple(float(np.float32(v)) for v in R.boundary_scalings(100, 1.0))


def test_guidance_embedding_against_the_formula():
    from cfgpp_amd.lcm import guidance_scale_embedding
    for scale, dim in ((8.5, 256), (1.0, 32), (7.5, 32), (3.0, 8)):
        got = guidance_scale_embedding(scale, dim)
        want = R.guidance_embedding(scale, dim)
        assert len(got) == dim and got == [float(v) for v in want.astype(np.float32)]
        w, half = (scale - 1.0) * 1000.0, dim // 2
        for i in (0, 1, half - 1):
            f = math.exp(-i * math.log(10000.0) / (half - 1))
            assert abs(want[i] - math.sin(w * f)) < 1e-12 and abs(want[half + i] - math.cos(w * f)) < 1e-12
    assert guidance_scale_embedding(1.0, 32) == [0.0] * 16 + [1.0] * 16
    with pytest.raises(ValueError, match="dim=7"):
        guidance_scale_embedding(8.5, 7)


def test_configs_and_param_tables():
    from cfgpp_amd.controlnet import controlnet_param_shapes
    from cfgpp_amd.unet_config import (CONFIGS, SD15, SD15_LCM, SDXL, SDXL_LCM, TINY_SD, TINY_SD_LCM, TINY_XL, TINY_XL_LCM, param_count,
                                       param_shapes, unet_flops_per_row)
    assert SD15.time_cond_proj_dim == 0 == SDXL.time_cond_proj_dim
    assert "time_embedding.cond_proj.weight" not in param_shapes(SD15)       # with 0 nothing changes
    for base, lcm, dim in ((SD15, SD15_LCM, 256), (SDXL, SDXL_LCM, 256), (TINY_SD, TINY_SD_LCM, 32), (TINY_XL, TINY_XL_LCM, 32)):
        assert lcm.time_cond_proj_dim == dim and CONFIGS[lcm.name] is lcm
        a, b = param_shapes(base), param_shapes(lcm)
        c0 = base.block_out_channels[0]
        assert set(b) - set(a) == {"time_embedding.cond_proj.weight"} and b["time_embedding.cond_proj.weight"] == (c0, dim)
        assert "time_embedding.cond_proj.bias" not in b and all(b[k] == a[k] for k in a)
        assert list(b).index("time_embedding.cond_proj.weight") == list(b).index("time_embedding.linear_1.bias") + 1
        assert param_count(lcm) == param_count(base) + c0 * dim
        assert unet_flops_per_row(lcm, 16, 16) == unet_flops_per_row(base, 16, 16)
        assert list(controlnet_param_shapes(lcm)) == list(controlnet_param_shapes(base))      # a ControlNet has no guidance embedding


# ------------------------------------------------------------------------------------------------ solver plumbing on the mock engine
def _unet(z, t, ehs, te, ti):
    v = 0.3 * z.float() * math.cos(0.004 * t) + 0.05 * ehs.float().mean(dim=(1, 2)).view(-1, 1, 1, 1) + 0.02 * math.sin(0.01 * t)
    if te is not None:
        v = v + 0.01 * te.float().mean(dim=1).view(-1, 1, 1, 1)
    return v.half()


def _solver(model="sd15", nfe=4, time_cond=0, **kw):
    from cfgpp_amd.lcm import get_lcm_solver
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    cfg = TINY_SD if model == "sd15" else TINY_XL
    eng = LCMMockEngine(_unet, (8, 8), time_cond_proj_dim=time_cond)
    s = get_lcm_solver("lcm", model=model, solver_config=types.SimpleNamespace(num_sampling=nfe), device="cpu", unet_config=cfg,
                       max_batch=3, latent_hw=(8, 8), engine=eng, vae=StubVAE(cfg.vae_scale), **kw)
    return s, eng, cfg


def _embeds(cfg, B=2, seed=5):
    return _rand((B, 77, cfg.cross_attention_dim), seed, dtype=H), _rand((B, 77, cfg.cross_attention_dim), seed + 1, dtype=H)


def _pair_fn(uc, c, te=None):
    B = c.shape[0]
    ehs = torch.cat([c if uc is None else uc, c], 0)

    def fn(z, t):
        e = _unet(torch.cat([z, z], 0), float(t), ehs, te, None)
        return e[:B].contiguous(), e[B:].contiguous()
    return fn


CASES = [  # (time_cond_proj_dim, cfg_guidance, prediction_type) -> single?, lam
    (0, 1.0, "epsilon"), (0, 1.5, "epsilon"), (0, 1.5, "v_prediction"), (32, 7.5, "epsilon"), (32, None, "v_prediction"),
]


@pytest.mark.parametrize("time_cond,cfg,pt", CASES)
@pytest.mark.parametrize("semantics", ["cpu", "cuda"])
def test_sd_lcm_loop_is_the_model(time_cond, cfg, pt, semantics):
    s, eng, ucfg = _solver(time_cond=time_cond, prediction_type=pt, scalar_semantics=semantics)
    uc, c = _embeds(ucfg)
    zT = _rand((2, 4, 8, 8), 1)
    seeds = [11, (7 << 40) + 5]
    seen = []
    den, zt = s.sample(cfg_guidance=cfg, prompt_embeds=(uc, c), latents=zT, seeds=seeds, return_latents=True,
                       callback_fn=lambda i, t, kw: (seen.append((i, int(t), kw["z0t"].clone())), kw)[1])
    single = bool(time_cond) or cfg <= 1.0
    lam = 1.0 if single else cfg
    sq_a, sq_1ma = R.pinned_sqrt_tables(SQRT_FILE)
    ts = R.lcm_timesteps(4)
    w_den, w_z, rec = R.lcm_chain(_pair_fn(None if single else uc, c), zT, seeds, ts, sq_a, sq_1ma, lam, pred_v=(pt == "v_prediction"),
                                  semantics=semantics)
    assert den.dtype == F and torch.equal(den, w_den) and torch.equal(zt, w_z)
    assert torch.equal(zt, den)                                     # the last step adds no noise
    # launch sequence: per step one UNet call and one step_lcm; the guidance embedding once per job, first
    steps = [v for n, v in eng.lcalls if n == "step_lcm"]
    assert [c_["t"] for c_ in eng.calls] == [float(t) for t in ts] and len(steps) == 4
    assert [n for n, _ in eng.lcalls] == (["guidance_embedding"] if time_cond else []) + ["step_lcm"] * 4
    for i, (st, r) in enumerate(zip(steps, rec)):
        assert st["coef"] == r["coef"] and st["draw"] == i and st["last"] == (i == 3) and st["seeds"] == seeds      # seeds reach the step
        assert st["lam"] == lam and st["pred_v"] == (pt == "v_prediction") and st["single"] == single and not st["noise_given"]
    if time_cond:
        from cfgpp_amd.lcm import guidance_scale_embedding
        assert eng.lcalls[0][1] == guidance_scale_embedding(8.5 if cfg is None else cfg, 32)
    # callbacks get z0t = denoised
    assert [(i, t) for i, t, _ in seen] == list(enumerate(ts)) and torch.equal(seen[-1][2], den)
    # decoded result = the decode of the last step's denoised
    img = s.sample(cfg_guidance=cfg, prompt_embeds=(uc, c), latents=zT, seeds=seeds)
    assert torch.equal(img, (StubVAE(ucfg.vae_scale).decode(den) / 2 + 0.5).clamp(0, 1))


def test_sdxl_lcm_loop_is_the_model():
    for time_cond, cfg in ((0, 1.0), (0, 2.0), (32, 8.0)):
        s, eng, ucfg = _solver("sdxl", time_cond=time_cond, scalar_semantics="cuda")
        uc, c = _embeds(ucfg)
        pool_n, pool = _rand((1, ucfg.addition_pooled_dim), 8, dtype=H), _rand((2, ucfg.addition_pooled_dim), 9, dtype=H)
        zT = _rand((2, 4, 8, 8), 2)
        seeds = [3, 4]
        den, zt = s.sample(cfg_guidance=cfg, prompt_embeds=(uc, c, pool_n, pool), latents=zT, seeds=seeds, return_latents=True,
                           target_size=(64, 64), original_size=(64, 64))
        single = bool(time_cond) or cfg <= 1.0
        te = eng.te
        assert int(te.shape[0]) == 4 and (torch.equal(te[:2], te[2:]) if single else not torch.equal(te[:2], te[2:]))
        sq_a, sq_1ma = R.pinned_sqrt_tables(SQRT_FILE)
        w_den, w_z, _ = R.lcm_chain(_pair_fn(None if single else uc, c, te), zT, seeds, R.lcm_timesteps(4), sq_a, sq_1ma,
                                    1.0 if single else cfg)
        assert torch.equal(den, w_den) and torch.equal(zt, w_z)
        assert [n for n, _ in eng.lcalls] == (["guidance_embedding"] if time_cond else []) + ["step_lcm"] * 4


def test_batched_chains_equal_independent_runs_and_seeds_none():
    s, eng, ucfg = _solver()
    uc, c = _embeds(ucfg, B=3)
    seeds = [101, 202, 303]
    den, zt = s.sample(cfg_guidance=1.5, prompt_embeds=(uc, c), seeds=seeds, return_latents=True)
    for b in range(3):
        d1, z1 = s.sample(cfg_guidance=1.5, prompt_embeds=(uc[b:b + 1], c[b:b + 1]), seeds=seeds[b:b + 1], return_latents=True)
        assert torch.equal(d1[0], den[b]) and torch.equal(z1[0], zt[b])
    # seeds=None: B seeds from torch's CPU generator, once per job, the same for every step; reproducible under manual_seed
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        del eng.lcalls[:]
        runs.append(s.sample(cfg_guidance=1.5, prompt_embeds=(uc, c), return_latents=True)[0])
        used = [v["seeds"] for n, v in eng.lcalls if n == "step_lcm"]
        assert len(used[0]) == 3 and all(u == used[0] for u in used) and len(set(used[0])) == 3
    assert torch.equal(runs[0], runs[1])
    with pytest.raises(ValueError, match="2 seeds for a batch of 3"):
        s.sample(cfg_guidance=1.5, prompt_embeds=(uc, c), latents=_rand((3, 4, 8, 8), 1), seeds=[1, 2])


def test_refusals_by_name():
    from cfgpp_amd.lcm import get_lcm_solver, lcm_solver_names
    assert lcm_solver_names() == ["lcm"]
    with pytest.raises(ValueError, match="LCMSolver lcm_cfg\\+\\+ does not exist"):
        _solver_named("lcm_cfg++")
    with pytest.raises(ValueError, match="LCMSolver model 'sd3'"):
        get_lcm_solver("lcm", model="sd3")
    with pytest.raises(ValueError, match="lcm.*zero_terminal_snr"):
        _solver(zero_terminal_snr=True, prediction_type="v_prediction", timestep_spacing="trailing")
    with pytest.raises(ValueError, match="51 sampling steps.*original_inference_steps=50"):
        _solver(nfe=51)
    with pytest.raises(ValueError, match="9 sampling steps.*original_inference_steps=8"):
        _solver(nfe=9, lcm_original_steps=8)
    s, eng, ucfg = _solver()
    uc, c = _embeds(ucfg)
    for k in ("src_img", "mask"):
        with pytest.raises(ValueError, match=f"lcm.*{k}.*inversion, edit and inpaint"):
            s.sample(cfg_guidance=1.0, prompt_embeds=(uc, c), **{k: torch.zeros(1, 3, 64, 64)})
    with pytest.raises(ValueError, match="lcm.*inversion is not supported"):
        s.inversion(torch.zeros(1, 4, 8, 8), uc, c)
    assert eng.lcalls == [] and eng.calls == []
    # graph replay is never used: the eager loop runs also when the engine offers graphs
    eng.graph_enabled = True
    eng.ddim_loop_graph = lambda *a, **k: (_ for _ in ()).throw(AssertionError("graph replay"))
    s.sample(cfg_guidance=1.0, prompt_embeds=(uc, c), seeds=[1, 2], return_latents=True)
    assert len([1 for n, _ in eng.lcalls if n == "step_lcm"]) == 4


def _solver_named(name):
    from cfgpp_amd.lcm import get_lcm_solver
    return get_lcm_solver(name, solver_config=types.SimpleNamespace(num_sampling=4), device="cpu", engine=LCMMockEngine(_unet))


def test_sharded_run_needs_seeds(monkeypatch):
    import torch.distributed as dist
    s, eng, ucfg = _solver()
    uc, c = _embeds(ucfg)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(ValueError, match="lcm.*sharded run.*seeds"):
        s.sample(cfg_guidance=1.0, prompt_embeds=(uc, c), latents=_rand((2, 4, 8, 8), 1))
    s.sample(cfg_guidance=1.0, prompt_embeds=(uc, c), latents=_rand((2, 4, 8, 8), 1), seeds=[5, 6], return_latents=True)   # its own seeds: fine


# ------------------------------------------------------------------------------------------------ seeded ancestral noise
def _anc_solver(name, **kw):
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    eng = LCMMockEngine(_unet, (8, 8))
    s = get_solver(name, solver_config=types.SimpleNamespace(num_sampling=4), device="cpu", unet_config=TINY_SD, max_batch=3,
                   latent_hw=(8, 8), engine=eng, vae=StubVAE(TINY_SD.vae_scale), **kw)
    return s, eng, TINY_SD


@pytest.mark.parametrize("name", ["euler_a", "euler_a_cfg++", "dpm++_2s_a", "dpm++_2s_a_cfg++"])
def test_ancestral_philox_noise(name):
    s, eng, ucfg = _anc_solver(name, noise="philox")
    uc, c = _embeds(ucfg, B=3)
    seeds = [9, 8, 7]
    den, x = s.sample(cfg_guidance=0.6 if name.endswith("++") else 5.0, prompt_embeds=(uc, c), seeds=seeds, return_latents=True)
    draws = [v for n, v in eng.lcalls if n == "philox_normal"]
    assert [d["draw"] for d in draws] == [0, 1, 2] and all(d["stream_id"] == 1 and d["seeds"] == seeds and d["dtype"] == H for d in draws)
    for b in range(3):           # chain b alone equals chain b of the batch
        d1, x1 = s.sample(cfg_guidance=0.6 if name.endswith("++") else 5.0, prompt_embeds=(uc[b:b + 1], c[b:b + 1]), seeds=seeds[b:b + 1],
                          return_latents=True)
        assert torch.equal(d1[0], den[b]) and torch.equal(x1[0], x[b])
    # the default stays torch.randn_like: no philox launch, the global generator's stream
    s2, eng2, _ = _anc_solver(name)
    assert s2.noise == "torch"
    torch.manual_seed(3)
    a = s2.sample(cfg_guidance=5.0, prompt_embeds=(uc, c), seeds=seeds, return_latents=True)
    torch.manual_seed(3)
    b_ = _anc_solver(name, noise="torch")[0].sample(cfg_guidance=5.0, prompt_embeds=(uc, c), seeds=seeds, return_latents=True)
    assert eng2.lcalls == [] and torch.equal(a[1], b_[1])


def test_philox_noise_is_refused_elsewhere():
    with pytest.raises(ValueError, match="ddim.*noise='philox'.*ancestral"):
        _anc_solver("ddim", noise="philox")
    with pytest.raises(ValueError, match="noise='sobol'"):
        _anc_solver("euler_a", noise="sobol")


# ------------------------------------------------------------------------------------------------ checkpoint directories, CLI
def _write(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f)


def _model_dir(tmp, unet, sched):
    _write(os.path.join(tmp, "unet", "config.json"), unet)
    _write(os.path.join(tmp, "scheduler", "scheduler_config.json"), sched)
    return str(tmp)


SD15_UNET = dict(in_channels=4, attention_head_dim=8, cross_attention_dim=768, use_linear_projection=False, sample_size=64,
                 block_out_channels=[320, 640, 1280, 1280])
SDXL_UNET = dict(in_channels=4, attention_head_dim=[5, 10, 20], cross_attention_dim=2048, use_linear_projection=True, sample_size=128,
                 block_out_channels=[320, 640, 1280])
LCM_SCHED = dict(_class_name="LCMScheduler", original_inference_steps=50, timestep_scaling=10.0, prediction_type="epsilon",
                 timestep_spacing="leading", steps_offset=1)


def test_checkpoint_reader(tmp_path):
    from cfgpp_amd.checkpoint import solver_kwargs_from_dir
    from cfgpp_amd.unet_config import SD15_LCM, SDXL_LCM
    d = _model_dir(tmp_path / "lcm", dict(SD15_UNET, time_cond_proj_dim=256), LCM_SCHED)
    kw, missing = solver_kwargs_from_dir(d, sdxl=False, device="cpu")
    assert kw == dict(unet_config=SD15_LCM, lcm_original_steps=50, timestep_scaling=10.0) and "unet" in missing
    d = _model_dir(tmp_path / "xl", dict(SDXL_UNET, time_cond_proj_dim=256), dict(LCM_SCHED, original_inference_steps=25, timestep_scaling=5.0,
                                                                                    prediction_type="v_prediction"))
    kw, _ = solver_kwargs_from_dir(d, sdxl=True, device="cpu")
    assert kw == dict(unet_config=SDXL_LCM, lcm_original_steps=25, timestep_scaling=5.0, prediction_type="v_prediction")
    d = _model_dir(tmp_path / "odd", dict(SD15_UNET, time_cond_proj_dim=128), dict(prediction_type="epsilon"))
    kw, _ = solver_kwargs_from_dir(d, sdxl=False, device="cpu")
    assert kw["unet_config"].time_cond_proj_dim == 128 and kw["unet_config"].name == "sd15_lcm" and set(kw) == {"unet_config"}
    # a plain directory yields the kwargs it always did
    d = _model_dir(tmp_path / "plain", dict(SD15_UNET, time_cond_proj_dim=None), dict(_class_name="PNDMScheduler", prediction_type="epsilon"))
    assert solver_kwargs_from_dir(d, sdxl=False, device="cpu")[0] == {}
    # the kwargs build a solver with the checkpoint's schedule
    from cfgpp_amd.lcm import get_lcm_solver
    d = _model_dir(tmp_path / "s", SD15_UNET, dict(LCM_SCHED, original_inference_steps=20, timestep_scaling=4.0))
    kw, _ = solver_kwargs_from_dir(d, sdxl=False, device="cpu")
    s = get_lcm_solver("lcm", solver_config=types.SimpleNamespace(num_sampling=4), device="cpu", engine=LCMMockEngine(_unet), **kw)
    assert s.lcm_ts == R.lcm_timesteps(4, 20) and s.timestep_scaling == 4.0
    # and the other solvers ignore them
    from cfgpp_amd.latent_diffusion import get_solver
    get_solver("ddim", solver_config=types.SimpleNamespace(num_sampling=4), device="cpu", engine=LCMMockEngine(_unet), **kw)


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_cli_method_lcm(tmp_path, model):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import text_to_img
    eng = LCMMockEngine(_unet, (8, 8), time_cond_proj_dim=32 if model == "sdxl" else 0)
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    cfg = TINY_SD if model == "sd15" else TINY_XL
    text_to_img.main(["--method", "lcm", "--model", model, "--cfg_guidance", "1.5", "--NFE", "2", "--prompt", "a cat", "--device", "cpu",
                      "--workdir", str(tmp_path), "--lcm_original_steps", "10", "--seed", "4"],
                     solver_kwargs=dict(engine=eng, vae=StubVAE(cfg.vae_scale), latent_hw=(8, 8), unet_config=cfg))
    assert [c["t"] for c in eng.calls] == [float(t) for t in R.lcm_timesteps(2, 10)]
    steps = [v for n, v in eng.lcalls if n == "step_lcm"]
    assert [s["last"] for s in steps] == [False, True] and steps[0]["single"] == (model == "sdxl")
    assert os.path.exists(tmp_path / "result" / "generated.png")


# ------------------------------------------------------------------------------------------------ the extension header
def test_extension_header_is_exported_and_bound():
    from cfgpp_amd import _lib
    from cfgpp_amd.build import SOURCES, build
    assert dict(SOURCES)["lcm_kernels.hip"] == ["-ffp-contract=off"] == dict(SOURCES)["step_kernels.hip"]
    build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cfgpp_lcm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cfgpp_[a-z0-9_]+)\s*\(", code))
    assert declared == {"cfgpp_philox_normal", "cfgpp_step_lcm", "cfgpp_unet_set_time_cond", "cfgpp_unet_guidance_embedding"} \
        == set(_lib.LCM_PROTOTYPES)
    assert all(hasattr(lib, n) for n in declared)
    for name in declared:        # the bound argument count is the declared one
        args = re.search(name + r"\((.*?)\);", code, flags=re.S).group(1)
        assert len(_lib.LCM_PROTOTYPES[name][1]) == args.count(",") + 1, name
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "logf", "sincospif", "Rounding contract".lower(), "(q, 0, draw, stream_id)",
                 "time_embedding.cond_proj"):
        assert word in hdr or word in hdr.lower(), word
    assert '#include "cfgpp.h"' in hdr and "cfgpp_lcm" not in open(os.path.join(ROOT, "include", "cfgpp.h")).read()
    assert "cfgpp_op_philox_raw" in _lib.DEBUG_PROTOTYPES and hasattr(lib, "cfgpp_op_philox_raw")
    assert "cfgpp_op_philox_raw" in open(os.path.join(ROOT, "cfgpp_amd", "csrc", "cfgpp_debug.h")).read()


# ------------------------------------------------------------------------------------------------ fault injection
def _guard_rows_keyed_by_their_own_seed(faults):
    seeds = [5, 6, 7]
    rows = R.normal_rows(3, 64, seeds, 2, 0, faults=faults)
    return all(np.array_equal(rows[b], R.normals(64, seeds[b], 2, 0)) for b in range(3))


def _chain(faults, n=3):
    uc, c = _rand((2, 77, 64), 5, dtype=H), _rand((2, 77, 64), 6, dtype=H)
    sq_a, sq_1ma = R.pinned_sqrt_tables(SQRT_FILE)
    return R.lcm_chain(_pair_fn(uc, c), _rand((2, 4, 8, 8), 1), [1, 2], R.lcm_timesteps(n), sq_a, sq_1ma, 1.5, faults=faults)


def _guard_draw_advances(faults):
    rec = _chain(faults)[2]
    return [r["draw"] for r in rec] == list(range(len(rec)))


def _guard_last_step_adds_no_noise(faults):
    den, z, _ = _chain(faults)
    return torch.equal(den, z)


def _guard_boundary_scalings(faults):
    c_skip, c_out = R.boundary_scalings(999, faults=faults)
    coef = _chain(faults)[2][0]["coef"]
    return c_skip < 1e-8 and abs(c_out - 1.0) < 1e-8 and coef[2] == 1.0 and coef[3] < 1e-8


def _guard_cos_first(faults):
    z = R.normals(8, 1234, 0, 0, faults=faults)
    r = R.philox4x32_10((0, 0, 0, 0), (1234, 0))
    u1, u2 = ((r[0] >> 8) + 1) * 2.0 ** -24, (r[1] >> 8) * 2.0 ** -24
    rho = math.sqrt(-2.0 * math.log(u1))
    return abs(z[0] - rho * math.cos(2 * math.pi * u2)) < 1e-12 and abs(z[1] - rho * math.sin(2 * math.pi * u2)) < 1e-12


def _guard_every_group_is_written(faults):
    z = R.normals(1020, 99, 1, 0, faults=faults)
    r = R.philox4x32_10((254, 0, 1, 0), (99, 0))
    u1, u2 = ((r[2] >> 8) + 1) * 2.0 ** -24, (r[3] >> 8) * 2.0 ** -24
    return abs(z[1018] - math.sqrt(-2.0 * math.log(u1)) * math.cos(2 * math.pi * u2)) < 1e-12 and bool(np.all(z[-4:] != 0))


def _guard_streams_differ(faults):
    a, b = R.normals(64, 42, 0, 0, faults=faults), R.normals(64, 42, 0, 1, faults=faults)
    return not np.array_equal(a, b) and np.array_equal(b[:4], R.normals(4, 42, 0, 1))


FAULTS = [("row0_seed", _guard_rows_keyed_by_their_own_seed), ("draw_stuck", _guard_draw_advances),
          ("noise_on_last", _guard_last_step_adds_no_noise), ("skip_out_swapped", _guard_boundary_scalings),
          ("sincos_swapped", _guard_cos_first), ("last_group_skipped", _guard_every_group_is_written),
          ("stream_ignored", _guard_streams_differ)]


@pytest.mark.parametrize("fault,guard", FAULTS, ids=[f for f, _ in FAULTS])
def test_each_fault_breaks_the_assertion_that_guards_it(fault, guard):
    assert bool(guard(())) is True, "the guard has to hold on the clean model"
    assert bool(guard((fault,))) is False, f"fault {fault!r} went unnoticed"
    # and the fault changes what the chain computes (except the coefficient-only ones, which the guard reads directly)
    if fault in ("draw_stuck", "noise_on_last", "skip_out_swapped", "sincos_swapped"):
        assert not torch.equal(_chain(())[1], _chain((fault,))[1])
