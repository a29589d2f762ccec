"""CPU: v-prediction, zero-terminal-SNR / trailing schedules, guidance rescale and SD2.x configs - the arithmetic against float64
and torch-CPU restatements (tests/vpred_ref.py), the solver loops on a mock engine (tests/vpred_mock.py), the refusals, the
checkpoint-directory plumbing and the library's v-prediction header."""
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import vpred_ref as R
from mock_engine import StubVAE
from vpred_mock import VPredMockEngine, emulate_step_ddim_v, emulate_v_to_eps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, F, D = torch.float16, torch.float32, torch.float64


def _rand(shape, seed, scale=1.0, dtype=F):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=D) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------ the update in float64
@pytest.mark.parametrize("inversion", [False, True])
@pytest.mark.parametrize("tweedie_uc,renoise_uc", [(False, False), (False, True), (True, False), (True, True)])
def test_v_update_reproduces_the_eps_update_in_float64(tweedie_uc, renoise_uc, inversion):
    """v = (eps - s*z)/a fed to the v update gives the eps update of the DDIM family (oracle/sampler.py ddim_step's formula; the
    function itself casts to fp32, so its formula is restated in float64 in vpred_ref.ddim_eps_f64 and the function is checked
    against the v update at fp32 accuracy below), forward and with the two alpha levels swapped (inversion)"""
    from cfgpp_amd.schedule import SchedulerTables
    from oracle import sampler as O
    tb = SchedulerTables(50)
    for k, t in enumerate([981, 501, 21]):
        at, ap = float(tb.alpha(t)), float(tb.alpha(t - 20))
        a_tw, a_rn = (ap, at) if inversion else (at, ap)
        z, e_uc, e_c = (_rand((2, 4, 8, 8), 10 * k + j, dtype=D) for j in range(3))
        for lam in (0.6, 7.5):
            want = R.ddim_eps_f64(z, e_uc, e_c, lam, a_tw, a_rn, tweedie_uc, renoise_uc)
            got = R.ddim_v_f64(z, R.v_from_eps(e_uc, z, a_tw), R.v_from_eps(e_c, z, a_tw), lam, a_tw, a_rn, tweedie_uc, renoise_uc)
            for w, g in zip(want, got):
                assert float((w - g).abs().max()) < 1e-10 * max(1.0, float(w.abs().max()))
            o = O.ddim_step(z.float(), e_uc.float(), e_c.float(), lam, a_tw, a_rn, tweedie_uc, renoise_uc)
            for w, g in zip(o, got):
                assert float((w.double() - g).abs().max()) < 2e-5 * max(1.0, float(g.abs().max()))


# ------------------------------------------------------------------------------------------------ roundings: three statements agree
@pytest.mark.parametrize("z_half", [False, True])
@pytest.mark.parametrize("tweedie_uc,renoise_uc", [(False, False), (False, True), (True, False), (True, True)])
def test_natural_expression_explicit_roundings_and_kernel_interface_agree(tweedie_uc, renoise_uc, z_half):
    """torch-CPU evaluating the update as a user writes it == the update with every rounding spelled out ("cpu" semantics) == the
    emulation of the kernel's interface fed ``coeffs.ddim_v_coeffs_pinned(..., "cpu")``; the "cuda" coefficients differ from the
    "cpu" ones exactly where a scalar multiplies an fp16 tensor"""
    from cfgpp_amd.coeffs import ddim_v_coeffs_pinned
    from cfgpp_amd.schedule import SchedulerTables
    tb = SchedulerTables(50)
    for k, t in enumerate([981, 501, 21]):
        s4 = tb.ddim_sqrt_coeffs(t)
        z = _rand((2, 4, 12, 12), 3 + k, 1.3, H if z_half else F)
        v_uc, v_c = _rand(z.shape, 20 + k, dtype=H), _rand(z.shape, 40 + k, dtype=H)
        rs = torch.tensor([0.83, 1.07])
        for lam in (0.0, 0.6, 1.0, 7.5):
            for row_scale in (None, rs):
                a = R.ddim_v_natural(z, v_uc, v_c, lam, s4, tweedie_uc, renoise_uc, row_scale)
                b = R.ddim_v_step(z, v_uc, v_c, lam, s4, tweedie_uc, renoise_uc, "cpu", row_scale)
                zz, z0 = z.clone(), torch.empty_like(z)
                emulate_step_ddim_v(zz, z0, v_uc, v_c, lam, ddim_v_coeffs_pinned(s4, "cpu", z_half), tweedie_uc, renoise_uc, row_scale)
                assert a[0].dtype == z.dtype and a[1].dtype == z.dtype
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
                assert torch.equal(z0, b[0]) and torch.equal(zz, b[1])
        cpu, cuda = ddim_v_coeffs_pinned(s4, "cpu", z_half), ddim_v_coeffs_pinned(s4, "cuda", z_half)
        as_h = lambda v: float(torch.tensor(v, dtype=F).to(H))  # noqa: E731
        for i, (p, q) in enumerate(zip(cpu, cuda)):
            assert q == (s4[1], s4[0], s4[1], s4[0], s4[2], s4[3])[i]
            assert p == (as_h(q) if (z_half or i in (1, 2)) else q)


def test_v_to_eps_three_statements_agree():
    from cfgpp_amd.coeffs import v_to_eps_coeffs
    for k, sigma in enumerate([14.6146, 1.7, 0.03]):
        x, v_uc, v_c = _rand((2, 4, 12, 12), k, 1.1, H), _rand((2, 4, 12, 12), 7 + k, dtype=H), _rand((2, 4, 12, 12), 9 + k, dtype=H)
        a, s = R.v_to_eps_scalars(sigma)
        e_uc, e_c = v_uc.clone(), v_c.clone()
        emulate_v_to_eps(e_uc, e_c, e_uc, e_c, x, *v_to_eps_coeffs(sigma, "cpu"))         # in place
        for v, e in ((v_uc, e_uc), (v_c, e_c)):
            assert torch.equal(R.v_to_eps_natural(v, x, a, s), e) and torch.equal(R.v_to_eps_step(v, x, a, s, "cpu"), e)
        # eps = a*v + s*x inverts v = a*eps - s*x0 at x = a*x0 + s*eps  (float64, a^2 + s^2 = 1)
        ad, sd = float(a), float(s)
        x0, eps = _rand((64,), 100 + k, dtype=D), _rand((64,), 200 + k, dtype=D)
        assert float(((ad * (ad * eps - sd * x0) + sd * (ad * x0 + sd * eps)) - eps).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------ schedules
def test_zero_terminal_snr_table():
    from cfgpp_amd.schedule import SchedulerTables, alphas_cumprod, zero_terminal_snr_tables
    abar = alphas_cumprod()
    az, sq_a, sq_1ma = zero_terminal_snr_tables()
    assert az.dtype == F and az.shape == (1000,) and float(az[999]) == 0.0
    ulp0 = float(np.spacing(np.float32(abar[0])))
    assert abs(float(az[0]) - float(abar[0])) <= ulp0
    assert bool((az[1:] < az[:-1]).all())
    # diffusers' rescale_zero_terminal_snr step by step in float64 (betas -> alphas -> cumprod -> sqrt -> shift, scale -> square ->
    # ratios -> betas), then the scheduler's own cumprod(1 - betas); the betas are those of the pinned table
    p = abar.numpy().astype(np.float64)
    betas = 1.0 - np.concatenate([p[:1], p[1:] / p[:-1]])
    alphas = 1.0 - betas
    bar_sqrt = np.sqrt(np.cumprod(alphas))
    s0, sT = bar_sqrt[0].copy(), bar_sqrt[-1].copy()
    bar_sqrt = (bar_sqrt - sT) * (s0 / (s0 - sT))
    bar = bar_sqrt ** 2
    alphas = np.concatenate([bar[:1], bar[1:] / bar[:-1]])
    ref = np.cumprod(1.0 - (1.0 - alphas))
    rel = np.abs(az.numpy().astype(np.float64)[:999] - ref[:999]) / ref[:999]
    assert rel.max() <= 2.0 ** -22, rel.max()
    # sqrt tables: float64, one rounding
    r = np.sqrt(p)
    a64 = ((r - r[-1]) * r[0] / (r[0] - r[-1])) ** 2            # the closed form, float64
    a64[-1] = 0.0
    assert float(sq_a[999]) == 0.0 and float(sq_1ma[999]) == 1.0
    assert np.array_equal(az.numpy(), a64.astype(np.float32))
    assert np.array_equal(sq_a.numpy(), np.sqrt(a64).astype(np.float32)) and np.array_equal(sq_1ma.numpy(), np.sqrt(1 - a64).astype(np.float32))
    # the defaults are today's object
    t0, t1 = SchedulerTables(20), SchedulerTables(20, "ddim", zero_terminal_snr=False, timestep_spacing="leading")
    assert torch.equal(t0.timesteps, t1.timesteps) and torch.equal(t0.alphas_cumprod, t1.alphas_cumprod)
    assert torch.equal(t0.total_alphas, abar) and t0.ddim_sqrt_coeffs(951) == t1.ddim_sqrt_coeffs(951)
    assert t0.timesteps.tolist()[:3] == [951, 901, 851]


@pytest.mark.parametrize("N", [1, 4, 20, 50, 30])
def test_trailing_timesteps(N):
    from cfgpp_amd.schedule import SchedulerTables, ddim_sqrt_tables
    for zts in (False, True):
        tb = SchedulerTables(N, timestep_spacing="trailing", zero_terminal_snr=zts)
        want = [int(round(1000 - i * 1000 / N)) - 1 for i in range(N)]
        assert tb.timesteps.dtype == torch.int64 and tb.timesteps.tolist() == want and want[0] == 999
        abar = tb.total_alphas
        sq_a, sq_1ma = ddim_sqrt_tables()
        for t in want:
            c1, c2, c3, c4 = tb.ddim_sqrt_coeffs(t, wrap=True)        # wrap plays no part
            tp = t - 1000 // N
            ap = float(abar[tp]) if tp >= 0 else float(abar[0])
            assert abs(c2 * c2 - float(abar[t])) < 3e-7 and abs(c1 * c1 - (1 - float(abar[t]))) < 3e-7
            assert abs(c3 * c3 - ap) < 3e-7 and abs(c4 * c4 - (1 - ap)) < 3e-7
            if not zts:        # the pinned sqrt tables, entry t + 1 of the shifted layout
                assert c2 == float(sq_a[t + 1]) and c1 == float(sq_1ma[t + 1])
            i1, i2, i3, i4 = tb.ddim_sqrt_coeffs(t, inversion=True)
            assert (i1, i2, i3, i4) == (c4, c3, c2, c1)
        last = tb.ddim_sqrt_coeffs(want[-1])
        if want[-1] - 1000 // N < 0:
            assert last[2] == float(tb._sqrt_a[1]) and abs(last[2] ** 2 - float(abar[0])) < 3e-7      # alpha_prev = abar[0]
        if zts:
            assert tb.ddim_sqrt_coeffs(999)[:2] == (1.0, 0.0)


def test_trailing_last_step_renoises_to_abar0():
    """alpha_prev of the last step is abar[0] for every N of the issue (t_last - 1000//N < 0)"""
    from cfgpp_amd.schedule import SchedulerTables
    for N in (1, 4, 20, 50, 30):
        tb = SchedulerTables(N, timestep_spacing="trailing")
        t_last = int(tb.timesteps[-1])
        assert t_last - 1000 // N < 0
        assert tb.ddim_sqrt_coeffs(t_last)[2] == float(tb._sqrt_a[1])
        assert abs(tb.ddim_sqrt_coeffs(t_last)[2] ** 2 - float(tb.total_alphas[0])) < 3e-7


def test_schedule_refusals():
    from cfgpp_amd.schedule import SchedulerTables
    with pytest.raises(ValueError, match="zero_terminal_snr.*trailing"):
        SchedulerTables(10, zero_terminal_snr=True)
    with pytest.raises(ValueError, match="timestep_spacing"):
        SchedulerTables(10, timestep_spacing="linspace")


# ------------------------------------------------------------------------------------------------ solver loops on the mock engine
def _unet(z, t, ehs, te, ti):
    return (0.3 * z.float() * math.cos(0.004 * t) + 0.05 * ehs.float().mean(dim=(1, 2)).view(-1, 1, 1, 1) + 0.02 * math.sin(0.01 * t)).half()


def _solver(name, model="sd15", nfe=4, **kw):
    from cfgpp_amd.unet_config import TINY_SD2, TINY_XL
    if model == "sd15":
        from cfgpp_amd.latent_diffusion import get_solver
        cfg = TINY_SD2
    else:
        from cfgpp_amd.latent_sdxl import get_solver
        cfg = TINY_XL
    eng = VPredMockEngine(_unet, (8, 8))
    s = get_solver(name, solver_config=types.SimpleNamespace(num_sampling=nfe), device="cpu", unet_config=cfg, max_batch=2,
                   latent_hw=(8, 8), engine=eng, vae=StubVAE(cfg.vae_scale), **kw)
    return s, eng, cfg


def _pair_fn(uc, c):
    ehs = torch.cat([uc, c], 0)
    B = uc.shape[0]

    def fn(z, t):
        e = _unet(torch.cat([z, z], 0), float(t), ehs, None, None)
        return e[:B].contiguous(), e[B:].contiguous()
    return fn


def _embeds(cfg, B=2, seed=5):
    return _rand((B, 77, cfg.cross_attention_dim), seed, dtype=H), _rand((B, 77, cfg.cross_attention_dim), seed + 1, dtype=H)


@pytest.mark.parametrize("name,lam", [("ddim", 7.5), ("ddim_cfg++", 0.6)])
def test_sd_ddim_v_loop_is_the_restatement(name, lam):
    s, eng, cfg = _solver(name, prediction_type="v_prediction")
    uc, c = _embeds(cfg)
    zT = _rand((2, 4, 8, 8), 1)
    z0t, zt = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, return_latents=True)
    w0, w1 = R.sample_ddim_v(_pair_fn(uc, c), zT, s.tables, lam, cfgpp=name.endswith("++"))
    assert torch.equal(z0t, w0) and torch.equal(zt, w1) and z0t.dtype == F
    assert [v[0] for v in eng.vcalls] == ["step_ddim_v"] * 4
    # and it is not the epsilon loop
    e = _solver(name)[0].sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, return_latents=True)
    assert not torch.equal(e[0], z0t)


def test_sd_inversion_v_loop_is_the_restatement():
    s, eng, cfg = _solver("ddim_inversion_cfg++", prediction_type="v_prediction")
    uc, c = _embeds(cfg)
    z0 = _rand((2, 4, 8, 8), 2, dtype=H)
    z0t, zt = s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), src_latent=z0, return_latents=True)
    fn = _pair_fn(uc, c)
    zT = R.sample_ddim_v(fn, z0, s.tables, 0.6, cfgpp=True, inversion=True)[1]
    w0, w1 = R.sample_ddim_v(fn, zT, s.tables, 0.6, cfgpp=True)
    assert z0t.dtype == H and torch.equal(z0t, w0) and torch.equal(zt, w1)
    assert len(eng.vcalls) == 8


def test_sdxl_ddim_cfgpp_v_loop_is_the_restatement():
    s, eng, cfg = _solver("ddim_cfg++", model="sdxl", prediction_type="v_prediction")
    uc, c = _embeds(cfg)
    pool = _rand((2, cfg.addition_pooled_dim), 9, dtype=H)
    zT = _rand((2, 4, 8, 8), 3)
    z = s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c, pool, pool), latents=zT, target_size=(64, 64), original_size=(64, 64),
                 return_latents=True)
    w0, _ = R.sample_ddim_v(_pair_fn(uc, c), zT, s.tables, 0.6, cfgpp=True, wrap=True)
    assert torch.equal(z, w0)


def test_sd_dpmpp_2m_cfgpp_v_loop_is_the_restatement():
    from oracle import sampler as O
    s, eng, cfg = _solver("dpm++_2m_cfg++", nfe=6, prediction_type="v_prediction")
    uc, c = _embeds(cfg)
    den, x = s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), seeds=[3, 4], return_latents=True)
    fn = _pair_fn(uc, c)
    sigmas = s.tables.karras_sigmas()
    xr = s._kdiff_start((2, 4, 8, 8), sigmas, [3, 4])
    old = None
    for i in range(6):
        sigma = sigmas[i]
        xc = O.kdiff_input_div(xr, sigma)
        v_uc, v_c = fn(xc, s.tables.timestep(sigma))
        a, sg = R.v_to_eps_scalars(sigma)
        e_uc, e_c = R.v_to_eps_step(v_uc, xc, a, sg), R.v_to_eps_step(v_c, xc, a, sg)
        d, ud = O.kdiff_denoised(xr, e_uc, e_c, 0.6, sigma)
        xr, old = O.dpm2m_step(xr, d, ud, old, sigmas, i, "cfgpp_sd")
    assert x.dtype == H and torch.equal(x, xr) and torch.equal(den, d)
    assert [v[0] for v in eng.vcalls] == ["v_to_eps"] * 6


def test_zero_terminal_snr_trailing_first_step_has_alpha_zero():
    s, eng, cfg = _solver("ddim", prediction_type="v_prediction", zero_terminal_snr=True, timestep_spacing="trailing", guidance_rescale=0.7)
    uc, c = _embeds(cfg)
    zT = _rand((2, 4, 8, 8), 4)
    z0t, zt = s.sample(cfg_guidance=7.5, prompt_embeds=(uc, c), latents=zT, return_latents=True)
    assert [c_["t"] for c_ in eng.calls] == [999.0, 749.0, 499.0, 249.0]
    steps = [v for v in eng.vcalls if v[0] == "step_ddim_v"]
    assert steps[0][1][:4] == (0.0, 1.0, 0.0, 1.0) and all(v[2] for v in steps)        # a = 0, s = 1; every step rescaled
    assert [v[0] for v in eng.vcalls] == ["cfg_rescale", "step_ddim_v"] * 4
    assert bool(torch.isfinite(z0t).all()) and bool(torch.isfinite(zt).all())
    w0, w1 = R.sample_ddim_v(_pair_fn(uc, c), zT, s.tables, 7.5, cfgpp=False, phi=0.7)
    assert torch.equal(z0t, w0) and torch.equal(zt, w1)
    # sample(guidance_rescale=) overrides the solver's value for one job
    n = len(eng.vcalls)
    s.sample(cfg_guidance=7.5, prompt_embeds=(uc, c), latents=zT, return_latents=True, guidance_rescale=0.0)
    assert [v[0] for v in eng.vcalls[n:]] == ["step_ddim_v"] * 4
    s.sample(cfg_guidance=7.5, prompt_embeds=(uc, c), latents=zT, return_latents=True)
    assert [v[0] for v in eng.vcalls[n + 4:]] == ["cfg_rescale", "step_ddim_v"] * 4


def test_graph_replay_is_not_used_with_v_prediction():
    s, eng, cfg = _solver("ddim_cfg++", prediction_type="v_prediction")
    eng.graph_enabled = True
    eng.ddim_loop_graph = lambda *a, **k: pytest.fail("graph replay with v-prediction")
    uc, c = _embeds(cfg)
    s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), latents=_rand((2, 4, 8, 8), 1), return_latents=True)
    assert len(eng.vcalls) == 4


# ------------------------------------------------------------------------------------------------ refusals
V = dict(prediction_type="v_prediction")
REFUSALS = [
    ("sdxl", "ddim_lightning", V, "lightning"), ("sdxl", "euler_lightning", V, "lightning"),
    ("sdxl", "ddim_cfg++_lightning", V, "lightning"), ("sdxl", "dpm++_2m_cfgpp_lightning", V, "lightning"),
    ("sd15", "euler", dict(V, zero_terminal_snr=True, timestep_spacing="trailing"), "zero_terminal_snr"),
    ("sd15", "dpm++_2m_cfg++", dict(V, zero_terminal_snr=True, timestep_spacing="trailing"), "zero_terminal_snr"),
    ("sd15", "dpm++_2s_a", dict(V, zero_terminal_snr=True, timestep_spacing="trailing"), "zero_terminal_snr"),
    ("sdxl", "euler_cfg++", dict(V, zero_terminal_snr=True, timestep_spacing="trailing"), "zero_terminal_snr"),
    ("sdxl", "dpm++_2m_cfgpp", dict(V, zero_terminal_snr=True, timestep_spacing="trailing"), "zero_terminal_snr"),
    ("sd15", "ddim", dict(V, zero_terminal_snr=True), "zero_terminal_snr"),                    # leading: the zero is never reached
    ("sd15", "ddim", dict(zero_terminal_snr=True, timestep_spacing="trailing"), "zero_terminal_snr"),     # epsilon divides by zero
    ("sd15", "ddim_cfg++", dict(guidance_rescale=0.7), "guidance_rescale"),                    # epsilon model
    ("sdxl", "ddim_cfg++", dict(guidance_rescale=0.7), "guidance_rescale"),
    ("sd15", "ddim_inversion_cfg++", dict(V, guidance_rescale=0.7), "guidance_rescale"),
    ("sd15", "ddim_edit", dict(V, guidance_rescale=0.7), "guidance_rescale"),
    ("sdxl", "ddim_edit_cfg++", dict(V, guidance_rescale=0.7), "guidance_rescale"),
    ("sd15", "euler_cfg++", dict(V, guidance_rescale=0.7), "guidance_rescale"),
    ("sd15", "dpm++_2m", dict(V, guidance_rescale=0.7), "guidance_rescale"),
    ("sd15", "euler_a", dict(V, guidance_rescale=0.7), "guidance_rescale"),
    ("sd15", "ddim", dict(prediction_type="sample"), "prediction_type"),
]


@pytest.mark.parametrize("model,name,kw,word", REFUSALS)
def test_refusals_name_what_they_refuse(model, name, kw, word):
    with pytest.raises(ValueError) as e:
        _solver(name, model=model, **kw)
    assert word in str(e.value)
    if word != "prediction_type" and not (word == "zero_terminal_snr" and name == "ddim" and "timestep_spacing" not in kw):
        assert name in str(e.value)


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
@pytest.mark.parametrize("name", ["ddim_inpaint", "ddim_inpaint_cfg++"])
def test_inpaint_solvers_refuse_v_prediction(model, name):
    from cfgpp_amd.inpaint import get_inpaint_solver
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    cfg = TINY_SD if model == "sd15" else TINY_XL
    with pytest.raises(ValueError, match="v_prediction.*inpaint") as e:
        get_inpaint_solver(name, model, solver_config=types.SimpleNamespace(num_sampling=4), device="cpu", unet_config=cfg,
                           latent_hw=(8, 8), engine=VPredMockEngine(_unet, (8, 8)), vae=StubVAE(cfg.vae_scale), **V)
    assert name in str(e.value)


def test_per_job_guidance_rescale_is_refused_where_the_solver_refuses_it():
    s, eng, cfg = _solver("ddim_inversion_cfg++", prediction_type="v_prediction")
    uc, c = _embeds(cfg)
    with pytest.raises(ValueError, match="guidance_rescale"):
        s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), src_latent=_rand((2, 4, 8, 8), 2, dtype=H), guidance_rescale=0.5)
    s, eng, cfg = _solver("ddim_cfg++")
    with pytest.raises(ValueError, match="guidance_rescale"):
        s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), guidance_rescale=0.5)


# ------------------------------------------------------------------------------------------------ configs and checkpoint directories
def test_sd2_configs():
    from cfgpp_amd.unet_config import CONFIGS, SD15, SD21, SD21_BASE, SDXL, TINY_SD2, param_count, param_shapes
    assert param_count(SD21_BASE) == 865_910_724 == param_count(SD21)
    assert param_count(SD15) == 859_520_964                      # unchanged by the new field
    assert SD21.num_heads == (5, 10, 20, 20) and SD21.cross_attention_dim == 1024 and (SD21.sample_size, SD21_BASE.sample_size) == (96, 64)
    assert all(c // h == 64 for c, h in zip(SD21.block_out_channels, SD21.num_heads))
    assert all(c // h == 64 for c, h in zip(TINY_SD2.block_out_channels, TINY_SD2.num_heads)) and TINY_SD2.sample_size == 12
    P = param_shapes(SD21_BASE)
    assert P["down_blocks.0.attentions.0.proj_in.weight"] == (320, 320) and P["mid_block.attentions.0.proj_out.weight"] == (1280, 1280)
    assert P["down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k.weight"] == (320, 1024)
    assert param_shapes(SD15)["down_blocks.0.attentions.0.proj_in.weight"] == (320, 320, 1, 1)
    assert SD15.linear_projection is None and not SD15.use_linear_projection and SDXL.use_linear_projection
    assert CONFIGS["sd21"] is SD21 and CONFIGS["tiny_sd2"] is TINY_SD2


def _write(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f)


def _model_dir(tmp, unet, sched, pad):
    _write(os.path.join(tmp, "unet", "config.json"), unet)
    _write(os.path.join(tmp, "scheduler", "scheduler_config.json"), sched)
    _write(os.path.join(tmp, "tokenizer", "special_tokens_map.json"), {"bos_token": "<|startoftext|>", "eos_token": "<|endoftext|>", "pad_token": pad})
    return str(tmp)


SD15_UNET = dict(in_channels=4, attention_head_dim=8, cross_attention_dim=768, use_linear_projection=False, sample_size=64,
                 block_out_channels=[320, 640, 1280, 1280])
SD21_UNET = dict(in_channels=4, attention_head_dim=[5, 10, 20, 20], cross_attention_dim=1024, use_linear_projection=True, sample_size=96,
                 block_out_channels=[320, 640, 1280, 1280])


def test_checkpoint_dir_sd21(tmp_path):
    from cfgpp_amd.checkpoint import solver_kwargs_from_dir
    from cfgpp_amd.unet_config import SD21, SD21_BASE
    d = _model_dir(tmp_path / "v", SD21_UNET, dict(prediction_type="v_prediction", timestep_spacing="leading", steps_offset=1),
                   {"content": "!", "lstrip": False})
    kw, missing = solver_kwargs_from_dir(d, sdxl=False, device="cpu")
    assert kw == dict(unet_config=SD21, prediction_type="v_prediction", pad_token="!") and "unet" in missing
    d = _model_dir(tmp_path / "base", dict(SD21_UNET, sample_size=64), dict(prediction_type="epsilon"), "!")
    kw, _ = solver_kwargs_from_dir(d, sdxl=False, device="cpu")
    assert kw == dict(unet_config=SD21_BASE, pad_token="!")
    d = _model_dir(tmp_path / "z", SD15_UNET, dict(prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing"),
                   "<|endoftext|>")
    kw, _ = solver_kwargs_from_dir(d, sdxl=False, device="cpu")
    assert kw == dict(prediction_type="v_prediction", zero_terminal_snr=True, timestep_spacing="trailing")
    # the kwargs build a solver
    from cfgpp_amd.latent_diffusion import get_solver
    s = get_solver("ddim", solver_config=types.SimpleNamespace(num_sampling=4), device="cpu", engine=VPredMockEngine(_unet, (8, 8)), **kw)
    assert s.prediction_type == "v_prediction" and s.tables.zero_terminal_snr and int(s.tables.timesteps[0]) == 999


def test_checkpoint_dir_sd15_and_sdxl_yield_todays_kwargs(tmp_path):
    from cfgpp_amd.checkpoint import solver_kwargs_from_dir
    sched = dict(prediction_type="epsilon", timestep_spacing="leading", steps_offset=1, set_alpha_to_one=False)
    d = _model_dir(tmp_path / "sd15", SD15_UNET, sched, "<|endoftext|>")
    kw, missing = solver_kwargs_from_dir(d, sdxl=False, device="cpu")
    assert kw == {} and missing == ["unet", "vae", "text_encoder"]
    xl = dict(in_channels=4, attention_head_dim=[5, 10, 20], cross_attention_dim=2048, use_linear_projection=True, sample_size=128,
              block_out_channels=[320, 640, 1280])
    d = _model_dir(tmp_path / "xl", xl, sched, "<|endoftext|>")
    kw, _ = solver_kwargs_from_dir(d, sdxl=True, device="cpu")
    assert kw == {}
    d = _model_dir(tmp_path / "inp", dict(SD15_UNET, in_channels=9), sched, "<|endoftext|>")
    from cfgpp_amd.unet_config import SD15_INPAINT
    assert solver_kwargs_from_dir(d, sdxl=False, device="cpu")[0] == dict(unet_config=SD15_INPAINT)


def test_cli_flags_win_over_the_checkpoint_files(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import inpaint as inpaint_cli
    import inversion as inversion_cli
    import text_to_img
    import text_to_mscoco
    for mod in (text_to_img, text_to_mscoco, inversion_cli, inpaint_cli):
        src = open(mod.__file__).read()
        assert "vpred.add_cli_flags(ap)" in src and "vpred.cli_kwargs(args, kw)" in src, mod.__name__
    d = _model_dir(tmp_path / "m", SD15_UNET, dict(prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing"),
                   "<|endoftext|>")
    base = ["--method", "ddim", "--cfg_guidance", "5.0", "--NFE", "2", "--prompt", "a cat", "--device", "cpu", "--workdir", str(tmp_path),
            "--model_dir", d]
    eng = VPredMockEngine(_unet, (8, 8))
    text_to_img.main(base + ["--guidance_rescale", "0.7"], solver_kwargs=dict(engine=eng, vae=StubVAE(0.18215), latent_hw=(8, 8)))
    assert [c["t"] for c in eng.calls] == [999.0, 499.0] and [v[0] for v in eng.vcalls] == ["cfg_rescale", "step_ddim_v"] * 2
    eng = VPredMockEngine(_unet, (8, 8))          # the flags undo what the files say: the reference's epsilon model
    text_to_img.main(base + ["--prediction_type", "epsilon", "--zero_terminal_snr", "0", "--timestep_spacing", "leading"],
                     solver_kwargs=dict(engine=eng, vae=StubVAE(0.18215), latent_hw=(8, 8)))
    assert [c["t"] for c in eng.calls] == [501.0, 1.0] and eng.vcalls == []


# ------------------------------------------------------------------------------------------------ guidance rescale: the model
RESCALE_SHAPES = [(1, 4), (3, 144), (2, 1024), (8, 16384), (2, 65536)]


@pytest.mark.parametrize("B,n", RESCALE_SHAPES)
def test_rescale_two_pass_fp32_model_meets_the_bound(B, n):
    v_uc, v_c = _rand((B, n), n, dtype=H), _rand((B, n), n + 1, 1.3, H)
    for lam, phi in ((7.5, 0.7), (0.6, 1.0)):
        want = R.rescale_f64(v_uc, v_c, lam, phi)
        got = R.rescale_f32_two_pass(v_uc, v_c, lam, phi)
        assert float(((got - want).abs() / want).max()) <= R.rescale_bound(n)
    const = torch.full((B, n), 0.3, dtype=H)
    assert R.rescale_f64(const, const, 7.5, 0.7).tolist() == [1.0] * B == R.rescale_f32_two_pass(const, const, 7.5, 0.7).tolist()


def test_rescale_cancellation_case_has_teeth():
    """8 + 0.01*randn in fp16: the two-pass fp32 model holds the bound, E[x^2] - E[x]^2 in fp32 misses it more than tenfold"""
    for B, n in ((2, 1024), (8, 16384)):
        v_uc, v_c = R.cancellation_case(B, n, seed=n)
        want = R.rescale_f64(v_uc, v_c, 7.5, 0.7)
        two = float(((R.rescale_f32_two_pass(v_uc, v_c, 7.5, 0.7) - want).abs() / want).max())
        naive = float(((R.rescale_f32_naive(v_uc, v_c, 7.5, 0.7) - want).abs() / want).max())
        assert two <= R.rescale_bound(n) and naive > 10 * R.rescale_bound(n), (two, naive)


# ------------------------------------------------------------------------------------------------ the header and the binding
def test_vpred_header_matches_the_binding():
    from cfgpp_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "cfgpp_vpred.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cfgpp_\w+)\s*\(", hdr))
    assert declared == {"cfgpp_step_ddim_v", "cfgpp_v_to_eps", "cfgpp_cfg_rescale"} == set(_lib.VPRED_PROTOTYPES)
    from cfgpp_amd.build import SOURCES
    assert ("vpred_kernels.hip", ["-ffp-contract=off"]) in SOURCES
    from cfgpp_amd.hip_engine import HipEngine
    assert all(hasattr(HipEngine, m) for m in ("step_ddim_v", "v_to_eps", "cfg_rescale"))
