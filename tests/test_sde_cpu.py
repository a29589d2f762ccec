"""CPU: DPM++ 2M / 3M SDE sampling - the expanded coefficients (cfgpp_amd/sde.py: sde_coeffs) against k-diffusion's two algorithms
written literally in float64 (tests/sde_ref.py), identities that hold exactly, eta = 0 against the update of the existing `dpm++_2m`
solvers, the exponential schedule, the solvers' plumbing on a mock engine (tests/sde_mock.py), the refusals, the CLI route, the
library's SDE header, and fault injection: each deliberate error switched into the model has to break the assertion that guards it."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import sde_ref as S
from mock_engine import StubVAE
from sde_mock import SDEMockEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, F, D = torch.float16, torch.float32, torch.float64
NAMES = ["dpm++_2m_sde", "dpm++_2m_sde_cfg++", "dpm++_3m_sde", "dpm++_3m_sde_cfg++"]


def _rand(shape, seed, scale=1.0, dtype=F):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=D) * scale).to(dtype)


def _schedule(name, n=6):
    """the product's fp32 sigma table"""
    from cfgpp_amd.schedule import SchedulerTables
    tb = SchedulerTables(n)
    return tb.karras_sigmas() if name == "karras" else tb.exponential_sigmas()


# ------------------------------------------------------------------------------------------------ coefficients
KINDS = [("2m", "midpoint"), ("2m", "heun"), ("3m", "midpoint")]


@pytest.mark.parametrize("schedule", ["karras", "exponential"])
@pytest.mark.parametrize("cfgpp", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("kind,solver_type", KINDS)
def test_expanded_coefficients_equal_the_literal_algorithm(kind, solver_type, eta, cfgpp, schedule):
    from cfgpp_amd.sde import sde_coeffs, sde_coeffs64
    sig = [float(v) for v in _schedule(schedule)]
    n = len(sig) - 1
    rng = np.random.default_rng(7)
    dens, udens, noises = rng.standard_normal((n, 16)), rng.standard_normal((n, 16)), rng.standard_normal((n, 16))
    x0 = rng.standard_normal(16) * sig[0]
    denoise = lambda x, i: (dens[i], udens[i])  # noqa: E731
    s_noise = 0.9
    want = S.literal_chain(kind, denoise, x0, sig, noises, eta, s_noise, solver_type, cfgpp)
    coef = lambda i, nh: sde_coeffs64(sig, i, kind, solver_type, eta, s_noise, cfgpp, nh)  # noqa: E731
    got = S.coefficient_chain(coef, kind, denoise, x0, sig, noises, cfgpp)
    scale = max(float(np.abs(w).max()) for w in want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert float(np.abs(g - w).max()) <= 1e-12 * scale, (i, float(np.abs(g - w).max()))
    assert np.array_equal(got[-1], dens[-1])                        # sigma_next = 0: x <- D
    depth = 1 if kind == "2m" else 2
    for i in range(n):
        nh = min(i, depth)
        c64, c32 = sde_coeffs64(sig, i, kind, solver_type, eta, s_noise, cfgpp, nh), sde_coeffs(sig, i, kind, solver_type, eta, s_noise, cfgpp, nh)
        assert c32 == tuple(float(np.float32(v)) for v in c64)      # each rounded once to fp32
        assert (c32[6] == 0.0) == (eta == 0.0 or i == n - 1)
        if not cfgpp:
            assert c32[3] == 0.0


@pytest.mark.parametrize("schedule", ["karras", "exponential"])
@pytest.mark.parametrize("kind,solver_type", KINDS)
def test_identities(kind, solver_type, schedule):
    from cfgpp_amd.sde import sde_coeffs64
    sig = [float(v) for v in _schedule(schedule)]
    depth = 1 if kind == "2m" else 2
    for eta in (0.0, 0.5, 1.0):
        for s_noise in (1.0, 0.7):
            for i in range(len(sig) - 2):
                for nh in range(min(i, depth) + 1):
                    sg, a_x, a_0, _, a_1, a_2, a_n, s_in = sde_coeffs64(sig, i, kind, solver_type, eta, s_noise, False, nh)
                    assert sg == sig[i] and abs(s_in - 1 / math.sqrt(sig[i + 1] ** 2 + 1)) <= 1e-15
                    assert abs(a_x + a_0 + a_1 + a_2 - 1.0) <= 1e-12                        # a constant D is a fixed point's weight
                    h = math.log(sig[i]) - math.log(sig[i + 1])
                    e = math.exp(-2 * eta * h)
                    want = s_noise ** 2 * sig[i + 1] ** 2 * (1 - e) + e * sig[i + 1] ** 2
                    assert abs(a_x ** 2 * sig[i] ** 2 + a_n ** 2 - want) <= 1e-12 * max(1.0, want)     # the point-mass case: exact
                    if s_noise == 1.0:
                        assert abs(a_x ** 2 * sig[i] ** 2 + a_n ** 2 - sig[i + 1] ** 2) <= 1e-12 * max(1.0, sig[i + 1] ** 2)
                    # CFG++: a_d = a_0 + a_x, a_u = -a_x, the rest unchanged
                    pp = sde_coeffs64(sig, i, kind, solver_type, eta, s_noise, True, nh)
                    assert pp[2] == a_0 + a_x and pp[3] == -a_x and (pp[0], pp[1]) + pp[4:] == (sg, a_x, a_1, a_2, a_n, s_in)


@pytest.mark.parametrize("cfgpp", [False, True])
def test_eta_zero_midpoint_is_the_dpmpp_2m_update(cfgpp):
    """`dpm++_2m_sde(_cfg++)` at eta = 0 against a float64 evaluation of the update that K.kdiff_coeffs plus variant 0 / 1 of
    kdiff_step_kernel define:  x' = den + (d_from * neg_exp - (den - old) * expm1 * inv_2r) + x * exp_mh,  d_from / old = den (variant
    0) or uden (variant 1).
    Tolerance.  kdiff_coeffs evaluates t = -log sigma, h, r and the exponentials in fp32 torch arithmetic: h = t_next - t carries an
    absolute error of up to 2 ulp(|t|) <= 2 * 2^-23 * 2.7 on |t| <= 2.7 (sigma in 0.13 .. 14.6) against h >= 0.7, a relative error
    <= 1e-6; r = h_last / h twice that; exp / expm1 of h add |dh| <= 7e-7 relative plus their own rounding.  Every coefficient is
    therefore within 4e-6 relative, and the two updates within 4e-6 * sum |coefficient| * |input|; asserted at 1e-5 of that sum."""
    from cfgpp_amd import coeffs as K
    from cfgpp_amd.sde import sde_coeffs
    sig = _schedule("karras")
    rng = np.random.default_rng(3)
    x, den, uden, old = (rng.standard_normal(64) for _ in range(4))
    for i in range(1, len(sig) - 2):
        co, euler = K.kdiff_coeffs(7.5, sig, i, False, xl_form=False, semantics="cuda")
        assert not euler and co[7] < 0
        neg_exp, expm1, inv_2r, exp_mh = co[5], co[6], -co[7], co[8]
        d_from = uden if cfgpp else den
        want = den + (d_from * neg_exp - (den - old) * expm1 * inv_2r) + x * exp_mh
        _, a_x, a_d, a_u, a_1, _, a_n, _ = sde_coeffs(sig, i, "2m", "midpoint", 0.0, 1.0, cfgpp, 1)
        assert a_n == 0.0
        got = a_x * x + a_d * den + (a_u * uden if cfgpp else 0.0) + a_1 * old
        mass = abs(a_x) * np.abs(x) + abs(a_d) * np.abs(den) + abs(a_u) * np.abs(uden) + abs(a_1) * np.abs(old)
        assert bool((np.abs(got - want) <= 1e-5 * mass).all()), float((np.abs(got - want) / mass).max())
    # the first step (no history) is the Euler / first-order step of both
    co, euler = K.kdiff_coeffs(7.5, sig, 0, True, xl_form=False, semantics="cuda")
    assert euler
    _, a_x, a_d, a_u, a_1, a_2, _, _ = sde_coeffs(sig, 0, "2m", "midpoint", 0.0, 1.0, cfgpp, 0)
    ratio = float(sig[1]) / float(sig[0])                            # x' = den + (x - d_from) / sigma * sigma_next
    assert abs(a_x - ratio) <= 1e-6 and abs(a_d - (1.0 if cfgpp else 1.0 - ratio)) <= 1e-6 and abs(a_u + (ratio if cfgpp else 0.0)) <= 1e-6
    assert a_1 == 0.0 == a_2


def test_exponential_schedule():
    from cfgpp_amd.schedule import SchedulerTables, get_sigmas_exponential
    s = get_sigmas_exponential(10, 0.03, 14.6)
    assert s.dtype == F and len(s) == 11 and float(s[-1]) == 0.0
    assert abs(float(s[0]) - 14.6) <= 1e-5 and abs(float(s[9]) - 0.03) <= 1e-7
    assert bool((s[1:] < s[:-1]).all())
    ratios = (s[1:10] / s[:9]).double()
    assert float((ratios - ratios[0]).abs().max()) <= 1e-5           # geometric
    assert np.abs(s.double().numpy() - S.sigmas_exponential(10, 0.03, 14.6)).max() <= 1e-5
    tb = SchedulerTables(6)
    k, e = tb.karras_sigmas(), tb.exponential_sigmas()
    assert len(e) == len(k) == 7 and float(e[-1]) == 0.0
    assert abs(float(e[0]) - float(k[0])) <= 1e-4 and abs(float(e[5]) - float(tb.sigmas.min())) <= 1e-6
    assert np.abs(k.double().numpy() - S.sigmas_karras(6, float(tb.sigmas.min()), float(tb.sigmas.max()))).max() <= 1e-4


# ------------------------------------------------------------------------------------------------ solver plumbing on the mock engine
def _unet(z, t, ehs, te, ti):
    v = 0.3 * z.float() * math.cos(0.004 * t) + 0.05 * ehs.float().mean(dim=(1, 2)).view(-1, 1, 1, 1) + 0.02 * math.sin(0.01 * t)
    if te is not None:
        v = v + 0.01 * te.float().mean(dim=1).view(-1, 1, 1, 1)
    return v.half()


def _solver(name="dpm++_2m_sde_cfg++", model="sd15", nfe=5, **kw):
    from cfgpp_amd.sde import get_sde_solver
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    cfg = TINY_SD if model == "sd15" else TINY_XL
    eng = SDEMockEngine(_unet, (8, 8))
    s = get_sde_solver(name, model=model, solver_config=types.SimpleNamespace(num_sampling=nfe), device="cpu", unet_config=cfg,
                       max_batch=3, latent_hw=(8, 8), engine=eng, vae=StubVAE(cfg.vae_scale), **kw)
    return s, eng, cfg


def _embeds(cfg, B=2, seed=5):
    return _rand((B, 77, cfg.cross_attention_dim), seed, dtype=H), _rand((B, 77, cfg.cross_attention_dim), seed + 1, dtype=H)


def _model_fn(s, uc, c, sigmas, te=None, v_pred=False):
    """what the solver's UNet call returns at step i, as epsilon: the mock UNet at the product's timestep of sigma_i (and, for a
    v-model, the mock's v -> eps conversion)"""
    B = c.shape[0]
    ehs = torch.cat([uc, c], 0)

    def fn(xc, i):
        e = _unet(torch.cat([xc, xc], 0), float(s.timestep(sigmas[i])), ehs, te, None)
        m_uc, m_c = e[:B].contiguous(), e[B:].contiguous()
        if v_pred:
            from cfgpp_amd import coeffs as K
            from vpred_mock import emulate_v_to_eps
            a, sc = K.v_to_eps_coeffs(sigmas[i], s.scalar_semantics)
            emulate_v_to_eps(m_uc, m_c, m_uc, m_c, xc, a, sc)
        return m_uc, m_c
    return fn


def _check_ring(steps, kind, n):
    """the history ring: n_hist 0, 1, (2, 2, ..) and every step's hist1 / hist2 are the buffers the previous / the one-before-previous
    step wrote; nothing else is ever passed"""
    depth = 1 if kind == "2m" else 2
    assert [st["n_hist"] for st in steps] == [min(i, depth) for i in range(n)]
    for i, st in enumerate(steps):
        assert st["draw"] == i and st["last"] == (i == n - 1)
        assert (st["hist_out"] is None) == (i == n - 1) == (st["xc_out"] is None)       # the last step writes neither
        assert st["hist1"] == (steps[i - 1]["hist_out"] if st["n_hist"] >= 1 else None)
        assert st["hist2"] == (steps[i - 2]["hist_out"] if st["n_hist"] == 2 else None)
        if st["hist_out"] is not None:
            assert st["hist_out"] not in (st["hist1"], st["hist2"], st["x"])
    assert len({st["hist_out"] for st in steps[:-1]}) <= depth + 1                      # a ring of depth + 1 buffers, no allocation per step


CASES = [("dpm++_2m_sde", {}, 7.5, "epsilon"), ("dpm++_2m_sde_cfg++", {}, 0.6, "epsilon"), ("dpm++_2m_sde", dict(solver_type="heun"), 5.0, "epsilon"),
         ("dpm++_3m_sde", {}, 7.5, "epsilon"), ("dpm++_3m_sde_cfg++", dict(sigma_schedule="exponential", eta=0.5, s_noise=0.9), 0.6, "epsilon"),
         ("dpm++_3m_sde_cfg++", dict(eta=0.0), 0.6, "epsilon"), ("dpm++_2m_sde_cfg++", {}, 0.6, "v_prediction")]


@pytest.mark.parametrize("name,opts,lam,pt", CASES)
def test_sd_loop_is_the_model(name, opts, lam, pt):
    from cfgpp_amd.sde import sde_coeffs
    s, eng, ucfg = _solver(name, prediction_type=pt, **opts)
    uc, c = _embeds(ucfg)
    zT = _rand((2, 4, 8, 8), 1)
    seeds = [11, (7 << 40) + 5]
    seen = []
    den, x = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, seeds=seeds, return_latents=True,
                      callback_fn=None)
    kind, cfgpp = ("2m" if "2m" in name else "3m"), name.endswith("++")
    sigmas = s.sde_sigmas()
    n = 5
    coef = lambda i, nh: sde_coeffs(sigmas, i, kind, opts.get("solver_type", "midpoint"), opts.get("eta", 1.0), opts.get("s_noise", 1.0),  # noqa: E731
                                    cfgpp, nh)
    w_den, w_x, rec = S.sde_chain(_model_fn(s, uc, c, sigmas, v_pred=(pt == "v_prediction")), zT, seeds, sigmas, coef, kind, lam, cfgpp)
    assert den.dtype == F and x.dtype == F and torch.equal(den, w_den) and torch.equal(x, w_x)
    assert torch.equal(x, den)                                       # the last step: x <- D, no noise
    # the call sequence is exactly sde_input, step_sde x N; per step one UNet call (and one v_to_eps for a v-model)
    assert [nm for nm, _ in eng.scalls] == ["sde_input"] + ["step_sde"] * n and eng.lcalls == []
    assert [c_["t"] for c_ in eng.calls] == [float(s.timestep(sigmas[i])) for i in range(n)]
    assert all(c_["z_dtype"] == H for c_ in eng.calls)
    assert [v[0] for v in eng.vcalls] == (["v_to_eps"] * n if pt == "v_prediction" else [])
    assert eng.scalls[0][1]["s_in"] == float(np.float32(1.0 / math.sqrt(float(sigmas[0]) ** 2 + 1.0)))
    steps = [v for _, v in eng.scalls[1:]]
    _check_ring(steps, kind, n)
    for st, r in zip(steps, rec):
        assert st["coef"] == r["coef"] and st["seeds"] == seeds and st["lam"] == lam and st["cfgpp"] == cfgpp and not st["single"]
        assert not st["noise_given"]
    assert steps[0]["xc_out"] == eng.scalls[0][1]["xc"]             # one UNet-input buffer for the job
    # callbacks get (denoised, x) at every step and leave the result alone
    d2, _ = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, seeds=seeds, return_latents=True,
                     callback_fn=lambda i, t, kw: (seen.append((i, int(t), kw["z0t"].clone(), kw["zt"].clone())), kw)[1])
    assert torch.equal(d2, den) and [i for i, *_ in seen] == list(range(n)) and torch.equal(seen[-1][2], den)
    assert [t for _, t, *_ in seen] == [int(s.timestep(sigmas[i])) for i in range(n)]
    # decoded result = the decode of the last step's denoised
    img = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, seeds=seeds)
    assert torch.equal(img, (StubVAE(ucfg.vae_scale).decode(den) / 2 + 0.5).clamp(0, 1))
    if opts.get("eta") == 0.0:                                       # deterministic: other seeds for the noise, the same result
        d3, _ = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, seeds=[1, 2], return_latents=True)
        assert torch.equal(d3, den) and all(st["coef"][6] == 0.0 for st in steps)
    else:
        d3, _ = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, seeds=[1, 2], return_latents=True)
        assert not torch.equal(d3, den)


@pytest.mark.parametrize("name,lam", [("dpm++_2m_sde_cfg++", 0.6), ("dpm++_3m_sde", 5.0)])
def test_sdxl_loop_is_the_model(name, lam):
    from cfgpp_amd.sde import sde_coeffs
    s, eng, ucfg = _solver(name, "sdxl")
    uc, c = _embeds(ucfg)
    pool_n, pool = _rand((1, ucfg.addition_pooled_dim), 8, dtype=H), _rand((2, ucfg.addition_pooled_dim), 9, dtype=H)
    zT = _rand((2, 4, 8, 8), 2)
    seeds = [3, 4]
    den, x = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c, pool_n, pool), latents=zT, seeds=seeds, return_latents=True,
                      target_size=(64, 64), original_size=(64, 64))
    te = eng.te
    assert int(te.shape[0]) == 4 and not torch.equal(te[:2], te[2:])                    # SDXL's added conditioning, both halves
    kind, cfgpp = ("2m" if "2m" in name else "3m"), name.endswith("++")
    sigmas = s.sde_sigmas()
    coef = lambda i, nh: sde_coeffs(sigmas, i, kind, "midpoint", 1.0, 1.0, cfgpp, nh)  # noqa: E731
    w_den, w_x, _ = S.sde_chain(_model_fn(s, uc, c, sigmas, te), zT, seeds, sigmas, coef, kind, lam, cfgpp)
    assert torch.equal(den, w_den) and torch.equal(x, w_x)
    assert [nm for nm, _ in eng.scalls] == ["sde_input"] + ["step_sde"] * 5
    _check_ring([v for _, v in eng.scalls[1:]], kind, 5)
    img = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c, pool_n, pool), latents=zT, seeds=seeds, target_size=(64, 64), original_size=(64, 64))
    assert torch.equal(img, (StubVAE(ucfg.vae_scale).decode(den) / 2 + 0.5).clamp(0, 1))


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_batched_chains_equal_independent_runs_and_seeds_none(model):
    s, eng, ucfg = _solver("dpm++_3m_sde_cfg++", model)
    uc, c = _embeds(ucfg, B=3)
    seeds = [101, 202, 303]
    if model == "sd15":
        run = lambda u, cc, **kw: s.sample(cfg_guidance=0.6, prompt_embeds=(u, cc), return_latents=True, **kw)  # noqa: E731
    else:
        pool_n, pool = _rand((1, ucfg.addition_pooled_dim), 8, dtype=H), _rand((3, ucfg.addition_pooled_dim), 9, dtype=H)
        run = lambda u, cc, **kw: s.sample(cfg_guidance=0.6, prompt_embeds=(u, cc, pool_n, pool[:cc.shape[0]] if cc.shape[0] == 3 else pool[kw.pop("row"):][:1]),  # noqa: E731
                                           return_latents=True, target_size=(64, 64), original_size=(64, 64), **kw)
    den, x = run(uc, c, seeds=seeds)
    for b in range(3):
        extra = {} if model == "sd15" else {"row": b}
        d1, x1 = run(uc[b:b + 1], c[b:b + 1], seeds=seeds[b:b + 1], **extra)
        assert torch.equal(d1[0], den[b]) and torch.equal(x1[0], x[b])
    # seeds=None: the start latent from torch's CPU generator and B noise seeds drawn once per job, the same for every step
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        del eng.scalls[:]
        runs.append(run(uc, c)[0])
        used = [v["seeds"] for nm, v in eng.scalls if nm == "step_sde" and not v["last"]]
        assert len(used) == 4 and len(used[0]) == 3 and all(u == used[0] for u in used) and len(set(used[0])) == 3
    assert torch.equal(runs[0], runs[1])
    with pytest.raises(ValueError, match="2 seeds for a batch of 3"):
        run(uc, c, seeds=[1, 2])


def test_refusals_by_name():
    from cfgpp_amd.sde import get_sde_solver, sde_solver_names
    assert sde_solver_names() == NAMES
    with pytest.raises(ValueError, match="SDESolver dpm\\+\\+_sde does not exist"):
        _solver("dpm++_sde")
    with pytest.raises(ValueError, match="SDESolver model 'sd3'"):
        get_sde_solver("dpm++_2m_sde", model="sd3")
    for model in ("sd15", "sdxl"):
        with pytest.raises(ValueError, match="'dpm\\+\\+_2m_sde'.*zero_terminal_snr"):
            _solver("dpm++_2m_sde", model, zero_terminal_snr=True, prediction_type="v_prediction", timestep_spacing="trailing")
        with pytest.raises(ValueError, match="'dpm\\+\\+_3m_sde_cfg\\+\\+'.*guidance_rescale=0.7"):
            _solver("dpm++_3m_sde_cfg++", model, guidance_rescale=0.7, prediction_type="v_prediction")
        with pytest.raises(ValueError, match="'dpm\\+\\+_3m_sde'.*solver_type='heun'.*2M"):
            _solver("dpm++_3m_sde", model, solver_type="heun")
        with pytest.raises(ValueError, match="solver_type='euler'"):
            _solver("dpm++_2m_sde", model, solver_type="euler")
        with pytest.raises(ValueError, match="sigma_schedule='linear'"):
            _solver("dpm++_2m_sde", model, sigma_schedule="linear")
        for k in ("eta", "s_noise"):
            for bad in (-0.1, float("nan"), float("inf")):
                with pytest.raises(ValueError, match=f"'dpm\\+\\+_2m_sde'.*{k}="):
                    _solver("dpm++_2m_sde", model, **{k: bad})
    s, eng, ucfg = _solver()
    uc, c = _embeds(ucfg)
    for k in ("src_img", "mask", "strength"):
        with pytest.raises(ValueError, match=f"dpm\\+\\+_2m_sde_cfg\\+\\+.*{k}.*inversion, edit and inpaint"):
            s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), **{k: torch.zeros(1, 3, 64, 64)})
    with pytest.raises(ValueError, match="dpm\\+\\+_2m_sde_cfg\\+\\+.*inversion is not supported"):
        s.inversion(torch.zeros(1, 4, 8, 8), uc, c)
    with pytest.raises(ValueError, match="dpm\\+\\+_2m_sde_cfg\\+\\+.*guidance_rescale"):      # the per-job form too
        s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), guidance_rescale=0.5)
    assert eng.scalls == [] and eng.calls == []
    # graph replay is never used: the eager loop runs also when the engine offers graphs
    eng.graph_enabled = True
    eng.ddim_loop_graph = lambda *a, **k: (_ for _ in ()).throw(AssertionError("graph replay"))
    s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), seeds=[1, 2], return_latents=True)
    assert len([1 for nm, _ in eng.scalls if nm == "step_sde"]) == 5
    # the reference registries keep their names
    from cfgpp_amd import latent_diffusion, latent_sdxl
    assert not set(NAMES) & set(latent_diffusion.__SOLVER__) and not set(NAMES) & set(latent_sdxl.__SOLVER__)


def test_sharded_run_needs_seeds(monkeypatch):
    import torch.distributed as dist
    s, eng, ucfg = _solver()
    uc, c = _embeds(ucfg)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(ValueError, match="dpm\\+\\+_2m_sde_cfg\\+\\+.*sharded run.*seeds"):
        s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), latents=_rand((2, 4, 8, 8), 1))
    s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), latents=_rand((2, 4, 8, 8), 1), seeds=[5, 6], return_latents=True)


# ------------------------------------------------------------------------------------------------ CLI
@pytest.mark.parametrize("model,method", [("sd15", "dpm++_2m_sde_cfg++"), ("sdxl", "dpm++_3m_sde")])
def test_cli_method_sde(tmp_path, model, method):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import text_to_img
    from cfgpp_amd.sde import sde_coeffs
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    eng = SDEMockEngine(_unet, (8, 8))
    cfg = TINY_SD if model == "sd15" else TINY_XL
    extra = ["--solver_type", "heun"] if "2m" in method else []
    text_to_img.main(["--method", method, "--model", model, "--cfg_guidance", "0.6", "--NFE", "3", "--prompt", "a cat", "--device", "cpu",
                      "--workdir", str(tmp_path), "--eta", "0.5", "--s_noise", "0.8", "--sigma_schedule", "exponential", "--seed", "4"] + extra,
                     solver_kwargs=dict(engine=eng, vae=StubVAE(cfg.vae_scale), latent_hw=(8, 8), unet_config=cfg))
    assert [nm for nm, _ in eng.scalls] == ["sde_input"] + ["step_sde"] * 3
    steps = [v for _, v in eng.scalls[1:]]
    assert [st["last"] for st in steps] == [False, False, True] and all(st["cfgpp"] == method.endswith("++") for st in steps)
    from cfgpp_amd.schedule import SchedulerTables
    sig = SchedulerTables(3).exponential_sigmas()
    kind = "2m" if "2m" in method else "3m"
    assert steps[1]["coef"] == sde_coeffs(sig, 1, kind, "heun" if extra else "midpoint", 0.5, 0.8, method.endswith("++"), 1)
    assert os.path.exists(tmp_path / "result" / "generated.png")


# ------------------------------------------------------------------------------------------------ the extension header
def test_sde_header_is_exported_and_bound():
    from cfgpp_amd import _lib
    from cfgpp_amd.build import CSRC, SOURCES, _deps, build
    assert dict(SOURCES)["sde_kernels.hip"] == ["-ffp-contract=off"] == dict(SOURCES)["lcm_kernels.hip"]
    build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cfgpp_sde.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cfgpp_[a-z0-9_]+)\s*\(", code))
    assert declared == {"cfgpp_sde_input", "cfgpp_step_sde"} == set(_lib.SDE_PROTOTYPES)
    assert all(hasattr(lib, n) for n in declared)
    for name in declared:        # the bound argument count is the declared one
        args = re.search(name + r"\((.*?)\);", code, flags=re.S).group(1)
        assert len(_lib.SDE_PROTOTYPES[name][1]) == args.count(",") + 1, name
    for word in ("rounding contract", "m_hat = h(m_uc + h(lam * h(m_c - m_uc)))", "den   = fl(x - fl(sigma * m_hat))", "acc = fl(a_x * x)",
                 "stream_id 2", "{sigma, a_x, a_d, a_u, a_1, a_2, a_n, s_in_next}", "hist_out may be the same buffer as hist2"):
        assert word in hdr, word
    assert '#include "cfgpp.h"' in hdr and "cfgpp_sde" not in open(os.path.join(ROOT, "include", "cfgpp.h")).read()
    # one Philox: both translation units reach the shared device header, and the library's source digest covers it and the new file
    philox = os.path.join(CSRC, "philox.h")
    for tu in ("lcm_kernels.hip", "sde_kernels.hip"):
        assert philox in _deps(os.path.join(CSRC, tu)), tu
        assert "philox4x32_10(uint32_t" not in open(os.path.join(CSRC, tu)).read()       # not defined a second time
    assert _lib.build_id().startswith("cfgpp-build:" + __import__("cfgpp_amd.build", fromlist=["source_digest"]).source_digest() + ":")


# ------------------------------------------------------------------------------------------------ fault injection
def _toy(lam_scale=0.25):
    """a linear toy epsilon model, the same in fp16 / fp32 (sde_chain) and in float64 (literal_chain)"""
    def fp(xc, i):
        m_uc = (xc.float() * 0.30).half()
        m_c = (xc.float() * 0.45 + 0.1).half()
        return m_uc, m_c
    return fp


def _chain(faults, kind="3m", cfgpp=True, n=5, lam=0.6):
    from cfgpp_amd.sde import sde_coeffs
    sig = _schedule("karras", n)
    coef = lambda i, nh: sde_coeffs(sig, i, kind, "midpoint", 1.0, 1.0, cfgpp, nh)  # noqa: E731
    z = _rand((2, 4, 8, 8), 1)
    den, x, rec = S.sde_chain(_toy(), z, [1, 2], sig, coef, kind, lam, cfgpp, faults=faults)
    return den, x, rec, sig, z


def _literal_of_chain(kind, cfgpp, sig, z, lam):
    """the literal float64 algorithm on the toy model and the model's noise"""
    sg = [float(v) for v in sig]
    n = len(sg) - 1
    noises = [S.noise_rows(2, 256, [1, 2], i, z.shape).double().numpy() for i in range(n)]

    def denoise(x, i):
        xc = x / math.sqrt(sg[i] ** 2 + 1)
        e_uc, e_c = 0.30 * xc, 0.45 * xc + 0.1
        return x - sg[i] * (e_uc + lam * (e_c - e_uc)), x - sg[i] * e_uc
    return S.literal_chain(kind, denoise, z.double().numpy() * sg[0], sg, noises, 1.0, 1.0, "midpoint", cfgpp)[-1]


def _guard_chain_is_the_literal_algorithm(faults, kind="3m"):
    """the fp32 / fp16 chain against the float64 literal algorithm: fp16 roundings of the model output and the UNet input (2^-11
    relative each, a handful per step, 5 steps) keep the two within 1e-2 of the result's scale; a wrong term is off by far more"""
    den, x, _, sig, z = _chain(faults, kind)
    want = _literal_of_chain(kind, True, sig, z, 0.6)
    return float(np.abs(den.double().numpy() - want).max()) <= 1e-2 * float(np.abs(want).max())


def _guard_last_step_adds_no_noise(faults):
    den, x, *_ = _chain(faults)
    return torch.equal(den, x)


def _guard_draw_advances(faults):
    rec = _chain(faults)[2]
    return [r["draw"] for r in rec] == list(range(len(rec)))


FAULTS = [("noise_on_last", _guard_last_step_adds_no_noise), ("draw_stuck", _guard_draw_advances),
          ("hist_not_rotated", _guard_chain_is_the_literal_algorithm), ("a_u_sign", _guard_chain_is_the_literal_algorithm),
          ("cfgpp_hist_den", _guard_chain_is_the_literal_algorithm)]


@pytest.mark.parametrize("fault,guard", FAULTS, ids=[f for f, _ in FAULTS])
def test_each_fault_breaks_the_assertion_that_guards_it(fault, guard):
    assert bool(guard(())) is True, "the guard has to hold on the clean model"
    assert bool(guard((fault,))) is False, f"fault {fault!r} went unnoticed"
    assert not torch.equal(_chain(())[1], _chain((fault,))[1])      # and the fault changes what the chain computes
    if guard is _guard_chain_is_the_literal_algorithm:               # 2M has a history too
        assert guard((), "2m") and (fault != "hist_not_rotated" or not guard((fault,), "2m"))
