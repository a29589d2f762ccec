"""CPU: DPM++ SDE sampling - the stage rows (cfgpp_amd/dpmpp_sde.py: dpmpp_sde_coeffs) against k-diffusion's ``sample_dpmpp_sde``
written literally in float64 with a noise sampler on ONE explicit Brownian path and against the reference's two 2S CFG++ lines
(tests/dpmpp_sde_ref.py), identities that hold exactly, the solvers' plumbing on a mock engine (tests/dpmpp_sde_mock.py), the
refusals, the CLI route and the library's DPM++ SDE header."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import dpmpp_sde_ref as S
from dpmpp_sde_mock import DPMppSDEMockEngine
from mock_engine import StubVAE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, F, D = torch.float16, torch.float32, torch.float64
NAMES = ["dpm++_sde", "dpm++_sde_cfg++"]
ETAS = [0.0, 0.5, 1.0, 1.7]


def _rand(shape, seed, scale=1.0, dtype=F):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=D) * scale).to(dtype)


def _schedule(name, n=6):
    """the product's fp32 sigma table"""
    from cfgpp_amd.schedule import SchedulerTables
    tb = SchedulerTables(n)
    return tb.karras_sigmas() if name == "karras" else tb.exponential_sigmas()


def _denoise64(lam):
    """a smooth nonlinear float64 model: (guided, unconditional) denoised estimate at (x, sigma)"""
    def fn(x, sigma):
        s_in = 1.0 / math.sqrt(float(sigma) ** 2 + 1.0)
        e_uc = 0.20 * x * s_in + 0.05 * np.sin(x)
        e_c = 0.35 * x * s_in + 0.10 * np.cos(x)
        return x - sigma * (e_uc + lam * (e_c - e_uc)), x - sigma * e_uc
    return fn


def _path(sig, seed=7, width=16):
    rng = np.random.default_rng(seed)
    n = len(sig) - 1
    return rng.standard_normal(width) * sig[0], rng.standard_normal((n, width)), rng.standard_normal((n, width))


# ------------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("schedule", ["karras", "exponential"])
@pytest.mark.parametrize("eta", ETAS)
def test_rows_equal_k_diffusion_written_literally(eta, schedule):
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_coeffs64
    sig = [float(v) for v in _schedule(schedule)]
    x0, n1s, n2s = _path(sig)
    s_noise = 0.9
    den = _denoise64(3.0)
    want = S.literal_chain(den, x0, sig, n1s, n2s, eta, s_noise)
    got = S.row_chain(lambda i, st: dpmpp_sde_coeffs64(sig, i, st, eta, s_noise, False), den, x0, sig, n1s, n2s)
    assert len(got) == len(want) == 6
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(w).all()
        assert float(np.abs(g - w).max()) <= 1e-12 * float(np.abs(w).max()), (i, float(np.abs(g - w).max() / np.abs(w).max()))
    assert np.array_equal(got[-1], den(got[-2], sig[-2])[0])            # sigma_next = 0: x' = D


@pytest.mark.parametrize("schedule", ["karras", "exponential"])
def test_cfgpp_rows_at_eta_zero_equal_the_references_two_stage_lines(schedule):
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_coeffs64
    sig = [float(v) for v in _schedule(schedule)]
    x0, n1s, n2s = _path(sig, 11)
    den = _denoise64(0.6)
    want = S.literal_2s_cfgpp(den, x0, sig)
    got = S.row_chain(lambda i, st: dpmpp_sde_coeffs64(sig, i, st, 0.0, 1.0, True), den, x0, sig, n1s * np.nan, n2s * np.nan)
    for i, (g, w) in enumerate(zip(got, want)):
        assert float(np.abs(g - w).max()) <= 1e-12 * float(np.abs(w).max()), (i, float(np.abs(g - w).max() / np.abs(w).max()))
    # and the guided and the unconditional estimate are told apart: with the plain rows the chain is another one
    plain = S.row_chain(lambda i, st: dpmpp_sde_coeffs64(sig, i, st, 0.0, 1.0, False), den, x0, sig, n1s, n2s)
    assert float(np.abs(plain[0] - want[0]).max()) > 1e-3 * float(np.abs(want[0]).max())


@pytest.mark.parametrize("schedule", ["karras", "exponential"])
def test_identities(schedule):
    from cfgpp_amd.dpmpp_sde import TERM_D, TERM_N1, TERM_N2, TERM_U, dpmpp_sde_coeffs, dpmpp_sde_coeffs64, sigma_mid
    sig = [float(v) for v in _schedule(schedule)]
    n = len(sig) - 1
    for eta in ETAS + [5.0]:
        for s_noise in (1.0, 0.7):
            for i in range(n - 1):
                mid = sigma_mid(sig, i)
                assert mid == math.sqrt(sig[i] * sig[i + 1])
                d1, d2 = sig[i] - mid, mid - sig[i + 1]
                sd1, su1 = S.get_ancestral_step(sig[i], mid, eta)
                sd2, su2 = S.get_ancestral_step(sig[i], sig[i + 1], eta)
                for cfgpp in (False, True):
                    a = dpmpp_sde_coeffs64(sig, i, "A", eta, s_noise, cfgpp)
                    b = dpmpp_sde_coeffs64(sig, i, "B", eta, s_noise, cfgpp)
                    assert not a.last and not b.last and all(math.isfinite(v) for v in a.coef + b.coef)
                    assert a.coef[0] == sig[i] and b.coef[0] == mid
                    assert a.coef[1] == sd1 / sig[i] and b.coef[1] == sd2 / sig[i]
                    assert a.coef[6] == 1 / math.sqrt(mid * mid + 1) and b.coef[6] == 1 / math.sqrt(sig[i + 1] ** 2 + 1)
                    # the noise: stage A's amplitude, stage B's two coefficients of one path
                    assert a.coef[4] == su1 * s_noise and a.coef[5] == 0.0
                    amp = su2 * s_noise
                    assert abs(b.coef[4] ** 2 + b.coef[5] ** 2 - amp ** 2) <= 4e-16 * amp ** 2
                    if amp:
                        assert abs(b.coef[4] / amp - math.sqrt(d1 / (d1 + d2))) <= 4e-16
                        assert abs(b.coef[5] / amp - math.sqrt(d2 / (d1 + d2))) <= 4e-16
                    noisy = eta > 0
                    assert bool(a.terms & TERM_N1) == noisy == bool(b.terms & TERM_N1) == bool(b.terms & TERM_N2) and not a.terms & TERM_N2
                    if not noisy:
                        assert a.coef[4] == a.coef[5] == b.coef[4] == b.coef[5] == 0.0
                    if eta == 5.0:                                          # sigma_down = 0: no t_fn(0), the rows stay finite
                        assert a.coef[1] == 0.0 == b.coef[1] and sd1 == 0.0 == sd2
                    # which denoised terms are on
                    if cfgpp:
                        assert a.terms & (TERM_D | TERM_U) == TERM_U and b.terms & (TERM_D | TERM_U) == TERM_D | TERM_U
                        assert a.coef[2] == 0.0 and a.coef[3] == 1.0 - a.coef[1]
                        assert b.coef[2] == (1.0 - b.coef[1]) + b.coef[1] and b.coef[3] == -b.coef[1]
                    else:
                        assert a.terms & (TERM_D | TERM_U) == TERM_D == b.terms & (TERM_D | TERM_U)
                        assert a.coef[3] == 0.0 == b.coef[3] and a.coef[2] == 1.0 - a.coef[1] and b.coef[2] == 1.0 - b.coef[1]
                    # fp32 rows: the float64 rows, each entry rounded once
                    for st, r64 in (("A", a), ("B", b)):
                        r32 = dpmpp_sde_coeffs(sig, i, st, eta, s_noise, cfgpp)
                        assert r32.coef == tuple(float(np.float32(v)) for v in r64.coef) and r32[1:] == r64[1:]
            # the last step: one stage, x' = D
            for cfgpp in (False, True):
                z = dpmpp_sde_coeffs64(sig, n - 1, "A", eta, s_noise, cfgpp)
                assert z.last and z.terms == 0 and z.coef == (sig[n - 1], 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
                assert dpmpp_sde_coeffs(sig, n - 1, "A", eta, s_noise, cfgpp) == z._replace(coef=tuple(float(np.float32(v)) for v in z.coef))
                with pytest.raises(ValueError, match="has one stage"):
                    dpmpp_sde_coeffs64(sig, n - 1, "B", eta, s_noise, cfgpp)
    with pytest.raises(ValueError, match="stage='C'"):
        dpmpp_sde_coeffs64(sig, 0, "C")


def test_stage_noises_are_increments_of_one_path():
    """n1 and nB = (c_1 n1 + c_2 n2) / (su2 s_noise): unit variance each and correlation sqrt(d1 / (d1 + d2)), from the rows alone"""
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_coeffs64
    sig = [float(v) for v in _schedule("karras")]
    for i in range(5):
        b = dpmpp_sde_coeffs64(sig, i, "B", 1.0, 1.0, False)
        _, su2 = S.get_ancestral_step(sig[i], sig[i + 1], 1.0)
        mid = math.sqrt(sig[i] * sig[i + 1])
        w1, w2 = b.coef[4] / su2, b.coef[5] / su2
        assert abs(w1 * w1 + w2 * w2 - 1.0) <= 1e-15                      # Var nB = 1
        assert abs(w1 - math.sqrt((sig[i] - mid) / (sig[i] - sig[i + 1]))) <= 1e-15      # Cov(n1, nB) = sqrt(d1 / (d1 + d2))


# ------------------------------------------------------------------------------------------------ solver plumbing on the mock engine
def _unet(z, t, ehs, te, ti):
    v = 0.3 * z.float() * math.cos(0.004 * t) + 0.05 * ehs.float().mean(dim=(1, 2)).view(-1, 1, 1, 1) + 0.02 * math.sin(0.01 * t)
    if te is not None:
        v = v + 0.01 * te.float().mean(dim=1).view(-1, 1, 1, 1)
    return v.half()


def _solver(name="dpm++_sde_cfg++", model="sd15", nfe=4, unet=_unet, **kw):
    from cfgpp_amd.dpmpp_sde import get_dpmpp_sde_solver
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    cfg = TINY_SD if model == "sd15" else TINY_XL
    eng = DPMppSDEMockEngine(unet, (8, 8))
    s = get_dpmpp_sde_solver(name, model=model, solver_config=types.SimpleNamespace(num_sampling=nfe), device="cpu", unet_config=cfg,
                             max_batch=3, latent_hw=(8, 8), engine=eng, vae=StubVAE(cfg.vae_scale), **kw)
    return s, eng, cfg


def _embeds(cfg, B=2, seed=5):
    return _rand((B, 77, cfg.cross_attention_dim), seed, dtype=H), _rand((B, 77, cfg.cross_attention_dim), seed + 1, dtype=H)


def _model_fn(s, uc, c, te=None, v_pred=False):
    """what a UNet call of the solver returns at ``sigma``, as epsilon: the mock UNet at the product's timestep of that sigma (and,
    for a v-model, the mock's v -> eps conversion with that sigma)"""
    B = c.shape[0]
    ehs = torch.cat([uc, c], 0)

    def fn(xc, sigma):
        sigma = torch.as_tensor(sigma, dtype=F)
        e = _unet(torch.cat([xc, xc], 0), float(s.timestep(sigma)), ehs, te, None)
        m_uc, m_c = e[:B].contiguous(), e[B:].contiguous()
        if v_pred:
            from cfgpp_amd import coeffs as K
            from vpred_mock import emulate_v_to_eps
            a, sc = K.v_to_eps_coeffs(sigma, s.scalar_semantics)
            emulate_v_to_eps(m_uc, m_c, m_uc, m_c, xc, a, sc)
        return m_uc, m_c
    return fn


CASES = [("dpm++_sde", {}, 7.5, "epsilon"), ("dpm++_sde_cfg++", {}, 0.6, "epsilon"),
         ("dpm++_sde_cfg++", dict(sigma_schedule="exponential", eta=0.5, s_noise=0.9), 0.6, "epsilon"),
         ("dpm++_sde", dict(eta=0.0), 5.0, "epsilon"), ("dpm++_sde", dict(eta=5.0), 5.0, "epsilon"),
         ("dpm++_sde_cfg++", {}, 0.6, "v_prediction")]


@pytest.mark.parametrize("name,opts,lam,pt", CASES)
def test_sd_loop_is_the_model(name, opts, lam, pt):
    from cfgpp_amd import coeffs as K
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_coeffs
    n = 4
    s, eng, ucfg = _solver(name, prediction_type=pt, **opts)
    uc, c = _embeds(ucfg)
    zT = _rand((2, 4, 8, 8), 1)
    seeds = [11, (7 << 40) + 5]
    den, x = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, seeds=seeds, return_latents=True)
    cfgpp = name.endswith("++")
    sigmas = s.sde_sigmas()
    row = lambda i, st: dpmpp_sde_coeffs(sigmas, i, st, opts.get("eta", 1.0), opts.get("s_noise", 1.0), cfgpp)  # noqa: E731
    w_den, w_x, rec = S.chain(_model_fn(s, uc, c, v_pred=(pt == "v_prediction")), zT, seeds, sigmas, row, lam)
    assert den.dtype == F and x.dtype == F and torch.equal(den, w_den) and torch.equal(x, w_x)
    assert torch.equal(x, den)                                       # the last step: x' = D, no noise
    # exactly sde_input, then two launches per step and ONE for the last; 2N - 1 UNet calls at timestep(sigma_i), timestep(sigma_mid)
    assert [nm for nm, _ in eng.scalls] == ["sde_input"] + ["step_sde_stage"] * (2 * n - 1) and eng.lcalls == []
    assert len(rec) == len(eng.calls) == 2 * n - 1
    mids = [torch.tensor(np.float32(math.sqrt(float(sigmas[i]) * float(sigmas[i + 1])))) for i in range(n - 1)]
    want_t = [float(s.timestep(v)) for i in range(n) for v in ([sigmas[i]] + ([mids[i]] if i < n - 1 else []))]
    assert [c_["t"] for c_ in eng.calls] == want_t and len(set(want_t)) == 2 * n - 1
    assert all(c_["z_dtype"] == H for c_ in eng.calls)
    if pt == "v_prediction":                                         # v -> eps after every UNet call, with that call's sigma
        assert [v[0] for v in eng.vcalls] == ["v_to_eps"] * (2 * n - 1)
        assert [v[1] for v in eng.vcalls] == [tuple(float(q) for q in K.v_to_eps_coeffs(torch.tensor(r["sigma"]), s.scalar_semantics))
                                              for r in rec]
    else:
        assert eng.vcalls == []
    assert eng.scalls[0][1]["s_in"] == float(np.float32(1.0 / math.sqrt(float(sigmas[0]) ** 2 + 1.0)))
    st = [v for _, v in eng.scalls[1:]]
    for k, r in zip(st, rec):
        i = r["i"]
        assert k["coef"] == r["row"].coef and k["terms"] == r["row"].terms and k["last"] == r["row"].last
        assert (k["draw1"], k["draw2"]) == (2 * i, 2 * i + 1)       # BOTH stages of step i: the same two counters
        assert k["seeds"] == seeds and k["lam"] == lam and not k["single"] and not k["noise_given"]
    A, B = st[0:-1:2], st[1::2]
    assert len(A) == len(B) == n - 1 and [r["stage"] for r in rec] == ["A", "B"] * (n - 1) + ["A"]
    xid, xcid = st[0]["x"], eng.scalls[0][1]["xc"]
    assert len({k["den_out"] for k in A} | {st[-1]["den_out"]}) == 1 and len({k["out"] for k in A}) == 1     # one den, one x2
    x2id, denid = A[0]["out"], A[0]["den_out"]
    assert len({xid, x2id, denid}) == 3
    for k in A:
        assert (k["x"], k["base"], k["out"], k["xc_out"]) == (xid, xid, x2id, xcid) and not k["last"]
    for k in B:                                                      # in place on x; D2 lands in the dead x2, den stays stage A's
        assert (k["x"], k["base"], k["out"], k["den_out"], k["xc_out"]) == (xid, x2id, xid, x2id, xcid) and not k["last"]
    z = st[-1]
    assert z["last"] and (z["x"], z["base"], z["out"], z["den_out"], z["xc_out"]) == (xid, xid, xid, denid, None)
    # callbacks: once per step after stage B, z0t = stage A's denoised, zt = x; they leave the result alone
    seen = []
    d2, _ = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, seeds=seeds, return_latents=True,
                     callback_fn=lambda i, t, kw: (seen.append((i, int(t), kw["z0t"].clone(), kw["zt"].clone())), kw)[1])
    assert torch.equal(d2, den) and [i for i, *_ in seen] == list(range(n)) and torch.equal(seen[-1][2], den)
    assert [t for _, t, *_ in seen] == [int(s.timestep(sigmas[i])) for i in range(n)]
    assert all(torch.equal(z0t, r["den"]) for (_, _, z0t, _), r in zip(seen, [r for r in rec if r["stage"] == "A"]))
    img = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, seeds=seeds)
    assert torch.equal(img, (StubVAE(ucfg.vae_scale).decode(den) / 2 + 0.5).clamp(0, 1))
    d3, _ = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, seeds=[1, 2], return_latents=True)
    if opts.get("eta") == 0.0:                                       # deterministic: other seeds for the noise, the same result
        assert torch.equal(d3, den) and all(k["coef"][4] == 0.0 == k["coef"][5] and k["terms"] < 4 for k in st)
    else:
        assert not torch.equal(d3, den)


@pytest.mark.parametrize("name,lam", [("dpm++_sde_cfg++", 0.6), ("dpm++_sde", 5.0)])
def test_sdxl_loop_is_the_model(name, lam):
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_coeffs
    s, eng, ucfg = _solver(name, "sdxl")
    uc, c = _embeds(ucfg)
    pool_n, pool = _rand((1, ucfg.addition_pooled_dim), 8, dtype=H), _rand((2, ucfg.addition_pooled_dim), 9, dtype=H)
    zT = _rand((2, 4, 8, 8), 2)
    seeds = [3, 4]
    den, x = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c, pool_n, pool), latents=zT, seeds=seeds, return_latents=True,
                      target_size=(64, 64), original_size=(64, 64))
    te = eng.te
    assert int(te.shape[0]) == 4 and not torch.equal(te[:2], te[2:])                    # SDXL's added conditioning, both halves
    sigmas = s.sde_sigmas()
    row = lambda i, st: dpmpp_sde_coeffs(sigmas, i, st, 1.0, 1.0, name.endswith("++"))  # noqa: E731
    w_den, w_x, _ = S.chain(_model_fn(s, uc, c, te), zT, seeds, sigmas, row, lam)
    assert torch.equal(den, w_den) and torch.equal(x, w_x)
    assert [nm for nm, _ in eng.scalls] == ["sde_input"] + ["step_sde_stage"] * 7 and len(eng.calls) == 7
    img = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c, pool_n, pool), latents=zT, seeds=seeds, target_size=(64, 64), original_size=(64, 64))
    assert torch.equal(img, (StubVAE(ucfg.vae_scale).decode(den) / 2 + 0.5).clamp(0, 1))


def _toy_unet(z, t, ehs, te, ti):
    """a linear toy epsilon model, the same in fp16 / fp32 (the mock) and in float64 (row_chain)"""
    B = z.shape[0] // 2
    return torch.cat([z[:B].float() * 0.30, z[B:].float() * 0.45 + 0.1], 0).half()


@pytest.mark.parametrize("name,eta", [("dpm++_sde", 1.0), ("dpm++_sde_cfg++", 1.0), ("dpm++_sde_cfg++", 0.0)])
def test_chain_on_the_mock_is_the_float64_model(name, eta):
    """the fp32 / fp16 chain on the mock engine against the float64 rows (which ARE k-diffusion's algorithm to 1e-12: the tests above)
    on the same noise.  The fp16 roundings of the model output and of the UNet input (2^-11 relative each, a handful per UNet call, 7
    calls) keep the two within 1e-2 of the result's scale (the bound of tests/test_sde_cpu.py's chain guard); a wrong term, a wrong
    base latent or a wrong draw index is off by far more."""
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_coeffs64
    lam = 0.6 if name.endswith("++") else 3.0
    s, eng, ucfg = _solver(name, unet=_toy_unet, eta=eta)
    uc, c = _embeds(ucfg)
    zT, seeds = _rand((2, 4, 8, 8), 1), [1, 2]
    den, _ = s.sample(cfg_guidance=lam, prompt_embeds=(uc, c), latents=zT, seeds=seeds, return_latents=True)
    sg = [float(v) for v in s.sde_sigmas()]
    noise = lambda d: S.noise_rows(2, 256, seeds, d, zT.shape).double().numpy()  # noqa: E731
    n1s, n2s = [noise(2 * i) for i in range(4)], [noise(2 * i + 1) for i in range(4)]

    def denoise(x, sigma):
        xc = x / math.sqrt(sigma ** 2 + 1)
        e_uc, e_c = 0.30 * xc, 0.45 * xc + 0.1
        return x - sigma * (e_uc + lam * (e_c - e_uc)), x - sigma * e_uc
    want = S.row_chain(lambda i, st: dpmpp_sde_coeffs64(sg, i, st, eta, 1.0, name.endswith("++")), denoise, zT.double().numpy() * sg[0],
                       sg, n1s, n2s)[-1]
    assert float(np.abs(den.double().numpy() - want).max()) <= 1e-2 * float(np.abs(want).max())
    # the draws matter: stage B's n1 swapped for a fresh draw gives another chain, by far more than the bound
    if eta:
        other = S.row_chain(lambda i, st: dpmpp_sde_coeffs64(sg, i, st, eta, 1.0, name.endswith("++")), denoise,
                            zT.double().numpy() * sg[0], sg, n1s, n2s, b_n1s=[noise(100 + i) for i in range(4)])[-1]
        assert float(np.abs(other - want).max()) > 5e-2 * float(np.abs(want).max())


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_batched_chains_equal_independent_runs_and_seeds_none(model):
    s, eng, ucfg = _solver("dpm++_sde_cfg++", model)
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
    # seeds=None: the start latent from torch's CPU generator and B noise seeds drawn once per job, the same for every launch
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        del eng.scalls[:]
        runs.append(run(uc, c)[0])
        used = [v["seeds"] for nm, v in eng.scalls if nm == "step_sde_stage" and not v["last"]]
        assert len(used) == 6 and len(used[0]) == 3 and all(u == used[0] for u in used) and len(set(used[0])) == 3
    assert torch.equal(runs[0], runs[1])
    with pytest.raises(ValueError, match="2 seeds for a batch of 3"):
        run(uc, c, seeds=[1, 2])


def test_a_callback_that_replaces_x_is_followed_by_sde_input():
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_coeffs
    s, eng, ucfg = _solver("dpm++_sde")
    uc, c = _embeds(ucfg)
    zT = _rand((2, 4, 8, 8), 1)
    repl = _rand((2, 4, 8, 8), 99, 2.0)

    def cb(i, t, kw):
        if i == 1:
            kw = dict(kw, zt=repl.clone())
        return kw
    s.sample(cfg_guidance=5.0, prompt_embeds=(uc, c), latents=zT, seeds=[1, 2], return_latents=True, callback_fn=cb)
    names = [nm for nm, _ in eng.scalls]
    step = ["step_sde_stage", "step_sde_stage", "sde_input"]
    assert names == ["sde_input"] + step * 3 + ["step_sde_stage"]       # after every step but the last
    sig = s.sde_sigmas()
    inputs = [v for nm, v in eng.scalls if nm == "sde_input"]
    assert [v["s_in"] for v in inputs] == [float(np.float32(1.0 / math.sqrt(float(sig[i]) ** 2 + 1.0))) for i in range(4)]
    assert inputs[2]["s_in"] == dpmpp_sde_coeffs(sig, 1, "B").coef[6]
    # the UNet call of step 2 saw the replaced latent
    assert torch.equal(eng.calls[4]["z"], (repl * torch.tensor(inputs[2]["s_in"])).half())


def test_refusals_by_name():
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_solver_names, get_dpmpp_sde_solver
    from cfgpp_amd.sde import get_sde_solver, sde_solver_names
    assert dpmpp_sde_solver_names() == NAMES
    assert not set(NAMES) & set(sde_solver_names())
    with pytest.raises(ValueError, match="SDESolver dpm\\+\\+_sde does not exist"):      # sde.py's registry keeps refusing it
        get_sde_solver("dpm++_sde")
    with pytest.raises(ValueError, match="DPMppSDESolver dpm\\+\\+_2m_sde does not exist"):
        _solver("dpm++_2m_sde")
    with pytest.raises(ValueError, match="DPMppSDESolver model 'sd3'"):
        get_dpmpp_sde_solver("dpm++_sde", model="sd3")
    for model in ("sd15", "sdxl"):
        with pytest.raises(ValueError, match="'dpm\\+\\+_sde'.*zero_terminal_snr"):
            _solver("dpm++_sde", model, zero_terminal_snr=True, prediction_type="v_prediction", timestep_spacing="trailing")
        with pytest.raises(ValueError, match="'dpm\\+\\+_sde_cfg\\+\\+'.*guidance_rescale=0.7"):
            _solver("dpm++_sde_cfg++", model, guidance_rescale=0.7, prediction_type="v_prediction")
        for st in ("heun", "midpoint"):
            with pytest.raises(ValueError, match=f"'dpm\\+\\+_sde'.*solver_type='{st}'.*2M"):
                _solver("dpm++_sde", model, solver_type=st)
        with pytest.raises(ValueError, match="sigma_schedule='linear'"):
            _solver("dpm++_sde", model, sigma_schedule="linear")
        for k in ("eta", "s_noise"):
            for bad in (-0.1, float("nan"), float("inf")):
                with pytest.raises(ValueError, match=f"'dpm\\+\\+_sde'.*{k}="):
                    _solver("dpm++_sde", model, **{k: bad})
    s, eng, ucfg = _solver()
    uc, c = _embeds(ucfg)
    for k in ("src_img", "mask", "strength"):
        with pytest.raises(ValueError, match=f"dpm\\+\\+_sde_cfg\\+\\+.*{k}.*inversion, edit and inpaint"):
            s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), **{k: torch.zeros(1, 3, 64, 64)})
    with pytest.raises(ValueError, match="dpm\\+\\+_sde_cfg\\+\\+.*inversion is not supported"):
        s.inversion(torch.zeros(1, 4, 8, 8), uc, c)
    with pytest.raises(ValueError, match="dpm\\+\\+_sde_cfg\\+\\+.*guidance_rescale"):      # the per-job form too
        s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), guidance_rescale=0.5)
    assert eng.scalls == [] and eng.calls == []
    # graph replay is never used: the eager loop runs also when the engine offers graphs
    eng.graph_enabled = True
    eng.ddim_loop_graph = lambda *a, **k: (_ for _ in ()).throw(AssertionError("graph replay"))
    s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), seeds=[1, 2], return_latents=True)
    assert len([1 for nm, _ in eng.scalls if nm == "step_sde_stage"]) == 7
    # the reference registries keep their names
    from cfgpp_amd import latent_diffusion, latent_sdxl
    assert not set(NAMES) & set(latent_diffusion.__SOLVER__) and not set(NAMES) & set(latent_sdxl.__SOLVER__)


def test_sharded_run_needs_seeds(monkeypatch):
    import torch.distributed as dist
    s, eng, ucfg = _solver()
    uc, c = _embeds(ucfg)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    with pytest.raises(ValueError, match="dpm\\+\\+_sde_cfg\\+\\+.*sharded run.*seeds"):
        s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), latents=_rand((2, 4, 8, 8), 1))
    s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), latents=_rand((2, 4, 8, 8), 1), seeds=[5, 6], return_latents=True)


# ------------------------------------------------------------------------------------------------ CLI
@pytest.mark.parametrize("model,method", [("sd15", "dpm++_sde_cfg++"), ("sdxl", "dpm++_sde")])
def test_cli_method_dpmpp_sde(tmp_path, model, method):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import text_to_img
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_coeffs
    from cfgpp_amd.schedule import SchedulerTables
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    eng = DPMppSDEMockEngine(_unet, (8, 8))
    cfg = TINY_SD if model == "sd15" else TINY_XL
    argv = ["--method", method, "--model", model, "--cfg_guidance", "0.6", "--NFE", "3", "--prompt", "a cat", "--device", "cpu",
            "--workdir", str(tmp_path), "--eta", "0.5", "--s_noise", "0.8", "--sigma_schedule", "exponential", "--seed", "4"]
    kw = dict(engine=eng, vae=StubVAE(cfg.vae_scale), latent_hw=(8, 8), unet_config=cfg)
    text_to_img.main(argv, solver_kwargs=kw)
    assert [nm for nm, _ in eng.scalls] == ["sde_input"] + ["step_sde_stage"] * 5
    st = [v for _, v in eng.scalls[1:]]
    assert [k["last"] for k in st] == [False] * 4 + [True]
    sig = SchedulerTables(3).exponential_sigmas()
    cfgpp = method.endswith("++")
    assert st[2]["coef"] == dpmpp_sde_coeffs(sig, 1, "A", 0.5, 0.8, cfgpp).coef and st[3]["coef"] == dpmpp_sde_coeffs(sig, 1, "B", 0.5, 0.8, cfgpp).coef
    assert st[3]["terms"] == dpmpp_sde_coeffs(sig, 1, "B", 0.5, 0.8, cfgpp).terms == (15 if cfgpp else 13)
    assert os.path.exists(tmp_path / "result" / "generated.png")
    with pytest.raises(ValueError, match="solver_type='heun'"):         # the 2M option is refused by name, not dropped
        text_to_img.main(argv + ["--solver_type", "heun"], solver_kwargs=kw)


# ------------------------------------------------------------------------------------------------ the extension header
def test_dpmpp_sde_header_is_exported_and_bound():
    from cfgpp_amd import _lib
    from cfgpp_amd.build import CSRC, SOURCES, _deps, build, source_digest
    assert dict(SOURCES)["dpmpp_sde_kernels.hip"] == ["-ffp-contract=off"] == dict(SOURCES)["sde_kernels.hip"]
    build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cfgpp_dpmpp_sde.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cfgpp_[a-z0-9_]+)\s*\(", code))
    assert declared == {"cfgpp_step_sde_stage"} == set(_lib.DPMPP_SDE_PROTOTYPES)
    for name in declared:        # exported, and bound with the declared argument count and this table's types
        fn = getattr(lib, name)
        args = re.search(name + r"\((.*?)\);", code, flags=re.S).group(1)
        res, argtypes = _lib.DPMPP_SDE_PROTOTYPES[name]
        assert len(argtypes) == args.count(",") + 1 and fn.restype == res and list(fn.argtypes) == argtypes, name
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("PROTOTYPES") and n != "DPMPP_SDE_PROTOTYPES"]
    assert len(others) >= 10 and not any(declared & set(t) for t in others)
    for word in ("rounding contract", "m_hat = h(m_uc + h(lam * h(m_c - m_uc)))", "den   = fl(base - fl(sigma_b * m_hat))",
                 "uden  = fl(base - fl(sigma_b * m_uc))", "acc = fl(a_x * x)", "acc = fl(acc + fl(c_2 * n2))", "stream_id 3",
                 "{sigma_b, a_x, a_d, a_u, c_1, c_2, s_in}", "out must not be base when base is not x"):
        assert word in hdr, word
    bits = dict(re.findall(r"#define (CFGPP_STAGE_[A-Z0-9]+) (\d+)", hdr))
    from cfgpp_amd import dpmpp_sde as P, engine as E
    assert bits == {"CFGPP_STAGE_D": "1", "CFGPP_STAGE_U": "2", "CFGPP_STAGE_N1": "4", "CFGPP_STAGE_N2": "8"}
    assert (P.TERM_D, P.TERM_U, P.TERM_N1, P.TERM_N2) == (1, 2, 4, 8) == (E.STAGE_D, E.STAGE_U, E.STAGE_N1, E.STAGE_N2)
    assert P.NOISE_STREAM == 3 == S.NOISE_STREAM
    # include/cfgpp.h stays the drop-in boundary with its 40 entries
    pub = open(os.path.join(ROOT, "include", "cfgpp.h")).read()
    assert '#include "cfgpp.h"' in hdr and "sde_stage" not in pub and len(_lib.PROTOTYPES) == 40
    # one Philox: the new translation unit reaches the shared device header, whose comment lists the new stream id
    philox = os.path.join(CSRC, "philox.h")
    tu = os.path.join(CSRC, "dpmpp_sde_kernels.hip")
    assert philox in _deps(tu) and "philox4x32_10(uint32_t" not in open(tu).read()
    assert "3: the path increments of the two-stage DPM++ SDE solver" in open(philox).read()
    assert _lib.build_id().startswith("cfgpp-build:" + source_digest() + ":")
