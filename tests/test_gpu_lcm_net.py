"""-m gpu: LCM on the HIP engine - guidance-embedded tiny UNets (time_embedding.cond_proj; include/cfgpp_lcm.h) against the oracle, `lcm`
chains of both families against the same solver on a mock engine whose UNet is the oracle and whose step is the model of
tests/lcm_ref.py fed the model's Philox noise, batched chains against independent runs, launch counts, the LCM-LoRA path on a plain
net, and the seeded ancestral noise.

The oracle takes no guidance embedding and needs none: linear_1(sinusoid + cond_proj w) = W1 sinusoid + (b1 + W1 cond_proj w), so it is
built from a state dict whose ``time_embedding.linear_1.bias`` is b1 + W1 cond_proj w (float64 on the host) - exact by linearity.

Chain tolerances (the convention of tests/test_gpu_unet.py's chain cases: measure the rel-L2 on the MI355X, assert twice it).
Measured, 4-step chains at 16 x 16, 2 chains (CHAIN_MEASURED below; profiles/lcm/README.md): guidance-embedded tiny SD 5.834e-4, tiny XL
4.702e-4; LCM-LoRA on the plain tiny SD 5.586e-4 (cfg_guidance 1.0) and 8.864e-4 (1.5).  The single forwards measured 0.91e-3 .. 1.18e-3
against the 2.5e-3 they are held to."""
import types

import numpy as np
import pytest
import torch

from lcm_mock import LCMMockEngine

pytestmark = pytest.mark.gpu

EPS_REL = 2.5e-3            # the project's per-forward tolerance (tests/test_gpu_unet.py)
H = torch.float16
# measured rel-L2 of the 4-step chains below against the oracle loop -> asserted at twice the value
CHAIN_MEASURED = {("sd15", "embedded"): 5.834e-4, ("sdxl", "embedded"): 4.702e-4, ("sd15", "lora_1.0"): 5.586e-4, ("sd15", "lora_1.5"): 8.864e-4}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def _oracle_sd(cfg, sd, w_emb):
    """the state dict of a plain UNet that computes what the guidance-embedded one does at this embedding"""
    out = {k: v for k, v in sd.items() if k != "time_embedding.cond_proj.weight"}
    w1, wc = sd["time_embedding.linear_1.weight"].double(), sd["time_embedding.cond_proj.weight"].double()
    out["time_embedding.linear_1.bias"] = (sd["time_embedding.linear_1.bias"].double()
                                           + w1 @ (wc @ torch.tensor(w_emb, dtype=torch.float64))).float()
    return out


def _launches(net, z, t=749.0):
    return sum(v["launches"] for k, v in net.profile(z, t).items())


# ---------------------------------------------------------------------------------------------------- one forward
@pytest.mark.parametrize("cfg_name,zr", [("tiny_sd_lcm", 1), ("tiny_sd_lcm", 2), ("tiny_xl_lcm", 1), ("tiny_xl_lcm", 2)])
def test_forward_vs_oracle(cfg_name, zr):
    need_gpu()
    from dataclasses import replace
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.lcm import guidance_scale_embedding
    from cfgpp_amd.unet_config import CONFIGS
    from cfgpp_amd.weights import synth_state_dict
    from oracle.unet_ref import UNetRef
    cfg, R, hw = CONFIGS[cfg_name], 2 * zr, (16, 16)
    base = replace(cfg, time_cond_proj_dim=0)
    g = torch.Generator().manual_seed(1)
    z = torch.randn(zr, 4, *hw, generator=g)
    ehs = (torch.randn(R, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().float()
    te = ti = ack = None
    if cfg.addition_embed:
        te = (torch.randn(R, cfg.addition_pooled_dim, generator=g) * 0.5).half().float()
        ti = torch.tensor([[128.0, 128, 0, 0, 128, 128]] * R)
        ack = {"text_embeds": te, "time_ids": ti}
    sd = synth_state_dict(cfg)
    assert tuple(sd["time_embedding.cond_proj.weight"].shape) == (cfg.block_out_channels[0], cfg.time_cond_proj_dim)
    net = HipUNet(cfg, R, hw).load_state_dict(sd).finalize()
    with pytest.raises(CfgppError, match="after cfgpp_unet_finalize"):
        net.set_time_cond(32)
    net.set_context(ehs, te, ti)
    zd = z.cuda()
    with pytest.raises(CfgppError, match="needs cfgpp_unet_guidance_embedding first"):      # a forward before the embedding is set
        net.forward(zd, 749.0)
    zz = z[torch.arange(R) % zr]
    outs = {}
    for scale in (8.5, 2.0):
        w = guidance_scale_embedding(scale, cfg.time_cond_proj_dim)
        net.guidance_embedding(w)
        got = net.forward(zd, 749.0).clone()
        ref = UNetRef(base, _oracle_sd(cfg, sd, w))(zz, 749.0, ehs, ack)["sample"]
        r = rel_l2(got, ref)
        print(f"{cfg_name} rows={R} guidance {scale}: rel-L2 {r:.3e}")
        assert torch.isfinite(got.float()).all() and r < EPS_REL, r
        outs[scale] = (got, ref)
    # the embedding matters (cannot pass with the feature absent), and the plain net is another function
    assert rel_l2(outs[8.5][0], outs[2.0][0]) > 10 * EPS_REL and rel_l2(outs[8.5][1], outs[2.0][1]) > 10 * EPS_REL
    plain_ref = UNetRef(base, {k: v for k, v in sd.items() if "cond_proj" not in k})(zz, 749.0, ehs, ack)["sample"]
    assert rel_l2(outs[8.5][0], plain_ref) > 10 * EPS_REL
    # launch count: a guidance-embedded engine runs exactly the launches of a plain one (the addend rides on linear_1's launch)
    plain = HipUNet(base, R, hw).load_state_dict({k: v for k, v in sd.items() if "cond_proj" not in k}).finalize()
    plain.set_context(ehs, te, ti)
    plain.forward(zd, 749.0)
    assert _launches(net, zd) == _launches(plain, zd) + 0
    # refusals of the setters
    with pytest.raises(CfgppError, match="has no time_embedding.cond_proj"):
        check_plain(plain)
    with pytest.raises(CfgppError, match="not finite"):
        net.guidance_embedding([float("nan")] + [0.0] * (cfg.time_cond_proj_dim - 1))


def check_plain(plain):
    """cfgpp_unet_guidance_embedding on an engine without cfgpp_unet_set_time_cond: refused by the library itself"""
    import ctypes as C
    from cfgpp_amd._lib import check
    check(plain.lib.cfgpp_unet_guidance_embedding(plain._h, (C.c_float * 32)(), None), "cfgpp_unet_guidance_embedding")


# ---------------------------------------------------------------------------------------------------- chains
def _lcm(model, cfg, **kw):
    from cfgpp_amd.lcm import get_lcm_solver
    return get_lcm_solver("lcm", model=model, unet_config=cfg, max_batch=2, latent_hw=(16, 16), scalar_semantics="cuda", **kw)


def _embeds(s, model):
    if model == "sd15":
        return s.get_text_embed("bad", ["a cat", "a dog"])
    return s.get_text_embed("bad", ["a cat", "a dog"], "bad", ["a cat", "a dog"])


def _sample(s, model, pe, seeds, **kw):
    if model == "sd15":
        return s.sample(prompt_embeds=pe, seeds=seeds, return_latents=True, **kw)
    return s.sample(prompt_embeds=pe, target_size=(128, 128), original_size=(128, 128), seeds=seeds, return_latents=True, **kw)


class OracleLCMMock(LCMMockEngine):
    """the mock engine whose UNet is the oracle: plain weights, or - once the solver has set a guidance embedding - the weights of
    ``_oracle_sd`` for that embedding"""

    def __init__(self, cfg, sd, time_cond=0):
        from dataclasses import replace
        from oracle.unet_ref import UNetRef
        self.ucfg, self.base, self.sd0, self.UNetRef = cfg, replace(cfg, time_cond_proj_dim=0), sd, UNetRef
        self.sd_eff = sd if not time_cond else None
        super().__init__(self._unet, (16, 16), time_cond_proj_dim=time_cond)

    def set_guidance_embedding(self, w_emb):
        super().set_guidance_embedding(w_emb)
        self.sd_eff = _oracle_sd(self.ucfg, self.sd0, [float(v) for v in w_emb])

    def _unet(self, z, t, ehs, te, ti):
        ack = None if te is None else {"text_embeds": te.float(), "time_ids": ti.float()}
        return self.UNetRef(self.base, self.sd_eff)(z.float(), t, ehs.float(), ack)["sample"].half()


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_embedded_chain_vs_oracle_loop(model):
    need_gpu()
    from cfgpp_amd.unet_config import TINY_SD_LCM, TINY_XL_LCM
    from cfgpp_amd.weights import synth_state_dict
    cfg = TINY_SD_LCM if model == "sd15" else TINY_XL_LCM
    sc = types.SimpleNamespace(num_sampling=4)
    hip = _lcm(model, cfg, solver_config=sc, device="cuda")
    assert hip.guidance_embedded and hip.engine.time_cond_proj_dim == 32
    eng = OracleLCMMock(cfg, synth_state_dict(cfg, 0), time_cond=32)
    ref = _lcm(model, cfg, solver_config=sc, device="cpu", text_encoder=hip.text_encoder, engine=eng)
    pe = _embeds(hip, model)
    seeds = [11, 12]
    a_den, a_z = (t.clone() for t in _sample(hip, model, pe, seeds, guidance_scale=8.5))
    b_den, b_z = _sample(ref, model, tuple(x.cpu() for x in pe), seeds, guidance_scale=8.5)
    assert [n for n, _ in eng.lcalls] == ["guidance_embedding"] + ["step_lcm"] * 4
    rel = rel_l2(a_den, b_den)
    other = _sample(hip, model, pe, seeds, guidance_scale=2.0)[0]
    print(f"{model}: embedded LCM chain rel-L2 {rel:.3e}; guidance 8.5 vs 2.0 {rel_l2(a_den, other):.3e}")
    assert torch.isfinite(a_den).all() and torch.equal(a_den, a_z)
    tol = 2 * CHAIN_MEASURED[(model, "embedded")]
    assert rel < tol, rel
    assert rel_l2(a_den, other) > 10 * tol                           # the guidance scale reaches the UNet
    # batched chains equal independent runs, bit for bit
    for b in range(2):
        pe_b = tuple(x[b:b + 1] if x.shape[0] == 2 else x for x in pe)
        d1, _ = _sample(hip, model, pe_b, seeds[b:b + 1], guidance_scale=8.5)
        assert torch.equal(d1[0], a_den[b]), f"chain {b} alone differs from chain {b} of the batch"
    # the same seeds again: the same bits; other seeds: another result
    assert torch.equal(_sample(hip, model, pe, seeds, guidance_scale=8.5)[0], a_den)
    assert not torch.equal(_sample(hip, model, pe, [11, 13], guidance_scale=8.5)[0][1], a_den[1])


def _dyadic_adapter(cfg, rank=4, seed=71):
    """a synthetic LoRA over every matrix of the net (linear, conv and time_emb_proj), entries in {-1, 0, 1} / 32"""
    from cfgpp_amd.lora import ParsedLora
    from cfgpp_amd.unet_config import param_shapes
    out = ParsedLora()
    keys = [k for k, s in param_shapes(cfg).items() if len(s) in (2, 4) and k not in ("conv_in.weight", "conv_out.weight")]
    for i, k in enumerate(keys):
        s = param_shapes(cfg)[k]
        O, K = int(s[0]), int(np.prod(s[1:]))
        g = torch.Generator().manual_seed(seed + i)
        out[k] = (torch.randint(-1, 2, (O, rank), generator=g).float() / 32.0, torch.randint(-1, 2, (rank, K), generator=g).float() / 32.0, None)
    return out


@pytest.mark.parametrize("cfg_guidance", [1.0, 1.5])
def test_lcm_lora_on_a_plain_net_vs_oracle_loop(cfg_guidance):
    need_gpu()
    from cfgpp_amd.lora import merge_into_state_dict
    from cfgpp_amd.unet_config import TINY_SD
    from cfgpp_amd.weights import synth_state_dict
    ad = _dyadic_adapter(TINY_SD)
    sc = types.SimpleNamespace(num_sampling=4)
    hip = _lcm("sd15", TINY_SD, solver_config=sc, device="cuda", lora=[(ad, 0.75)])
    assert not hip.guidance_embedded
    eng = OracleLCMMock(TINY_SD, merge_into_state_dict(synth_state_dict(TINY_SD, 0), [(ad, 0.75)], TINY_SD))
    ref = _lcm("sd15", TINY_SD, solver_config=sc, device="cpu", text_encoder=hip.text_encoder, engine=eng)
    pe = _embeds(hip, "sd15")
    a = _sample(hip, "sd15", pe, [21, 22], cfg_guidance=cfg_guidance)[0].clone()
    b = _sample(ref, "sd15", tuple(x.cpu() for x in pe), [21, 22], cfg_guidance=cfg_guidance)[0]
    steps = [v for n, v in eng.lcalls if n == "step_lcm"]
    assert len(steps) == 4 and all(s["single"] == (cfg_guidance <= 1.0) for s in steps)
    rel = rel_l2(a, b)
    print(f"LCM-LoRA cfg_guidance={cfg_guidance}: chain rel-L2 {rel:.3e}")
    assert torch.isfinite(a).all() and float(a.std()) > 0
    assert rel < 2 * CHAIN_MEASURED[("sd15", f"lora_{cfg_guidance}")], rel
    hip.set_lora([])
    assert rel_l2(_sample(hip, "sd15", pe, [21, 22], cfg_guidance=cfg_guidance)[0], a) > 1e-2       # the adapter matters


# ---------------------------------------------------------------------------------------------------- the plain engine is untouched
def test_plain_engine_runs_the_same_launches_and_bits_around_an_lcm_job():
    need_gpu()
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    mk = lambda: get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=5), device="cuda", unet_config=TINY_SD,  # noqa: E731
                            max_batch=2, latent_hw=(16, 16), scalar_semantics="cuda")
    s = mk()
    pe = s.get_text_embed("bad", ["a cat", "a dog"])
    run = lambda sv: [t.clone() for t in sv.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=[5, 6], return_latents=True)]  # noqa: E731
    before = run(s)
    z = torch.randn(2, 4, 16, 16).cuda()
    n0 = _launches(s.engine.unet, z)
    lcm = _lcm("sd15", TINY_SD, solver_config=types.SimpleNamespace(num_sampling=4), device="cuda", engine=s.engine,
               text_encoder=s.text_encoder)
    den, zt = lcm.sample(cfg_guidance=1.5, prompt_embeds=pe, seeds=[5, 6], return_latents=True)
    assert torch.isfinite(den).all()
    s._ctx_key = None                                                # the LCM job set the engine's context: the next job sets its own
    after = run(s)
    assert _launches(s.engine.unet, z) == n0
    fresh = run(mk())
    for x, y, w in zip(before, after, fresh):
        assert torch.equal(x, y) and torch.equal(x, w)


# ---------------------------------------------------------------------------------------------------- seeded ancestral noise
def test_euler_a_cfgpp_with_philox_noise():
    need_gpu()
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    mk = lambda **kw: get_solver("euler_a_cfg++", solver_config=types.SimpleNamespace(num_sampling=4), device="cuda", unet_config=TINY_SD,  # noqa: E731
                                 max_batch=3, latent_hw=(16, 16), scalar_semantics="cuda", **kw)
    s = mk(noise="philox")
    uc, c = s.get_text_embed("bad", ["a cat", "a dog", "a bird"])
    seeds = [31, 32, 33]
    run = lambda sv, pe, sd: [t.clone() for t in sv.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=sd, return_latents=True)]  # noqa: E731
    a = run(s, (uc, c), seeds)
    b = run(s, (uc, c), seeds)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.isfinite(a[1].float()).all()      # the same seeds: the same bits
    for k in range(3):           # chain k alone equals chain k in the batch of 3
        one = run(s, (uc, c[k:k + 1]), seeds[k:k + 1])
        assert torch.equal(one[0][0], a[0][k]) and torch.equal(one[1][0], a[1][k])
    # noise="torch" is the existing path: torch.randn_like, no Philox launch, and with the global generator reseeded the same bits
    calls = []
    t = mk()
    real = t.engine.philox_normal
    t.engine.philox_normal = lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1]
    torch.manual_seed(9)
    x = run(t, (uc, c), seeds)
    torch.manual_seed(9)
    y = run(t, (uc, c), seeds)
    assert calls == [] and t.noise == "torch" and all(torch.equal(p, q) for p, q in zip(x, y))
    assert not torch.equal(x[1], a[1])
