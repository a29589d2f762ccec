"""-m gpu: text contexts of 154 .. 308 tokens through the UNet engine (include/cfgpp_long_prompt.h: cfgpp_unet_set_max_tokens) against the fp32
CPU oracle (oracle/unet_ref.py takes any token count) on synthetic weights, with the per-forward bound of tests/test_gpu_unet.py.
Three nets: TINY_XL (cross-attention head dim 64: xattn64_long_kernel, fp32 denominator), TINY_SD (32: attn_kernel) and a
two-level 320-channel, 8-head net (40: xattn64_long_kernel with the ones row of V^T).  The oracle comparison runs twice: with the
default dispatch (the kernel for the classes it measured faster in: head dim 40 at 154 and 308 tokens, 64 at 154) and with
cfgpp_attention_set_cross_long(2), under which head dims 40 and 64 take it at every token count."""
import types

import pytest
import torch

from test_gpu_unet import EPS_REL

pytestmark = pytest.mark.gpu
HW = 16


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def configs():
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL, UNetConfig
    d40 = UNetConfig(name="tiny_d40", block_out_channels=(320, 320), level_has_attn=(1, 1), transformer_depth=(1, 1), num_heads=(8, 8),
                     cross_attention_dim=64, sample_size=16)
    return {"tiny_xl": (TINY_XL, 2), "tiny_sd": (TINY_SD, 4), "tiny_d40": (d40, 2)}


NETS = ("tiny_xl", "tiny_sd", "tiny_d40")
_cache = {}


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).half().float()


def setup(name):
    """per net, built once: (cfg, R, state dict, oracle, engine at max_tokens = 308, inputs)"""
    need_gpu()
    if name not in _cache:
        from cfgpp_amd.engine import HipUNet
        from cfgpp_amd.weights import synth_state_dict
        from oracle.unet_ref import UNetRef
        cfg, R = configs()[name]
        sd = synth_state_dict(cfg, 0)
        net = HipUNet(cfg, max_rows=R, sample_hw=(HW, HW), max_tokens=308)
        net.load_state_dict(sd).finalize()
        z = rnd(R // 2, 4, HW, HW, seed=60)
        ehs = rnd(R, 308, cfg.cross_attention_dim, seed=61, scale=0.5)
        te = ti = ack = None
        if cfg.addition_embed:
            te = rnd(R, cfg.addition_pooled_dim, seed=62, scale=0.5)
            ti = torch.tensor([[HW * 8.0, HW * 8.0, 0, 0, HW * 8.0, HW * 8.0]] * R)
            ack = {"text_embeds": te, "time_ids": ti}
        _cache[name] = dict(cfg=cfg, R=R, sd=sd, ref=UNetRef(cfg, sd), net=net, z=z, ehs=ehs, te=te, ti=ti, ack=ack)
    return _cache[name]


def forward(s, net, ehs, t):
    net.set_context(ehs, s["te"], s["ti"])
    out = net.forward(s["z"].cuda(), t).float().cpu()
    torch.cuda.synchronize()
    return out


def oracle(s, ehs, t):
    return s["ref"](torch.cat([s["z"], s["z"]]), t, ehs, s["ack"])["sample"].float()


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def cross_attention_records(s, tokens):
    """what the cross-attention op dispatches at this net's head dims (the same call the plan makes), on scratch buffers"""
    import hip_ops as H
    cfg = s["cfg"]
    out = set()
    for lvl in range(cfg.num_levels):
        if not cfg.level_has_attn[lvl]:
            continue
        h = cfg.num_heads[lvl]
        d = cfg.block_out_channels[lvl] // h
        dp = H.round_up(d, 32)
        q = torch.zeros((h, 128, dp), dtype=torch.float16, device=H.DEV)
        k = torch.zeros((h, 320, dp), dtype=torch.float16, device=H.DEV)
        vt = torch.zeros((h, dp, 320), dtype=torch.float16, device=H.DEV)
        H.check(H.lib().cfgpp_op_attention_prepare_vt(H.P(vt), h, d, 320, H.stream()), "prepare_vt")
        o = torch.empty((1, 16, h * d), dtype=torch.float16, device=H.DEV)
        H.check(H.lib().cfgpp_op_attention_cross(H.P(q), H.P(k), H.P(vt), H.P(o), 1, h, d, 16, tokens, 128, 320, H.stream()), "attention_cross")
        out.add(H.attention_last_launch()[0])
    torch.cuda.synchronize()
    return out


# kernel record of the cross-attention op per (net, tokens) under cfgpp_attention_set_cross_long(mode)
RECORDS = {1: {("tiny_xl", 154): {6}, ("tiny_xl", 308): {2}, ("tiny_sd", 154): {1}, ("tiny_sd", 308): {1}, ("tiny_d40", 154): {6}, ("tiny_d40", 308): {6}},
           2: {("tiny_xl", 154): {6}, ("tiny_xl", 308): {6}, ("tiny_sd", 154): {1}, ("tiny_sd", 308): {1}, ("tiny_d40", 154): {6}, ("tiny_d40", 308): {6}}}


@pytest.fixture
def cross_long_mode(request):
    import hip_ops as H
    if torch.cuda.is_available():
        H.lib().cfgpp_attention_set_cross_long(request.param)
    try:
        yield request.param
    finally:
        if torch.cuda.is_available():
            H.lib().cfgpp_attention_set_cross_long(1)


@pytest.mark.parametrize("cross_long_mode", (1, 2), indirect=True, ids=("default", "whole-scope"))
@pytest.mark.parametrize("name", NETS)
def test_long_contexts_vs_oracle(name, cross_long_mode):
    """154 and 308 tokens on an engine built for 308, at t = 981 and t = 1"""
    s = setup(name)
    from test_gpu_configs import record
    for tokens in (154, 308):
        assert cross_attention_records(s, tokens) == RECORDS[cross_long_mode][(name, tokens)]
        ehs = s["ehs"][:, :tokens].contiguous()
        for t in (981.0, 1.0):
            got, want = forward(s, s["net"], ehs, t), oracle(s, ehs, t)
            r = rel(got, want)
            record("long_prompt_forward", cfg=name, cross_long=cross_long_mode, tokens=tokens, t=t, rel_l2=r)
            print(f"{name} tokens {tokens} t {t}: rel-L2 {r:.3e}")
            assert bool(torch.isfinite(got).all()) and r < EPS_REL, (name, tokens, t, r)


@pytest.mark.parametrize("name", NETS)
def test_77_tokens_after_308_are_the_default_engines_bits(name):
    s = setup(name)
    from cfgpp_amd.engine import HipUNet
    base = HipUNet(s["cfg"], max_rows=s["R"], sample_hw=(HW, HW))
    base.load_state_dict(s["sd"]).finalize()
    assert s["net"].device_bytes() > base.device_bytes()           # the longer buffers are counted
    e77 = s["ehs"][:, :77].contiguous()
    for t in (981.0, 1.0):
        want = forward(s, base, e77, t)
        fresh = forward(s, s["net"], e77, t)
        forward(s, s["net"], s["ehs"], t)                          # 308 tokens: slots [77, 320) now hold their K / V^T
        again = forward(s, s["net"], e77, t)
        assert torch.equal(want, fresh) and torch.equal(want, again), (name, t)
    assert base.flops(s["R"]) == s["net"].flops(s["R"])            # at 77 tokens the figures are unchanged
    s["net"].set_context(s["ehs"], s["te"], s["ti"])
    assert s["net"].flops(s["R"]) > base.flops(s["R"])


@pytest.mark.parametrize("name", NETS)
def test_a_late_token_reaches_the_output(name):
    """two 308-token contexts that differ in token 300 only: both match the oracle, and they differ by more than the bound.  The
    other token is drawn four times as wide as the rest (scale 2.0 against 0.5): in the fp32 oracle a token of the others' width
    moves the output by rel-L2 0.8e-3 .. 1.2e-3, less than the bound, this one by 3.7e-2 .. 5.2e-2 on the three nets."""
    s = setup(name)
    a = s["ehs"].clone()
    b = a.clone()
    b[:, 300] = rnd(s["R"], s["cfg"].cross_attention_dim, seed=63, scale=2.0)
    t = 981.0
    ga, gb = forward(s, s["net"], a, t), forward(s, s["net"], b, t)
    ra, rb = oracle(s, a, t), oracle(s, b, t)
    moved = rel(gb, ga)
    print(f"{name}: token 300 moves the output by rel-L2 {moved:.3e}; vs oracle {rel(ga, ra):.3e} / {rel(gb, rb):.3e}")
    assert rel(ga, ra) < EPS_REL and rel(gb, rb) < EPS_REL
    assert moved > EPS_REL and rel(rb, ra) > EPS_REL


@pytest.mark.parametrize("name", NETS)
def test_graph_replay_at_154_tokens_is_the_eager_loop(monkeypatch, name):
    need_gpu()
    cfg, _ = configs()[name]
    mod = __import__("cfgpp_amd.latent_sdxl" if cfg.addition_embed else "cfgpp_amd.latent_diffusion", fromlist=["get_solver"])
    sol = mod.get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=6), device="cuda", unet_config=cfg, max_batch=2,
                         latent_hw=(HW, HW), max_prompt_chunks=2)
    long = "a (castle:1.3) on a hill, " + " ".join(f"detail{i}" for i in range(80))
    if cfg.addition_embed:
        emb = sol.get_text_embed("", [long, "a [dog]"], "", [long, "a [dog]"])
        assert emb[0].shape[1] == emb[1].shape[1] == 154
        kw = dict(prompt_embeds=emb, cfg_guidance=0.6)
    else:
        uc, c = sol.get_text_embed("", [long, "a [dog]"])
        assert uc.shape[1] == c.shape[1] == 154
        kw = dict(prompt_embeds=(uc, c), cfg_guidance=0.6)

    def run():
        out = sol.sample(seeds=[5, 6], return_latents=True, **kw)
        return [t.clone() for t in (out if isinstance(out, (tuple, list)) else [out])]
    monkeypatch.setenv("CFGPP_GRAPH", "0")
    eager = run()
    monkeypatch.setenv("CFGPP_GRAPH", "1")
    graph, again = run(), run()
    assert bool(torch.isfinite(eager[0]).all())
    for other in (graph, again):
        assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(eager, other))


@pytest.mark.parametrize("first", (154, 77))
@pytest.mark.parametrize("name", NETS)
def test_graph_replay_follows_the_token_count(monkeypatch, name, first):
    """one solver, one set of graph buffers: a loop at 154 tokens, then one at 77 (or the reverse), then the first again.  The
    captured cross-attention launches bake in the key count, the kernel and its LDS size, so each token count needs its own
    graph: every replay must equal the eager loop of the same context bit for bit."""
    need_gpu()
    cfg, _ = configs()[name]
    mod = __import__("cfgpp_amd.latent_sdxl" if cfg.addition_embed else "cfgpp_amd.latent_diffusion", fromlist=["get_solver"])
    sol = mod.get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=4), device="cuda", unet_config=cfg, max_batch=2,
                         latent_hw=(HW, HW), max_prompt_chunks=2)
    prompts = {154: ["a (castle:1.3), " + " ".join(f"detail{i}" for i in range(80)), "a [dog]"], 77: ["a castle", "a (dog:1.2)"]}
    embeds = {}
    for tokens, p in prompts.items():
        e = sol.get_text_embed("", p, "", p) if cfg.addition_embed else sol.get_text_embed("", p)
        assert e[0].shape[1] == e[1].shape[1] == tokens
        embeds[tokens] = e

    def run(tokens):
        out = sol.sample(seeds=[5, 6], return_latents=True, prompt_embeds=embeds[tokens], cfg_guidance=0.6)
        return [t.clone() for t in (out if isinstance(out, (tuple, list)) else [out])]
    monkeypatch.setenv("CFGPP_GRAPH", "0")
    eager = {tokens: run(tokens) for tokens in (154, 77)}
    assert not all(torch.equal(x, y) for x, y in zip(eager[154], eager[77]))
    monkeypatch.setenv("CFGPP_GRAPH", "1")
    second = 231 - first
    for tokens in (first, second, first, second):
        got = run(tokens)
        assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(eager[tokens], got)), (name, tokens)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_what_they_refuse():
    s = setup("tiny_sd")
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.latent_diffusion import get_solver
    base = HipUNet(s["cfg"], max_rows=s["R"], sample_hw=(HW, HW))
    base.load_state_dict(s["sd"]).finalize()
    with pytest.raises(CfgppError, match=r"tokens=154 .*max_tokens=77"):
        base.set_context(s["ehs"][:, :154].contiguous())
    with pytest.raises(CfgppError, match=r"tokens=100 .*max_tokens=308"):
        s["net"].set_context(s["ehs"][:, :100].contiguous())
    with pytest.raises(CfgppError, match=r"set_max_tokens: max_tokens=154 after cfgpp_unet_finalize"):
        base.set_max_tokens(154)
    fresh = HipUNet(s["cfg"], max_rows=s["R"], sample_hw=(HW, HW))
    with pytest.raises(CfgppError, match=r"max_tokens=200 \(77, 154, 231 or 308\)"):
        fresh.set_max_tokens(200)
    with pytest.raises(ValueError, match=r"ip_adapter=... together with max_prompt_chunks=2"):
        get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=2), device="cuda", unet_config=s["cfg"], max_batch=1,
                   ip_adapter="synthetic", max_prompt_chunks=2)
    from cfgpp_amd.hip_engine import HipEngine
    eng = HipEngine(s["cfg"], max_batch=1, latent_hw=(HW, HW), max_tokens=154)
    with pytest.raises(CfgppError, match=r"IP-Adapter on an engine with max_tokens=154"):
        eng.set_ip_adapter("synthetic")
    with pytest.raises(CfgppError, match=r"ip_load: IP-Adapter on an engine with max_tokens=308"):
        s["net"].ip_load("image_proj.proj.weight", torch.zeros(4, 4))


def test_controlnet_takes_the_same_max_tokens():
    """HipEngine hands its max_tokens to the ControlNet it builds: a controlled forward at 154 tokens runs, a default ControlNet refuses"""
    need_gpu()
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.controlnet import build_controlnet
    from cfgpp_amd.hip_engine import HipEngine
    from cfgpp_amd.unet_config import TINY_SD as cfg
    eng = HipEngine(cfg, max_batch=1, latent_hw=(HW, HW), max_tokens=154)
    cn = eng.build_controlnet("synthetic")
    assert cn.max_tokens == 154
    uc, c = rnd(1, 154, cfg.cross_attention_dim, seed=70, scale=0.5).cuda().half(), rnd(1, 154, cfg.cross_attention_dim, seed=71, scale=0.5).cuda().half()
    z = rnd(1, 4, HW, HW, seed=72).cuda()
    eng.set_context(uc, c)
    plain = torch.cat(eng.predict(z, 500.0)).clone()
    eng.set_control(cn, torch.rand(1, 3, HW * 8, HW * 8, generator=torch.Generator().manual_seed(1)), 1.0)
    ctl = torch.cat(eng.predict(z, 500.0)).clone()
    eng.clear_control()
    assert bool(torch.isfinite(ctl).all()) and torch.equal(torch.cat(eng.predict(z, 500.0)), plain)
    small = build_controlnet("synthetic", cfg, 2, (HW, HW), eng.device.index)
    with pytest.raises(CfgppError, match=r"tokens=154 .*max_tokens=77"):
        small.set_context(torch.cat([uc, c]))
