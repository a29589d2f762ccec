"""-m gpu: soft regional prompts through the UNet engine (include/cfgpp_regions_soft.h: cfgpp_unet_set_region_weights) against the fp32
CPU oracle of tests/region_soft_ref.py (oracle.unet_ref.UNetRef with the per-pixel blend in attn2) on synthetic weights, with the
per-forward bound of tests/test_gpu_unet.py (2.5e-3) and the project's chain bar (7.5e-3) - the bars of the hard path.  The nets are
the three of tests/region_ref.py at 16 x 16 (cross-attention head dims 64, 32, 40) and a two-level net whose head dims are 80 and 160
(dp = 96 and 160).  The region contexts differ loudly (region_ref.REGION_SCALE): regions swapped, the weights shifted by one pixel, the
level-0 weights used undownsampled each move the oracle by far more than the bar
(tests/test_regions_soft_cpu.py::test_weight_mistakes_are_loud_in_the_oracle)."""
import types

import pytest
import torch

import region_ref as RR
import region_soft_ref as SR
from test_gpu_unet import EPS_REL

pytestmark = pytest.mark.gpu
HW = RR.HW
CHAIN_BAR = 7.5e-3
_cache = {}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def setup(name):
    """per net, built once: (cfg, R, state dict, oracle, engine at max_tokens = 308 with region weights enabled, inputs)"""
    need_gpu()
    if name not in _cache:
        from cfgpp_amd.engine import HipUNet
        from cfgpp_amd.weights import synth_state_dict
        cfg, R = SR.configs()[name]
        sd = synth_state_dict(cfg, 0)
        net = HipUNet(cfg, max_rows=R, sample_hw=(HW, HW), max_tokens=308, soft_regions=True)
        net.load_state_dict(sd).finalize()
        z = RR.rnd(R // 2, 4, HW, HW, seed=60)
        te = ti = ack = None
        if cfg.addition_embed:
            te = RR.rnd(R, cfg.addition_pooled_dim, seed=62, scale=0.5)
            ti = torch.tensor([[HW * 8.0, HW * 8.0, 0, 0, HW * 8.0, HW * 8.0]] * R)
            ack = {"text_embeds": te, "time_ids": ti}
        _cache[name] = dict(cfg=cfg, R=R, sd=sd, ref=SR.SoftRegionUNetRef(cfg, sd), net=net, z=z, te=te, ti=ti, ack=ack)
    return _cache[name]


def forward(s, net, ehs, t, w=None):
    net.set_context(ehs, s["te"], s["ti"])
    net.set_region_weights(w)
    out = net.forward(s["z"].cuda(), t).float().cpu()
    torch.cuda.synchronize()
    return out


def oracle(s, ehs, t, w=None):
    s["ref"].set_region_weights(w)
    return s["ref"](torch.cat([s["z"]] * (s["R"] // s["z"].shape[0])), t, ehs, s["ack"])["sample"].float()


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("kind", ("feather", "mixed"))
@pytest.mark.parametrize("n", (2, 3, 4))
@pytest.mark.parametrize("name", SR.NETS)
def test_soft_forward_vs_oracle(name, n, kind):
    """feathered stripes and fully mixed weights of n regions, one map for every row, at t = 981 and t = 1"""
    s = setup(name)
    from test_gpu_configs import record
    w = SR.region_weights(kind, n)
    ehs = RR.region_context(s["R"], n, s["cfg"].cross_attention_dim)
    try:
        for t in (981.0, 1.0):
            got, want = forward(s, s["net"], ehs, t, w), oracle(s, ehs, t, w)
            r = rel(got, want)
            record("regions_soft_forward", cfg=name, regions=n, map=kind, t=t, rel_l2=r)
            print(f"{name} R={n} {kind} t {t}: rel-L2 {r:.3e}")
            assert bool(torch.isfinite(got).all()) and r < EPS_REL, (name, n, kind, t, r)
    finally:
        s["net"].set_region_weights(None)


@pytest.mark.parametrize("name", SR.NETS)
def test_weights_per_row(name):
    """map_rows = rows: every row its own weights (rolled by 3 pixels per row), and the same forward with one shared map differs"""
    s = setup(name)
    n = 3
    w = SR.region_weights("feather", n, rows=s["R"])
    ehs = RR.region_context(s["R"], n, s["cfg"].cross_attention_dim)
    try:
        got, want = forward(s, s["net"], ehs, 981.0, w), oracle(s, ehs, 981.0, w)
        shared = forward(s, s["net"], ehs, 981.0, w[:1])
    finally:
        s["net"].set_region_weights(None)
    assert rel(got, want) < EPS_REL, rel(got, want)
    assert rel(shared, want) > 10 * EPS_REL


@pytest.mark.parametrize("name", SR.NETS)
def test_one_hot_weights_against_the_hard_map_and_exclusivity(name):
    """one-hot weights run the soft kernel and land within the bar of the hard job (kernels 7 / 8) and of the oracle; setting one
    clears the other"""
    s = setup(name)
    n = 3
    ehs = RR.region_context(s["R"], n, s["cfg"].cross_attention_dim)
    net = s["net"]
    try:
        soft = forward(s, net, ehs, 981.0, SR.region_weights("onehot", n))
        assert net.soft_regions == n and " soft_regions=3" in net.profile(s["z"].cuda(), 981.0, detail=True)["detail"]
        net.set_regions(RR.region_ids("stripes", n), n)
        assert net.soft_regions == 0 and net.regions == n
        d = net.profile(s["z"].cuda(), 981.0, detail=True)["detail"]
        assert " regions=3" in d and "soft_regions" not in d
        hard = net.forward(s["z"].cuda(), 981.0).float().cpu()
        net.set_region_weights(SR.region_weights("onehot", n))
        assert net.regions == 0 and net.soft_regions == n
        again = net.forward(s["z"].cuda(), 981.0).float().cpu()
    finally:
        net.set_region_weights(None)
        net.set_regions(None)
    want = oracle(s, ehs, 981.0, SR.region_weights("onehot", n))
    print(f"{name}: soft vs hard {rel(soft, hard):.3e}, soft vs oracle {rel(soft, want):.3e}, hard vs oracle {rel(hard, want):.3e}")
    assert rel(soft, hard) < EPS_REL and rel(soft, want) < EPS_REL and torch.equal(soft, again)


@pytest.mark.parametrize("name", SR.NETS)
def test_base_ratio_one_is_the_plain_prompt_job(name):
    """beta = 1: region 0 alone - the plain 77-token forward of the base prompt on the same engine, within the bar"""
    s = setup(name)
    from cfgpp_amd.regions import build_region_weights
    n = 3
    ehs = RR.region_context(s["R"], n, s["cfg"].cross_attention_dim)
    w = build_region_weights([torch.rand(HW, HW), torch.rand(HW, HW)], (HW, HW), None, base_ratio=1.0)
    try:
        got = forward(s, s["net"], ehs, 981.0, w)
    finally:
        s["net"].set_region_weights(None)
    plain = forward(s, s["net"], ehs[:, :77].contiguous(), 981.0)
    assert rel(got, plain) < EPS_REL, rel(got, plain)
    assert rel(got, oracle(s, ehs[:, :77].contiguous(), 981.0)) < EPS_REL


def test_an_engine_without_the_switch_is_the_parents():
    """soft_regions=False: the byte count and the launch count of an engine that never heard of region weights; the switch costs
    exactly the per-level fp32 buffers, max_rows x 4 x q_tok_pad x 4 bytes"""
    s = setup("tiny_sd")
    from cfgpp_amd.engine import HipUNet
    cfg, R = s["cfg"], s["R"]
    base = HipUNet(cfg, max_rows=R, sample_hw=(HW, HW), max_tokens=308)
    base.load_state_dict(s["sd"]).finalize()
    q_pads, h = [], HW
    for lvl in range(cfg.num_levels):
        if cfg.level_has_attn[lvl] or lvl == cfg.num_levels - 1:
            q_pads.append((h * h + 127) // 128 * 128)
        if lvl != cfg.num_levels - 1:
            h //= 2
    assert s["net"].device_bytes() - base.device_bytes() == R * 4 * 4 * sum(q_pads)
    e77 = RR.rnd(R, 77, cfg.cross_attention_dim, seed=90, scale=0.5)
    launches = lambda p: sum(p[k]["launches"] for k in ("igemm", "attention", "norm", "small"))
    base.set_context(e77, s["te"], s["ti"])
    a = base.forward(s["z"].cuda(), 981.0).float().cpu()
    p_base = base.profile(s["z"].cuda(), 981.0, detail=True)
    b = forward(s, s["net"], e77, 981.0)
    p_off = s["net"].profile(s["z"].cuda(), 981.0, detail=True)
    n = 2
    on = forward(s, s["net"], RR.region_context(R, n, cfg.cross_attention_dim), 981.0, SR.region_weights("feather", n))
    p_on = s["net"].profile(s["z"].cuda(), 981.0, detail=True)
    s["net"].set_region_weights(None)
    assert torch.equal(a, b) and not torch.equal(a, on)
    assert launches(p_base) == launches(p_off) == launches(p_on)
    strip = lambda d: [ln.split("\t")[2] for ln in d.splitlines()]
    assert strip(p_off["detail"]) == strip(p_base["detail"]) and "soft_regions" not in p_base["detail"]


def test_refusals_name_what_they_refuse():
    s = setup("tiny_sd")
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.engine import HipUNet
    net, cfg, R = s["net"], s["cfg"], s["R"]
    w = SR.region_weights("feather", 3)
    try:
        forward(s, net, RR.region_context(R, 3, cfg.cross_attention_dim), 981.0, w)
        net.set_context(RR.region_context(R, 2, cfg.cross_attention_dim))
        with pytest.raises(CfgppError, match=r"n_regions=3 \(a context of 231 tokens\) but the context has tokens=154"):
            net.forward(s["z"].cuda(), 981.0)
        bad = w.clone(); bad[0, 1, 2, 5] = -0.25
        with pytest.raises(CfgppError, match=r"weight -0.25 at row 0, region 1, pixel \(2, 5\)"):
            net.set_region_weights(bad)
        bad = w.clone(); bad[0, 2, 3, 4] = float("nan")
        with pytest.raises(CfgppError, match=r"at row 0, region 2, pixel \(3, 4\)"):
            net.set_region_weights(bad)
        bad = w.clone(); bad[0, 0, 7, 9] += 0.01
        with pytest.raises(CfgppError, match=r"row 0, pixel \(7, 9\) sum to 1.01"):
            net.set_region_weights(bad)
        with pytest.raises(CfgppError, match=r"n_regions=5"):
            net.set_region_weights(torch.full((1, 5, HW, HW), 0.2))
        with pytest.raises(CfgppError, match=r"n_regions=1"):
            net.set_region_weights(torch.ones((1, 1, HW, HW)))
        with pytest.raises(CfgppError, match=r"map_rows=3"):
            net.set_region_weights(SR.region_weights("feather", 2, rows=3))
        with pytest.raises(CfgppError, match=r"expected a float \[1 or rows, R, 16, 16\]"):
            net.set_region_weights(torch.zeros(1, 2, 8, 8))
        assert net.soft_regions == 3                      # a refused call changes nothing
    finally:
        net.set_region_weights(None)
    plain = HipUNet(cfg, max_rows=R, sample_hw=(HW, HW), max_tokens=308)
    with pytest.raises(CfgppError, match=r"not finalized"):
        plain.set_region_weights(w)
    plain.load_state_dict(s["sd"]).finalize()
    with pytest.raises(CfgppError, match=r"not enabled for region weights \(cfgpp_unet_enable_region_weights before finalize\)"):
        plain.set_region_weights(w)
    with pytest.raises(CfgppError, match=r"after cfgpp_unet_finalize"):
        plain.enable_region_weights()
    with pytest.raises(CfgppError, match=r"max_tokens=77 \(regions need max_tokens > 77"):
        HipUNet(cfg, max_rows=R, sample_hw=(HW, HW), soft_regions=True)
    small = HipUNet(cfg, max_rows=R, sample_hw=(HW, HW), max_tokens=154, soft_regions=True)
    small.load_state_dict(s["sd"]).finalize()
    with pytest.raises(CfgppError, match=r"n_regions=3 needs max_tokens >= 231, the engine was built with max_tokens=154"):
        small.set_region_weights(w)
    from cfgpp_amd.hip_engine import HipEngine
    eng = HipEngine(cfg, max_batch=1, latent_hw=(HW, HW), max_tokens=154)
    with pytest.raises(CfgppError, match=r"built without soft_regions=True"):
        eng.set_region_weights(SR.region_weights("feather", 2))
    cn = HipEngine(cfg, max_batch=1, latent_hw=(HW, HW), max_tokens=154).build_controlnet("synthetic")
    with pytest.raises(CfgppError, match=r"ControlNet-mode engine"):
        from cfgpp_amd import _lib
        host = SR.region_weights("feather", 2).contiguous()
        _lib.check(_lib.load().cfgpp_unet_set_region_weights(cn._h, host.data_ptr(), 1, 2), "cfgpp_unet_set_region_weights")


# ---- chains: the solvers' soft path on the HIP engine against the same solver on a mock engine whose UNet is the oracle ---------
def _solver(name, net, **kw):
    cfg = SR.configs()[net][0]
    if cfg.addition_embed:
        from cfgpp_amd.latent_sdxl import get_solver
    else:
        from cfgpp_amd.latent_diffusion import get_solver
    return get_solver(name, unet_config=cfg, max_batch=2, latent_hw=(HW, HW), scalar_semantics="cuda", max_regions=3, soft_regions=True, **kw), cfg


@pytest.mark.parametrize("solver", ("ddim_cfg++", "ddim"))
@pytest.mark.parametrize("net", SR.NETS)
def test_three_step_chain_vs_mock_chain(net, solver):
    """every net of the forward tests, the head dims 80 / 160 included"""
    need_gpu()
    from cfgpp_amd.regions import soft_rect_mask
    from cfgpp_amd.weights import synth_state_dict
    sc = types.SimpleNamespace(num_sampling=3)
    model = "sdxl" if SR.configs()[net][0].addition_embed else "sd15"
    hip, cfg = _solver(solver, net, solver_config=sc, device="cuda")
    sd = synth_state_dict(cfg, 0)
    eng = SR.SoftRegionMockEngine(cfg, sd, (HW, HW))
    ref, _ = _solver(solver, net, solver_config=sc, device="cpu", text_encoder=hip.text_encoder, engine=eng)
    masks = [soft_rect_mask(0.5, 0.0, 1.0, 1.0, (HW, HW), 0.25), soft_rect_mask(0.25, 0.25, 0.75, 0.75, (HW, HW), 0.25)]
    kw = dict(cfg_guidance=0.6 if solver.endswith("++") else 5.0, seeds=[11, 12], return_latents=True,
              region_prompts=[["a snowy pine", "a birch"], "a red fox"], region_masks=masks, region_base_ratio=0.3,
              region_negative_prompts=[None, "blurry"])
    if model == "sd15":
        run = lambda s: s.sample(prompt=["bad", ["a meadow", "a lake"]], **kw)[0].clone().float().cpu()
    else:
        p = ["bad", ["a meadow", "a lake"]]
        run = lambda s: s.sample(prompt1=p, prompt2=p, target_size=(128, 128), original_size=(128, 128), **kw).clone().float().cpu()
    a, b = run(hip), run(ref)
    assert eng.weight_calls and eng.weight_calls[-1].shape[1] == 3
    r = rel(a, b)
    for k in ("region_prompts", "region_masks", "region_base_ratio", "region_negative_prompts"):
        kw.pop(k)
    plain = run(hip)
    print(f"{net} {solver}: soft regional chain rel-L2 {r:.3e}, vs the plain chain {rel(a, plain):.3e}")
    assert bool(torch.isfinite(a).all()) and r < CHAIN_BAR, r
    # the regions did something: the plain chain lies further from the soft chain than the oracle's chain does, by a clear factor
    # (30 % base prompt everywhere and feathered borders keep the two jobs closer than the hard partition of test_gpu_regions_net.py)
    assert rel(a, plain) > 3 * r and hip.engine.regions == 0


def test_graph_replay_refuses_region_weights(monkeypatch):
    need_gpu()
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.hip_engine import HipEngine
    from cfgpp_amd.unet_config import TINY_SD as cfg
    monkeypatch.setenv("CFGPP_GRAPH", "1")
    eng = HipEngine(cfg, max_batch=1, latent_hw=(HW, HW), max_tokens=154, soft_regions=True)
    ctx = RR.region_context(2, 2, cfg.cross_attention_dim).cuda().half()
    eng.set_context(ctx[:1], ctx[1:])
    assert eng.graph_enabled
    eng.set_region_weights(SR.region_weights("feather", 2))
    assert not eng.graph_enabled and eng.regions == 2
    z = RR.rnd(1, 4, HW, HW, seed=60).cuda()
    with pytest.raises(CfgppError, match=r"sample_graph: region weights are on .*n_regions=2"):
        eng.ddim_loop_graph(z, [(981.0, 0.1, 0.9, 0.9, 0.1)], 0.6, True, True)
    eng.set_regions(None)
    assert eng.graph_enabled and eng.regions == 0
