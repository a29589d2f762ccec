"""-m gpu: regional prompts through the UNet engine (include/cfgpp_regions.h: cfgpp_unet_set_regions) against the fp32 CPU oracle of
tests/region_ref.py (oracle.unet_ref.UNetRef with the per-pixel selection in attn2) on synthetic weights, with the per-forward bound
of tests/test_gpu_unet.py and the project's chain bar.  The nets are those of tests/test_gpu_long_prompt.py at 16 x 16: TINY_XL
(cross-attention head dim 64: kernel 7, fp32 denominator), TINY_SD (32: kernel 8) and the two-level 320-channel net (40: kernel 7
with the ones row of V^T).  The region contexts differ loudly (region_ref.REGION_SCALE): regions swapped, the map shifted by one
pixel, the level-0 map used undownsampled each move the oracle's output by 0.099 .. 0.42 rel-L2 - 40 times the bound and more
(tests/test_regions_cpu.py::test_map_mistakes_are_loud_in_the_oracle; profiles/regional/README.md)."""
import types

import pytest
import torch

import region_ref as RR
from test_gpu_unet import EPS_REL

pytestmark = pytest.mark.gpu
HW = RR.HW
CHAIN_BAR = 7.5e-3          # the project's chain bar (tests/test_gpu_pano_net.py)
_cache = {}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def setup(name):
    """per net, built once: (cfg, R, state dict, oracle, engine at max_tokens = 308, inputs)"""
    need_gpu()
    if name not in _cache:
        from cfgpp_amd.engine import HipUNet
        from cfgpp_amd.weights import synth_state_dict
        cfg, R = RR.configs()[name]
        sd = synth_state_dict(cfg, 0)
        net = HipUNet(cfg, max_rows=R, sample_hw=(HW, HW), max_tokens=308)
        net.load_state_dict(sd).finalize()
        z = RR.rnd(R // 2, 4, HW, HW, seed=60)
        te = ti = ack = None
        if cfg.addition_embed:
            te = RR.rnd(R, cfg.addition_pooled_dim, seed=62, scale=0.5)
            ti = torch.tensor([[HW * 8.0, HW * 8.0, 0, 0, HW * 8.0, HW * 8.0]] * R)
            ack = {"text_embeds": te, "time_ids": ti}
        _cache[name] = dict(cfg=cfg, R=R, sd=sd, ref=RR.RegionUNetRef(cfg, sd), net=net, z=z, te=te, ti=ti, ack=ack)
    return _cache[name]


def forward(s, net, ehs, t, ids=None, n=0):
    net.set_context(ehs, s["te"], s["ti"])
    net.set_regions(ids, n)
    out = net.forward(s["z"].cuda(), t).float().cpu()
    torch.cuda.synchronize()
    return out


def oracle(s, ehs, t, ids=None, n=0):
    s["ref"].set_regions(ids, n)
    return s["ref"](torch.cat([s["z"]] * (s["R"] // s["z"].shape[0])), t, ehs, s["ack"])["sample"].float()


def rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("kind", ("stripes", "checker"))
@pytest.mark.parametrize("n", (2, 3, 4))
@pytest.mark.parametrize("name", RR.NETS)
def test_regional_forward_vs_oracle(name, n, kind):
    """left / right stripes and a checkerboard of n regions, one map for every row, at t = 981 and t = 1"""
    s = setup(name)
    from test_gpu_configs import record
    ids = RR.region_ids(kind, n)
    ehs = RR.region_context(s["R"], n, s["cfg"].cross_attention_dim)
    try:
        for t in (981.0, 1.0):
            got, want = forward(s, s["net"], ehs, t, ids, n), oracle(s, ehs, t, ids, n)
            r = rel(got, want)
            record("regions_forward", cfg=name, regions=n, map=kind, t=t, rel_l2=r)
            print(f"{name} R={n} {kind} t {t}: rel-L2 {r:.3e}")
            assert bool(torch.isfinite(got).all()) and r < EPS_REL, (name, n, kind, t, r)
    finally:
        s["net"].set_regions(None)


@pytest.mark.parametrize("name", RR.NETS)
def test_a_map_per_row(name):
    """map_rows = rows: every row its own map (rolled by 3 pixels per row), and the same forward with one shared map differs"""
    s = setup(name)
    n = 3
    ids = RR.region_ids("checker", n, rows=s["R"])
    ehs = RR.region_context(s["R"], n, s["cfg"].cross_attention_dim)
    try:
        got, want = forward(s, s["net"], ehs, 981.0, ids, n), oracle(s, ehs, 981.0, ids, n)
        shared = forward(s, s["net"], ehs, 981.0, ids[:1], n)
    finally:
        s["net"].set_regions(None)
    assert rel(got, want) < EPS_REL, rel(got, want)
    assert rel(shared, want) > 10 * EPS_REL


@pytest.mark.parametrize("name", RR.NETS)
def test_identical_prompts_in_all_regions_are_the_plain_forward(name):
    s = setup(name)
    n = 4
    e77 = RR.rnd(s["R"], 77, s["cfg"].cross_attention_dim, seed=90, scale=0.5)
    try:
        got = forward(s, s["net"], e77.repeat(1, n, 1), 981.0, RR.region_ids("checker", n), n)
    finally:
        s["net"].set_regions(None)
    want = oracle(s, e77, 981.0)
    assert rel(got, want) < EPS_REL, rel(got, want)


@pytest.mark.parametrize("name", RR.NETS)
def test_off_after_on_is_the_plain_engine(name):
    """set_regions(None) after a regional forward: the bits of an engine that never had regions, the same launch count, the plain
    tags; while on, the cross-attention ops carry regions=R and the launch count is the same"""
    s = setup(name)
    from cfgpp_amd.engine import HipUNet
    base = HipUNet(s["cfg"], max_rows=s["R"], sample_hw=(HW, HW), max_tokens=308)
    base.load_state_dict(s["sd"]).finalize()
    e77 = RR.rnd(s["R"], 77, s["cfg"].cross_attention_dim, seed=90, scale=0.5)
    want = forward(s, base, e77, 981.0)
    launches = lambda p: sum(p[k]["launches"] for k in ("igemm", "attention", "norm", "small"))
    p_base = base.profile(s["z"].cuda(), 981.0, detail=True)
    n = 2
    ehs = RR.region_context(s["R"], n, s["cfg"].cross_attention_dim)
    on = forward(s, s["net"], ehs, 981.0, RR.region_ids("stripes", n), n)
    p_on = s["net"].profile(s["z"].cuda(), 981.0, detail=True)
    off = forward(s, s["net"], e77, 981.0)
    p_off = s["net"].profile(s["z"].cuda(), 981.0, detail=True)
    assert torch.equal(want, off) and not torch.equal(want, on)
    assert launches(p_base) == launches(p_on) == launches(p_off)
    assert " regions=2" in p_on["detail"] and "regions=" not in p_off["detail"] and "regions=" not in p_base["detail"]
    strip = lambda d: [ln.split("\t")[2] for ln in d.splitlines()]
    assert strip(p_off["detail"]) == strip(p_base["detail"])


def test_refusals_name_what_they_refuse():
    s = setup("tiny_sd")
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.engine import HipUNet
    net, cfg, R = s["net"], s["cfg"], s["R"]
    ids = RR.region_ids("stripes", 3)
    try:
        forward(s, net, RR.region_context(R, 3, cfg.cross_attention_dim), 981.0, ids, 3)
        net.set_context(RR.region_context(R, 2, cfg.cross_attention_dim))
        with pytest.raises(CfgppError, match=r"n_regions=3 \(a context of 231 tokens\) but the context has tokens=154"):
            net.forward(s["z"].cuda(), 981.0)
        with pytest.raises(CfgppError, match=r"region id 2 .*n_regions=2"):
            net.set_regions(ids, 2)
        with pytest.raises(CfgppError, match=r"n_regions=5"):
            net.set_regions(ids, 5)
        with pytest.raises(CfgppError, match=r"map_rows=3"):
            net.set_regions(RR.region_ids("stripes", 2, rows=3), 2)
        with pytest.raises(CfgppError, match=r"expected \[1 or rows, 16, 16\]"):
            net.set_regions(torch.zeros(1, 8, 8, dtype=torch.long), 2)
    finally:
        net.set_regions(None)
    small = HipUNet(cfg, max_rows=R, sample_hw=(HW, HW), max_tokens=154)
    with pytest.raises(CfgppError, match=r"not finalized"):
        small.set_regions(ids, 3)
    small.load_state_dict(s["sd"]).finalize()
    with pytest.raises(CfgppError, match=r"n_regions=3 needs max_tokens >= 231, the engine was built with max_tokens=154"):
        small.set_regions(ids, 3)
    from cfgpp_amd.hip_engine import HipEngine
    eng = HipEngine(cfg, max_batch=1, latent_hw=(HW, HW))
    eng.set_ip_adapter("synthetic")
    with pytest.raises(CfgppError, match=r"IP-Adapter is loaded"):
        eng.unet.set_regions(RR.region_ids("stripes", 2), 2)
    cn = HipEngine(cfg, max_batch=1, latent_hw=(HW, HW), max_tokens=154).build_controlnet("synthetic")
    with pytest.raises(CfgppError, match=r"ControlNet-mode engine"):
        from cfgpp_amd import _lib
        host = RR.region_ids("stripes", 2).to(torch.uint8).contiguous()
        _lib.check(_lib.load().cfgpp_unet_set_regions(cn._h, host.data_ptr(), 1, 2), "cfgpp_unet_set_regions")


def test_device_bytes_count_the_map_buffers():
    """an engine with max_tokens > 77 owns the per-level map buffers (rows x q_tok_pad bytes each): the step 77 -> 154 costs them
    on top of the 64 key slots per block that the step 154 -> 231 costs alone"""
    need_gpu()
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.unet_config import TINY_SD as cfg
    R = 4
    b = {}
    for mt in (77, 154, 231):
        net = HipUNet(cfg, max_rows=R, sample_hw=(HW, HW), max_tokens=mt)
        net.load_state_dict(setup("tiny_sd")["sd"]).finalize()
        b[mt] = net.device_bytes()
        del net
    q_pads, h = [], HW
    for lvl in range(cfg.num_levels):
        if cfg.level_has_attn[lvl] or lvl == cfg.num_levels - 1:
            q_pads.append((h * h + 127) // 128 * 128)
        if lvl != cfg.num_levels - 1:
            h //= 2
    assert (b[154] - b[77]) - (b[231] - b[154]) == R * sum(q_pads)


# ---- chains: the solvers' region path on the HIP engine against the same solver on a mock engine whose UNet is the oracle ---------
def _solver(name, model, **kw):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    if model == "sd15":
        from cfgpp_amd.latent_diffusion import get_solver
        cfg = TINY_SD
    else:
        from cfgpp_amd.latent_sdxl import get_solver
        cfg = TINY_XL
    return get_solver(name, unet_config=cfg, max_batch=2, latent_hw=(HW, HW), scalar_semantics="cuda", max_regions=3, **kw), cfg


@pytest.mark.parametrize("solver", ("ddim_cfg++", "ddim"))
@pytest.mark.parametrize("model", ("sd15", "sdxl"))
def test_three_step_chain_vs_mock_chain(model, solver):
    need_gpu()
    from cfgpp_amd.regions import rect_mask
    from cfgpp_amd.weights import synth_state_dict
    from mock_region_engine import RegionMockEngine
    sc = types.SimpleNamespace(num_sampling=3)
    hip, cfg = _solver(solver, model, solver_config=sc, device="cuda")
    sd = synth_state_dict(cfg, 0)
    eng = RegionMockEngine(cfg, sd, (HW, HW))
    ref, _ = _solver(solver, model, solver_config=sc, device="cpu", text_encoder=hip.text_encoder, engine=eng)
    masks = [rect_mask(0.5, 0.0, 1.0, 1.0, (HW, HW)), rect_mask(0.25, 0.25, 0.75, 0.75, (HW, HW))]
    kw = dict(cfg_guidance=0.6 if solver.endswith("++") else 5.0, seeds=[11, 12], return_latents=True,
              region_prompts=[["a snowy pine", "a birch"], "a red fox"], region_masks=masks)
    if model == "sd15":
        run = lambda s: s.sample(prompt=["bad", ["a meadow", "a lake"]], **kw)[0].clone().float().cpu()
    else:
        p = ["bad", ["a meadow", "a lake"]]
        run = lambda s: s.sample(prompt1=p, prompt2=p, target_size=(128, 128), original_size=(128, 128), **kw).clone().float().cpu()
    a, b = run(hip), run(ref)
    assert eng.region_calls and eng.region_calls[-1][1] == 3
    r = rel(a, b)
    kw.pop("region_prompts"), kw.pop("region_masks")
    plain = run(hip)
    print(f"{model} {solver}: regional chain rel-L2 {r:.3e}, vs the plain chain {rel(a, plain):.3e}")
    assert bool(torch.isfinite(a).all()) and r < CHAIN_BAR, r
    assert rel(a, plain) > CHAIN_BAR and hip.engine.regions == 0


def test_graph_replay_refuses_regions(monkeypatch):
    """a region-masked step is not captured: the engine reports no graph replay while regions are on (the solvers' loops then run
    eagerly), and cfgpp_sample_graph_ddim itself refuses by name"""
    need_gpu()
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.hip_engine import HipEngine
    from cfgpp_amd.unet_config import TINY_SD as cfg
    monkeypatch.setenv("CFGPP_GRAPH", "1")
    eng = HipEngine(cfg, max_batch=1, latent_hw=(HW, HW), max_tokens=154)
    ctx = RR.region_context(2, 2, cfg.cross_attention_dim).cuda().half()
    eng.set_context(ctx[:1], ctx[1:])
    assert eng.graph_enabled
    eng.set_regions(RR.region_ids("stripes", 2), 2)
    assert not eng.graph_enabled and eng.regions == 2
    z = RR.rnd(1, 4, HW, HW, seed=60).cuda()
    with pytest.raises(CfgppError, match=r"sample_graph: regional prompts are on .*n_regions=2"):
        eng.ddim_loop_graph(z, [(981.0, 0.1, 0.9, 0.9, 0.1)], 0.6, True, True)
    eng.set_regions(None)
    assert eng.graph_enabled and eng.regions == 0
