"""-m gpu: IP-Adapter image prompts through the C ABI (include/cfgpp_ip_adapter.h: cfgpp_unet_ip_load, cfgpp_unet_image_context) and the
solvers, on the tiny nets: TINY_SD (head dim 32: text pass + image pass) and TINY_XL (head dim 64: the fused one-launch kernel),
against tests/ip_adapter_ref.py (oracle.unet_ref.UNetRef with diffusers' decoupled cross-attention).

EPS_REL is the project's UNet tolerance (tests/test_gpu_unet.py).  Every comparison with the adapter also asserts that the oracle
with and without it differ by more than 10 x EPS_REL: an engine that ignored the adapter would fail."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS_REL = 2.5e-3
HW = 16


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _cfg(name):
    from cfgpp_amd.unet_config import CONFIGS
    return CONFIGS[name]


def _inputs(cfg, rows, seed=0, embed_dim=None):
    g = torch.Generator().manual_seed(100 + seed)
    zr = rows // 2
    z = (torch.randn(zr, 4, HW, HW, generator=g) * 0.8).half().float()
    ehs = torch.randn(rows, 77, cfg.cross_attention_dim, generator=g).half().float()
    te = ti = None
    if cfg.addition_embed:
        te = torch.randn(rows, cfg.addition_pooled_dim, generator=g).half().float()
        ti = torch.tensor([[HW * 8, HW * 8, 0, 0, HW * 8, HW * 8]] * rows, dtype=torch.float32)
    emb = None
    if embed_dim:
        emb = torch.randn(rows, embed_dim, generator=g).half().float()
        emb[:zr] = 0                                   # the default negative embeds
    return z, ehs, te, ti, emb


_STATE = {}


def _nets(name, n_img):
    """(cfg, sd, parsed adapter, oracle) per (net, n_img), built once"""
    key = (name, n_img)
    if key not in _STATE:
        from cfgpp_amd.ip_adapter import parse_ip_adapter, synthetic_ip_adapter
        from cfgpp_amd.weights import synth_state_dict
        from ip_adapter_ref import IPUNetRef
        cfg = _cfg(name)
        sd = synth_state_dict(cfg, 0)
        ad = parse_ip_adapter(synthetic_ip_adapter(cfg, n_img=n_img, seed=3 + n_img), cfg)
        _STATE[key] = (cfg, sd, ad, IPUNetRef(cfg, sd, ad))
    return _STATE[key]


def _engine(cfg, sd, max_rows=4):
    from cfgpp_amd.engine import HipUNet
    return HipUNet(cfg, max_rows=max_rows, sample_hw=(HW, HW)).load_state_dict(sd).finalize()


def _load(u, ad):
    for k, v in ad.items():
        u.ip_load(k, v)


def _oracle(net, z, t, ehs, te, ti, emb, scale):
    net.set_image(emb, scale)
    zz = torch.cat([z, z], 0)
    kw = dict(text_embeds=te, time_ids=ti) if te is not None else None
    return net(zz, t, ehs, kw)["sample"]


def _descriptions(prof):
    """(family, description, GFLOP) of every launch of a cfgpp_unet_profile detail text"""
    return [tuple(ln.split("\t")[i] for i in (1, 2, 4)) for ln in prof["detail"].splitlines()]


def _fwd(u, z, t, ehs, te, ti):
    u.set_context(ehs, te, ti)
    return u.forward(z.cuda(), t)


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl"])
@pytest.mark.parametrize("n_img", [4, 16])
@pytest.mark.parametrize("rows", [2, 4])
def test_forward_vs_oracle(name, n_img, rows):
    from test_gpu_configs import record
    cfg, sd, ad, net = _nets(name, n_img)
    z, ehs, te, ti, emb = _inputs(cfg, rows, seed=rows + n_img, embed_dim=ad.embed_dim)
    u = _engine(cfg, sd)
    _load(u, ad)
    u.set_context(ehs, te, ti)
    u.set_image_context(emb, 0.7)
    got = u.forward(z.cuda(), 321.0).float().cpu()
    ref = _oracle(net, z, 321.0, ehs, te, ti, emb, 0.7)
    plain = _oracle(net, z, 321.0, ehs, te, ti, None, 0.0)
    moved, rel = rel_l2(ref, plain), rel_l2(got, ref)
    record("ip_adapter_forward", net=name, n_img=n_img, rows=rows, rel_l2=rel, adapter_moves=moved)
    print(f"{name} n_img={n_img} rows={rows}: rel-L2 {rel:.3e}, oracle with vs without the adapter {moved:.3e}")
    assert moved > 10 * EPS_REL, f"the adapter moves the oracle by only {moved:.3e}"
    assert torch.isfinite(got).all() and rel < EPS_REL, f"{name}: rel-L2 {rel:.3e}"


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl"])
def test_engine_state_transitions(name):
    """on ONE engine: scale 0 / NULL embeds / ip_load(NULL) are the plain engine bit for bit; n_img 16 then 4 leaves no stale
    keys; a new text context keeps the image branch; launch count and device bytes"""
    cfg, sd, ad4, net4 = _nets(name, 4)
    _, _, ad16, net16 = _nets(name, 16)
    rows = 4
    z, ehs, te, ti, emb = _inputs(cfg, rows, seed=7, embed_dim=ad4.embed_dim)
    fresh = _fwd(_engine(cfg, sd), z, 500.0, ehs, te, ti).clone()
    u = _engine(cfg, sd)
    bytes0 = u.device_bytes()
    assert torch.equal(_fwd(u, z, 500.0, ehs, te, ti), fresh)
    launches0 = sum(v["launches"] for v in u.profile(z.cuda(), 500.0).values())
    detail0 = _descriptions(u.profile(z.cuda(), 500.0, detail=True))
    _load(u, ad16)
    bytes16 = u.device_bytes()
    assert bytes16 > bytes0
    u.set_image_context(emb, 1.0)
    got16 = u.forward(z.cuda(), 500.0).float().cpu()
    assert rel_l2(got16, _oracle(net16, z, 500.0, ehs, te, ti, emb, 1.0)) < EPS_REL
    prof = u.profile(z.cuda(), 500.0)
    launches_ip = sum(v["launches"] for v in prof.values())
    if name == "tiny_xl":           # head dim 64: the image branch rides in the text attention's launch
        assert launches_ip == launches0, (launches_ip, launches0)
    # scale 0 and NULL embeds: the plain engine, bit for bit
    u.set_image_context(emb, 0.0)
    assert torch.equal(u.forward(z.cuda(), 500.0), fresh)
    u.set_image_context(emb, 1.0)
    u.set_image_context(None)
    assert torch.equal(u.forward(z.cuda(), 500.0), fresh)
    assert _descriptions(u.profile(z.cuda(), 500.0, detail=True)) == detail0
    # n_img 16 -> 4 on the same engine, every tensor replaced in place (no drop in between, so the only clear of slots 100 .. 111
    # is the one inside cfgpp_unet_image_context; the op itself: tests/test_gpu_attention_ip.py)
    _load(u, ad4)
    assert bytes0 < u.device_bytes() < bytes16
    u.set_image_context(emb, 1.0)
    got4 = u.forward(z.cuda(), 500.0).float().cpu()
    ref4 = _oracle(net4, z, 500.0, ehs, te, ti, emb, 1.0)
    assert rel_l2(got4, ref4) < EPS_REL, rel_l2(got4, ref4)
    assert rel_l2(ref4, _oracle(net16, z, 500.0, ehs, te, ti, emb, 1.0)) > 10 * EPS_REL
    # a new scale alone, then a new text context: the image branch stays
    u.set_image_context(emb, 0.4)
    assert rel_l2(u.forward(z.cuda(), 500.0), _oracle(net4, z, 500.0, ehs, te, ti, emb, 0.4)) < EPS_REL
    ehs2 = torch.randn(ehs.shape, generator=torch.Generator().manual_seed(9)).half().float()
    got = _fwd(u, z, 500.0, ehs2, te, ti).float().cpu()
    ref = _oracle(net4, z, 500.0, ehs2, te, ti, emb, 0.4)
    assert rel_l2(got, ref) < EPS_REL, rel_l2(got, ref)
    assert rel_l2(ref, _oracle(net4, z, 500.0, ehs2, te, ti, None, 0.0)) > 10 * EPS_REL
    # drop: the plain engine again
    u.ip_load(None)
    assert u.device_bytes() == bytes0
    assert torch.equal(_fwd(u, z, 500.0, ehs, te, ti), fresh)


def test_load_refusals_name_the_key():
    from cfgpp_amd._lib import CfgppError
    cfg, sd, ad, _ = _nets("tiny_sd", 4)
    u = _engine(cfg, sd)
    b0 = u.device_bytes()
    with pytest.raises(CfgppError, match="unknown key nope.attn2.to_k_ip.weight"):
        u.ip_load("nope.attn2.to_k_ip.weight", torch.zeros(64, 64))
    k = "down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k_ip.weight"
    with pytest.raises(CfgppError, match=k.replace(".", r"\.")):
        u.ip_load(k, torch.zeros(64, 32))
    with pytest.raises(CfgppError, match=r"image_proj\.proj\.weight"):
        u.ip_load("image_proj.proj.weight", torch.zeros(33 * 64, 64))       # 33 image tokens
    assert u.device_bytes() == b0
    z, ehs, te, ti, emb = _inputs(cfg, 4, embed_dim=ad.embed_dim)
    u.set_context(ehs, te, ti)
    u.ip_load("image_proj.proj.weight", ad["image_proj.proj.weight"])
    with pytest.raises(CfgppError, match=r"missing .*image_proj\.proj\.bias"):
        u.set_image_context(emb, 1.0)
    _load(u, ad)
    with pytest.raises(CfgppError, match="rows=2"):
        u.set_image_context(emb[:2], 1.0)


# ---------------------------------------------------------------------------------------------------- solver level
def _pair(model, name, nfe, n_img=4):
    """(HIP solver, CPU solver on the mock engine with image tokens) with the same synthetic weights and adapter"""
    from ip_adapter_mock import IPMockEngine
    from mock_engine import StubVAE
    if model == "sd15":
        from cfgpp_amd.latent_diffusion import get_solver
    else:
        from cfgpp_amd.latent_sdxl import get_solver
    cfg, sd, ad, _ = _nets("tiny_sd" if model == "sd15" else "tiny_xl", n_img)
    sc = types.SimpleNamespace(num_sampling=nfe)
    hip = get_solver(name, solver_config=sc, device="cuda", unet_config=cfg, max_batch=2, latent_hw=(HW, HW), ip_adapter=ad,
                     scalar_semantics="cuda")
    ref = get_solver(name, solver_config=sc, device="cpu", unet_config=cfg, max_batch=2, latent_hw=(HW, HW), text_encoder=hip.text_encoder,
                     engine=IPMockEngine(cfg, sd, (HW, HW), adapter=ad), vae=StubVAE(cfg.vae_scale), scalar_semantics="cuda")
    return hip, ref, ad


def _sample_kw(model, lam, solver, cpu=False):
    """sample() arguments with the prompt embeddings of `solver` (shared by both sides of a comparison)"""
    prompts = ["a cat", "a dog"]
    pe = solver.get_text_embed("bad", prompts) if model == "sd15" else solver.get_text_embed("bad", prompts, "bad", prompts)
    if cpu:
        pe = tuple(x.cpu() for x in pe)
    kw = dict(cfg_guidance=lam, prompt_embeds=pe, seeds=[11, 12], return_latents=True)
    if model != "sd15":
        kw.update(target_size=(128, 128), original_size=(128, 128))
    return kw


# tolerances: those of the tiny chain tests (tests/test_gpu_unet.py ddim_cfg++ 3e-3; tests/test_gpu_configs.py XL_CASES 1.5e-3)
@pytest.mark.parametrize("model,name,nfe,lam,tol", [("sd15", "ddim_cfg++", 4, 0.6, 3e-3), ("sdxl", "ddim_cfg++", 4, 0.6, 1.5e-3),
                                                    ("sdxl", "ddim_cfg++_lightning", 2, 1.0, 1.5e-3)])
def test_chain_with_image_prompt_vs_mock(model, name, nfe, lam, tol):
    from test_gpu_configs import record
    hip, ref, ad = _pair(model, name, nfe)
    emb = torch.randn(1, ad.embed_dim, generator=torch.Generator().manual_seed(21)).half().float()
    kw, kwc = _sample_kw(model, lam, hip), _sample_kw(model, lam, hip, cpu=True)
    first = lambda r: (r[0] if isinstance(r, (tuple, list)) else r).float().cpu()  # noqa: E731
    a = first(hip.sample(ip_adapter_image_embeds=emb, ip_adapter_scale=0.8, **kw))
    b = first(ref.sample(ip_adapter_image_embeds=emb, ip_adapter_scale=0.8, **kwc))
    plain = first(ref.sample(**kwc))
    rel, moved = rel_l2(a, b), rel_l2(b, plain)
    record("ip_adapter_chain", model=model, name=name, nfe=nfe, rel_l2=rel, adapter_moves=moved)
    print(f"{model} {name}: chain rel-L2 {rel:.3e}; the image prompt moves the mock chain by {moved:.3e}")
    assert moved > 10 * tol
    assert torch.isfinite(a).all() and rel < tol, f"{name}: chain rel-L2 {rel:.3e}"
    # the next call without an image prompt is the plain chain
    assert rel_l2(first(hip.sample(**kw)), plain) < tol


def test_graph_replay_with_adapter_is_bit_identical_and_follows_the_scale(monkeypatch):
    cfg, sd, ad, _ = _nets("tiny_xl", 4)
    from cfgpp_amd.latent_sdxl import get_solver
    s = get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=4), device="cuda", unet_config=cfg, max_batch=2,
                   latent_hw=(HW, HW), ip_adapter=ad)
    emb = torch.randn(1, ad.embed_dim, generator=torch.Generator().manual_seed(22))
    kw = _sample_kw("sdxl", 0.6, s)

    def run(scale):
        extra = {} if scale is None else dict(ip_adapter_image_embeds=emb, ip_adapter_scale=scale)
        r = s.sample(**extra, **kw)
        return [t.clone() for t in (r if isinstance(r, (tuple, list)) else [r])]
    monkeypatch.setenv("CFGPP_GRAPH", "0")
    eager = {sc: run(sc) for sc in (0.8, 0.3, None)}
    monkeypatch.setenv("CFGPP_GRAPH", "1")
    for sc in (0.8, 0.3, 0.8, None, 0.3):              # scale change, detach and re-attach between replays
        got = run(sc)
        assert all(torch.equal(x, y) for x, y in zip(got, eager[sc])), sc
    assert not torch.equal(eager[0.8][0], eager[0.3][0]) and not torch.equal(eager[0.8][0], eager[None][0])


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl"])
def test_adapter_with_lora_and_with_controlnet(name):
    """one forward each, against the composed oracle: LoRA merges are independent of the adapter; an attached ControlNet sees
    the text only"""
    from cfgpp_amd.controlnet import HipControlNet, synth_controlnet_state_dict
    from cfgpp_amd.lora import merge_into_state_dict
    from controlnet_ref import ControlNetRef, controlled_unet
    from ip_adapter_ref import IPUNetRef
    from test_gpu_lora import dyadic_adapter, KEYS
    cfg, sd, ad, _ = _nets(name, 4)
    rows = 4
    z, ehs, te, ti, emb = _inputs(cfg, rows, seed=31, embed_dim=ad.embed_dim)
    kw = dict(text_embeds=te, time_ids=ti) if te is not None else None
    zz = torch.cat([z, z], 0)
    u = _engine(cfg, sd)
    _load(u, ad)
    # LoRA on attention and conv weights, merged on the device
    lora = dyadic_adapter(cfg, KEYS[name][:6], 32, seed=5)      # rank 32: moves the oracle by 6e-3 (tiny_sd) / 9e-2 (tiny_xl)
    for k, (up, down, _) in lora.items():
        u.lora(k, up, down)
    u.set_context(ehs, te, ti)
    u.set_image_context(emb, 0.9)
    got = u.forward(z.cuda(), 400.0).float().cpu()
    net = IPUNetRef(cfg, merge_into_state_dict(dict(sd), [(lora, 1.0)], cfg), ad).set_image(emb, 0.9)
    ref = net(zz, 400.0, ehs, kw)["sample"]
    assert rel_l2(got, ref) < EPS_REL, rel_l2(got, ref)
    assert rel_l2(ref, _oracle(_nets(name, 4)[3], z, 400.0, ehs, te, ti, emb, 0.9)) > 2 * EPS_REL       # the LoRA matters
    for k in lora:
        u.lora(k, None, None)
    # ControlNet next to the active adapter
    img = torch.rand(1, 3, 8 * HW, 8 * HW, generator=torch.Generator().manual_seed(32)).half().float()
    csd = synth_controlnet_state_dict(cfg, 0)
    cn = HipControlNet(cfg, max_rows=rows, sample_hw=(HW, HW))
    cn.load_state_dict(csd).finalize()
    cn.set_context(ehs, te, ti)
    cn.set_image(img.cuda())
    u.set_context(ehs, te, ti)
    u.attach_control(cn, 0.7)
    got = u.forward(z.cuda(), 400.0).float().cpu()
    u.attach_control(None, 0.0)
    down, mid = ControlNetRef(cfg, csd)(zz, 400.0, ehs, torch.cat([img] * rows), 0.7, kw)       # plain text-only ControlNet
    ipnet = IPUNetRef(cfg, sd, ad).set_image(emb, 0.9)
    ref = controlled_unet(ipnet, zz, 400.0, ehs, kw, down, mid)
    assert rel_l2(got, ref) < EPS_REL, rel_l2(got, ref)


# ---------------------------------------------------------------------------------------------------- real size
def test_real_sd15_ip_adapter_forward_vs_oracle_fixture():
    """SD1.5 at 512 x 512 (64 x 64 latent, shipped widths: head dims 40 / 80 / 160), 2 rows, a 4-token adapter with embed_dim
    1024, against the committed fp32 fixture (tests/golden/make_ip_adapter_golden.py); in its own process"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "realsize_ip.py")], cwd=root, capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("REALSIZE_RESULT ")]
    assert line, f"no result (rc={r.returncode}): {r.stdout[-2000:]} {r.stderr[-2000:]}"
    out = json.loads(line[-1].split(" ", 1)[1])
    print(out)
    assert r.returncode == 0 and out["ok"], out
