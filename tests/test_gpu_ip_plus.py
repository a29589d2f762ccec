"""-m gpu: IP-Adapter Plus - the Resampler image projection through the C ABI (include/cfgpp_ip_plus.h: cfgpp_unet_ip_load with the
Resampler's keys, cfgpp_unet_image_context_seq; csrc/cfgpp_debug.h: cfgpp_unet_ip_tokens) and the solvers, on the tiny nets: TINY_SD
(head dim 32: text pass + image pass) and TINY_XL (head dim 64: the fused one-launch kernel), against tests/ip_plus_ref.py.

Tokens are held to attn_cases.FACTOR x E_model per token row, E_model being the error against the fp64 Resampler of a CPU model that
keeps fp16 wherever the executor stores an activation (ip_plus_ref.resampler_tokens(storage16=True)) - computed on the CPU, never
from the GPU output.  Forwards are held to EPS_REL, the project's UNet tolerance, and every comparison also asserts that the oracle
with and without the adapter differ by more than 10 x EPS_REL."""
import ctypes
import dataclasses
import types

import pytest
import torch

import attn_cases as A
from test_gpu_ip_adapter import EPS_REL, HW, _cfg, _descriptions, _engine, _fwd, _load, _oracle, _sample_kw, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


_STATE = {}


def _nets(name, n_img=16, **geo):
    """(cfg, sd, parsed plus adapter, oracle) per (net, geometry), built once"""
    key = (name, n_img, tuple(sorted(geo.items())))
    if key not in _STATE:
        from cfgpp_amd.ip_adapter import parse_ip_adapter, synthetic_ip_adapter
        from cfgpp_amd.weights import synth_state_dict
        from ip_plus_ref import IPPlusUNetRef
        cfg = _cfg(name)
        cross = geo.pop("cross", None)
        if cross:
            cfg = dataclasses.replace(cfg, cross_attention_dim=cross)
        sd = synth_state_dict(cfg, 0)
        ad = parse_ip_adapter(synthetic_ip_adapter(cfg, kind="plus", n_img=n_img, seed=5 + n_img, **geo), cfg)
        _STATE[key] = (cfg, sd, ad, IPPlusUNetRef(cfg, sd, ad))
    return _STATE[key]


def _inputs(cfg, rows, S, E, seed=0, zero_uc=True):
    g = torch.Generator().manual_seed(300 + seed)
    zr = rows // 2
    z = (torch.randn(zr, 4, HW, HW, generator=g) * 0.8).half().float()
    ehs = torch.randn(rows, 77, cfg.cross_attention_dim, generator=g).half().float()
    te = ti = None
    if cfg.addition_embed:
        te = torch.randn(rows, cfg.addition_pooled_dim, generator=g).half().float()
        ti = torch.tensor([[HW * 8, HW * 8, 0, 0, HW * 8, HW * 8]] * rows, dtype=torch.float32)
    hid = torch.randn(rows, S, E, generator=g).half().float()
    if zero_uc:
        hid[:zr] = 0                                    # the default negative: zeros of the same shape
    return z, ehs, te, ti, hid


def _token_check(ad, got, hid, what, **rec):
    """got [rows, n_q, cross] (engine) against the fp64 Resampler, per token row, bound FACTOR x E_model"""
    from ip_plus_ref import resampler_tokens
    from test_gpu_configs import record
    cross = got.shape[-1]
    h = hid.half().float()
    ref = resampler_tokens(ad, h, torch.float64)
    e_model = A.max_row_err(resampler_tokens(ad, h, torch.float64, storage16=True), ref, cross)
    err = A.max_row_err(got, ref, cross)
    record(what, e_model=e_model, max_row_err=err, ratio=err / e_model, **rec)
    print(f"{what} {rec}: E_model {e_model:.3e} engine {err:.3e} ratio {err / e_model:.2f}")
    assert 0 < e_model < 2e-2, e_model
    assert err <= A.FACTOR * e_model, f"max token-row error {err:.3e} > {A.FACTOR:g} x E_model = {A.FACTOR * e_model:.3e}"


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl"])
@pytest.mark.parametrize("S", [5, 70])
@pytest.mark.parametrize("n_q", [4, 16])
@pytest.mark.parametrize("rows", [2, 4])
def test_tokens_vs_fp64_resampler(name, S, n_q, rows):
    cfg, sd, ad, _ = _nets(name, n_q)
    z, ehs, te, ti, hid = _inputs(cfg, rows, S, ad.embed_dim, seed=S + n_q + rows, zero_uc=False)
    u = _engine(cfg, sd)
    _load(u, ad)
    u.set_context(ehs, te, ti)
    u.set_image_context(hid, 1.0)
    _token_check(ad, u.ip_tokens(rows, n_q), hid, "ip_plus_tokens", net=name, S=S, n_q=n_q, rows=rows)


@pytest.mark.parametrize("name,geo", [("tiny_sd", dict(embed_dim=1280, hidden_dim=768, heads=12, depth=4, cross=768)),
                                      ("tiny_xl", dict(embed_dim=1280, hidden_dim=1280, heads=20, depth=4, cross=2048))])
def test_tokens_at_the_shipped_geometries(name, geo):
    """plus / plus-face SD1.5 and SDXL vit-h Resamplers (synthetic weights) on a tiny UNet with their cross_attention_dim, S = 257"""
    cfg, sd, ad, _ = _nets(name, 16, **geo)
    rows, S = 2, 257
    z, ehs, te, ti, hid = _inputs(cfg, rows, S, 1280, seed=1, zero_uc=False)
    u = _engine(cfg, sd)
    _load(u, ad)
    u.set_context(ehs, te, ti)
    u.set_image_context(hid, 1.0)
    _token_check(ad, u.ip_tokens(rows, 16), hid, "ip_plus_tokens_real", net=name, D=geo["hidden_dim"])


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl"])
@pytest.mark.parametrize("S,n_q,rows", [(5, 4, 2), (70, 16, 4)])
def test_forward_vs_oracle(name, S, n_q, rows):
    from test_gpu_configs import record
    cfg, sd, ad, net = _nets(name, n_q)
    z, ehs, te, ti, hid = _inputs(cfg, rows, S, ad.embed_dim, seed=rows + n_q)
    u = _engine(cfg, sd)
    _load(u, ad)
    u.set_context(ehs, te, ti)
    u.set_image_context(hid, 0.7)
    got = u.forward(z.cuda(), 321.0).float().cpu()
    ref = _oracle(net, z, 321.0, ehs, te, ti, hid, 0.7)
    plain = _oracle(net, z, 321.0, ehs, te, ti, None, 0.0)
    moved, rel = rel_l2(ref, plain), rel_l2(got, ref)
    record("ip_plus_forward", net=name, S=S, n_q=n_q, rows=rows, rel_l2=rel, adapter_moves=moved)
    print(f"{name} S={S} n_q={n_q} rows={rows}: rel-L2 {rel:.3e}, oracle with vs without the adapter {moved:.3e}")
    assert moved > 10 * EPS_REL, f"the adapter moves the oracle by only {moved:.3e}"
    assert torch.isfinite(got).all() and rel < EPS_REL, f"{name}: rel-L2 {rel:.3e}"


def _raw_seq(u, t, rows, seq, embed, scale):
    """cfgpp_unet_image_context_seq as the C caller sees it (no wrapper in between)"""
    from cfgpp_amd._lib import check
    stream = torch.cuda.current_stream().cuda_stream
    check(u.lib.cfgpp_unet_image_context_seq(u._h, t.data_ptr(), rows, seq, embed, ctypes.c_float(scale), stream), "cfgpp_unet_image_context_seq")


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl"])
def test_engine_state_transitions(name):
    """on ONE engine: scale 0 / NULL / ip_load(NULL) are the plain engine bit for bit; a Resampler adapter after a Linear one and
    back; S 70 then 5; a new scale alone launches nothing; a new text context keeps the image branch; device bytes"""
    from cfgpp_amd._lib import CfgppError
    from test_gpu_ip_adapter import _nets as _linear_nets
    cfg, sd, ad, net = _nets(name, 16)
    _, _, lin, lin_net = _linear_nets(name, 4)
    rows, E = 4, ad.embed_dim
    z, ehs, te, ti, hid70 = _inputs(cfg, rows, 70, E, seed=7)
    hid5 = _inputs(cfg, rows, 5, E, seed=8)[4]
    fresh = _fwd(_engine(cfg, sd), z, 500.0, ehs, te, ti).clone()
    u = _engine(cfg, sd)
    bytes0 = u.device_bytes()
    assert torch.equal(_fwd(u, z, 500.0, ehs, te, ti), fresh)
    detail0 = _descriptions(u.profile(z.cuda(), 500.0, detail=True))
    # a Linear adapter first ...
    _load(u, lin)
    emb = torch.randn(rows, lin.embed_dim, generator=torch.Generator().manual_seed(1)).half().float()
    u.set_image_context(emb, 1.0)
    assert rel_l2(u.forward(z.cuda(), 500.0), _oracle(lin_net, z, 500.0, ehs, te, ti, emb, 1.0)) < EPS_REL
    with pytest.raises(CfgppError, match=r"image_proj\.latents.*Resampler.*Linear \+ LayerNorm adapter: drop it"):
        u.ip_load("image_proj.latents", ad["image_proj.latents"])               # the other kind's key before a drop
    with pytest.raises(CfgppError, match="Linear.*cfgpp_unet_image_context "):
        u.set_image_context(hid5, 1.0)                                           # the wrong call for this kind names the other
    u.ip_load(None)
    assert u.device_bytes() == bytes0
    # ... then the Resampler adapter
    _load(u, ad)
    bytes_loaded = u.device_bytes()
    assert bytes_loaded > bytes0
    with pytest.raises(CfgppError, match=r"image_proj\.proj\.weight.*Linear \+ LayerNorm.*Resampler.*drop it"):
        u.ip_load("image_proj.proj.weight", lin["image_proj.proj.weight"])
    with pytest.raises(CfgppError, match="Resampler.*cfgpp_unet_image_context_seq"):
        u.set_image_context(emb, 1.0)
    assert u.device_bytes() == bytes_loaded
    u.set_image_context(hid70, 1.0)
    bytes70 = u.device_bytes()
    assert bytes70 > bytes_loaded                       # the scratch is adapter memory
    got = u.forward(z.cuda(), 500.0).float().cpu()
    assert rel_l2(got, _oracle(net, z, 500.0, ehs, te, ti, hid70, 1.0)) < EPS_REL
    # scale 0 and NULL: the plain engine, bit for bit, launch list included
    u.set_image_context(hid70, 0.0)
    assert torch.equal(u.forward(z.cuda(), 500.0), fresh)
    u.set_image_context(hid70, 1.0)
    u.set_image_context(None)
    assert torch.equal(u.forward(z.cuda(), 500.0), fresh)
    assert _descriptions(u.profile(z.cuda(), 500.0, detail=True)) == detail0
    # S 70 then 5: no stale tokens, no new scratch
    u.set_image_context(hid5, 1.0)
    assert u.device_bytes() == bytes70
    from ip_plus_ref import resampler_tokens
    tok5 = u.ip_tokens(rows, 16)
    ref5 = resampler_tokens(ad, hid5, torch.float64)
    assert A.max_row_err(tok5, ref5, cfg.cross_attention_dim) < 2e-2
    assert A.max_row_err(resampler_tokens(ad, hid70, torch.float64), ref5, cfg.cross_attention_dim) > 0.2
    ref = _oracle(net, z, 500.0, ehs, te, ti, hid5, 1.0)
    assert rel_l2(u.forward(z.cuda(), 500.0), ref) < EPS_REL
    assert rel_l2(ref, _oracle(net, z, 500.0, ehs, te, ti, hid70, 1.0)) > 10 * EPS_REL
    # a new scale alone launches nothing: the engine's copy of the hidden states is overwritten in place first, and the tokens stay
    kept = u._keep["ip_embeds"]
    kept.zero_()
    _raw_seq(u, kept, rows, 5, E, 0.4)
    assert torch.equal(u.ip_tokens(rows, 16), tok5)
    assert rel_l2(u.forward(z.cuda(), 500.0), _oracle(net, z, 500.0, ehs, te, ti, hid5, 0.4)) < EPS_REL
    kept.copy_(hid5.half())
    # a new text context keeps the image branch
    ehs2 = torch.randn(ehs.shape, generator=torch.Generator().manual_seed(9)).half().float()
    got = _fwd(u, z, 500.0, ehs2, te, ti).float().cpu()
    ref = _oracle(net, z, 500.0, ehs2, te, ti, hid5, 0.4)
    assert rel_l2(got, ref) < EPS_REL, rel_l2(got, ref)
    assert rel_l2(ref, _oracle(net, z, 500.0, ehs2, te, ti, None, 0.0)) > 10 * EPS_REL
    # refusals by name; none of them changes the active state
    for args, msg in (((kept[:2], 2, 5, E), "rows=2"), ((kept, rows, 5, 64), "embed_dim=64"), ((kept, rows, 0, E), "seq=0"),
                      ((kept, rows, 1025, E), "seq=1025")):
        with pytest.raises(CfgppError, match=msg):
            _raw_seq(u, *args, 0.4)
    assert rel_l2(u.forward(z.cuda(), 500.0), ref) < EPS_REL
    # drop: the plain engine again, every byte returned; and back to a Linear adapter
    u.ip_load(None)
    assert u.device_bytes() == bytes0
    assert torch.equal(_fwd(u, z, 500.0, ehs, te, ti), fresh)
    _load(u, lin)
    u.set_image_context(emb, 1.0)
    assert rel_l2(u.forward(z.cuda(), 500.0), _oracle(lin_net, z, 500.0, ehs, te, ti, emb, 1.0)) < EPS_REL
    u.ip_load(None)
    assert u.device_bytes() == bytes0


def test_load_refusals_name_the_key():
    from cfgpp_amd._lib import CfgppError
    cfg, sd, ad, _ = _nets("tiny_sd", 4)
    u = _engine(cfg, sd)
    b0 = u.device_bytes()
    Z = torch.zeros
    for key, t, msg in (("image_proj.latents", Z(1, 33, 128), r"image_proj\.latents.*1 <= n_q <= 32"),
                        ("image_proj.layers.0.0.to_q.weight", Z(96, 128), r"to_q\.weight.*inner = 96 must be a positive multiple of 64"),
                        ("image_proj.proj_in.weight", Z(128, 100), r"proj_in\.weight.*E = 100"),
                        ("image_proj.layers.0.1.1.weight", Z(200, 128), r"1\.1\.weight.*ff_inner = 200"),
                        ("image_proj.layers.8.0.to_q.weight", Z(128, 128), r"layers\.8\..*layer 8.*1 \.\. 8 layers"),
                        ("image_proj.norm_out.weight", Z(32), r"norm_out\.weight.*cross_attention_dim = 64"),
                        ("image_proj.layers.0.0.nope.weight", Z(128, 128), "unknown key")):
        with pytest.raises(CfgppError, match=msg):
            u.ip_load(key, t)
    assert u.device_bytes() == b0
    # tensors that disagree with what is loaded: layer 1 against layer 0, to_kv against to_q
    u.ip_load("image_proj.layers.0.0.to_q.weight", ad["image_proj.layers.0.0.to_q.weight"])
    b1 = u.device_bytes()
    with pytest.raises(CfgppError, match=r"layers\.1\.0\.to_q\.weight.*inner = 64.*loaded before have inner = 128"):
        u.ip_load("image_proj.layers.1.0.to_q.weight", Z(64, 128))
    with pytest.raises(CfgppError, match=r"to_kv\.weight.*192 rows.*2 \* inner = 256"):
        u.ip_load("image_proj.layers.0.0.to_kv.weight", Z(192, 128))
    assert u.device_bytes() == b1
    # missing tensors are named
    z, ehs, te, ti, hid = _inputs(cfg, 4, 5, ad.embed_dim)
    u.set_context(ehs, te, ti)
    with pytest.raises(CfgppError, match=r"missing .*image_proj\.latents"):
        u.set_image_context(hid, 1.0)
    for k, v in ad.items():
        if k != "image_proj.layers.1.1.3.weight":
            u.ip_load(k, v)
    with pytest.raises(CfgppError, match=r"missing 1 adapter tensors.*image_proj\.layers\.1\.1\.3\.weight"):
        u.set_image_context(hid, 1.0)
    with pytest.raises(CfgppError, match="no image tokens computed"):
        u.ip_tokens(4, 4)


# ---------------------------------------------------------------------------------------------------- solver level
def _pair(model, name, nfe):
    from ip_plus_mock import IPPlusMockEngine
    from mock_engine import StubVAE
    if model == "sd15":
        from cfgpp_amd.latent_diffusion import get_solver
    else:
        from cfgpp_amd.latent_sdxl import get_solver
    cfg, sd, ad, _ = _nets("tiny_sd" if model == "sd15" else "tiny_xl", 16)
    sc = types.SimpleNamespace(num_sampling=nfe)
    hip = get_solver(name, solver_config=sc, device="cuda", unet_config=cfg, max_batch=2, latent_hw=(HW, HW), ip_adapter=ad,
                     scalar_semantics="cuda")
    ref = get_solver(name, solver_config=sc, device="cpu", unet_config=cfg, max_batch=2, latent_hw=(HW, HW), text_encoder=hip.text_encoder,
                     engine=IPPlusMockEngine(cfg, sd, (HW, HW), adapter=ad), vae=StubVAE(cfg.vae_scale), scalar_semantics="cuda")
    return hip, ref, ad


# tolerances: those of the IP-Adapter chain tests (tests/test_gpu_ip_adapter.py)
@pytest.mark.parametrize("model,name,nfe,lam,tol", [("sd15", "ddim_cfg++", 4, 0.6, 3e-3), ("sdxl", "ddim_cfg++", 4, 0.6, 1.5e-3)])
def test_chain_with_image_prompt_vs_mock(model, name, nfe, lam, tol):
    from test_gpu_configs import record
    hip, ref, ad = _pair(model, name, nfe)
    hid = torch.randn(1, 9, ad.embed_dim, generator=torch.Generator().manual_seed(21)).half().float()
    kw, kwc = _sample_kw(model, lam, hip), _sample_kw(model, lam, hip, cpu=True)
    first = lambda r: (r[0] if isinstance(r, (tuple, list)) else r).float().cpu()  # noqa: E731
    a = first(hip.sample(ip_adapter_image_embeds=hid, ip_adapter_scale=0.8, **kw))
    b = first(ref.sample(ip_adapter_image_embeds=hid, ip_adapter_scale=0.8, **kwc))
    plain = first(ref.sample(**kwc))
    rel, moved = rel_l2(a, b), rel_l2(b, plain)
    record("ip_plus_chain", model=model, name=name, nfe=nfe, rel_l2=rel, adapter_moves=moved)
    print(f"{model} {name}: chain rel-L2 {rel:.3e}; the image prompt moves the mock chain by {moved:.3e}")
    assert moved > 10 * tol
    assert torch.isfinite(a).all() and rel < tol, f"{name}: chain rel-L2 {rel:.3e}"
    assert rel_l2(first(hip.sample(**kw)), plain) < tol                          # the next call without an image prompt: the plain chain
    from cfgpp_amd._lib import CfgppError
    with pytest.raises(CfgppError, match=r"Resampler.*\[1 or 2, seq, embed_dim\]"):
        hip.sample(ip_adapter_image_embeds=torch.zeros(1, ad.embed_dim), **kw)   # a 2-D tensor is refused with the expected shape


def test_graph_replay_with_a_plus_adapter_is_bit_identical(monkeypatch):
    cfg, sd, ad, _ = _nets("tiny_xl", 16)
    from cfgpp_amd.latent_sdxl import get_solver
    s = get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=4), device="cuda", unet_config=cfg, max_batch=2,
                   latent_hw=(HW, HW), ip_adapter=ad)
    hid = torch.randn(1, 9, ad.embed_dim, generator=torch.Generator().manual_seed(22))
    kw = _sample_kw("sdxl", 0.6, s)

    def run(scale):
        extra = {} if scale is None else dict(ip_adapter_image_embeds=hid, ip_adapter_scale=scale)
        r = s.sample(**extra, **kw)
        return [t.clone() for t in (r if isinstance(r, (tuple, list)) else [r])]
    monkeypatch.setenv("CFGPP_GRAPH", "0")
    eager = {sc: run(sc) for sc in (0.8, 0.3, None)}
    monkeypatch.setenv("CFGPP_GRAPH", "1")
    for sc in (0.8, 0.3, 0.8, None, 0.3):              # scale change, detach and re-attach between replays
        got = run(sc)
        assert all(torch.equal(x, y) for x, y in zip(got, eager[sc])), sc
    assert not torch.equal(eager[0.8][0], eager[0.3][0]) and not torch.equal(eager[0.8][0], eager[None][0])
