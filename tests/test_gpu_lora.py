"""-m gpu: LoRA merged on the device into the repacked UNet weights (include/cfgpp.h: cfgpp_unet_lora, csrc/lora_kernels.hip).

Exactness argument of the dyadic cases: adapter entries are in {-1, 0, 1} * 2^-5, so every product is 0 or +-2^-10 and every
partial sum of `rank` of them a multiple of 2^-10 of magnitude <= rank * 2^-10 <= 0.25; a base weight is fp16 with |w| < 0.75,
i.e. a multiple of 2^-24 - so base + delta is a multiple of 2^-24 below 1 and fits the 24-bit significand of fp32 whatever the
summation order.  The device result therefore has to equal the float64 host result rounded to fp16 BIT FOR BIT, and an engine
built from the host-merged state dict holds the same weights as one merged on the device."""
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

RANKS = (1, 4, 5, 130)
TB = "down_blocks.0.attentions.0.transformer_blocks.0"
KEYS = {
    "tiny_sd": [
        TB + ".attn1.to_q.weight", TB + ".attn1.to_k.weight", TB + ".attn1.to_v.weight",      # the three row offsets of the fused QKV
        TB + ".attn2.to_k.weight", TB + ".attn2.to_v.weight",                                  # K = cross dim, fused K/V
        TB + ".attn1.to_out.0.weight", TB + ".ff.net.0.proj.weight", TB + ".ff.net.2.weight",   # GEGLU: value and gate rows
        "down_blocks.0.attentions.0.proj_in.weight",                                           # conv1x1
        "down_blocks.0.resnets.0.conv1.weight",                                                # 64-channel 3x3
        "up_blocks.0.resnets.0.conv1.weight",                                                  # concatenated input: I / 64 = 4, tap minor
        "down_blocks.1.resnets.0.conv_shortcut.weight",
        "down_blocks.0.downsamplers.0.conv.weight", "up_blocks.0.upsamplers.0.conv.weight",
        "down_blocks.0.resnets.0.time_emb_proj.weight", "up_blocks.2.resnets.2.time_emb_proj.weight",     # first / last of the block
    ],
    "tiny_xl": [
        "down_blocks.1.attentions.0.proj_in.weight",                                           # linear proj_in
        "down_blocks.1.attentions.0.transformer_blocks.1.attn1.to_k.weight",
        "down_blocks.1.attentions.0.transformer_blocks.1.attn2.to_v.weight",
        "mid_block.attentions.0.transformer_blocks.1.ff.net.0.proj.weight",
        "up_blocks.0.resnets.2.conv1.weight", "up_blocks.0.upsamplers.0.conv.weight",
        "mid_block.resnets.1.time_emb_proj.weight", "up_blocks.1.resnets.2.time_emb_proj.weight",         # the last one of the block
        "add_embedding.linear_1.weight", "time_embedding.linear_2.weight",
    ],
}


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _cfg(name):
    from cfgpp_amd.unet_config import CONFIGS
    return CONFIGS[name]


def _matrix_keys(cfg):
    from cfgpp_amd.unet_config import param_shapes
    return [k for k, s in param_shapes(cfg).items() if len(s) in (2, 4) and k not in ("conv_in.weight", "conv_out.weight")]


def _flat_shape(shape):
    return int(shape[0]), int(np.prod(shape[1:]))


def dyadic(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, shape, generator=g).float() / 32.0


def dyadic_adapter(cfg, keys, rank, seed=0):
    """{key: (up, down, None)} with entries in {-1, 0, 1} / 32"""
    from cfgpp_amd.lora import ParsedLora
    from cfgpp_amd.unet_config import param_shapes
    shapes = param_shapes(cfg)
    out = ParsedLora()
    for i, k in enumerate(keys):
        O, K = _flat_shape(shapes[k])
        out[k] = (dyadic((O, rank), seed + 2 * i), dyadic((rank, K), seed + 2 * i + 1), None)
    return out


def expect_fp16(base, up, down):
    """float64 host result rounded once to fp16 (numpy: float64 -> float16 is a single correct rounding)"""
    w = base.double().numpy().reshape(up.shape[0], -1) + up.double().numpy() @ down.double().numpy()
    return torch.from_numpy(w.astype(np.float16)).reshape(base.shape)


_ENGINES = {}


def engine(name, weights="synthetic"):
    """one pristine-weights engine per config for the whole module (tests restore what they merge)"""
    from cfgpp_amd.hip_engine import HipEngine
    if weights != "synthetic":
        return HipEngine(_cfg(name), max_batch=1, latent_hw=(16, 16), weights=weights)
    if name not in _ENGINES:
        _ENGINES[name] = HipEngine(_cfg(name), max_batch=1, latent_hw=(16, 16))
    return _ENGINES[name]


def eps_at(eng, ts=(801.0, 201.0), seed=3):
    """eps of a fixed latent / conditioning at two timesteps; the conditioning is set afresh (set_context) every time"""
    cfg = eng.cfg
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((1, 4, 16, 16), generator=g).cuda()
    uc = (torch.randn((1, 77, cfg.cross_attention_dim), generator=g) * 0.5).half().cuda()
    c = (torch.randn((1, 77, cfg.cross_attention_dim), generator=g) * 0.5).half().cuda()
    te = ti = None
    if cfg.addition_embed:
        te = (torch.randn((2, cfg.addition_pooled_dim), generator=g) * 0.5).half().cuda()
        ti = torch.tensor([[128.0, 128, 0, 0, 128, 128]] * 2).cuda()
    eng.set_context(uc, c, te, ti)
    out = []
    for t in ts:
        a, b = eng.predict(z, t)
        out.append(torch.cat([a, b]).clone())
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl"])
def test_exact_merge_in_every_layout(name):
    cfg = _cfg(name)
    from cfgpp_amd.unet_config import param_shapes
    shapes = param_shapes(cfg)
    from cfgpp_amd.hip_engine import HipEngine
    unet = HipEngine(cfg, max_batch=1, latent_hw=(16, 16)).unet      # its own engine: the device-bytes accounting below starts from zero
    allk = _matrix_keys(cfg)
    before = {k: unet.read_weight(k) for k in allk}
    bytes0 = unet.device_bytes()
    for k, w in before.items():             # preconditions of the exactness argument
        assert w.dtype == torch.float16 and tuple(w.shape) == tuple(shapes[k]) and float(w.abs().max()) < 0.75, k
    assert max(RANKS) * 2.0 ** -10 <= 0.25
    for i, key in enumerate(KEYS[name]):
        O, K = _flat_shape(shapes[key])
        for rank in RANKS:
            up, down = dyadic((O, rank), 1000 * i + rank), dyadic((rank, K), 1000 * i + rank + 500)
            unet.lora(key, up, down)
            got = unet.read_weight(key)
            want = expect_fp16(before[key], up, down)
            assert not torch.equal(want, before[key])
            bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
            assert bad.numel() == 0, (key, rank, bad[:4].tolist(), got.flatten()[:4], want.flatten()[:4])
            # nothing else moved: a wrong row offset / stride would land in a neighbouring matrix
            for k2 in allk:
                if k2 != key:
                    assert torch.equal(unet.read_weight(k2).view(torch.int16), before[k2].view(torch.int16)), (key, rank, k2)
        unet.lora(key, None, None)          # rank 0: the base, bit for bit
        assert torch.equal(unet.read_weight(key).view(torch.int16), before[key].view(torch.int16)), key
    # the saved bases are device memory the engine accounts for; untouched keys cost nothing
    saved = sum(2 * int(np.prod(shapes[k])) for k in KEYS[name])
    assert unet.device_bytes() - bytes0 == saved


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl"])
def test_general_values_within_one_ulp(name):
    """Gaussian rank-16 adapter at a realistic scale: the only freedom against the float64 result is the fp32 summation order,
    which the single final rounding can turn into at most one fp16 ulp"""
    cfg = _cfg(name)
    from cfgpp_amd.unet_config import param_shapes
    shapes = param_shapes(cfg)
    unet = engine(name).unet
    g = torch.Generator().manual_seed(11)
    for key in KEYS[name]:
        O, K = _flat_shape(shapes[key])
        base = unet.read_weight(key)
        up = torch.randn((O, 16), generator=g) * 0.05
        down = torch.randn((16, K), generator=g) * (1.0 / K ** 0.5)
        unet.lora(key, up, down)
        got = unet.read_weight(key)
        want = expect_fp16(base, up, down)
        gi, wi = got.view(torch.int16).int(), want.view(torch.int16).int()
        # ordered-integer view of fp16: adjacent representable values differ by 1
        oi = lambda v: torch.where(v < 0, -(v & 0x7FFF), v)  # noqa: E731
        ulp = (oi(gi) - oi(wi)).abs().max().item()
        print(f"{key}: max ulp distance {ulp}, changed {(got != base).float().mean().item():.3f}")
        assert ulp <= 1, (key, ulp)
        assert (got != base).float().mean().item() > 0.5
        unet.lora(key, None, None)
        assert torch.equal(unet.read_weight(key).view(torch.int16), base.view(torch.int16))


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl"])
def test_forward_equals_an_engine_built_from_the_host_merged_weights(name):
    from cfgpp_amd.lora import merge_into_state_dict
    from cfgpp_amd.weights import synth_state_dict
    cfg = _cfg(name)
    ad = dyadic_adapter(cfg, _matrix_keys(cfg), rank=4, seed=7)
    A = engine(name)
    pristine = eps_at(A)
    A.set_lora([(ad, 1.0)])
    eps_a = eps_at(A)
    merged = merge_into_state_dict(synth_state_dict(cfg), [(ad, 1.0)], cfg)
    B = engine(name, weights=merged)
    for k in (TB + ".ff.net.0.proj.weight", "up_blocks.0.resnets.0.conv1.weight") if name == "tiny_sd" else ("add_embedding.linear_1.weight",):
        assert torch.equal(A.unet.read_weight(k).view(torch.int16), B.unet.read_weight(k).view(torch.int16)), k
    eps_b = eps_at(B)
    assert all(torch.isfinite(e.float()).all() for e in eps_a)
    assert _same(eps_a, eps_b)
    assert not _same(eps_a, pristine)                      # the adapter does something
    A.set_lora([])
    assert _same(eps_at(A), pristine)


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl"])
def test_restore_and_rescale_do_not_drift(name):
    cfg = _cfg(name)
    ad = dyadic_adapter(cfg, _matrix_keys(cfg), rank=4, seed=21)
    E = engine(name)
    pristine = eps_at(E)
    E.set_lora([(ad, 1.0)])
    E.set_lora([])
    assert _same(eps_at(E), pristine)
    E.set_lora([(ad, 0.5)])
    half_1 = eps_at(E)
    E.set_lora([(ad, 1.0)])
    full = eps_at(E)
    E.set_lora([(ad, 0.5)])
    half_2 = eps_at(E)
    E.set_lora([])
    assert _same(half_1, half_2) and not _same(half_1, full) and not _same(half_1, pristine)
    assert _same(eps_at(E), pristine)


def _kv_adapter(cfg, rank=4, seed=31):
    keys = [k for k in _matrix_keys(cfg) if k.endswith("attn2.to_k.weight") or k.endswith("attn2.to_v.weight")]
    return dyadic_adapter(cfg, keys, rank, seed)


def _sd_solver(nfe=3, **kw):
    from cfgpp_amd.latent_diffusion import get_solver
    return get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=nfe), device="cuda", unet_config=_cfg("tiny_sd"),
                      latent_hw=(16, 16), max_batch=1, **kw)


def test_cross_attention_cache_follows_the_adapters():
    """the cached cross-attention K / V^T are functions of attn2.to_k / to_v: one solver, the SAME embedding tensors, an adapter
    on those two matrices only - the second job must equal a fresh solver's that was built with the adapter"""
    ad = _kv_adapter(_cfg("tiny_sd"))
    s = _sd_solver()
    uc, c = s.get_text_embed("bad", ["a cat"])
    run = lambda sv: [t.clone() for t in sv.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), seeds=[5], return_latents=True)]  # noqa: E731
    plain = run(s)
    s.set_lora([(ad, 1.0)])
    adapted = run(s)
    fresh = run(_sd_solver(lora=[(ad, 1.0)]))
    assert _same(adapted, fresh) and not _same(adapted, plain)
    assert _same(run(s), adapted)
    s.set_lora([])
    assert _same(run(s), plain)


def test_graph_replay_survives_a_change_of_adapters(monkeypatch):
    """CFGPP_GRAPH=1: weight addresses do not move, so the captured step keeps replaying - with the new weights"""
    cfg = _cfg("tiny_sd")
    ad1 = dyadic_adapter(cfg, _matrix_keys(cfg), rank=4, seed=41)
    ad2 = _kv_adapter(cfg, seed=43)
    s = _sd_solver(nfe=4)
    uc, c = s.get_text_embed("bad", ["a cat"])
    run = lambda: [t.clone() for t in s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), seeds=[5], return_latents=True)]  # noqa: E731
    eager, graph = [], []
    for env, out in (("0", eager), ("1", graph)):
        monkeypatch.setenv("CFGPP_GRAPH", env)
        for adapters in ([(ad1, 1.0)], [(ad2, 0.5)], []):
            s.set_lora(adapters)
            out.append(run())
    for e, g in zip(eager, graph):
        assert _same(e, g)
    assert not _same(eager[0], eager[1]) and not _same(eager[1], eager[2])


def test_solver_lora_argument_equals_host_merged_weights_sd():
    from cfgpp_amd.lora import merge_into_state_dict
    from cfgpp_amd.weights import synth_state_dict
    cfg = _cfg("tiny_sd")
    ad = dyadic_adapter(cfg, _matrix_keys(cfg), rank=4, seed=51)
    a = _sd_solver(lora=[(ad, 0.75)])
    b = _sd_solver(unet_weights=merge_into_state_dict(synth_state_dict(cfg), [(ad, 0.75)], cfg))
    img_a = a.sample(cfg_guidance=0.6, prompt=["bad", "a cat"], seeds=[5])
    img_b = b.sample(cfg_guidance=0.6, prompt=["bad", "a cat"], seeds=[5])
    assert torch.equal(img_a, img_b) and torch.isfinite(img_a).all() and float(img_a.std()) > 0
    # lora_scale= on sample(): the same adapters at another scale, then back
    img_c = a.sample(cfg_guidance=0.6, prompt=["bad", "a cat"], seeds=[5], lora_scale=0.25)
    assert not torch.equal(img_c, img_a)
    assert torch.equal(a.sample(cfg_guidance=0.6, prompt=["bad", "a cat"], seeds=[5], lora_scale=0.75), img_a)


def test_solver_lora_argument_equals_host_merged_weights_sdxl():
    from cfgpp_amd.latent_sdxl import get_solver
    from cfgpp_amd.lora import merge_into_state_dict
    from cfgpp_amd.weights import synth_state_dict
    cfg = _cfg("tiny_xl")
    ad = dyadic_adapter(cfg, _matrix_keys(cfg), rank=4, seed=61)
    mk = lambda **kw: get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=3), device="cuda", unet_config=cfg,  # noqa: E731
                                 latent_hw=(16, 16), max_batch=1, **kw)
    a, b = mk(lora=[(ad, 0.75)]), mk(unet_weights=merge_into_state_dict(synth_state_dict(cfg), [(ad, 0.75)], cfg))
    kw = dict(prompt1=["bad", "a cat"], prompt2=["bad", "a cat"], cfg_guidance=0.6, target_size=(128, 128), original_size=(128, 128),
              seeds=[5], return_latents=True)
    za, zb = a.sample(**kw), b.sample(**kw)
    assert torch.equal(za, zb) and torch.isfinite(za.float()).all()


def test_cli_lora_flag_writes_the_api_image(tmp_path):
    from PIL import Image
    from safetensors.torch import save_file
    import text_to_img
    from cfgpp_amd.callback_util import save_image
    cfg = _cfg("tiny_sd")
    ad = dyadic_adapter(cfg, _matrix_keys(cfg)[:40], rank=4, seed=71)
    sd = {}
    for k, (up, down, _) in ad.items():
        stem = "lora_unet_" + k[:-len(".weight")].replace(".", "_")
        sd[stem + ".lora_up.weight"], sd[stem + ".lora_down.weight"], sd[stem + ".alpha"] = up, down, torch.tensor(2.0)
    path = tmp_path / "adapter.safetensors"
    save_file(sd, str(path))
    small = dict(unet_config=cfg, latent_hw=(16, 16))
    args = ["--prompt", "a cat", "--method", "ddim_cfg++", "--cfg_guidance", "0.6", "--NFE", "3"]
    text_to_img.main(args + ["--lora", f"{path}:0.75", "--workdir", str(tmp_path / "cli")], solver_kwargs=small)
    text_to_img.main(args + ["--workdir", str(tmp_path / "plain")], solver_kwargs=small)
    torch.manual_seed(42)                                  # the CLI's default --seed
    img = _sd_solver(lora=[(str(path), 0.75)]).sample(
        prompt=["low quality,jpeg artifacts,blurry,poorly drawn,ugly,worst quality,", "a cat"], cfg_guidance=0.6)
    save_image(img, tmp_path / "api.png", normalize=True)
    cli = np.asarray(Image.open(tmp_path / "cli" / "result" / "generated.png"))
    assert np.array_equal(cli, np.asarray(Image.open(tmp_path / "api.png")))
    assert not np.array_equal(cli, np.asarray(Image.open(tmp_path / "plain" / "result" / "generated.png")))


def test_refusals_on_the_device_leave_the_weights_alone():
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.engine import HipUNet
    cfg = _cfg("tiny_sd")
    unet = engine("tiny_sd").unet
    key = TB + ".attn1.to_k.weight"
    before = {k: unet.read_weight(k) for k in (key, TB + ".attn1.to_q.weight", TB + ".attn1.to_v.weight")}
    ok_up, ok_down = dyadic((64, 4), 1), dyadic((4, 64), 2)
    cases = [("conv_in.weight", dyadic((64, 4), 3), dyadic((4, 36), 4)),
             ("conv_out.weight", dyadic((4, 4), 3), dyadic((4, 576), 4)),
             (key, dyadic((64, 4), 5), dyadic((4, 32), 6)),                 # wrong K
             (key, dyadic((32, 4), 5), ok_down),                            # wrong O
             (key, dyadic((64, 3), 5), ok_down),                            # ranks differ
             (TB + ".norm1.weight", ok_up, ok_down),                        # 1-D parameter
             (TB + ".attn1.to_x.weight", ok_up, ok_down)]                   # unknown key
    for k, up, down in cases:
        with pytest.raises(CfgppError) as e:
            unet.lora(k, up, down)
        assert k in str(e.value), (k, str(e.value))
    for k, w in before.items():
        assert torch.equal(unet.read_weight(k).view(torch.int16), w.view(torch.int16)), k
    with pytest.raises(CfgppError) as e:
        unet.read_weight("conv_in.weight")
    assert "conv_in.weight" in str(e.value)
    raw = HipUNet(cfg, max_rows=2, sample_hw=(16, 16))            # created, not loaded, not finalized
    with pytest.raises(CfgppError) as e:
        raw.lora(key, ok_up, ok_down)
    assert key in str(e.value) and "finalized" in str(e.value)


def test_controlnet_engine_takes_adapters_and_the_unet_set_leaves_it_alone():
    """a ControlNet-mode engine has the same slot table; HipEngine.set_lora touches the UNet only"""
    E = engine("tiny_sd")
    cn = E.build_controlnet("synthetic")
    key = TB + ".attn2.to_v.weight"
    zc = "controlnet_down_blocks.1.weight"
    base, zbase = cn.read_weight(key), cn.read_weight(zc)
    cfg = _cfg("tiny_sd")
    E.set_lora([(dyadic_adapter(cfg, [key], rank=4, seed=81), 1.0)])
    assert torch.equal(cn.read_weight(key).view(torch.int16), base.view(torch.int16))          # the attached-or-not ControlNet is untouched
    E.set_lora([])
    up, down = dyadic((64, 5), 82), dyadic((5, 64), 83)
    cn.lora(key, up, down)
    assert torch.equal(cn.read_weight(key).view(torch.int16), expect_fp16(base, up, down).view(torch.int16))
    up2, down2 = dyadic((64, 5), 84), dyadic((5, 64), 85)
    cn.lora(zc, up2, down2)
    assert torch.equal(cn.read_weight(zc).view(torch.int16), expect_fp16(zbase, up2, down2).view(torch.int16))
    cn.lora(key, None, None); cn.lora(zc, None, None)
    assert torch.equal(cn.read_weight(key).view(torch.int16), base.view(torch.int16))


class _PinnedVAE:
    """the HIP VAE with the encoder's posterior noise pinned, shared by the two solvers of a comparison"""

    def __init__(self, scale, hw, noise):
        from cfgpp_amd.vae import HipVAE, synth_vae_state_dict
        self.v, self.noise = HipVAE(scale, hw, max_batch=1, state_dict=synth_vae_state_dict(0)), noise

    def encode(self, x):
        return self.v.encode(x, noise=self.noise[: x.shape[0]])

    def decode(self, z):
        return self.v.decode(z)


@pytest.mark.parametrize("nine", [True, False])
def test_inpaint_solver_lora_argument_equals_host_merged_weights(nine):
    """get_inpaint_solver(..., lora=) on a 9-channel inpaint UNet and on an ordinary one (masked update)"""
    from cfgpp_amd.inpaint import get_inpaint_solver
    from cfgpp_amd.lora import merge_into_state_dict
    from cfgpp_amd.weights import synth_state_dict
    cfg = _cfg("tiny_sd_inpaint" if nine else "tiny_sd")
    ad = dyadic_adapter(cfg, _matrix_keys(cfg), rank=4, seed=91)
    g = torch.Generator().manual_seed(5)
    img = torch.rand((1, 3, 128, 128), generator=g) * 2 - 1
    vae = _PinnedVAE(cfg.vae_scale, (16, 16), torch.randn((1, 4, 16, 16), generator=g))
    mask = torch.zeros(1, 1, 128, 128)
    mask[..., 48:112, 32:96] = 1.0
    mk = lambda **kw: get_inpaint_solver("ddim_inpaint_cfg++", model="sd15", solver_config=types.SimpleNamespace(num_sampling=3),  # noqa: E731
                                         device="cuda", unet_config=cfg, max_batch=1, latent_hw=(16, 16), vae=vae, **kw)
    a = mk(lora=[(ad, 0.75)])
    b = mk(unet_weights=merge_into_state_dict(synth_state_dict(cfg), [(ad, 0.75)], cfg))
    plain = mk()
    uc, c = a.get_text_embed("bad", ["a cat"])
    run = lambda s: s.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), src_img=img, mask=mask, seeds=[11], return_latents=True)[0].clone()  # noqa: E731
    za, zb, zp = run(a), run(b), run(plain)
    assert torch.isfinite(za.float()).all() and torch.equal(za, zb) and not torch.equal(za, zp)
    a.set_lora([])
    assert torch.equal(run(a), zp)


def test_refusals_of_the_c_entry_point_itself():
    """the same refusals straight through the C ABI (no Python-side check in between): rc != 0, the key in cfgpp_last_error(), the
    weight untouched.  (The entry point receives pointers and a rank only - extents are the caller's contract, include/cfgpp.h -
    so what it can refuse about the operands is a negative rank and a missing matrix.)"""
    from cfgpp_amd import _lib
    unet = engine("tiny_sd").unet
    lib, h = unet.lib, unet._h
    key = TB + ".attn1.to_k.weight"
    before = unet.read_weight(key)
    up, down = dyadic((64, 4), 1).cuda(), dyadic((4, 64), 2).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for k, u, d, rank, word in ((key, up, down, -1, "rank"), (key, None, down, 4, "null"), (key, up, None, 4, "null"),
                                ("conv_in.weight", up, down, 4, "fp32"), ("conv_out.weight", up, down, 4, "fp32"),
                                (TB + ".norm1.bias", up, down, 4, "1-D"), ("no.such.weight", up, down, 4, "unknown")):
        rc = lib.cfgpp_unet_lora(h, k.encode(), None if u is None else u.data_ptr(), None if d is None else d.data_ptr(), rank, stream)
        err = _lib.last_error()
        assert rc != 0 and k in err and word in err, (k, rank, rc, err)
    torch.cuda.synchronize()
    assert torch.equal(unet.read_weight(key).view(torch.int16), before.view(torch.int16))
