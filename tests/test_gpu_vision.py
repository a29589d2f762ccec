"""-m gpu: the CLIP image tower on the HIP kernels (csrc/vision.hip, cfgpp_amd/vision.py, include/cfgpp_vision.h) against
`transformers.CLIPVisionModelWithProjection` on the same weights - fp16-rounded on both sides, the reference evaluated in fp32 on
the CPU, as tests/test_gpu_text.py does for the text tower - and through the solvers: ``ip_adapter_image=`` takes the HIP tower,
falls back to the torch tower only for a geometry refused by name, and leaves a plain job's launches and bits alone.

The bar is the text tower's 4e-3 whole-tensor rel-L2 (same building blocks, same depths)."""
import types

import pytest
import torch

from test_gpu_configs import need_gpu, record

pytestmark = pytest.mark.gpu

BAR = 4e-3
CONFIGS = {
    # name: hidden, heads, layers, image px, activation, projection, intermediate         (patch 14 everywhere)
    "d64": (128, 2, 3, 56, "quick_gelu", 64, 256),             # 17 tokens
    "d80": (320, 4, 3, 84, "gelu", 64, 640),                   # 37 tokens
    "d104": (832, 8, 2, 56, "gelu", 128, 1664),                # 17 tokens
    "vit_h_width": (1280, 16, 2, 224, "gelu", 1024, 5120),     # 257 tokens
    "bigG_width": (1664, 16, 2, 224, "gelu", 1280, 8192),      # 257 tokens
}
_REF = {}


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def _vision_config(name, image=None):
    from transformers import CLIPVisionConfig
    hidden, heads, layers, px, act, proj, inter = CONFIGS[name]
    return CLIPVisionConfig(hidden_size=hidden, intermediate_size=inter, num_hidden_layers=layers, num_attention_heads=heads,
                            image_size=image or px, patch_size=14, projection_dim=proj, hidden_act=act)


def _reference(name):
    """(config, fp16 state dict, fp32 CPU model holding the same values), built once per configuration and shared"""
    if name not in _REF:
        from transformers import CLIPVisionModelWithProjection
        cfg = _vision_config(name)
        torch.manual_seed(7)
        ref = CLIPVisionModelWithProjection(cfg).eval()
        sd = {k: v.half() for k, v in ref.state_dict().items()}           # the engine stores fp16 matrices: compare like with like
        ref.load_state_dict({k: v.float() for k, v in sd.items()})
        _REF[name] = (cfg, sd, ref)
    return _REF[name]


def _tower(name, sd=None, max_batch=2):
    from cfgpp_amd.vision import HipClipImageTower
    hidden, heads, layers, px, act, proj, inter = CONFIGS[name]
    return HipClipImageTower(hidden, layers, heads, inter, act, proj, px, 14, sd if sd is not None else _reference(name)[1], max_batch=max_batch)


def _images(n, H, W, seed):
    return torch.rand((n, 3, H, W), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_hip_image_tower_vs_transformers(name):
    need_gpu()
    from cfgpp_amd.ip_adapter import preprocess_image
    cfg, sd, ref = _reference(name)
    hidden, heads, layers, px, act, proj, inter = CONFIGS[name]
    T = 1 + (px // 14) ** 2
    img = _images(3, 70, 90, 1) if px < 224 else _images(3, 240, 300, 1)           # 3 images through max_batch = 2: two slices
    with torch.no_grad():
        out = ref(pixel_values=preprocess_image(img, px).half().float(), output_hidden_states=True)
    assert len(out.hidden_states) == layers + 1
    tower = _tower(name)
    assert tower.torch_ops is False and tower.tokens == T
    emb = tower(img)
    assert emb.shape == (3, proj) and emb.dtype == torch.float16 and torch.isfinite(emb.float()).all()
    errs = dict(image_embeds=_rel(emb, out.image_embeds))
    pix = tower.preprocess(img)
    for label, k in (("hidden_states[-2]", -2), ("hidden_states[0]", 0), (f"hidden_states[{layers}]", layers)):
        hs = tower.encode_pixels(pix, hidden=True, layer=k)
        assert hs.shape == (3, T, hidden) and hs.dtype == torch.float16 and torch.isfinite(hs.float()).all()
        errs[label] = _rel(hs, out.hidden_states[k])
        if k == -2:
            assert torch.equal(hs, tower(img, hidden=True))                         # the default of hidden=True is the penultimate state
            errs["hidden_states[-2][:, 0]"] = _rel(hs[:, 0], out.hidden_states[-2][:, 0])          # the class token alone
    record("vision_tower", config=name, tokens=T, **errs)
    print(f"VISION_TOWER {name} (T = {T}): " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert tower.flops(1) > 0 and tower.device_bytes() > 0
    for k, v in errs.items():
        assert v < BAR, f"{name}: {k} rel-L2 {v:.3e} >= {BAR:g}"


def test_negative_hidden_is_the_tower_on_zero_pixels():
    need_gpu()
    tower = _tower("d64")
    img = _images(2, 70, 90, 2)
    neg = tower.negative_hidden(img)
    zeros = tower.encode_pixels(torch.zeros((2, 3, 56, 56)), hidden=True)
    assert neg.shape == (2, 17, 128) and torch.equal(neg, zeros)
    assert float(neg.float().abs().max()) > 0.1                                      # NOT zeros of the hidden states
    assert not torch.equal(neg, tower(img, hidden=True))


def test_keys_without_the_vision_model_prefix_load():
    """transformers 5.x drops the prefix on a bare CLIPVisionTransformer: both spellings give the same tower, bit for bit"""
    need_gpu()
    cfg, sd, ref = _reference("d64")
    bare = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}
    bare["embeddings.position_ids"] = torch.arange(17)[None]                          # skipped, in either spelling
    assert not any(k.startswith("vision_model.") for k in bare)
    img = _images(2, 60, 60, 3)
    assert torch.equal(_tower("d64", bare)(img, hidden=True), _tower("d64")(img, hidden=True))


def test_c_abi_refusals_name_the_problem():
    need_gpu()
    import hip_ops as H
    from cfgpp_amd import _lib
    from cfgpp_amd._lib import CfgppError
    lib = H.lib()
    for args, msg in (((1536, 2, 16, 4096, 1, 64, 224, 14, 1, 0), "unsupported head dim"), ((1280, 2, 16, 5000, 1, 64, 224, 14, 1, 0), "multiples of 64"),
                      ((1280, 2, 16, 5120, 1, 64, 225, 14, 1, 0), "not a multiple of patch_size"), ((1280, 2, 16, 5120, 1, 64, 336, 14, 1, 0), "577 tokens"),
                      ((1280, 2, 16, 5120, 2, 64, 224, 14, 1, 0), "activation 2")):
        assert not lib.cfgpp_vision_create(*args)
        assert msg in _lib.last_error(), (_lib.last_error(), msg)
    tower = _tower("d64")
    pix = torch.zeros((3, 3, 56, 56), dtype=torch.float16, device="cuda")
    out = torch.zeros((3, 17, 128), dtype=torch.float16, device="cuda")
    for n, layer, o, msg in ((3, 0, out, "N=3 images"), (1, 4, out, "layer 4 outside"), (1, 0, None, "hidden_out is NULL"), (1, -1, None, "no output requested")):
        with pytest.raises(CfgppError, match=msg):
            _lib.check(lib.cfgpp_vision_encode(tower._h, pix.data_ptr(), n, layer, None if o is None else o.data_ptr(), None, H.stream()), "encode")
    import ctypes as C
    raw = lib.cfgpp_vision_create(128, 1, 2, 256, 0, 64, 56, 14, 1, 0)                 # an engine that is not finalized yet
    assert raw
    try:
        t = torch.zeros(4)
        with pytest.raises(CfgppError, match="unknown key nonsense.weight"):
            _lib.check(lib.cfgpp_vision_load_tensor(raw, b"nonsense.weight", t.data_ptr(), 0, (C.c_long * 1)(4), 1), "load")
        with pytest.raises(CfgppError, match="has 4 elements, expected 128"):
            _lib.check(lib.cfgpp_vision_load_tensor(raw, b"pre_layrnorm.weight", t.data_ptr(), 0, (C.c_long * 1)(4), 1), "load")
        with pytest.raises(CfgppError, match="parameters not loaded"):
            _lib.check(lib.cfgpp_vision_finalize(raw), "finalize")
    finally:
        lib.cfgpp_vision_destroy(raw)


# ---------------------------------------------------------------------------------------------------- solver level
def _encoder_dir(tmp_path, name, image=None):
    """a diffusers-layout folder: image_encoder/config.json + model.safetensors (fp16), and the fp32 CPU reference of the same values"""
    from safetensors.torch import save_file
    from transformers import CLIPVisionModelWithProjection
    cfg = _vision_config(name, image)
    torch.manual_seed(9)
    ref = CLIPVisionModelWithProjection(cfg).eval()
    sd = {k: v.half() for k, v in ref.state_dict().items()}
    ref.load_state_dict({k: v.float() for k, v in sd.items()})
    d = tmp_path / "image_encoder"
    d.mkdir(parents=True)
    cfg.to_json_file(str(d / "config.json"))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
    return ref


def _solver(tmp_path, kind, **kw):
    from cfgpp_amd.ip_adapter import synthetic_ip_adapter
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    ad = synthetic_ip_adapter(TINY_SD, kind=kind, embed_dim=128 if kind == "plus" else 64, seed=3)     # d64 tower: hidden 128, projection 64
    return get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=4), device="cuda", unet_config=TINY_SD, max_batch=2,
                      latent_hw=(16, 16), ip_adapter=ad, ip_adapter_dir=str(tmp_path), scalar_semantics="cuda", **kw)


@pytest.mark.parametrize("kind", ["linear", "plus"])
def test_solver_takes_the_hip_tower_from_a_folder(tmp_path, kind):
    """exact: the solver built the HIP tower and recorded no fallback; approximate, at the IP-Adapter chain tests' bar (3e-3 for the tiny
    SD1.5 ddim_cfg++ chain): the chain equals the one fed with the reference tower's output on preprocess_image(img)"""
    need_gpu()
    from cfgpp_amd import vision
    from cfgpp_amd.ip_adapter import preprocess_image
    from test_gpu_ip_adapter import _sample_kw, rel_l2
    ref = _encoder_dir(tmp_path, "d64")
    n_fallbacks = len(vision.last_image_tower_fallbacks)
    s = _solver(tmp_path, kind)
    img = _images(1, 70, 90, 4)
    kw = _sample_kw("sd15", 0.6, s)
    first = lambda r: (r[0] if isinstance(r, (tuple, list)) else r).float().cpu()  # noqa: E731
    a = first(s.sample(ip_adapter_image=img, ip_adapter_scale=0.8, **kw))
    assert isinstance(s.image_encoder, vision.HipClipImageTower) and s.image_encoder.torch_ops is False
    assert len(vision.last_image_tower_fallbacks) == n_fallbacks
    with torch.no_grad():
        out = ref(pixel_values=preprocess_image(img, 56).half().float(), output_hidden_states=True)
        zero = ref(pixel_values=torch.zeros(1, 3, 56, 56), output_hidden_states=True)
    if kind == "plus":
        extra = dict(ip_adapter_image_embeds=out.hidden_states[-2], negative_ip_adapter_image_embeds=zero.hidden_states[-2])
    else:
        extra = dict(ip_adapter_image_embeds=out.image_embeds)
    b = first(s.sample(ip_adapter_scale=0.8, **extra, **kw))
    plain = first(s.sample(**kw))
    rel, moved = rel_l2(a, b), rel_l2(b, plain)
    record("vision_chain", kind=kind, rel_l2=rel, adapter_moves=moved)
    print(f"VISION_CHAIN {kind}: image vs reference-tower embeds rel-L2 {rel:.3e}; the image prompt moves the chain by {moved:.3e}")
    assert moved > 10 * 3e-3
    assert torch.isfinite(a).all() and rel < 3e-3, rel


def test_336_px_tower_is_refused_by_name_and_the_solver_falls_back(tmp_path):
    need_gpu()
    from cfgpp_amd import vision
    from cfgpp_amd.ip_adapter import ImageEncoder
    _encoder_dir(tmp_path, "d64", image=336)
    with pytest.raises(vision.UnsupportedTower, match="577 tokens"):
        vision.HipClipImageTower.from_dir(str(tmp_path))
    n = len(vision.last_image_tower_fallbacks)
    enc = vision.build_image_encoder(str(tmp_path), "cuda")
    assert isinstance(enc, ImageEncoder) and enc.torch_ops is True
    assert len(vision.last_image_tower_fallbacks) == n + 1 and "577 tokens" in vision.last_image_tower_fallbacks[-1]
    assert str(tmp_path) in vision.last_image_tower_fallbacks[-1]
    (tmp_path / "image_encoder" / "model.safetensors").unlink()                      # any OTHER failure propagates: no silent torch tower
    (tmp_path / "image_encoder" / "config.json").write_text(_vision_config("d64").to_json_string())
    with pytest.raises(Exception) as e:
        vision.build_image_encoder(str(tmp_path), "cuda")
    assert not isinstance(e.value, vision.UnsupportedTower) and len(vision.last_image_tower_fallbacks) == n + 1


def test_image_tower_torch_selects_the_old_tower_and_image_encoder_overrides(tmp_path):
    need_gpu()
    from cfgpp_amd import vision
    from cfgpp_amd.ip_adapter import ImageEncoder
    from test_gpu_ip_adapter import _sample_kw
    _encoder_dir(tmp_path, "d64", image=224)
    n = len(vision.last_image_tower_fallbacks)
    s = _solver(tmp_path, "linear", image_tower="torch")
    img = _images(1, 70, 90, 5)
    r = s.sample(ip_adapter_image=img, ip_adapter_scale=0.8, **_sample_kw("sd15", 0.6, s))
    assert isinstance(s.image_encoder, ImageEncoder) and len(vision.last_image_tower_fallbacks) == n          # a choice, not a fallback
    assert torch.isfinite(r[0].float()).all()
    calls = []

    class Mine:
        def __call__(self, image, hidden=False):
            calls.append(hidden)
            return torch.full((1, 64), 0.25)

    s2 = _solver(tmp_path, "linear", image_encoder=Mine())
    s2.sample(ip_adapter_image=img, **_sample_kw("sd15", 0.6, s2))
    assert calls == [False] and isinstance(s2.image_encoder, Mine)


def test_plain_job_runs_the_same_launches_and_bits_around_an_image_prompted_job(tmp_path):
    need_gpu()
    from cfgpp_amd import vision
    from test_gpu_ip_adapter import _sample_kw
    from test_gpu_pano_net import _launches
    _encoder_dir(tmp_path, "d64")
    s = _solver(tmp_path, "plus")
    kw = _sample_kw("sd15", 0.6, s)
    run = lambda: [t.clone() for t in s.sample(**kw)]  # noqa: E731
    before = run()
    z = torch.randn(2, 4, 16, 16).cuda()
    n0 = _launches(s.engine.unet, z)
    moved = s.sample(ip_adapter_image=_images(1, 70, 90, 6), ip_adapter_scale=0.8, **kw)
    assert isinstance(s.image_encoder, vision.HipClipImageTower)
    assert not torch.equal(moved[0], before[0])
    after = run()
    assert _launches(s.engine.unet, z) == n0
    fresh = [t.clone() for t in _solver(tmp_path, "plus").sample(**kw)]
    for x, y, w in zip(before, after, fresh):
        assert torch.equal(x, y) and torch.equal(x, w)
