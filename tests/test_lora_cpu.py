"""CPU: LoRA parsing (the three published namings, conv adapters, refusals) and the adapter bookkeeping (scale folding, rank
concatenation, restore of dropped keys, the epoch in the solvers' context-cache key) against an engine that records the
``lora()`` calls it receives."""
import types

import pytest
import torch

from cfgpp_amd import lora as L
from cfgpp_amd.unet_config import TINY_SD, param_shapes
from mock_engine import MockEngine, StubVAE

SHAPES = param_shapes(TINY_SD)
TB = "down_blocks.0.attentions.0.transformer_blocks.0"
K_Q = TB + ".attn1.to_q.weight"
K_KX = TB + ".attn2.to_k.weight"
K_OUT = TB + ".attn1.to_out.0.weight"
K_CONV = "down_blocks.1.resnets.0.conv1.weight"          # [128, 64, 3, 3]


def dyadic(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-1, 2, shape, generator=g).float() / 32.0)


def hand_made(rank=4, seed=0):
    """{weight key: (up, down, alpha)} - linear, cross-attention, to_out.0 and a 3x3 conv"""
    out = {}
    for i, key in enumerate((K_Q, K_KX, K_OUT, K_CONV)):
        shp = SHAPES[key]
        O, K = shp[0], int(torch.tensor(shp[1:]).prod())
        out[key] = (dyadic((O, rank), seed + 2 * i), dyadic((rank, K), seed + 2 * i + 1), float(rank) / 2)
    return out


def as_peft(ad, prefix="unet."):
    sd = {}
    for key, (up, down, alpha) in ad.items():
        m, shp = key[:-len(".weight")], SHAPES[key]
        if len(shp) == 4:
            up, down = up.reshape(shp[0], -1, 1, 1), down.reshape(-1, *shp[1:])
        sd[f"{prefix}{m}.lora_A.weight"], sd[f"{prefix}{m}.lora_B.weight"], sd[f"{prefix}{m}.alpha"] = down, up, torch.tensor(alpha)
    return sd


def as_old_diffusers(ad):
    sd = {}
    for key, (up, down, alpha) in ad.items():
        m, shp = key[:-len(".weight")], SHAPES[key]
        if len(shp) == 4:
            up, down = up.reshape(shp[0], -1, 1, 1), down.reshape(-1, *shp[1:])
        if key == K_Q:          # the attention-processor form
            parent, leaf = m.rsplit(".", 1)
            stem = f"unet.{parent}.processor.{leaf}_lora"
        else:
            stem = f"unet.{m}.lora"
        sd[stem + ".down.weight"], sd[stem + ".up.weight"], sd[f"unet.{m}.alpha"] = down, up, torch.tensor(alpha)
    return sd


def as_kohya(ad):
    sd = {}
    for key, (up, down, alpha) in ad.items():
        m, shp = key[:-len(".weight")], SHAPES[key]
        if len(shp) == 4:
            up, down = up.reshape(shp[0], -1, 1, 1), down.reshape(-1, *shp[1:])
        stem = "lora_unet_" + m.replace(".", "_")
        sd[stem + ".lora_down.weight"], sd[stem + ".lora_up.weight"], sd[stem + ".alpha"] = down, up, torch.tensor(alpha)
    return sd


def same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) and a[k][2] == b[k][2], k


def test_three_namings_parse_to_the_same_adapter():
    ad = hand_made()
    for form in (as_peft, as_old_diffusers, as_kohya, lambda a: as_peft(a, prefix="")):
        same(L.parse_lora(form(ad), TINY_SD), ad)
    no_alpha = {k: v for k, v in as_kohya(ad).items() if not k.endswith(".alpha")}
    assert all(v[2] is None for v in L.parse_lora(no_alpha, TINY_SD).values())


def test_parse_reads_a_safetensors_file(tmp_path):
    from safetensors.torch import save_file
    ad = hand_made()
    path = str(tmp_path / "adapter.safetensors")
    save_file({k: v.contiguous() for k, v in as_kohya(ad).items()}, path)
    same(L.parse_lora(path, TINY_SD), ad)


def test_conv_adapter_is_flattened_in_oihw_order():
    shp = SHAPES[K_CONV]
    r = 3
    down4 = torch.arange(r * shp[1] * 9, dtype=torch.float32).reshape(r, shp[1], 3, 3)
    up4 = dyadic((shp[0], r, 1, 1), 5)
    m = K_CONV[:-len(".weight")]
    p = L.parse_lora({f"{m}.lora_A.weight": down4, f"{m}.lora_B.weight": up4}, TINY_SD)
    up, down, alpha = p[K_CONV]
    assert alpha is None and tuple(up.shape) == (shp[0], r) and tuple(down.shape) == (r, shp[1] * 9)
    i, ky, kx = 5, 2, 1
    assert down[1, (i * 3 + ky) * 3 + kx] == down4[1, i, ky, kx] and torch.equal(up, up4.reshape(shp[0], r))
    delta = (up.double() @ down.double()).reshape(shp)
    want = torch.einsum("or,rikl->oikl", up4[:, :, 0, 0].double(), down4.double())
    assert torch.equal(delta, want)


class Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, key, up, down):
        self.calls.append((key, None if up is None else up.clone(), None if down is None else down.clone()))


def test_scales_alpha_and_rank_concatenation():
    a, b = hand_made(rank=4, seed=0), hand_made(rank=2, seed=100)
    b = {K_Q: b[K_Q], K_CONV: b[K_CONV]}
    rec = Recorder()
    st = L.LoraState(TINY_SD, rec)
    st.set([(as_peft(a), 0.75), (as_kohya(b), 0.5)])
    assert [c[0] for c in rec.calls] == list(a)           # one call per touched key, however many adapters
    got = {k: (u, d) for k, u, d in rec.calls}
    assert got[K_Q][0].shape[1] == 6 and got[K_Q][1].shape[0] == 6 and got[K_OUT][0].shape[1] == 4
    assert all(u.dtype == torch.float32 and d.dtype == torch.float32 for u, d in got.values())
    da, db = L.merged_delta(L.parse_lora(as_peft(a), TINY_SD), 0.75), L.merged_delta(L.parse_lora(as_kohya(b), TINY_SD), 0.5)
    for k, (u, d) in got.items():
        want = da[k] + (db[k] if k in db else 0)
        assert torch.equal(u.double() @ d.double(), want), k
    # alpha / rank is applied: alpha = rank / 2 halves the delta
    up, down, alpha = a[K_OUT]
    assert torch.equal(da[K_OUT], 0.75 * 0.5 * (up.double() @ down.double()))


def test_second_set_restores_dropped_keys_and_bumps_the_epoch():
    a = hand_made()
    rec = Recorder()
    st = L.LoraState(TINY_SD, rec)
    e0 = st.epoch
    st.set([(as_peft(a), 1.0)])
    assert st.epoch == e0 + 1 and set(st.keys) == set(a)
    del rec.calls[:]
    st.set([(as_peft({K_Q: a[K_Q]}), 1.0)])
    assert st.epoch == e0 + 2
    merged = [c[0] for c in rec.calls if c[1] is not None]
    restored = [c[0] for c in rec.calls if c[1] is None]
    assert merged == [K_Q] and sorted(restored) == sorted(k for k in a if k != K_Q)
    del rec.calls[:]
    st.set([])
    assert [(c[0], c[1]) for c in rec.calls] == [(K_Q, None)] and st.keys == ()
    del rec.calls[:]
    st.set([(as_peft(a), 1.0)])
    st.rescale(0.5)
    assert torch.equal(rec.calls[-1][1], 0.5 * rec.calls[len(a) - 1][1])


class LoraMockEngine(MockEngine):
    def __init__(self, fn, cfg):
        super().__init__(fn)
        self.rec = Recorder()
        self._lora = L.LoraState(cfg, self.rec)

    def set_lora(self, adapters, ignore_text_encoder=False):
        self._lora.set(adapters, ignore_text_encoder=ignore_text_encoder)

    lora_epoch = property(lambda self: self._lora.epoch)
    lora_adapters = property(lambda self: list(self._lora.adapters))


class StubText:
    def __init__(self, dim):
        self.dim = dim

    def __call__(self, prompts):
        return torch.zeros(len(prompts), 77, self.dim, dtype=torch.float16), torch.zeros(len(prompts), self.dim, dtype=torch.float16)


def _solver(mod, name, eng, **kw):
    return mod.get_solver(name, solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", engine=eng, latent_hw=(8, 8), **kw)


def test_epoch_changes_the_context_cache_key_sd():
    import cfgpp_amd.latent_diffusion as sd
    eng = LoraMockEngine(lambda z, t, ehs, te, ti: (z * 0.1).half(), TINY_SD)
    ad = as_peft(hand_made())
    s = _solver(sd, "ddim_cfg++", eng, unet_config=TINY_SD, text_encoder=StubText(64), vae=StubVAE(0.18215), lora=[(ad, 0.5)])
    assert len(eng.rec.calls) == 4                       # get_solver(lora=...) merged the adapter
    uc, c = torch.zeros(1, 77, 64, dtype=torch.float16), torch.ones(1, 77, 64, dtype=torch.float16)
    run = lambda **k: s.sample(prompt_embeds=(uc, c), seeds=[1], return_latents=True, **k)  # noqa: E731
    run(); run()
    assert len(eng.contexts) == 1                        # same embeddings, same adapters: the context is cached
    s.set_lora([(ad, 1.0)])
    run()
    assert len(eng.contexts) == 2                        # same embedding tensors, new adapters: set_context ran again
    run(lora_scale=1.0)
    assert len(eng.contexts) == 2                        # unchanged scale: nothing to do
    n = len(eng.rec.calls)
    run(lora_scale=0.25)
    assert len(eng.contexts) == 3 and len(eng.rec.calls) == n + 4
    assert torch.equal(eng.rec.calls[-1][1], 0.25 * eng.rec.calls[n - 1][1])
    s.set_lora([])
    assert all(c[1] is None for c in eng.rec.calls[-4:])


def test_epoch_changes_the_context_cache_key_sdxl():
    import cfgpp_amd.latent_sdxl as xl
    from cfgpp_amd.unet_config import TINY_XL
    eng = LoraMockEngine(lambda z, t, ehs, te, ti: (z * 0.1).half(), TINY_XL)
    s = _solver(xl, "ddim_cfg++", eng, unet_config=TINY_XL, text_encoder=(StubText(64), StubText(64)), vae=StubVAE(0.13025))
    pe = (torch.zeros(1, 77, 128, dtype=torch.float16), torch.ones(1, 77, 128, dtype=torch.float16),
          torch.zeros(1, 64, dtype=torch.float16), torch.ones(1, 64, dtype=torch.float16))
    kw = dict(prompt_embeds=pe, seeds=[1], return_latents=True, target_size=(64, 64), original_size=(64, 64))
    s.sample(**kw)
    n = len(eng.contexts)
    key = "mid_block.attentions.0.transformer_blocks.0.attn2.to_v"
    s.set_lora([({f"{key}.lora_A.weight": dyadic((2, 128), 1), f"{key}.lora_B.weight": dyadic((128, 2), 2)}, 1.0)])
    s.sample(**kw)
    assert len(eng.contexts) > n and [c[0] for c in eng.rec.calls] == [key + ".weight"]


def test_engine_without_lora_support_is_refused():
    import cfgpp_amd.latent_diffusion as sd
    with pytest.raises(ValueError, match="cannot merge LoRA"):
        _solver(sd, "ddim", MockEngine(lambda *a: None), unet_config=TINY_SD, text_encoder=StubText(64), lora=[(as_peft(hand_made()), 1.0)])


M_Q = K_Q[:-len(".weight")]
_UP, _DOWN = dyadic((64, 2), 1), dyadic((2, 64), 2)


@pytest.mark.parametrize("sd_, names", [
    ({"lora_unet_input_blocks_1_1_proj_in.lora_down.weight": _DOWN, "lora_unet_input_blocks_1_1_proj_in.lora_up.weight": _UP},
     "lora_unet_input_blocks_1_1_proj_in"),
    ({f"lora_unet_{M_Q.replace('.', '_')}.hada_w1_a": _UP}, "hada_w1_a"),
    ({f"lora_unet_{M_Q.replace('.', '_')}.lokr_w1": _UP}, "lokr_w1"),
    ({f"unet.{M_Q}.lora_A.weight": _DOWN, f"unet.{M_Q}.lora_B.weight": _UP, f"unet.{M_Q}.lora_magnitude_vector": _UP[:, 0]},
     "lora_magnitude_vector"),
    ({f"lora_unet_{M_Q.replace('.', '_')}.dora_scale": _UP[:, 0]}, "dora_scale"),
    ({"unet.down_blocks.7.attentions.0.proj_in.lora_A.weight": _DOWN}, "down_blocks.7.attentions.0.proj_in"),
    ({"lora_unet_down_blocks_7_attentions_0_proj_in.lora_down.weight": _DOWN}, "down_blocks_7_attentions_0_proj_in"),
    ({f"unet.{M_Q}.lora_A.weight": _DOWN}, K_Q),                                              # incomplete pair
    ({f"unet.{M_Q}.lora_A.weight": _DOWN, f"unet.{M_Q}.lora_B.weight": dyadic((32, 2), 3)}, K_Q),       # wrong shape
    ({f"unet.{M_Q}.lora_A.weight": dyadic((3, 64), 4), f"unet.{M_Q}.lora_B.weight": _UP}, K_Q),         # ranks differ
    ({f"unet.{TB}.norm1.lora_A.weight": _DOWN, f"unet.{TB}.norm1.lora_B.weight": _UP}, "norm1"),      # 1-D parameter
    ({"lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight": _DOWN}, "lora_te_text_model_encoder_layers_0_mlp_fc1"),
    ({"text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight": _DOWN}, "text_encoder.text_model.encoder.layers.0.mlp.fc1"),
    ({f"unet.{M_Q}.something_else": _DOWN}, "something_else"),
])
def test_refusals_name_the_key(sd_, names):
    with pytest.raises(L.LoraError) as e:
        L.parse_lora(sd_, TINY_SD)
    assert names in str(e.value), str(e.value)


def test_text_encoder_entries_are_reported_when_ignored():
    sd_ = as_kohya({K_Q: hand_made()[K_Q]})
    sd_["lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight"] = _DOWN
    sd_["text_encoder.text_model.encoder.layers.0.mlp.fc1.lora_A.weight"] = _DOWN
    p = L.parse_lora(sd_, TINY_SD, ignore_text_encoder=True)
    assert list(p) == [K_Q] and sorted(p.report["ignored_text_encoder"]) == sorted(k for k in sd_ if "text" in k)


def test_cli_spec():
    assert L.parse_cli(["a.safetensors:0.75", "/x/b.safetensors", "c:d.safetensors"]) == [
        ("a.safetensors", 0.75), ("/x/b.safetensors", 1.0), ("c:d.safetensors", 1.0)]


def test_host_merge_rounds_once():
    from cfgpp_amd.weights import synth_tensor
    ad = {K_Q: hand_made()[K_Q]}
    w = synth_tensor(K_Q, SHAPES[K_Q], 0)
    out = L.merge_into_state_dict({K_Q: w}, [(as_peft(ad), 0.5)], TINY_SD)
    up, down, alpha = ad[K_Q]
    want = (w.double() + 0.5 * (alpha / 4) * (up.double() @ down.double())).half().float()
    assert torch.equal(out[K_Q], want) and not torch.equal(out[K_Q], w)


def test_lora_file_next_to_the_model_is_picked_up_and_the_cli_flag_replaces_it(tmp_path, caplog):
    """checkpoint.solver_kwargs_from_dir: <dir>/pytorch_lora_weights.safetensors (or lora.safetensors) becomes lora=[(path, 1.0)]
    with a logged warning and its text-encoder entries set aside; --lora on the command line replaces it (and refuses
    text-encoder entries again); a directory without such a file is untouched"""
    import logging
    import os
    import sys
    from safetensors.torch import save_file
    from cfgpp_amd.checkpoint import solver_kwargs_from_dir
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import text_to_img
    d = tmp_path / "ckpt"
    d.mkdir()
    assert "lora" not in solver_kwargs_from_dir(d, sdxl=False, device="cpu")[0]
    a, b = {K_Q: hand_made(seed=0)[K_Q]}, {K_OUT: hand_made(seed=50)[K_OUT]}
    beside = as_kohya(a)
    beside["lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight"] = _DOWN
    save_file({k: v.contiguous() for k, v in beside.items()}, str(d / "pytorch_lora_weights.safetensors"))
    save_file({k: v.contiguous() for k, v in as_kohya(b).items()}, str(tmp_path / "other.safetensors"))
    with caplog.at_level(logging.WARNING, logger="cfgpp_amd"):
        kw, _ = solver_kwargs_from_dir(d, sdxl=False, device="cpu")
    assert kw["lora"] == [(str(d / "pytorch_lora_weights.safetensors"), 1.0)] and kw["lora_ignore_text_encoder"] is True
    assert "pytorch_lora_weights.safetensors" in caplog.text
    os.rename(d / "pytorch_lora_weights.safetensors", d / "lora.safetensors")
    assert solver_kwargs_from_dir(d, sdxl=False, device="cpu")[0]["lora"] == [(str(d / "lora.safetensors"), 1.0)]

    def run(extra):
        eng = LoraMockEngine(lambda z, t, ehs, te, ti: (z * 0.1).half(), TINY_SD)
        text_to_img.main(["--method", "ddim_cfg++", "--cfg_guidance", "0.6", "--NFE", "2", "--prompt", "a cat", "--device", "cpu",
                          "--model_dir", str(d), "--workdir", str(tmp_path / "out")] + extra,
                         solver_kwargs=dict(engine=eng, vae=StubVAE(0.18215), latent_hw=(8, 8), unet_config=TINY_SD, text_encoder=StubText(64)))
        return eng
    eng = run([])
    assert [c[0] for c in eng.rec.calls] == [K_Q] and torch.equal(eng.rec.calls[0][1], a[K_Q][0] * 0.5)      # alpha / rank = 1/2, scale 1
    eng = run(["--lora", f"{tmp_path / 'other.safetensors'}:0.5"])
    assert [c[0] for c in eng.rec.calls] == [K_OUT] and torch.equal(eng.rec.calls[0][1], b[K_OUT][0] * 0.25)
    with pytest.raises(L.LoraError, match="lora_te_text_model"):       # an explicit --lora does not inherit the pickup's leniency
        run(["--lora", str(d / "lora.safetensors")])
