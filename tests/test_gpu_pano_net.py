"""-m gpu: MultiDiffusion panoramas on the HIP engine - 3-step `ddim_panorama` / `ddim_panorama_cfg++` chains of both families on a
16 x 32 panorama of 16 x 16 windows (stride 8, plain and circular, 2 chains) against the same solver on a mock engine whose UNet is
the oracle and whose step is the slice model of tests/pano_ref.py; the one-view panorama against the plain solver bit for bit; the
wrap, FreeU and LoRA reach the result; a plain engine is untouched by a panorama job; the decoded image.

Chain tolerances (the convention of tests/test_gpu_unet.py's chain cases and tests/test_gpu_lcm_net.py: measure the rel-L2 of the
final z0t on the MI355X against the oracle loop, assert twice it; the headroom is for box-to-box tile-tuning draws).  Measured:
CHAIN_MEASURED below and profiles/panorama/README.md.  Every value is far below steps x 2.5e-3, the per-forward tolerance times
the chain length, above which a value would be a defect to find: the CFG++ chains (cfg_guidance 0.6) sit at 2.7e-4 .. 3.6e-4, the CFG
chains (cfg_guidance 7.5, where eps_hat carries 7.5 times the difference of the two halves) at 2.4e-3 .. 3.3e-3 of the 7.5e-3."""
import types

import numpy as np
import pytest
import torch

from pano_mock import PanoMockEngine

pytestmark = pytest.mark.gpu

EPS_REL = 2.5e-3            # the project's per-forward tolerance (tests/test_gpu_unet.py)
STEPS = 3
HW, PANO = (16, 16), (16, 32)
# measured rel-L2 of the final z0t of the 3-step chains below against the oracle loop -> asserted at twice the value
CHAIN_MEASURED = {
    ("sd15", "ddim_panorama", False): 3.267e-3, ("sd15", "ddim_panorama", True): 2.736e-3,
    ("sd15", "ddim_panorama_cfg++", False): 3.557e-4, ("sd15", "ddim_panorama_cfg++", True): 3.025e-4,
    ("sdxl", "ddim_panorama", False): 2.814e-3, ("sdxl", "ddim_panorama", True): 2.371e-3,
    ("sdxl", "ddim_panorama_cfg++", False): 3.136e-4, ("sdxl", "ddim_panorama_cfg++", True): 2.666e-4,
}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def _cfg(model):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    return TINY_SD if model == "sd15" else TINY_XL


def _pano(name, model, circular, pano=PANO, **kw):
    from cfgpp_amd.panorama import get_panorama_solver
    kw.setdefault("solver_config", types.SimpleNamespace(num_sampling=STEPS))
    kw.setdefault("max_batch", 8)
    return get_panorama_solver(name, model=model, panorama_hw=pano, stride=8, circular_padding=circular, unet_config=_cfg(model),
                               latent_hw=HW, scalar_semantics="cuda", **kw)


def _embeds(s, model):
    if model == "sd15":
        return s.get_text_embed("bad", ["a cat", "a dog"])
    return s.get_text_embed("bad", ["a cat", "a dog"], "bad", ["a cat", "a dog"])


def _sample(s, pe, seeds, lam=0.6, **kw):
    return s.sample(prompt_embeds=pe, seeds=seeds, cfg_guidance=lam, return_latents=True, **kw)


class OraclePanoMock(PanoMockEngine):
    """the mock engine whose UNet is the oracle"""

    def __init__(self, cfg, sd):
        from oracle.unet_ref import UNetRef
        self.net = UNetRef(cfg, sd)
        super().__init__(self._unet, HW)

    def _unet(self, z, t, ehs, te, ti):
        ack = None if te is None else {"text_embeds": te.float(), "time_ids": ti.float()}
        return self.net(z.float(), t, ehs.float(), ack)["sample"].half()


# ---------------------------------------------------------------------------------------------------- chains against the oracle
@pytest.mark.parametrize("circular", [False, True], ids=["plain", "circular"])
@pytest.mark.parametrize("name", ["ddim_panorama", "ddim_panorama_cfg++"])
@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_chain_vs_oracle_loop(model, name, circular):
    need_gpu()
    from cfgpp_amd.weights import synth_state_dict
    cfg = _cfg(model)
    hip = _pano(name, model, circular, device="cuda")
    eng = OraclePanoMock(cfg, synth_state_dict(cfg, 0))
    ref = _pano(name, model, circular, device="cpu", text_encoder=hip.text_encoder, engine=eng)
    pe = _embeds(hip, model)
    seeds = [11, 12]
    lam = 0.6 if name.endswith("cfg++") else 7.5
    a0, az = (t.clone() for t in _sample(hip, pe, seeds, lam))
    b0, bz = _sample(ref, tuple(x.cpu() for x in pe), seeds, lam)
    V = 4 if circular else 3
    assert [n for n, _ in eng.pcalls] == ["gather_views"] + ["predict_into", "step_ddim_views"] * STEPS          # all views in one forward
    assert eng.contexts[0]["rows"] == 2 * V * 2 and len(eng.contexts) == 1
    rel, rel_z = rel_l2(a0, b0), rel_l2(az, bz)
    print(f"PANO_CHAIN {model} {name} {'circular' if circular else 'plain'}: z0t rel-L2 {rel:.3e}, zt rel-L2 {rel_z:.3e}")
    assert a0.shape == (2, 4) + PANO and torch.isfinite(a0).all() and torch.isfinite(az).all()
    assert rel < STEPS * EPS_REL, rel
    tol = 2 * CHAIN_MEASURED[(model, name, circular)]
    assert rel < tol, (rel, tol)
    # the same seeds again: the same bits
    again = _sample(hip, pe, seeds, lam)
    assert torch.equal(again[0], a0) and torch.equal(again[1], az)


# ---------------------------------------------------------------------------------------------------- the other properties
@pytest.mark.parametrize("model", ["sd15", "sdxl"])
def test_one_view_panorama_is_the_plain_solver_bit_for_bit(model):
    need_gpu()
    from cfgpp_amd import latent_diffusion as sd, latent_sdxl as xl
    pan = _pano("ddim_panorama_cfg++", model, False, pano=HW, device="cuda", max_batch=2)
    pe = _embeds(pan, model)
    a0, az = (t.clone() for t in _sample(pan, pe, [5, 6]))
    mod = sd if model == "sd15" else xl
    plain = mod.get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=STEPS), device="cuda", unet_config=_cfg(model),
                           max_batch=2, latent_hw=HW, scalar_semantics="cuda", text_encoder=pan.text_encoder)
    if model == "sd15":
        b0, bz = plain.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=[5, 6], return_latents=True)
        assert torch.equal(az, bz)
    else:          # (the SDXL ddim solvers return z0t)
        b0 = plain.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=[5, 6], return_latents=True, target_size=(128, 128),
                          original_size=(128, 128))
    assert torch.equal(a0, b0)


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


def test_wrap_freeu_and_lora_reach_the_result_and_the_image_is_the_panorama():
    need_gpu()
    # the tolerance of the chains this test runs: tiny SD, ddim_panorama_cfg++ at cfg_guidance 0.6, the larger of the two paddings
    tol = 2 * max(CHAIN_MEASURED[("sd15", "ddim_panorama_cfg++", c)] for c in (False, True))
    circ = _pano("ddim_panorama_cfg++", "sd15", True, device="cuda")
    pe = _embeds(circ, "sd15")
    seeds = [21, 22]
    base = _sample(circ, pe, seeds)[0].clone()
    plain = _pano("ddim_panorama_cfg++", "sd15", False, device="cuda", text_encoder=circ.text_encoder)
    other = _sample(plain, pe, seeds)[0]
    print(f"PANO_WRAP circular vs plain rel-L2 {rel_l2(base, other):.3e}")
    assert rel_l2(base, other) > 10 * tol                                     # the wrap is live
    # FreeU and LoRA are engine state: they change the result, and None / [] restore it bit for bit
    circ.set_freeu((0.9, 0.2, 1.2, 1.4))
    assert rel_l2(_sample(circ, pe, seeds)[0], base) > 10 * tol
    circ.set_freeu(None)
    assert torch.equal(_sample(circ, pe, seeds)[0], base)
    circ.set_lora([(_dyadic_adapter(_cfg("sd15")), 0.75)])
    assert rel_l2(_sample(circ, pe, seeds)[0], base) > 10 * tol
    circ.set_lora([])
    assert torch.equal(_sample(circ, pe, seeds)[0], base)
    # the image: the whole panorama, decoded by a VAE of the panorama's size
    img = circ.sample(prompt_embeds=pe, seeds=seeds, cfg_guidance=0.6)
    assert img.shape == (2, 3, 8 * PANO[0], 8 * PANO[1]) and torch.isfinite(img).all() and float(img.std()) > 0
    # a callback sees the panorama; a replaced zt is re-gathered (the run differs from the untouched one)
    shapes = []

    def cb(step, t, kw):
        shapes.append(tuple(kw["zt"].shape))
        if step == 0:
            kw["zt"] = kw["zt"] * 0.5
        return kw

    edited = _sample(circ, pe, seeds, callback_fn=cb)[0]
    assert shapes == [(2, 4) + PANO] * STEPS and rel_l2(edited, base) > 10 * tol


def _launches(net, z, t=749.0):
    return sum(v["launches"] for k, v in net.profile(z, t).items())


def test_plain_engine_runs_the_same_launches_and_bits_around_a_panorama_job():
    need_gpu()
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    mk = lambda: get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=5), device="cuda", unet_config=TINY_SD,  # noqa: E731
                            max_batch=4, latent_hw=HW, scalar_semantics="cuda")
    s = mk()
    pe = s.get_text_embed("bad", ["a cat", "a dog"])
    run = lambda sv: [t.clone() for t in sv.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=[5, 6], return_latents=True)]  # noqa: E731
    before = run(s)
    z = torch.randn(2, 4, 16, 16).cuda()
    n0 = _launches(s.engine.unet, z)
    pan = _pano("ddim_panorama_cfg++", "sd15", True, device="cuda", engine=s.engine, text_encoder=s.text_encoder, max_batch=4)
    z0t, zt = _sample(pan, pe, [5, 6])                                # 4 views, 2 chains, 4 rows per half: two forwards per step
    assert torch.isfinite(z0t).all() and z0t.shape == (2, 4) + PANO
    s._ctx_key = None                                                # the panorama job set the engine's context: the next job sets its own
    after = run(s)
    assert _launches(s.engine.unet, z) == n0
    fresh = run(mk())
    for x, y, w in zip(before, after, fresh):
        assert torch.equal(x, y) and torch.equal(x, w)
