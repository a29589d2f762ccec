"""FreeU inside the HIP UNet (cfgpp_unet_set_freeu, the plan ops of csrc/unet.hip) against the oracle with FreeU applied
(tests/freeu_ref.py: FreeUUNetRef) at the project's forward tolerance; off / (1, 1, 1, 1) / on -> off -> on bit-identity; composition
with a ControlNet; hipGraph replays of DDIM loops under two FreeU states; one short ddim_cfg++ chain per family against the mock."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS_REL = 2.5e-3            # tests/test_gpu_unet.py
FREEU = (0.9, 0.2, 1.5, 1.6)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def _tiny(cfg_name, zr, hw, seed=0):
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.unet_config import CONFIGS
    from cfgpp_amd.weights import synth_state_dict
    cfg, R = CONFIGS[cfg_name], 2 * zr
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(zr, 4, *hw, generator=g)
    ehs = (torch.randn(R, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().float()
    te = ti = ack = None
    if cfg.addition_embed:
        te = (torch.randn(R, cfg.addition_pooled_dim, generator=g) * 0.5).half().float()
        ti = torch.tensor([[128.0, 128, 0, 0, 128, 128]] * R)
        ack = {"text_embeds": te, "time_ids": ti}
    sd = synth_state_dict(cfg)
    net = HipUNet(cfg, R, hw).load_state_dict(sd).finalize()
    net.set_context(ehs, te, ti)
    return types.SimpleNamespace(cfg=cfg, z=z, ehs=ehs, te=te, ti=ti, ack=ack, sd=sd, net=net, R=R, zr=zr, hw=hw)


@pytest.mark.parametrize("cfg_name,zr,hw", [("tiny_sd", 2, (16, 16)), ("tiny_xl", 2, (16, 16)), ("tiny_sd", 2, (16, 24)), ("tiny_xl", 1, (24, 16))])
def test_forward_vs_oracle_and_bit_identity(cfg_name, zr, hw):
    need_gpu()
    import ctypes as C
    from freeu_ref import FreeUUNetRef
    T = _tiny(cfg_name, zr, hw)
    zd = T.z.cuda()
    assert T.net.freeu is None
    plain = T.net.forward(zd, 749.0).clone()
    launches_off = sum(v["launches"] for k, v in T.net.profile(zd, 749.0).items())
    T.net.set_freeu(FREEU)
    assert T.net.freeu == FREEU
    on = T.net.forward(zd, 749.0).clone()
    out = (C.c_int * 5)()
    T.net.lib.cfgpp_freeu_last_launch(out)
    assert out[0] == 1 and out[2] > 0 and out[3] > 0            # the forward ran the kernel, both halves
    assert sum(v["launches"] for k, v in T.net.profile(zd, 749.0).items()) == launches_off + 6
    zz = T.z[torch.arange(T.R) % zr]
    ref = FreeUUNetRef(T.cfg, T.sd, FREEU)(zz, 749.0, T.ehs, T.ack)["sample"]
    ref_plain = FreeUUNetRef(T.cfg, T.sd, None)(zz, 749.0, T.ehs, T.ack)["sample"]
    r_on, r_plain, moved = rel_l2(on, ref), rel_l2(plain, ref_plain), rel_l2(on, plain)
    print(f"{cfg_name} {hw}: FreeU rel-L2 {r_on:.3e}, plain {r_plain:.3e}, FreeU vs plain {moved:.3e}")
    assert torch.isfinite(on.float()).all() and r_on < EPS_REL, r_on
    assert r_plain < EPS_REL, r_plain
    assert moved > 10 * EPS_REL, moved                          # cannot pass with the feature absent
    assert rel_l2(ref, ref_plain) > 10 * EPS_REL
    # off, unit scales, and switching back and forth
    T.net.set_freeu(None)
    assert T.net.freeu is None and torch.equal(T.net.forward(zd, 749.0), plain)
    assert sum(v["launches"] for k, v in T.net.profile(zd, 749.0).items()) == launches_off
    T.net.set_freeu((1, 1, 1, 1))
    assert torch.equal(T.net.forward(zd, 749.0), plain)
    T.net.lib.cfgpp_freeu_last_launch(out)
    assert out[0] == 1                                          # explicit values run the kernel
    T.net.set_freeu(FREEU)
    assert torch.equal(T.net.forward(zd, 749.0), on)
    T.net.set_freeu(dict(s1=0.5, s2=0.5, b1=1.2, b2=1.2))
    other = T.net.forward(zd, 749.0).clone()
    assert not torch.equal(other, on)
    T.net.set_freeu(None)
    assert torch.equal(T.net.forward(zd, 749.0), plain)
    T.net.set_freeu(FREEU)
    assert torch.equal(T.net.forward(zd, 749.0), on)


def test_setter_refusals():
    need_gpu()
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.controlnet import HipControlNet, synth_controlnet_state_dict
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.unet_config import TINY_SD
    from cfgpp_amd.weights import synth_state_dict
    net = HipUNet(TINY_SD, 2, (16, 16))
    with pytest.raises(CfgppError, match="not finalized"):
        net.set_freeu(FREEU)
    net.load_state_dict(synth_state_dict(TINY_SD)).finalize()
    lib = net.lib
    assert lib.cfgpp_unet_set_freeu(net._h, float("inf"), 0.2, 1.5, 1.6, 1) != 0
    from cfgpp_amd import _lib
    assert "non-finite" in _lib.last_error()
    cn = HipControlNet(TINY_SD, 2, (16, 16)).load_state_dict(synth_controlnet_state_dict(TINY_SD)).finalize()
    assert lib.cfgpp_unet_set_freeu(cn._h, 0.9, 0.2, 1.5, 1.6, 1) != 0
    assert "ControlNet-mode" in _lib.last_error()
    assert lib.cfgpp_unet_set_freeu(net._h, float("nan"), 0.2, 1.5, 1.6, 0) == 0       # switching off ignores the values


@pytest.mark.parametrize("cfg_name", ["tiny_sd", "tiny_xl"])
def test_composes_with_controlnet(cfg_name):
    need_gpu()
    from cfgpp_amd.controlnet import HipControlNet, synth_controlnet_state_dict
    from controlnet_ref import ControlNetRef, controlled_unet, image_rows
    from freeu_ref import FreeUUNetRef
    T = _tiny(cfg_name, 2, (16, 16), seed=3)
    csd = synth_controlnet_state_dict(T.cfg)
    cn = HipControlNet(T.cfg, T.R, T.hw).load_state_dict(csd).finalize()
    cn.set_context(T.ehs, T.te, T.ti)
    g = torch.Generator().manual_seed(4)
    img = torch.rand(1, 3, 8 * T.hw[0], 8 * T.hw[1], generator=g)
    cn.set_image(img.cuda())
    zd = T.z.cuda()
    T.net.attach_control(cn, 0.8)
    controlled = T.net.forward(zd, 749.0).clone()
    T.net.set_freeu(FREEU)
    both = T.net.forward(zd, 749.0).clone()
    zz = T.z[torch.arange(T.R) % T.zr]
    down, mid = ControlNetRef(T.cfg, csd)(zz, 749.0, T.ehs, image_rows(img, T.R, T.zr), 0.8, T.ack)
    ref = controlled_unet(FreeUUNetRef(T.cfg, T.sd, FREEU), zz, 749.0, T.ehs, T.ack, down, mid)
    r = rel_l2(both, ref)
    print(f"{cfg_name}: ControlNet + FreeU rel-L2 {r:.3e}")
    assert r < EPS_REL, r
    assert rel_l2(both, controlled) > 10 * EPS_REL
    T.net.set_freeu(None)
    assert torch.equal(T.net.forward(zd, 749.0), controlled)
    T.net.attach_control(None, 0.0)


def _ddim(model, **kw):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    if model == "sd15":
        from cfgpp_amd.latent_diffusion import get_solver
        cfg = TINY_SD
    else:
        from cfgpp_amd.latent_sdxl import get_solver
        cfg = TINY_XL
    return get_solver("ddim_cfg++", unet_config=cfg, max_batch=2, latent_hw=(16, 16), scalar_semantics="cuda", **kw), cfg


def _sample(s, model, pe, seeds):
    if model == "sd15":
        return s.sample(cfg_guidance=0.6, prompt_embeds=pe, seeds=seeds, return_latents=True)[0].clone()
    return s.sample(cfg_guidance=0.6, prompt_embeds=pe, target_size=(128, 128), original_size=(128, 128), seeds=seeds,
                    return_latents=True).clone()


def _embeds(s, model):
    if model == "sd15":
        return s.get_text_embed("bad", ["a cat", "a dog"])
    return s.get_text_embed("bad", ["a cat", "a dog"], "bad", ["a cat", "a dog"])


def test_graph_replay_equals_eager_under_two_freeu_states(monkeypatch):
    """one engine: graph jobs with FreeU A, FreeU B, off, A again - each equals its eager run (a stale graph would show), and the
    states differ from each other"""
    need_gpu()
    s, cfg = _ddim("sd15", solver_config=types.SimpleNamespace(num_sampling=5), device="cuda")
    pe = _embeds(s, "sd15")
    A, B = FREEU, (0.5, 0.6, 1.2, 1.3)
    eager = {}
    monkeypatch.setenv("CFGPP_GRAPH", "0")
    for name, spec in (("A", A), ("B", B), ("off", None)):
        s.set_freeu(spec)
        eager[name] = _sample(s, "sd15", pe, [5, 6])
    assert not torch.equal(eager["A"], eager["B"]) and not torch.equal(eager["A"], eager["off"])
    monkeypatch.setenv("CFGPP_GRAPH", "1")
    for name, spec in (("A", A), ("B", B), ("off", None), ("A", A), ("B", B)):
        s.set_freeu(spec)
        got = _sample(s, "sd15", pe, [5, 6])
        assert torch.equal(got, eager[name]), f"graph job under FreeU state {name} differs from its eager run"


@pytest.mark.parametrize("model,tol", [("sd15", 3e-3), ("sdxl", 1.5e-3)])
def test_chain_vs_mock_chain(model, tol):
    """a 10-step ddim_cfg++ chain with FreeU on the HIP engine against the same solver on a mock engine whose UNet is the oracle
    with FreeU (tolerances: tests/test_gpu_controlnet.py's for these chains)"""
    need_gpu()
    from cfgpp_amd.weights import synth_state_dict
    from freeu_ref import FreeUUNetRef
    from mock_engine import MockEngine
    sc = types.SimpleNamespace(num_sampling=10)
    hip, cfg = _ddim(model, solver_config=sc, device="cuda", freeu=FREEU)
    assert hip.freeu == FREEU

    class FreeUMock(MockEngine):
        freeu = None

        def set_freeu(self, spec):
            self.freeu = spec

    sd = synth_state_dict(cfg, 0)

    def ack(te, ti):
        return None if te is None else {"text_embeds": te.float(), "time_ids": ti.float()}
    eng = FreeUMock(lambda z, t, ehs, te, ti: FreeUUNetRef(cfg, sd, eng.freeu)(z.float(), t, ehs.float(), ack(te, ti))["sample"].half(), (16, 16))
    ref, _ = _ddim(model, solver_config=sc, device="cpu", text_encoder=hip.text_encoder, engine=eng, freeu=FREEU)
    assert eng.freeu == FREEU
    pe = _embeds(hip, model)
    a = _sample(hip, model, pe, [11, 12])
    b = _sample(ref, model, tuple(x.cpu() for x in pe), [11, 12])
    hip.set_freeu(None)
    plain = _sample(hip, model, pe, [11, 12])
    rel = rel_l2(a, b)
    print(f"{model}: FreeU chain rel-L2 {rel:.3e}, vs plain {rel_l2(a, plain):.3e}")
    assert torch.isfinite(a.float()).all() and rel < tol, rel
    assert rel_l2(a, plain) > 10 * tol


# ---------------------------------------------------------------------------------------------------- real size
def test_real_sd15_freeu_forward_vs_oracle_fixture():
    """SD1.5 at 512 x 512 (64 x 64 latent, shipped widths: 8 x 8 and 16 x 16 planes of 1280 / 640 channels), 2 rows, against the
    committed fp32 fixture (tests/golden/make_freeu_golden.py) with the FreeU values stored there; in its own process"""
    need_gpu()
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "realsize_freeu.py")], cwd=root, capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("REALSIZE_RESULT ")]
    assert line, f"no result (rc={r.returncode}): {r.stdout[-2000:]} {r.stderr[-2000:]}"
    out = json.loads(line[-1].split(" ", 1)[1])
    print(out)
    assert r.returncode == 0 and out["ok"], out
