"""The upsampler convolutions in the 2x2 phase form (IGemmArgs::amode 4) inside the engines: tiny UNet and tiny VAE built with
cfgpp_igemm_set_upsample_phase on and off (the switch is read when a plan is built).  Tolerances are the neighbouring tiny-net
tests': eps rel-L2 2.5e-3 (tests/test_gpu_unet.py), image rel-L2 1e-2 (tests/test_gpu_vae.py) - against the oracle, and between
the two engines."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS_REL = 2.5e-3
IMG_REL = 1e-2
UP_KEY = "up_blocks.1.upsamplers.0.conv.weight"


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


def _build_unet(on, cfg, sd, rows, hw, ctx):
    from cfgpp_amd import _lib
    from cfgpp_amd.engine import HipUNet
    lib = _lib.load()
    lib.cfgpp_igemm_set_upsample_phase(1 if on else 0)
    try:
        net = HipUNet(cfg, rows, (hw, hw))
        net.load_state_dict(sd).finalize()
    finally:
        lib.cfgpp_igemm_set_upsample_phase(1)
    net.set_context(ctx)
    return net


@pytest.fixture(scope="module")
def unets():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from cfgpp_amd.unet_config import TINY_SD as cfg
    from cfgpp_amd.weights import synth_state_dict
    from oracle.unet_ref import UNetRef
    rows, hw = 4, 32                    # three levels: the upsamplers read 8 x 8 and 16 x 16 maps - both take the phase form
    sd = synth_state_dict(cfg)
    g = torch.Generator().manual_seed(21)
    ctx = (torch.randn(rows, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().float()
    z = torch.randn(rows, 4, hw, hw, generator=g)
    ref = UNetRef(cfg, sd)(z, 500.0, ctx)["sample"]
    on = _build_unet(True, cfg, sd, rows, hw, ctx)
    off = _build_unet(False, cfg, sd, rows, hw, ctx)
    return dict(on=on, off=off, z=z.cuda(), ref=ref, cfg=cfg)


def test_unet_plans_differ_only_in_the_upsampler_launches(unets):
    d_on = unets["on"].profile(unets["z"], 500.0, detail=True)["detail"]
    d_off = unets["off"].profile(unets["z"], 500.0, detail=True)["detail"]
    up_on = [ln.split("\t")[2] for ln in d_on.splitlines() if "as 4x2x2" in ln]
    assert len(up_on) == 2 and all("amode=4" in s and "K=1152 as 4x2x2 K=512" in s for s in up_on), up_on
    assert "4x2x2" not in d_off and sum("amode=3" in ln for ln in d_off.splitlines()) == 2
    # the tags keep the operation's algorithmic MACs: the flops a forward reports do not move
    assert unets["on"].flops(4) == unets["off"].flops(4)


def test_unet_forward_on_off_and_oracle(unets):
    a = unets["on"].forward(unets["z"], 500.0).clone()
    b = unets["off"].forward(unets["z"], 500.0).clone()
    r_on, r_off, r_ab = _rel(a, unets["ref"]), _rel(b, unets["ref"]), _rel(a, b)
    print(f"tiny_sd 4 rows @ 32x32: phase form vs oracle {r_on:.3e}, 9-tap vs oracle {r_off:.3e}, phase vs 9-tap {r_ab:.3e}")
    assert torch.isfinite(a.float()).all()
    assert r_on < EPS_REL and r_off < EPS_REL and r_ab < EPS_REL
    assert torch.equal(unets["on"].forward(unets["z"], 500.0), a)


def test_folded_weights_follow_a_lora_merge_and_unmerge(unets):
    on, off, z = unets["on"], unets["off"], unets["z"]
    base = on.forward(z, 500.0).clone()
    g = torch.Generator().manual_seed(22)
    O, K = 128, 128 * 9
    up, down = torch.randn(O, 4, generator=g) * 0.2, torch.randn(4, K, generator=g) * 0.2
    try:
        on.lora(UP_KEY, up, down)
        off.lora(UP_KEY, up, down)
        assert torch.equal(on.read_weight(UP_KEY), off.read_weight(UP_KEY))      # the 3x3 slot stays the merge target
        a, b = on.forward(z, 500.0).clone(), off.forward(z, 500.0).clone()
        moved, r_ab = _rel(a, base), _rel(a, b)
        print(f"merge moved eps by {moved:.3e}; merged phase form vs merged 9-tap {r_ab:.3e}")
        assert r_ab < EPS_REL
        assert moved > 10 * EPS_REL                                              # the folded copy followed the merge
    finally:
        on.lora(UP_KEY, None, None)
        off.lora(UP_KEY, None, None)
    assert torch.equal(on.forward(z, 500.0), base)                                # ... and the unmerge, bit for bit


def test_vae_decode_on_off_and_oracle():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from cfgpp_amd import _lib
    from cfgpp_amd.vae import HipVAE, synth_vae_state_dict
    from oracle.vae_ref import VAERef
    lib = _lib.load()
    sd = synth_vae_state_dict(0)
    hw, B = (16, 16), 2                 # the three upsamplers read 16 x 16, 32 x 32 and 64 x 64 maps
    g = torch.Generator().manual_seed(23)
    z = torch.randn((B, 4) + hw, generator=g) * 0.18215 * 1.5
    imgs = {}
    for on in (1, 0):
        lib.cfgpp_igemm_set_upsample_phase(on)
        try:
            vae = HipVAE(0.18215, hw, max_batch=B, state_dict=sd)
        finally:
            lib.cfgpp_igemm_set_upsample_phase(1)
        imgs[on] = vae.decode(z.cuda()).cpu()
        if on:
            assert torch.equal(vae.decode(z.cuda()).cpu(), imgs[on])
        del vae
    ref = VAERef(0.18215, device="cpu", dtype=torch.float32, state_dict=sd).decode(z)
    r_on, r_off, r_ab = _rel(imgs[1], ref), _rel(imgs[0], ref), _rel(imgs[1], imgs[0])
    print(f"tiny VAE decode: phase form vs oracle {r_on:.3e}, 9-tap vs oracle {r_off:.3e}, phase vs 9-tap {r_ab:.3e}")
    assert torch.isfinite(imgs[1]).all() and r_on < IMG_REL and r_off < IMG_REL and r_ab < IMG_REL
