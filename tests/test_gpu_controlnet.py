"""-m gpu: ControlNet on the MI355X - the conditioning-embedding convolutions against an fp32 torch conv chain, conv_in's
addend, the multi-tensor residual add (bit-exact against torch-ROCm), ControlNet residuals and controlled UNet forwards of
TINY nets against the CPU restatement (tests/controlnet_ref.py), controlled chains against the mock chain, graph replay
staying eager, and one real-size SD1.5 ControlNet + UNet forward against a committed fp32 fixture."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS_REL = 2.5e-3            # tests/test_gpu_unet.py


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------------- embedding convolutions
@pytest.mark.parametrize("S,rows", [(128, 1), (128, 3), (512, 1), (512, 2)])
def test_embedding_convs_vs_fp32_torch_chain(S, rows):
    need_gpu()
    import hip_ops as HO
    g = torch.Generator().manual_seed(S + rows)
    e = (16, 32, 96, 256)
    layers = [(3, e[0], 1)]
    for i in range(3):
        layers += [(e[i], e[i], 1), (e[i], e[i + 1], 2)]
    img = torch.rand(rows, 3, S, S, generator=g)
    ws = [((torch.randn(co, ci, 3, 3, generator=g) / (9 * ci) ** 0.5).half().float(), (torch.randn(co, generator=g) * 0.05).half().float())
          for ci, co, _ in layers]
    keep = []
    x_dev, kind, h = img.cuda(), 2, S
    for li, ((ci, co, st), (w, b)) in enumerate(zip(layers, ws)):
        ho = (h - 1) // st + 1
        last = li == len(layers) - 1
        out = HO.empty_pn(rows, ho, ho, co) if last else torch.empty(rows, ho, ho, co, dtype=torch.float16, device="cuda")
        wk = w.permute(2, 3, 1, 0).reshape(9 * ci, co).contiguous().cuda()
        bd = b.cuda()
        keep += [wk, bd, out]
        HO.check(HO.lib().cfgpp_op_cn_conv3x3(HO.P(x_dev), kind, HO.P(out), int(last), HO.P(wk), HO.P(bd), rows, ci, co, h, h, st, 1,
                                              HO.stream()), "cfgpp_op_cn_conv3x3")
        x_dev, kind, h = out, 0, ho
    got = x_dev[:, 1:h + 1, 1:h + 1, :].permute(0, 3, 1, 2).float().cpu()
    assert torch.all(x_dev[:, 0] == 0) and torch.all(x_dev[:, :, 0] == 0)        # the halo is not touched
    ref = img.half().float()
    for (ci, co, st), (w, b) in zip(layers, ws):
        ref = F.silu(F.conv2d(ref, w, b, stride=st, padding=1))
    assert rel_l2(got, ref) < EPS_REL, rel_l2(got, ref)


def test_conv_in_zero_addend_gives_todays_bits():
    need_gpu()
    import hip_ops as HO
    R, zB, H, W, Cout = 4, 2, 24, 20, 128
    g = torch.Generator().manual_seed(7)
    z = torch.randn(zB, 4, H, W, generator=g).cuda()
    wk = (torch.randn(36, Cout, generator=g) * 0.2).cuda()
    b = (torch.randn(Cout, generator=g) * 0.1).cuda()
    zero = HO.empty_pn(1, H, W, Cout)
    add = HO.to_pn(torch.randn(2, Cout, H, W, generator=g))
    o1, o2, o3 = HO.empty_pn(R, H, W, Cout), HO.empty_pn(R, H, W, Cout), HO.empty_pn(R, H, W, Cout)
    HO.check(HO.lib().cfgpp_op_conv_in(HO.P(z), 0, HO.P(o1), HO.P(wk), HO.P(b), R, zB, 4, H, W, Cout, HO.stream()), "conv_in")
    HO.check(HO.lib().cfgpp_op_conv_in_add(HO.P(z), 0, None, 1, 0, HO.P(zero), 1, HO.P(o2), HO.P(wk), HO.P(b), R, zB, 4, H, W, Cout,
                                           HO.stream()), "conv_in_add")
    HO.check(HO.lib().cfgpp_op_conv_in_add(HO.P(z), 0, None, 1, 0, HO.P(add), 2, HO.P(o3), HO.P(wk), HO.P(b), R, zB, 4, H, W, Cout,
                                           HO.stream()), "conv_in_add")
    assert torch.equal(o1, o2)
    rows = (torch.arange(R) % zB) % 2
    assert torch.equal(o3, (o1.float() + add[rows].float()).half())              # fp16 sample + fp16 embedding


# ---------------------------------------------------------------------------------------------------- residual add
@pytest.mark.parametrize("scale", [1.0, 0.7])
def test_residual_add_is_torch_fp16_s_plus_r_times_scale(scale):
    """bit for bit against torch's fp16 `s + r * scale` with its two roundings: the opmath form written out on the device, and
    torch-CPU fp16 arithmetic (torch-ROCm's own fp16 elementwise kernels do not give one answer: on these inputs its
    non-contiguous and contiguous paths differ from each other in the last bit)"""
    need_gpu()
    import ctypes as C
    import hip_ops as HO
    g = torch.Generator().manual_seed(int(scale * 10))
    rows = 3
    # the last entry has rows * H * W * C / 8 = 552960 units for the launch's 2048 x 256 threads: the grid-stride loop takes a second
    # trip in that entry while the small entries of the same table idle
    shapes = [(32, 32, 64), (16, 16, 128), (8, 8, 128), (5, 7, 64), (96, 96, 160)]
    assert rows * 96 * 96 * 160 // 8 > 2048 * 256
    dst, src, want_cpu = [], [], []
    for H, W, Cc in shapes:
        d = (torch.randn(rows, Cc, H, W, generator=g) * 3).half()
        s = (torch.randn(rows, Cc, H, W, generator=g) * 3).half()
        want_cpu.append(HO.to_pn(d + s * scale))                  # torch-CPU fp16
        dst.append(HO.to_pn(d))
        src.append(HO.to_pn(s))
    want_dev = [(d.float() + (s.float() * scale).half().float()).half() for d, s in zip(dst, src)]    # opmath, two roundings
    n = len(shapes)
    dp = (C.c_void_p * n)(*[d.data_ptr() for d in dst])
    sp = (C.c_void_p * n)(*[s.data_ptr() for s in src])
    hwc = (C.c_int * (3 * n))(*[v for sh in shapes for v in sh])
    HO.check(HO.lib().cfgpp_op_residual_add(dp, sp, hwc, n, rows, float(scale), HO.stream()), "cfgpp_op_residual_add")
    torch.cuda.synchronize()
    for d, wc, wd in zip(dst, want_cpu, want_dev):
        assert torch.equal(d, wc) and torch.equal(d, wd)           # interior bit for bit; the halo is still zero


# ---------------------------------------------------------------------------------------------------- TINY nets
def _tiny(cfg_name, zr=2, image_rows=1, seed=0):
    from cfgpp_amd.controlnet import HipControlNet, synth_controlnet_state_dict
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.unet_config import CONFIGS
    from cfgpp_amd.weights import synth_state_dict
    cfg, hw, R = CONFIGS[cfg_name], 16, 2 * zr
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(zr, 4, hw, hw, generator=g)
    img = torch.rand(image_rows, 3, 8 * hw, 8 * hw, generator=g)
    ehs = (torch.randn(R, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().float()
    te = ti = ack = None
    if cfg.addition_embed:
        te = (torch.randn(R, cfg.addition_pooled_dim, generator=g) * 0.5).half().float()
        ti = torch.tensor([[128.0, 128, 0, 0, 128, 128]] * R)
        ack = {"text_embeds": te, "time_ids": ti}
    usd, csd = synth_state_dict(cfg), synth_controlnet_state_dict(cfg)
    net = HipUNet(cfg, R, (hw, hw)).load_state_dict(usd).finalize()
    cn = HipControlNet(cfg, R, (hw, hw)).load_state_dict(csd).finalize()
    net.set_context(ehs, te, ti)
    cn.set_context(ehs, te, ti)
    return types.SimpleNamespace(cfg=cfg, z=z, img=img, ehs=ehs, te=te, ti=ti, ack=ack, usd=usd, csd=csd, net=net, cn=cn, R=R, zr=zr)


@pytest.mark.parametrize("cfg_name,zr,image_rows,scale", [("tiny_sd", 2, 1, 1.0), ("tiny_sd", 2, 2, 0.7), ("tiny_xl", 1, 1, 0.8)])
def test_controlnet_residuals_and_controlled_forward_vs_restatement(cfg_name, zr, image_rows, scale):
    need_gpu()
    from cfgpp_amd._lib import CfgppError
    from controlnet_ref import ControlNetRef, controlled_unet, image_rows as rows_of
    from oracle.unet_ref import UNetRef
    T = _tiny(cfg_name, zr, image_rows)
    zd = T.z.cuda()
    plain = T.net.forward(zd, 749.0).clone()
    T.net.attach_control(T.cn, scale)
    with pytest.raises(CfgppError, match="control image"):
        T.net.forward(zd, 749.0)                       # attached, no image yet
    T.cn.set_image(T.img.cuda())
    eps = T.net.forward(zd, 749.0).clone()
    zz = T.z[torch.arange(T.R) % zr]
    down, mid = ControlNetRef(T.cfg, T.csd)(zz, 749.0, T.ehs, rows_of(T.img, T.R, zr), scale, T.ack)
    res = down + [mid]
    assert T.cn.num_residuals() == len(res)
    for i, r in enumerate(res):
        got = T.cn.residual(i, scale)
        assert rel_l2(got, r) < EPS_REL, (i, rel_l2(got, r))
    ref = controlled_unet(UNetRef(T.cfg, T.usd), zz, 749.0, T.ehs, T.ack, down, mid)
    assert rel_l2(eps, ref) < EPS_REL, rel_l2(eps, ref)
    assert rel_l2(eps, plain) > 20 * EPS_REL            # the control is not vacuous
    # scale 0, detached, attach-then-detach: the plain engine's bits
    T.net.attach_control(T.cn, 0.0)
    assert torch.equal(T.net.forward(zd, 749.0), plain)
    T.net.attach_control(None, 0.0)
    assert torch.equal(T.net.forward(zd, 749.0), plain)
    T.net.attach_control(T.cn, scale)
    assert torch.equal(T.net.forward(zd, 749.0), eps)   # deterministic
    T.net.attach_control(None, 0.0)
    assert torch.equal(T.net.forward(zd, 749.0), plain)


def test_attach_refuses_mismatch_and_graph_refuses_control():
    need_gpu()
    from cfgpp_amd import _lib
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.controlnet import HipControlNet, synth_controlnet_state_dict
    from cfgpp_amd.unet_config import CONFIGS
    T = _tiny("tiny_sd")
    other = HipControlNet(CONFIGS["tiny_sd"], T.R, (8, 8)).load_state_dict(synth_controlnet_state_dict(CONFIGS["tiny_sd"])).finalize()
    with pytest.raises(CfgppError, match="latent 8 x 8"):
        T.net.attach_control(other, 1.0)
    with pytest.raises(CfgppError, match="ControlNet"):
        T.net.attach_control(T.net, 1.0)
    T.cn.set_image(T.img.cuda())
    T.net.attach_control(T.cn, 1.0)
    z = T.z.cuda()
    z0 = torch.empty_like(z)
    eps = torch.empty(T.R, 4, 16, 16, dtype=torch.float16, device="cuda")
    with pytest.raises(CfgppError, match="ControlNet is attached"):
        T.net.sample_graph_ddim(z, z0, eps, eps[:2], eps[2:], [(749.0, 0.1, 0.9, 0.9, 0.1)], 0.6, False, True)
    assert "sample_graph" in _lib.last_error()


# ---------------------------------------------------------------------------------------------------- chains
def _controlled_fn(cfg):
    from cfgpp_amd.controlnet import synth_controlnet_state_dict
    from cfgpp_amd.weights import synth_state_dict
    from controlnet_ref import ControlNetRef, controlled_unet
    from oracle.unet_ref import UNetRef
    net, cnr = UNetRef(cfg, synth_state_dict(cfg, 0)), ControlNetRef(cfg, synth_controlnet_state_dict(cfg, 0))

    def ack(te, ti):
        return None if te is None else {"text_embeds": te.float(), "time_ids": ti.float()}

    def fn(z, t, ehs, te, ti, cn, rows, scale):
        down, mid = cnr(z.float(), t, ehs.float(), rows, scale, ack(te, ti))
        return controlled_unet(net, z.float(), t, ehs.float(), ack(te, ti), down, mid).half()
    return fn, lambda z, t, ehs, te, ti: net(z.float(), t, ehs.float(), ack(te, ti))["sample"].half()


@pytest.mark.parametrize("model,name,nfe,lam,tol", [("sd15", "ddim_cfg++", 10, 0.6, 3e-3), ("sd15", "dpm++_2m_cfg++", 10, 0.6, 5e-3),
                                                    ("sdxl", "ddim_cfg++", 10, 0.6, 1.5e-3)])
def test_controlled_chain_vs_mock_chain(model, name, nfe, lam, tol, monkeypatch):
    need_gpu()
    from controlnet_mock import ControlMockEngine
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    B, hw = 2, 16
    cfg = TINY_SD if model == "sd15" else TINY_XL
    if model == "sd15":
        from cfgpp_amd.latent_diffusion import get_solver
    else:
        from cfgpp_amd.latent_sdxl import get_solver
    sc = types.SimpleNamespace(num_sampling=nfe)
    hip = get_solver(name, solver_config=sc, device="cuda", unet_config=cfg, max_batch=B, latent_hw=(hw, hw), scalar_semantics="cuda",
                     controlnet="synthetic")
    fn, plain = _controlled_fn(cfg)
    ref = get_solver(name, solver_config=sc, device="cpu", unet_config=cfg, max_batch=B, latent_hw=(hw, hw), scalar_semantics="cuda",
                     text_encoder=hip.text_encoder, engine=ControlMockEngine(plain, fn, (hw, hw)), controlnet="synthetic")
    g = torch.Generator().manual_seed(9)
    img = torch.rand(1, 3, 8 * hw, 8 * hw, generator=g)
    if model == "sd15":
        uc, c = hip.get_text_embed("bad", ["a cat", "a dog"])
        kw = dict(cfg_guidance=lam, seeds=[11, 12], return_latents=True, control_image=img, controlnet_conditioning_scale=0.8)
        a = hip.sample(prompt_embeds=(uc, c), **kw)[0]
        b = ref.sample(prompt_embeds=(uc.cpu(), c.cpu()), **kw)[0]
        uncontrolled = hip.sample(prompt_embeds=(uc, c), cfg_guidance=lam, seeds=[11, 12], return_latents=True)[0]
    else:
        pe = hip.get_text_embed("bad", ["a cat", "a dog"], "bad", ["a cat", "a dog"])
        kw = dict(cfg_guidance=lam, target_size=(128, 128), original_size=(128, 128), seeds=[21, 22], return_latents=True,
                  control_image=img, controlnet_conditioning_scale=0.8)
        a = hip.sample(prompt_embeds=pe, **kw)
        b = ref.sample(prompt_embeds=tuple(x.cpu() for x in pe), **kw)
        kw.pop("control_image")
        uncontrolled = hip.sample(prompt_embeds=pe, **kw)
    assert torch.isfinite(a.float()).all()
    rel = rel_l2(a, b)
    assert rel < tol, f"{model} {name}: controlled chain rel-L2 {rel:.3e}"
    assert rel_l2(a, uncontrolled) > 10 * tol
    assert hip.engine.control is None                  # detached after the call
    if model == "sd15" and name == "ddim_cfg++":       # $CFGPP_GRAPH=1 stays eager while a control is set: the same bits
        monkeypatch.setenv("CFGPP_GRAPH", "1")
        again = hip.sample(prompt_embeds=(uc, c), **kw)[0]
        assert torch.equal(again, a)


def test_controlled_solvers_refuse_inversion_and_edit():
    need_gpu()
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    hip = get_solver("ddim_inversion_cfg++", solver_config=types.SimpleNamespace(num_sampling=2), device="cuda", unet_config=TINY_SD,
                     max_batch=1, latent_hw=(16, 16), controlnet="synthetic")
    with pytest.raises(ValueError, match="control_image"):
        hip.sample(src_img=None, control_image=torch.rand(1, 3, 128, 128))


# ---------------------------------------------------------------------------------------------------- real size
def test_real_sd15_controlnet_forward_vs_oracle_fixture():
    """SD1.5 ControlNet + UNet at 512 x 512 (64 x 64 latent, shipped channel widths), 2 rows, against the fp32 fixture - the
    case where the up path's GroupNorms would otherwise read the skips' pre-add statistics"""
    need_gpu()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "realsize_controlnet.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("REALSIZE_RESULT ")]
    assert line, f"no result (rc={r.returncode}): {r.stdout[-2000:]} {r.stderr[-2000:]}"
    out = json.loads(line[-1].split(" ", 1)[1])
    print(out)
    assert r.returncode == 0 and out["ok"], out
