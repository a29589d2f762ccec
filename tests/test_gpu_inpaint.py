"""-m gpu: inpainting on the MI355X - the masked DDIM step kernel (bit-exact against torch-ROCm), the conv_in gather of
the image condition, 9-channel UNet forwards against the oracle, whole inpaint chains against the CPU restatement
(tests/inpaint_mock.py), graph replay, and one real-size inpaint UNet forward against a committed fp32 fixture."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS_REL = 2.5e-3            # tests/test_gpu_unet.py


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ---------------------------------------------------------------------------------------------------- masked step kernel
# (3, 4, 2, 2): hw = 4, one float4 per (row, channel) and 12 working threads in all; (2, 4, 4, 6): hw = 24, a partial block; (2, 4, 512, 514):
# B * hw = 526336 float4 items for the 2048 x 256 = 524288 threads of the capped grid, a second trip of the grid-stride loop.  The mask
# is drawn per batch row (no two rows share one), and every operand lives between guard elements (tests/test_gpu_small.py) that must
# keep their bits.
@pytest.mark.parametrize("shape", [(8, 4, 64, 64), (3, 4, 24, 40), (3, 4, 2, 2), (2, 4, 4, 6), (2, 4, 512, 514)])
@pytest.mark.parametrize("cfgpp,last", [(True, False), (False, False), (True, True)])
def test_masked_step_matches_torch_where_on_the_device(shape, cfgpp, last):
    need_gpu()
    from cfgpp_amd import engine as E
    from cfgpp_amd.coeffs import ddim_coeffs_pinned
    from cfgpp_amd.schedule import SchedulerTables
    tb = SchedulerTables(50)
    t = tb.timesteps[-1] if last else tb.timesteps[20]
    sq = tb.ddim_sqrt_coeffs(t)
    co = ddim_coeffs_pinned(sq, eps_half=True, semantics="cuda", device_alpha="rn" if last else None)
    a, b = (1.0, 0.0) if last else (sq[2], sq[3])
    g = torch.Generator().manual_seed(sum(shape))
    B, _, h, w = shape
    from test_gpu_small import guarded, guards_intact

    def gin(t):
        buf, v = guarded(tuple(t.shape), t.dtype)
        v.copy_(t.cuda())
        return buf, v
    z = torch.randn(shape, generator=g).cuda()
    (bu, euc), (bc, ec) = gin(torch.randn(shape, generator=g).half()), gin(torch.randn(shape, generator=g).half())
    bs, src = gin((torch.randn(shape, generator=g) * 0.8).half())
    bn, noise = gin(torch.randn(shape, generator=g))
    m = (torch.rand(B, 1, h, w, generator=g) < 0.4).cuda()
    for r in range(1, B):                                   # a mask of its own in every batch row: redraw a row that repeats an earlier one
        while any(torch.equal(m[r], m[q]) for q in range(r)):
            m[r] = (torch.rand(1, h, w, generator=g) < 0.4).cuda()
    assert all(not torch.equal(m[r], m[q]) for r in range(B) for q in range(r))
    mbuf = torch.full((2 * 4096 + m.numel(),), 0xA5, dtype=torch.uint8, device="cuda")       # the mask bytes between guard bytes of their own
    m8 = mbuf[4096:-4096].view(B, 1, h, w)
    m8.copy_(m)
    (bz, zk), (b0, z0k) = guarded(shape, torch.float32), guarded(shape, torch.float32)
    zk.copy_(z)
    E.step_ddim_masked(zk, z0k, euc, ec, 0.6, co, False, cfgpp, m8, src, noise, a, b)
    torch.cuda.synchronize()
    assert all(guards_intact(x) for x in (bz, b0, bu, bc, bs, bn)) and bool((mbuf[:4096] == 0xA5).all()) and bool((mbuf[-4096:] == 0xA5).all())
    assert torch.equal(m8.bool(), m)
    zp, z0p = z.clone(), torch.empty_like(z)
    E.step_ddim(zp, z0p, euc, ec, 0.6, co, False, cfgpp)
    want_z = torch.where(m.bool(), zp, a * src.float() + b * noise)
    want_z0 = torch.where(m.bool(), z0p, src.float())
    assert torch.equal(zk, want_z) and torch.equal(z0k, want_z0)
    zo, z0o = z.clone(), torch.empty_like(z)
    E.step_ddim_masked(zo, z0o, euc, ec, 0.6, co, False, cfgpp, torch.ones_like(m), src, noise, a, b)
    assert torch.equal(zo, zp) and torch.equal(z0o, z0p)           # all ones: exactly cfgpp_step_ddim


# ---------------------------------------------------------------------------------------------------- conv_in with a condition
@pytest.mark.parametrize("R,zB,cond_rows,H,W,Cout,z_half", [(4, 2, 2, 16, 16, 64, False), (2, 1, 1, 64, 64, 320, False),
                                                             (6, 3, 1, 24, 20, 128, True)])
def test_conv_in_with_condition_vs_conv2d(R, zB, cond_rows, H, W, Cout, z_half):
    need_gpu()
    import hip_ops as HO
    g = torch.Generator().manual_seed(R * H + Cout)
    z = torch.randn(zB, 4, H, W, generator=g)
    cond = torch.randn(cond_rows, 5, H, W, generator=g).half()
    w = torch.randn(Cout, 9, 3, 3, generator=g) * 0.2
    bias = torch.randn(Cout, generator=g) * 0.1
    # every device tensor stays referenced until the launch has been enqueued (a freed temporary's block is reused at once)
    zd, cd, bd = (z.half() if z_half else z).cuda(), cond.cuda(), bias.cuda()
    wk = w.permute(2, 3, 1, 0).reshape(81, Cout).cuda().contiguous()
    out = HO.empty_pn(R, H, W, Cout)
    HO.check(HO.lib().cfgpp_op_conv_in_cond(HO.P(zd), int(z_half), HO.P(cd), cond_rows, 5, HO.P(out), HO.P(wk),
                                            HO.P(bd), R, zB, 4, H, W, Cout, HO.stream()), "cfgpp_op_conv_in_cond")
    rows = torch.arange(R) % zB
    x = torch.cat([z.half().float()[rows], cond.float()[rows % cond_rows]], 1)
    ref = torch.nn.functional.conv2d(x, w, bias, padding=1)
    got = out[:, 1:H + 1, 1:W + 1, :].permute(0, 3, 1, 2).float().cpu()
    assert rel_l2(got, ref) < 1e-3
    # no condition: the 4-channel kernel's bits
    w4 = torch.randn(Cout, 4, 3, 3, generator=g) * 0.2
    wk4 = w4.permute(2, 3, 1, 0).reshape(36, Cout).cuda().contiguous()
    o1, o2 = HO.empty_pn(R, H, W, Cout), HO.empty_pn(R, H, W, Cout)
    HO.check(HO.lib().cfgpp_op_conv_in_cond(HO.P(zd), int(z_half), None, 0, 0, HO.P(o1), HO.P(wk4), HO.P(bd), R, zB, 4, H, W,
                                            Cout, HO.stream()), "cfgpp_op_conv_in_cond")
    HO.check(HO.lib().cfgpp_op_conv_in(HO.P(zd), int(z_half), HO.P(o2), HO.P(wk4), HO.P(bd), R, zB, 4, H, W, Cout, HO.stream()),
             "cfgpp_op_conv_in")
    assert torch.equal(o1, o2)


# ---------------------------------------------------------------------------------------------------- 9-channel UNet forward
@pytest.mark.parametrize("cfg_name,zr,cond_rows", [("tiny_sd_inpaint", 2, 2), ("tiny_xl_inpaint", 1, 1), ("tiny_sd_inpaint", 3, 1)])
def test_inpaint_unet_forward_vs_oracle(cfg_name, zr, cond_rows):
    need_gpu()
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.unet_config import CONFIGS
    from cfgpp_amd.weights import synth_state_dict
    from oracle.unet_ref import UNetRef
    cfg, hw, R = CONFIGS[cfg_name], 16, 2 * zr
    sd = synth_state_dict(cfg)
    g = torch.Generator().manual_seed(zr)
    z = torch.randn(zr, 4, hw, hw, generator=g)
    cond = torch.cat([(torch.rand(cond_rows, 1, hw, hw, generator=g) < 0.5).float(), torch.randn(cond_rows, 4, hw, hw, generator=g)], 1).half()
    ehs = (torch.randn(R, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().float()
    ack, te, ti = None, None, None
    if cfg.addition_embed:
        te = (torch.randn(R, cfg.addition_pooled_dim, generator=g) * 0.5).half().float()
        ti = torch.tensor([[128.0, 128, 0, 0, 128, 128]] * R)
        ack = {"text_embeds": te, "time_ids": ti}
    net = HipUNet(cfg, R, (hw, hw))
    net.load_state_dict(sd).finalize()
    net.set_context(ehs, te, ti)
    with pytest.raises(CfgppError, match="image_condition"):
        net.forward(z.cuda(), 749.0)                   # an inpaint engine without its condition
    net.image_condition(cond.cuda())
    eps = net.forward(z.cuda(), 749.0)
    rows = torch.arange(R) % zr
    x = torch.cat([z[rows], cond.float()[rows % cond_rows]], 1)
    ref = UNetRef(cfg, sd)(x, 749.0, ehs, ack)["sample"]
    assert rel_l2(eps, ref) < EPS_REL, rel_l2(eps, ref)
    plain = HipUNet(CONFIGS[cfg_name.replace("_inpaint", "")], R, (hw, hw))
    plain.load_state_dict(synth_state_dict(plain.cfg)).finalize()
    zc = torch.zeros(1, 5, hw, hw, dtype=torch.float16, device="cuda")
    with pytest.raises(CfgppError, match="no image condition"):
        plain.image_condition(zc)
    from cfgpp_amd import _lib
    assert plain.lib.cfgpp_unet_image_condition(plain._h, zc.data_ptr(), 1, torch.cuda.current_stream().cuda_stream) != 0
    assert "not an inpaint UNet" in _lib.last_error()


# ---------------------------------------------------------------------------------------------------- whole chains
class _PinnedNoiseVAE:
    """``solver.encode`` with the posterior noise pinned (the pattern of tests/test_gpu_configs.py): the HIP VAE or the CPU
    restatement, both sampling the SAME posterior point"""

    def __init__(self, kind, scale, hw, B, noise, sd):
        self.noise = noise
        if kind == "hip":
            from cfgpp_amd.vae import HipVAE
            self.v = HipVAE(scale, hw, max_batch=B, state_dict=sd)
            self.enc = lambda x: self.v.encode(x, noise=self.noise[: x.shape[0]])
        else:
            from oracle.vae_ref import VAERef
            self.v = VAERef(scale, device="cpu", dtype=torch.float32, state_dict=sd)

            def enc(x):
                mean, logvar = self.v.encode_moments(x.float().cpu())
                return (mean + torch.exp(0.5 * logvar) * self.noise[: x.shape[0]]) * scale
            self.enc = enc

    def encode(self, x):
        return self.enc(x)

    def decode(self, z):
        return self.v.decode(z)


def _inputs(B, hw, seed=5):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand((B, 3, 8 * hw, 8 * hw), generator=g) * 2 - 1
    noise = torch.randn((B, 4, hw, hw), generator=g)
    mask = torch.zeros(1, 1, 8 * hw, 8 * hw)
    mask[..., 3 * hw:7 * hw, 2 * hw:6 * hw] = 1.0
    return img, noise, mask


def _pair(model, name, cfg, nfe, B, hw, vae_noise):
    """(HIP solver, CPU mock solver) sharing weights, text encoders and the pinned VAE posterior noise"""
    from cfgpp_amd.inpaint import get_inpaint_solver
    from cfgpp_amd.vae import synth_vae_state_dict
    from cfgpp_amd.weights import synth_state_dict
    from inpaint_mock import InpaintMockEngine
    from oracle.unet_ref import UNetRef
    sc = types.SimpleNamespace(num_sampling=nfe)
    hip = get_inpaint_solver(name, model=model, solver_config=sc, device="cuda", unet_config=cfg, max_batch=B, latent_hw=(hw, hw))
    net = UNetRef(cfg, synth_state_dict(cfg, 0))
    if cfg.addition_embed:
        fn = lambda z, t, ehs, te, ti: net(z.float(), t, ehs.float(), {"text_embeds": te.float(), "time_ids": ti.float()})["sample"].half()  # noqa: E731
    else:
        fn = lambda z, t, ehs, te, ti: net(z.float(), t, ehs.float())["sample"].half()  # noqa: E731
    ref = get_inpaint_solver(name, model=model, solver_config=sc, device="cpu", unet_config=cfg, max_batch=B, latent_hw=(hw, hw),
                             text_encoder=hip.text_encoder, engine=InpaintMockEngine(fn, (hw, hw)))
    vsd = synth_vae_state_dict(0)
    hip.vae = _PinnedNoiseVAE("hip", cfg.vae_scale, (hw, hw), B, vae_noise, vsd)
    ref.vae = _PinnedNoiseVAE("cpu", cfg.vae_scale, (hw, hw), B, vae_noise, vsd)
    return hip, ref


@pytest.mark.parametrize("model", ["sd15", "sdxl"])
@pytest.mark.parametrize("name,lam", [("ddim_inpaint_cfg++", 0.6), ("ddim_inpaint", 5.0)])
@pytest.mark.parametrize("nine", [False, True])
def test_inpaint_chain_vs_cpu_restatement(model, name, lam, nine):
    need_gpu()
    from cfgpp_amd.unet_config import TINY_SD, TINY_SD_INPAINT, TINY_XL, TINY_XL_INPAINT
    cfg = {("sd15", False): TINY_SD, ("sd15", True): TINY_SD_INPAINT, ("sdxl", False): TINY_XL, ("sdxl", True): TINY_XL_INPAINT}[(model, nine)]
    B, hw, nfe = 2, 16, 6
    img, vnoise, mask = _inputs(B, hw)
    hip, ref = _pair(model, name, cfg, nfe, B, hw, vnoise)
    kw = dict(cfg_guidance=lam, src_img=img, mask=mask, seeds=[11, 12], return_latents=True)
    if model == "sd15":
        uc, c = hip.get_text_embed("bad", ["a cat", "a dog"])
        a = hip.sample(prompt_embeds=(uc, c), **kw)[0]
        b = ref.sample(prompt_embeds=(uc.cpu(), c.cpu()), **kw)[0]
    else:
        pe = hip.get_text_embed("bad", ["a cat", "a dog"], "bad", ["a cat", "a dog"])
        a = hip.sample(prompt_embeds=pe, **kw)
        b = ref.sample(prompt_embeds=tuple(x.cpu() for x in pe), **kw)
    rel = rel_l2(a, b)
    assert a.shape == (B, 4, hw, hw) and torch.isfinite(a).all() and rel < 1e-2, f"{model} {name} nine={nine}: chain rel-L2 {rel:.3e}"
    if not nine:        # outside the mask the last step leaves the clean source latent, bit for bit
        keep = (torch.nn.functional.interpolate(mask, size=(hw, hw)) < 0.5).expand(B, 4, hw, hw)
        z_src = hip.encode(img).float().cpu()
        assert torch.equal(a.float().cpu()[keep], z_src[keep])


def test_graph_replay_of_inpaint_jobs_equals_eager(monkeypatch):
    """9-channel engine: hipGraph replay == eager loop bit for bit, over two jobs with different conditions on one solver
    (the condition buffer's address is fixed, so the captured graph serves both); 4-channel: CFGPP_GRAPH=1 changes nothing"""
    need_gpu()
    from cfgpp_amd.unet_config import TINY_SD, TINY_SD_INPAINT
    B, hw = 2, 16
    img, vnoise, mask = _inputs(B, hw)
    mask2 = torch.zeros_like(mask)
    mask2[..., :, : 4 * hw] = 1.0
    for cfg in (TINY_SD_INPAINT, TINY_SD):
        hip, _ = _pair("sd15", "ddim_inpaint_cfg++", cfg, 5, B, hw, vnoise)
        uc, c = hip.get_text_embed("bad", ["a cat", "a dog"])
        run = lambda m: hip.sample(cfg_guidance=0.6, prompt_embeds=(uc, c), src_img=img, mask=m, seeds=[3, 4], return_latents=True)  # noqa: E731
        monkeypatch.setenv("CFGPP_GRAPH", "0")
        eager = [run(m) for m in (mask, mask2)]
        monkeypatch.setenv("CFGPP_GRAPH", "1")
        graph = [run(m) for m in (mask, mask2)]
        assert not torch.equal(eager[0][0], eager[1][0])
        for e, gr in zip(eager, graph):
            assert torch.equal(e[0], gr[0]) and torch.equal(e[1], gr[1]), cfg.name
        if cfg is TINY_SD_INPAINT:
            assert hip.engine._g_buf is not None            # the graph path ran
        else:
            assert hip.engine._g_buf is None                # the masked update never replays a graph


# ---------------------------------------------------------------------------------------------------- real size
def test_real_sd15_inpaint_forward_vs_oracle_fixture():
    """synthetic-weight SD15_INPAINT at 512 x 512, 2 rows, against the fp32 fixture of tests/golden/make_inpaint_golden.py
    (own process, own time limit: tests/realsize_inpaint.py)"""
    need_gpu()
    env = dict(os.environ, PYTHONFAULTHANDLER="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "realsize_inpaint.py")], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("REALSIZE_RESULT ")]
    tail = r.stdout[-1500:] + "\n--- stderr ---\n" + r.stderr[-3000:]
    assert lines, f"the child (rc {r.returncode}) printed no result\n{tail}"
    res = json.loads(lines[-1][len("REALSIZE_RESULT "):])
    assert r.returncode == 0 and res["ok"], f"{res}\n{tail}"
