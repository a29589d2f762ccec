"""-m gpu: the HIP UNet and ControlNet engines on the non-square and minimal latents of tests/geometry_cases.py against the fp32 oracle, at
the tolerance of the existing engine tests (T = 2.5e-3 for a UNet / ControlNet forward and every residual).  Every other engine test runs
a square latent, where a plane read with pitch H instead of W is read correctly; at these latents such a fault at any site of the plan
moves the oracle by at least 4 T, and the fp16-activation emulation of the oracle stays within 0.6 T of it
(tests/test_geometry_cases_cpu.py: G1 .. G5).  The degenerate cases run the kernels on 3 x 1, 1 x 3 and 1 x 1 planes and on one-token
attentions.  Every forward runs twice: identical bits.  A failure names the three spatial faults whose oracle change is most collinear
with the residual (geometry_cases.suspects): a swapped pitch names itself.

FreeU, regional prompts and the inpaint condition keep spatial state of their own (twiddle tables and plane sums, a region map per
level, the condition's planes): each once at (8, 24) and (20, 12) on tiny_sd against the reference it already has.  Refusals by message.

Measured on the MI355X: profiles/latent_geometry/README.md."""
import pytest
import torch

import geometry_cases as G
import loud_cases as L

pytestmark = pytest.mark.gpu
_NETS = {}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def check(case, t, got, again):
    """every output of the right shape and finite, twice the same bits, rel-L2 < bound against the oracle; returns the rel-L2 per output"""
    from test_gpu_configs import record
    e = G.engine(case)
    base = e.base(t)
    names = e.output_names()
    assert len(got) == len(base) == len(again) == len(names)
    rels = [L.rel_l2(g, b) for g, b in zip(got, base)]
    for n, r in zip(names, rels):
        record("latent_geometry", case=G.case_id(case), t=t, output=n, rel_l2=r, emulated=G.emulated(case, t))
        print(f"{G.case_id(case)} t={t} {n}: rel-L2 {r:.3e} (emulated {G.emulated(case, t):.3e})")
    bound = G.bound(case, t)
    for n, g, a, b, r in zip(names, got, again, base, rels):
        assert tuple(g.shape) == tuple(b.shape), f"{G.case_id(case)} {n}: shape {tuple(g.shape)}, the oracle's {tuple(b.shape)}"
        assert torch.equal(g, a), f"{G.case_id(case)} t={t} {n}: two runs, two results"
        ok = bool(torch.isfinite(g.float()).all()) and r < bound
        assert ok, f"{G.case_id(case)} t={t} {n}: rel-L2 {r:.3e} (bound {bound:g}); suspects: {G.suspects(case, t, got)}"
    return rels


# ---------------------------------------------------------------------------------------------------- UNets
def build_unet(case):
    from cfgpp_amd.engine import HipUNet
    e = G.engine(case)
    inp = e.inputs
    net = HipUNet(e.cfg, G.R, case.hw, max_tokens=int(inp["ehs"].shape[1])).load_state_dict(e.sd).finalize()
    net.set_context(inp["ehs"], inp.get("te"), inp.get("ti"))
    if "cond" in inp:
        net.image_condition(inp["cond"].cuda())
    if "w_emb" in inp:
        net.guidance_embedding(inp["w_emb"].tolist())
    if case.engine == "freeu":
        net.set_freeu(G.FREEU)
    if case.engine == "regions":
        net.set_regions(inp["ids"], G.N_REGIONS)
    return net


def unet_of(case):
    if case not in _NETS:
        _NETS[case] = build_unet(case)
    return _NETS[case]


def run_unet(case, t):
    net, z = unet_of(case), G.engine(case).inputs["z"].cuda()
    got = net.forward(z, t).clone()
    assert got.shape == (G.R, 4) + tuple(case.hw)
    return got, check(case, t, [got], [net.forward(z, t).clone()])


@pytest.mark.parametrize("t", G.TS)
@pytest.mark.parametrize("case", G.unet_cases(), ids=G.case_id)
def test_unet_forward_vs_oracle(case, t):
    need_gpu()
    run_unet(case, t)


@pytest.mark.parametrize("case", G.FEATURES, ids=G.case_id)
def test_feature_forward_vs_its_reference(case):
    """FreeU against FreeUUNetRef, regions against RegionUNetRef, the inpaint condition through image_condition - at t = 500 and 981;
    and the feature is on: the same engine without it (another condition, for the inpaint UNet) gives another result"""
    need_gpu()
    net, e = unet_of(case), G.engine(case)
    z = e.inputs["z"].cuda()
    for t in G.TS[:2]:
        got, _ = run_unet(case, t)
    try:
        if case.engine == "freeu":
            net.set_freeu(None)
        elif case.engine == "regions":
            net.set_regions(None)
            net.set_context(e.inputs["ehs"][:, :77])
        else:
            net.image_condition(e.inputs["cond"].flip(0).cuda())
        off = net.forward(z, G.TS[1]).clone()
    finally:
        _NETS.pop(case)             # the next user builds it afresh, with the feature on
    assert L.rel_l2(off, got) > 10 * G.T, L.rel_l2(off, got)


# ---------------------------------------------------------------------------------------------------- ControlNet
def controlnet_of(case):
    from cfgpp_amd.controlnet import HipControlNet
    from cfgpp_amd.engine import HipUNet
    if case not in _NETS:
        e = G.engine(case)
        net = HipUNet(e.cfg, G.R, case.hw).load_state_dict(e.usd).finalize()
        net.set_context(e.inputs["ehs"])
        cn = HipControlNet(e.cfg, G.R, case.hw).load_state_dict(e.sd).finalize()
        cn.set_context(e.inputs["ehs"])
        H, W = case.hw
        assert e.inputs["img"].shape[2:] == (8 * H, 8 * W)
        cn.set_image(e.inputs["img"].cuda())
        net.attach_control(cn, G.CN_SCALE)
        _NETS[case] = (net, cn)
    return _NETS[case]


def controlnet_outputs(net, cn, e, t):
    eps = net.forward(e.inputs["z"].cuda(), t).clone()
    return [cn.residual(i, G.CN_SCALE).clone() for i in range(cn.num_residuals())] + [eps]


@pytest.mark.parametrize("t", G.TS)
@pytest.mark.parametrize("case", G.controlnet_cases(), ids=G.case_id)
def test_controlnet_residuals_and_controlled_forward_vs_oracle(case, t):
    need_gpu()
    net, cn = controlnet_of(case)
    e = G.engine(case)
    got = controlnet_outputs(net, cn, e, t)
    rels = check(case, t, got, controlnet_outputs(net, cn, e, t))
    assert len(rels) == len(e.output_names()) == cn.num_residuals() + 1
    assert got[-1].shape == (G.R, 4) + tuple(case.hw)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_sizes():
    need_gpu()
    from cfgpp_amd._lib import CfgppError
    from cfgpp_amd.controlnet import HipControlNet
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    with pytest.raises(CfgppError, match=r"sample size 6 x 8 must be divisible by 2\^\(levels-1\) = 4"):
        HipUNet(TINY_SD, G.R, (6, 8))
    with pytest.raises(CfgppError, match=r"sample size 8 x 7 must be divisible by 2\^\(levels-1\) = 2"):
        HipUNet(TINY_XL, G.R, (8, 7))
    with pytest.raises(CfgppError, match=r"sample size 6 x 8 must be divisible by 2\^\(levels-1\) = 4"):
        HipControlNet(TINY_SD, G.R, (6, 8))
    small = next(c for c in G.DEGENERATE if c.engine == "unet" and c.cfg == "tiny_sd" and c.hw == (4, 4))
    net = unet_of(small)
    with pytest.raises(CfgppError, match=r"set_freeu: up_blocks\.0 runs on 1 x 1 planes"):
        net.set_freeu(G.FREEU)
    assert net.freeu is None
    with pytest.raises(CfgppError, match=r"set_freeu: up_blocks\.0 runs on 3 x 1 planes"):
        unet_of(next(c for c in G.DEGENERATE if c.engine == "unet" and c.hw == (12, 4))).set_freeu(G.FREEU)
    # the refused call left the engine as it was: the same bits as before
    z = G.engine(small).inputs["z"].cuda()
    first = net.forward(z, 500.0).clone()
    with pytest.raises(CfgppError, match=r"1 x 1 planes"):
        net.set_freeu(G.FREEU)
    assert torch.equal(net.forward(z, 500.0), first)
    wide = next(c for c in G.LOUD if c.engine == "controlnet" and c.hw == (8, 24) and c.weights == "synth")
    _, cn = controlnet_of(wide)
    with pytest.raises(CfgppError, match=r"attach_control: latent 8 x 24 vs the UNet's 4 x 4"):
        net.attach_control(cn, G.CN_SCALE)
    tall = unet_of(next(c for c in G.LOUD if c.engine == "unet" and c.cfg == "tiny_sd" and c.hw == (20, 12)))
    with pytest.raises(CfgppError, match=r"attach_control: latent 8 x 24 vs the UNet's 20 x 12"):
        tall.attach_control(cn, G.CN_SCALE)
    with pytest.raises(CfgppError, match=r"expected \[1 or rows, 20, 12\]"):
        tall.set_regions(torch.zeros(1, 12, 20, dtype=torch.long), 2)
    with pytest.raises(CfgppError, match=r"z shape .* != \[\*, 4, 20, 12\]"):
        tall.forward(torch.zeros(2, 4, 12, 20).cuda(), 500.0)
