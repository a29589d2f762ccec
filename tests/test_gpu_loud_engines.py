"""-m gpu: the HIP engines on the LOUD weights of tests/loud_cases.py against the fp32 oracle, at the tolerances of the existing
engine tests (2.5e-3 for a UNet / ControlNet forward and every residual, 1e-2 for VAE decode, moments and z).  With these weights
every parameter and every conditioning input moves the oracle's output by at least 4 T (tests/test_loud_cases_cpu.py), so an
engine that passes here read every key from the right place in the right layout.  Every forward runs twice: identical bits.  A
failure names the three faults whose oracle change is most collinear with the residual (loud_cases.explain).

Second group: the same loud state dict through every loader route the product has - an iterator of (key, tensor) in another
order next to the dict, fp16 tensors (dtype 1 of cfgpp_unet_load_tensor / cfgpp_vae_load_tensor) next to fp32, the deprecated
VAE attention names with [C, C, 1, 1] weights, the tile tuner off next to on - must give the first route's bits.

Measured on the MI355X: profiles/loud_weights/README.md."""
import pytest
import torch

import loud_cases as L

pytestmark = pytest.mark.gpu
R = 2 * L.ZR
_ENGINES = {}


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def suspects(name, t, got):
    """explain()'s top three for a failing item: the residual against every drop and input fault at this t"""
    e = L.engine(name)
    res = [g.float().cpu() - b for g, b in zip(got, e.base(t))]
    rows = L.explain(res, L.change_table(name, t))
    return "; ".join(f"{label} (cos {c:+.2f}, |res|/|change| {r:.2g})" for label, c, r in rows)


def check(name, t, got, again, weights="loud"):
    """every output finite, twice the same bits, rel-L2 < T against the oracle; returns the rel-L2 per output"""
    from test_gpu_configs import record
    e = L.engine(name, weights)
    base = e.base(t)
    assert len(got) == len(base) == len(again)
    rels = [L.rel_l2(g, b) for g, b in zip(got, base)]
    for n, r in zip(e.output_names(), rels):
        record("loud_engines", engine=name, weights=weights, t=t, output=n, rel_l2=r)
        print(f"{name} [{weights}] t={t} {n}: rel-L2 {r:.3e}")
    if weights != "loud":
        return rels
    for n, g, a, r in zip(e.output_names(), got, again, rels):
        assert g.shape == a.shape and torch.equal(g, a), f"{name} t={t} {n}: two runs, two results"
        ok = bool(torch.isfinite(g.float()).all()) and r < e.T
        assert ok, f"{name} t={t} {n}: rel-L2 {r:.3e} (T = {e.T:g}); suspects: {suspects(name, t, got)}"
    return rels


# ---------------------------------------------------------------------------------------------------- UNets
def build_unet(e, items=None, cfg=None, sd_of="sd"):
    from cfgpp_amd.engine import HipUNet
    net = HipUNet(cfg or e.cfg, R, (L.HW, L.HW)).load_state_dict(items if items is not None else getattr(e, sd_of)).finalize()
    inp = e.inputs
    net.set_context(inp["ehs"], inp.get("te"), inp.get("ti"))
    if "cond" in inp:
        net.image_condition(inp["cond"].cuda())
    if "w_emb" in inp:
        net.guidance_embedding(inp["w_emb"].tolist())
    return net


def unet_of(name, weights="loud"):
    if (name, weights) not in _ENGINES:
        _ENGINES[(name, weights)] = build_unet(L.engine(name, weights))
    return _ENGINES[(name, weights)]


def run_unet(name, t, weights="loud"):
    net, z = unet_of(name, weights), L.engine(name, weights).inputs["z"].cuda()
    got = net.forward(z, t).clone()
    return check(name, t, [got], [net.forward(z, t).clone()], weights)


@pytest.mark.parametrize("t", L.TS)
@pytest.mark.parametrize("name", L.UNETS)
def test_loud_unet_forward_vs_oracle(name, t):
    need_gpu()
    run_unet(name, t)


# ---------------------------------------------------------------------------------------------------- ControlNet
def controlnet_of(weights="loud"):
    from cfgpp_amd.controlnet import HipControlNet
    if ("controlnet", weights) not in _ENGINES:
        e = L.engine("controlnet", weights)
        net = build_unet(e, sd_of="usd")
        cn = HipControlNet(e.cfg, R, (L.HW, L.HW)).load_state_dict(e.sd).finalize()
        cn.set_context(e.inputs["ehs"])
        cn.set_image(e.inputs["img"].cuda())
        net.attach_control(cn, L.CN_SCALE)
        _ENGINES[("controlnet", weights)] = (net, cn)
    return _ENGINES[("controlnet", weights)]


def controlnet_outputs(net, cn, e, t):
    eps = net.forward(e.inputs["z"].cuda(), t).clone()
    return [cn.residual(i, L.CN_SCALE).clone() for i in range(cn.num_residuals())] + [eps]


def run_controlnet(t, weights="loud"):
    net, cn = controlnet_of(weights)
    e = L.engine("controlnet", weights)
    got = controlnet_outputs(net, cn, e, t)
    return check("controlnet", t, got, controlnet_outputs(net, cn, e, t), weights)


@pytest.mark.parametrize("t", L.TS)
def test_loud_controlnet_residuals_and_controlled_forward_vs_oracle(t):
    need_gpu()
    rels = run_controlnet(t)
    assert len(rels) == len(L.engine("controlnet").output_names())


# ---------------------------------------------------------------------------------------------------- VAE
def full_vae_sd(weights="loud"):
    return L.engine("vae_dec", weights).full_sd


def build_vae(sd):
    from cfgpp_amd.vae import HipVAE
    return HipVAE(L.VAE_SCALE, L.VAE_HW, max_batch=1, state_dict=sd)


def vae_of(weights="loud"):
    if ("vae", weights) not in _ENGINES:
        _ENGINES[("vae", weights)] = build_vae(full_vae_sd(weights))
    return _ENGINES[("vae", weights)]


def vae_decode_outputs(hip, e):
    return [hip.decode(e.inputs["z"].cuda()).clone()]


def vae_encode_outputs(hip, e):
    z, mom = hip.encode(e.inputs["img"], noise=e.inputs["noise"], return_moments=True)
    return [mom.clone(), z.clone(), hip.encode(e.inputs["img"], sample=False).clone()]


def run_vae(name, weights="loud"):
    hip, e = vae_of(weights), L.engine(name, weights)
    outs = vae_decode_outputs if name == "vae_dec" else vae_encode_outputs
    got = outs(hip, e)
    return check(name, None, got, outs(hip, e), weights), got


def test_loud_vae_decode_vs_oracle():
    need_gpu()
    _, (img,) = run_vae("vae_dec")
    h, w = L.VAE_HW
    assert img.shape == (1, 3, 8 * h, 8 * w)
    # the folded image post-processing, bit for bit (tests/test_gpu_vae.py)
    z = L.engine("vae_dec").inputs["z"].cuda()
    assert torch.equal(vae_of().decode_image(z), (img / 2 + 0.5).clamp(0, 1))


def test_loud_vae_encode_vs_oracle():
    need_gpu()
    run_vae("vae_enc")


# ---------------------------------------------------------------------------------------------------- loader routes
def _fwd(net, e, t=500.0):
    return net.forward(e.inputs["z"].cuda(), t).clone()


@pytest.mark.parametrize("name", ["tiny_sd", "tiny_xl", "tiny_sd_lcm"])
def test_unet_loader_routes_give_the_same_bits(name):
    """dict / iterator in reversed key order (engine.HipUNet.load_state_dict takes either: the streaming path of
    weights.load_safetensors_iter) / fp16 tensors (load_tensor: dtype 1)"""
    need_gpu()
    e = L.engine(name)
    first = _fwd(unet_of(name), e)
    assert torch.isfinite(first.float()).all()
    stream = _fwd(build_unet(e, items=iter(reversed(list(e.sd.items())))), e)
    assert torch.equal(stream, first)
    half = {k: v.half() for k, v in e.sd.items()}
    assert all(v.dtype == torch.float16 for v in half.values())
    assert torch.equal(_fwd(build_unet(e, items=half), e), first)


def test_controlnet_loader_routes_give_the_same_bits():
    need_gpu()
    from cfgpp_amd.controlnet import HipControlNet
    e = L.engine("controlnet")
    net, cn = controlnet_of()
    first = controlnet_outputs(net, cn, e, 500.0)
    try:
        for items in (iter(reversed(list(e.sd.items()))), {k: v.half() for k, v in e.sd.items()}):
            other = HipControlNet(e.cfg, R, (L.HW, L.HW)).load_state_dict(items).finalize()
            other.set_context(e.inputs["ehs"])
            other.set_image(e.inputs["img"].cuda())
            net.attach_control(other, L.CN_SCALE)
            got = controlnet_outputs(net, other, e, 500.0)
            assert len(got) == len(first) and all(torch.equal(a, b) for a, b in zip(got, first))
    finally:
        net.attach_control(cn, L.CN_SCALE)


def test_unet_output_same_with_the_tile_tuner_on_and_off():
    need_gpu()
    from cfgpp_amd import _lib
    lib = _lib.load()
    e = L.engine("tiny_sd")
    outs = []
    try:
        for tune in (0, 1):
            lib.cfgpp_igemm_set_autotune(tune)
            outs.append(_fwd(build_unet(e), e))
    finally:
        lib.cfgpp_igemm_set_autotune(1)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], _fwd(unet_of("tiny_sd"), e))


def _vae_all(hip):
    return vae_decode_outputs(hip, L.engine("vae_dec")) + vae_encode_outputs(hip, L.engine("vae_enc"))


def test_vae_loader_routes_give_the_same_bits():
    """The VAE's loud weights are not fp16 values and the engine keeps norms, biases and the 4 / 3 / 8-channel convs in fp32, so
    the first route here is the loud state dict rounded through fp16, as fp32 tensors; then the same values as fp16 tensors
    (vae.py: dtype 1), under the deprecated attention names query / key / value / proj_attn with [C, C, 1, 1] weights
    (vae._canonical_vae_key), in reversed key order, and with the tile tuner off."""
    need_gpu()
    from cfgpp_amd import _lib
    from cfgpp_amd.vae import _DEPRECATED_ATTN
    sd = {k: v.half().float() for k, v in full_vae_sd().items()}
    first = _vae_all(build_vae(sd))
    assert all(torch.isfinite(x).all() for x in first)
    # rounding the weights on the host or in the loader is the same rounding, so the loud engine itself agrees where the engine
    # stores fp16; it need not in the fp32-held parameters, hence no comparison with vae_of() here
    half = {k: v.half() for k, v in sd.items()}
    old = {}
    for k, v in sd.items():
        for new_name, old_name in ((n, o) for o, n in _DEPRECATED_ATTN.items()):
            if ".attentions." in k and new_name in k:
                k = k.replace(new_name, old_name)
                if v.dim() == 2:
                    v = v[:, :, None, None].contiguous()
                break
        old[k] = v
    assert sum(".query." in k or ".key." in k or ".value." in k or ".proj_attn." in k for k in old) == 16 and len(old) == len(sd)
    assert old["decoder.mid_block.attentions.0.proj_attn.weight"].shape == (512, 512, 1, 1)
    routes = {"fp16 tensors": half, "deprecated names": old, "reversed order": dict(reversed(list(sd.items())))}
    for label, items in routes.items():
        got = _vae_all(build_vae(items))
        assert all(torch.equal(a, b) for a, b in zip(got, first)), label
    lib = _lib.load()
    try:
        lib.cfgpp_igemm_set_autotune(0)
        got = _vae_all(build_vae(sd))
    finally:
        lib.cfgpp_igemm_set_autotune(1)
    assert all(torch.equal(a, b) for a, b in zip(got, first)), "tile tuner off"
