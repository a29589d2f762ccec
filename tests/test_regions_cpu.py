"""CPU: the host side of regional prompts (cfgpp_amd/regions.py and the solvers' region path) on the mock engine of
tests/mock_region_engine.py: map building, the per-level downsample, context stacking, every refusal by name, --region parsing,
max_regions = 1 making no new call - and the loudness of the engine tests' inputs, shown with the oracle alone."""
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import region_ref as RR
from cfgpp_amd import regions as RG
from mock_region_engine import RegionMockEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (8, 8)
EPS_REL = 2.5e-3            # tests/test_gpu_unet.py


# ---- maps -----------------------------------------------------------------------------------------------------------------------
def test_later_masks_win_and_the_map_starts_at_zero():
    a = torch.zeros(8, 8); a[:, 2:6] = 1
    b = torch.zeros(8, 8); b[3:5, 4:8] = 1
    ids = RG.build_region_map([a, b], HW, 1)
    assert ids.shape == (1, 8, 8) and ids.dtype == torch.long
    assert int(ids[0, 0, 0]) == 0 and int(ids[0, 0, 3]) == 1 and int(ids[0, 3, 5]) == 2 and int(ids[0, 3, 7]) == 2 and int(ids[0, 5, 5]) == 1
    assert torch.equal(RG.build_region_map([b, a], HW, 1)[0, 3, 4:8], torch.tensor([2, 2, 1, 1]))      # the other order: a wins where both are set


def test_pixel_masks_are_binarized_at_half_and_reduced_like_the_inpaint_mask():
    from cfgpp_amd.inpaint import prepare_mask
    g = torch.Generator().manual_seed(3)
    pix = torch.rand((1, 1, 64, 64), generator=g)
    ids = RG.build_region_map([pix], HW, 1)
    _, _, lmask = prepare_mask(pix, torch.zeros(1, 3, 64, 64), HW)
    assert torch.equal(ids[0], lmask[0, 0].long())
    assert torch.equal(ids[0], (pix[0, 0, ::8, ::8] >= 0.5).long())                   # pixel (8i, 8j)
    lat = (torch.rand((2, 8, 8), generator=g))
    ids2 = RG.build_region_map([lat], HW, 2)
    assert ids2.shape == (2, 8, 8) and torch.equal(ids2, (lat >= 0.5).long())


def test_level_maps_are_the_nearest_downsample():
    ids = RR.region_ids("checker", 4, rows=2, hw=16)
    for lvl in (0, 1, 2):
        want = F.interpolate(ids[:, None].float(), size=(16 >> lvl, 16 >> lvl), mode="nearest")[:, 0].long()
        assert torch.equal(RG.level_map(ids, lvl), want)
        ref = RR.RegionUNetRef.__new__(RR.RegionUNetRef)
        ref.set_regions(ids, 4)
        assert torch.equal(ref.level_map(2, (16 >> lvl) ** 2), want.reshape(2, -1))


def test_rect_mask_and_region_parsing():
    m = RG.rect_mask(0.5, 0.0, 1.0, 1.0, (4, 8))
    assert m.shape == (4, 8) and torch.equal(m[0], torch.tensor([0, 0, 0, 0, 1, 1, 1, 1.0]))
    assert float(RG.rect_mask(0.0, 0.25, 1.0, 0.75, (4, 8)).sum()) == 16
    assert RG.parse_region("0.5,0,1,1:a snowy pine, at dusk: blue") == ((0.5, 0.0, 1.0, 1.0), "a snowy pine, at dusk: blue")
    for bad, what in (("0.5,0,1:pine", "x0,y0,x1,y1:prompt"), ("a,b,c,d:pine", "four numbers"), ("0,0,1,1:", "empty prompt"), ("0,0,1,1", "x0,y0,x1,y1:prompt")):
        with pytest.raises(ValueError, match=what):
            RG.parse_region(bad)
    with pytest.raises(ValueError, match=r"0 <= x0 < x1 <= 1"):
        RG.rect_mask(0.6, 0.0, 0.5, 1.0, (4, 8))


def test_context_stacking_repeats_the_negative_prompt():
    uc, c = torch.randn(1, 77, 16), torch.randn(2, 77, 16)
    e1, e2 = torch.randn(2, 77, 16), torch.randn(1, 77, 16)
    suc, sc = RG.stack_context(uc, c, [e1, e2])
    assert suc.shape == (1, 231, 16) and sc.shape == (2, 231, 16)
    for r in range(3):
        assert torch.equal(suc[:, 77 * r: 77 * (r + 1)], uc)
    assert torch.equal(sc[:, :77], c) and torch.equal(sc[:, 77:154], e1) and torch.equal(sc[:, 154:], e2.expand(2, -1, -1))
    with pytest.raises(ValueError, match=r"154 tokens"):
        RG.stack_context(torch.randn(1, 154, 16), None, [e1])


# ---- the solvers' region path on the mock engine -------------------------------------------------------------------------------
def _solver(model="sd15", name="ddim_cfg++", engine=None, **kw):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    mod = __import__("cfgpp_amd.latent_diffusion" if model == "sd15" else "cfgpp_amd.latent_sdxl", fromlist=["get_solver"])
    eng = engine if engine is not None else RegionMockEngine(latent_hw=HW)
    s = mod.get_solver(name, solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", unet_config=TINY_SD if model == "sd15" else TINY_XL,
                       max_batch=2, latent_hw=HW, engine=eng, **kw)
    return s, eng


def _run(s, model, **kw):
    if model == "sd15":
        return s.sample(prompt=["bad", ["a meadow", "a lake"]], cfg_guidance=0.6, seeds=[1, 2], return_latents=True, **kw)
    p = ["bad", ["a meadow", "a lake"]]
    return s.sample(prompt1=p, prompt2=p, cfg_guidance=0.6, target_size=(64, 64), original_size=(64, 64), seeds=[1, 2], return_latents=True, **kw)


MASKS = [RG.rect_mask(0.5, 0.0, 1.0, 1.0, HW), RG.rect_mask(0.25, 0.25, 0.75, 0.75, HW)]


@pytest.mark.parametrize("model", ("sd15", "sdxl"))
def test_sample_stacks_the_context_and_sets_the_map_after_it(model):
    s, eng = _solver(model, max_regions=3)
    _run(s, model, region_prompts=["a snowy pine", ["a red fox", "a hare"]], region_masks=MASKS)
    assert eng.order[:2] == ["context", "regions"] and eng.order.count("context") == 1
    ids, n = eng.region_calls[0]
    assert n == 3 and torch.equal(ids, RG.build_region_map(MASKS, HW, 2))
    ehs = eng.ehs                                               # rows [uc_1, uc_2, c_1, c_2]
    assert ehs.shape[:2] == (4, 231)
    for r in (1, 2):
        assert torch.equal(ehs[:2, 77 * r: 77 * (r + 1)], ehs[:2, :77])          # the negative prompt, repeated
    pine, fox = s._region_hidden("a snowy pine"), s._region_hidden(["a red fox", "a hare"])
    assert torch.equal(ehs[2:, 77:154], pine.expand(2, -1, -1)) and torch.equal(ehs[2:, 154:], fox)
    assert not torch.equal(ehs[2:, :77], ehs[2:, 77:154])
    if model == "sdxl":                                         # the pooled embedding comes from region 0's prompt
        te_plain = _solver(model)[0]
        _run(te_plain, model)
        assert torch.equal(eng.te, te_plain.engine.te)
    # the next plain call on the same solver turns the engine's regions off, after its own context
    _run(s, model)
    assert eng.order[-2:] == ["context", "regions"] and eng.region_calls[-1] == (None, 0) and eng.regions == 0
    _run(s, model, region_prompts=[], region_masks=[])
    assert eng.region_calls[-1] == (None, 0) and len(eng.region_calls) == 2


@pytest.mark.parametrize("model", ("sd15", "sdxl"))
def test_max_regions_1_makes_no_new_call(model):
    class Strict(RegionMockEngine):
        def set_regions(self, *a, **k):
            raise AssertionError("set_regions called on a max_regions=1 solver")
    s, eng = _solver(model, engine=Strict(latent_hw=HW))
    assert s.max_regions == 1
    a = _run(s, model)
    b = _run(s, model, region_prompts=[], region_masks=[])
    la, lb = (a[0], b[0]) if isinstance(a, (tuple, list)) else (a, b)
    assert torch.equal(la, lb) and eng.ehs.shape[1] == 77 and "regions" not in eng.order


@pytest.mark.parametrize("family", ("lcm", "sde", "dpmpp_sde"))
def test_the_other_text_to_image_registries_take_regions(family):
    """get_lcm_solver / get_sde_solver / get_dpmpp_sde_solver build their context through the shared path: the stacked context, then
    the map"""
    from cfgpp_amd.unet_config import TINY_SD
    from mock_engine import StubVAE
    from mock_region_engine import RegionCalls
    if family == "lcm":
        from cfgpp_amd.lcm import get_lcm_solver as get
        from lcm_mock import LCMMockEngine as Base
        name, call = "lcm", dict(guidance_scale=8.5)
    elif family == "sde":
        from cfgpp_amd.sde import get_sde_solver as get
        from sde_mock import SDEMockEngine as Base
        name, call = "dpm++_2m_sde_cfg++", dict(cfg_guidance=0.6)
    else:
        from cfgpp_amd.dpmpp_sde import get_dpmpp_sde_solver as get
        from dpmpp_sde_mock import DPMppSDEMockEngine as Base
        name, call = "dpm++_sde_cfg++", dict(cfg_guidance=0.6)
    eng = type("RegionEngine", (RegionCalls, Base), {})(lambda z, t, ehs, te, ti: (z.float() * 0.9 + 0.01 * ehs.float().mean()).half(), HW)
    s = get(name, model="sd15", solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", unet_config=TINY_SD, max_batch=2,
            latent_hw=HW, engine=eng, vae=StubVAE(TINY_SD.vae_scale), max_regions=2)
    s.sample(prompt=["bad", ["a meadow", "a lake"]], seeds=[1, 2], return_latents=True, region_prompts=["a red fox"], region_masks=MASKS[:1], **call)
    assert eng.order[:2] == ["context", "regions"] and eng.region_calls[0][1] == 2 and eng.ehs.shape[1] == 154
    assert torch.equal(eng.region_calls[0][0], RG.build_region_map(MASKS[:1], HW, 1))


def test_refusals_by_name():
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    base = dict(solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", unet_config=TINY_SD, max_batch=2, latent_hw=HW)
    with pytest.raises(ValueError, match=r"max_regions=2 together with max_prompt_chunks=2"):
        get_solver("ddim", engine=RegionMockEngine(latent_hw=HW), max_regions=2, max_prompt_chunks=2, **base)
    with pytest.raises(ValueError, match=r"max_regions=2 together with ip_adapter"):
        get_solver("ddim", engine=RegionMockEngine(latent_hw=HW), max_regions=2, ip_adapter="synthetic", **base)
    with pytest.raises(ValueError, match=r"max_regions=5: 1 \(off\) .. 4"):
        get_solver("ddim", engine=RegionMockEngine(latent_hw=HW), max_regions=5, **base)
    for name in ("ddim_inversion", "ddim_edit"):
        with pytest.raises(ValueError, match=r"takes no regional prompts"):
            get_solver(name, engine=RegionMockEngine(latent_hw=HW), max_regions=2, **base)
    from cfgpp_amd.inpaint import get_inpaint_solver
    from cfgpp_amd.panorama import get_panorama_solver
    for get, name, extra in ((get_inpaint_solver, "ddim_inpaint", {}), (get_panorama_solver, "ddim_panorama", dict(panorama_hw=(8, 16)))):
        with pytest.raises(ValueError, match=r"takes no regional prompts"):
            get(name, engine=RegionMockEngine(latent_hw=HW), max_regions=2, **extra, **base)
    s, eng = _solver("sd15", max_regions=2)
    with pytest.raises(ValueError, match=r"region_prompts has 2 entries, region_masks 1"):
        _run(s, "sd15", region_prompts=["a", "b"], region_masks=MASKS[:1])
    with pytest.raises(ValueError, match=r"= 3 regions, the solver was built with max_regions=2"):
        _run(s, "sd15", region_prompts=["a", "b"], region_masks=MASKS)
    with pytest.raises(ValueError, match=r"region_masks\[0\]: size \(4, 4\), expected the latent size \(8, 8\) or the pixel size \(64, 64\)"):
        _run(s, "sd15", region_prompts=["a"], region_masks=[torch.ones(4, 4)])
    with pytest.raises(ValueError, match=r"control_image together with region_prompts"):
        _run(s, "sd15", region_prompts=["a"], region_masks=MASKS[:1], control_image=torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match=r"ip_adapter_image_embeds together with region_prompts"):
        _run(s, "sd15", region_prompts=["a"], region_masks=MASKS[:1], ip_adapter_image_embeds=torch.zeros(1, 8))
    assert eng.region_calls == []
    plain, _ = _solver("sd15")
    with pytest.raises(ValueError, match=r"built with max_regions=1"):
        _run(plain, "sd15", region_prompts=["a"], region_masks=MASKS[:1])
    inv = get_solver("ddim_inversion", engine=RegionMockEngine(latent_hw=HW), **base)
    with pytest.raises(ValueError, match=r"does not take region_prompts"):
        inv.sample(src_img=torch.zeros(1, 3, 64, 64), region_prompts=["a"], region_masks=MASKS[:1])


def test_sharded_runs_are_refused(monkeypatch):
    import torch.distributed as dist
    s, eng = _solver("sd15", max_regions=2)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(ValueError, match=r"region_prompts in a sharded run"):
        _run(s, "sd15", region_prompts=["a"], region_masks=MASKS[:1])
    assert eng.region_calls == []


def test_cli_region_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("text_to_img_example", os.path.join(ROOT, "examples", "text_to_img.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    solver = types.SimpleNamespace(latent_hw=HW)
    args = types.SimpleNamespace(region=["0.5,0,1,1:a snowy pine", "0,0,0.5,1:a red fox"], max_regions=3)
    kw = mod._region_kwargs(args, solver)
    assert kw["region_prompts"] == ["a snowy pine", "a red fox"]
    assert torch.equal(kw["region_masks"][0], RG.rect_mask(0.5, 0, 1, 1, HW)) and torch.equal(kw["region_masks"][1], RG.rect_mask(0, 0, 0.5, 1, HW))
    assert mod._region_kwargs(types.SimpleNamespace(region=[], max_regions=1), solver) == {}
    with pytest.raises(SystemExit, match=r"--max_regions 3"):
        mod._region_kwargs(types.SimpleNamespace(region=args.region, max_regions=2), solver)


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_header_and_prototypes_agree():
    """include/cfgpp_regions.h: every declaration has a ctypes prototype in its own table (include/cfgpp.h stays at its size)"""
    from cfgpp_amd import _lib
    from cfgpp_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cfgpp_regions.h")).read()
    declared = set(re.findall(r"\b(cfgpp_[a-z0-9_]+)\s*\(", hdr)) - {"cfgpp_last_error"}       # (named in the header's opening comment)
    assert declared == {"cfgpp_unet_set_regions"} == set(_lib.REGIONS_PROTOTYPES)
    args = re.search(r"cfgpp_unet_set_regions\(([^)]*)\)", hdr).group(1)
    res, argtypes = _lib.REGIONS_PROTOTYPES["cfgpp_unet_set_regions"]
    assert len(argtypes) == args.count(",") + 1
    fn = getattr(lib, "cfgpp_unet_set_regions")
    assert fn.restype == res and list(fn.argtypes) == argtypes
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("PROTOTYPES") and n != "REGIONS_PROTOTYPES"]
    assert not any(set(_lib.REGIONS_PROTOTYPES) & set(o) for o in others)
    assert "cfgpp_op_attention_region" in _lib.DEBUG_PROTOTYPES and hasattr(lib, "cfgpp_op_attention_region")
    assert "cfgpp_unet_set_regions" not in open(os.path.join(ROOT, "include", "cfgpp.h")).read()


# ---- the engine tests' inputs are loud -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RR.NETS)
def test_map_mistakes_are_loud_in_the_oracle(name):
    """regions swapped, the map shifted by one pixel, the level-0 map used undownsampled at the deeper levels: each moves the
    oracle's whole-tensor rel-L2 by at least 10 x EPS_REL on the contexts of region_ref.region_context (figures: profiles/regional/README.md)"""
    from cfgpp_amd.weights import synth_state_dict
    cfg, R = RR.configs()[name]
    sd = synth_state_dict(cfg, 0)
    z = RR.rnd(R // 2, 4, RR.HW, RR.HW, seed=60)
    ack = None
    if cfg.addition_embed:
        ack = {"text_embeds": RR.rnd(R, cfg.addition_pooled_dim, seed=62, scale=0.5), "time_ids": torch.tensor([[128.0, 128.0, 0, 0, 128.0, 128.0]] * R)}
    zz = torch.cat([z] * (R // z.shape[0]))
    ref = RR.RegionUNetRef(cfg, sd)
    for n in (2, 3, 4):
        for kind in ("stripes", "checker"):
            ids, ehs = RR.region_ids(kind, n), RR.region_context(R, n, cfg.cross_attention_dim)
            base = ref.set_regions(ids, n)(zz, 981.0, ehs, ack)["sample"].float()
            for fault in ("swapped", "shifted", "no_downsample"):
                out = ref.set_regions(ids, n, fault)(zz, 981.0, ehs, ack)["sample"].float()
                moved = float((out - base).norm() / base.norm())
                assert moved >= 10 * EPS_REL, (name, n, kind, fault, moved)
