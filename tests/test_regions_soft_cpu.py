"""CPU: the host side of soft regional prompts and per-region negative prompts (cfgpp_amd/regions.py and the solvers' region path) on
the mock engine of tests/region_soft_ref.py: the weights against hand-written expectations, the level downsample, the negative
context layout, every refusal by name, the command line's parsing, and the loudness of the engine tests' inputs with the oracle
alone."""
import os
import types

import pytest
import torch
import torch.nn.functional as F

import region_ref as RR
import region_soft_ref as SR
from cfgpp_amd import regions as RG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (8, 8)
EPS_REL = 2.5e-3            # tests/test_gpu_unet.py


# ---- weights --------------------------------------------------------------------------------------------------------------------
def test_layer_compositing_by_hand():
    a = torch.zeros(8, 8); a[:, 2:6] = 0.5
    b = torch.zeros(8, 8); b[3:5, 4:8] = 0.25
    w = RG.build_region_weights([a, b], HW, 1)
    assert w.shape == (1, 3, 8, 8) and w.dtype == torch.float32
    assert w[0, :, 0, 0].tolist() == [1.0, 0.0, 0.0]                      # outside both
    assert w[0, :, 0, 3].tolist() == [0.5, 0.5, 0.0]                      # a only
    assert w[0, :, 3, 5].tolist() == [0.375, 0.375, 0.25]                 # both: b on top scales what lies under it by 0.75
    assert w[0, :, 3, 7].tolist() == [0.75, 0.0, 0.25]                    # b only
    wb = RG.build_region_weights([a, b], HW, 1, base_ratio=0.2)
    assert torch.allclose(wb[0, :, 3, 5], torch.tensor([0.2 + 0.8 * 0.375, 0.8 * 0.375, 0.8 * 0.25]), atol=1e-7)
    for x in (w, wb):
        assert float((x.sum(1) - 1).abs().max()) < 1e-6 and bool((x >= 0).all())


def test_binary_masks_give_the_one_hot_map_and_later_masks_win():
    g = torch.Generator().manual_seed(5)
    masks = [(torch.rand((2, 8, 8), generator=g) < 0.4).float() for _ in range(3)]
    w = RG.build_region_weights(masks, HW, 2)
    ids = RG.build_region_map(masks, HW, 2)
    assert torch.equal(w, F.one_hot(ids, 4).permute(0, 3, 1, 2).float())


def test_base_ratio_one_is_region_zero_alone():
    w = RG.build_region_weights([torch.rand(8, 8), torch.rand(8, 8)], HW, 1, base_ratio=1.0)
    assert torch.equal(w[:, 0], torch.ones(1, 8, 8)) and float(w[:, 1:].abs().max()) == 0.0


def test_soft_masks_are_not_binarized_and_pixel_masks_take_pixel_8i_8j():
    g = torch.Generator().manual_seed(3)
    pix = torch.rand((1, 1, 64, 64), generator=g)
    w = RG.build_region_weights([pix], HW, 1)
    assert torch.equal(w[0, 1], pix[0, 0, ::8, ::8]) and torch.equal(w[0, 0], 1.0 - pix[0, 0, ::8, ::8])
    lat = torch.rand((2, 8, 8), generator=g)
    assert torch.equal(RG.build_region_weights([lat], HW, 2)[:, 1], lat)


def test_level_weights_are_the_nearest_downsample():
    w = SR.region_weights("mixed", 4, rows=2, hw=16)
    for lvl in (0, 1, 2):
        want = F.interpolate(w, size=(16 >> lvl, 16 >> lvl), mode="nearest")
        assert torch.equal(RG.level_weights(w, lvl), want)
        ref = SR.SoftRegionUNetRef.__new__(SR.SoftRegionUNetRef)
        ref.set_region_weights(w)
        assert torch.equal(ref.level_weights((16 >> lvl) ** 2), want)
    for kind in ("onehot", "feather", "mixed"):
        x = SR.region_weights(kind, 3)
        assert x.shape == (1, 3, 16, 16) and float((x.sum(1) - 1).abs().max()) < 1e-6 and bool((x >= 0).all())


def test_soft_rect_mask():
    for rect in ((0.5, 0.0, 1.0, 1.0), (0.25, 0.25, 0.75, 0.75), (0.0, 0.0, 1.0, 0.5)):
        assert torch.equal(RG.soft_rect_mask(*rect, (8, 16), 0.0), RG.rect_mask(*rect, (8, 16)))
    m = RG.soft_rect_mask(0.5, 0.0, 1.0, 1.0, (8, 16), 0.5)                  # ramp 4 latent pixels wide (0.5 x 8) centred on x = 0.5
    row = m[4]
    want = torch.tensor([0, 0, 0, 0, 0, 0, 0.125, 0.375, 0.625, 0.875, 1, 1, 1, 1, 0.875, 0.625])       # the image border is an edge too
    assert torch.allclose(row, want, atol=1e-6)
    assert abs(float(row[7]) + float(row[8]) - 1.0) < 1e-6                    # 0.5 on the edge: symmetric about it
    assert torch.allclose(m[:, 12], torch.tensor([0.625, 0.875, 1, 1, 1, 1, 0.875, 0.625]), atol=1e-6)       # y: 4 pixels wide as well
    assert 0.0 <= float(m.min()) and float(m.max()) <= 1.0
    with pytest.raises(ValueError, match="feather=1.5"):
        RG.soft_rect_mask(0, 0, 1, 1, (8, 8), 1.5)


def test_weight_refusals():
    with pytest.raises(ValueError, match=r"region_base_ratio=1.5"):
        RG.build_region_weights([torch.zeros(8, 8)], HW, 1, 1.5)
    with pytest.raises(ValueError, match=r"soft masks hold values in \[0, 1\]"):
        RG.build_region_weights([torch.full((8, 8), 1.5)], HW, 1)
    with pytest.raises(ValueError, match=r"4 masks"):
        RG.build_region_weights([torch.zeros(8, 8)] * 4, HW, 1)
    with pytest.raises(ValueError, match=r"expected the latent size \(8, 8\)"):
        RG.build_region_weights([torch.zeros(4, 4)], HW, 1)
    with pytest.raises(ValueError, match=r"3 rows for a batch of 2"):
        RG.build_region_weights([torch.zeros(3, 8, 8)], HW, 2)


# ---- negative prompts -----------------------------------------------------------------------------------------------------------
def test_negative_context_layout():
    uc, c = torch.randn(1, 77, 16), torch.randn(2, 77, 16)
    e1, e2 = torch.randn(2, 77, 16), torch.randn(1, 77, 16)
    n2 = torch.randn(2, 77, 16)
    plain = RG.stack_context(uc, c, [e1, e2])
    again = RG.stack_context(uc, c, [e1, e2], negative_embeds=None)
    assert torch.equal(plain[0], again[0]) and torch.equal(plain[1], again[1])        # without the keyword: exactly as before
    suc, sc = RG.stack_context(uc, c, [e1, e2], negative_embeds=[None, n2])
    assert torch.equal(sc, plain[1]) and suc.shape == (2, 231, 16)
    assert torch.equal(suc[:, :77], uc.expand(2, -1, -1)) and torch.equal(suc[:, 77:154], uc.expand(2, -1, -1)) and torch.equal(suc[:, 154:], n2)
    with pytest.raises(ValueError, match=r"region_negative_prompts has 1 entries, region_prompts 2"):
        RG.stack_context(uc, c, [e1, e2], negative_embeds=[n2])
    assert RG.check_negatives(None, 2) is None and RG.check_negatives([None, None], 2) is None
    assert RG.check_negatives([None, "blurry"], 2) == [None, "blurry"]
    with pytest.raises(ValueError, match=r"region_negative_prompts has 1 entries, region_prompts 2"):
        RG.check_negatives(["x"], 2)
    assert RG.parse_region_negative("2:blurry, low: quality", 2) == (2, "blurry, low: quality")
    for bad in ("3:x", "0:x", "x", "1:"):
        with pytest.raises(ValueError, match="--region_negative"):
            RG.parse_region_negative(bad, 2)


# ---- the solvers' region path on the mock engine -------------------------------------------------------------------------------
def _solver(model="sd15", name="ddim_cfg++", engine=None, get=None, **kw):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    mod = __import__("cfgpp_amd.latent_diffusion" if model == "sd15" else "cfgpp_amd.latent_sdxl", fromlist=["get_solver"])
    eng = engine if engine is not None else SR.SoftRegionMockEngine(latent_hw=HW)
    s = mod.get_solver(name, solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", unet_config=TINY_SD if model == "sd15" else TINY_XL,
                       max_batch=2, latent_hw=HW, engine=eng, **kw)
    return s, eng


def _run(s, model, **kw):
    if model == "sd15":
        return s.sample(prompt=["bad", ["a meadow", "a lake"]], cfg_guidance=0.6, seeds=[1, 2], return_latents=True, **kw)
    p = ["bad", ["a meadow", "a lake"]]
    return s.sample(prompt1=p, prompt2=p, cfg_guidance=0.6, target_size=(64, 64), original_size=(64, 64), seeds=[1, 2], return_latents=True, **kw)


SOFT = [RG.soft_rect_mask(0.5, 0.0, 1.0, 1.0, HW, 0.5), RG.soft_rect_mask(0.25, 0.25, 0.75, 0.75, HW, 0.25)]
HARD = [RG.rect_mask(0.5, 0.0, 1.0, 1.0, HW), RG.rect_mask(0.25, 0.25, 0.75, 0.75, HW)]


@pytest.mark.parametrize("model", ("sd15", "sdxl"))
def test_soft_solver_sets_weights_after_the_context(model):
    s, eng = _solver(model, max_regions=3, soft_regions=True)
    _run(s, model, region_prompts=["a snowy pine", ["a red fox", "a hare"]], region_masks=SOFT, region_base_ratio=0.3)
    assert eng.order[:2] == ["context", "weights"] and eng.order.count("context") == 1 and not eng.region_calls
    assert torch.equal(eng.weight_calls[0], RG.build_region_weights(SOFT, HW, 2, 0.3)) and eng.regions == 3
    assert eng.ehs.shape[:2] == (4, 231)
    # 0/1 masks on a soft solver: still the weights call (the documented way onto the soft kernel), one-hot
    _run(s, model, region_prompts=["a snowy pine", "a red fox"], region_masks=HARD)
    assert torch.equal(eng.weight_calls[-1], F.one_hot(RG.build_region_map(HARD, HW, None), 3).permute(0, 3, 1, 2).float())
    # the next plain call turns the weights off, after its own context
    _run(s, model)
    assert eng.order[-2:] == ["context", "weights"] and eng.weight_calls[-1] is None and eng.regions == 0


@pytest.mark.parametrize("soft", (False, True))
def test_per_region_negative_prompts_change_the_unconditional_rows_only(soft):
    kw = dict(max_regions=3, soft_regions=True) if soft else dict(max_regions=3)
    s, eng = _solver("sd15", **kw)
    masks = SOFT if soft else HARD
    _run(s, "sd15", region_prompts=["a snowy pine", "a red fox"], region_masks=masks)
    plain = eng.ehs.clone()
    _run(s, "sd15", region_prompts=["a snowy pine", "a red fox"], region_masks=masks, region_negative_prompts=[None, "blurry"])
    ehs = eng.ehs                                               # rows [uc_1, uc_2, c_1, c_2]
    assert torch.equal(ehs[2:], plain[2:])                      # the conditional rows: untouched
    assert torch.equal(ehs[:2, :154], plain[:2, :154])          # uc | uc (None = the job's negative prompt)
    assert torch.equal(ehs[:2, 154:], s._region_hidden("blurry").expand(2, -1, -1)) and not torch.equal(ehs[:2, 154:], plain[:2, 154:])
    _run(s, "sd15", region_prompts=["a snowy pine", "a red fox"], region_masks=masks, region_negative_prompts=[None, None])
    assert torch.equal(eng.ehs, plain)


@pytest.mark.parametrize("family", ("lcm", "sde", "dpmpp_sde"))
def test_the_other_text_to_image_registries_take_soft_regions(family):
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
    eng = type("SoftEngine", (SR.WeightCalls, RegionCalls, Base), {})(lambda z, t, ehs, te, ti: (z.float() * 0.9 + 0.01 * ehs.float().mean()).half(), HW)
    s = get(name, model="sd15", solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", unet_config=TINY_SD, max_batch=2,
            latent_hw=HW, engine=eng, vae=StubVAE(TINY_SD.vae_scale), max_regions=3, soft_regions=True)
    assert s.soft_regions and s.max_regions == 3
    s.sample(prompt=["bad", ["a meadow", "a lake"]], seeds=[1, 2], return_latents=True, region_prompts=["a snowy pine", "a red fox"],
             region_masks=SOFT, region_base_ratio=0.25, **call)
    assert eng.order[:2] == ["context", "weights"] and eng.ehs.shape[1] == 231 and "regions" not in eng.order
    assert torch.equal(eng.weight_calls[0], RG.build_region_weights(SOFT, HW, None, 0.25))


def test_solver_refusals_name_what_they_refuse():
    hard, _ = _solver("sd15", max_regions=3)
    with pytest.raises(ValueError, match=r"region_base_ratio=0.3 needs a soft-regions solver: get_solver\(\.\.\., max_regions=R, soft_regions=True\)"):
        _run(hard, "sd15", region_prompts=["a pine"], region_masks=HARD[:1], region_base_ratio=0.3)
    with pytest.raises(ValueError, match=r"region_negative_prompts has 2 entries, region_prompts 1"):
        _run(hard, "sd15", region_prompts=["a pine"], region_masks=HARD[:1], region_negative_prompts=["x", "y"])
    with pytest.raises(ValueError, match=r"without region_prompts"):
        _run(hard, "sd15", region_base_ratio=0.3)
    with pytest.raises(ValueError, match=r"region_base_ratio=-0.1"):
        _run(hard, "sd15", region_prompts=["a pine"], region_masks=HARD[:1], region_base_ratio=-0.1)
    with pytest.raises(ValueError, match=r"soft_regions=True needs max_regions=R"):
        _solver("sd15", soft_regions=True)
    soft, _ = _solver("sd15", max_regions=2, soft_regions=True)
    with pytest.raises(ValueError, match=r"soft masks hold values in \[0, 1\]"):
        _run(soft, "sd15", region_prompts=["a pine"], region_masks=[torch.full(HW, 2.0)])
    with pytest.raises(ValueError, match=r"3 regions, the solver was built with max_regions=2"):
        _run(soft, "sd15", region_prompts=["a", "b"], region_masks=SOFT)
    with pytest.raises(ValueError, match=r"control_image together with region_prompts"):
        _run(soft, "sd15", region_prompts=["a"], region_masks=SOFT[:1], control_image=torch.zeros(1, 3, 64, 64))
    from cfgpp_amd.latent_diffusion import get_solver
    for name in ("ddim_inversion", "ddim_edit"):
        with pytest.raises(ValueError, match=r"takes no regional prompts"):
            get_solver(name, solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", latent_hw=HW, engine=SR.SoftRegionMockEngine(latent_hw=HW),
                       max_regions=2, soft_regions=True)


def test_soft_regions_off_makes_no_new_call():
    class Strict(SR.SoftRegionMockEngine):
        def set_region_weights(self, *a, **k):
            raise AssertionError("set_region_weights called on a solver without soft_regions")
    s, eng = _solver("sd15", engine=Strict(latent_hw=HW), max_regions=3)
    assert not s.soft_regions
    _run(s, "sd15", region_prompts=["a snowy pine", "a red fox"], region_masks=SOFT)          # binarized, as before
    assert torch.equal(eng.region_calls[0][0], RG.build_region_map(SOFT, HW, None)) and "weights" not in eng.order
    _run(s, "sd15")
    assert eng.region_calls[-1] == (None, 0)


def test_cli_soft_region_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("text_to_img_example", os.path.join(ROOT, "examples", "text_to_img.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    solver = types.SimpleNamespace(latent_hw=HW)
    region = ["0.5,0,1,1:a snowy pine", "0,0,0.5,1:a red fox"]
    args = types.SimpleNamespace(region=region, max_regions=3, soft_regions=True, region_feather=0.25, region_base_ratio=0.3,
                                 region_negative=["2:blurry"])
    kw = mod._region_kwargs(args, solver)
    assert kw["region_prompts"] == ["a snowy pine", "a red fox"] and kw["region_base_ratio"] == 0.3
    assert kw["region_negative_prompts"] == [None, "blurry"]
    assert torch.equal(kw["region_masks"][0], RG.soft_rect_mask(0.5, 0, 1, 1, HW, 0.25)) and not torch.equal(kw["region_masks"][0], RG.rect_mask(0.5, 0, 1, 1, HW))
    hard = mod._region_kwargs(types.SimpleNamespace(region=region, max_regions=3, soft_regions=False, region_feather=0.0, region_base_ratio=0.0,
                                                    region_negative=[]), solver)
    assert set(hard) == {"region_prompts", "region_masks"} and torch.equal(hard["region_masks"][0], RG.rect_mask(0.5, 0, 1, 1, HW))
    with pytest.raises(ValueError, match=r"--region_negative '3:x'"):
        mod._region_kwargs(types.SimpleNamespace(region=region, max_regions=3, soft_regions=False, region_negative=["3:x"]), solver)


def test_library_and_header_agree():
    from cfgpp_amd import _lib
    from cfgpp_amd.build import build
    import re
    build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cfgpp_regions_soft.h")).read()
    declared = set(re.findall(r"^int (cfgpp_[a-z0-9_]+)\s*\(", hdr, re.M))
    assert declared == set(_lib.REGIONS_SOFT_PROTOTYPES) == {"cfgpp_unet_enable_region_weights", "cfgpp_unet_set_region_weights"}
    assert all(hasattr(lib, n) for n in declared)
    assert "cfgpp_op_attention_region_soft" in _lib.DEBUG_PROTOTYPES and hasattr(lib, "cfgpp_op_attention_region_soft")


# ---- the oracle: the engine tests' inputs are loud -----------------------------------------------------------------------------
def test_weight_mistakes_are_loud_in_the_oracle():
    """regions swapped, the weights shifted by one pixel, the level-0 weights used undownsampled: each moves the oracle's output by
    far more than the engine tests' bar (figures printed; TINY_SD, R = 3, the feathered stripes)"""
    from cfgpp_amd.unet_config import TINY_SD as cfg
    from cfgpp_amd.weights import synth_state_dict
    sd = synth_state_dict(cfg, 0)
    w = SR.region_weights("feather", 3)
    ehs = RR.region_context(2, 3, cfg.cross_attention_dim)
    z = torch.cat([RR.rnd(1, 4, 16, 16, seed=60)] * 2)
    ref = SR.SoftRegionUNetRef(cfg, sd, w)
    want = ref(z, 981.0, ehs, None)["sample"].float()
    for fault in ("swapped", "shifted", "no_downsample"):
        got = SR.SoftRegionUNetRef(cfg, sd, w, fault)(z, 981.0, ehs, None)["sample"].float()
        r = float((got - want).norm() / want.norm())
        print(f"{fault}: rel-L2 {r:.3e}")
        assert r > 10 * EPS_REL, (fault, r)
    onehot = SR.region_weights("onehot", 3)
    hard = RR.RegionUNetRef(cfg, sd, RR.region_ids("stripes", 3), 3)(z, 981.0, ehs, None)["sample"].float()
    soft = SR.SoftRegionUNetRef(cfg, sd, onehot)(z, 981.0, ehs, None)["sample"].float()
    assert float((hard - soft).norm() / hard.norm()) < 1e-5
