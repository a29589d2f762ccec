"""CPU: MultiDiffusion panoramas - the view geometry against the pinned case table (tests/pano_cases.py), every refusal, the
``view_batch_size`` rule, the solvers' plumbing on a mock engine (tests/pano_mock.py) against the slice model of tests/pano_ref.py run
as a plain per-view loop, the one-view panorama against the plain solvers, the library's extension header, the CLI, and fault
injection: each deliberate error switched into the model has to break the equality that guards it."""
import os
import re
import sys
import types

import pytest
import torch

import pano_ref as R
from mock_engine import MockEngine, StubVAE
from pano_cases import CASES, case_id, divisors
from pano_mock import PanoMockEngine

from cfgpp_amd import coeffs as K
from cfgpp_amd import panorama as P
from cfgpp_amd.unet_config import TINY_SD, TINY_XL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, F = torch.float16, torch.float32
NAMES = ("ddim_panorama", "ddim_panorama_cfg++")


def cfgn(n):
    return types.SimpleNamespace(num_sampling=n)


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("case", list(CASES), ids=case_id)
def test_views_and_coverage_against_the_table(case):
    n, lo, hi = CASES[case]
    Hp, Wp, h, w, stride, circ = case
    vs = P.panorama_views(*case)
    assert vs == R.views(case) and len(vs) == n
    nbw = len({x for _, x in vs})
    assert vs == [((i // nbw) * stride, (i % nbw) * stride) for i in range(n)]          # the order: rows of views, left to right
    cov = R.coverage(case)
    assert int(cov.min()) == lo and int(cov.max()) == hi
    # every pixel's count, from the definition: view (y0, x0) covers (y, x) iff y0 <= y < y0 + h and (x - x0) mod Wp < w (plain: no mod)
    for y in range(Hp):
        for x in range(Wp):
            want = sum(1 for y0, x0 in vs if y0 <= y < y0 + h and (((x - x0) % Wp) < w if circ else x0 <= x < x0 + w))
            assert int(cov[y, x]) == want, (y, x)
    g = P.ViewGeometry(Hp, Wp, h, w, stride, bool(circ))
    assert g.n_views == n and g.with_chunk(n).chunk_views == n and g.chunk_views == 1


@pytest.mark.parametrize("args,word", [
    ((13, 16, 8, 8, 4, False), r"\(Hp - h\)"),
    ((8, 20, 8, 8, 8, False), r"\(Wp - w\)"),
    ((8, 20, 8, 8, 8, True), "circular_padding with Wp = 20"),
    ((4, 16, 8, 8, 4, False), "smaller than the window"),
    ((8, 4, 8, 8, 4, False), "smaller than the window"),
    ((8, 16, 8, 8, 6, False), "stride = 6"),
    ((8, 18, 8, 6, 4, False), "window's width = 6"),
    ((8, 18, 8, 8, 2, False), "stride = 2"),
    ((8, 18, 8, 8, 4, False), "panorama's width = 18"),
    ((32, 32, 8, 16, 12, False), "stride=12 exceeds the window"),
    ((32, 32, 16, 8, 12, False), "stride=12 exceeds the window"),
    ((8, 16, 8, 8, 0, False), "must be positive"),
])
def test_geometry_refusals_by_name(args, word):
    with pytest.raises(ValueError, match=word):
        P.panorama_views(*args)


def test_view_batch_size_rule():
    assert P.view_chunk(25, 1, 32) == 25 and P.view_chunk(25, 2, 32) == 5 and P.view_chunk(25, 1, 8) == 5 and P.view_chunk(25, 8, 8) == 1
    assert P.view_chunk(6, 2, 7) == 3 and P.view_chunk(6, 2, 7, 1) == 1 and P.view_chunk(6, 1, 6, 2) == 2
    with pytest.raises(ValueError, match=r"view_batch_size=4.*\[1, 2, 3\]"):
        P.view_chunk(6, 2, 7, 4)
    with pytest.raises(ValueError, match=r"view_batch_size=6.*\[1, 2, 3\]"):          # a divisor, but 6 * 2 rows do not fit
        P.view_chunk(6, 2, 7, 6)
    with pytest.raises(ValueError, match="exceeds max_batch=4"):
        P.view_chunk(6, 5, 4)


def test_panorama_solvers_have_their_own_registry():
    from cfgpp_amd import latent_diffusion as sd, latent_sdxl as xl
    assert P.panorama_solver_names() == ["ddim_panorama", "ddim_panorama_cfg++"]
    assert not any("panorama" in k for k in list(sd.__SOLVER__) + list(xl.__SOLVER__))
    with pytest.raises(ValueError, match="one of"):
        P.get_panorama_solver("ddim_panorama", model="sd20", panorama_hw=(8, 16))
    with pytest.raises(ValueError, match="does not exist"):
        P.get_panorama_solver("ddim", model="sd15", panorama_hw=(8, 16))
    with pytest.raises(ValueError, match="needs panorama_hw"):
        P.get_panorama_solver("ddim_panorama", model="sd15")


# ------------------------------------------------------------------------------------------------ a cheap row-wise UNet stand-in
def _unet_fn(z, t, ehs, te, ti):
    """eps of row r from row r's inputs only, whatever the batch it runs in: elementwise in z, per-row scalars from the conditioning"""
    out = torch.empty(z.shape, dtype=H)
    for r in range(z.shape[0]):
        s = float(ehs[r].float().mean()) * 4.0 + float(t) * 1e-3
        if te is not None:
            s += float(te[r].float().mean()) + float(ti[r].float().sum()) * 1e-4
        zr = z[r].float()
        out[r] = (torch.tanh(zr * 0.7 + zr.roll(1, -1) * 0.2 + zr.roll(1, -2) * 0.1) + s).to(H)
    return out


def _solver(name, model, case, B, Vc=None, nfe=3, engine=None, **kw):
    Hp, Wp, h, w, stride, circ = case
    cfg = TINY_SD if model == "sd15" else TINY_XL
    eng = engine or PanoMockEngine(_unet_fn, (h, w))
    V = CASES[case][0]
    s = P.get_panorama_solver(name, model=model, panorama_hw=(Hp, Wp), stride=stride, circular_padding=bool(circ), view_batch_size=Vc,
                              solver_config=cfgn(nfe), device="cpu", unet_config=cfg, max_batch=V * B, latent_hw=(h, w), engine=eng,
                              vae=StubVAE(cfg.vae_scale), **kw)
    return s, eng


def _prompts(B):
    return ["a cat", "a dog", "a bird"][:B]


def _sample(s, model, B, seeds, **kw):
    if model == "sd15":
        return s.sample(cfg_guidance=0.6, prompt=["bad", _prompts(B)], seeds=seeds, return_latents=True, **kw)
    return s.sample(cfg_guidance=0.6, prompt=["bad", _prompts(B)], seeds=seeds, return_latents=True, **kw)


def _plain_loop(s, model, case, B, seeds, faults=()):
    """the slice model as a per-view loop, fed by the solver's own conditioning and coefficient tables"""
    Hp, Wp, h, w, _, _ = case
    wrap = model == "sdxl"
    if model == "sd15":
        uc, c = s.get_text_embed("bad", _prompts(B))
        te = ti = None
    else:
        uc, c, pool_null, pool = s.get_text_embed("bad", _prompts(B), "bad", _prompts(B))
        ack = s._cond_kwargs(pool, pool_null, 0.6, (8 * h, 8 * w), (0, 0), (8 * h, 8 * w), None, (0, 0), None, c.dtype)
        te, ti = ack["text_embeds"], ack["time_ids"]
        assert te.shape[0] == 2 * B and torch.equal(ti[0], torch.tensor([8.0 * h, 8 * w, 0, 0, 8 * h, 8 * w]).to(ti.dtype))
    ehs = torch.cat([uc.expand(B, -1, -1), c], 0)

    def pair(zv, t):
        eps = _unet_fn(torch.cat([zv, zv], 0), float(t), ehs, te, ti)
        return eps[:B], eps[B:]

    def co(t):
        sqrt4, dev_a = s._ddim_step_coeffs(t, False, wrap)
        return K.ddim_coeffs_pinned(sqrt4, eps_half=True, semantics=s.scalar_semantics, z_half=False, device_alpha=dev_a)

    ts = s.scheduler.timesteps
    z = s._randn((B, 4, Hp, Wp), seeds)
    return R.loop(case, pair, z, ts.int() if wrap else ts, co, B, 0.6, False, s.cfgpp, faults)


# ------------------------------------------------------------------------------------------------ the solvers on the mock
@pytest.mark.parametrize("model", ["sd15", "sdxl"])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("case", [(12, 16, 8, 8, 4, 0), (12, 16, 8, 8, 4, 1), (8, 12, 8, 8, 4, 1)], ids=case_id)
def test_solver_on_the_mock_equals_the_plain_loop(case, name, model):
    V = CASES[case][0]
    for B in (1, 2):
        seeds = [3, 4][:B]
        want = None
        for Vc in divisors(V):
            s, eng = _solver(name, model, case, B, Vc)
            z0t, zt = _sample(s, model, B, seeds)
            if want is None:
                want = _plain_loop(s, model, case, B, seeds)
            assert torch.equal(z0t, want[0]) and torch.equal(zt, want[1]), (B, Vc)
            assert z0t.shape == (B, 4, case[0], case[1]) and not torch.equal(z0t, zt)
            # per step V / Vc forwards at Vc * B rows and ONE step; one gather per job; the context set once per job
            names = [n for n, _ in eng.pcalls]
            assert names == ["gather_views"] + (["predict_into"] * (V // Vc) + ["step_ddim_views"]) * 3
            assert all(d["rows"] == Vc * B for n, d in eng.pcalls if n == "predict_into")
            assert len(eng.contexts) == 1 and eng.contexts[0]["rows"] == 2 * Vc * B
            steps = [d for n, d in eng.pcalls if n == "step_ddim_views"]
            assert all(d["renoise_uc"] == name.endswith("cfg++") and not d["tweedie_uc"] and d["chunk"] == Vc for d in steps)


def test_default_view_batch_size_is_the_largest_that_fits():
    case = (12, 16, 8, 8, 4, 1)          # 8 views
    eng = PanoMockEngine(_unet_fn, (8, 8))
    s = P.get_panorama_solver("ddim_panorama_cfg++", panorama_hw=(12, 16), stride=4, circular_padding=True, solver_config=cfgn(2),
                              device="cpu", unet_config=TINY_SD, max_batch=5, latent_hw=(8, 8), engine=eng, vae=StubVAE(TINY_SD.vae_scale))
    _sample(s, "sd15", 1, [1])
    assert [d["rows"] for n, d in eng.pcalls if n == "predict_into"] == [4] * 4          # Vc = 4: 8 views, 4 <= 5
    _sample(s, "sd15", 2, [1, 2])
    assert [d["rows"] for n, d in eng.pcalls if n == "predict_into"][4:] == [4] * 8      # B = 2: Vc = 2
    with pytest.raises(ValueError, match=r"view_batch_size=3.*\[1, 2, 4, 8\]"):          # refused before anything is built
        _solver("ddim_panorama", "sd15", case, 1, 3)
    s2, _ = _solver("ddim_panorama", "sd15", case, 1, 8)          # fits one chain ...
    with pytest.raises(ValueError, match=r"view_batch_size=8.*2 chains.*\[1, 2, 4\]"):
        _sample(s2, "sd15", 2, [1, 2])                             # ... not two


@pytest.mark.parametrize("name,plain", [("ddim_panorama", "ddim"), ("ddim_panorama_cfg++", "ddim_cfg++")])
def test_one_view_panorama_is_the_plain_solver_bit_for_bit(name, plain):
    from cfgpp_amd import latent_diffusion as sd, latent_sdxl as xl
    case = (8, 8, 8, 8, 4, 0)
    s, _ = _solver(name, "sd15", case, 2, nfe=4)
    a = _sample(s, "sd15", 2, [1, 2])
    ref = sd.get_solver(plain, solver_config=cfgn(4), device="cpu", unet_config=TINY_SD, max_batch=2, latent_hw=(8, 8),
                        engine=MockEngine(_unet_fn, (8, 8)), vae=StubVAE(TINY_SD.vae_scale))
    b = ref.sample(cfg_guidance=0.6, prompt=["bad", _prompts(2)], seeds=[1, 2], return_latents=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    sx, _ = _solver(name, "sdxl", case, 2, nfe=4)
    ax = _sample(sx, "sdxl", 2, [1, 2])
    refx = xl.get_solver(plain, solver_config=cfgn(4), device="cpu", unet_config=TINY_XL, max_batch=2, latent_hw=(8, 8),
                         engine=MockEngine(_unet_fn, (8, 8)), vae=StubVAE(TINY_XL.vae_scale))
    bx = refx.sample(prompt1=["bad", _prompts(2)], prompt2=["bad", _prompts(2)], cfg_guidance=0.6, target_size=(64, 64),
                     original_size=(64, 64), seeds=[1, 2], return_latents=True)
    assert torch.equal(ax[0], bx)          # (the SDXL ddim solvers return z0t)


def test_callbacks_see_the_panorama_and_an_edit_regathers_the_views():
    case = (8, 16, 8, 8, 4, 1)
    s, eng = _solver("ddim_panorama_cfg++", "sd15", case, 1)
    seen = []

    def cb(step, t, kw):
        seen.append((step, tuple(kw["z0t"].shape), tuple(kw["zt"].shape)))
        if step == 0:
            kw["zt"] = kw["zt"] * 0.5          # a replaced latent
        return kw

    z0t, zt = _sample(s, "sd15", 1, [7], callback_fn=cb)
    assert seen == [(i, (1, 4, 8, 16), (1, 4, 8, 16)) for i in range(3)]
    names = [n for n, _ in eng.pcalls]
    step = ["predict_into", "step_ddim_views"]          # (all 4 views in one forward)
    assert names == ["gather_views"] + step + ["gather_views"] + step + step          # re-gathered right after step 0's callback, only
    s2, _ = _solver("ddim_panorama_cfg++", "sd15", case, 1)
    plain = _sample(s2, "sd15", 1, [7])
    assert not torch.equal(plain[1], zt)
    # the image: the whole panorama decoded
    img = s2.sample(cfg_guidance=0.6, prompt=["bad", "a cat"], seeds=[7])
    assert img.shape == (1, 3, 64, 128) and torch.isfinite(img).all()


def test_sdxl_time_ids_are_the_windows_and_can_be_overridden():
    case = (8, 16, 8, 8, 4, 0)
    s, eng = _solver("ddim_panorama", "sdxl", case, 1)
    _sample(s, "sdxl", 1, [1])
    ti = eng.contexts[0]["ti"]
    assert ti.shape[0] == 2 * 3 and all(torch.equal(r, torch.tensor([64.0, 64, 0, 0, 64, 64]).to(ti.dtype)) for r in ti)
    _sample(s, "sdxl", 1, [1], target_size=(64, 128), original_size=(64, 128), crops_coords_top_left=(0, 8))
    ti = eng.contexts[-1]["ti"]
    assert all(torch.equal(r, torch.tensor([64.0, 128, 0, 8, 64, 128]).to(ti.dtype)) for r in ti)


def test_job_refusals_by_name():
    case = (8, 16, 8, 8, 4, 0)
    s, _ = _solver("ddim_panorama_cfg++", "sd15", case, 1)
    sx, _ = _solver("ddim_panorama_cfg++", "sdxl", case, 1)
    for sv in (s, sx):
        with pytest.raises(ValueError, match="does not take control_image"):
            sv.sample(prompt=["", "a"], control_image=torch.zeros(1, 3, 64, 64))
        with pytest.raises(ValueError, match="does not take ip_adapter_image_embeds"):
            sv.sample(prompt=["", "a"], ip_adapter_image_embeds=torch.zeros(1, 8))
        with pytest.raises(ValueError, match="does not take ip_adapter_image"):
            sv.sample(prompt=["", "a"], ip_adapter_image=torch.zeros(1, 3, 8, 8))
        with pytest.raises(ValueError, match="guidance_rescale=0.5 is not supported by the panorama"):
            sv.sample(prompt=["", "a"], guidance_rescale=0.5)
    for model in ("sd15", "sdxl"):
        with pytest.raises(ValueError, match="v_prediction' is not supported by the panorama"):
            _solver("ddim_panorama", model, case, 1, prediction_type="v_prediction")
        with pytest.raises(ValueError, match="guidance_rescale=0.7 is not supported by the panorama"):
            _solver("ddim_panorama", model, case, 1, guidance_rescale=0.7)
    with pytest.raises(ValueError, match=r"latent shape \(1, 4, 8, 8\)"):
        s.sample(prompt=["", "a"], latents=torch.zeros(1, 4, 8, 8))
    import torch.distributed as dist
    real = (dist.is_initialized, dist.get_world_size)
    dist.is_initialized, dist.get_world_size = (lambda: True), (lambda *a, **k: 2)
    try:
        with pytest.raises(ValueError, match="world size > 1"):
            s.sample(prompt=["", "a"])
    finally:
        dist.is_initialized, dist.get_world_size = real


# ------------------------------------------------------------------------------------------------ fault injection
def _step_inputs(case, B, Vc, seed=0):
    Hp, Wp, h, w, _, _ = case
    V = CASES[case][0]
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 4, Hp, Wp, generator=g)
    eps = torch.randn(V // Vc, 2 * Vc * B, 4, h, w, generator=g).to(H)
    return z, eps


def _one_step(case, B, Vc, faults=()):
    z, eps = _step_inputs(case, B, Vc)
    zv = R.gather(case, z, B)
    zn, z0 = R.step(case, z, zv, eps, B, Vc, 0.6, (0.6, 0.8, 0.7, 0.71), False, True, faults)
    return zn, z0, zv


# fault -> the table cases on which it has to show (B, Vc chosen so that the fault has something to act on)
FAULT_CASES = {
    "start_off_by_stride": [c for c in CASES if CASES[c][0] > 1],
    "no_wrap": [c for c in CASES if c[5]],
    "div_max_count": [c for c in CASES if CASES[c][1] != CASES[c][2]],
    "wrong_batch_row": list(CASES),
    "eps_next_view": [c for c in CASES if CASES[c][0] > 1],
    "swap_halves": list(CASES),
    "no_wrapped_scatter": [c for c in CASES if c[5]],
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_each_fault_breaks_the_equality(fault):
    assert FAULT_CASES[fault]
    for case in FAULT_CASES[fault]:
        V = CASES[case][0]
        for Vc in divisors(V):
            good = _one_step(case, 2, Vc)
            again = _one_step(case, 2, Vc)
            assert all(torch.equal(a, b) for a, b in zip(good, again))
            bad = _one_step(case, 2, Vc, (fault,))
            # NaN (0 / 0 where the faulty views leave a hole) counts as different
            same = all(torch.equal(a, b) for a, b in zip(good, bad))
            assert not same, (fault, case, Vc)
            if fault == "no_wrapped_scatter":          # only the views' copies are stale: the panorama itself is right
                assert torch.equal(good[0], bad[0]) and torch.equal(good[1], bad[1]) and not torch.equal(good[2], bad[2])


def test_faulted_model_breaks_the_solver_comparison():
    """the chain-level form: the solver on the fault-free mock against the faulted plain loop"""
    case = (12, 16, 8, 8, 4, 1)
    s, _ = _solver("ddim_panorama_cfg++", "sd15", case, 2, 4)
    z0t, zt = _sample(s, "sd15", 2, [3, 4])
    for fault in R.FAULTS:
        w0, w1 = _plain_loop(s, "sd15", case, 2, [3, 4], (fault,))
        assert not (torch.equal(z0t, w0) and torch.equal(zt, w1)), fault


# ------------------------------------------------------------------------------------------------ the extension header
def test_extension_header_is_exported_and_bound():
    from cfgpp_amd import _lib
    from cfgpp_amd.build import SOURCES, build
    assert dict(SOURCES)["pano_kernels.hip"] == ["-ffp-contract=off"] == dict(SOURCES)["step_kernels.hip"]
    build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cfgpp_panorama.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cfgpp_[a-z0-9_]+)\s*\(", code))
    assert declared == {"cfgpp_views_gather", "cfgpp_step_ddim_views"} == set(_lib.PANORAMA_PROTOTYPES)
    assert all(hasattr(lib, n) for n in declared)
    for name in declared:        # the bound argument count is the declared one
        args = re.search(name + r"\((.*?)\);", code, flags=re.S).group(1)
        assert len(_lib.PANORAMA_PROTOTYPES[name][1]) == args.count(",") + 1, name
    fields = re.search(r"typedef struct cfgpp_pano_views \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"\b([A-Za-z_]+)\s*[,;]", fields) == [n for n, _ in _lib.PanoViewsC._fields_]
    main_hdr = open(os.path.join(ROOT, "include", "cfgpp.h")).read()
    assert '#include "cfgpp.h"' in hdr and "pano" not in main_hdr
    # the helpers are defined once: the step files include the shared header and restate nothing
    csrc = os.path.join(ROOT, "cfgpp_amd", "csrc")
    for f in ("step_kernels.hip", "vpred_kernels.hip", "lcm_kernels.hip", "pano_kernels.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "step_math.h"' in text and "float h_round(" not in text and "float div_as_ref(" not in text, f
    assert "float h_round(" in open(os.path.join(csrc, "step_math.h")).read()


# ------------------------------------------------------------------------------------------------ the CLI
def test_panorama_cli_writes_an_image_on_the_cpu_mock(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import panorama as cli
    for model, cfg in (("sd15", TINY_SD), ("sdxl", TINY_XL)):
        eng = PanoMockEngine(_unet_fn, (8, 8))
        cli.main(["--prompt", "a cat", "--NFE", "2", "--device", "cpu", "--workdir", str(tmp_path / model), "--cfg_guidance", "0.6",
                  "--panorama_size", "64x128", "--stride", "4", "--circular_padding", "--view_batch_size", "2", "--model", model],
                 solver_kwargs=dict(engine=eng, unet_config=cfg, vae=StubVAE(cfg.vae_scale), latent_hw=(8, 8)))
        assert (tmp_path / model / "result" / "panorama.png").exists()
        assert [n for n, _ in eng.pcalls] == ["gather_views"] + (["predict_into"] * 2 + ["step_ddim_views"]) * 2
        from PIL import Image
        assert Image.open(tmp_path / model / "result" / "panorama.png").size == (128, 64)
    with pytest.raises(SystemExit, match="multiples of 8"):
        cli.parse_size("60x128")
    with pytest.raises(SystemExit, match="expected HxW"):
        cli.parse_size("512")
