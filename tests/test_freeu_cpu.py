"""FreeU without a GPU: (1) the two fp64 statements of the skip filter agree; (2) an fp32 model of the kernel stays within the bound
the GPU test uses, on every case and in two summation orders, and every planted fault exceeds it tenfold somewhere; (3) the solver /
engine / command-line plumbing on a recording mock engine; (4) the extension header."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import freeu_cases as FC
import freeu_ref as FR
from mock_engine import MockEngine, StubVAE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = dict(ids=lambda c: c.id)


# ---- (1) the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(8, 8), (16, 16), (64, 64), (8, 12), (7, 9), (24, 40), (2, 2), (2, 6), (12, 24)])
@pytest.mark.parametrize("s", [0.0, 0.2, 0.9, 1.0])
def test_closed_form_is_fourier_filter(hw, s):
    x = np.random.RandomState(hw[0] * 100 + hw[1]).randn(3, 5, *hw) + 0.7
    a, b = FR.fourier_filter_np(x, s), FR.closed_form_np(x, s)
    assert np.abs(a - b).max() < 1e-13 * max(1.0, np.abs(x).max())


def test_closed_form_does_not_hold_for_one_pixel_axes():
    """H = 1 or W = 1: frequency -1 IS frequency 0 there and the sums count it twice - the op refuses such planes"""
    x = np.random.RandomState(0).randn(2, 1, 8)
    assert np.abs(FR.fourier_filter_np(x, 0.2) - FR.closed_form_np(x, 0.2)).max() > 1e-3


def test_torch_restatement_is_the_numpy_one():
    x = torch.randn(2, 6, 6, 10, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    a = FR.fourier_filter_t(x, 0.2).double().numpy()
    assert np.abs(a - FR.fourier_filter_np(x.numpy(), 0.2)).max() < 1e-5


def test_mask_is_not_hermitian():
    """only frequency -1 is scaled: a filter that scales +1 too differs by about the signal"""
    c = FC.Case(8, 16, 64, 64, 1, 0.2, 1.5, seed=3)
    h, k = FC.make_inputs(c)
    good, bad = FC.model32(c, h, k)[1], FC.model32(c, h, k, fault="both_pm1")[1]
    assert np.abs(good.astype(np.float64) - bad.astype(np.float64)).max() > 0.1


# ---- (2) the model, the bound, the faults -------------------------------------------------------------------------------------
def test_case_table_covers_the_paths():
    C = FC.CASES
    assert {(c.H, c.W) for c in C} >= {(4, 4), (8, 8), (8, 16), (6, 10), (16, 16), (32, 32), (64, 64)}
    assert {c.C_h for c in C} >= {64, 128, 192, 1280} and {c.C_s for c in C} >= {64, 128, 320, 640}
    assert {c.rows for c in C} >= {1, 3} and {c.half for c in C} == {"both", "hidden", "skip"}
    assert {c.s for c in C} >= {0.0, 0.2, 0.9, 1.0} and {c.b for c in C} >= {1.0, 1.5}
    launches = [FC.expected_launch(c) for c in C]
    assert {l[0] for l in launches} == {1, 2, 3}                       # resident, two-phase, hidden only
    assert {l[1] for l in launches if l[0] == 1} == {8, 16, 32, 64}     # every slab width of the resident path
    assert any(c.H * c.W * 16 == FC.LDS_PLANE_CAP for c in C) and any(c.H * c.W * 16 > FC.LDS_PLANE_CAP for c in C)
    assert len({c.id for c in C}) == len(C)


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(c):
        if c not in cache:
            h, k = FC.make_inputs(c)
            cache[c] = (h, k) + FC.reference(c, h, k)
        return cache[c]
    return get


@pytest.mark.parametrize("c", FC.CASES, **ids)
def test_fp32_model_is_within_the_bound(c, refs):
    h, k, rh, rk = refs(c)
    orders = ("pairwise", "sequential") if c.H * c.W <= 1024 or c.C_s <= 64 else ("pairwise",)
    for order in orders:
        mh, mk = FC.model32(c, h, k, order=order)
        a, b = FC.worst_ratio(c, mh, mk, h, k, rh, rk)
        assert a <= 1.0 and b <= 1.0, f"{c.id} {order}: hidden {a:.3f} x, skip {b:.3f} x the bound"
        if c.half != "skip":
            share = FC.hidden_mismatch_share(c, mh, rh)
            assert share <= FC.MISMATCH_CAP / 10, f"{c.id}: the fp32 model alone mismatches {share:.2e} of the scaled elements"


FAULT_CASES = [FC.Case(8, 16, 192, 320, 3, 0.2, 1.5, seed=7), FC.Case(6, 10, 64, 64, 3, 0.2, 1.5, seed=8),
               FC.Case(16, 16, 128, 128, 1, 0.0, 1.5, seed=9)]


@pytest.mark.parametrize("fault", FC.FAULTS)
def test_bound_sees_every_fault(fault):
    worst = 0.0
    for c in FAULT_CASES:
        h, k = FC.make_inputs(c)
        rh, rk = FC.reference(c, h, k)
        assert max(FC.worst_ratio(c, *FC.model32(c, h, k), h, k, rh, rk)) <= 1.0
        worst = max(worst, *FC.worst_ratio(c, *FC.model32(c, h, k, fault=fault), h, k, rh, rk))
    assert worst > 10.0, f"{fault}: only {worst:.2f} x the bound on every fault case"


def test_s1_b1_keeps_the_bits():
    c = FC.Case(6, 10, 64, 64, 3, 1.0, 1.0, seed=11)
    h, k = FC.make_inputs(c)
    h[0, 0, 0, 0] = np.float16(-0.0)
    k[0, 0, 0, 0] = np.float16(-0.0)
    mh, mk = FC.model32(c, h, k)
    assert mh.tobytes() == h.tobytes() and mk.tobytes() == k.tobytes()


# ---- (3) plumbing -----------------------------------------------------------------------------------------------------------
class RecordingEngine(MockEngine):
    def __init__(self):
        super().__init__(lambda *a: None, (8, 8))
        self.freeu_calls = []
        self.freeu = None

    def set_freeu(self, spec):
        self.freeu_calls.append(spec)
        self.freeu = spec


def _solver(kind, **kw):
    from cfgpp_amd.unet_config import TINY_SD, TINY_XL
    eng = RecordingEngine()
    common = dict(solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", latent_hw=(8, 8), engine=eng)
    if kind == "sd15":
        from cfgpp_amd.latent_diffusion import get_solver
        s = get_solver("ddim_cfg++", unet_config=TINY_SD, vae=StubVAE(TINY_SD.vae_scale), **common, **kw)
    elif kind == "sdxl":
        from cfgpp_amd.latent_sdxl import get_solver
        s = get_solver("ddim_cfg++", unet_config=TINY_XL, vae=StubVAE(TINY_XL.vae_scale), **common, **kw)
    elif kind == "inversion":
        from cfgpp_amd.latent_diffusion import get_solver
        s = get_solver("ddim_inversion_cfg++", unet_config=TINY_SD, vae=StubVAE(TINY_SD.vae_scale), **common, **kw)
    else:
        from cfgpp_amd.inpaint import get_inpaint_solver
        s = get_inpaint_solver("ddim_inpaint_cfg++", "sd15", unet_config=TINY_SD, vae=StubVAE(TINY_SD.vae_scale), **common, **kw)
    return s, eng


@pytest.mark.parametrize("kind", ["sd15", "sdxl", "inversion", "inpaint"])
def test_solver_freeu_reaches_the_engine(kind):
    s, eng = _solver(kind)
    assert eng.freeu_calls == [] and s.freeu is None                # absent: the engine is never told
    s, eng = _solver(kind, freeu=None)
    assert eng.freeu_calls == [] and s.freeu is None
    s, eng = _solver(kind, freeu=(0.9, 0.2, 1.5, 1.6))
    assert eng.freeu_calls == [(0.9, 0.2, 1.5, 1.6)] and s.freeu == (0.9, 0.2, 1.5, 1.6)
    s.set_freeu(dict(b1=1.1, s1=0.5, b2=1.2, s2=0.25))
    assert eng.freeu_calls[-1] == (0.5, 0.25, 1.1, 1.2) and s.freeu == (0.5, 0.25, 1.1, 1.2)
    s.set_freeu(None)
    assert eng.freeu_calls[-1] is None and s.freeu is None


@pytest.mark.parametrize("bad,word", [((1, 2, 3), "four values"), ((1, 2, 3, float("nan")), "b2=nan is not finite"),
                                      (dict(s1=1, s2=1, b1=1), "exactly the keys"), ("sd21", "four comma-separated"),
                                      ((1, 2, "x", 4), "as numbers"), (dict(s1=1, s2=1, b1=1, b3=1), "exactly the keys")])
def test_bad_specs_are_refused_by_name(bad, word):
    with pytest.raises(ValueError, match=word):
        _solver("sd15", freeu=bad)
    s, eng = _solver("sd15")
    with pytest.raises(ValueError, match=word):
        s.set_freeu(bad)
    assert eng.freeu_calls == []


def test_engine_without_freeu_is_an_error():
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    with pytest.raises(ValueError, match="has no FreeU"):
        get_solver("ddim_cfg++", solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", unet_config=TINY_SD, latent_hw=(8, 8),
                   engine=MockEngine(lambda *a: None, (8, 8)), freeu=(1, 1, 1, 1))


def _cli(name):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    return __import__(name)


@pytest.mark.parametrize("name", ["text_to_img", "text_to_mscoco", "inversion", "inpaint"])
def test_cli_parses_freeu(name, monkeypatch, tmp_path):
    """--freeu S1,S2,B1,B2 becomes the solver's freeu= (seen at the solver factory, which the test stops there)"""
    mod = _cli(name)
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop()
    import cfgpp_amd.inpaint as INP
    import cfgpp_amd.latent_diffusion as LD
    import cfgpp_amd.latent_sdxl as XL
    monkeypatch.setattr(LD, "get_solver", fake)
    monkeypatch.setattr(XL, "get_solver", fake)
    monkeypatch.setattr(INP, "get_inpaint_solver", fake)
    for attr in ("get_solver", "get_inpaint_solver"):
        if hasattr(mod, attr):
            monkeypatch.setattr(mod, attr, fake)
    argv = ["--device", "cpu", "--freeu", "0.9,0.2,1.5,1.6"]
    with pytest.raises((Stop, SystemExit)) as e:
        mod.main(argv + _cli_required(name, tmp_path))
    assert e.type is Stop, f"{name} ended before building a solver: {e.value}"
    assert seen["freeu"] == (0.9, 0.2, 1.5, 1.6)
    with pytest.raises(SystemExit, match="--freeu: .*four comma-separated"):
        mod.main(["--device", "cpu", "--freeu", "0.9,0.2"] + _cli_required(name, tmp_path))


def _cli_required(name, tmp_path):
    """the files each command line insists on before it builds its solver"""
    from PIL import Image
    args = ["--workdir", str(tmp_path / "out")]
    if name == "text_to_mscoco":
        (tmp_path / "caps.txt").write_text("a cat\n")
        args += ["--prompt_dir", str(tmp_path / "caps.txt")]
    if name in ("inversion", "inpaint"):
        Image.fromarray(np.zeros((64, 64, 3), dtype=np.uint8)).save(tmp_path / "src.png")
        args += ["--img_path", str(tmp_path / "src.png"), "--img_size", "64"]
    if name == "inpaint":
        Image.fromarray(np.full((64, 64), 255, dtype=np.uint8)).save(tmp_path / "mask.png")
        args += ["--mask_path", str(tmp_path / "mask.png")]
    return args


# ---- (4) the extension header ---------------------------------------------------------------------------------------------------
def test_extension_header_is_exported_and_bound():
    import re
    from cfgpp_amd import _lib
    from cfgpp_amd.build import SOURCES, build
    assert "freeu_kernel.hip" in [f for f, _ in SOURCES]
    build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cfgpp_freeu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cfgpp_[a-z0-9_]+)\s*\(", code))
    assert declared == {"cfgpp_unet_set_freeu"} == set(_lib.FREEU_PROTOTYPES)
    assert all(hasattr(lib, n) for n in declared)
    res, args = _lib.FREEU_PROTOTYPES["cfgpp_unet_set_freeu"]
    assert len(args) == 6 and re.search(r"cfgpp_unet_set_freeu\(cfgpp_unet\*\s*u,\s*float s1,\s*float s2,\s*float b1,\s*float b2,\s*int enable\)", code)
    for word in ("enable_freeu", "fourier_filter", "allocates nothing", "ControlNet-mode"):
        assert word in hdr, word
    assert set(_lib.DEBUG_PROTOTYPES) >= {"cfgpp_op_freeu", "cfgpp_freeu_last_launch"}
