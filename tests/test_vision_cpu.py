"""CPU: the image tower's front-end reference (tests/vision_ref.py) pinned to ``ip_adapter.preprocess_image`` on torch-CPU, its tap
windows against a brute-force walk, two faults that break the equality, the patch rows against torch's own convolution, the
geometry refusals of cfgpp_amd/vision.py, the solver's tower choice on a CPU device, and include/cfgpp_vision.h against the built
library and the ctypes table."""
import os
import re
import types

import numpy as np
import pytest
import torch

import vision_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(300, 500), (224, 224), (100, 60), (1000, 700), (225, 224), (1, 1)]          # H x W
# the largest |preprocess_image - fp64 model| over SIZES x S in {224, 28}, measured on the CPU: 1.191e-05 (300 x 500 at S = 224; the
# other sizes 2e-8 .. 7e-6).  It is torch's fp32 arithmetic: the sample position scale * (i + 0.5) alone is uncertain by ~1e-5 pixel.
MEASURED = 1.191e-05
BOUND = 4 * MEASURED


@pytest.fixture(scope="module")
def pinned():
    """(H, W, S) -> (image, model result, torch result), computed once and shared (do not modify)"""
    from cfgpp_amd.ip_adapter import preprocess_image
    out = {}
    for H, W in SIZES:
        for S in (224, 28):
            img = R.coordinate_image(2, H, W, seed=H + W)
            out[(H, W, S)] = (img, R.preprocess(img, S), preprocess_image(torch.from_numpy(img), S).double().numpy())
    return out


@pytest.mark.parametrize("S", [224, 28])
@pytest.mark.parametrize("H,W", SIZES)
def test_model_is_preprocess_image(pinned, H, W, S):
    """measured: 1.191e-05 at most (see MEASURED); asserted: 4 x that"""
    img, r, got = pinned[(H, W, S)]
    assert got.shape == r["want"].shape == (2, 3, S, S)
    diff = float(np.abs(got - r["want"]).max())
    print(f"{H}x{W} -> {S}: max |torch - fp64 model| = {diff:.3e}")
    assert diff <= BOUND


def test_same_size_is_the_identity_before_normalisation(pinned):
    img, r, _ = pinned[(224, 224, 224)]
    assert np.array_equal(r["resized"], img.astype(np.float64))          # weights (0, 1, 0, 0): exact
    assert int(r["taps_y"].max()) == 4 and int(r["taps_x"].max()) == 4


def test_tap_counts_are_run_time_quantities(pinned):
    assert int(pinned[(1000, 700, 224)][1]["taps_y"].max()) >= 13        # 700 -> 224 along the short side: support 2 * 3.125
    assert int(pinned[(100, 60, 224)][1]["taps_x"].max()) <= 5           # an upscale: support 2
    assert int(pinned[(1, 1, 224)][1]["taps_x"].max()) == 1


@pytest.mark.parametrize("n_in,n_out", [(300, 224), (500, 373), (100, 373), (60, 224), (1000, 320), (700, 224), (225, 225), (224, 28), (1, 224),
                                        (7, 3), (3, 7), (2, 1)])
def test_windows_against_a_brute_force_walk(n_in, n_out):
    for i in range(n_out):
        xmin, xsize, centre, inv = R.window(i, n_in, n_out)
        assert (xmin, xsize) == R.window_brute(i, n_in, n_out), (n_in, n_out, i)
        assert 0 <= xmin and xmin + xsize <= n_in and xsize >= 1


@pytest.mark.parametrize("fault", ["start_off_by_one", "no_renormalise"])
@pytest.mark.parametrize("H,W", [(300, 500), (100, 60), (1000, 700)])
def test_faults_break_the_equality(pinned, H, W, fault):
    """a window that starts one sample late, and weights that are not renormalised where the border cuts the window"""
    img, r, got = pinned[(H, W, 224)]
    bad = R.preprocess(img, 224, fault)["want"]
    assert float(np.abs(bad - got).max()) > 100 * BOUND


def test_resized_size_is_preprocess_image_rounding():
    assert R.resized_size(300, 500, 224) == (224, 373, 0, 74)
    assert R.resized_size(225, 224, 224) == (225, 224, 0, 0)
    assert R.resized_size(1000, 700, 224) == (320, 224, 48, 0)
    assert R.resized_size(1, 1, 28) == (28, 28, 0, 0)


def test_patch_rows_are_the_patch_convolution():
    """rows @ weight[H, 3 ps ps]^T equals torch's stride-ps convolution; the pad columns are zeros"""
    g = torch.Generator().manual_seed(0)
    pix = torch.randn((2, 3, 28, 28), generator=g, dtype=torch.float64)
    w = torch.randn((5, 3, 14, 14), generator=g, dtype=torch.float64)
    rows = R.patch_rows(pix.numpy(), 14, 640)
    assert rows.shape == (2 * 4, 640) and not rows[:, 588:].any()
    got = torch.from_numpy(rows[:, :588]) @ w.reshape(5, -1).T
    want = torch.nn.functional.conv2d(pix, w, stride=14).flatten(2).transpose(1, 2).reshape(8, 5)
    assert torch.allclose(got, want, atol=1e-10)
    assert rows[5, 1 * 196 + 3 * 14 + 2] == pix[1, 1, 14 * 0 + 3, 14 * 1 + 2]          # row n=1 p=(0, 1), column (c=1, dy=3, dx=2)


# ---- cfgpp_amd/vision.py without a GPU ------------------------------------------------------------------------------------------
VIT_H = dict(hidden=1280, layers=32, heads=16, intermediate=5120, act="gelu", proj_dim=1024, image_size=224, patch_size=14)


def test_geometry_refusals_by_name():
    from cfgpp_amd.vision import UnsupportedTower, check_geometry
    from cfgpp_amd._lib import CfgppError
    assert issubclass(UnsupportedTower, CfgppError)
    assert check_geometry(**VIT_H) == 257
    assert check_geometry(**dict(VIT_H, hidden=1664, heads=16, intermediate=8192, proj_dim=1280)) == 257          # bigG: d = 104
    assert check_geometry(**dict(VIT_H, hidden=1024, heads=16, intermediate=4096, proj_dim=768, act="quick_gelu")) == 257   # ViT-L/14
    for kw, msg in ((dict(hidden=1536, heads=16), "unsupported head dim"), (dict(hidden=1280, heads=12), "unsupported head dim"),
                    (dict(hidden=520, heads=5), "multiples of 64"), (dict(intermediate=5000), "multiples of 64"),
                    (dict(image_size=225), "not a multiple of patch_size"), (dict(image_size=336), "577 tokens"),
                    (dict(act="gelu_new"), "activation 'gelu_new'"), (dict(layers=0), "non-positive")):
        with pytest.raises(UnsupportedTower, match=msg):
            check_geometry(**dict(VIT_H, **kw))


def test_solver_on_a_cpu_device_keeps_the_torch_tower(tmp_path):
    """build_image_encoder: ImageEncoder on a CPU device and for image_tower="torch"; an unknown choice is refused"""
    transformers = pytest.importorskip("transformers")
    from cfgpp_amd import vision
    from cfgpp_amd.ip_adapter import ImageEncoder
    cfgv = transformers.CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, image_size=64,
                                         patch_size=32, projection_dim=16)
    torch.manual_seed(0)
    transformers.CLIPVisionModelWithProjection(cfgv).save_pretrained(str(tmp_path / "image_encoder"))
    n = len(vision.last_image_tower_fallbacks)
    for choice in ("hip", "torch"):
        enc = vision.build_image_encoder(str(tmp_path), "cpu", choice)
        assert isinstance(enc, ImageEncoder) and enc.torch_ops is True
    assert len(vision.last_image_tower_fallbacks) == n                  # a CPU device is not a fallback: there is no HIP path to fall from
    with pytest.raises(ValueError, match="image_tower='onnx'"):
        vision.build_image_encoder(str(tmp_path), "cpu", "onnx")
    assert vision.HipClipImageTower.torch_ops is False


def test_get_solver_takes_image_tower():
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import TINY_SD
    from cfgpp_amd.weights import synth_state_dict
    from ip_plus_mock import IPPlusMockEngine
    from test_ip_plus_cpu import StubVAE
    eng = IPPlusMockEngine(TINY_SD, synth_state_dict(TINY_SD, 0), (8, 8))
    kw = dict(solver_config=types.SimpleNamespace(num_sampling=2), device="cpu", unet_config=TINY_SD, max_batch=2, latent_hw=(8, 8), engine=eng,
              vae=StubVAE(TINY_SD.vae_scale), ip_adapter="synthetic")
    assert get_solver("ddim_cfg++", **kw).image_tower == "hip"
    assert get_solver("ddim_cfg++", image_tower="torch", **kw).image_tower == "torch"
    with pytest.raises(ValueError, match="image_tower='eager'"):
        get_solver("ddim_cfg++", image_tower="eager", **kw)


# ---- the extension header ----------------------------------------------------------------------------------------------------
def test_extension_header_is_exported_and_bound():
    """include/cfgpp_vision.h: every declaration is exported by the built library and has a ctypes prototype in its own table, with
    the declaration's argument count; include/cfgpp.h stays at its 40 entries"""
    from cfgpp_amd import _lib
    from cfgpp_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cfgpp_vision.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decls = dict(re.findall(r"\b(cfgpp_vision_[a-z0-9_]+)\s*\(([^)]*)\)", code))
    assert set(decls) == {"cfgpp_vision_create", "cfgpp_vision_destroy", "cfgpp_vision_load_tensor", "cfgpp_vision_finalize",
                          "cfgpp_vision_preprocess", "cfgpp_vision_encode", "cfgpp_vision_flops", "cfgpp_vision_device_bytes"}
    assert set(decls) == set(_lib.VISION_PROTOTYPES)
    for name, args in decls.items():
        assert hasattr(lib, name), f"{name} declared in include/cfgpp_vision.h but not exported"
        assert len(_lib.VISION_PROTOTYPES[name][1]) == args.count(",") + 1, name
        fn = getattr(lib, name)
        assert fn.restype == _lib.VISION_PROTOTYPES[name][0] and list(fn.argtypes) == _lib.VISION_PROTOTYPES[name][1]
    others = set(_lib.PROTOTYPES) | set(_lib.DEBUG_PROTOTYPES) | set(_lib.IP_ADAPTER_PROTOTYPES) | set(_lib.IP_PLUS_PROTOTYPES)
    assert not set(_lib.VISION_PROTOTYPES) & others
    main_hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cfgpp.h")).read(), flags=re.S)
    assert '#include "cfgpp.h"' in hdr and "cfgpp_vision" not in main_hdr and len(_lib.PROTOTYPES) == 40
    dbg = open(os.path.join(ROOT, "cfgpp_amd", "csrc", "cfgpp_debug.h")).read()
    for name in ("cfgpp_op_attention_vit", "cfgpp_vit_attention_last_launch", "cfgpp_op_vit_preprocess", "cfgpp_op_vit_patch_rows"):
        assert name in _lib.DEBUG_PROTOTYPES and hasattr(lib, name) and name in dbg
    from cfgpp_amd.build import SOURCES
    assert ("vision.hip", ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]) in SOURCES
