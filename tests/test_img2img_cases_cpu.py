"""The case table of cfgpp_img2img_start without a GPU: the fp64 model (tests/img2img_ref.py) against torch's fp64 F.interpolate, the
fp32 restatement of a correct kernel against the derived bound, every planted fault against ten times the bound, and the C boundary
(include/cfgpp_img2img.h against its ctypes prototype)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import img2img_cases as T
import img2img_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAULTS = ("align_corners", "no_half_pixel", "swap_scales", "clamp_wrong_edge", "tap_off_by_one", "bilinear_for_bicubic",
          "broadcast_row_b", "noise_per_image_row")


@pytest.fixture(scope="module")
def table():
    """inputs, the fp64 model and the bound of every case, computed once"""
    out = {}
    for c in T.CASES:
        inp = T.make_inputs(c)
        ref, mag = T.model(c, inp)
        out[c["name"]] = (c, inp, ref, M.bound(ref, mag, c["x_half"]))
    return out


def test_table_covers_what_it_claims():
    names = [c["name"] for c in T.CASES]
    assert len(set(names)) == len(names)
    for sname, hw0, hw in T.SHAPES:
        modes = {c["mode"] for c in T.CASES if c["hw0"] == hw0 and c["hw"] == hw and c["B"] == 3 and c["src_rows"] == 3}
        assert modes >= ({"identity"} if hw0 == hw else set(T.RESAMPLERS)), sname
        dts = {(c["x_half"], c["src_half"]) for c in T.CASES if c["hw0"] == hw0 and c["hw"] == hw}
        assert len(dts) == 4, sname
    assert any(c["src_rows"] == 1 and c["B"] == 3 for c in T.CASES) and any(c["B"] == 33 for c in T.CASES)
    assert any(c["a"] == 0.0 for c in T.CASES) and any(c["s"] == 0.0 and c["noise"] is None for c in T.CASES)
    assert any(c["hw"][1] % 4 and c["hw"][0] % 2 for c in T.CASES) and all(4 * c["hw"][0] * c["hw"][1] % 4 == 0 for c in T.CASES)


@pytest.mark.parametrize("mode", T.RESAMPLERS + ("identity",))
def test_fp64_model_is_torch_interpolate(mode):
    """the integer-rational model agrees with F.interpolate(double, size=, align_corners=False) to 1e-12 on every shape of the table
    (bilinear with antialias=True coincides with the plain kernel when upscaling, which is why no antialias mode is built)"""
    rng = np.random.default_rng(7)
    for _, hw0, hw in T.SHAPES:
        if (mode == "identity") != (hw0 == hw):
            continue
        v = rng.standard_normal((2, T.C) + hw0)
        got = M.resample(v, hw[0], hw[1], M.MODES[mode])
        if mode == "identity":
            want = torch.from_numpy(v)
        else:
            kw = {} if mode == "nearest-exact" else dict(align_corners=False)
            want = F.interpolate(torch.from_numpy(v), size=hw, mode=mode, **kw)
            if mode == "bilinear":          # (torch's antialiased bicubic is another kernel, A = -0.5: not this one at any scale)
                aa = F.interpolate(torch.from_numpy(v), size=hw, mode=mode, antialias=True, **kw)
                assert float((aa - want).abs().max()) < 1e-12
        assert float(np.abs(got - want.numpy()).max()) < 1e-12, (mode, hw0, hw)


def test_correct_fp32_kernel_is_inside_the_bound(table):
    for name, (c, inp, ref, bnd) in table.items():
        got, _ = T.model(c, inp, dtype=np.float32)
        assert got.shape == ref.shape == (c["B"], T.C) + c["hw"]
        worst = float((np.abs(got - ref) / bnd).max())
        assert worst <= 1.0, (name, worst)


def test_identity_fp32_is_the_torch_expression(table):
    """mode 0 with an fp32 x: the restatement gives torch's a * z.float() + s * noise bit for bit"""
    for name, (c, inp, ref, bnd) in table.items():
        if c["mode"] != "identity" or c["x_half"] or c["a"] == 0.0 or c["noise"] != "tensor":
            continue
        got, _ = T.model(c, inp, dtype=np.float32)
        z = torch.from_numpy(inp["src_parent"][: c["src_rows"]]).to(torch.float16 if c["src_half"] else torch.float32)
        want = float(np.float32(c["a"])) * z.float() + float(np.float32(c["s"])) * torch.from_numpy(inp["noise"])
        assert np.array_equal(got.astype(np.float32), want.numpy()), name


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_exceeds_the_bound_tenfold(table, fault):
    worst, where = 0.0, None
    for name, (c, inp, ref, bnd) in table.items():
        bad, _ = T.model(c, inp, dtype=np.float32, faults={fault})
        r = float((np.abs(bad - ref) / bnd).max())
        if r > worst:
            worst, where = r, name
    assert worst >= 10.0, (fault, worst, where)


def test_noise_model_is_stream_4_draw_0():
    import lcm_ref as R
    n = M.noise_rows(2, 4, 3, 4, [5, 6])
    assert np.array_equal(n.reshape(2, -1), R.normal_rows(2, 48, [5, 6], 0, 4).astype(np.float32))
    assert not np.array_equal(n.reshape(2, -1), R.normal_rows(2, 48, [5, 6], 0, 2).astype(np.float32))
    assert M.NOISE_STREAM == 4 and "4:" in open(os.path.join(ROOT, "cfgpp_amd", "csrc", "philox.h")).read().split("#pragma once")[0]


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_header_and_prototypes_agree():
    """include/cfgpp_img2img.h: every declaration has a ctypes prototype in its own table (include/cfgpp.h stays at its size)"""
    from cfgpp_amd import _lib
    from cfgpp_amd.build import SOURCES, build
    build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "cfgpp_img2img.h")).read()
    body = hdr[hdr.index("#ifndef CFGPP_IMG2IMG_H"):]
    declared = set(re.findall(r"^int\s+(cfgpp_[a-z0-9_]+)\s*\(", body, re.M))
    assert declared == {"cfgpp_img2img_start"} == set(_lib.IMG2IMG_PROTOTYPES)
    args = re.search(r"^int\s+cfgpp_img2img_start\(([^)]*)\)", body, re.M).group(1)
    res, argtypes = _lib.IMG2IMG_PROTOTYPES["cfgpp_img2img_start"]
    assert len(argtypes) == args.count(",") + 1 == 17
    fn = getattr(lib, "cfgpp_img2img_start")
    assert fn.restype == res and list(fn.argtypes) == argtypes
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("PROTOTYPES") and n != "IMG2IMG_PROTOTYPES"]
    assert not any(set(_lib.IMG2IMG_PROTOTYPES) & set(o) for o in others)
    assert "cfgpp_img2img_start" not in open(os.path.join(ROOT, "include", "cfgpp.h")).read()
    assert ("img2img_kernels.hip", ["-ffp-contract=off"]) in SOURCES


def test_launcher_refuses_by_name_before_any_launch():
    """the argument checks run on the host before a launch, so they can be exercised without a GPU: no pointer is dereferenced.  (The
    buffer is sized for the largest shape below and lives on the GPU where there is one, so that even a check that had stopped
    refusing would stay inside it.)"""
    from cfgpp_amd import _lib
    from cfgpp_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    buf = torch.zeros(4 * 2049 * 8 + 8, dtype=torch.float32, device="cuda" if torch.cuda.is_available() else "cpu")
    p = buf.data_ptr() + (-buf.data_ptr()) % 16

    def call(a=1.0, s=1.0, B=1, rows=1, C=4, h0=8, w0=8, h=8, w=8, mode=0, src=p, noise=p, x=p):
        rc = lib.cfgpp_img2img_start(x, src, noise, None, a, s, B, rows, C, h0, w0, h, w, mode, 0, 0, None)
        return rc, _lib.last_error()
    for kw, word in ((dict(h0=16, mode=2), "downscaling is not built"), (dict(mode=4), "mode=4"), (dict(h0=4, w0=4), "identity"),
                     (dict(rows=2, B=3), "src_rows=2"), (dict(C=1, h=3, w=3, h0=3, w0=3), "multiple of 4"), (dict(a=0.0, s=0.0), "nothing to write"),
                     (dict(a=float("nan")), "not finite"), (dict(src=None), "needs src"), (dict(noise=None), "noise or seeds_host"),
                     (dict(x=p + 4), "aligned"), (dict(x=None), "null pointer"), (dict(h=2049, mode=2), "sides in"),
                     (dict(B=0), "B=0")):
        rc, msg = call(**kw)
        assert rc < 0 and word in msg, (kw, rc, msg)
