"""The case table of cfgpp_img2img_start (include/cfgpp_img2img.h), shared by tests/test_img2img_cases_cpu.py (the model against
torch-fp64, a correct kernel's fp32 restatement and the planted faults against the bound) and tests/test_gpu_img2img_step.py (the
kernel against the model).  The smallest shapes at which the kernel can go wrong; C = 4 throughout.

Inputs are seeded normals with planted large-magnitude pixels (the corners, the last row / column, an interior checker), so that a
wrong tap, edge or weight moves an element by far more than the bound - the convention of the attention and norm tables."""
from __future__ import annotations

import itertools

import numpy as np

import img2img_ref as M

C = 4
# (name, (h0, w0), (h, w)): identity; exactly 2x; non-integer scales that differ per axis; every tap clamps; odd h and w % 4 != 0
# (Philox groups straddle image rows and planes); a second larger shape
SHAPES = [("id8", (8, 8), (8, 8)), ("4to8", (4, 4), (8, 8)), ("5x3to8", (5, 3), (8, 8)), ("1to4", (1, 1), (4, 4)),
          ("6to9x10", (6, 6), (9, 10)), ("8to12x20", (8, 8), (12, 20))]
RESAMPLERS = ("nearest-exact", "bilinear", "bicubic")


def _case(name, hw0, hw, mode, x_half, src_half, B=3, src_rows=None, a=0.8125, s=0.59375, noise="tensor", seed=0):
    return dict(name=name, hw0=hw0, hw=hw, mode=mode, x_half=x_half, src_half=src_half, B=B, src_rows=B if src_rows is None else src_rows,
                a=a, s=s, noise=noise, seed=seed)


def _table():
    out = []
    k = 0
    for (sname, hw0, hw), (xh, sh) in itertools.product(SHAPES, itertools.product((False, True), (False, True))):
        modes = ("identity",) if hw0 == hw else RESAMPLERS
        for mode in modes:
            k += 1
            out.append(_case(f"{sname}-{mode}-x{'16' if xh else '32'}-s{'16' if sh else '32'}", hw0, hw, mode, xh, sh, seed=k))
    # one source row broadcast to 3 chains; one launch more than PHILOX_ROWS carries (both noise forms); the in-kernel draw; a = 0 with
    # a NULL source; s = 0 with NULL noise and NULL seeds
    out.append(_case("bcast-bilinear", (6, 6), (9, 10), "bilinear", False, True, src_rows=1, seed=101))
    out.append(_case("bcast-bicubic-philox", (5, 3), (8, 8), "bicubic", True, False, src_rows=1, noise="philox", seed=102))
    out.append(_case("b33-bilinear", (4, 4), (8, 8), "bilinear", False, False, B=33, seed=103))
    out.append(_case("b33-bicubic-philox", (6, 6), (9, 10), "bicubic", False, True, B=33, noise="philox", seed=104))
    out.append(_case("philox-6to9x10", (6, 6), (9, 10), "bilinear", False, False, noise="philox", seed=105))
    out.append(_case("philox-id8-x16", (8, 8), (8, 8), "identity", True, True, noise="philox", seed=106))
    out.append(_case("a0-null-src", (8, 8), (8, 8), "identity", False, False, a=0.0, s=14.5, seed=107))
    out.append(_case("a0-null-src-x16-philox", (9, 10), (9, 10), "identity", True, False, a=0.0, s=14.5, noise="philox", seed=108))
    out.append(_case("s0-null-noise", (6, 6), (9, 10), "bicubic", False, True, s=0.0, noise=None, seed=109))
    out.append(_case("s0-null-noise-id-x16", (8, 8), (8, 8), "identity", True, False, s=0.0, noise=None, seed=110))
    return out


CASES = _table()
BY_NAME = {c["name"]: c for c in CASES}


def make_inputs(case):
    """-> dict(src_parent [B, C, h0, w0] float64 holding values exact in the source dtype (the source is its first ``src_rows`` rows;
    None for a == 0), noise [B, C, h, w] float32 or None, seeds list or None)"""
    rng = np.random.default_rng(1000 + case["seed"])
    B, (h0, w0), (h, w) = case["B"], case["hw0"], case["hw"]
    src = None
    if case["a"] != 0.0:
        src = rng.standard_normal((B, C, h0, w0))
        src[:, :, 0, 0] += 64.0                                  # the corners and the far edges: clamping, broadcasts
        src[:, :, -1, -1] -= 48.0
        src[:, :, -1, :] += 24.0
        src[:, :, :, -1] -= 20.0
        yy, xx = np.meshgrid(np.arange(h0), np.arange(w0), indexing="ij")
        src += 12.0 * (((yy + 2 * xx) % 3) - 1.0)                 # an interior pattern no two neighbouring taps share
        src += 8.0 * np.arange(B).reshape(B, 1, 1, 1)            # rows differ: a wrong source row is loud
        src = src.astype(np.float16 if case["src_half"] else np.float32).astype(np.float64)
    noise = seeds = None
    if case["noise"] == "tensor":
        noise = rng.standard_normal((B, C, h, w)).astype(np.float32)
    elif case["noise"] == "philox":
        seeds = [int(v) for v in rng.integers(0, 2 ** 63 - 1, B)]
    return dict(src_parent=src, noise=noise, seeds=seeds)


def model(case, inp, dtype=np.float64, faults=()):
    """(x, magnitude) of tests/img2img_ref.py for one case"""
    src = None if inp["src_parent"] is None else inp["src_parent"][: case["src_rows"]]
    return M.start(src, inp["noise"], case["a"], case["s"], case["B"], case["hw"][0], case["hw"][1], M.MODES[case["mode"]],
                   case["x_half"], dtype, faults, src_parent=inp["src_parent"], seeds=inp["seeds"], C=C)
