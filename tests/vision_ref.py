"""fp64 restatement of the image tower's front end (cfgpp_amd/csrc/vision.hip: vit_preprocess_kernel, vit_patch_rows_kernel) - numpy
only, no product code in here.

What it restates is ``cfgpp_amd.ip_adapter.preprocess_image``: short side to S with torch's antialiased bicubic
(``F.interpolate(mode="bicubic", antialias=True, align_corners=False)``), clamp to [0, 1], centre crop, CLIP mean / std.  Torch's filter,
per axis resized from ``n_in`` to ``n_out`` samples (tests/test_vision_cpu.py pins this file to torch on the CPU):
    scale = n_in / n_out;  support = 2 * max(scale, 1);  centre(i) = scale * (i + 0.5)
    xmin = max(0, int(centre - support + 0.5));  xsize = min(n_in, int(centre + support + 0.5)) - xmin
    w(k) = cubic((k + xmin - centre + 0.5) / max(scale, 1)), a = -0.5, then w /= sum(w)
The passes are separable, horizontal first; because both are linear the fp64 value does not depend on the order, the fp32 kernel's does.
"""
from __future__ import annotations

import numpy as np

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
A = -0.5


def cubic(x):
    x = np.abs(np.asarray(x, dtype=np.float64))
    near = ((A + 2) * x - (A + 3)) * x * x + 1
    far = ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return np.where(x < 1, near, np.where(x < 2, far, 0.0))


def window(i, n_in, n_out):
    """-> (xmin, xsize, centre, invscale) of output sample i"""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    centre = scale * (i + 0.5)
    xmin = max(0, int(centre - support + 0.5))
    xsize = min(n_in, int(centre + support + 0.5)) - xmin
    return xmin, xsize, centre, (1.0 / scale if scale >= 1.0 else 1.0)


def window_brute(i, n_in, n_out):
    """the same window by walking every input sample: those whose centre k + 0.5 lies in (centre - support, centre + support]"""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    centre = scale * (i + 0.5)
    ks = [k for k in range(n_in) if centre - support < k + 0.5 <= centre + support]
    return ks[0], len(ks)


def weight_matrix(n_in, n_out, first, count, fault=None):
    """[count, n_in] fp64: row r holds the normalised weights of output sample first + r.  ``fault``: "start_off_by_one" (the window
    starts one sample late) | "no_renormalise" (weights divided by the interior sum 1 instead of their own sum: wrong where the
    window is cut by the border)"""
    Wm = np.zeros((count, n_in), dtype=np.float64)
    taps = np.zeros(count, dtype=np.int64)
    for r in range(count):
        xmin, xsize, centre, inv = window(first + r, n_in, n_out)
        if fault == "start_off_by_one":
            xmin, xsize = min(xmin + 1, n_in - 1), max(1, min(xsize, n_in - xmin - 1))
        k = np.arange(xsize)
        w = cubic((k + xmin - centre + 0.5) * inv)
        if fault == "no_renormalise":
            w = w * inv                                  # the continuous filter integrates to max(scale, 1): the interior sum is ~1 after this
        else:
            tot = w.sum()
            w = w / tot if tot != 0 else w               # (only a faulted window can miss every non-zero tap)
        Wm[r, xmin:xmin + xsize] = w
        taps[r] = xsize
    return Wm, taps


def resized_size(H, W, S):
    """preprocess_image: ``max(size, round(H * size / min(H, W)))`` (Python's round: half to even) and the crop offsets"""
    s = S / min(H, W)
    nh, nw = max(S, round(H * s)), max(S, round(W * s))
    return nh, nw, (nh - S) // 2, (nw - S) // 2


def preprocess(img, S, fault=None):
    """img [N, 3, H, W] in [0, 1] -> dict(want [N, 3, S, S] fp64 pixel values, T = sum|w_y| sum|w_x| |x| per element (the magnitude the
    fp32 accumulation error scales with), taps_y [S], taps_x [S], resized [N, 3, S, S] = the crop before clamp and normalisation)"""
    x = np.asarray(img, dtype=np.float64)
    N, C, H, W = x.shape
    assert C == 3
    nh, nw, top, left = resized_size(H, W, S)
    Wy, ty = weight_matrix(H, nh, top, S, fault)
    Wx, tx = weight_matrix(W, nw, left, S, fault)
    res = np.einsum("yh,nchw,xw->ncyx", Wy, x, Wx, optimize=True)
    T = np.einsum("yh,nchw,xw->ncyx", np.abs(Wy), np.abs(x), np.abs(Wx), optimize=True)
    mean = np.asarray(CLIP_MEAN, dtype=np.float32).astype(np.float64)[None, :, None, None]
    std = np.asarray(CLIP_STD, dtype=np.float32).astype(np.float64)[None, :, None, None]
    want = (np.clip(res, 0.0, 1.0) - mean) / std
    return dict(want=want, T=T, taps_y=ty, taps_x=tx, resized=res, std=std)


def ulp16(v):
    """spacing of fp16 at |v| (normal range; 2^-24 below it)"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def preprocess_bound(r):
    """per element: 0.5 ulp16(want) + (taps_y + taps_x + 8) 2^-23 T / std_c - the output rounding plus fp32 accumulation of the two passes
    (one rounding per tap of each pass, 8 for the weights' own evaluation, normalisation, clamp and the mean / std arithmetic)"""
    taps = r["taps_y"][None, None, :, None] + r["taps_x"][None, None, None, :] + 8
    return 0.5 * ulp16(r["want"]) + taps * 2.0 ** -23 * r["T"] / r["std"]


def patch_rows(pix, ps, Kp):
    """pix [N, 3, S, S] -> [N * G * G, Kp]: row n G G + py G + px, column c ps^2 + dy ps + dx = pix[n, c, ps py + dy, ps px + dx]; pad columns 0"""
    pix = np.asarray(pix)
    N, C, S, _ = pix.shape
    G = S // ps
    out = np.zeros((N * G * G, Kp), dtype=pix.dtype)
    for n in range(N):
        for py in range(G):
            for px in range(G):
                out[(n * G + py) * G + px, :C * ps * ps] = pix[n, :, ps * py:ps * (py + 1), ps * px:ps * (px + 1)].reshape(-1)
    return out


def coordinate_image(N, H, W, seed=0):
    """[N, 3, H, W] float32 in [0, 1] whose value encodes (n, c, y, x) - a smooth ramp per axis plus seeded texture, so a transposition
    or a wrong plane is visible and the bicubic has something to interpolate"""
    g = np.random.default_rng(seed)
    y = np.arange(H, dtype=np.float64)[:, None] / max(H - 1, 1)
    x = np.arange(W, dtype=np.float64)[None, :] / max(W - 1, 1)
    out = np.empty((N, 3, H, W), dtype=np.float64)
    for n in range(N):
        for c in range(3):
            out[n, c] = 0.15 + 0.4 * y * (c + 1) / 3 + 0.25 * x * (n + 1) / (N + 1) + 0.2 * g.random((H, W))
    return np.clip(out, 0.0, 1.0).astype(np.float32)
