"""-m gpu: the image tower's front end (vit_preprocess_kernel, vit_patch_rows_kernel of csrc/vision.hip) per element against the fp64
model of tests/vision_ref.py, which tests/test_vision_cpu.py pins to ``ip_adapter.preprocess_image``.

Preprocess bound, per element: 0.5 ulp16(want) + (taps_y + taps_x + 8) 2^-23 T / std_c with T = sum|w_y| sum|w_x| |x| - the fp16 rounding
of the output plus the fp32 accumulation of the two separable passes (vision_ref.preprocess_bound).  Patch rows: exact."""
import numpy as np
import pytest
import torch

import vision_ref as R
from test_gpu_configs import need_gpu, record
from test_gpu_small import guarded, guards_intact, untouched

pytestmark = pytest.mark.gpu

SIZES = [(300, 500), (224, 224), (100, 60), (1000, 700), (225, 224), (1, 1)]
_REF = {}


def ref(H, W, S):
    """image (2 samples) and fp64 model, once per (H, W, S): N = 1 uses the first sample of the same reference"""
    if (H, W, S) not in _REF:
        img = R.coordinate_image(2, H, W, seed=H + W)
        _REF[(H, W, S)] = (img, R.preprocess(img, S))
    return _REF[(H, W, S)]


@pytest.mark.parametrize("S", [28, 224])
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("H,W", SIZES)
def test_preprocess_per_element(H, W, N, S):
    need_gpu()
    import hip_ops as H_
    img, r = ref(H, W, S)
    x = torch.from_numpy(img[:N]).to(H_.DEV).contiguous()
    buf, out = guarded((N, 3, S, S), torch.float16)
    assert bool(untouched(out).all())
    H_.check(H_.lib().cfgpp_op_vit_preprocess(H_.P(x), N, H, W, S, H_.P(out), H_.stream()), "cfgpp_op_vit_preprocess")
    torch.cuda.synchronize()
    assert guards_intact(buf) and not bool(untouched(out).any())
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    want = r["want"][:N]
    bound = R.preprocess_bound(r)[:N]
    err = np.abs(got - want)
    worst = float((err / bound).max())
    record("vit_preprocess", H=H, W=W, N=N, S=S, worst_ratio=worst, max_abs=float(err.max()), taps=int(r["taps_y"].max()))
    print(f"{H}x{W} N={N} S={S}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}, taps {int(r['taps_y'].max())} x {int(r['taps_x'].max())}")
    assert worst <= 1.0, f"{int((err > bound).sum())} elements over the bound, worst {worst:.3f} x"


@pytest.mark.parametrize("N,S,ps", [(1, 28, 14), (2, 28, 14), (2, 224, 14), (1, 64, 32)])
def test_patch_rows_every_element(N, S, ps):
    """an input whose value encodes (n, c, y, x): position (p, c ps^2 + dy ps + dx) must hold pixel (c, ps py + dy, ps px + dx); pad
    columns exact zeros"""
    need_gpu()
    import hip_ops as H_
    K = 3 * ps * ps
    Kp = (K + 63) // 64 * 64
    idx = np.arange(N * 3 * S * S, dtype=np.int64).reshape(N, 3, S, S)
    pix = ((idx % 1009).astype(np.float32) - 500.0).astype(np.float16)            # exact in fp16, distinct within any 1009 consecutive elements
    pix += (np.arange(3, dtype=np.float16) * 0.25)[None, :, None, None]            # ... and the channel in the fraction (|v| < 512: exact)
    want = R.patch_rows(pix, ps, Kp)
    G = S // ps
    buf, rows = guarded((N * G * G, Kp), torch.float16)
    x = torch.from_numpy(pix).to(H_.DEV).contiguous()
    H_.check(H_.lib().cfgpp_op_vit_patch_rows(H_.P(x), H_.P(rows), N, S, ps, Kp, H_.stream()), "cfgpp_op_vit_patch_rows")
    torch.cuda.synchronize()
    assert guards_intact(buf) and not bool(untouched(rows).any())
    got = rows.cpu().numpy()
    assert np.array_equal(got.view(np.int16), want.view(np.int16))
    assert (Kp > K) == (ps == 14) and not got[:, K:].any()          # patch 14: 588 -> 640, 52 pad columns; patch 32: 3072, none


def test_refusals():
    need_gpu()
    import hip_ops as H_
    from cfgpp_amd._lib import CfgppError
    x = torch.zeros((1, 3, 30, 30), dtype=torch.float16, device=H_.DEV)
    buf, rows = guarded((4, 640), torch.float16)
    for S, ps, Kp, msg in ((30, 14, 640, "S=30 patch=14"), (28, 14, 576, "Kp=576")):
        with pytest.raises(CfgppError, match=msg):
            H_.check(H_.lib().cfgpp_op_vit_patch_rows(H_.P(x), H_.P(rows), 1, S, ps, Kp, H_.stream()), "cfgpp_op_vit_patch_rows")
    xf = torch.zeros((1, 3, 4, 4), dtype=torch.float32, device=H_.DEV)
    with pytest.raises(CfgppError, match="H=0"):
        H_.check(H_.lib().cfgpp_op_vit_preprocess(H_.P(xf), 1, 0, 4, 28, H_.P(rows), H_.stream()), "cfgpp_op_vit_preprocess")
    torch.cuda.synchronize()
    assert guards_intact(buf) and bool(untouched(rows).all())
