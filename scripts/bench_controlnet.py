"""ControlNet cost on the HIP path: ms per UNet forward without and with a ControlNet attached (SD1.5 512x512 batch 8 = 16 rows,
SDXL 1024x1024 batch 2 = 4 rows, synthetic weights) and the conditioning embedding's one-off cost per job.  One JSON line
per case.

    python scripts/bench_controlnet.py [sd15|sdxl|all] [--iters N]

The residual add's share of a controlled forward by kernel name: run the same script under
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python scripts/bench_controlnet.py sd15 --iters 5
and read cn_residual_add_kernel against the total in the stats file.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cfgpp_amd import _lib  # noqa: E402
from cfgpp_amd.controlnet import HipControlNet, synth_controlnet_state_dict  # noqa: E402
from cfgpp_amd.hip_engine import HipEngine  # noqa: E402


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def case(name, B, iters):
    eng = HipEngine(name, max_batch=B)
    cfg = eng.cfg
    g = torch.Generator().manual_seed(0)
    uc = (torch.randn(1, 77, cfg.cross_attention_dim, generator=g) * 0.5).half()
    c = (torch.randn(B, 77, cfg.cross_attention_dim, generator=g) * 0.5).half()
    te = ti = None
    if cfg.addition_embed:
        te = (torch.randn(2 * B, cfg.addition_pooled_dim, generator=g) * 0.5).half()
        ti = torch.tensor([[8.0 * eng.H, 8.0 * eng.W, 0, 0, 8.0 * eng.H, 8.0 * eng.W]] * (2 * B))
    eng.set_context(uc.cuda(), c.cuda(), te, ti)
    z = torch.randn(B, 4, eng.H, eng.W, device="cuda")
    plain = timed(lambda: eng.predict(z, 500.0), iters)
    cn = HipControlNet(cfg, 2 * B, (eng.H, eng.W), device=eng.device.index).load_state_dict(synth_controlnet_state_dict(cfg)).finalize()
    img = torch.rand(1, 3, 8 * eng.H, 8 * eng.W, generator=g).cuda()
    embed = timed(lambda: cn.set_image(img), max(3, iters // 4))
    eng.set_control(cn, img, 1.0)
    controlled = timed(lambda: eng.predict(z, 500.0), iters)
    n = cn.num_residuals()
    eng.clear_control()
    out = dict(case=f"{name}_b{B}", rows=2 * B, latent=[eng.H, eng.W], ms_forward=round(plain, 3), ms_forward_controlnet=round(controlled, 3),
               overhead=round(controlled / plain - 1.0, 4), ms_embedding_once=round(embed, 3), residuals=n,
               controlnet_gb=round(cn.device_bytes() / 1e9, 3), build_id=_lib.build_id())
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", nargs="?", default="all", choices=("sd15", "sdxl", "all"))
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.which in ("sd15", "all"):
        case("sd15", 8, a.iters)
    if a.which in ("sdxl", "all"):
        case("sdxl", 2, a.iters)


if __name__ == "__main__":
    main()
