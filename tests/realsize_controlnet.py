"""The real-size ControlNet case - ONE definition of the inputs, used by

* ``tests/golden/make_controlnet_golden.py`` (build container, CPU): runs tests/controlnet_ref.py (ControlNetRef +
  controlled_unet on ``oracle.unet_ref.UNetRef``) on SD15 once and commits its fp32 output as
  ``tests/golden/realsize_sd15_controlnet_fwd.npz``;
* ``tests/test_gpu_controlnet.py`` (-m gpu): starts ``python tests/realsize_controlnet.py`` as a subprocess (under a time limit);
  the HIP forward runs there, is compared with the fixture, and prints one JSON line.

A synthetic-weight SD1.5 UNet with a synthetic-weight SD1.5 ControlNet at 512 x 512 (64 x 64 latent), 2 UNet rows (uc, c) over
one latent and one control image, conditioning scale 1.  At the shipped channel widths the skips' producers write GroupNorm
statistics that the residual add makes stale - the case the add's statistics handling is for.
"""
from __future__ import annotations

import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "realsize_sd15_controlnet_fwd.npz")
TVAL = 501.0
SCALE = 1.0
TOL = 2.5e-3          # tests/test_gpu_unet.py: EPS_REL


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().float()


def inputs():
    hw = 64
    yy, xx = torch.meshgrid(torch.arange(8 * hw), torch.arange(8 * hw), indexing="ij")
    edges = ((((xx // 37) + (yy // 53)) % 2) == 0).float()                 # a hard-edged pattern, like an edge / segmentation map
    img = torch.stack([edges, (xx.float() / (8 * hw)), 1 - edges * 0.5])[None]
    return dict(z=rnd(1, 4, hw, hw, seed=70), image=img.half().float(), ehs=rnd(2, 77, 768, scale=0.5, seed=72))


def oracle():
    from cfgpp_amd.controlnet import synth_controlnet_state_dict
    from cfgpp_amd.unet_config import SD15
    from cfgpp_amd.weights import synth_state_dict
    from controlnet_ref import ControlNetRef, controlled_unet
    from oracle.unet_ref import UNetRef
    i = inputs()
    zz = torch.cat([i["z"], i["z"]])
    down, mid = ControlNetRef(SD15, synth_controlnet_state_dict(SD15, 0))(zz, TVAL, i["ehs"], torch.cat([i["image"]] * 2), SCALE)
    eps = controlled_unet(UNetRef(SD15, synth_state_dict(SD15, 0)), zz, TVAL, i["ehs"], None, down, mid)
    return dict(eps=eps.float().numpy())


def hip():
    from cfgpp_amd.controlnet import HipControlNet, synth_controlnet_state_dict
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.unet_config import SD15
    from cfgpp_amd.weights import synth_state_dict_iter
    i = inputs()
    with np.load(FIXTURE) as f:
        gold = torch.from_numpy(f["eps"])
    net = HipUNet(SD15, max_rows=2, sample_hw=(64, 64))
    net.load_state_dict(synth_state_dict_iter(SD15, 0)).finalize()
    cn = HipControlNet(SD15, max_rows=2, sample_hw=(64, 64))
    cn.load_state_dict(synth_controlnet_state_dict(SD15, 0)).finalize()
    net.set_context(i["ehs"])
    cn.set_context(i["ehs"])
    plain = net.forward(i["z"].cuda(), TVAL).float().cpu()
    cn.set_image(i["image"].cuda())
    net.attach_control(cn, SCALE)
    got = net.forward(i["z"].cuda(), TVAL).float().cpu()
    torch.cuda.synchronize()
    rel = float((got - gold).norm() / gold.norm())
    worst = max(float((got[r] - gold[r]).norm() / gold[r].norm()) for r in range(2))
    moved = float((plain - gold).norm() / gold.norm())
    ok = bool(torch.isfinite(got).all()) and rel < TOL and worst < 4e-3 and moved > 10 * TOL
    from cfgpp_amd import _lib
    return dict(ok=ok, rel_l2=rel, worst_row=worst, uncontrolled_rel_l2=moved, tol=TOL, build_id=_lib.build_id())


def main():
    t0 = time.time()
    out = hip()
    out.update(case="sd15_controlnet_fwd", seconds=round(time.time() - t0, 1))
    print("REALSIZE_RESULT " + json.dumps(out), flush=True)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
