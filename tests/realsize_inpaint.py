"""The real-size inpaint-UNet case - ONE definition of the inputs, used by

* ``tests/golden/make_inpaint_golden.py`` (build container, CPU): runs ``oracle.unet_ref.UNetRef`` on ``SD15_INPAINT`` once
  and commits its fp32 output as ``tests/golden/realsize_sd15_inpaint_fwd.npz``;
* ``tests/test_gpu_inpaint.py`` (-m gpu): starts ``python tests/realsize_inpaint.py`` as a subprocess (under a time limit);
  the HIP forward runs there, is compared with the fixture, and prints one JSON line.

A synthetic-weight SD1.5 inpaint UNet at 512 x 512 (64 x 64 latent), 2 UNet rows (uc, c) over one latent and one image
condition (mask + masked-image latent, the broadcast cond_rows = 1 form) - diffusers' per-step
``torch.cat([latent_model_input, mask, masked_image_latents], dim=1)`` as the engine's conv_in gather.
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "realsize_sd15_inpaint_fwd.npz")
TVAL = 501.0
TOL = 2.5e-3          # tests/test_gpu_unet.py: EPS_REL


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().float()


def inputs():
    hw = 64
    mask = torch.zeros(1, 1, hw, hw)
    mask[..., 12:44, 20:56] = 1.0
    return dict(z=rnd(1, 4, hw, hw, seed=60), cond=torch.cat([mask, rnd(1, 4, hw, hw, seed=61) * (1 - mask)], 1),
                ehs=rnd(2, 77, 768, scale=0.5, seed=62))


def oracle():
    from cfgpp_amd.unet_config import SD15_INPAINT
    from cfgpp_amd.weights import synth_state_dict
    from oracle.unet_ref import UNetRef
    i = inputs()
    x = torch.cat([i["z"], i["cond"]], 1)
    eps = UNetRef(SD15_INPAINT, synth_state_dict(SD15_INPAINT, 0))(torch.cat([x, x]), TVAL, i["ehs"])["sample"]
    return dict(eps=eps.float().numpy())


def hip():
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.unet_config import SD15_INPAINT
    from cfgpp_amd.weights import synth_state_dict_iter
    i = inputs()
    with np.load(FIXTURE) as f:
        gold = torch.from_numpy(f["eps"])
    net = HipUNet(SD15_INPAINT, max_rows=2, sample_hw=(64, 64))
    net.load_state_dict(synth_state_dict_iter(SD15_INPAINT, 0)).finalize()
    net.set_context(i["ehs"])
    net.image_condition(i["cond"].cuda())
    got = net.forward(i["z"].cuda(), TVAL).float().cpu()
    torch.cuda.synchronize()
    rel = float((got - gold).norm() / gold.norm())
    worst = max(float((got[r] - gold[r]).norm() / gold[r].norm()) for r in range(2))
    ok = bool(torch.isfinite(got).all()) and rel < TOL and worst < 4e-3
    from cfgpp_amd import _lib
    return dict(ok=ok, rel_l2=rel, worst_row=worst, tol=TOL, build_id=_lib.build_id())


def main():
    t0 = time.time()
    out = hip()
    out.update(case="sd15_inpaint_fwd", seconds=round(time.time() - t0, 1))
    print("REALSIZE_RESULT " + json.dumps(out), flush=True)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
