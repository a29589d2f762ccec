"""The real-size FreeU case - ONE definition of the inputs, used by

* ``tests/golden/make_freeu_golden.py`` (CPU): runs tests/freeu_ref.py (FreeUUNetRef on ``oracle.unet_ref.UNetRef``) on SD15 once
  and commits its fp32 output as ``tests/golden/realsize_freeu_sd15.npz``, with the FreeU values it used;
* ``tests/test_gpu_freeu_net.py`` (-m gpu): starts ``python tests/realsize_freeu.py`` as a subprocess (under a time limit); the HIP
  forward runs there, is compared with the fixture, and prints one JSON line.

A synthetic-weight SD1.5 UNet at 512 x 512 (64 x 64 latent), 2 UNet rows (uc, c) over one latent: up_blocks.0 edits 8 x 8 planes
of 1280 + 1280 channels, up_blocks.1 16 x 16 planes of 1280 + 1280 / 640 channels.
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "realsize_freeu_sd15.npz")
TVAL = 501.0
FREEU = (0.9, 0.2, 1.5, 1.6)          # (s1, s2, b1, b2): the recorder's starting values; the fixture stores the ones it used
TOL = 2.5e-3                          # tests/test_gpu_realsize.py / tests/test_gpu_unet.py: EPS_REL


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().float()


def inputs():
    return dict(z=rnd(1, 4, 64, 64, seed=90), ehs=rnd(2, 77, 768, scale=0.5, seed=92))


def oracle():
    from cfgpp_amd.unet_config import SD15
    from cfgpp_amd.weights import synth_state_dict
    from freeu_ref import FreeUUNetRef
    i = inputs()
    zz = torch.cat([i["z"], i["z"]])
    sd = synth_state_dict(SD15, 0)
    plain = FreeUUNetRef(SD15, sd, None)(zz, TVAL, i["ehs"])["sample"]
    freeu = FREEU
    for _ in range(4):
        eps = FreeUUNetRef(SD15, sd, freeu)(zz, TVAL, i["ehs"])["sample"]
        moved = float((eps - plain).norm() / eps.norm())
        if moved > 10 * TOL:
            break
        freeu = tuple(1.0 + 2.0 * (v - 1.0) for v in freeu)          # twice as far from the identity
    assert moved > 10 * TOL, f"FreeU {freeu} moves the oracle by only {moved:.3e}"
    return dict(eps=eps.float().numpy(), moved=np.float32(moved), freeu=np.asarray(freeu, dtype=np.float32))


def hip():
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.unet_config import SD15
    from cfgpp_amd.weights import synth_state_dict_iter
    i = inputs()
    with np.load(FIXTURE) as f:
        gold = torch.from_numpy(f["eps"])
        freeu = tuple(float(v) for v in f["freeu"])
    net = HipUNet(SD15, max_rows=2, sample_hw=(64, 64))
    net.load_state_dict(synth_state_dict_iter(SD15, 0)).finalize()
    net.set_context(i["ehs"])
    plain = net.forward(i["z"].cuda(), TVAL).float().cpu()
    net.set_freeu(freeu)
    got = net.forward(i["z"].cuda(), TVAL).float().cpu()
    torch.cuda.synchronize()
    rel = float((got - gold).norm() / gold.norm())
    worst = max(float((got[r] - gold[r]).norm() / gold[r].norm()) for r in range(2))
    moved = float((plain - gold).norm() / gold.norm())
    ok = bool(torch.isfinite(got).all()) and rel < TOL and moved > 10 * TOL
    from cfgpp_amd import _lib
    return dict(ok=ok, rel_l2=rel, worst_row=worst, without_freeu_rel_l2=moved, freeu=freeu, tol=TOL, build_id=_lib.build_id())


def main():
    t0 = time.time()
    out = hip()
    out.update(case="sd15_freeu_fwd", seconds=round(time.time() - t0, 1))
    print("REALSIZE_RESULT " + json.dumps(out), flush=True)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
