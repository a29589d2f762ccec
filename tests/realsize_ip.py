"""The real-size IP-Adapter case - ONE definition of the inputs, used by

* ``tests/golden/make_ip_adapter_golden.py`` (build container, CPU): runs tests/ip_adapter_ref.py (IPUNetRef on
  ``oracle.unet_ref.UNetRef``) on SD15 once and commits its fp32 output as ``tests/golden/realsize_ip_sd15.npz``;
* ``tests/test_gpu_ip_adapter.py`` (-m gpu): starts ``python tests/realsize_ip.py`` as a subprocess (under a time limit); the
  HIP forward runs there, is compared with the fixture, and prints one JSON line.

A synthetic-weight SD1.5 UNet with a synthetic IP-Adapter (4 image tokens, embed_dim 1024: the geometry of ip-adapter_sd15) at
512 x 512 (64 x 64 latent), 2 UNet rows (uc with zero image embeds, c) over one latent, scale 1.  SD1.5 has all three kinds of
cross-attention: head dim 40 (fused kernel, ones-row denominator) and head dims 80 / 160 (text pass + image pass).
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "realsize_ip_sd15.npz")
TVAL = 501.0
SCALE = 1.0
N_IMG, EMBED = 4, 1024
TOL = 2.5e-3          # tests/test_gpu_realsize.py / tests/test_gpu_unet.py: EPS_REL


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().float()


def inputs():
    emb = rnd(2, EMBED, seed=83)
    emb[0] = 0                                  # the uncond row: diffusers' zeros_like
    return dict(z=rnd(1, 4, 64, 64, seed=80), ehs=rnd(2, 77, 768, scale=0.5, seed=82), emb=emb)


def adapter():
    from cfgpp_amd.ip_adapter import parse_ip_adapter, synthetic_ip_adapter
    from cfgpp_amd.unet_config import SD15
    return parse_ip_adapter(synthetic_ip_adapter(SD15, n_img=N_IMG, embed_dim=EMBED, seed=1), SD15)


def oracle():
    from cfgpp_amd.unet_config import SD15
    from cfgpp_amd.weights import synth_state_dict
    from ip_adapter_ref import IPUNetRef
    i = inputs()
    zz = torch.cat([i["z"], i["z"]])
    net = IPUNetRef(SD15, synth_state_dict(SD15, 0), adapter())
    eps = net.set_image(i["emb"], SCALE)(zz, TVAL, i["ehs"])["sample"]
    plain = net.set_image(None, 0.0)(zz, TVAL, i["ehs"])["sample"]
    moved = float((eps - plain).norm() / eps.norm())
    assert moved > 10 * TOL, f"the adapter moves the oracle by only {moved:.3e}"
    return dict(eps=eps.float().numpy(), moved=np.float32(moved))


def hip():
    from cfgpp_amd.engine import HipUNet
    from cfgpp_amd.unet_config import SD15
    from cfgpp_amd.weights import synth_state_dict_iter
    i = inputs()
    with np.load(FIXTURE) as f:
        gold = torch.from_numpy(f["eps"])
    net = HipUNet(SD15, max_rows=2, sample_hw=(64, 64))
    net.load_state_dict(synth_state_dict_iter(SD15, 0)).finalize()
    net.set_context(i["ehs"])
    plain = net.forward(i["z"].cuda(), TVAL).float().cpu()
    for k, v in adapter().items():
        net.ip_load(k, v)
    net.set_image_context(i["emb"], SCALE)
    got = net.forward(i["z"].cuda(), TVAL).float().cpu()
    torch.cuda.synchronize()
    rel = float((got - gold).norm() / gold.norm())
    worst = max(float((got[r] - gold[r]).norm() / gold[r].norm()) for r in range(2))
    moved = float((plain - gold).norm() / gold.norm())
    ok = bool(torch.isfinite(got).all()) and rel < TOL and moved > 10 * TOL
    from cfgpp_amd import _lib
    return dict(ok=ok, rel_l2=rel, worst_row=worst, without_adapter_rel_l2=moved, tol=TOL, build_id=_lib.build_id())


def main():
    t0 = time.time()
    out = hip()
    out.update(case="sd15_ip_adapter_fwd", seconds=round(time.time() - t0, 1))
    print("REALSIZE_RESULT " + json.dumps(out), flush=True)
    return 0 if out["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
