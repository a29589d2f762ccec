"""LoRA merge cost on the HIP path, real-size SD1.5 and SDXL with synthetic weights and a synthetic all-linear adapter (every 2-D
weight of the UNet) of rank 16 and rank 128.  One JSON line per (model, rank):

  ms_set_lora        `HipEngine.set_lora` end to end, host adapter tensors in (scale folding, upload, one merge kernel per key), device idle after
  ms_merge_kernels   the merge launches alone (operands already on the device): sum over keys, with the per-key min / median / max
  merge_gbps         bytes the merges move (saved base read + weight written, fp16, + the fp32 up / down) over ms_merge_kernels
  ms_restore         `set_lora([])`
  s_rebuild          the only path without the device merge: a new `HipEngine` from an (already merged) state dict - load_state_dict
                     (host repack) + finalize (upload, buffers), no tile tuning; the host-side merge itself is not even counted

    python scripts/bench_lora.py [sd15|sdxl|all] [--ranks 16,128]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cfgpp_amd import _lib  # noqa: E402
from cfgpp_amd.hip_engine import HipEngine  # noqa: E402
from cfgpp_amd.lora import ParsedLora  # noqa: E402
from cfgpp_amd.unet_config import CONFIGS, param_shapes  # noqa: E402
from cfgpp_amd.weights import synth_state_dict_iter  # noqa: E402


def adapter(cfg, rank, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = ParsedLora()
    for k, s in param_shapes(cfg).items():
        if len(s) == 2:
            out[k] = (torch.randn((s[0], rank), generator=g) * 0.02, torch.randn((rank, s[1]), generator=g) * (1.0 / s[1] ** 0.5), None)
    return out


def case(name, B, ranks):
    cfg = CONFIGS[name]
    sd = {k: v.half() for k, v in synth_state_dict_iter(cfg, 0)}        # stands for the merged state dict of the rebuild path
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng = HipEngine(cfg, max_batch=B, weights=sd)
    torch.cuda.synchronize()
    s_rebuild = time.perf_counter() - t0
    del sd
    for rank in ranks:
        ad = adapter(cfg, rank)
        eng.set_lora([(ad, 1.0)])                                       # first merge: saves the bases (not part of a switch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.set_lora([(ad, 0.5)])
        torch.cuda.synchronize()
        ms_set = (time.perf_counter() - t0) * 1e3
        per_key, nbytes = [], 0
        for k, (up, down, _) in ad.items():
            u, d = up.cuda(), down.cuda()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            eng.unet.lora(k, u, d)
            s.record()
            eng.unet.lora(k, u, d)
            e.record()
            torch.cuda.synchronize()
            per_key.append(s.elapsed_time(e))
            nbytes += 4 * up.shape[0] * down.shape[1] + 4 * (up.numel() + down.numel())
        t0 = time.perf_counter()
        eng.set_lora([])
        torch.cuda.synchronize()
        ms_restore = (time.perf_counter() - t0) * 1e3
        tot = sum(per_key)
        print(json.dumps(dict(case=f"{name}_rank{rank}", keys=len(ad), ms_set_lora=round(ms_set, 2), ms_merge_kernels=round(tot, 3),
                              ms_per_key=[round(min(per_key), 4), round(statistics.median(per_key), 4), round(max(per_key), 4)],
                              merge_gbps=round(nbytes / tot / 1e6, 1), ms_restore=round(ms_restore, 2), s_rebuild=round(s_rebuild, 2),
                              saved_base_gb=round(sum(2 * u.shape[0] * d.shape[1] for u, d, _ in ad.values()) / 1e9, 3),
                              build_id=_lib.build_id())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", nargs="?", default="all", choices=("sd15", "sdxl", "all"))
    ap.add_argument("--ranks", default="16,128")
    a = ap.parse_args()
    ranks = [int(r) for r in a.ranks.split(",")]
    if a.which in ("sd15", "all"):
        case("sd15", 8, ranks)
    if a.which in ("sdxl", "all"):
        case("sdxl", 2, ranks)


if __name__ == "__main__":
    main()
