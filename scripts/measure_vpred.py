"""What v-prediction costs the DDIM loop, and the forward time of an SD2.1-shaped UNet.

    python scripts/measure_vpred.py [--pairs 4] [--nfe 50] [--batch 8] [--out FILE.jsonl]

One process, one SD1.5 engine (synthetic weights, batch 8, 64 x 64 latents, tiles tuned by itself) shared by three `ddim_cfg++`
solvers: epsilon (the untouched path), v-prediction, and v-prediction with guidance_rescale = 0.7.  `--pairs` times the three are
run one after the other, order alternating; a run is one 50-NFE `sample(return_latents=True)` timed with device events, reported
per step (UNet forward + update).  The spread between equal runs of one state is the noise of the box.  The v loop replaces one
step launch by one step launch; rescale adds one small launch per step.

Then a second engine: `SD21_BASE` (865.9 M parameters, 64-wide heads, linear projections, 1024-wide context) with synthetic
weights at 16 rows, 64 x 64: forward time, and that its output is finite.

One JSON line per run, then one "summary" line per part.
"""
import argparse
import json
import os
import statistics
import sys
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--nfe", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    os.environ["CFGPP_TUNE_CACHE"] = "0"            # the engines tune their own tiles, here
    import torch
    from cfgpp_amd import _lib
    from cfgpp_amd.hip_engine import HipEngine
    from cfgpp_amd.latent_diffusion import get_solver
    from cfgpp_amd.unet_config import SD15, SD21_BASE
    out = open(a.out, "w") if a.out else None

    def say(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    B = a.batch
    eng = HipEngine(SD15, max_batch=B)
    say(ready=True, build=_lib.build_id(), device=torch.cuda.get_device_name(0), net="sd15", batch=B, nfe=a.nfe)
    sc = types.SimpleNamespace(num_sampling=a.nfe)
    states = {"epsilon": {}, "v": dict(prediction_type="v_prediction"), "v_rescale": dict(prediction_type="v_prediction", guidance_rescale=0.7)}
    solvers = {k: get_solver("ddim_cfg++", solver_config=sc, device="cuda", unet_config=SD15, max_batch=B, engine=eng,
                             scalar_semantics="cuda", **kw) for k, kw in states.items()}
    g = torch.Generator().manual_seed(0)
    uc = (torch.randn(1, 77, SD15.cross_attention_dim, generator=g) * 0.5).half().cuda()
    c = (torch.randn(B, 77, SD15.cross_attention_dim, generator=g) * 0.5).half().cuda()
    job = dict(cfg_guidance=0.6, prompt_embeds=(uc, c), seeds=list(range(B)), return_latents=True)

    def run(tag, pair):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        z0t, _ = solvers[tag].sample(**job)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.nfe
        say(state=tag, pair=pair, ms_per_step=round(ms, 4), finite=bool(torch.isfinite(z0t).all()))
        return ms

    for tag in states:                                # the in-situ tile tuning runs inside the first forwards
        solvers[tag].sample(**job)
    torch.cuda.synchronize()
    res = {k: [] for k in states}
    order = list(states)
    for i in range(a.pairs):
        for tag in (order if i % 2 == 0 else order[::-1]):
            res[tag].append(run(tag, i))
    med = {k: statistics.median(v) for k, v in res.items()}
    say(summary="ddim_cfg++ loop", ms_per_step={k: [round(x, 4) for x in v] for k, v in res.items()},
        median_ms_per_step={k: round(v, 4) for k, v in med.items()},
        spread_pct={k: round(100 * (max(v) - min(v)) / med[k], 3) for k, v in res.items()},
        v_vs_epsilon_pct=round(100 * (med["v"] / med["epsilon"] - 1), 3),
        rescale_vs_v_pct=round(100 * (med["v_rescale"] / med["v"] - 1), 3),
        rescale_us_per_step=round(1e3 * (med["v_rescale"] - med["v"]), 1))
    del solvers, eng
    torch.cuda.empty_cache()

    rows = 16
    eng = HipEngine(SD21_BASE, max_batch=rows // 2)
    uc = (torch.randn(1, 77, SD21_BASE.cross_attention_dim, generator=g) * 0.5).half().cuda()
    c = (torch.randn(rows // 2, 77, SD21_BASE.cross_attention_dim, generator=g) * 0.5).half().cuda()
    z = torch.randn(rows // 2, 4, eng.H, eng.W, generator=g).cuda()
    eng.set_context(uc, c)
    for _ in range(40):
        eng.predict(z, 500.0)
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            eng.predict(z, 500.0)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 10)
    v = torch.cat(eng.predict(z, 999.0)).float()
    torch.cuda.synchronize()
    say(summary="sd21_base forward", rows=rows, latent=[eng.H, eng.W], ms_per_forward=[round(x, 4) for x in ms],
        median_ms=round(statistics.median(ms), 4), finite=bool(torch.isfinite(v).all()), out_rms=round(float(v.pow(2).mean().sqrt()), 4),
        device_GB=round(eng.device_bytes() / 1e9, 2), tflops=round(eng.flops_per_forward(rows) / statistics.median(ms) / 1e9, 1))


if __name__ == "__main__":
    main()
