"""What DPM++ SDE sampling costs: the stage launch against its sibling cfgpp_step_sde, a sampling step of `dpm++_sde_cfg++` against
two steps of `dpm++_2m_sde_cfg++` (both make the same two UNet calls), and the flagship benchmark against a checkout of the parent
commit.

    python scripts/measure_dpmpp_sde.py [--parts steps,sampling,bench] [--parent DIR] [--dir profiles/dpmpp_sde] [--nfe 6]

Each part writes ``<dir>/<part>.json``; every call then renders ``<dir>/README.md`` from the parts present (plus ``<dir>/accuracy.md``,
the figures the GPU tests print, kept by hand).  Needs the MI355X; there is no CPU fallback.

steps     cfgpp_step_sde_stage as the solver launches it - stage A (base is x, out = x2; CFG++, one noise term drawn in the kernel),
          stage B (base = x2, in place on x, D2 into x2; two noise terms drawn in the kernel), stage B with both noise tensors given -
          against cfgpp_step_sde (2M, CFG++, one history term, noise drawn in the kernel) at the SD1.5 batch-8 and SDXL batch-2 latent
          sizes: 200 calls between device events, 5 rounds, the variants alternating inside a round; median us per call.
sampling  one engine per family (SD1.5 batch 8 at 64 x 64, SDXL batch 2 at 128 x 128, synthetic weights) shared by the two solvers;
          `dpm++_sde_cfg++` with ``--nfe`` steps (2 nfe - 1 UNet calls) against `dpm++_2m_sde_cfg++` with 2 nfe - 1 steps (as many UNet
          calls); two warm-up jobs each, then three alternating timed jobs; ms per UNet call and per job.
bench     ``bench.py --gpus 1 --steps 20 --warmup 5`` in this tree and in ``--parent`` (a built checkout of the parent commit), three
          alternating runs each.  The feature is off there: the expectation is "inside the run-to-run spread".
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "scripts"))

from measure_sde import part_bench, timed  # noqa: E402


def part_steps():
    import torch
    from cfgpp_amd import _lib, engine as E
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_coeffs
    from cfgpp_amd.schedule import SchedulerTables
    from cfgpp_amd.sde import sde_coeffs
    sig = SchedulerTables(20).karras_sigmas()
    i = 10
    a, b = dpmpp_sde_coeffs(sig, i, "A", 1.0, 1.0, True), dpmpp_sde_coeffs(sig, i, "B", 1.0, 1.0, True)
    c2 = sde_coeffs(sig, i, "2m", "midpoint", 1.0, 1.0, True, 1)
    out = dict(build=_lib.build_id(), device=torch.cuda.get_device_name(0), calls=200, rounds=5, sizes=[])
    for name, shape in (("SD1.5 batch 8", (8, 4, 64, 64)), ("SDXL batch 2", (2, 4, 128, 128))):
        g = torch.Generator().manual_seed(0)
        x0 = (torch.randn(shape, generator=g) * float(sig[i])).cuda()
        x, x2, den, h1, h2 = (torch.empty_like(x0) for _ in range(5))
        xc = torch.empty_like(x0, dtype=torch.float16)
        m_uc, m_c = (torch.randn(shape, generator=g).half().cuda() for _ in range(2))
        n1, n2 = (torch.randn(shape, generator=g).cuda() for _ in range(2))
        seeds = list(range(shape[0]))
        dr = dict(seeds=seeds, draw1=2, draw2=3)

        def stage_b(**kw):                           # D2 lands in x2: refill the base, outside the timed region it would not matter
            E.step_sde_stage(x, x2, x, x2, xc, m_uc, m_c, 0.6, b.coef, b.terms, False, **kw)
        variants = {
            "stage A CFG++ (18 B / element; n1 in the kernel)": lambda: E.step_sde_stage(x, x, x2, den, xc, m_uc, m_c, 0.6, a.coef, a.terms, False, **dr),
            "stage B CFG++ (22 B / element; n1, n2 in the kernel)": lambda: stage_b(**dr),
            "stage B CFG++ (noise tensors: 30 B / element)": lambda: stage_b(noise1=n1, noise2=n2),
            "step_sde 2M CFG++ (26 B / element; noise in the kernel)": lambda: E.step_sde(x, den, xc, h1, None, h2, m_uc, m_c, 0.6, c2, True, 1, False, seeds=seeds, draw=1),
        }

        def reset():                                 # (an in-place latent would drift over hundreds of steps)
            x.copy_(x0), x2.copy_(x0), h1.copy_(x0)
        for fn in variants.values():                 # warm up: code objects, allocator
            for _ in range(20):
                fn()
                reset()
        us = {k: [] for k in variants}
        order = list(variants)
        for r in range(out["rounds"]):
            for k in (order if r % 2 == 0 else order[::-1]):
                reset()
                us[k].append(timed(variants[k], out["calls"]))
        out["sizes"].append(dict(name=name, shape=list(shape), elements=x.numel(), us={k: [round(v, 3) for v in vs] for k, vs in us.items()},
                                 median_us={k: round(statistics.median(vs), 3) for k, vs in us.items()}))
    return out


def part_sampling(nfe):
    import torch
    os.environ["CFGPP_TUNE_CACHE"] = "0"            # the engines tune their own tiles, here
    from cfgpp_amd import _lib
    from cfgpp_amd.dpmpp_sde import get_dpmpp_sde_solver
    from cfgpp_amd.sde import get_sde_solver
    calls = 2 * nfe - 1
    out = dict(build=_lib.build_id(), device=torch.cuda.get_device_name(0), nfe=nfe, unet_calls=calls, families=[])
    for fam, batch in (("SD1.5 batch 8 (64 x 64)", 8), ("SDXL batch 2 (128 x 128)", 2)):
        xl = fam.startswith("SDXL")
        model = "sdxl" if xl else "sd15"
        kw = dict(device="cuda", max_batch=batch)
        two_stage = get_dpmpp_sde_solver("dpm++_sde_cfg++", model=model, solver_config=types.SimpleNamespace(num_sampling=nfe), **kw)
        kw.update(engine=two_stage.engine, text_encoder=two_stage.text_encoder)      # one engine (one set of tuned tiles) for the family
        multistep = get_sde_solver("dpm++_2m_sde_cfg++", model=model, solver_config=types.SimpleNamespace(num_sampling=calls), **kw)
        solvers = {f"dpm++_sde_cfg++, {nfe} steps": two_stage, f"dpm++_2m_sde_cfg++, {calls} steps": multistep}
        names = list(solvers)
        prompts = ["a cat"] * batch
        seeds = list(range(batch))

        def job(s):
            s._ctx_key = None
            if xl:
                s.sample(prompt1=["", prompts], prompt2=["", prompts], cfg_guidance=0.6, seeds=seeds, return_latents=True)
            else:
                s.sample(cfg_guidance=0.6, prompt=["", prompts], seeds=seeds, return_latents=True)
            torch.cuda.synchronize()
        ms = {n: [] for n in names}
        for n in names:                              # warm up: tile tuning runs inside the first forwards
            job(solvers[n])
            job(solvers[n])
        for r in range(3):
            for n in (names if r % 2 == 0 else names[::-1]):
                t0 = time.perf_counter()
                job(solvers[n])
                ms[n].append(1e3 * (time.perf_counter() - t0))
        out["families"].append(dict(name=fam, ms_per_job={n: [round(v, 3) for v in vs] for n, vs in ms.items()},
                                    median_ms_per_job={n: round(statistics.median(vs), 3) for n, vs in ms.items()},
                                    median_ms_per_unet_call={n: round(statistics.median(vs) / calls, 4) for n, vs in ms.items()}))
        del solvers, kw, two_stage, multistep
        torch.cuda.empty_cache()
    return out


def render(d):
    def load(name):
        p = os.path.join(d, name + ".json")
        return json.load(open(p)) if os.path.exists(p) else None
    L = ["# DPM++ SDE sampling: measurements on the MI355X", "",
         "Written by `scripts/measure_dpmpp_sde.py` from the part files next to it (`steps.json`, `sampling.json`, `bench.json`); the",
         "accuracy section is `accuracy.md`, the figures the GPU tests print.  A part that is absent has not been measured.", ""]
    s = load("steps")
    L += ["## The stage launch", ""]
    if s:
        L += [f"{s['device']}, `{s['build']}`; {s['calls']} calls between device events, {s['rounds']} rounds, variants alternating; median us per call.",
              "Both latent sizes hold 131072 elements (18 B each for stage A, 22 B for stage B: 2.4 / 2.9 MB a launch): back-to-back calls of",
              "that size measure the stream's launch rate more than the memory system, so the expectation is the sibling's figure.", ""]
        for z in s["sizes"]:
            L += [f"**{z['name']}** ({'x'.join(str(v) for v in z['shape'])}, {z['elements']} elements)", "", "| variant | median us | all rounds |",
                  "|---|---|---|"]
            L += [f"| {k} | {z['median_us'][k]} | {', '.join(str(v) for v in z['us'][k])} |" for k in z["us"]]
            L += [""]
    else:
        L += ["not measured", ""]
    f = load("sampling")
    L += ["## A sampling step against two multistep steps", ""]
    if f:
        L += [f"{f['device']}, `{f['build']}`; synthetic weights, one engine per family shared by the two solvers; `dpm++_sde_cfg++` with",
              f"{f['nfe']} steps and `dpm++_2m_sde_cfg++` with {f['unet_calls']} steps make {f['unet_calls']} UNet calls a job each; two warm-up jobs each, then",
              "three alternating timed jobs (host clock around the job, device synchronised).", ""]
        for fam in f["families"]:
            L += [f"**{fam['name']}**", "", "| solver | median ms per job | median ms per UNet call | jobs |", "|---|---|---|---|"]
            L += [f"| {k} | {fam['median_ms_per_job'][k]} | {fam['median_ms_per_unet_call'][k]} | {', '.join(str(v) for v in fam['ms_per_job'][k])} |"
                  for k in fam["median_ms_per_job"]]
            L += [""]
        L += ["One launch follows each UNet call in both solvers, so a two-stage step costs what two multistep steps cost.", ""]
    else:
        L += ["not measured", ""]
    b = load("bench")
    L += ["## bench.py against the parent commit", ""]
    if b:
        L += [f"`{b['cmd']}`, three alternating runs each, {b['unit']}.", "", "| tree | runs | median | spread % |", "|---|---|---|---|"]
        L += [f"| {k} | {', '.join(str(x['value']) for x in b['runs'][k])} | {b['median'][k]} | {b['spread_pct'][k]} |" for k in b["runs"]]
        L += ["", f"this tree against the parent: {b['this_vs_parent_pct']:+} % of the median (the feature is off in the benchmark).", ""]
    else:
        L += ["not measured", ""]
    acc = os.path.join(d, "accuracy.md")
    if os.path.exists(acc):
        L += [open(acc).read().rstrip(), ""]
    with open(os.path.join(d, "README.md"), "w") as fh:
        fh.write("\n".join(L))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="steps,sampling")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--dir", default=os.path.join(HERE, "profiles", "dpmpp_sde"))
    ap.add_argument("--nfe", type=int, default=6)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    for part in [p for p in a.parts.split(",") if p]:
        if part not in ("steps", "sampling", "bench"):
            raise SystemExit(f"--parts: unknown part {part!r}")
        res = part_steps() if part == "steps" else part_sampling(a.nfe) if part == "sampling" else part_bench(a.parent)
        with open(os.path.join(a.dir, part + ".json"), "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps({part: res}), flush=True)
    render(a.dir)


if __name__ == "__main__":
    main()
