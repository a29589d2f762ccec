"""What DPM++ 2M / 3M SDE sampling costs: the fused step against the launches of the ancestral loop it stands in for, a sampling step
of `dpm++_2m_sde_cfg++` against the existing Karras-sigma solvers, and the flagship benchmark against a checkout of the parent commit.

    python scripts/measure_sde.py [--parts steps,sampling,bench] [--parent DIR] [--dir profiles/sde] [--nfe 10]

Each part writes ``<dir>/<part>.json``; every call then renders ``<dir>/README.md`` from the parts present (plus ``<dir>/accuracy.md``,
the figures the GPU tests print, kept by hand).  Needs the MI355X; there is no CPU fallback.

steps     cfgpp_step_sde (3M, CFG++, two history terms, noise drawn in the kernel; the same with a noise tensor; 2M CFG with one
          history term) against the four launches of one Euler-ancestral CFG++ step of ``_ancestral_loop`` with noise="philox"
          (kdiff_input, step_kdiff, philox_normal, the noise lincomb) at the SD1.5 batch-8 and SDXL batch-2 latent sizes: 200 calls
          between device events, 5 rounds, the variants alternating inside a round; median us per call.
sampling  one engine per family (SD1.5 batch 8 at 64 x 64, SDXL batch 2 at 128 x 128, synthetic weights) shared by the solvers;
          ``--nfe`` steps per job, two warm-up jobs each, then three alternating timed jobs; ms per sampling step (job time / steps;
          SDXL's `dpm++_2m_cfgpp` makes one UNet call fewer than it has steps).
bench     ``bench.py --gpus 1 --steps 20 --warmup 5`` in this tree and in ``--parent`` (a built checkout of the parent commit), three
          alternating runs each.  The feature is off there: the expectation is "inside the run-to-run spread".
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls        # us per call


def part_steps():
    import torch
    from cfgpp_amd import _lib, coeffs as K, engine as E
    from cfgpp_amd.schedule import SchedulerTables
    from cfgpp_amd.sde import sde_coeffs
    sig = SchedulerTables(20).karras_sigmas()
    i = 10
    c3 = sde_coeffs(sig, i, "3m", "midpoint", 1.0, 1.0, True, 2)
    c2 = sde_coeffs(sig, i, "2m", "midpoint", 1.0, 1.0, False, 1)
    sigma = sig[i]
    euler = [0.6, float(sigma), 0.0, K.divisor(sigma.item(), "cuda"), float(sig[i + 1]), 0.0, 0.0, 1.0, 0.0]
    s_in = K.kdiff_input_scale_sd(sigma, "cuda")
    out = dict(build=_lib.build_id(), device=torch.cuda.get_device_name(0), calls=200, rounds=5, sizes=[])
    for name, shape in (("SD1.5 batch 8", (8, 4, 64, 64)), ("SDXL batch 2", (2, 4, 128, 128))):
        g = torch.Generator().manual_seed(0)
        x0 = (torch.randn(shape, generator=g) * float(sigma)).cuda()
        x, den, h1, h2, h3 = (torch.empty_like(x0) for _ in range(5))
        xc = torch.empty_like(x0, dtype=torch.float16)
        m_uc, m_c = (torch.randn(shape, generator=g).half().cuda() for _ in range(2))
        noise = torch.randn(shape, generator=g).cuda()
        h1.copy_(x0), h2.copy_(x0)
        xh, denh, xch, nbuf = x0.half(), torch.empty_like(xc), torch.empty_like(xc), torch.empty_like(xc)
        seeds = list(range(shape[0]))

        def ancestral():
            E.kdiff_input(xh, xch, s_in, 0)
            E.step_kdiff(xh, denh, None, m_uc, m_c, euler, 1, False, True, False)
            E.philox_normal(nbuf, seeds, 1, 1)
            E.lincomb(xh, xh, nbuf, None, 0.5, 0.0, 2)
        variants = {
            "step_sde 3M CFG++ (noise in the kernel)": lambda: E.step_sde(x, den, xc, h1, h2, h3, m_uc, m_c, 0.6, c3, True, 2, False, seeds=seeds, draw=1),
            "step_sde 3M CFG++ (noise tensor)": lambda: E.step_sde(x, den, xc, h1, h2, h3, m_uc, m_c, 0.6, c3, True, 2, False, noise=noise),
            "step_sde 2M CFG (noise in the kernel)": lambda: E.step_sde(x, den, xc, h1, None, h3, m_uc, m_c, 7.5, c2, False, 1, False, seeds=seeds, draw=1),
            "euler_a_cfg++ step: kdiff_input + step_kdiff + philox_normal + lincomb": ancestral,
        }

        def reset():                                 # (an in-place latent would drift over hundreds of steps)
            x.copy_(x0)
            xh.copy_(x0)
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
    from cfgpp_amd import _lib, latent_diffusion, latent_sdxl
    from cfgpp_amd.sde import get_sde_solver
    out = dict(build=_lib.build_id(), device=torch.cuda.get_device_name(0), nfe=nfe, families=[])
    sc = types.SimpleNamespace(num_sampling=nfe)
    for fam, batch, names in (("SD1.5 batch 8 (64 x 64)", 8, ("dpm++_2m_sde_cfg++", "euler_a_cfg++", "dpm++_2m_cfg++")),
                              ("SDXL batch 2 (128 x 128)", 2, ("dpm++_2m_sde_cfg++", "euler_cfg++", "dpm++_2m_cfgpp"))):
        xl = fam.startswith("SDXL")
        mod = latent_sdxl if xl else latent_diffusion
        solvers, kw = {}, dict(solver_config=sc, device="cuda", max_batch=batch)
        for n in names:
            s = get_sde_solver(n, model="sdxl" if xl else "sd15", **kw) if n.endswith("_sde_cfg++") else mod.get_solver(n, **kw)
            kw.setdefault("engine", s.engine)        # one engine (one set of tuned tiles) for the family
            kw.setdefault("text_encoder", s.text_encoder)
            solvers[n] = s
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
                ms[n].append(1e3 * (time.perf_counter() - t0) / nfe)
        out["families"].append(dict(name=fam, ms_per_step={n: [round(v, 4) for v in vs] for n, vs in ms.items()},
                                    median_ms={n: round(statistics.median(vs), 4) for n, vs in ms.items()}))
        del solvers, kw
        torch.cuda.empty_cache()
    return out


def part_bench(parent):
    if not parent or not os.path.exists(os.path.join(parent, "bench.py")):
        raise SystemExit("--parent DIR: a built checkout of the parent commit (its bench.py is run there)")
    trees = {"this tree": HERE, "parent": os.path.abspath(parent)}
    runs = {k: [] for k in trees}
    order = list(trees)
    for r in range(3):
        for k in (order if r % 2 == 0 else order[::-1]):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=trees[k], capture_output=True,
                               text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
            if p.returncode != 0 or not line:
                raise SystemExit(f"bench.py in {k} failed (rc={p.returncode}): {p.stdout[-1500:]} {p.stderr[-1500:]}")
            j = json.loads(line[-1])
            runs[k].append(dict(value=j["value"], ms_per_step=j.get("ms_per_step"), build=j.get("config", {}).get("build_id")))
            print(k, runs[k][-1], flush=True)
    med = {k: statistics.median(x["value"] for x in v) for k, v in runs.items()}
    return dict(cmd="bench.py --gpus 1 --steps 20 --warmup 5", unit="images/sec", runs=runs, median={k: round(v, 4) for k, v in med.items()},
                spread_pct={k: round(100 * (max(x["value"] for x in v) - min(x["value"] for x in v)) / med[k], 3) for k, v in runs.items()},
                this_vs_parent_pct=round(100 * (med["this tree"] / med["parent"] - 1), 3))


def render(d):
    def load(name):
        p = os.path.join(d, name + ".json")
        return json.load(open(p)) if os.path.exists(p) else None
    L = ["# DPM++ 2M / 3M SDE sampling: measurements on the MI355X", "",
         "Written by `scripts/measure_sde.py` from the part files next to it (`steps.json`, `sampling.json`, `bench.json`); the accuracy",
         "section is `accuracy.md`, the figures the GPU tests print.  A part that is absent has not been measured.", ""]
    s = load("steps")
    L += ["## The fused step", ""]
    if s:
        L += [f"{s['device']}, `{s['build']}`; {s['calls']} calls between device events, {s['rounds']} rounds, variants alternating; median us per call.",
              "Both latent sizes hold 131072 elements (at most 30 B each for the fused step): back-to-back calls of that size measure the",
              "stream's launch rate more than the memory system, so read the differences between the variants - what a launch costs or",
              "saves per sampling step.", ""]
        for z in s["sizes"]:
            L += [f"**{z['name']}** ({'x'.join(str(v) for v in z['shape'])}, {z['elements']} elements)", "", "| variant | median us | all rounds |",
                  "|---|---|---|"]
            L += [f"| {k} | {z['median_us'][k]} | {', '.join(str(v) for v in z['us'][k])} |" for k in z["us"]]
            L += [""]
    else:
        L += ["not measured", ""]
    f = load("sampling")
    L += ["## A sampling step", ""]
    if f:
        L += [f"{f['device']}, `{f['build']}`; synthetic weights, one engine per family shared by the solvers, {f['nfe']} steps per job, two warm-up",
              "jobs each, then three alternating timed jobs (host clock around the job, device synchronised); ms per sampling step = job / steps.", ""]
        for fam in f["families"]:
            L += [f"**{fam['name']}**", "", "| solver | median ms per step | jobs |", "|---|---|---|"]
            L += [f"| {k} | {fam['median_ms'][k]} | {', '.join(str(v) for v in fam['ms_per_step'][k])} |" for k in fam["median_ms"]]
            L += [""]
        L += ["SDXL's `dpm++_2m_cfgpp` makes `steps - 1` UNet calls per job (the reference's loop), hence its lower figure; SDXL has no `euler_a`",
              "solver, so `euler_cfg++` stands in.  The sampler arithmetic is a few launches next to a UNet forward of hundreds: the solvers of a",
              "family differ by less than the jobs of one solver do.", ""]
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
    ap.add_argument("--dir", default=os.path.join(HERE, "profiles", "sde"))
    ap.add_argument("--nfe", type=int, default=10)
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
