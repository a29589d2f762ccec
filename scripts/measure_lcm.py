"""What LCM sampling costs: the fused step against the DDIM step and against the three-launch alternative it replaces, a forward of
a guidance-embedded UNet against a plain one, and the flagship benchmark against a checkout of the parent commit.

    python scripts/measure_lcm.py [--parts steps,forward,bench] [--parent DIR] [--dir profiles/lcm] [--batch 4]

Each part writes ``<dir>/<part>.json``; every call then renders ``<dir>/README.md`` from the parts present (plus ``<dir>/accuracy.md``,
the figures the GPU tests print, kept by hand).  Needs the MI355X; there is no CPU fallback.

steps    cfgpp_step_lcm (noise drawn in the kernel), cfgpp_step_lcm fed a noise tensor, cfgpp_step_ddim, and the three launches the
         fused step replaces (torch.randn_like + cfgpp_step_ddim + one torch add of the noise) at the SD1.5 batch-8 and SDXL batch-2
         latent sizes: 200 calls between device events, 5 rounds, the variants alternating inside a round; median us per call and
         the bytes the step has to move (16 B per element) over that time.
forward  one engine with time_cond_proj_dim = 256 (SD15_LCM) and one without (SD15), synthetic weights, ``--batch`` chains (2 x batch
         rows): 10 forwards between device events, four pairs, order alternating.
bench    ``bench.py --gpus 1 --steps 20 --warmup 5`` in this tree and in ``--parent`` (a built checkout of the parent commit), three
         alternating runs each.  The feature is off there: the expectation is "inside the run-to-run spread".
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

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
    from cfgpp_amd import _lib, engine as E
    from cfgpp_amd.lcm import step_coeffs
    from cfgpp_amd.schedule import SchedulerTables
    tb = SchedulerTables(4)
    coef = step_coeffs(tb, 499, 499, False, "cuda")     # a unit-gain step (t_prev = t): the in-place latent stays finite over a window
    ddim = (coef[0], coef[1], coef[4], coef[5])
    out = dict(build=_lib.build_id(), device=torch.cuda.get_device_name(0), calls=200, rounds=5, sizes=[])
    for name, shape in (("SD1.5 batch 8", (8, 4, 64, 64)), ("SDXL batch 2", (2, 4, 128, 128))):
        g = torch.Generator().manual_seed(0)
        z = torch.randn(shape, generator=g).cuda()
        den = torch.empty_like(z)
        m_uc, m_c = (torch.randn(shape, generator=g).half().cuda() for _ in range(2))
        noise = torch.randn(shape, generator=g).cuda()
        seeds = list(range(shape[0]))

        def three():
            n = torch.randn_like(z)
            E.step_ddim(z, den, m_uc, m_c, 1.5, ddim, False, False)
            z.add_(n, alpha=coef[5])
        variants = {
            "step_lcm (noise in the kernel)": lambda: E.step_lcm(z, den, m_uc, m_c, 1.5, coef, False, False, seeds=seeds, draw=1),
            "step_lcm (noise tensor)": lambda: E.step_lcm(z, den, m_uc, m_c, 1.5, coef, False, False, noise=noise),
            "step_ddim": lambda: E.step_ddim(z, den, m_uc, m_c, 1.5, ddim, False, False),
            "randn_like + step_ddim + add": three,
        }
        for fn in variants.values():                 # warm up: code objects, allocator
            for _ in range(20):
                fn()
                z.copy_(noise)                       # (the latent would drift to inf over hundreds of in-place steps)
        us = {k: [] for k in variants}
        order = list(variants)
        for r in range(out["rounds"]):
            for k in (order if r % 2 == 0 else order[::-1]):
                z.copy_(noise)
                us[k].append(timed(variants[k], out["calls"]))
        n = z.numel()
        out["sizes"].append(dict(name=name, shape=list(shape), elements=n, us={k: [round(v, 3) for v in vs] for k, vs in us.items()},
                                 median_us={k: round(statistics.median(vs), 3) for k, vs in us.items()},
                                 step_GBps={k: round(16.0 * n / statistics.median(vs) / 1e3, 1) for k, vs in us.items()}))
    return out


def part_forward(batch):
    import torch
    os.environ["CFGPP_TUNE_CACHE"] = "0"            # the engines tune their own tiles, here
    from cfgpp_amd import _lib
    from cfgpp_amd.hip_engine import HipEngine
    from cfgpp_amd.lcm import guidance_scale_embedding
    from cfgpp_amd.unet_config import SD15, SD15_LCM
    g = torch.Generator().manual_seed(0)
    uc = (torch.randn(1, 77, 768, generator=g) * 0.5).half().cuda()
    c = (torch.randn(batch, 77, 768, generator=g) * 0.5).half().cuda()
    z = torch.randn(batch, 4, 64, 64, generator=g).cuda()
    engines = {"plain (sd15)": HipEngine(SD15, max_batch=batch), "time_cond 256 (sd15_lcm)": HipEngine(SD15_LCM, max_batch=batch)}
    engines["time_cond 256 (sd15_lcm)"].set_guidance_embedding(guidance_scale_embedding(8.5, 256))
    launches = {}
    for k, e in engines.items():
        e.set_context(uc, c)
        for _ in range(30):                          # in-situ tile tuning runs inside the first forwards
            e.predict(z, 500.0)
        torch.cuda.synchronize()
        launches[k] = sum(v["launches"] for v in e.unet.profile(z, 500.0).values())
    ms = {k: [] for k in engines}
    order = list(engines)
    for p in range(4):
        for k in (order if p % 2 == 0 else order[::-1]):
            ms[k].append(timed(lambda: engines[k].predict(z, 500.0), 10) / 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    a, b = order
    return dict(build=_lib.build_id(), device=torch.cuda.get_device_name(0), rows=2 * batch, latent=[64, 64], forwards_per_window=10,
                ms_per_forward={k: [round(x, 4) for x in v] for k, v in ms.items()}, median_ms={k: round(v, 4) for k, v in med.items()},
                spread_pct={k: round(100 * (max(v) - min(v)) / med[k], 3) for k, v in ms.items()}, launches=launches,
                time_cond_vs_plain_pct=round(100 * (med[b] / med[a] - 1), 3))


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
    L = ["# LCM sampling: measurements on the MI355X", "",
         "Written by `scripts/measure_lcm.py` from the part files next to it (`steps.json`, `forward.json`, `bench.json`); the accuracy",
         "section is `accuracy.md`, the figures the GPU tests print.  A part that is absent has not been measured.", ""]
    s = load("steps")
    L += ["## The fused step", ""]
    if s:
        L += [f"{s['device']}, `{s['build']}`; {s['calls']} calls between device events, {s['rounds']} rounds, variants alternating; median us per call",
              "and the step's own traffic (16 B per element) over that time.  Both latent sizes hold 131072 elements (2 MiB of step traffic):",
              "back-to-back calls of that size measure the stream's launch rate more than the memory system, so read the differences between",
              "the variants - what a launch costs or saves per sampling step - not the GB/s column as a share of the HBM peak.", ""]
        for z in s["sizes"]:
            L += [f"**{z['name']}** ({'x'.join(str(v) for v in z['shape'])}, {z['elements']} elements)", "", "| variant | median us | all rounds | GB/s of step traffic |",
                  "|---|---|---|---|"]
            L += [f"| {k} | {z['median_us'][k]} | {', '.join(str(v) for v in z['us'][k])} | {z['step_GBps'][k]} |" for k in z["us"]]
            L += [""]
    else:
        L += ["not measured", ""]
    f = load("forward")
    L += ["## Forward of a guidance-embedded UNet", ""]
    if f:
        L += [f"{f['device']}, `{f['build']}`; SD1.5 topology, {f['rows']} rows at 64 x 64, synthetic weights, {f['forwards_per_window']} forwards per window,",
              "four pairs, order alternating.", "", "| engine | median ms | windows | spread % | launches per forward |", "|---|---|---|---|---|"]
        L += [f"| {k} | {f['median_ms'][k]} | {', '.join(str(v) for v in f['ms_per_forward'][k])} | {f['spread_pct'][k]} | {f['launches'][k]} |"
              for k in f["median_ms"]]
        L += ["", f"time_cond against plain: {f['time_cond_vs_plain_pct']:+} % of the median.", ""]
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
    ap.add_argument("--parts", default="steps,forward")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--dir", default=os.path.join(HERE, "profiles", "lcm"))
    ap.add_argument("--batch", type=int, default=4)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    for part in [p for p in a.parts.split(",") if p]:
        if part not in ("steps", "forward", "bench"):
            raise SystemExit(f"--parts: unknown part {part!r}")
        res = part_steps() if part == "steps" else part_forward(a.batch) if part == "forward" else part_bench(a.parent)
        with open(os.path.join(a.dir, part + ".json"), "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps({part: res}), flush=True)
    render(a.dir)


if __name__ == "__main__":
    main()
