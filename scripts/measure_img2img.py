"""What the img2img / hires-fix start costs: the fused start launch against the torch composition it replaces, and the flagship benchmark
against a checkout of the parent commit.

    python scripts/measure_img2img.py [--parts start,bench] [--parent DIR] [--dir profiles/img2img]

Each part writes ``<dir>/<part>.json``; every call then renders ``<dir>/README.md`` from the parts present (plus ``<dir>/accuracy.md``,
the figures the GPU tests print, kept by hand).  Needs the MI355X; there is no CPU fallback.

start   cfgpp_img2img_start at the SD1.5 batch-8 (64 x 64) and SDXL batch-2 (128 x 128) latent sizes, fp16 source at half the size,
        bilinear, fp32 destination, a = 1, s = sigma: with the noise drawn in the kernel, and with a noise tensor already on the device -
        against the torch composition it replaces: F.interpolate(bilinear) on the device, host randn + upload, mul, add, cast (and the
        same without the host randn, the noise already on the device).  The bicubic and fp16-destination forms are timed too.  200 calls
        between device events, 5 rounds, the variants alternating inside a round; median us per call.  The host-randn variant is timed
        by the host clock around synchronised calls (its cost is on the host), 20 calls a round.
bench   ``bench.py --gpus 1 --steps 20 --warmup 5`` in this tree and in ``--parent`` (a built checkout of the parent commit), three
        alternating runs each.  The feature is off there: the expectation is "inside the run-to-run spread".
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "scripts"))

from measure_sde import part_bench, timed  # noqa: E402


def part_start():
    import torch
    import torch.nn.functional as F
    from cfgpp_amd import _lib, engine as E
    sigma = 3.0
    out = dict(build=_lib.build_id(), device=torch.cuda.get_device_name(0), calls=200, host_calls=20, rounds=5, sizes=[])
    for name, shape in (("SD1.5 batch 8", (8, 4, 64, 64)), ("SDXL batch 2", (2, 4, 128, 128))):
        B, C, h, w = shape
        g = torch.Generator().manual_seed(0)
        src = torch.randn((B, C, h // 2, w // 2), generator=g).half().cuda()
        noise = torch.randn(shape, generator=g).cuda()
        x32, x16 = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda", dtype=torch.float16)
        seeds = list(range(B))

        def torch_form(n):
            return (F.interpolate(src.float(), size=(h, w), mode="bilinear", align_corners=False) + sigma * n).to(torch.float32)

        def torch_host():
            return torch_form(torch.randn(shape, generator=g).cuda())
        device = {
            "fused, bilinear, noise drawn in the kernel": lambda: E.img2img_start(x32, src, 1.0, sigma, "bilinear", seeds=seeds),
            "fused, bilinear, noise tensor": lambda: E.img2img_start(x32, src, 1.0, sigma, "bilinear", noise=noise),
            "fused, bicubic, noise drawn in the kernel": lambda: E.img2img_start(x32, src, 1.0, sigma, "bicubic", seeds=seeds),
            "fused, bilinear, fp16 destination, noise drawn in the kernel": lambda: E.img2img_start(x16, src, 1.0, sigma, "bilinear", seeds=seeds),
            "torch: interpolate, mul, add, cast (noise on the device)": lambda: torch_form(noise),
        }
        host = {
            "torch: host randn + upload, interpolate, mul, add, cast": torch_host,
            "fused, bilinear, host randn + upload": lambda: E.img2img_start(x32, src, 1.0, sigma, "bilinear",
                                                                            noise=torch.randn(shape, generator=g).cuda()),
        }
        for fn in list(device.values()) + list(host.values()):      # warm up: code objects, allocator
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in list(device) + list(host)}
        order = list(device)
        for r in range(out["rounds"]):
            for k in (order if r % 2 == 0 else order[::-1]):
                us[k].append(timed(device[k], out["calls"]))
            for k, fn in host.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(out["host_calls"]):
                    fn()
                torch.cuda.synchronize()
                us[k].append(1e6 * (time.perf_counter() - t0) / out["host_calls"])
        out["sizes"].append(dict(name=name, shape=list(shape), elements=x32.numel(), us={k: [round(v, 3) for v in vs] for k, vs in us.items()},
                                 median_us={k: round(statistics.median(vs), 3) for k, vs in us.items()}))
    return out


def render(d):
    def load(name):
        p = os.path.join(d, name + ".json")
        return json.load(open(p)) if os.path.exists(p) else None
    L = ["# img2img and latent hires fix: measurements on the MI355X", "",
         "Written by `scripts/measure_img2img.py` from the part files next to it (`start.json`, `bench.json`); the accuracy section is",
         "`accuracy.md`, the figures the GPU tests print.  A part that is absent has not been measured.", ""]
    s = load("start")
    L += ["## The start launch", ""]
    if s:
        L += [f"{s['device']}, `{s['build']}`; {s['calls']} calls between device events, {s['rounds']} rounds, variants alternating; median us per call.",
              f"The two host-randn variants are timed by the host clock around {s['host_calls']} synchronised calls a round: their cost is the host's",
              "generator and the upload.  Both latent sizes hold 131072 elements: back-to-back device calls of that size measure the stream's",
              "launch rate more than the memory system - one launch against torch's four or five.", ""]
        for z in s["sizes"]:
            L += [f"**{z['name']}** ({'x'.join(str(v) for v in z['shape'])}, {z['elements']} elements; source fp16 at half the size)", "",
                  "| variant | median us | all rounds |", "|---|---|---|"]
            L += [f"| {k} | {z['median_us'][k]} | {', '.join(str(v) for v in z['us'][k])} |" for k in z["us"]]
            L += [""]
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
    ap.add_argument("--parts", default="start")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--dir", default=os.path.join(HERE, "profiles", "img2img"))
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    for part in [p for p in a.parts.split(",") if p]:
        if part not in ("start", "bench"):
            raise SystemExit(f"--parts: unknown part {part!r}")
        res = part_start() if part == "start" else part_bench(a.parent)
        with open(os.path.join(a.dir, part + ".json"), "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps({part: res}), flush=True)
    render(a.dir)


if __name__ == "__main__":
    main()
