"""What a MultiDiffusion panorama step costs: the fused view step against the per-view composition it replaces, a whole step (the views'
forwards plus the one launch) at several view batch sizes, and the flagship benchmark against a checkout of the parent commit.

    python scripts/measure_panorama.py [--parts step,views,bench] [--parent DIR] [--dir profiles/panorama]

Each part writes ``<dir>/<part>.json``; every call then renders ``<dir>/README.md`` from the parts present (plus ``<dir>/accuracy.md``,
the figures the GPU tests print, kept by hand).  Needs the MI355X; there is no CPU fallback.

step     SD1.5's 64 x 256 latent panorama of 64 x 64 windows, stride 8, plain (25 views) and circular (32 views), one chain:
         cfgpp_step_ddim_views against the diffusers-style composition on the same buffers - per view a slice copy, cfgpp_step_ddim
         on it and two torch adds into value / count slices (two pieces each for a wrapped view), then one division, plus the
         cfgpp_views_gather that composition needs before the next forwards.  100 calls between device events, 5 rounds, alternating.
views    one SD1.5 engine (synthetic weights), the same panoramas: ms per sampling step - V / Vc forwards at 2 Vc rows and the one step
         launch - at each view batch size, and the 16-row forward of the text-to-image benchmark for scale.
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

PANO, WIN, STRIDE = (64, 256), (64, 64), 8
CO = (0.59, -1.0 / 0.8068, 0.8170, 0.5766)          # a representative step; c2 < 0: the GPU path's multiply by the reciprocal


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / calls        # us per call


def _geometry(circular, Vc=1):
    from cfgpp_amd.panorama import ViewGeometry
    return ViewGeometry(PANO[0], PANO[1], WIN[0], WIN[1], STRIDE, circular, Vc)


def _pieces(x0):
    """(panorama columns, window columns) of a view that starts at column x0: two pieces when it wraps"""
    Wp, w = PANO[1], WIN[1]
    if x0 + w <= Wp:
        return [(slice(x0, x0 + w), slice(0, w))]
    return [(slice(x0, Wp), slice(0, Wp - x0)), (slice(0, x0 + w - Wp), slice(Wp - x0, w))]


def part_step():
    import torch
    from cfgpp_amd import _lib, engine as E
    out = dict(build=_lib.build_id(), device=torch.cuda.get_device_name(0), calls=100, rounds=5, cases=[])
    for circular in (False, True):
        g = _geometry(circular)
        V, h, w = g.n_views, g.h, g.w
        gen = torch.Generator().manual_seed(0)
        z0 = torch.randn(1, 4, *PANO, generator=gen).cuda()
        eps = torch.randn(V, 2, 4, h, w, generator=gen).half().cuda()
        z, z0t = z0.clone(), torch.empty_like(z0)
        z_views = torch.empty(V, 4, h, w, device="cuda")
        value, value0, count = (torch.empty_like(z0) for _ in range(3))
        tmp, tmp0 = torch.empty(1, 4, h, w, device="cuda"), torch.empty(1, 4, h, w, device="cuda")
        views = g.views

        def fused():
            E.step_ddim_views(g, z, z0t, z_views, eps, 0.6, CO, False, True)

        def composed():
            value.zero_(), value0.zero_(), count.zero_()
            for v, (y0, x0) in enumerate(views):
                for ps, ws in _pieces(x0):
                    zc = z[:, :, y0:y0 + h, ps].contiguous()
                    z0c = torch.empty_like(zc)
                    E.step_ddim(zc, z0c, eps[v, 0, :, :, ws].contiguous(), eps[v, 1, :, :, ws].contiguous(), 0.6, CO, False, True)
                    value[:, :, y0:y0 + h, ps] += zc
                    value0[:, :, y0:y0 + h, ps] += z0c
                    count[:, :, y0:y0 + h, ps] += 1
            torch.div(value, count, out=z)
            torch.div(value0, count, out=z0t)
            E.gather_views(g, z, z_views)

        variants = {"cfgpp_step_ddim_views (one launch)": fused, "per-view step_ddim + adds, div, gather": composed}
        # the two give the same bits (the composition IS the slice model)
        z.copy_(z0), fused()
        a = (z.clone(), z0t.clone(), z_views.clone())
        z.copy_(z0), composed()
        same = all(bool(torch.equal(x, y)) for x, y in zip(a, (z, z0t, z_views)))
        for fn in variants.values():
            for _ in range(10):
                z.copy_(z0), fn()
        us = {k: [] for k in variants}
        order = list(variants)
        calls = {order[0]: out["calls"], order[1]: 10}          # (the composition is hundreds of launches per call)
        for r in range(out["rounds"]):
            for k in (order if r % 2 == 0 else order[::-1]):
                z.copy_(z0)
                us[k].append(timed(variants[k], calls[k]))
        cov = torch.zeros(PANO, dtype=torch.int64)
        for y0, x0 in views:
            for ps, _ in _pieces(x0):
                cov[y0:y0 + h, ps] += 1
        elems = 4 * PANO[0] * PANO[1]
        nbytes = elems * 12 + int(cov.sum()) * 4 * 8          # z in, z / z0t out; per covering view 2 + 2 B eps in and 4 B scatter out
        med = {k: statistics.median(v) for k, v in us.items()}
        out["cases"].append(dict(circular=circular, views=V, coverage=[int(cov.min()), int(cov.max())], bytes=nbytes, same_bits=same,
                                 us={k: [round(x, 2) for x in v] for k, v in us.items()}, median_us={k: round(v, 2) for k, v in med.items()},
                                 fused_GBps=round(nbytes / med[order[0]] / 1e3, 1), composed_over_fused=round(med[order[1]] / med[order[0]], 1)))
    return out


def part_views():
    import torch
    os.environ["CFGPP_TUNE_CACHE"] = "0"            # the engine tunes its own tiles, here
    from cfgpp_amd import _lib
    from cfgpp_amd.hip_engine import HipEngine
    from cfgpp_amd.unet_config import SD15
    gen = torch.Generator().manual_seed(0)
    uc = (torch.randn(1, 77, 768, generator=gen) * 0.5).half().cuda()
    c = (torch.randn(1, 77, 768, generator=gen) * 0.5).half().cuda()
    eng = HipEngine(SD15, max_batch=32)
    out = dict(build=_lib.build_id(), device=torch.cuda.get_device_name(0), windows=3, cases=[])

    def warm(fn, n=30):                              # in-situ tile tuning runs inside the first forwards at a row count
        for _ in range(n):
            fn()
        torch.cuda.synchronize()

    z16 = torch.randn(8, 4, *WIN, generator=gen).cuda()
    eng.set_context(uc, c.expand(8, -1, -1))
    warm(lambda: eng.predict(z16, 500.0))
    out["forward_16_rows_ms"] = round(statistics.median(timed(lambda: eng.predict(z16, 500.0), 10) / 1e3 for _ in range(3)), 3)
    for circular, chunks in ((False, (1, 5, 25)), (True, (1, 4, 8, 32))):
        V = _geometry(circular).n_views
        z0 = torch.randn(1, 4, *PANO, generator=gen).cuda()
        row = dict(circular=circular, views=V, per_Vc=[])
        for Vc in chunks:
            g = _geometry(circular, Vc)
            z, z0t = z0.clone(), torch.empty_like(z0)
            z_views = torch.empty(V, 4, *WIN, device="cuda")
            eps = torch.empty(V // Vc, 2 * Vc, 4, *WIN, dtype=torch.float16, device="cuda")
            eng.set_context(uc.expand(Vc, -1, -1), c.expand(Vc, -1, -1))
            eng.gather_views(g, z, z_views)

            def forwards():
                for k in range(V // Vc):
                    eng.predict_into(z_views[k * Vc:(k + 1) * Vc], 500.0, eps[k])

            def step():
                forwards()
                eng.step_ddim_views(g, z, z0t, z_views, eps, 0.6, CO, False, True)

            warm(forwards, max(2, 30 // (V // Vc)))
            n = 3 if Vc < 4 else 5
            ms_step = [timed(step, n) / 1e3 for _ in range(out["windows"])]
            ms_fwd = [timed(forwards, n) / 1e3 for _ in range(out["windows"])]
            z.copy_(z0)
            us_launch = timed(lambda: eng.step_ddim_views(g, z, z0t, z_views, eps, 0.6, CO, False, True), 100)
            row["per_Vc"].append(dict(Vc=Vc, forwards=V // Vc, rows=2 * Vc, ms_per_step=[round(x, 3) for x in ms_step],
                                      median_ms_per_step=round(statistics.median(ms_step), 3), median_ms_forwards=round(statistics.median(ms_fwd), 3),
                                      step_launch_us=round(us_launch, 2)))
            print(json.dumps(row["per_Vc"][-1]), flush=True)
        out["cases"].append(row)
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
    L = ["# MultiDiffusion panoramas: measurements on the MI355X", "",
         "Written by `scripts/measure_panorama.py` from the part files next to it (`step.json`, `views.json`, `bench.json`); the accuracy",
         "section is `accuracy.md`, the figures the GPU tests print.  A part that is absent has not been measured.", ""]
    s = load("step")
    L += ["## The fused view step", ""]
    if s:
        L += [f"{s['device']}, `{s['build']}`; SD1.5 panorama latent {PANO[0]} x {PANO[1]}, windows {WIN[0]} x {WIN[1]}, stride {STRIDE}, one chain; the fused",
              f"step {s['calls']} calls between device events (the composition 10), {s['rounds']} rounds, alternating; median us per call.  The bytes are",
              "what the step has to move (z in, z and z0t out, per covering view 4 B of eps in and 4 B of scatter out); at this size the",
              "launch is short enough that back-to-back calls measure the stream's launch rate as much as the memory system.", "",
              "| padding | views | coverage min / max | bytes | fused us | composition us | composition / fused | fused GB/s | same bits |", "|---|---|---|---|---|---|---|---|---|"]
        for c in s["cases"]:
            k0, k1 = list(c["median_us"])
            L += [f"| {'circular' if c['circular'] else 'plain'} | {c['views']} | {c['coverage'][0]} / {c['coverage'][1]} | {c['bytes']} | {c['median_us'][k0]} | "
                  f"{c['median_us'][k1]} | {c['composed_over_fused']} | {c['fused_GBps']} | {c['same_bits']} |"]
        L += [""]
    else:
        L += ["not measured", ""]
    v = load("views")
    L += ["## A sampling step at several view batch sizes", ""]
    if v:
        L += [f"{v['device']}, `{v['build']}`; one SD1.5 engine, synthetic weights, one chain; a step = V / Vc forwards at 2 Vc rows plus the one step",
              f"launch; {v['windows']} windows of 3 - 5 steps between device events.  For scale: the 16-row forward of the text-to-image benchmark",
              f"takes {v['forward_16_rows_ms']} ms here.", "", "| padding | views | Vc | forwards x rows | ms per step (median) | windows | forwards alone ms | step launch us |",
              "|---|---|---|---|---|---|---|---|"]
        for c in v["cases"]:
            for r in c["per_Vc"]:
                L += [f"| {'circular' if c['circular'] else 'plain'} | {c['views']} | {r['Vc']} | {r['forwards']} x {r['rows']} | {r['median_ms_per_step']} | "
                      f"{', '.join(str(x) for x in r['ms_per_step'])} | {r['median_ms_forwards']} | {r['step_launch_us']} |"]
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
    ap.add_argument("--parts", default="step,views")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--dir", default=os.path.join(HERE, "profiles", "panorama"))
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    for part in [p for p in a.parts.split(",") if p]:
        if part not in ("step", "views", "bench"):
            raise SystemExit(f"--parts: unknown part {part!r}")
        res = part_step() if part == "step" else part_views() if part == "views" else part_bench(a.parent)
        with open(os.path.join(a.dir, part + ".json"), "w") as fh:
            json.dump(res, fh, indent=1)
        print(json.dumps({part: res}), flush=True)
    render(a.dir)


if __name__ == "__main__":
    main()
