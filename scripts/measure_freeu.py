"""What FreeU costs a UNet forward, and that the off state launches what the plain engine launches.

    python scripts/measure_freeu.py [--nets sd15:16,sdxl:4] [--pairs 4] [--rounds 5] [--per 10] [--out FILE.jsonl]

Per net one worker process with ONE engine (synthetic weights, tiles tuned by itself; SD1.5 at a 64 x 64 latent, SDXL at 128 x 128).
Everything is interleaved on one device in one call:

  * `--pairs` times (FreeU off, FreeU on), order alternating: `--rounds` x `--per` back-to-back forwards timed with device events
    (the spread between equal runs of one state is the noise of the box), and three `cfgpp_unet_profile` passes per state: the
    forward's summed launch time, its launch count, and with FreeU on the six per-launch times of the FreeU ops;
  * sha1 of eps after a fixed forward: the off state must give one value throughout, (1, 1, 1, 1) must give the same.

One JSON line per run, then one "summary" line per net.  The off state runs the launches and computes the bits of an engine
without the feature (tests/test_gpu_freeu_net.py), so its time stands for the parent commit's on the same box.
A worker that fails ends the measurement.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREEU = (0.9, 0.2, 1.5, 1.6)


# ------------------------------------------------------------------------------------------------ worker (one net)
def worker(net, rows, pairs, rounds, per):
    sys.path.insert(0, HERE)
    import torch
    from cfgpp_amd import _lib
    from cfgpp_amd.hip_engine import HipEngine
    os.environ["CFGPP_TUNE_CACHE"] = "0"            # the engine tunes its own tiles, here
    B = rows // 2
    eng = HipEngine(net, max_batch=B)
    cfg = eng.cfg
    g = torch.Generator().manual_seed(0)
    uc = (torch.randn(1, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
    c = (torch.randn(B, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
    te = ti = None
    if cfg.addition_embed:
        te = (torch.randn(rows, cfg.addition_pooled_dim, generator=g) * 0.5).half()
        ti = torch.tensor([[1024., 1024, 0, 0, 1024, 1024]] * rows)
    z = torch.randn(B, 4, eng.H, eng.W, generator=g).cuda()
    eng.set_context(uc, c, te, ti)
    for _ in range(40):                              # the in-situ tile tuning runs inside the first forwards
        eng.predict(z, 500.0)
    torch.cuda.synchronize()

    def say(**kw):
        print("RESULT " + json.dumps(dict(net=net, rows=rows, **kw)), flush=True)

    def sha():
        eps = torch.cat(eng.predict(z, 500.0))
        torch.cuda.synchronize()
        return hashlib.sha1(eps.cpu().numpy().tobytes()).hexdigest()[:16]

    def run(spec, tag, pair):
        eng.set_freeu(spec)
        for _ in range(3):
            eng.predict(z, 500.0)
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                eng.predict(z, 500.0)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / per)
        prof_ms, launches, ops = [], 0, []
        for _ in range(3):
            pr = eng.unet.profile(z, 500.0, detail=True)
            lines = [ln.split("\t") for ln in pr["detail"].strip().split("\n")]
            prof_ms.append(sum(v["ms"] for k, v in pr.items() if k != "detail"))
            launches = sum(v["launches"] for k, v in pr.items() if k != "detail")
            ops.append([(r[2], float(r[3])) for r in lines if r[2].startswith("freeu ")])
        per_op = {name: round(statistics.median(o[i][1] for o in ops), 1) for i, (name, _) in enumerate(ops[0])}
        out = dict(state=tag, pair=pair, ms_per_forward=[round(x, 4) for x in ms], median_ms=round(statistics.median(ms), 4),
                   profile_ms=[round(x, 4) for x in prof_ms], profile_median_ms=round(statistics.median(prof_ms), 4), launches=launches,
                   freeu_ops_us=per_op, freeu_us=round(sum(per_op.values()), 1), eps_sha1=sha())
        say(**out)
        return out

    say(ready=True, build=_lib.build_id(), device=torch.cuda.get_device_name(0), latent=[eng.H, eng.W])
    res = {"off": [], "on": []}
    for i in range(pairs):
        for tag in (("off", "on") if i % 2 == 0 else ("on", "off")):
            res[tag].append(run(None if tag == "off" else FREEU, tag, i))
    unit = run((1, 1, 1, 1), "unit", pairs)
    med = {k: statistics.median(r["median_ms"] for r in v) for k, v in res.items()}
    pmed = {k: statistics.median(r["profile_median_ms"] for r in v) for k, v in res.items()}
    say(summary=True, freeu=list(FREEU), off_ms=[r["median_ms"] for r in res["off"]], on_ms=[r["median_ms"] for r in res["on"]],
        off_median_ms=round(med["off"], 4), on_median_ms=round(med["on"], 4), cost_pct=round(100 * (med["on"] / med["off"] - 1), 3),
        noise_pct={k: round(100 * (max(r["median_ms"] for r in v) - min(r["median_ms"] for r in v)) / med[k], 3) for k, v in res.items()},
        profile_off_median_ms=round(pmed["off"], 4), profile_on_median_ms=round(pmed["on"], 4),
        profile_cost_pct=round(100 * (pmed["on"] / pmed["off"] - 1), 3),
        freeu_us=statistics.median(r["freeu_us"] for r in res["on"]),
        freeu_us_pct_of_off_forward=round(100 * statistics.median(r["freeu_us"] for r in res["on"]) * 1e-3 / med["off"], 3),
        freeu_ops_us=res["on"][-1]["freeu_ops_us"], launches_off=res["off"][0]["launches"], launches_on=res["on"][0]["launches"],
        off_bits_one_value=len({r["eps_sha1"] for r in res["off"]}) == 1, on_bits_one_value=len({r["eps_sha1"] for r in res["on"]}) == 1,
        unit_scales_give_off_bits=unit["eps_sha1"] == res["off"][0]["eps_sha1"], unit_ms=unit["median_ms"])


# ------------------------------------------------------------------------------------------------ driver
def driver(a):
    out = open(a.out, "w") if a.out else None
    for spec in a.nets.split(","):
        net, rows = spec.split(":")
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--net", net, "--rows", rows, "--pairs", str(a.pairs),
                              "--rounds", str(a.rounds), "--per", str(a.per)], stdout=subprocess.PIPE, text=True, cwd=HERE)
        done = False
        for line in p.stdout:
            if line.startswith("RESULT "):
                print(line[7:], end="", flush=True)
                if out:
                    out.write(line[7:])
                    out.flush()
                done = done or '"summary": true' in line
        if p.wait() != 0 or not done:
            raise SystemExit(f"measure_freeu: the {net} worker ended without a summary (exit status {p.returncode})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="sd15:16,sdxl:4")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--net")
    ap.add_argument("--rows", type=int)
    a = ap.parse_args()
    if a.worker:
        worker(a.net, a.rows, a.pairs, a.rounds, a.per)
    else:
        driver(a)


if __name__ == "__main__":
    main()
