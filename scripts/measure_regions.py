"""What regional prompts cost a UNet forward: the region-masked cross-attention (cfgpp_op_attention_region, ONE launch per block over
77 R resident keys) against the plain 77-token forward, against the long-prompt forward of the same key count on the same engine,
and - the cross-attention launches alone - against R plain 77-key launches, the design it replaces.

    python scripts/measure_regions.py [--nets sd15:16,sdxl:4] [--pairs 4] [--rounds 5] [--per 10] [--out FILE.jsonl]

Per net one worker process with ONE engine at max_tokens = 308 (synthetic weights, tiles tuned by itself; SD1.5 at a 64 x 64 latent,
SDXL at 128 x 128).  For R = 2, 3, 4, `--pairs` times the states (plain 77 tokens, long 77 R tokens, regions R with a map of R
vertical stripes), order alternating: `--rounds` x `--per` back-to-back forwards timed with device events (the spread between equal
runs of one state is the noise of the box), and three `cfgpp_unet_profile` passes per state for the summed time of the
cross-attention launches and the launch count.  One JSON line per run, then one "summary" line per (net, R).
A worker that fails ends the measurement.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ worker (one net)
def worker(net, rows, pairs, rounds, per):
    sys.path.insert(0, HERE)
    import torch
    from cfgpp_amd import _lib
    from cfgpp_amd.hip_engine import HipEngine
    os.environ["CFGPP_TUNE_CACHE"] = "0"            # the engine tunes its own tiles, here
    B = rows // 2
    eng = HipEngine(net, max_batch=B, max_tokens=308)
    cfg = eng.cfg
    g = torch.Generator().manual_seed(0)
    uc = (torch.randn(1, 308, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
    c = (torch.randn(B, 308, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
    te = ti = None
    if cfg.addition_embed:
        te = (torch.randn(rows, cfg.addition_pooled_dim, generator=g) * 0.5).half()
        ti = torch.tensor([[1024., 1024, 0, 0, 1024, 1024]] * rows)
    z = torch.randn(B, 4, eng.H, eng.W, generator=g).cuda()

    def state(tokens, regions):
        eng.set_context(uc[:, :tokens].contiguous(), c[:, :tokens].contiguous(), te, ti)
        if regions:
            x = torch.arange(eng.W)[None, :].expand(eng.H, eng.W)
            eng.set_regions((x * regions // eng.W).clamp(max=regions - 1)[None], regions)
        else:
            eng.set_regions(None)

    state(77, 0)
    for _ in range(40):                              # the in-situ tile tuning runs inside the first forwards
        eng.predict(z, 500.0)
    torch.cuda.synchronize()

    def say(**kw):
        print("RESULT " + json.dumps(dict(net=net, rows=rows, **kw)), flush=True)

    def run(tag, tokens, regions, R, pair):
        state(tokens, regions)
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
        cross_us, launches = [], 0
        for _ in range(3):
            pr = eng.unet.profile(z, 500.0, detail=True)
            lines = [ln.split("\t") for ln in pr["detail"].strip().split("\n")]
            launches = sum(v["launches"] for k, v in pr.items() if k != "detail")
            cross_us.append(sum(float(r[3]) for r in lines if r[2].startswith("cross_attn ")))
        out = dict(state=tag, R=R, pair=pair, tokens=tokens, ms_per_forward=[round(x, 4) for x in ms], median_ms=round(statistics.median(ms), 4),
                   cross_attn_us=round(statistics.median(cross_us), 1), launches=launches)
        say(**out)
        return out

    say(ready=True, build=_lib.build_id(), device=torch.cuda.get_device_name(0), latent=[eng.H, eng.W])
    for R in (2, 3, 4):
        states = (("plain", 77, 0), ("long", 77 * R, 0), ("regions", 77 * R, R))
        res = {s[0]: [] for s in states}
        for i in range(pairs):
            for tag, tokens, regions in (states if i % 2 == 0 else states[::-1]):
                res[tag].append(run(tag, tokens, regions, R, i))
        med = {k: statistics.median(r["median_ms"] for r in v) for k, v in res.items()}
        cross = {k: statistics.median(r["cross_attn_us"] for r in v) for k, v in res.items()}
        say(summary=True, R=R, median_ms={k: round(v, 4) for k, v in med.items()},
            runs_ms={k: [r["median_ms"] for r in v] for k, v in res.items()},
            noise_pct={k: round(100 * (max(r["median_ms"] for r in v) - min(r["median_ms"] for r in v)) / med[k], 3) for k, v in res.items()},
            regions_vs_plain_pct=round(100 * (med["regions"] / med["plain"] - 1), 3),
            regions_vs_long_pct=round(100 * (med["regions"] / med["long"] - 1), 3),
            long_vs_plain_pct=round(100 * (med["long"] / med["plain"] - 1), 3),
            cross_attn_us={k: round(v, 1) for k, v in cross.items()},
            cross_attn_R_plain_launches_us=round(R * cross["plain"], 1),
            cross_attn_regions_vs_R_plain_pct=round(100 * (cross["regions"] / (R * cross["plain"]) - 1), 2),
            launches={k: v[0]["launches"] for k, v in res.items()})
    eng.set_regions(None)


# ------------------------------------------------------------------------------------------------ driver
def driver(a):
    out = open(a.out, "w") if a.out else None
    for spec in a.nets.split(","):
        net, rows = spec.split(":")
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--net", net, "--rows", rows, "--pairs", str(a.pairs),
                              "--rounds", str(a.rounds), "--per", str(a.per)], stdout=subprocess.PIPE, text=True, cwd=HERE)
        done = 0
        for line in p.stdout:
            if line.startswith("RESULT "):
                print(line[7:], end="", flush=True)
                if out:
                    out.write(line[7:])
                    out.flush()
                done += '"summary": true' in line
        if p.wait() != 0 or done != 3:
            raise SystemExit(f"measure_regions: the {net} worker ended without its three summaries (exit status {p.returncode})")


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
