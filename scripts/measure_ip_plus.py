"""What an IP-Adapter Plus (Resampler) image prompt costs: the once-per-job projection and the per-step forward.

    python scripts/measure_ip_plus.py [--nets sd15:16,sdxl:4] [--seq 257] [--pairs 4] [--rounds 5] [--per 10] [--out FILE.jsonl]

Per net one worker process with ONE engine (synthetic weights, tiles tuned by itself; SD1.5 at a 64 x 64 latent, SDXL at 128 x 128)
and a synthetic Resampler adapter of the shipped geometry (plus / plus-face SD1.5: E 1280, D 768, 12 heads, 16 tokens, 4 layers;
SDXL vit-h: D 1280, 20 heads, cross 2048).  Everything is interleaved on one device in one call:

  * the job: `--rounds` x `--per` calls of cfgpp_unet_image_context_seq, alternating between two buffers of hidden states so that
    every call projects (the engine identifies the hidden states by address), timed with device events; and the same count of
    cfgpp_op_perceiver_attention launches at the job's shape, `depth` per job - the perceiver kernel's share of the job;
  * `--pairs` times (adapter off, adapter on), order alternating: `--rounds` x `--per` back-to-back forwards timed with device
    events; the spread between equal runs of one state is the noise of the box.

One JSON line per run, then one "summary" line per net.  The off state runs the launches and computes the bits of an engine
without an adapter (tests/test_gpu_ip_plus.py), so its time stands for the parent commit's on the same box.
A worker that fails ends the measurement.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRY = dict(sd15=dict(embed_dim=1280, hidden_dim=768, heads=12, depth=4), sdxl=dict(embed_dim=1280, hidden_dim=1280, heads=20, depth=4))
N_IMG = 16


# ------------------------------------------------------------------------------------------------ worker (one net)
def worker(net, rows, seq, pairs, rounds, per):
    sys.path.insert(0, HERE)
    import torch
    from cfgpp_amd import _lib
    from cfgpp_amd.hip_engine import HipEngine
    from cfgpp_amd.ip_adapter import parse_ip_adapter, synthetic_ip_adapter
    os.environ["CFGPP_TUNE_CACHE"] = "0"            # the engine tunes its own tiles, here
    B = rows // 2
    eng = HipEngine(net, max_batch=B)
    cfg, geo = eng.cfg, GEOMETRY[net]
    ad = parse_ip_adapter(synthetic_ip_adapter(cfg, kind="plus", n_img=N_IMG, seed=1, **geo), cfg)
    eng.set_ip_adapter(ad)
    g = torch.Generator().manual_seed(0)
    uc = (torch.randn(1, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
    c = (torch.randn(B, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
    te = ti = None
    if cfg.addition_embed:
        te = (torch.randn(rows, cfg.addition_pooled_dim, generator=g) * 0.5).half()
        ti = torch.tensor([[1024., 1024, 0, 0, 1024, 1024]] * rows)
    z = torch.randn(B, 4, eng.H, eng.W, generator=g).cuda()
    hid = [torch.randn(rows, seq, geo["embed_dim"], generator=g).half().cuda() for _ in range(2)]
    eng.set_context(uc, c, te, ti)
    for _ in range(40):                              # the in-situ tile tuning runs inside the first forwards
        eng.predict(z, 500.0)
    torch.cuda.synchronize()
    lib, u = _lib.load(), eng.unet
    stream = torch.cuda.current_stream().cuda_stream

    def say(**kw):
        print("RESULT " + json.dumps(dict(net=net, rows=rows, seq=seq, **kw)), flush=True)

    def timed(fn):
        ms = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(per):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / per)
        return ms

    def job(i):
        _lib.check(lib.cfgpp_unet_image_context_seq(u._h, hid[i % 2].data_ptr(), rows, seq, geo["embed_dim"], ctypes.c_float(1.0), stream),
                   "cfgpp_unet_image_context_seq")

    say(ready=True, build=_lib.build_id(), device=torch.cuda.get_device_name(0), latent=[eng.H, eng.W], geometry=geo, n_img=N_IMG)
    for i in range(3):
        job(i)
    job_ms = timed(job)
    inner = geo["heads"] * 64
    q = torch.randn(rows, N_IMG, inner, generator=g).half().cuda()
    kvx = torch.randn(rows, seq, 2 * inner, generator=g).half().cuda()
    kvl = torch.randn(rows, N_IMG, 2 * inner, generator=g).half().cuda()
    o = torch.empty_like(q)

    def attn(i):
        for _ in range(geo["depth"]):
            _lib.check(lib.cfgpp_op_perceiver_attention(q.data_ptr(), kvx.data_ptr(), kvl.data_ptr(), o.data_ptr(), rows, geo["heads"], N_IMG,
                                                        seq, stream), "cfgpp_op_perceiver_attention")
    attn(0)
    attn_ms = timed(attn)
    macs = rows * (seq * geo["embed_dim"] * geo["hidden_dim"] + geo["depth"] * (
        (seq + N_IMG) * geo["hidden_dim"] * 2 * inner + 2 * N_IMG * geo["hidden_dim"] * inner + 2 * N_IMG * (seq + N_IMG) * inner
        + 8 * N_IMG * geo["hidden_dim"] ** 2) + N_IMG * geo["hidden_dim"] * cfg.cross_attention_dim)
    say(job=True, job_ms=[round(x, 4) for x in job_ms], job_median_ms=round(statistics.median(job_ms), 4),
        perceiver_ms=[round(x, 4) for x in attn_ms], perceiver_median_ms=round(statistics.median(attn_ms), 4), gflop=round(2e-9 * macs, 2))

    def run(tag, pair):
        if tag == "on":
            job(0)
        else:
            eng.set_image_embeds(None)
        for _ in range(3):
            eng.predict(z, 500.0)
        torch.cuda.synchronize()
        ms = timed(lambda i: eng.predict(z, 500.0))
        out = dict(state=tag, pair=pair, ms_per_forward=[round(x, 4) for x in ms], median_ms=round(statistics.median(ms), 4))
        say(**out)
        return out

    res = {"off": [], "on": []}
    for i in range(pairs):
        for tag in (("off", "on") if i % 2 == 0 else ("on", "off")):
            res[tag].append(run(tag, i))
    med = {k: statistics.median(r["median_ms"] for r in v) for k, v in res.items()}
    jm, am = statistics.median(job_ms), statistics.median(attn_ms)
    say(summary=True, job_median_ms=round(jm, 4), perceiver_median_ms=round(am, 4), perceiver_share_pct=round(100 * am / jm, 2),
        gflop=round(2e-9 * macs, 2), job_tflops=round(2e-9 * macs / jm, 2), off_ms=[r["median_ms"] for r in res["off"]],
        on_ms=[r["median_ms"] for r in res["on"]], off_median_ms=round(med["off"], 4), on_median_ms=round(med["on"], 4),
        cost_pct=round(100 * (med["on"] / med["off"] - 1), 3), job_pct_of_off_forward=round(100 * jm / med["off"], 2),
        noise_pct={k: round(100 * (max(r["median_ms"] for r in v) - min(r["median_ms"] for r in v)) / med[k], 3) for k, v in res.items()})


# ------------------------------------------------------------------------------------------------ driver
def driver(a):
    out = open(a.out, "w") if a.out else None
    for spec in a.nets.split(","):
        net, rows = spec.split(":")
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--net", net, "--rows", rows, "--seq", str(a.seq),
                              "--pairs", str(a.pairs), "--rounds", str(a.rounds), "--per", str(a.per)], stdout=subprocess.PIPE, text=True, cwd=HERE)
        done = False
        for line in p.stdout:
            if line.startswith("RESULT "):
                print(line[7:], end="", flush=True)
                if out:
                    out.write(line[7:])
                    out.flush()
                done = done or '"summary": true' in line
        if p.wait() != 0 or not done:
            raise SystemExit(f"measure_ip_plus: the {net} worker ended without a summary (exit status {p.returncode})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="sd15:16,sdxl:4")
    ap.add_argument("--seq", type=int, default=257)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--net")
    ap.add_argument("--rows", type=int)
    a = ap.parse_args()
    if a.worker:
        worker(a.net, a.rows, a.seq, a.pairs, a.rounds, a.per)
    else:
        driver(a)


if __name__ == "__main__":
    main()
