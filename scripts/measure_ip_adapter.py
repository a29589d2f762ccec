"""What the IP-Adapter costs a UNet forward, and that a build with the feature but no adapter costs what a build without it does.

    python scripts/measure_ip_adapter.py --other TREE [--nets sd15:16,sdxl:4] [--pairs 3] [--rounds 5] [--per 10] [--out FILE.jsonl]

TREE is a second checkout of this project with its own built library (the commit before the feature).  Per net two worker
processes stay alive, one per tree, each with ONE engine (synthetic weights, tiles tuned by itself); the driver hands them the GPU
in turn, so every comparison is interleaved on one device in one call:

  * `--pairs` times (this tree, other tree), order alternating: `--rounds` x `--per` back-to-back forwards without an adapter,
    timed with device events; the spread between equal runs of one tree is the noise of the box;
  * this tree with a 4-token and a 16-token synthetic adapter active (scale 1), a no-adapter run between them;
  * per mode three `cfgpp_unet_profile` passes: the cross-attention launches' summed time, their count, the forward's launch count.

One JSON line per run (ms per forward: every round and the median; sha1 of eps after a fixed forward - without an adapter it
must be the other tree's), then one "summary" line per net.  A worker that fails ends the measurement.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ worker (one tree, one net)
def worker(tree, net, rows, rounds, per):
    sys.path.insert(0, tree)
    import torch
    from cfgpp_amd import _lib
    from cfgpp_amd.hip_engine import HipEngine
    os.environ["CFGPP_TUNE_CACHE"] = "0"            # each engine tunes its own tiles, here
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
    state = {"n_img": 0}

    def say(**kw):
        print("RESULT " + json.dumps(kw), flush=True)

    def mode(n_img):
        if n_img == state["n_img"]:
            return
        if n_img == 0:
            eng.set_image_embeds(None)
            eng.set_ip_adapter(None)
        else:
            from cfgpp_amd.ip_adapter import parse_ip_adapter, synthetic_ip_adapter
            ad = parse_ip_adapter(synthetic_ip_adapter(cfg, n_img=n_img, seed=3), cfg)
            eng.set_ip_adapter(ad)
            emb = torch.randn(1, ad.embed_dim, generator=torch.Generator().manual_seed(5)).half()
            eng.set_image_embeds(emb, None, 1.0)
        state["n_img"] = n_img
        for _ in range(3):
            eng.predict(z, 500.0)
        torch.cuda.synchronize()

    say(ready=True, build=_lib.build_id(), device=torch.cuda.get_device_name(0))
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        n_img = int(cmd[1])
        mode(n_img)
        if cmd[0] == "time":
            ms = []
            for _ in range(rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(per):
                    eng.predict(z, 500.0)
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / per)
            eps = torch.cat(eng.predict(z, 500.0))
            torch.cuda.synchronize()
            say(n_img=n_img, ms_per_forward=[round(x, 4) for x in ms], median_ms=round(statistics.median(ms), 4),
                eps_sha1=hashlib.sha1(eps.cpu().numpy().tobytes()).hexdigest()[:16])
        elif cmd[0] == "profile":
            cross, count, launches = [], 0, 0
            for _ in range(3):
                pr = eng.unet.profile(z, 500.0, detail=True)
                rows_ = [ln.split("\t") for ln in pr["detail"].strip().split("\n")]
                x = [float(r[3]) for r in rows_ if r[2].startswith("cross_attn")]
                cross.append(sum(x))
                count = len(x)
                launches = sum(v["launches"] for k, v in pr.items() if k != "detail")
            say(n_img=n_img, cross_attn_us=[round(x, 1) for x in cross], cross_attn_median_us=round(statistics.median(cross), 1),
                cross_attn_ops=count, launches=launches)


# ------------------------------------------------------------------------------------------------ driver
class Worker:
    def __init__(self, tree, net, rows, a):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--net", net, "--rows", str(rows),
                                   "--rounds", str(a.rounds), "--per", str(a.per)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True, cwd=tree)
        self.ready = self.read()

    def read(self):
        for line in self.p.stdout:
            if line.startswith("RESULT "):
                return json.loads(line[7:])
        raise SystemExit(f"measure_ip_adapter: a worker ended without a result (exit status {self.p.wait()})")

    def ask(self, cmd):
        self.p.stdin.write(cmd + "\n")
        self.p.stdin.flush()
        return self.read()

    def close(self):
        if self.p.poll() is None:
            try:
                self.p.stdin.write("quit\n")
                self.p.stdin.flush()
            except OSError:
                pass
            self.p.wait(timeout=60)


def driver(a):
    out = open(a.out, "w") if a.out else None

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    other = os.path.abspath(a.other)
    for spec in a.nets.split(","):
        net, rows = spec.split(":")
        rows = int(rows)
        ws = {}
        try:
            ws["this"] = Worker(HERE, net, rows, a)
            ws["other"] = Worker(other, net, rows, a)
            for k, w in ws.items():
                emit(net=net, rows=rows, tree=k, **w.ready)
            plain = {"this": [], "other": []}
            sha = {"this": set(), "other": set()}
            for i in range(a.pairs):
                for k in (("this", "other") if i % 2 == 0 else ("other", "this")):
                    r = ws[k].ask("time 0")
                    plain[k].append(r["median_ms"])
                    sha[k].add(r["eps_sha1"])
                    emit(net=net, rows=rows, tree=k, run="no adapter", pair=i, **r)
            ip = {}
            for n_img in (4, 16):
                r = ws["this"].ask(f"time {n_img}")
                ip[n_img] = r["median_ms"]
                emit(net=net, rows=rows, tree="this", run=f"adapter n_img={n_img}", **r)
                r = ws["this"].ask("time 0")
                plain["this"].append(r["median_ms"])
                sha["this"].add(r["eps_sha1"])
                emit(net=net, rows=rows, tree="this", run="no adapter", pair=f"after n_img={n_img}", **r)
            prof = {}
            for k, n_img in (("other", 0), ("this", 0), ("this", 4), ("this", 16)):
                r = ws[k].ask(f"profile {n_img}")
                prof[(k, n_img)] = r
                emit(net=net, rows=rows, tree=k, run="profile", **r)
            med = {k: statistics.median(v) for k, v in plain.items()}
            emit(summary=True, net=net, rows=rows, this_no_adapter_ms=plain["this"], other_no_adapter_ms=plain["other"],
                 this_median_ms=round(med["this"], 4), other_median_ms=round(med["other"], 4),
                 this_vs_other_pct=round(100 * (med["this"] / med["other"] - 1), 3),
                 noise_pct={k: round(100 * (max(v) - min(v)) / med[k], 3) for k, v in plain.items()},
                 no_adapter_bits_equal=bool(len(sha["this"] | sha["other"]) == 1),
                 adapter_ms={str(n): v for n, v in ip.items()},
                 adapter_cost_pct={str(n): round(100 * (v / med["this"] - 1), 3) for n, v in ip.items()},
                 cross_attn_us={f"{k} n_img={n}": r["cross_attn_median_us"] for (k, n), r in prof.items()},
                 cross_attn_ops={f"{k} n_img={n}": r["cross_attn_ops"] for (k, n), r in prof.items()},
                 launches={f"{k} n_img={n}": r["launches"] for (k, n), r in prof.items()})
        finally:
            for w in ws.values():
                w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="a second checkout with its own built library (the commit before the feature)")
    ap.add_argument("--nets", default="sd15:16,sdxl:4")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree")
    ap.add_argument("--net")
    ap.add_argument("--rows", type=int)
    a = ap.parse_args()
    if a.worker:
        worker(a.tree, a.net, a.rows, a.rounds, a.per)
    elif not a.other:
        ap.error("--other TREE is required")
    else:
        driver(a)


if __name__ == "__main__":
    main()
