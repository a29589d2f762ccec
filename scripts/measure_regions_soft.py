"""What soft regional prompts cost a UNet forward: the soft regional cross-attention (cfgpp_op_attention_region_soft, kernel 9) with a
one-hot map of R vertical stripes and with a fully mixed map, against the hard region map on the same engine (kernels 7 / 8), against
the plain 77-token forward, and - the cross-attention launches alone - against R plain 77-key launches.

    python scripts/measure_regions_soft.py [--nets sd15:16,sdxl:4] [--pairs 4] [--rounds 5] [--per 10] [--out FILE.jsonl]

First the launches alone (one worker process, LAUNCH_SHAPES below): per shape and R the soft kernel with the one-hot stripes and with
a mixed map, the hard launch and R plain `cfgpp_op_attention` launches over 77 keys, alternating, one "launch" summary line each.
Then, per net one worker process with ONE engine at max_tokens = 308 and region weights enabled (synthetic weights, tiles tuned by itself;
SD1.5 at a 64 x 64 latent, SDXL at 128 x 128).  For R = 2, 3, 4, `--pairs` times the states (plain, hard, soft one-hot, soft mixed),
order alternating: `--rounds` x `--per` back-to-back forwards timed with device events (the spread between equal runs of one state is
the noise of the box), and three `cfgpp_unet_profile` passes per state for the summed time of the cross-attention launches.  One JSON
line per run, then one "summary" line per (net, R).  A worker that fails ends the measurement.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATES = ("plain", "hard", "soft_onehot", "soft_mixed")


# (rows, heads, d, queries): SD1.5 at 16 rows (d = 40 / 80 / 160 at 64^2 / 32^2 / 16^2), SDXL at 4 rows (d = 64 at 64^2 and 32^2)
LAUNCH_SHAPES = (("sd15", 16, 8, 40, 4096), ("sd15", 16, 8, 80, 1024), ("sd15", 16, 8, 160, 256), ("sdxl", 4, 10, 64, 4096), ("sdxl", 4, 20, 64, 1024))
LAUNCH_STATES = ("soft_onehot", "soft_mixed", "hard", "R_plain")


# ------------------------------------------------------------------------------------------------ worker (the launches alone)
def launch_worker(pairs, rounds, per):
    """per shape and R: the soft kernel with a one-hot map of R vertical stripes and with a fully mixed map, the hard launch
    (kernel 7 / 8) with the same stripes, and R plain 77-key launches of cfgpp_op_attention - same buffers, same process,
    alternating order, `pairs` runs of `rounds` x `per` back-to-back launches between device events"""
    sys.path.insert(0, HERE)
    import torch
    from cfgpp_amd import _lib
    lib = _lib.load()
    dev, st = "cuda", lambda: torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(0)

    def say(**kw):
        print("RESULT " + json.dumps(dict(kind="launch", **kw)), flush=True)

    say(ready=True, build=_lib.build_id(), device=torch.cuda.get_device_name(0))
    for net, B, h, d, nq in LAUNCH_SHAPES:
        dp, BH, kp, side = (d + 31) // 32 * 32, B * h, 320, int(nq ** 0.5)
        q = torch.zeros((BH, nq, dp), dtype=torch.float16)
        k = torch.zeros((BH, kp, dp), dtype=torch.float16)
        q[:, :, :d] = torch.randn((BH, nq, d), generator=g).half()
        k[:, :, :d] = torch.randn((BH, kp, d), generator=g).half()
        vt = torch.zeros((BH, dp, kp), dtype=torch.float16)
        vt[:, :d] = torch.randn((BH, d, kp), generator=g).half()
        q, k, vt = q.to(dev), k.to(dev), vt.to(dev)
        _lib.check(lib.cfgpp_op_attention_prepare_vt(vt.data_ptr(), BH, d, kp, st()), "prepare_vt")
        o = torch.empty((B, nq, h * d), dtype=torch.float16, device=dev)
        for R in (2, 3, 4):
            x = torch.arange(side)[None, :].expand(side, side)
            ids = (x * R // side).clamp(max=R - 1).reshape(1, nq)
            w1 = torch.nn.functional.one_hot(ids, R).permute(0, 2, 1).float().contiguous().to(dev)
            wm = torch.rand((1, R, nq), generator=g) + 0.05
            wm = (wm / wm.sum(1, keepdim=True)).contiguous().to(dev)
            ids8 = ids.to(torch.uint8).contiguous().to(dev)

            def call(tag):
                if tag == "soft_onehot" or tag == "soft_mixed":
                    ww = w1 if tag == "soft_onehot" else wm
                    return lib.cfgpp_op_attention_region_soft(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), B, h, d, nq, R, ww.data_ptr(), 1, nq, kp, st())
                if tag == "hard":
                    return lib.cfgpp_op_attention_region(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), B, h, d, nq, R, ids8.data_ptr(), 1, nq, kp, st())
                rc = 0
                for _ in range(R):
                    rc |= lib.cfgpp_op_attention(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), B, h, d, nq, 77, nq, kp, st())
                return rc

            res = {s: [] for s in LAUNCH_STATES}
            for i in range(pairs):
                for tag in (LAUNCH_STATES if i % 2 == 0 else LAUNCH_STATES[::-1]):
                    for _ in range(3):
                        _lib.check(call(tag), tag)
                    torch.cuda.synchronize()
                    us = []
                    for _ in range(rounds):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(per):
                            call(tag)
                        e1.record()
                        torch.cuda.synchronize()
                        us.append(1000.0 * e0.elapsed_time(e1) / per)
                    res[tag].append(statistics.median(us))
            med = {s: statistics.median(v) for s, v in res.items()}
            say(summary=True, net=net, rows=B, heads=h, d=d, nq=nq, R=R, us={s: round(v, 2) for s, v in med.items()},
                runs_us={s: [round(x, 2) for x in v] for s, v in res.items()},
                spread_pct={s: round(100 * (max(v) - min(v)) / med[s], 2) for s, v in res.items()},
                soft_onehot_vs_R_plain=round(med["soft_onehot"] / med["R_plain"], 3), soft_mixed_vs_R_plain=round(med["soft_mixed"] / med["R_plain"], 3),
                soft_onehot_vs_hard=round(med["soft_onehot"] / med["hard"], 3))


# ------------------------------------------------------------------------------------------------ worker (one net)
def worker(net, rows, pairs, rounds, per):
    sys.path.insert(0, HERE)
    os.environ["CFGPP_TUNE_CACHE"] = "0"            # the engine tunes its own tiles, here
    import torch
    import torch.nn.functional as F
    from cfgpp_amd import _lib
    from cfgpp_amd.hip_engine import HipEngine
    B = rows // 2
    eng = HipEngine(net, max_batch=B, max_tokens=308, soft_regions=True)
    cfg = eng.cfg
    g = torch.Generator().manual_seed(0)
    uc = (torch.randn(1, 308, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
    c = (torch.randn(B, 308, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
    te = ti = None
    if cfg.addition_embed:
        te = (torch.randn(rows, cfg.addition_pooled_dim, generator=g) * 0.5).half()
        ti = torch.tensor([[1024., 1024, 0, 0, 1024, 1024]] * rows)
    z = torch.randn(B, 4, eng.H, eng.W, generator=g).cuda()

    def state(tag, R):
        tokens = 77 if tag == "plain" else 77 * R
        eng.set_context(uc[:, :tokens].contiguous(), c[:, :tokens].contiguous(), te, ti)
        x = torch.arange(eng.W)[None, :].expand(eng.H, eng.W)
        stripes = (x * R // eng.W).clamp(max=R - 1)[None]
        if tag == "plain":
            eng.set_regions(None)
        elif tag == "hard":
            eng.set_regions(stripes, R)
        elif tag == "soft_onehot":
            eng.set_region_weights(F.one_hot(stripes, R).permute(0, 3, 1, 2).float())
        else:
            w = torch.rand((1, R, eng.H, eng.W), generator=g) + 0.05
            eng.set_region_weights(w / w.sum(1, keepdim=True))

    state("plain", 1)
    for _ in range(40):                              # the in-situ tile tuning runs inside the first forwards
        eng.predict(z, 500.0)
    torch.cuda.synchronize()

    def say(**kw):
        print("RESULT " + json.dumps(dict(net=net, rows=rows, **kw)), flush=True)

    def run(tag, R, pair):
        state(tag, R)
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
        cross_us, per_shape, launches = [], {}, 0
        for _ in range(3):
            pr = eng.unet.profile(z, 500.0, detail=True)
            lines = [ln.split("\t") for ln in pr["detail"].strip().split("\n")]
            launches = sum(v["launches"] for k, v in pr.items() if k != "detail")
            rows_ = [r for r in lines if r[2].startswith("cross_attn ")]
            cross_us.append(sum(float(r[3]) for r in rows_))
            for r in rows_:                          # per shape ("heads=.. N=.. d=.."): the mean launch of that shape
                key = " ".join(r[2].split()[1:4])
                per_shape.setdefault(key, []).append(float(r[3]))
        out = dict(state=tag, R=R, pair=pair, ms_per_forward=[round(x, 4) for x in ms], median_ms=round(statistics.median(ms), 4),
                   cross_attn_us=round(statistics.median(cross_us), 1), launches=launches,
                   launch_us={k: round(statistics.mean(v), 2) for k, v in per_shape.items()})
        say(**out)
        return out

    say(ready=True, build=_lib.build_id(), device=torch.cuda.get_device_name(0), latent=[eng.H, eng.W])
    for R in (2, 3, 4):
        res = {s: [] for s in STATES}
        for i in range(pairs):
            for tag in (STATES if i % 2 == 0 else STATES[::-1]):
                res[tag].append(run(tag, R, i))
        med = {k: statistics.median(r["median_ms"] for r in v) for k, v in res.items()}
        cross = {k: statistics.median(r["cross_attn_us"] for r in v) for k, v in res.items()}
        shapes = res["plain"][0]["launch_us"].keys()
        say(summary=True, R=R, median_ms={k: round(v, 4) for k, v in med.items()},
            runs_ms={k: [r["median_ms"] for r in v] for k, v in res.items()},
            noise_pct={k: round(100 * (max(r["median_ms"] for r in v) - min(r["median_ms"] for r in v)) / med[k], 3) for k, v in res.items()},
            vs_plain_pct={k: round(100 * (med[k] / med["plain"] - 1), 3) for k in STATES[1:]},
            soft_onehot_vs_hard_pct=round(100 * (med["soft_onehot"] / med["hard"] - 1), 3),
            cross_attn_us={k: round(v, 1) for k, v in cross.items()},
            cross_attn_R_plain_launches_us=round(R * cross["plain"], 1),
            launch_us={s: {k: round(statistics.median(r["launch_us"][k] for r in res[s]), 2) for k in shapes} for s in STATES},
            launches={k: v[0]["launches"] for k, v in res.items()})
    eng.set_regions(None)


# ------------------------------------------------------------------------------------------------ driver
def driver(a):
    out = open(a.out, "w") if a.out else None
    if not a.skip_launches:
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--launch-worker", "--pairs", str(a.pairs), "--rounds", str(a.rounds),
                              "--per", str(a.launch_per)], stdout=subprocess.PIPE, text=True, cwd=HERE)
        done = 0
        for line in p.stdout:
            if line.startswith("RESULT "):
                print(line[7:], end="", flush=True)
                if out:
                    out.write(line[7:])
                    out.flush()
                done += '"summary": true' in line
        if p.wait() != 0 or done != 3 * len(LAUNCH_SHAPES):
            raise SystemExit(f"measure_regions_soft: the launch worker ended without its {3 * len(LAUNCH_SHAPES)} summaries (exit status {p.returncode})")
    for spec in [s for s in a.nets.split(",") if s]:
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
            raise SystemExit(f"measure_regions_soft: the {net} worker ended without its three summaries (exit status {p.returncode})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="sd15:16,sdxl:4")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--launch_per", type=int, default=20, help="back-to-back launches per timed round of the per-launch part")
    ap.add_argument("--skip_launches", action="store_true", help="the per-forward part only")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--launch-worker", action="store_true")
    ap.add_argument("--net")
    ap.add_argument("--rows", type=int)
    a = ap.parse_args()
    if a.launch_worker:
        launch_worker(a.pairs, a.rounds, a.per)
    elif a.worker:
        worker(a.net, a.rows, a.pairs, a.rounds, a.per)
    else:
        driver(a)


if __name__ == "__main__":
    main()
