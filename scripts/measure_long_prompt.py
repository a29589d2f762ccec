"""What long prompts cost, and whether xattn64_long_kernel earns its place (the tables of profiles/long_prompt/).

    python scripts/measure_long_prompt.py launch  [--out FILE.jsonl] [--reps 7] [--per 1500]
    python scripts/measure_long_prompt.py forward [--out FILE.jsonl] [--nets sd15:8,sdxl:2] [--rounds 5] [--per 5]

launch   per-launch A/B of cfgpp_op_attention_cross on the UNets' cross-attention shapes (SD1.5 64 x 64: d = 40, Nq 4096, B * heads
         128; SDXL: d = 64, Nq 4096 x 40 and Nq 1024 x 80) at 154 / 231 / 308 keys: cfgpp_attention_set_cross_long(2) - the
         resident-K/V kernel over its whole scope - against (0) - the flash loop, what cfgpp_op_attention runs at these key counts - in ONE process on one
         device, the two interleaved `--reps` times, `--per` back-to-back launches per timing between two device events.  The
         outputs of the two paths are compared (max |a - b|: both are fp16 roundings of the same softmax).
forward  one engine per net, built for 308 tokens: forwards at 77 / 154 / 231 / 308 tokens, interleaved `--rounds` times (device
         events around `--per` forwards), then the family sums of cfgpp_unet_profile (three passes, median) and the summed time of
         the cross-attention launches.

One JSON line per measurement, a "table" line per shape / net at the end.  No GPU: the script fails.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))

SHAPES = [("sd15 64x64", 40, 4096, 128), ("sdxl 64x64", 64, 4096, 40), ("sdxl 32x32", 64, 1024, 80)]
KEYS = (154, 231, 308)


def emitter(path):
    out = open(path, "w") if path else None

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    return emit


def launch(a):
    import torch
    import hip_ops as H
    from cfgpp_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("measure_long_prompt: needs the GPU")
    emit = emitter(a.out)
    lib = H.lib()
    emit(build=_lib.build_id(), device=torch.cuda.get_device_name(0), reps=a.reps, per=a.per)
    g = torch.Generator().manual_seed(0)
    for name, d, nq, bh in SHAPES:
        dp = 64
        hq = torch.zeros((bh, nq, dp), dtype=torch.float16, device=H.DEV)
        hq[:, :, :d] = torch.randn((bh, nq, d), generator=g).half().to(H.DEV)
        o = torch.empty((1, nq, bh * d), dtype=torch.float16, device=H.DEV)
        for nk in KEYS:
            kp = 320
            hk = torch.zeros((bh, kp, dp), dtype=torch.float16, device=H.DEV)
            hvt = torch.zeros((bh, dp, kp), dtype=torch.float16, device=H.DEV)
            hk[:, :nk, :d] = torch.randn((bh, nk, d), generator=g).half().to(H.DEV)
            hvt[:, :d, H.vt_pos(kp)[:nk].to(H.DEV)] = torch.randn((bh, d, nk), generator=g).half().to(H.DEV)
            H.check(lib.cfgpp_op_attention_prepare_vt(H.P(hvt), bh, d, kp, H.stream()), "prepare_vt")

            def run(mode, n):
                lib.cfgpp_attention_set_cross_long(mode)
                for _ in range(n):
                    H.check(lib.cfgpp_op_attention_cross(H.P(hq), H.P(hk), H.P(hvt), H.P(o), 1, bh, d, nq, nk, nq, kp, H.stream()), "attention_cross")
                return H.attention_last_launch()

            outs, rec = {}, {}
            default = run(1, 1)[0]                      # what the shipped dispatch takes at this shape
            for mode in (2, 0):                         # warm both, keep their outputs
                rec[mode] = run(mode, 10)
                torch.cuda.synchronize()
                outs[mode] = o.clone()
            for mode in (2, 0):                         # an unrecorded window each: clocks and caches in the state the timed ones see
                run(mode, max(1, a.per // 4))
            torch.cuda.synchronize()
            us = {2: [], 0: []}
            for r in range(a.reps):
                for mode in ((2, 0) if r % 2 == 0 else (0, 2)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(mode, a.per)
                    e1.record()
                    torch.cuda.synchronize()
                    us[mode].append(1e3 * e0.elapsed_time(e1) / a.per)
            lib.cfgpp_attention_set_cross_long(1)
            med = {m: statistics.median(v) for m, v in us.items()}
            flops = 4.0 * bh * nq * nk * d
            emit(table="launch", shape=name, d=d, nq=nq, bh=bh, nk=nk, record_long=rec[2], record_flash=rec[0], default_kernel=default,
                 long_us=[round(x, 2) for x in us[2]], flash_us=[round(x, 2) for x in us[0]],
                 long_median_us=round(med[2], 2), flash_median_us=round(med[0], 2),
                 long_vs_flash_pct=round(100 * (med[2] / med[0] - 1), 2),
                 spread_pct={"long": round(100 * (max(us[2]) - min(us[2])) / med[2], 2), "flash": round(100 * (max(us[0]) - min(us[0])) / med[0], 2)},
                 long_tflops=round(flops / med[2] * 1e-6, 1), flash_tflops=round(flops / med[0] * 1e-6, 1),
                 max_abs_diff=float((outs[2].float() - outs[0].float()).abs().max()))


def forward(a):
    import torch
    from cfgpp_amd import _lib
    from cfgpp_amd.hip_engine import HipEngine
    if not torch.cuda.is_available():
        raise SystemExit("measure_long_prompt: needs the GPU")
    os.environ["CFGPP_TUNE_CACHE"] = "0"
    emit = emitter(a.out)
    emit(build=_lib.build_id(), device=torch.cuda.get_device_name(0), rounds=a.rounds, per=a.per)
    for spec in a.nets.split(","):
        net, B = spec.split(":")
        B = int(B)
        eng = HipEngine(net, max_batch=B, max_tokens=308)
        cfg = eng.cfg
        g = torch.Generator().manual_seed(0)
        full_uc = (torch.randn(1, 308, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
        full_c = (torch.randn(B, 308, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
        te = ti = None
        if cfg.addition_embed:
            te = (torch.randn(2 * B, cfg.addition_pooled_dim, generator=g) * 0.5).half()
            ti = torch.tensor([[1024., 1024, 0, 0, 1024, 1024]] * (2 * B))
        z = torch.randn(B, 4, eng.H, eng.W, generator=g).cuda()

        def ctx(tokens):
            eng.set_context(full_uc[:, :tokens].contiguous(), full_c[:, :tokens].contiguous(), te, ti)

        ctx(77)
        for _ in range(30):                             # the in-situ tile tuning runs inside the first forwards
            eng.predict(z, 500.0)
        torch.cuda.synchronize()
        ms = {t: [] for t in (77,) + KEYS}
        for r in range(a.rounds):
            order = list(ms) if r % 2 == 0 else list(ms)[::-1]
            for tokens in order:
                ctx(tokens)
                for _ in range(2):
                    eng.predict(z, 500.0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.per):
                    eng.predict(z, 500.0)
                e1.record()
                torch.cuda.synchronize()
                ms[tokens].append(e0.elapsed_time(e1) / a.per)
        prof = {}
        for tokens in ms:
            ctx(tokens)
            fam, cross = [], []
            for _ in range(3):
                pr = eng.unet.profile(z, 500.0, detail=True)
                rows_ = [ln.split("\t") for ln in pr["detail"].strip().split("\n")]
                cross.append(sum(float(r[3]) for r in rows_ if r[2].startswith("cross_attn")) / 1e3)
                fam.append({k: v["ms"] for k, v in pr.items() if k != "detail"})
            prof[tokens] = dict(cross_attn_ms=round(statistics.median(cross), 4),
                                family_ms={k: round(statistics.median(f[k] for f in fam), 4) for k in fam[0]},
                                gflop=round(eng.flops_per_forward(2 * B) * 1e-9, 1))
        med = {t: statistics.median(v) for t, v in ms.items()}
        emit(table="forward", net=net, batch=B, rows=2 * B, latent=[eng.H, eng.W],
             ms_per_forward={str(t): [round(x, 4) for x in v] for t, v in ms.items()},
             median_ms={str(t): round(m, 4) for t, m in med.items()},
             vs_77_pct={str(t): round(100 * (m / med[77] - 1), 2) for t, m in med.items()},
             spread_pct={str(t): round(100 * (max(v) - min(v)) / med[t], 2) for t, v in ms.items()},
             profile={str(t): p for t, p in prof.items()})
        del eng
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("launch", "forward"))
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--per", type=int, default=1500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--nets", default="sd15:8,sdxl:2")
    a = ap.parse_args()
    if a.what == "forward" and a.per == 1500:
        a.per = 5
    (launch if a.what == "launch" else forward)(a)


if __name__ == "__main__":
    main()
