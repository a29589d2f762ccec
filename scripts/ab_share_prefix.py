"""In-process A/B of the shared CFG prefix (cfgpp_unet_set_share_prefix): two engines of the same net, one only ever run with the
switch on, the other only with it off (each tunes its own tiles), timed in interleaved rounds of back-to-back forwards.
    python scripts/ab_share_prefix.py sd15 16 [rounds] [forwards per round]"""
import json, os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from cfgpp_amd.hip_engine import HipEngine
from cfgpp_amd import engine as E
name = sys.argv[1] if len(sys.argv) > 1 else "sd15"
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 16
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
per = int(sys.argv[4]) if len(sys.argv) > 4 else 20
os.environ["CFGPP_TUNE_CACHE"] = "0"        # every engine tunes for itself, in its own mode
B = rows // 2
engs = {}
for on in (1, 0):
    E.set_share_prefix(bool(on))
    eng = HipEngine(name, max_batch=B)
    cfg = eng.cfg
    g = torch.Generator().manual_seed(0)
    uc = (torch.randn(1, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
    c = (torch.randn(B, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().cuda()
    eng.set_context(uc, c)
    z = torch.randn(B, 4, eng.H, eng.W, generator=g).cuda()
    for _ in range(3): eng.predict(z, 500.0)
    torch.cuda.synchronize()
    engs[on] = (eng, z)
ms = {1: [], 0: []}
for r in range(rounds):
    for on in ((1, 0) if r % 2 == 0 else (0, 1)):
        E.set_share_prefix(bool(on))
        eng, z = engs[on]
        eng.predict(z, 500.0); torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per): eng.predict(z, 500.0)
        e1.record(); torch.cuda.synchronize()
        ms[on].append(e0.elapsed_time(e1) / per)
E.set_share_prefix(True); a = torch.cat(engs[1][0].predict(engs[1][1], 500.0)).float()
E.set_share_prefix(False); b = torch.cat(engs[0][0].predict(engs[0][1], 500.0)).float()
E.set_share_prefix(True)
print(json.dumps({"net": name, "rows": rows, "rounds": rounds, "forwards_per_round": per,
                  "shared_ms_per_forward": [round(x, 4) for x in ms[1]], "unshared_ms_per_forward": [round(x, 4) for x in ms[0]],
                  "shared_median": round(statistics.median(ms[1]), 4), "unshared_median": round(statistics.median(ms[0]), 4),
                  "gain_pct_of_unshared": round(100 * (1 - statistics.median(ms[1]) / statistics.median(ms[0])), 2),
                  "bit_equal": bool(torch.equal(a, b)), "rel_l2_shared_vs_unshared": float((a - b).norm() / b.norm()),
                  "shared_prefix_ops": engs[1][0].unet.shared_prefix_ops(rows, B)}))
