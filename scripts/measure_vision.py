"""What the CLIP image tower costs on the HIP path, against the same tower in torch-ROCm.

    python scripts/measure_vision.py [--towers vit_h,bigG] [--images 2] [--pairs 3] [--rounds 5] [--per 3] [--out profiles/vision/towers.jsonl]

Per tower one worker process: ViT-H/14 (32 layers, hidden 1280, 16 heads of 80) or ViT-bigG/14 (48 layers, hidden 1664, 16 heads of
104) at full depth, 224 px, 257 tokens, synthetic weights (a `transformers` CLIPVisionModelWithProjection initialised on the device in
fp16; the HIP tower loads ITS state dict, so both sides hold the same values).  Everything is interleaved on one device in one call:

  * `--pairs` times (hip, torch), order alternating: `--rounds` x `--per` back-to-back encodes of `--images` preprocessed images
    (hidden_states[-2] requested, what a "plus" adapter reads), timed with device events; the spread between equal runs of one side is
    the noise of the box;
  * the attention launches' share: `layers` cfgpp_op_attention_vit launches at the job's shape, timed the same way, over the HIP encode;
  * the front end alone (cfgpp_vision_preprocess of 1000 x 700 pictures), device bytes, FLOPs, and the rel-L2 between the two sides.

One JSON line per run, then one "summary" line per tower.  A worker that fails ends the measurement.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOWERS = dict(vit_h=dict(hidden=1280, layers=32, heads=16, inter=5120, proj=1024), bigG=dict(hidden=1664, layers=48, heads=16, inter=8192, proj=1280))


def worker(name, images, pairs, rounds, per):
    sys.path.insert(0, HERE)
    import torch
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from cfgpp_amd import _lib
    from cfgpp_amd.ip_adapter import ImageEncoder
    from cfgpp_amd.vision import HipClipImageTower
    g = TOWERS[name]
    cfg = CLIPVisionConfig(hidden_size=g["hidden"], intermediate_size=g["inter"], num_hidden_layers=g["layers"], num_attention_heads=g["heads"],
                           image_size=224, patch_size=14, projection_dim=g["proj"], hidden_act="gelu")
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = CLIPVisionModelWithProjection(cfg).half().eval()
    enc = ImageEncoder.__new__(ImageEncoder)                # the torch tower without a folder: the same class, the same call
    enc.model, enc.device = model, "cuda"
    tower = HipClipImageTower(g["hidden"], g["layers"], g["heads"], g["inter"], "gelu", g["proj"], 224, 14, model.state_dict(), max_batch=images)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(1)
    img = torch.rand((images, 3, 1000, 700), generator=gen).cuda()
    pix = tower.preprocess(img)

    def say(**kw):
        print("RESULT " + json.dumps(dict(tower=name, images=images, **kw)), flush=True)

    def timed(fn):
        ms = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / per)
        return ms

    sides = dict(hip=lambda: tower.encode_pixels(pix, hidden=True), torch=lambda: enc.encode_pixels(pix, hidden=True))
    a, b = sides["hip"]().float(), sides["torch"]().float()
    say(ready=True, build=_lib.build_id(), device=torch.cuda.get_device_name(0), geometry=g, tokens=tower.tokens,
        device_bytes=tower.device_bytes(), gflop=round(1e-9 * tower.flops(images), 1), hip_vs_torch_rel_l2=float((a - b).norm() / b.norm()))
    res = {"hip": [], "torch": []}
    for i in range(pairs):
        for tag in (("hip", "torch") if i % 2 == 0 else ("torch", "hip")):
            for _ in range(2):
                sides[tag]()
            torch.cuda.synchronize()
            ms = timed(sides[tag])
            res[tag].append(statistics.median(ms))
            say(side=tag, pair=i, ms_per_encode=[round(x, 3) for x in ms], median_ms=round(statistics.median(ms), 3))
    d = g["hidden"] // g["heads"]
    qkv = torch.randn((images, tower.tokens, 3 * g["hidden"]), generator=torch.Generator().manual_seed(2)).half().cuda()
    o = torch.empty((images, tower.tokens, g["hidden"]), dtype=torch.float16, device="cuda")

    def attn():
        for _ in range(g["layers"]):
            _lib.check(lib.cfgpp_op_attention_vit(qkv.data_ptr(), o.data_ptr(), images, g["heads"], d, tower.tokens, stream), "cfgpp_op_attention_vit")
    attn()
    attn_ms = statistics.median(timed(attn))
    pre_ms = statistics.median(timed(lambda: tower.preprocess(img)))
    med = {k: statistics.median(v) for k, v in res.items()}
    say(summary=True, hip_ms=[round(x, 3) for x in res["hip"]], torch_ms=[round(x, 3) for x in res["torch"]], hip_median_ms=round(med["hip"], 3),
        torch_median_ms=round(med["torch"], 3), hip_over_torch=round(med["hip"] / med["torch"], 3),
        noise_pct={k: round(100 * (max(v) - min(v)) / med[k], 2) for k, v in res.items()},
        attention_ms=round(attn_ms, 3), attention_share_pct=round(100 * attn_ms / med["hip"], 1), attention_us_per_launch=round(1e3 * attn_ms / g["layers"], 1),
        preprocess_1000x700_ms=round(pre_ms, 3), gflop=round(1e-9 * tower.flops(images), 1), hip_tflops=round(1e-9 * tower.flops(images) / med["hip"], 1),
        device_gbytes=round(tower.device_bytes() / 1e9, 3))


def driver(a):
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "w")
    for name in a.towers.split(","):
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tower", name, "--images", str(a.images), "--pairs", str(a.pairs),
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
            raise SystemExit(f"measure_vision: the {name} worker ended without a summary (exit status {p.returncode})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--towers", default="vit_h,bigG")
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tower")
    a = ap.parse_args()
    if a.worker:
        worker(a.tower, a.images, a.pairs, a.rounds, a.per)
    else:
        driver(a)


if __name__ == "__main__":
    main()
