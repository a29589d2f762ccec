"""Panoramas from the command line on the MI355X path: an image larger than the UNet's window by MultiDiffusion
(``ddim_panorama`` / ``ddim_panorama_cfg++``, cfgpp_amd/panorama.py).

    python examples/panorama.py --prompt "a photo of the dolomites" --method ddim_panorama_cfg++ --cfg_guidance 0.6 --NFE 50 \
        --panorama_size 512x2048 [--stride 8] [--circular_padding] [--view_batch_size 5] [--model sd15|sdxl] \
        [--model_dir <diffusers checkpoint>] [--unet_weights ... --vae_weights ...] [--batch 2]

The flags of examples/text_to_img.py that apply (no ControlNet, no IP-Adapter: the panorama solvers refuse them) plus
``--panorama_size HxW`` in pixels, ``--stride`` in latent units (8 = 64 pixels, diffusers' default), ``--circular_padding`` (views wrap
around the width: a 360-degree panorama) and ``--view_batch_size`` (views per UNet forward; default: as many as divide the view count
and fit ``--max_rows``).  The window is the model's own size (512 x 512 for SD1.5, 1024 x 1024 for SDXL).
"""
from __future__ import annotations

import argparse
import os
import sys
import types
from pathlib import Path

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from text_to_img import REFERENCE_FLAGS as _T2I_FLAGS  # noqa: E402

_DEFAULTS = {"workdir": Path("examples/workdir/panorama"), "method": "ddim_panorama_cfg++", "cfg_guidance": 0.6}
REFERENCE_FLAGS = tuple((f, k, _DEFAULTS.get(f, d)) for f, k, d in _T2I_FLAGS)
EXTRA_FLAGS = (("unet_weights", str, "synthetic"), ("vae_weights", str, None), ("model_dir", str, None), ("batch", int, 1),
               ("panorama_size", str, None), ("stride", int, 8), ("view_batch_size", int, None), ("max_rows", int, 32))


def parse_size(text: str, what: str = "--panorama_size"):
    """'512x2048' -> (512, 2048) pixels, both multiples of 8"""
    try:
        hh, ww = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise SystemExit(f"{what} {text!r}: expected HxW in pixels, e.g. 512x2048") from None
    if hh % 8 or ww % 8 or hh <= 0 or ww <= 0:
        raise SystemExit(f"{what} {text!r}: both sides must be positive multiples of 8 pixels")
    return hh, ww


def main(argv=None, solver_kwargs=None) -> None:
    """``solver_kwargs`` lets tests inject ``engine=`` / ``vae=`` / ``latent_hw=`` (CPU mock); the CLI never passes it."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for flag, kind, default in REFERENCE_FLAGS + EXTRA_FLAGS:
        ap.add_argument(f"--{flag}", type=kind, default=default)
    ap.add_argument("--model", default="sd15", choices=("sd15", "sdxl"))
    ap.add_argument("--circular_padding", action="store_true", help="views wrap around the panorama's width")
    ap.add_argument("--max_prompt_chunks", type=int, default=1, choices=(1, 2, 3, 4),
                    help="2 .. 4: prompts of up to 75 ids per chunk with (emphasis:1.3) / [de-emphasis] / BREAK, the engine built for "
                         "77 x K text tokens (cfgpp_amd/prompt.py); 1 (default): prompts cut at 75 ids, brackets literal")
    ap.add_argument("--lora", action="append", default=[], metavar="PATH[:SCALE]",
                    help="LoRA safetensors file merged into the UNet on the device (repeatable; scale defaults to 1)")
    ap.add_argument("--draw", action="store_true", help="save z0t / zt decodes of the panorama every step (draw_tweedie + draw_noisy)")
    from cfgpp_amd.freeu import add_cli_flag, cli_kwargs
    add_cli_flag(ap)
    args = ap.parse_args(argv)

    from cfgpp_amd.callback_util import ComposeCallback, save_image
    from cfgpp_amd.panorama import get_panorama_solver
    (args.workdir / "result").mkdir(parents=True, exist_ok=True)
    torch.manual_seed(args.seed)
    xl = args.model == "sdxl"
    size = parse_size(args.panorama_size or ("1024x4096" if xl else "512x2048"))
    callback = ComposeCallback(workdir=args.workdir, frequency=1, callbacks=["draw_noisy", "draw_tweedie"]) if args.draw else None
    kw = dict(solver_config=types.SimpleNamespace(num_sampling=args.NFE), device=args.device, max_batch=args.max_rows,
              unet_weights=args.unet_weights)
    if args.vae_weights:
        kw["vae_weights"] = args.vae_weights
    if args.model_dir:        # a local diffusers-layout checkpoint: UNet / VAE weights, CLIP tower(s) + BPE tokenizer(s)
        from cfgpp_amd.checkpoint import solver_kwargs_from_dir
        found, missing = solver_kwargs_from_dir(args.model_dir, xl, args.device)
        if missing:
            print(f"--model_dir {args.model_dir}: no {', '.join(missing)} there - synthetic stand-in(s) used")
        for k, v in found.items():
            if k.endswith("_weights") and getattr(args, k, None) not in (None, "synthetic"):
                continue                                   # an explicit --unet_weights / --vae_weights wins
            kw[k] = v
    if args.lora:
        from cfgpp_amd.lora import parse_cli
        kw["lora"] = parse_cli(args.lora)
        kw.pop("lora_ignore_text_encoder", None)
    cli_kwargs(args, kw)
    if args.max_prompt_chunks > 1:
        kw["max_prompt_chunks"] = args.max_prompt_chunks
    kw.update(solver_kwargs or {})
    solver = get_panorama_solver(args.method, model=args.model, panorama_hw=(size[0] // 8, size[1] // 8), stride=args.stride,
                                 circular_padding=args.circular_padding, view_batch_size=args.view_batch_size, **kw)
    prompts = [args.prompt] * args.batch if args.batch > 1 else args.prompt
    seeds = None if args.batch == 1 else [args.seed + i for i in range(args.batch)]   # B = 1: global CPU RNG, like text_to_img.py
    result = solver.sample(prompt=[args.null_prompt, prompts], cfg_guidance=args.cfg_guidance, callback_fn=callback, seeds=seeds)
    for i in range(result.shape[0]):
        name = "panorama.png" if result.shape[0] == 1 else f"panorama_{i}.png"
        save_image(result[i:i + 1], args.workdir / "result" / name, normalize=True)
    g = solver.geometry
    print(f"saved {result.shape[0]} panorama(s) of {size[0]} x {size[1]} ({g.n_views} views of {8 * g.h} x {8 * g.w}) to {args.workdir / 'result'}")


if __name__ == "__main__":
    main()
