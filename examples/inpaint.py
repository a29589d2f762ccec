"""Inpainting from the command line on the MI355X path: repaint the white region of a mask image, keep the rest
(``ddim_inpaint`` / ``ddim_inpaint_cfg++``, cfgpp_amd/inpaint.py).

    python examples/inpaint.py --img_path cat.jpg --mask_path mask.png --prompt "a photo of a dog" \
        --method ddim_inpaint_cfg++ --cfg_guidance 0.6 --NFE 50 [--strength 1.0] [--model sd15|sdxl] \
        [--model_dir <diffusers checkpoint>] [--unet_weights ... --vae_weights ...]

The flags of examples/inversion.py plus ``--mask_path`` (white = repaint; binarized at 0.5) and ``--strength``.  A checkpoint
whose ``unet/config.json`` says ``"in_channels": 9`` (SD1.5 / SDXL inpainting) runs as an inpaint UNet; any other UNet takes
the masked update.  ``--inpaint_unet`` selects the 9-channel architecture for synthetic weights.
"""
from __future__ import annotations

import argparse
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from inversion import REFERENCE_FLAGS as _INV_FLAGS, load_img  # noqa: E402

REFERENCE_FLAGS = tuple((f, k, Path("examples/workdir/inpaint") if f == "workdir" else d) for f, k, d in _INV_FLAGS
                        if f != "method") + (("method", str, "ddim_inpaint_cfg++"),)
EXTRA_FLAGS = (("unet_weights", str, "synthetic"), ("vae_weights", str, None), ("model_dir", str, None),
               ("mask_path", Path, None), ("strength", float, 1.0))


def load_mask(mask_path, size: int) -> torch.Tensor:
    """grey-scale mask image -> [1,1,size,size] float in [0, 1] (1 = repaint)"""
    from PIL import Image
    arr = np.asarray(Image.open(mask_path).convert("L").resize((size, size), Image.NEAREST), dtype=np.float32)
    return (torch.from_numpy(arr) / 255.0)[None, None]


def main(argv=None, solver_kwargs=None) -> None:
    """``solver_kwargs`` lets tests inject ``engine=`` / ``vae=`` (CPU mock); the CLI never passes it."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for flag, kind, default in REFERENCE_FLAGS + EXTRA_FLAGS:
        ap.add_argument(f"--{flag}", type=kind, default=default)
    ap.add_argument("--model", default="sd15", choices=("sd15", "sdxl"))
    ap.add_argument("--max_prompt_chunks", type=int, default=1, choices=(1, 2, 3, 4),
                    help="2 .. 4: prompts of up to 75 ids per chunk with (emphasis:1.3) / [de-emphasis] / BREAK, the engine built for "
                         "77 x K text tokens (cfgpp_amd/prompt.py); 1 (default): prompts cut at 75 ids, brackets literal")
    ap.add_argument("--lora", action="append", default=[], metavar="PATH[:SCALE]",
                    help="LoRA safetensors file merged into the UNet on the device (repeatable; scale defaults to 1)")
    ap.add_argument("--inpaint_unet", action="store_true", help="synthetic 9-channel inpaint UNet instead of the 4-channel one")
    from cfgpp_amd.freeu import add_cli_flag, cli_kwargs
    add_cli_flag(ap)
    from cfgpp_amd import vpred
    vpred.add_cli_flags(ap)      # --prediction_type / --zero_terminal_snr / --timestep_spacing / --guidance_rescale
    args = ap.parse_args(argv)
    if args.mask_path is None:
        ap.error("--mask_path is required")

    from cfgpp_amd.callback_util import save_image
    from cfgpp_amd.inpaint import get_inpaint_solver
    from cfgpp_amd.unet_config import SD15_INPAINT, SDXL_INPAINT
    (args.workdir / "result").mkdir(parents=True, exist_ok=True)
    torch.manual_seed(args.seed)
    xl = args.model == "sdxl"
    size = args.img_size if not xl or args.img_size != 512 else 1024
    img = load_img(args.img_path, size)
    mask = load_mask(args.mask_path, size)
    kw = dict(solver_config=types.SimpleNamespace(num_sampling=args.NFE), device=args.device, max_batch=1,
              unet_weights=args.unet_weights, latent_hw=(size // 8, size // 8))
    if args.inpaint_unet:
        kw["unet_config"] = SDXL_INPAINT if xl else SD15_INPAINT
    if args.vae_weights:
        kw["vae_weights"] = args.vae_weights
    if args.model_dir:        # a local diffusers-layout checkpoint: UNet (9 input channels -> inpaint UNet) / VAE / CLIP tower(s)
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
        kw["lora"] = parse_cli(args.lora)          # replaces a LoRA file --model_dir found next to the model
        kw.pop("lora_ignore_text_encoder", None)
    cli_kwargs(args, kw)
    vpred.cli_kwargs(args, kw)        # explicit flags win over the checkpoint's files
    if args.max_prompt_chunks > 1:
        kw["max_prompt_chunks"] = args.max_prompt_chunks
    kw.update(solver_kwargs or {})
    solver = get_inpaint_solver(args.method, model=args.model, **kw)
    common = dict(src_img=img, mask=mask, strength=args.strength, cfg_guidance=args.cfg_guidance, seeds=[args.seed], callback_fn=None)
    if xl:
        result = solver.sample(prompt1=[args.null_prompt, args.prompt], prompt2=[args.null_prompt, args.prompt],
                               target_size=(size, size), original_size=(size, size), **common)
    else:
        result = solver.sample(prompt=[args.null_prompt, args.prompt], **common)
    save_image(result, args.workdir / "result" / "inpaint.png", normalize=True)
    print(f"saved {args.workdir / 'result' / 'inpaint.png'} ({'9-channel inpaint UNet' if solver.inpaint_unet else 'masked update'})")


if __name__ == "__main__":
    main()
