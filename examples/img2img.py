"""Image-to-image from the command line on the MI355X path: start from a picture, noised to ``--strength`` of the schedule, and denoise
the rest with the prompt (cfgpp_amd/img2img.py: DDIM, Euler, DPM++ 2M and the SDE solvers, CFG and CFG++).

    python examples/img2img.py --src_img cat.png --strength 0.6 --prompt "a watercolour of a cat" --method ddim_cfg++ \
        --cfg_guidance 0.6 --NFE 50 [--model sd15|sdxl] [--img_size 512] [--noise torch|philox] [--batch 4] \
        [--model_dir <diffusers checkpoint>] [--unet_weights ... --vae_weights ...] [--lora PATH[:SCALE]] [--eta 1.0 ...]

The flags and plumbing of examples/text_to_img.py plus ``--src_img`` (resized to ``--img_size``, 1024 for SDXL), ``--strength`` and
``--noise``.  The result goes to <workdir>/result/img2img.png.
"""
from __future__ import annotations

import argparse
import os
import sys
import types
from pathlib import Path

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from inversion import load_img  # noqa: E402
from text_to_img import EXTRA_FLAGS as _T2I_EXTRA, REFERENCE_FLAGS as _T2I_FLAGS  # noqa: E402

REFERENCE_FLAGS = tuple((f, k, Path("examples/workdir/img2img") if f == "workdir" else ("ddim_cfg++" if f == "method" else d))
                        for f, k, d in _T2I_FLAGS)
EXTRA_FLAGS = tuple(t for t in _T2I_EXTRA if t[0] in ("unet_weights", "vae_weights", "model_dir", "batch")) + (
    ("src_img", Path, None), ("strength", float, 0.75), ("img_size", int, None))
SDE_FLAGS = ("eta", "s_noise", "solver_type", "sigma_schedule")


def build_parser(doc, flags):
    ap = argparse.ArgumentParser(description=doc.split("\n")[0])
    for flag, kind, default in flags:
        ap.add_argument(f"--{flag}", type=kind, default=default)
    ap.add_argument("--model", default="sd15", choices=("sd15", "sdxl"))
    ap.add_argument("--noise", default="torch", choices=("torch", "philox"),
                    help="the start's forward noise: host randn (default) or drawn inside the start launch, keyed by the seeds")
    ap.add_argument("--max_prompt_chunks", type=int, default=1, choices=(1, 2, 3, 4),
                    help="2 .. 4: long / weighted prompts (cfgpp_amd/prompt.py); 1 (default): prompts cut at 75 ids")
    ap.add_argument("--lora", action="append", default=[], metavar="PATH[:SCALE]",
                    help="LoRA safetensors file merged into the UNet on the device (repeatable; scale defaults to 1)")
    ap.add_argument("--eta", type=float, default=None, help="--method dpm++_*_sde*: noise level (default 1; 0 = deterministic)")
    ap.add_argument("--s_noise", type=float, default=None, help="--method dpm++_*_sde*: noise multiplier (default 1)")
    ap.add_argument("--solver_type", default=None, choices=("midpoint", "heun"), help="--method dpm++_2m_sde*: second-order form")
    ap.add_argument("--sigma_schedule", default=None, choices=("karras", "exponential"), help="--method dpm++_*_sde*: sigma schedule")
    from cfgpp_amd import vpred
    from cfgpp_amd.freeu import add_cli_flag
    add_cli_flag(ap)
    vpred.add_cli_flags(ap)      # --prediction_type / --zero_terminal_snr / --timestep_spacing / --guidance_rescale
    return ap


def solver_kwargs_of(args, latent_hw, solver_kwargs=None):
    """the get_img2img_solver / get_solver kwargs of the shared flags (examples/text_to_img.py's plumbing)"""
    from cfgpp_amd import vpred
    from cfgpp_amd.freeu import cli_kwargs
    kw = dict(solver_config=types.SimpleNamespace(num_sampling=args.NFE), device=args.device, max_batch=args.batch,
              unet_weights=args.unet_weights, latent_hw=tuple(latent_hw))
    if args.vae_weights:
        kw["vae_weights"] = args.vae_weights
    if args.model_dir:        # a local diffusers-layout checkpoint: UNet / VAE weights, CLIP tower(s) + BPE tokenizer(s)
        from cfgpp_amd.checkpoint import solver_kwargs_from_dir
        found, missing = solver_kwargs_from_dir(args.model_dir, args.model == "sdxl", args.device)
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
    vpred.cli_kwargs(args, kw)        # explicit flags win over the checkpoint's files
    if args.max_prompt_chunks > 1:
        kw["max_prompt_chunks"] = args.max_prompt_chunks
    kw.update(solver_kwargs or {})
    return kw


def sde_kwargs_of(args, method):
    return {k: getattr(args, k) for k in SDE_FLAGS if "sde" in method and getattr(args, k) is not None}


def job_kwargs(args, size):
    """the sample() kwargs every job of these command lines shares: prompts for ``--batch`` chains, seeds seed, seed + 1, ..."""
    prompts = [args.prompt] * args.batch if args.batch > 1 else args.prompt
    kw = dict(prompt=[args.null_prompt, prompts], cfg_guidance=args.cfg_guidance, seeds=[args.seed + i for i in range(args.batch)])
    if args.model == "sdxl":
        kw.update(target_size=(size, size), original_size=(size, size))
    return kw


def save_results(result, folder, stem):
    from cfgpp_amd.callback_util import save_image
    for i in range(result.shape[0]):
        name = f"{stem}.png" if result.shape[0] == 1 else f"{stem}_{i}.png"
        save_image(result[i:i + 1], folder / name, normalize=True)
    print(f"saved {result.shape[0]} image(s) to {folder}")


def main(argv=None, solver_kwargs=None) -> None:
    """``solver_kwargs`` lets tests inject ``engine=`` / ``vae=`` (CPU mock); the CLI never passes it."""
    ap = build_parser(__doc__, REFERENCE_FLAGS + EXTRA_FLAGS)
    args = ap.parse_args(argv)
    if args.src_img is None:
        ap.error("--src_img is required")
    from cfgpp_amd.img2img import get_img2img_solver
    (args.workdir / "result").mkdir(parents=True, exist_ok=True)
    torch.manual_seed(args.seed)
    size = args.img_size or (1024 if args.model == "sdxl" else 512)
    img = load_img(args.src_img, size)
    kw = solver_kwargs_of(args, (size // 8, size // 8), solver_kwargs)
    solver = get_img2img_solver(args.method, model=args.model, noise=args.noise, **sde_kwargs_of(args, args.method), **kw)
    size = 8 * solver.latent_hw[0]
    result = solver.sample(src_img=load_img(args.src_img, size) if size != img.shape[-1] else img, strength=args.strength,
                           **job_kwargs(args, size))
    print(f"ran {solver.last_start['steps']} of {args.NFE} steps from step {solver.last_start['i0']} (strength {args.strength})")
    save_results(result, args.workdir / "result", "img2img")


if __name__ == "__main__":
    main()
