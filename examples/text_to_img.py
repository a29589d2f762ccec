"""Command-line twin of the reference's examples/text_to_img.py (same flags and defaults) on the MI355X path.

    python examples/text_to_img.py --prompt "a corgi" --method ddim_cfg++ --cfg_guidance 0.6 --NFE 50 \
        [--model sd15|sdxl|sdxl_lightning] [--unet_weights unet.safetensors --vae_weights vae.safetensors] \
        [--batch 8] [--draw] [--controlnet_dir <diffusers controlnet/ folder> --control_image edges.png] \
        [--ip_adapter ip-adapter_sd15.safetensors[:SCALE] (--ip_image ref.png --ip_adapter_dir <folder with image_encoder/> | --ip_embeds e.npy)]

Differences from the reference, all additive: ``--unet_weights / --vae_weights`` (diffusers-layout safetensors;
default = seeded synthetic weights, because no checkpoint exists offline), ``--batch`` (B chains with seeds
seed, seed+1, ... in one UNet batch of 2B rows) and ``--draw`` (the reference keeps its ComposeCallback
commented out).  Text goes through ``solver.text_encoder`` (synthetic embeddings unless a CLIP callable is
plugged in, cfgpp_amd/conditioning.py).  Reference behaviour kept: CPU-generator initial latent from
``--seed``, default null prompt, 1024x1024 target for SDXL, result saved (min-max normalised, as torchvision's
``save_image(normalize=True)`` does there) to <workdir>/result/generated.png.
"""
from __future__ import annotations

import argparse
import os
import sys
import types
from pathlib import Path

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# (flag, type, default) - the reference CLI's flags with its defaults, then ours
REFERENCE_FLAGS = (
    ("workdir", Path, Path("examples/workdir/t2i")), ("device", str, "cuda"),
    ("null_prompt", str, "low quality,jpeg artifacts,blurry,poorly drawn,ugly,worst quality,"), ("prompt", str, ""),
    ("cfg_guidance", float, 7.5), ("method", str, "ddim"), ("NFE", int, 50), ("seed", int, 42),
)
EXTRA_FLAGS = (("unet_weights", str, "synthetic"), ("vae_weights", str, None), ("model_dir", str, None), ("batch", int, 1),
               ("controlnet_dir", str, None), ("control_image", str, None), ("controlnet_conditioning_scale", float, 1.0))


def load_control_image(path, size):
    """a PNG / JPEG -> [1, 3, h, w] in [0, 1]: converted to RGB and resized to the target size, no normalisation (diffusers'
    ControlNet image processor: do_convert_rgb=True, do_normalize=False)"""
    from PIL import Image
    import numpy as np
    img = Image.open(path).convert("RGB").resize((size[1], size[0]), Image.BICUBIC)
    return torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1)[None].contiguous()


def main(argv=None, solver_kwargs=None) -> None:
    """``solver_kwargs`` lets tests inject ``engine=`` / ``vae=`` (CPU mock); the CLI never passes it."""
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for flag, kind, default in REFERENCE_FLAGS + EXTRA_FLAGS:
        ap.add_argument(f"--{flag}", type=kind, default=default)
    ap.add_argument("--model", default="sd15", choices=("sd15", "sd20", "sdxl", "sdxl_lightning"))
    ap.add_argument("--max_prompt_chunks", type=int, default=1, choices=(1, 2, 3, 4),
                    help="2 .. 4: prompts of up to 75 ids per chunk with (emphasis:1.3) / [de-emphasis] / BREAK, the engine built for "
                         "77 x K text tokens (cfgpp_amd/prompt.py); 1 (default): prompts cut at 75 ids, brackets literal")
    ap.add_argument("--max_regions", type=int, default=1, choices=(1, 2, 3, 4),
                    help="regional prompts: size the engine for up to this many regions (the prompt is region 0; 1 = off)")
    ap.add_argument("--region", action="append", default=[], metavar="X0,Y0,X1,Y1:PROMPT",
                    help="repeatable: a rectangle as fractions of width and height, and the prompt that applies inside it (later ones win)")
    ap.add_argument("--soft_regions", action="store_true",
                    help="regions blend by per-pixel weights (soft masks, --region_feather, --region_base_ratio) on the soft regional kernel")
    ap.add_argument("--region_feather", type=float, default=0.0, metavar="F",
                    help="--soft_regions: width of the linear ramp on every rectangle edge, as a fraction of the shorter side "
                         "(edges on the image border ramp too: a region touching the border fades to the base prompt there)")
    ap.add_argument("--region_base_ratio", type=float, default=0.0, metavar="B",
                    help="--soft_regions: this fraction of the base prompt everywhere, the regions share the rest")
    ap.add_argument("--region_negative", action="append", default=[], metavar="I:PROMPT",
                    help="repeatable: a negative prompt of its own for the I-th --region (1-based); the others keep --null_prompt")
    ap.add_argument("--lora", action="append", default=[], metavar="PATH[:SCALE]",
                    help="LoRA safetensors file merged into the UNet on the device (repeatable; scale defaults to 1)")
    ap.add_argument("--ip_adapter", default=None, metavar="PATH[:SCALE]",
                    help="IP-Adapter safetensors file (ip-adapter_sd15 / _sdxl / _sdxl_vit-h, or 'synthetic'); needs --ip_image or --ip_embeds")
    ap.add_argument("--ip_image", default=None, help="reference picture (PNG / JPEG) for the IP-Adapter; needs --ip_adapter_dir")
    ap.add_argument("--ip_adapter_dir", default=None, help="folder that holds the CLIP image tower (image_encoder/)")
    ap.add_argument("--ip_embeds", default=None, metavar="FILE.npy", help="precomputed CLIP image embeds [1 or batch, embed_dim]")
    ap.add_argument("--draw", action="store_true", help="save z0t / zt decodes every step (draw_tweedie + draw_noisy)")
    ap.add_argument("--lcm_original_steps", type=int, default=None,
                    help="--method lcm: original_inference_steps of the LCM schedule (default: the checkpoint's scheduler_config.json, else 50)")
    ap.add_argument("--eta", type=float, default=None, help="--method dpm++_2m_sde* / dpm++_3m_sde* / dpm++_sde*: noise level (default 1; 0 = deterministic)")
    ap.add_argument("--s_noise", type=float, default=None, help="--method dpm++_*_sde*: noise multiplier (default 1)")
    ap.add_argument("--solver_type", default=None, choices=("midpoint", "heun"), help="--method dpm++_2m_sde*: second-order form (default midpoint)")
    ap.add_argument("--sigma_schedule", default=None, choices=("karras", "exponential"), help="--method dpm++_*_sde*: sigma schedule (default karras)")
    from cfgpp_amd.freeu import add_cli_flag, cli_kwargs
    add_cli_flag(ap)
    from cfgpp_amd import vpred
    vpred.add_cli_flags(ap)      # --prediction_type / --zero_terminal_snr / --timestep_spacing / --guidance_rescale
    args = ap.parse_args(argv)

    from cfgpp_amd.callback_util import ComposeCallback, save_image
    (args.workdir / "result").mkdir(parents=True, exist_ok=True)
    torch.manual_seed(args.seed)
    cfg = types.SimpleNamespace(num_sampling=args.NFE)
    callback = ComposeCallback(workdir=args.workdir, frequency=1, callbacks=["draw_noisy", "draw_tweedie"]) if args.draw else None
    kw = dict(solver_config=cfg, device=args.device, max_batch=args.batch, unet_weights=args.unet_weights)
    if args.vae_weights:
        kw["vae_weights"] = args.vae_weights
    if args.model_dir:        # a local diffusers-layout checkpoint: UNet / VAE weights, CLIP tower(s) + BPE tokenizer(s)
        from cfgpp_amd.checkpoint import solver_kwargs_from_dir
        found, missing = solver_kwargs_from_dir(args.model_dir, args.model in ("sdxl", "sdxl_lightning"), args.device)
        if missing:
            print(f"--model_dir {args.model_dir}: no {', '.join(missing)} there - synthetic stand-in(s) used")
        for k, v in found.items():
            if k.endswith("_weights") and getattr(args, k, None) not in (None, "synthetic"):
                continue                                   # an explicit --unet_weights / --vae_weights wins
            kw[k] = v
    if args.controlnet_dir:   # a local diffusers controlnet/ folder (config.json + safetensors); "synthetic" = seeded weights
        kw["controlnet"] = args.controlnet_dir
    if args.lora:
        from cfgpp_amd.lora import parse_cli
        kw["lora"] = parse_cli(args.lora)          # replaces a LoRA file --model_dir found next to the model
        kw.pop("lora_ignore_text_encoder", None)
    ip_kwargs = _ip_kwargs(args, kw)
    cli_kwargs(args, kw)
    vpred.cli_kwargs(args, kw)        # explicit flags win over the checkpoint's files
    if args.max_prompt_chunks > 1:
        kw["max_prompt_chunks"] = args.max_prompt_chunks
    if args.max_regions > 1:
        kw["max_regions"] = args.max_regions
    if args.soft_regions:
        if args.max_regions < 2:
            raise SystemExit("--soft_regions needs --max_regions 2 .. 4")
        kw["soft_regions"] = True
    elif args.region_feather or args.region_base_ratio:
        raise SystemExit("--region_feather / --region_base_ratio need --soft_regions")
    kw.update(solver_kwargs or {})
    prompts = [args.prompt] * args.batch if args.batch > 1 else args.prompt
    seeds = None if args.batch == 1 else [args.seed + i for i in range(args.batch)]   # B = 1: global CPU RNG, like the reference

    lcm = args.method == "lcm"      # the LCM sampler has its own registry (cfgpp_amd/lcm.py); --NFE, --cfg_guidance and --lora as ever
    if lcm:
        from cfgpp_amd.lcm import get_lcm_solver
        if args.lcm_original_steps is not None:
            kw["lcm_original_steps"] = args.lcm_original_steps
    from cfgpp_amd.sde import get_sde_solver, sde_solver_names
    sde = args.method in sde_solver_names()      # the SDE samplers have their own registry too (cfgpp_amd/sde.py)
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_solver_names, get_dpmpp_sde_solver
    if args.method in dpmpp_sde_solver_names():      # the two-stage DPM++ SDE sampler: the same options, its own registry again
        sde, get_sde_solver = True, get_dpmpp_sde_solver
    if sde:
        kw.update({k: getattr(args, k) for k in ("eta", "s_noise", "solver_type", "sigma_schedule") if getattr(args, k) is not None})
    if args.model in ("sdxl", "sdxl_lightning"):
        from cfgpp_amd.latent_sdxl import get_solver
        solver = (get_lcm_solver("lcm", model="sdxl", **kw) if lcm else get_sde_solver(args.method, model="sdxl", **kw) if sde
                  else get_solver(args.method, **kw))
        result = solver.sample(prompt1=[args.null_prompt, prompts], prompt2=[args.null_prompt, prompts],
                               cfg_guidance=args.cfg_guidance, target_size=(1024, 1024), callback_fn=callback, seeds=seeds,
                               **_control_kwargs(args, solver), **_ip_fit_embeds(ip_kwargs, solver), **_region_kwargs(args, solver))
    else:                                   # "sd20" is accepted and runs SD1.5, like the reference (quirk Q8)
        from cfgpp_amd.latent_diffusion import get_solver
        solver = (get_lcm_solver("lcm", model="sd15", **kw) if lcm else get_sde_solver(args.method, model="sd15", **kw) if sde
                  else get_solver(args.method, **kw))
        result = solver.sample(prompt=[args.null_prompt, prompts], cfg_guidance=args.cfg_guidance, callback_fn=callback, seeds=seeds,
                               **_control_kwargs(args, solver), **_ip_fit_embeds(ip_kwargs, solver), **_region_kwargs(args, solver))

    for i in range(result.shape[0]):
        name = "generated.png" if result.shape[0] == 1 else f"generated_{i}.png"
        save_image(result[i:i + 1], args.workdir / "result" / name, normalize=True)
    print(f"saved {result.shape[0]} image(s) to {args.workdir / 'result'}")


def _region_kwargs(args, solver):
    """--region X0,Y0,X1,Y1:PROMPT (repeatable) -> sample() kwargs: the region prompts and their rectangle masks at latent size"""
    if not args.region:
        return {}
    from cfgpp_amd.regions import parse_region, rect_mask
    if args.max_regions < 1 + len(args.region):
        raise SystemExit(f"--region given {len(args.region)} times: needs --max_regions {1 + len(args.region)} (the prompt is region 0; up to 4)")
    parsed = [parse_region(r) for r in args.region]
    out = dict(region_prompts=[p for _, p in parsed], region_masks=[rect_mask(*rect, solver.latent_hw) for rect, _ in parsed])
    if getattr(args, "soft_regions", False):
        from cfgpp_amd.regions import soft_rect_mask
        out["region_masks"] = [soft_rect_mask(*rect, solver.latent_hw, getattr(args, "region_feather", 0.0)) for rect, _ in parsed]
        out["region_base_ratio"] = getattr(args, "region_base_ratio", 0.0)
    if getattr(args, "region_negative", None):
        from cfgpp_amd.regions import parse_region_negative
        neg = [None] * len(parsed)
        for spec in args.region_negative:
            i, p = parse_region_negative(spec, len(parsed))
            neg[i - 1] = p
        out["region_negative_prompts"] = neg
    return out


def _ip_kwargs(args, kw):
    """--ip_adapter PATH[:SCALE] with --ip_image / --ip_embeds -> solver kwargs added to ``kw``, sample() kwargs returned"""
    if not args.ip_adapter:
        if args.ip_image or args.ip_embeds:
            raise SystemExit("--ip_image / --ip_embeds need --ip_adapter (an IP-Adapter safetensors file, or 'synthetic')")
        return {}
    path, _, scale = args.ip_adapter.rpartition(":")
    try:
        scale = float(scale) if path else 1.0
    except ValueError:
        path, scale = args.ip_adapter, 1.0
    kw["ip_adapter"] = path or args.ip_adapter
    if bool(args.ip_image) == bool(args.ip_embeds):
        raise SystemExit("--ip_adapter needs exactly one of --ip_image (with --ip_adapter_dir) and --ip_embeds")
    if args.ip_embeds:
        import numpy as np
        emb = torch.from_numpy(np.load(args.ip_embeds)).float()
        return dict(ip_adapter_image_embeds=emb, ip_adapter_scale=scale)       # shaped by _ip_fit_embeds once the adapter's kind is known
    if not args.ip_adapter_dir:
        raise SystemExit("--ip_image needs --ip_adapter_dir (the folder that holds the CLIP image_encoder/)")
    kw["ip_adapter_dir"] = args.ip_adapter_dir
    from PIL import Image
    import numpy as np
    img = torch.from_numpy(np.asarray(Image.open(args.ip_image).convert("RGB"), dtype=np.float32) / 255.0).permute(2, 0, 1)[None].contiguous()
    return dict(ip_adapter_image=img, ip_adapter_scale=scale)


def _ip_fit_embeds(ip_kwargs, solver):
    """--ip_embeds as the solver's adapter reads it: a Linear adapter takes pooled embeds ([E], [B, E] or [B, 1, E] -> [B, E]); a
    Resampler ("plus") adapter takes hidden states ([S, E] -> one row [1, S, E], or [B, S, E])"""
    emb = ip_kwargs.get("ip_adapter_image_embeds")
    if emb is None:
        return ip_kwargs
    adapter = getattr(getattr(solver, "engine", None), "ip_adapter", None)
    if adapter is not None and getattr(adapter, "seq_input", False):
        if emb.dim() not in (2, 3):
            raise SystemExit(f"--ip_embeds: shape {tuple(emb.shape)}; a plus (Resampler) adapter takes [S, E] or [B, S, E] hidden states")
        emb = emb[None] if emb.dim() == 2 else emb
    else:
        emb = emb.reshape(-1, emb.shape[-1])
    return dict(ip_kwargs, ip_adapter_image_embeds=emb)


def _control_kwargs(args, solver):
    if not args.control_image:
        return {}
    if not args.controlnet_dir:
        raise SystemExit("--control_image needs --controlnet_dir (a diffusers controlnet/ folder, or 'synthetic')")
    h, w = solver.latent_hw
    return dict(control_image=load_control_image(args.control_image, (8 * h, 8 * w)),
                controlnet_conditioning_scale=args.controlnet_conditioning_scale)


if __name__ == "__main__":
    main()
