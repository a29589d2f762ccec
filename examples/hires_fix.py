"""Latent hires fix from the command line on the MI355X path: sample at a small size, upscale the LATENT inside the second job's start
launch, and denoise again at partial strength at the large size (cfgpp_amd/img2img.py: hires_fix).

    python examples/hires_fix.py --prompt "a corgi" --method ddim_cfg++ --cfg_guidance 0.6 --NFE 30 --img_size 512 \
        --hires_scale 1.5 --hires_strength 0.5 --hires_upscaler bilinear|bicubic|nearest-exact \
        [--hires_method dpm++_2m_sde_cfg++] [--hires_NFE 30] [--model sd15|sdxl] [--noise torch|philox] [--batch 4]

``--img_size`` is the FIRST pass's size; the second pass runs at ``img_size * hires_scale`` rounded to a multiple of 8.  Both passes take
the flags and plumbing of examples/text_to_img.py; ``--hires_method`` (default: ``--method``) is an img2img solver name.  Two engines
are built: an engine has one latent size.  The result goes to <workdir>/result/hires.png.
"""
from __future__ import annotations

import os
import sys
import types
from pathlib import Path

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import img2img as cli  # noqa: E402

REFERENCE_FLAGS = tuple((f, k, Path("examples/workdir/hires_fix") if f == "workdir" else d) for f, k, d in cli.REFERENCE_FLAGS)
EXTRA_FLAGS = tuple(t for t in cli.EXTRA_FLAGS if t[0] not in ("src_img", "strength")) + (
    ("hires_scale", float, 2.0), ("hires_strength", float, 0.5), ("hires_upscaler", str, "bilinear"), ("hires_method", str, None),
    ("hires_NFE", int, None))


def first_solver(args, kw):
    """the small pass: any text-to-image solver of the three registries examples/text_to_img.py serves"""
    from cfgpp_amd.dpmpp_sde import dpmpp_sde_solver_names, get_dpmpp_sde_solver
    from cfgpp_amd.sde import get_sde_solver, sde_solver_names
    kw = dict(kw, **cli.sde_kwargs_of(args, args.method))
    if args.method in dpmpp_sde_solver_names():
        return get_dpmpp_sde_solver(args.method, model=args.model, **kw)
    if args.method in sde_solver_names():
        return get_sde_solver(args.method, model=args.model, **kw)
    if args.model == "sdxl":
        from cfgpp_amd.latent_sdxl import get_solver
    else:
        from cfgpp_amd.latent_diffusion import get_solver
    return get_solver(args.method, **kw)


def main(argv=None, solver_kwargs=None, hires_solver_kwargs=None) -> None:
    """``solver_kwargs`` / ``hires_solver_kwargs`` let tests inject ``engine=`` / ``vae=`` (CPU mocks) into the two passes; the CLI never
    passes them."""
    ap = cli.build_parser(__doc__, REFERENCE_FLAGS + EXTRA_FLAGS)
    args = ap.parse_args(argv)
    from cfgpp_amd.img2img import UPSCALERS, get_img2img_solver, hires_fix
    if args.hires_upscaler not in UPSCALERS:
        ap.error(f"--hires_upscaler {args.hires_upscaler}: one of {', '.join(UPSCALERS)}")
    if not args.hires_scale >= 1.0:
        ap.error(f"--hires_scale {args.hires_scale}: at least 1 (downscaling is not built)")
    (args.workdir / "result").mkdir(parents=True, exist_ok=True)
    torch.manual_seed(args.seed)
    size = args.img_size or (1024 if args.model == "sdxl" else 512)
    small = size // 8
    big = max(small, int(round(small * args.hires_scale)))
    first = first_solver(args, cli.solver_kwargs_of(args, (small, small), solver_kwargs))
    method2 = args.hires_method or args.method
    kw2 = cli.solver_kwargs_of(args, (big, big), hires_solver_kwargs)
    kw2["solver_config"] = types.SimpleNamespace(num_sampling=args.hires_NFE or args.NFE)
    if first.text_encoder is not None:
        kw2.setdefault("text_encoder", first.text_encoder)         # one set of text towers serves both passes
    second = get_img2img_solver(method2, model=args.model, noise=args.noise, **cli.sde_kwargs_of(args, method2), **kw2)
    job = cli.job_kwargs(args, 8 * small)
    sizes = lambda n: dict(target_size=(8 * n, 8 * n), original_size=(8 * n, 8 * n)) if args.model == "sdxl" else {}  # noqa: E731
    for k in ("target_size", "original_size"):
        job.pop(k, None)
    result = hires_fix(first, second, job.pop("cfg_guidance"), job.pop("prompt"), strength=args.hires_strength, upscale=args.hires_upscaler,
                       seeds=job.pop("seeds"), first_kw=sizes(first.latent_hw[0]), second_kw=sizes(second.latent_hw[0]))
    st = second.last_start
    print(f"first pass {8 * first.latent_hw[0]} px, {args.NFE} steps; second pass {8 * second.latent_hw[0]} px, {st['steps']} of "
          f"{st['i0'] + st['steps']} steps ({st['mode']} latent upscale, strength {args.hires_strength})")
    cli.save_results(result, args.workdir / "result", "hires")


if __name__ == "__main__":
    main()
