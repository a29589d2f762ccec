"""Command-line face of the v-prediction options (DESIGN.md "v-prediction"): the four flags the example command lines share.
The arithmetic lives in csrc/vpred_kernels.hip (include/cfgpp_vpred.h), the schedules in schedule.py, the plumbing in
latent_diffusion.py; a checkpoint's own files are read by checkpoint.solver_kwargs_from_dir."""
from __future__ import annotations


def add_cli_flags(ap) -> None:
    """``--prediction_type`` / ``--zero_terminal_snr`` / ``--timestep_spacing`` / ``--guidance_rescale``; every default is "not
    given", so that a checkpoint directory's scheduler_config.json decides unless the flag is on the command line"""
    ap.add_argument("--prediction_type", default=None, choices=("epsilon", "v_prediction"),
                    help="what the UNet predicts (default: the checkpoint's scheduler_config.json, else epsilon)")
    ap.add_argument("--zero_terminal_snr", default=None, type=int, choices=(0, 1),
                    help="1: the zero-terminal-SNR noise schedule (needs --timestep_spacing trailing and v_prediction); default: the "
                         "checkpoint's rescale_betas_zero_snr, else 0")
    ap.add_argument("--timestep_spacing", default=None, choices=("leading", "trailing"),
                    help="DDIM timestep spacing (default: the checkpoint's, else leading)")
    ap.add_argument("--guidance_rescale", default=None, type=float,
                    help="rescale_noise_cfg factor phi in 0 .. 1 for ddim / ddim_cfg++ with v_prediction (default 0: off)")


def cli_kwargs(args, kw) -> None:
    """the flags that were given -> ``kw`` (they win over what ``solver_kwargs_from_dir`` put there)"""
    if getattr(args, "prediction_type", None) is not None:
        kw["prediction_type"] = args.prediction_type
    if getattr(args, "zero_terminal_snr", None) is not None:
        kw["zero_terminal_snr"] = bool(args.zero_terminal_snr)
    if getattr(args, "timestep_spacing", None) is not None:
        kw["timestep_spacing"] = args.timestep_spacing
    if getattr(args, "guidance_rescale", None) is not None:
        kw["guidance_rescale"] = float(args.guidance_rescale)
