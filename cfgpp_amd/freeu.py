"""FreeU settings (diffusers ``UNet2DConditionModel.enable_freeu(s1, s2, b1, b2)``): parsing only.  The edit itself is a HIP
kernel inside the UNet's up path (csrc/freeu_kernel.hip, include/cfgpp_freeu.h).

A spec is ``None`` (off: the plain engine), a sequence ``(s1, s2, b1, b2)`` or a mapping with exactly those four keys - diffusers'
parameter names and order.  There are no named presets: the published values differ by source and model."""
from __future__ import annotations

import math
from typing import Optional, Tuple

KEYS = ("s1", "s2", "b1", "b2")


def add_cli_flag(ap) -> None:
    """``--freeu S1,S2,B1,B2`` of the example command lines"""
    ap.add_argument("--freeu", default=None, metavar="S1,S2,B1,B2",
                    help="FreeU (diffusers enable_freeu(s1, s2, b1, b2)): skip low-pass scales s1, s2 and backbone scales b1, b2 of "
                         "up_blocks.0 / up_blocks.1; absent = off")


def cli_kwargs(args, kw) -> None:
    """--freeu -> ``kw['freeu']`` (a malformed value ends the command with its reason)"""
    if getattr(args, "freeu", None):
        try:
            kw["freeu"] = parse_freeu(args.freeu)
        except ValueError as e:
            raise SystemExit(f"--freeu: {e}") from None


def parse_freeu(spec) -> Optional[Tuple[float, float, float, float]]:
    """-> (s1, s2, b1, b2) as floats, or None.  Raises ValueError naming what is wrong."""
    if spec is None:
        return None
    if isinstance(spec, str):
        parts = [p.strip() for p in spec.split(",")]
        if len(parts) != 4:
            raise ValueError(f"freeu={spec!r}: expected four comma-separated numbers S1,S2,B1,B2")
        spec = parts
    if isinstance(spec, dict):
        if set(spec) != set(KEYS):
            raise ValueError(f"freeu=...: a mapping needs exactly the keys s1, s2, b1, b2 (got {sorted(map(str, spec))})")
        spec = [spec[k] for k in KEYS]
    try:
        vals = tuple(float(v) for v in spec)
    except (TypeError, ValueError):
        raise ValueError(f"freeu={spec!r}: expected (s1, s2, b1, b2) as numbers, a mapping with those keys, or None") from None
    if len(vals) != 4:
        raise ValueError(f"freeu=...: expected four values (s1, s2, b1, b2), got {len(vals)}")
    for k, v in zip(KEYS, vals):
        if not math.isfinite(v):
            raise ValueError(f"freeu=...: {k}={v} is not finite")
    return vals
