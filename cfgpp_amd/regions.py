"""Regional prompts ("attention couple" / Regional Prompter, attention mode): region maps and the stacked text context for the
region-masked cross-attention of the HIP UNet (include/cfgpp_regions.h: cfgpp_unet_set_regions; csrc/attn_kernel.hip:
cfgpp_op_attention_region).  Host code, plain torch.

Semantics: R = 2 .. 4 regions per job.  Region 0 is the base prompt (the ordinary ``prompt`` of the call), regions 1 .. R - 1 come
with a prompt and a mask each.  The region map is an integer id per latent pixel, [1 or B, h, w]: it starts at 0, then mask i (in
list order, i = 1 ..) writes id i where it is set - later masks win over earlier ones; a hard partition.  Masks are accepted at
latent size [.., h, w] or at pixel size [.., 8h, 8w]; both are binarized at 0.5, and pixel masks are reduced the way
``inpaint.prepare_mask`` reduces its mask: nearest neighbour, pixel (8i, 8j).  The context of the job is [B, 77 R, D]: region r's
77-token prompt in tokens [77 r, 77 r + 77); the unconditional rows repeat their negative prompt R times and use the same map.

Not built: soft masks and a base-prompt ratio, per-region negative prompts, ControlNet and IP-Adapter with regions, long (chunked)
region prompts, graph replay of a region-masked loop.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

TOKENS = 77
MAX_REGIONS = 4


class RegionJob(NamedTuple):
    ids: torch.Tensor              # int64 [1 or B, h, w]
    embeds: Tuple[torch.Tensor, ...]   # the region prompts' hidden states, each [1 or B, 77, D] (regions 1 .. R - 1)
    serial: int

    @property
    def n_regions(self) -> int:
        return 1 + len(self.embeds)


def rect_mask(x0: float, y0: float, x1: float, y1: float, latent_hw: Tuple[int, int]) -> torch.Tensor:
    """a rectangle given as fractions of width (x) and height (y) -> latent-size mask [h, w] (1 inside): the latent pixels whose
    centre lies in [x0, x1) x [y0, y1)"""
    h, w = int(latent_hw[0]), int(latent_hw[1])
    if not (0.0 <= x0 < x1 <= 1.0 and 0.0 <= y0 < y1 <= 1.0):
        raise ValueError(f"rect_mask: rectangle ({x0}, {y0}, {x1}, {y1}) must satisfy 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1")
    cy = (torch.arange(h, dtype=torch.float64) + 0.5) / h
    cx = (torch.arange(w, dtype=torch.float64) + 0.5) / w
    return (((cy >= y0) & (cy < y1))[:, None] & ((cx >= x0) & (cx < x1))[None, :]).to(torch.float32)


def parse_region(spec: str) -> Tuple[Tuple[float, float, float, float], str]:
    """``"x0,y0,x1,y1:prompt"`` (the command line's --region) -> ((x0, y0, x1, y1), prompt)"""
    head, sep, prompt = str(spec).partition(":")
    parts = head.split(",")
    if not sep or len(parts) != 4:
        raise ValueError(f"--region {spec!r}: expected \"x0,y0,x1,y1:prompt\" with the rectangle as fractions of width and height")
    try:
        rect = tuple(float(p) for p in parts)
    except ValueError:
        raise ValueError(f"--region {spec!r}: the rectangle must be four numbers (fractions of width and height)") from None
    if not prompt.strip():
        raise ValueError(f"--region {spec!r}: empty prompt")
    return rect, prompt.strip()


def _latent_mask(mask: torch.Tensor, latent_hw: Tuple[int, int], i: int) -> torch.Tensor:
    """one mask -> bool [1 or B, h, w]"""
    h, w = int(latent_hw[0]), int(latent_hw[1])
    m = torch.as_tensor(mask).detach().cpu().float()
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3:
        raise ValueError(f"region_masks[{i}]: shape {tuple(m.shape)}, expected [h, w], [B, h, w] or [B, 1, h, w]")
    m = (m >= 0.5).to(torch.float32)
    if tuple(m.shape[1:]) == (8 * h, 8 * w):       # pixel size: nearest neighbour, pixel (8i, 8j), as inpaint.prepare_mask
        m = F.interpolate(m[:, None], size=(h, w))[:, 0]
    elif tuple(m.shape[1:]) != (h, w):
        raise ValueError(f"region_masks[{i}]: size {tuple(m.shape[1:])}, expected the latent size ({h}, {w}) or the pixel size ({8 * h}, {8 * w})")
    return m >= 0.5


def build_region_map(masks: Sequence[torch.Tensor], latent_hw: Tuple[int, int], batch: Optional[int]) -> torch.Tensor:
    """-> int64 [1 or B, h, w]: 0 everywhere, then mask i (1-based, list order) writes id i where it is set.  ``batch``: the job's
    batch size B, or None when it is not known yet (the engine then checks the rows against its context)"""
    if not 1 <= len(masks) <= MAX_REGIONS - 1:
        raise ValueError(f"region_masks: {len(masks)} masks (1 .. {MAX_REGIONS - 1}: with the base prompt that is 2 .. {MAX_REGIONS} regions)")
    ms = [_latent_mask(m, latent_hw, i) for i, m in enumerate(masks)]
    rows = max(int(m.shape[0]) for m in ms)
    for i, m in enumerate(ms):
        if int(m.shape[0]) not in (1, rows) or (batch is not None and rows not in (1, int(batch))):
            raise ValueError(f"region_masks[{i}]: {int(m.shape[0])} rows for a batch of {batch if batch is not None else rows} (1 or the batch size)")
    ids = torch.zeros((rows, int(latent_hw[0]), int(latent_hw[1])), dtype=torch.long)
    for i, m in enumerate(ms):
        ids = torch.where(m.expand_as(ids), torch.full_like(ids, i + 1), ids)
    return ids


def level_map(ids: torch.Tensor, level: int) -> torch.Tensor:
    """the map of UNet level ``level``: id_l[y, x] = id_0[y * 2^l, x * 2^l] (what the engine computes on the host)"""
    f = 1 << int(level)
    return ids[..., ::f, ::f]


def stack_context(uc: Optional[torch.Tensor], c: Optional[torch.Tensor], embeds: Sequence[torch.Tensor]):
    """(uc, c) [1 or B, 77, D] + the region prompts' hidden states -> (uc repeated R times, [c | region 1 | ..]) along the token
    axis, each [.., 77 R, D].  A side that is None stays None."""
    R = 1 + len(embeds)
    for t in (uc, c):
        if t is not None and int(t.shape[1]) != TOKENS:
            raise ValueError(f"region_prompts: the base context has {int(t.shape[1])} tokens; regions take plain 77-token prompts")
    out_uc = None if uc is None else uc.repeat(1, R, 1)
    out_c = None
    if c is not None:
        B = max([int(c.shape[0])] + [int(e.shape[0]) for e in embeds])
        parts = [c] + [e.to(c.device, c.dtype) for e in embeds]
        for i, p in enumerate(parts):
            if int(p.shape[0]) not in (1, B) or int(p.shape[1]) != TOKENS or int(p.shape[2]) != int(c.shape[2]):
                raise ValueError(f"region_prompts[{i - 1}]: hidden states {tuple(p.shape)} do not fit the base context {tuple(c.shape)}")
        out_c = torch.cat([p.expand(B, -1, -1) for p in parts], dim=1).contiguous()
    return out_uc, out_c


def check_lists(region_prompts, region_masks, max_regions: int) -> int:
    """-> number of regions of the call (1: a plain call)"""
    prompts = list(region_prompts or [])
    masks = list(region_masks or [])
    if len(prompts) != len(masks):
        raise ValueError(f"region_prompts has {len(prompts)} entries, region_masks {len(masks)}: one mask per region prompt")
    if not prompts:
        return 1
    R = 1 + len(prompts)
    if R > int(max_regions):
        raise ValueError(f"region_prompts: {len(prompts)} region prompts + the base prompt = {R} regions, the solver was built with "
                         f"max_regions={int(max_regions)} (get_solver(..., max_regions=R), R <= {MAX_REGIONS})")
    return R
