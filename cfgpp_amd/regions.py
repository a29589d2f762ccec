"""Regional prompts ("attention couple" / Regional Prompter, attention mode): region maps and the stacked text context for the
region-masked cross-attention of the HIP UNet (include/cfgpp_regions.h: cfgpp_unet_set_regions; csrc/attn_kernel.hip:
cfgpp_op_attention_region).  Host code, plain torch.

Semantics: R = 2 .. 4 regions per job.  Region 0 is the base prompt (the ordinary ``prompt`` of the call), regions 1 .. R - 1 come
with a prompt and a mask each.  The region map is an integer id per latent pixel, [1 or B, h, w]: it starts at 0, then mask i (in
list order, i = 1 ..) writes id i where it is set - later masks win over earlier ones; a hard partition.  Masks are accepted at
latent size [.., h, w] or at pixel size [.., 8h, 8w]; both are binarized at 0.5, and pixel masks are reduced the way
``inpaint.prepare_mask`` reduces its mask: nearest neighbour, pixel (8i, 8j).  The context of the job is [B, 77 R, D]: region r's
77-token prompt in tokens [77 r, 77 r + 77); the unconditional rows repeat their negative prompt R times and use the same map.

Soft mode (``get_solver(..., max_regions=R, soft_regions=True)``; include/cfgpp_regions_soft.h: cfgpp_unet_set_region_weights;
csrc/attn_kernel.hip: cfgpp_op_attention_region_soft): masks are float masks in [0, 1] and are NOT binarized (pixel-size masks are
reduced by the same nearest-neighbour rule).  A pixel gets a weight per region, ``build_region_weights``: layer compositing (w_0 = 1;
mask i sets w_j <- w_j (1 - m_i) for j < i and w_i = m_i), then the base ratio ``region_base_ratio`` = beta (w_0 <- beta + (1 - beta)
w_0, w_i <- (1 - beta) w_i); the cross-attention output at the pixel is sum_r w_r softmax(q K_r) V_r.  The level maps are the same
nearest downsample (``level_weights``).  0/1 masks with beta = 0 are the hard partition, computed by the soft kernel (per launch
faster than the hard path's row kernel at head dims 80 / 160, slower than its resident kernel at head dims padded to 64:
profiles/regional_soft/README.md).  ``soft_rect_mask`` feathers a rectangle.

Per-region negative prompts (both modes): ``sample(..., region_negative_prompts=[n1, ..])``, one entry per region prompt, None = the
job's negative prompt; the unconditional context becomes [uc | uc_1 | ..] (``stack_context(..., negative_embeds=)``).

Not built: area-averaged level weights, ControlNet and IP-Adapter with regions, long (chunked) region prompts, graph replay of a
region-masked loop, routing hard maps onto the soft kernel.
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
    weights: Optional[torch.Tensor] = None      # soft mode: float32 [1 or B, R, h, w] (build_region_weights); ids is then None
    negative_embeds: Optional[Tuple[Optional[torch.Tensor], ...]] = None    # per region prompt; None entries = the job's negative prompt

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


def _float_mask(mask: torch.Tensor, latent_hw: Tuple[int, int], i: int) -> torch.Tensor:
    """one soft mask -> float32 [1 or B, h, w] in [0, 1], NOT binarized; a pixel-size mask is reduced by _latent_mask's rule"""
    h, w = int(latent_hw[0]), int(latent_hw[1])
    m = torch.as_tensor(mask).detach().cpu().float()
    if m.dim() == 4 and m.shape[1] == 1:
        m = m[:, 0]
    if m.dim() == 2:
        m = m[None]
    if m.dim() != 3:
        raise ValueError(f"region_masks[{i}]: shape {tuple(m.shape)}, expected [h, w], [B, h, w] or [B, 1, h, w]")
    if not bool(torch.isfinite(m).all()) or float(m.min()) < 0.0 or float(m.max()) > 1.0:
        raise ValueError(f"region_masks[{i}]: soft masks hold values in [0, 1]")
    if tuple(m.shape[1:]) == (8 * h, 8 * w):       # pixel size: nearest neighbour, pixel (8i, 8j)
        m = F.interpolate(m[:, None], size=(h, w))[:, 0]
    elif tuple(m.shape[1:]) != (h, w):
        raise ValueError(f"region_masks[{i}]: size {tuple(m.shape[1:])}, expected the latent size ({h}, {w}) or the pixel size ({8 * h}, {8 * w})")
    return m


def check_base_ratio(base_ratio) -> float:
    b = float(base_ratio)
    if not 0.0 <= b <= 1.0:           # (NaN fails both comparisons)
        raise ValueError(f"region_base_ratio={base_ratio}: a fraction in [0, 1]")
    return b


def build_region_weights(masks: Sequence[torch.Tensor], latent_hw: Tuple[int, int], batch: Optional[int], base_ratio: float = 0.0) -> torch.Tensor:
    """soft masks m_i in [0, 1] -> float32 weights [1 or B, R, h, w], R = 1 + len(masks), computed in fp32.  Layer compositing, the
    generalisation of "later masks win": w_0 = 1; mask i = 1, 2, .. in list order sets w_j <- w_j (1 - m_i) for j < i and w_i = m_i.
    Then the base ratio beta: w_0 <- beta + (1 - beta) w_0, w_i <- (1 - beta) w_i.  The weights of a pixel sum to 1 up to fp32
    rounding and are not renormalised; 0/1 masks with beta = 0 give the one-hot map of ``build_region_map``."""
    beta = check_base_ratio(base_ratio)
    if not 1 <= len(masks) <= MAX_REGIONS - 1:
        raise ValueError(f"region_masks: {len(masks)} masks (1 .. {MAX_REGIONS - 1}: with the base prompt that is 2 .. {MAX_REGIONS} regions)")
    ms = [_float_mask(m, latent_hw, i) for i, m in enumerate(masks)]
    rows = max(int(m.shape[0]) for m in ms)
    for i, m in enumerate(ms):
        if int(m.shape[0]) not in (1, rows) or (batch is not None and rows not in (1, int(batch))):
            raise ValueError(f"region_masks[{i}]: {int(m.shape[0])} rows for a batch of {batch if batch is not None else rows} (1 or the batch size)")
    h, w = int(latent_hw[0]), int(latent_hw[1])
    ws = [torch.ones((rows, h, w), dtype=torch.float32)]
    for m in ms:
        m = m.expand(rows, h, w)
        ws = [x * (1.0 - m) for x in ws] + [m.clone()]
    out = torch.stack(ws, 1)
    if beta != 0.0:
        out = out * (1.0 - beta)
        out[:, 0] += beta
    return out.contiguous()


def level_weights(w: torch.Tensor, level: int) -> torch.Tensor:
    """the weights of UNet level ``level``: w_l[r, y, x] = w_0[r, y * 2^l, x * 2^l], the nearest downsample the hard path uses (what
    the engine computes on the host; no area averaging)"""
    f = 1 << int(level)
    return w[..., ::f, ::f]


def soft_rect_mask(x0: float, y0: float, x1: float, y1: float, latent_hw: Tuple[int, int], feather: float = 0.0) -> torch.Tensor:
    """``rect_mask`` with feathered borders: a linear ramp of width ``feather`` (a fraction of the image's shorter side) centred on
    each edge of the rectangle - 0 at feather / 2 outside, 0.5 on the edge, 1 at feather / 2 inside; the two axes multiply.
    ``feather = 0`` is exactly ``rect_mask``.  EVERY edge ramps, one that coincides with the image border included: a feathered
    "right half" (x1 = 1) also fades towards the base prompt over the last feather / 2 of the image (0.5 would be reached on the
    border itself).  Pass a float mask of your own where the border should stay at 1."""
    f = float(feather)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"soft_rect_mask: feather={feather} must be a fraction in [0, 1]")
    hard = rect_mask(x0, y0, x1, y1, latent_hw)
    if f == 0.0:
        return hard
    h, w = int(latent_hw[0]), int(latent_hw[1])
    side = float(min(h, w))
    cy = (torch.arange(h, dtype=torch.float64) + 0.5) / h
    cx = (torch.arange(w, dtype=torch.float64) + 0.5) / w

    def ramp(c, lo, hi, n):
        fa = f * side / n                         # the ramp's width as a fraction of this axis
        return (torch.minimum(c - lo, hi - c) / fa + 0.5).clamp(0.0, 1.0)
    return (ramp(cy, y0, y1, h)[:, None] * ramp(cx, x0, x1, w)[None, :]).to(torch.float32)


def parse_region_negative(spec: str, n_region_prompts: int) -> Tuple[int, str]:
    """``"i:prompt"`` (the command line's --region_negative; i = 1 .. the number of --region entries) -> (i, prompt)"""
    head, sep, prompt = str(spec).partition(":")
    try:
        i = int(head)
    except ValueError:
        i = 0
    if not sep or not 1 <= i <= int(n_region_prompts):
        raise ValueError(f"--region_negative {spec!r}: expected \"i:prompt\" with i = 1 .. {int(n_region_prompts)} (the --region entries, in order)")
    if not prompt.strip():
        raise ValueError(f"--region_negative {spec!r}: empty prompt")
    return i, prompt.strip()


def check_negatives(region_negative_prompts, n_region_prompts: int):
    """-> the list (None entries: the job's negative prompt), or None when no region has a negative prompt of its own"""
    if region_negative_prompts is None:
        return None
    neg = list(region_negative_prompts)
    if len(neg) != int(n_region_prompts):
        raise ValueError(f"region_negative_prompts has {len(neg)} entries, region_prompts {int(n_region_prompts)}: one per region prompt (None = the "
                         "job's negative prompt)")
    return neg if any(n is not None for n in neg) else None


def stack_context(uc: Optional[torch.Tensor], c: Optional[torch.Tensor], embeds: Sequence[torch.Tensor], *,
                  negative_embeds: Optional[Sequence[Optional[torch.Tensor]]] = None):
    """(uc, c) [1 or B, 77, D] + the region prompts' hidden states -> (uc repeated R times, [c | region 1 | ..]) along the token
    axis, each [.., 77 R, D].  A side that is None stays None.  ``negative_embeds`` (per region prompt, None entries = uc): the
    unconditional side becomes [uc | uc_1 | ..] instead of uc repeated."""
    R = 1 + len(embeds)
    for t in (uc, c):
        if t is not None and int(t.shape[1]) != TOKENS:
            raise ValueError(f"region_prompts: the base context has {int(t.shape[1])} tokens; regions take plain 77-token prompts")
    if negative_embeds is not None and uc is not None:
        if len(negative_embeds) != len(embeds):
            raise ValueError(f"region_negative_prompts has {len(negative_embeds)} entries, region_prompts {len(embeds)}")
        parts = [uc] + [uc if e is None else e.to(uc.device, uc.dtype) for e in negative_embeds]
        B = max(int(p.shape[0]) for p in parts)
        for i, p in enumerate(parts):
            if int(p.shape[0]) not in (1, B) or int(p.shape[1]) != TOKENS or int(p.shape[2]) != int(uc.shape[2]):
                raise ValueError(f"region_negative_prompts[{i - 1}]: hidden states {tuple(p.shape)} do not fit the unconditional context {tuple(uc.shape)}")
        out_uc = torch.cat([p.expand(B, -1, -1) for p in parts], dim=1).contiguous()
    else:
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
