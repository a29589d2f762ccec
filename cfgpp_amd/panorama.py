"""MultiDiffusion panoramas: images larger than the UNet's window (DDIM and DDIM-CFG++, SD1.5 and SDXL).

The method of diffusers' ``StableDiffusionPanoramaPipeline`` (Bar-Tal et al., ICML'23): the panorama latent ``[B, 4, Hp, Wp]`` is cut
into overlapping views of the UNet's own latent size, every view takes an ordinary denoising step, and where views overlap the
results are averaged.  The DDIM / CFG++ update is affine in a view's eps, so CFG++ composes with it unchanged: each view is updated
with its own ``eps_uc`` / ``eps_c``.

What a step costs here: ``V / Vc`` UNet forwards at ``2 * Vc * B`` rows (the views are batch rows: one prompt fills the large-batch
tiles) and ONE launch - ``engine.step_ddim_views`` (include/cfgpp_panorama.h) updates every view, averages, and scatters the new
latent into the views' UNet input slots, so nothing is sliced, accumulated or gathered between steps.

Like the inpaint solvers these are not in the ``latent_diffusion`` / ``latent_sdxl`` registries (those mirror the reference's
lists): ``get_panorama_solver(name, model="sd15" | "sdxl", panorama_hw=(Hp, Wp), stride=8, ...)``.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Tuple

import torch

from . import coeffs as K
from .latent_diffusion import StableDiffusion, _progress
from .latent_sdxl import SDXL
from .registry import Registry

__PANORAMA_SOLVER__ = Registry("PanoramaSolver")
MODELS = ("sd15", "sdxl")


# ---------------------------------------------------------------------------------------------------- view geometry (host)
def panorama_views(Hp: int, Wp: int, h: int, w: int, stride: int, circular: bool = False) -> List[Tuple[int, int]]:
    """``(y0, x0)`` of every view, in view order, in latent units: diffusers' ``get_views`` rule.  With ``circular`` the views also
    start in the last ``w - stride`` columns and their columns are taken mod ``Wp``.  Sizes diffusers would silently leave
    uncovered (value 0) are refused here."""
    Hp, Wp, h, w, stride = int(Hp), int(Wp), int(h), int(w), int(stride)
    if min(Hp, Wp, h, w) < 1 or stride < 1:
        raise ValueError(f"panorama: sizes and stride must be positive (panorama {Hp} x {Wp}, window {h} x {w}, stride {stride})")
    if Hp < h or Wp < w:
        raise ValueError(f"panorama_hw=({Hp}, {Wp}) is smaller than the window ({h}, {w}) (latent units)")
    for name, v in (("stride", stride), ("the window's width", w), ("the panorama's width", Wp)):
        if v % 4:
            raise ValueError(f"panorama: {name} = {v} latent columns must be a multiple of 4 (the step kernel moves 16-byte vectors)")
    if stride > h or stride > w:
        raise ValueError(f"panorama: stride={stride} exceeds the window ({h}, {w}): pixels between views would stay uncovered")
    if (Hp - h) % stride:
        raise ValueError(f"panorama: (Hp - h) = {Hp} - {h} is not a multiple of stride={stride}: the last rows would stay uncovered")
    if circular and Wp % stride:
        raise ValueError(f"panorama: circular_padding with Wp = {Wp} not a multiple of stride={stride}: the seam would be covered unevenly")
    if not circular and (Wp - w) % stride:
        raise ValueError(f"panorama: (Wp - w) = {Wp} - {w} is not a multiple of stride={stride}: the last columns would stay uncovered")
    nbh = (Hp - h) // stride + 1 if Hp > h else 1
    nbw = (Wp // stride if circular else (Wp - w) // stride + 1) if Wp > w else 1
    return [((i // nbw) * stride, (i % nbw) * stride) for i in range(nbh * nbw)]


@dataclasses.dataclass(frozen=True)
class ViewGeometry:
    """what the engine's panorama entry points take: the sizes, and ``chunk_views`` (Vc) views per UNet forward"""
    Hp: int
    Wp: int
    h: int
    w: int
    stride: int
    circular: bool
    chunk_views: int = 1

    @property
    def views(self) -> List[Tuple[int, int]]:
        return panorama_views(self.Hp, self.Wp, self.h, self.w, self.stride, self.circular)

    @property
    def n_views(self) -> int:
        return len(self.views)

    def with_chunk(self, Vc: int) -> "ViewGeometry":
        return dataclasses.replace(self, chunk_views=int(Vc))


def view_chunk(n_views: int, B: int, max_batch: int, view_batch_size: Optional[int] = None) -> int:
    """Vc, the views per forward: it divides the view count and ``Vc * B <= max_batch`` (the engine's rows per CFG half).  Default:
    the largest such divisor."""
    fits = [d for d in range(1, int(n_views) + 1) if n_views % d == 0 and d * int(B) <= int(max_batch)]
    if not fits:
        raise ValueError(f"panorama: a batch of {B} chains exceeds max_batch={max_batch}")
    if view_batch_size is None:
        return fits[-1]
    if int(view_batch_size) not in fits:
        raise ValueError(f"view_batch_size={view_batch_size}: it must divide the {n_views} views and view_batch_size * {B} chains must "
                         f"fit max_batch={max_batch}; the values that do: {fits}")
    return int(view_batch_size)


# ---------------------------------------------------------------------------------------------------- registry
def register_panorama_solver(name: str, model: str):
    return __PANORAMA_SOLVER__.register(f"{model}/{name}")


def get_panorama_solver(name: str, model: str = "sd15", panorama_hw: Optional[Tuple[int, int]] = None, stride: int = 8,
                        circular_padding: bool = False, view_batch_size: Optional[int] = None, **kwargs):
    """``name`` in {"ddim_panorama", "ddim_panorama_cfg++"}, ``model`` in {"sd15", "sdxl"}.  ``panorama_hw`` = (Hp, Wp) and
    ``stride`` in latent units; ``latent_hw`` (a ``get_solver`` kwarg) is the window; ``max_batch`` bounds ``view_batch_size * B``.
    Every other kwarg as ``get_solver``'s."""
    if model not in MODELS:
        raise ValueError(f"PanoramaSolver model {model!r}: one of {MODELS}")
    try:
        cls = __PANORAMA_SOLVER__[f"{model}/{name}"]
    except KeyError:
        raise ValueError(f"PanoramaSolver {name} does not exist.") from None
    if panorama_hw is None:
        raise ValueError("get_panorama_solver needs panorama_hw=(Hp, Wp) in latent units")
    cfg = kwargs.get("unet_config", cls.unet_config)
    h, w = kwargs.get("latent_hw", (cfg.sample_size, cfg.sample_size))
    geom = ViewGeometry(int(panorama_hw[0]), int(panorama_hw[1]), int(h), int(w), int(stride), bool(circular_padding))
    view_chunk(geom.n_views, 1, int(kwargs.get("max_batch", 1)), view_batch_size)      # every refusal before anything is built
    return cls(panorama=geom, view_batch_size=view_batch_size, **kwargs)


def panorama_solver_names():
    return sorted({k.split("/", 1)[1] for k in __PANORAMA_SOLVER__})


# ---------------------------------------------------------------------------------------------------- the loop
_REFUSED_KWARGS = ("control_image", "ip_adapter_image_embeds", "negative_ip_adapter_image_embeds", "ip_adapter_image")


class _PanoramaMixin:
    """shared by the SD1.5 and SDXL classes: the views, the tiled conditioning, the loop"""

    cfgpp = False
    controllable = False
    vpred_ok = False
    rescale_ok = False

    def __init__(self, *args, panorama: ViewGeometry, view_batch_size: Optional[int] = None, **kwargs):
        self.geometry = panorama
        self.view_batch_size = view_batch_size
        self.panorama_hw = (panorama.Hp, panorama.Wp)
        self._vae_rows = 1
        super().__init__(*args, **kwargs)
        if tuple(self.latent_hw) != (panorama.h, panorama.w):
            raise ValueError(f"panorama: window {tuple(self.latent_hw)} != the geometry's ({panorama.h}, {panorama.w})")

    def _refuse_unsupported_prediction(self, zero_snr: bool, spacing: str):
        if self.prediction_type == "v_prediction":
            raise ValueError(f"{self._name()}: prediction_type='v_prediction' is not supported by the panorama solvers (the fused view "
                             "step is the epsilon update)")
        super()._refuse_unsupported_prediction(zero_snr, spacing)

    def _check_guidance_rescale(self, phi) -> float:
        if float(phi) > 0.0:
            raise ValueError(f"{self._name()}: guidance_rescale={float(phi)} is not supported by the panorama solvers")
        return super()._check_guidance_rescale(phi)

    def _refuse_job(self, kwargs):
        """what a panorama job does not take, by name, before anything runs"""
        for k in _REFUSED_KWARGS:
            if kwargs.get(k) is not None:
                what = "ControlNet conditioning" if k == "control_image" else "IP-Adapter image prompts"
                raise ValueError(f"{type(self).__name__}.sample() does not take {k}: {what} per view are not supported by the panorama "
                                 "solvers")
        if kwargs.get("region_prompts") or kwargs.get("region_masks"):
            raise ValueError(f"{type(self).__name__}.sample() does not take region_prompts: regional prompts per view are not supported by "
                             "the panorama solvers")
        if kwargs.get("guidance_rescale"):
            self._check_guidance_rescale(kwargs["guidance_rescale"])
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("the panorama solvers are not supported in sharded runs (world size > 1): the views of one panorama share "
                             "one latent")

    def _get_vae(self):
        """the VAE decodes the whole panorama: built at ``panorama_hw``, for the chains of the job"""
        if self.vae is not None and getattr(self.vae, "_pano_rows", self._vae_rows) < self._vae_rows:
            self.vae = None                      # a later job with more chains
        if self.vae is None:
            if self.work_device.type != "cuda":
                return super()._get_vae()        # (raises: on CPU the VAE is injected)
            from .vae import HipVAE
            self.vae = HipVAE(self.cfg.vae_scale, self.panorama_hw, max_batch=self._vae_rows, device=self.work_device, **self._vae_kwargs)
            self.vae._pano_rows = self._vae_rows
        return self.vae

    @staticmethod
    def _tile_rows(x, B: int, Vc: int):
        """conditioning rows for ``Vc`` views of ``B`` chains: row v * B + b = chain b's.  [B | 1, ...] -> [Vc * B, ...]; a
        [2B, ...] tensor (negative rows, then positive rows) is tiled half by half."""
        n = int(x.shape[0])
        rep = (1,) * (x.dim() - 1)
        if n == 2 * B and B >= 1 and x.dim() == 2:
            return torch.cat([x[:B].repeat(Vc, *rep), x[B:].repeat(Vc, *rep)], 0)
        if n == 1:
            x = x.expand(B, *x.shape[1:])
        elif n != B:
            raise ValueError(f"panorama: conditioning with {n} rows for {B} chains")
        return x.repeat(Vc, *rep).contiguous()

    def _panorama_loop(self, zt, uc, c, lam, wrap: bool, added=None, callback_fn=None, desc="SD-panorama"):
        """THE loop: per step V / Vc forwards into the views' eps slots, then one fused view step.  ``zt`` [B, 4, Hp, Wp] fp32.
        Always eager (also under $CFGPP_GRAPH=1): the captured step has no view form.  Returns the panorama's (z0t, zt)."""
        g0, eng = self.geometry, self.engine
        B = int(zt.shape[0])
        if tuple(zt.shape[1:]) != (self.cfg.out_channels, g0.Hp, g0.Wp):
            raise ValueError(f"panorama: latent shape {tuple(zt.shape)} != [B, {self.cfg.out_channels}, {g0.Hp}, {g0.Wp}]")
        V = g0.n_views
        Vc = view_chunk(V, B, self.max_batch, self.view_batch_size)
        g = g0.with_chunk(Vc)
        rows = Vc * B
        self._vae_rows = max(self._vae_rows, B)
        zt = self._own_latent(zt.float())
        dev = zt.device
        z0t = torch.empty_like(zt)
        z_views = torch.empty((V * B, self.cfg.out_channels, g.h, g.w), dtype=torch.float32, device=dev)
        eps = torch.empty((V // Vc, 2 * rows, self.cfg.out_channels, g.h, g.w), dtype=torch.float16, device=dev)
        # the text context of one chunk, set once per job: every chunk has the same rows (view v of chain b -> chain b's prompt)
        uc_t, c_t = self._tile_rows(uc, B, Vc), self._tile_rows(c, B, Vc)
        if added is not None:
            added = {k: self._tile_rows(v, B, Vc) for k, v in added.items()}
        self._ensure_context(uc_t, c_t, added)
        ts = self.scheduler.timesteps
        ts = ts.int() if wrap else ts
        eng.gather_views(g, zt, z_views)
        for step, t in enumerate(_progress(ts, desc)):
            sqrt4, dev_a = self._ddim_step_coeffs(t, False, wrap)
            for k in range(V // Vc):
                eng.predict_into(z_views[k * rows:(k + 1) * rows], float(t), eps[k])
            co = K.ddim_coeffs_pinned(sqrt4, eps_half=True, semantics=self.scalar_semantics, z_half=False, device_alpha=dev_a)
            eng.step_ddim_views(g, zt, z0t, z_views, eps, lam, co, False, self.cfgpp)
            if callback_fn is not None:
                z0d, zd, version = z0t.detach(), zt.detach(), zt._version
                kw = callback_fn(step, t, {"z0t": z0d, "zt": zd, "decode": self.decode})
                if kw["z0t"] is not z0d:
                    z0t.copy_(kw["z0t"])
                if kw["zt"] is not zd or zt._version != version:      # the callback replaced or edited the panorama: the views follow it
                    if kw["zt"] is not zd:
                        zt.copy_(kw["zt"])
                    eng.gather_views(g, zt, z_views)
        return z0t, zt

    def _start_latent(self, B: int, seeds, latents):
        if latents is not None:
            return latents
        return self._randn((B, self.cfg.out_channels) + self.panorama_hw, seeds).to(self.work_device)


# ---------------------------------------------------------------------------------------------------- SD1.5
class PanoramaDDIM(_PanoramaMixin, StableDiffusion):
    """SD1.5 MultiDiffusion, DDIM with CFG (eps_hat renoises)."""

    @torch.no_grad()
    def sample(self, cfg_guidance=7.5, prompt=["", ""], callback_fn=None, **kwargs):
        """-> the decoded panorama [B, 3, 8 Hp, 8 Wp], or the panorama's ``(z0t, zt)`` with ``return_latents=True``.  ``prompt`` /
        ``prompt_embeds`` / ``seeds`` / ``latents`` ([B, 4, Hp, Wp]) / ``lora_scale`` as the text-to-image solvers'."""
        self._refuse_job(kwargs)
        if kwargs.get("lora_scale") is not None:
            self.set_lora_scale(kwargs["lora_scale"])
        uc, c = self._embeds(prompt, kwargs)
        B = int(c.shape[0])
        zt = self._start_latent(B, kwargs.get("seeds"), kwargs.get("latents"))
        z0t, zt = self._panorama_loop(zt, uc, c, cfg_guidance, False, callback_fn=callback_fn)
        return self._result(kwargs.get("return_latents"), (z0t, zt), z0t)


class PanoramaDDIMCFGpp(PanoramaDDIM):
    """SD1.5 MultiDiffusion, DDIM with CFG++ (renoise with eps_uc)."""
    cfgpp = True


register_panorama_solver("ddim_panorama", "sd15")(PanoramaDDIM)
register_panorama_solver("ddim_panorama_cfg++", "sd15")(PanoramaDDIMCFGpp)


# ---------------------------------------------------------------------------------------------------- SDXL
class PanoramaDDIMXL(_PanoramaMixin, SDXL):
    """SDXL MultiDiffusion, DDIM with CFG; the SDXL DDIM index rule (quirk Q3: ``wrap``), as ``InpaintDDIMXL``.  Every view gets the
    same size conditioning: ``original_size = target_size =`` the window's pixel size, crop (0, 0), unless ``sample`` is given
    others.  A single ``prompt=[null, text]`` is taken for both towers."""

    @torch.no_grad()
    def sample(self, *args, **kwargs):
        self._refuse_job(kwargs)
        p = kwargs.pop("prompt", None)
        if p is not None:
            kwargs.setdefault("prompt1", p)
            kwargs.setdefault("prompt2", p)
        if kwargs.get("target_size") is None:
            h, w = self.latent_hw
            kwargs["target_size"] = (8 * h, 8 * w)
            if kwargs.get("original_size") is None:
                kwargs["original_size"] = (8 * h, 8 * w)
        ret_lat = kwargs.pop("return_latents", False)
        z0t = super().sample(*args, return_latents=True, **kwargs)
        return self._last_latents if ret_lat else self._finish(z0t)

    def reverse_process(self, null_prompt_embeds, prompt_embeds, cfg_guidance, add_cond_kwargs, shape=(1024, 1024), callback_fn=None,
                        seeds=None, latents=None, **kwargs):
        B = int(prompt_embeds.shape[0])
        zt = self._start_latent(B, seeds, latents)
        self._last_latents = self._panorama_loop(zt, null_prompt_embeds, prompt_embeds, cfg_guidance, True, add_cond_kwargs, callback_fn,
                                                 "SDXL-panorama")
        return self._last_latents[0]


class PanoramaDDIMXLCFGpp(PanoramaDDIMXL):
    """SDXL MultiDiffusion, DDIM with CFG++ (renoise with eps_uc)."""
    cfgpp = True


register_panorama_solver("ddim_panorama", "sdxl")(PanoramaDDIMXL)
register_panorama_solver("ddim_panorama_cfg++", "sdxl")(PanoramaDDIMXLCFGpp)


if __name__ == "__main__":
    print(f"panorama solvers: {panorama_solver_names()} for models {MODELS}")
