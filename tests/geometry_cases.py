"""Non-square and minimal latents for the engine tests, the spatial fault models that prove them loud, and an fp16-activation emulation
of the oracle that says how much room the tolerance leaves (numpy / torch on the CPU, no HIP).

Shared by tests/test_geometry_cases_cpu.py (G1 .. G5 below, on the fp32 oracle) and tests/test_gpu_geometry_engines.py /
tests/test_gpu_geometry_pipelines.py (the HIP engines on the same weights and inputs against the same oracle).

Why.  Every other engine test runs the UNet and the ControlNet on a square latent.  The plan of csrc/unet.hip is built from H, W, H + 2,
W + 2 and H * W at every level; a place that uses H where it means W computes the same on every square input.  The fault models say so:

    pitch      a plane read with pitch H instead of W: out[y, x] = flat[(y * H + x) mod (H * W)] - the identity when H == W
    transpose  x.transpose(-1, -2).reshape(B, C, H, W): the plane filled in x-major order

applied at one site of the oracle's forward (``SpatialFaults``): the outputs of conv_in, conv_out and of every down- and upsampler conv,
the input of every transformer (its tokens gathered in the wrong order), the concatenated input of every up-path resnet; the inpaint
condition; a ControlNet's hint image, its hint embedding's output and every residual it hands to the UNet; under FreeU the (hidden,
skip) pair behind the filter; under regional prompts the region map of every attention level (the map reshaped, not the activations).

    G1  the gap: at 16 x 16 every pitch fault has effect exactly 0.
    G2  loudness: every site, both kinds: effect >= 4 T in one of the engine's non-square cases at t = 500 (condition A of
        tests/loud_cases.py: an honest engine lies within T, a faulty one at least 3 T away).
    G3  room: ``emulated(case, t)`` <= 0.6 T at every tested t for every case asserted at T.  The emulation (``Fp16Acts``: the result of
        every linear, conv, norm, resnet and transformer block rounded through fp16) is a predictor of an honest fp16 engine's distance
        from the oracle, not a reference.  At 16 x 16 the MI355X measured up to 1.4 x what it predicts (profiles/loud_weights/README.md),
        at the cases of this table up to 1.37 x (profiles/latent_geometry/README.md), so an honest engine is expected below 1.4 x 0.6 =
        0.84 T.  Not so ONE_TOKEN, tiny_xl at (2, 2): there the engine measured 1.67 x the emulation, and what speaks for its margin is
        the measurement itself (0.61 T), not this argument.
    G4  the inventory: the sites of a case are all the sites its config has.
    G5  the models themselves, on a hand-made 2 x 3 plane.

Weights are the project's synth weights (seed 0): the spatial faults are 40 T loud on them, and the loud weights leave too little room
at the smallest latents (emulation 2.0e-3 at (12, 4), 2.1e-3 at (4, 4); the loud ControlNet at (8, 24): 2.0e-3).  One exception, two
added ControlNet cases: on the synth weights a fault in the hint image or in the hint embedding's output moves the residuals by 0.0033
.. 0.0065 (1.3 .. 2.6 T) at every geometry and seed, and by at most 0.010 with the loudest hint a [0, 1] image can be (binary 8 x 8
blocks) - the embedding is a small addend of conv_in's output.  The weights "hint10" are the synth ControlNet with
controlnet_cond_embedding.conv_out x 10 and nothing else (the factor loud_cases.RECIPES gives that key, for that reason): 0.032 and
more, emulation 0.96e-3 .. 0.99e-3.  So for the ControlNet G2 holds at those two sites ONLY through the "hint10" cases, whose weights
are not the project's synth weights; on the synth ControlNet a pitch fault in the hint path is below 4 T and the engine tests
could miss it.

Rows as in loud_cases: ZR = 2 latent rows, 4 UNet rows, row r reads latent r % ZR; context at scale 0.5; SDXL time_ids with six
different values, different between the uc and the c rows.

tiny_xl at (2, 2) is there for the one-token attentions and the 1 x 1 GroupNorm, not for H / W faults.  Its output is 64 numbers per
row and its rel-L2 is not stable enough for T at every seed (emulation 0.9e-3 .. 4.9e-3 over the seeds 0 .. 29, within 0.6 T at all
three t for 9 of them): the seed in the table, 10, is the one of those with the most room (0.90e-3 .. 1.04e-3).  ``bound`` would give a
case named in RELAXED max(T, 2 x emulated) instead of T; RELAXED is empty.
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import replace

import torch

import loud_cases as L
from oracle.unet_ref import UNetRef

T = L.T_UNET
TS = L.TS
ZR = L.ZR
R = 2 * ZR
CN_SCALE = L.CN_SCALE
KINDS = ("pitch", "transpose")
ROOM = 0.6                          # G3: emulated <= ROOM * T
ENGINE_OVER_EMULATION = 1.4         # engine / emulation: the largest ratio measured at 16 x 16 (profiles/loud_weights/README.md); at
                                    # these cases 1.37 and less, but for ONE_TOKEN below: 1.67 (profiles/latent_geometry/README.md)
FREEU = (0.9, 0.2, 1.5, 1.6)        # tests/test_gpu_freeu_net.py
N_REGIONS = 3
# weights "hint10": the synth ControlNet with the last conv of its hint embedding x 10, the factor (and the reason) of loud_cases.RECIPES:
# the embedding is one small addend of conv_in's output, and with a hint in [0, 1] no geometry or seed lifts a fault in it over 4 T
HINT_KEY, HINT_GAIN = "controlnet_cond_embedding.conv_out.", 10.0

# engine: "unet" (cfg is the config's name), "controlnet" (on cfg), "freeu", "regions"
Case = namedtuple("Case", "engine cfg hw seed what weights", defaults=("synth",))

SQUARE = (Case("unet", "tiny_sd", (16, 16), 0, "G1: the shape of every other engine test"),
          Case("unet", "tiny_xl", (16, 16), 0, "G1"))
LOUD = (Case("unet", "tiny_sd", (8, 24), 0, "levels 8x24, 4x12, 2x6"),
        Case("unet", "tiny_sd", (20, 12), 0, "levels 20x12, 10x6, 5x3: 240, 60, 15 tokens, none a multiple of 64"),
        Case("unet", "tiny_xl", (6, 10), 0, "levels 6x10, 3x5"),
        Case("unet", "tiny_xl", (8, 24), 0, "levels 8x24, 4x12"),
        Case("unet", "tiny_sd2", (8, 12), 0, "linear projections, 64-wide heads"),
        Case("unet", "tiny_sd_inpaint", (8, 12), 0, "the 5-channel condition"),
        Case("unet", "tiny_sd_lcm", (12, 8), 0, "guidance-embedded"),
        Case("controlnet", "tiny_sd", (8, 24), 0, "hint 64 x 192"),
        Case("controlnet", "tiny_sd", (20, 12), 0, "hint 160 x 96"),
        Case("controlnet", "tiny_sd", (8, 24), 0, "hint 64 x 192, its embedding audible", "hint10"),
        Case("controlnet", "tiny_sd", (20, 12), 0, "hint 160 x 96, its embedding audible", "hint10"))
DEGENERATE = (Case("unet", "tiny_sd", (12, 4), 0, "bottom level 3x1"),
              Case("unet", "tiny_sd", (4, 12), 0, "bottom level 1x3"),
              Case("unet", "tiny_sd", (4, 4), 0, "bottom level 1x1; the top attention has 16 tokens"),
              Case("unet", "tiny_xl", (2, 6), 0, "bottom level 1x3"),
              Case("unet", "tiny_xl", (2, 2), 10, "bottom level 1x1; every attention has one token"),
              Case("controlnet", "tiny_sd", (12, 4), 0, "bottom level 3x1"))
# features that keep spatial state of their own, each at both tiny_sd geometries
FEATURES = tuple(Case(e, c, hw, 0, what) for e, c, what in (("freeu", "tiny_sd", "FreeU: twiddle tables and plane sums per level"),
                                                            ("regions", "tiny_sd", "regional prompts: a region map per attention level"),
                                                            ("unet", "tiny_sd_inpaint", "the inpaint condition through image_condition"))
                 for hw in ((8, 24), (20, 12)))
RELAXED = ()                        # cases whose bound is max(T, 2 x emulated) instead of T: none
ONE_TOKEN = next(c for c in DEGENERATE if c.cfg == "tiny_xl" and c.hw == (2, 2))


def case_id(c):
    name = c.cfg if c.engine == "unet" else f"{c.engine}-{c.cfg}"
    return f"{name}-{c.hw[0]}x{c.hw[1]}" + ("" if c.weights == "synth" else "-" + c.weights)


def all_cases():
    return LOUD + DEGENERATE + FEATURES


def unet_cases():
    return tuple(c for c in LOUD + DEGENERATE if c.engine == "unet")


def controlnet_cases():
    return tuple(c for c in LOUD + DEGENERATE if c.engine == "controlnet")


def engine_key(c):
    """the engine G2 groups the cases by: every site of it must be loud in one of its cases"""
    return (c.engine, c.cfg)


# ------------------------------------------------------------------------------------------------------------------ fault models
def _laid_out_like(x, values):
    """``values`` in x's own memory layout: the oracle then runs the same ATen kernels with and without the fault (a conv on a
    channels-last view and on a contiguous copy of it differ in the last bits), so a fault that moves nothing changes nothing"""
    return torch.empty_like(x).copy_(values)


def pitch(x):
    """[..., H, W] read with pitch H instead of W"""
    H, W = x.shape[-2:]
    y, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    idx = ((y * H + xx) % (H * W)).reshape(-1)
    return _laid_out_like(x, x.reshape(*x.shape[:-2], H * W)[..., idx].reshape(x.shape))


def transpose(x):
    """[..., H, W] filled in x-major order"""
    return _laid_out_like(x, x.transpose(-1, -2).reshape(x.shape))


MODELS = {"pitch": pitch, "transpose": transpose}
CONV_SITES = ("conv_in", "conv_out", "controlnet_cond_embedding.conv_out")
SAMPLER_CONVS = ("downsamplers.0.conv", "upsamplers.0.conv")


class _Sites(UNetRef):
    spatial = None              # (site, kind): the one fault of this forward
    seen = None                 # a list: the sites of a forward, in order

    def _site(self, site, x):
        if self.seen is not None and site not in self.seen:
            self.seen.append(site)
        if self.spatial is not None and self.spatial[0] == site:
            return MODELS[self.spatial[1]](x)
        return x


class SpatialFaults(_Sites):
    """a mixin over oracle.unet_ref.UNetRef and what derives from it (ControlNetRef, FreeUUNetRef, RegionUNetRef)"""

    def _conv(self, p, x, stride=1, pad=1):
        if p == "controlnet_cond_embedding.conv_in":
            x = self._site("hint image", x)
        y = super()._conv(p, x, stride, pad)
        if p in CONV_SITES or p.endswith(SAMPLER_CONVS):
            y = self._site(p, y)
        return y

    def _transformer(self, p, x, ctx, depth, heads):
        return super()._transformer(p, self._site(p + " tokens", x), ctx, depth, heads)

    def _resnet(self, p, x, emb):
        if p.startswith("up_blocks."):
            x = self._site(p + " concat", x)
        return super()._resnet(p, x, emb)

    def level_ids(self, N):     # RegionUNetRef: the level of N tokens is 4^level times smaller than the level-0 map
        level = (self.ids.shape[-2] * self.ids.shape[-1] // N).bit_length() // 2
        return self._site(f"region map of level {level}", super().level_ids(N))


class FreeUPairFaults(_Sites):
    """behind FreeUUNetRef in the method order: the (hidden, skip) pair after the filter"""

    def _resnet(self, p, x, emb):
        if self.freeu is not None and p.startswith(("up_blocks.0.resnets.", "up_blocks.1.resnets.")):
            x = self._site(p + " freeu pair", x)
        return super()._resnet(p, x, emb)


class Fp16Acts(UNetRef):
    """the oracle with the result of every linear, conv, norm, resnet and transformer block rounded through fp16"""

    def _lin(self, p, x):
        return super()._lin(p, x).half().float()

    def _conv(self, p, x, stride=1, pad=1):
        return super()._conv(p, x, stride, pad).half().float()

    def _gn(self, p, x, eps=1e-5):
        return super()._gn(p, x, eps).half().float()

    def _ln(self, p, x):
        return super()._ln(p, x).half().float()

    def _resnet(self, p, x, emb):
        return super()._resnet(p, x, emb).half().float()

    def _tblock(self, p, x, ctx, heads):
        return super()._tblock(p, x, ctx, heads).half().float()


_CLASSES = {}


def ref_class(kind, emulate=False):
    """the oracle class of ``kind`` ("unet", "controlnet", "freeu", "regions") with the spatial faults mixed in, and with ``emulate``
    the fp16 roundings in front of them"""
    if (kind, emulate) not in _CLASSES:
        if kind == "unet":
            bases = (SpatialFaults, UNetRef)
        elif kind == "controlnet":
            from controlnet_ref import ControlNetRef
            bases = (SpatialFaults, ControlNetRef)
        elif kind == "freeu":
            from freeu_ref import FreeUUNetRef
            bases = (SpatialFaults, FreeUUNetRef, FreeUPairFaults)
        elif kind == "regions":
            from region_ref import RegionUNetRef
            bases = (SpatialFaults, RegionUNetRef)
        else:
            raise ValueError(kind)
        _CLASSES[(kind, emulate)] = type(("Fp16" if emulate else "") + "Geo_" + kind, ((Fp16Acts,) if emulate else ()) + bases, {})
    return _CLASSES[(kind, emulate)]


def spatial_fault(site, kind):
    return L.Fault(kind, site, lambda sd, inputs: (sd, dict(inputs, spatial=(site, kind))))


def _model_of(inputs, site):
    """the fault model of ``inputs`` if it sits at ``site`` (the sites outside the oracle's forward), else None"""
    sp = inputs.get("spatial")
    return MODELS[sp[1]] if sp is not None and sp[0] == site else None


# ------------------------------------------------------------------------------------------------------------------ engines
class GeoUNet(L.UNetEngine):
    """loud_cases.UNetEngine at the case's (H, W) on the synth weights; ``kind`` chooses the oracle (plain, FreeU, regions)"""
    kind = "unet"

    def __init__(self, case):
        self.case, self.hw = case, tuple(case.hw)
        super().__init__(case.cfg, "synth", case.seed)

    def _weights(self, which):
        return L.synth_weights(which, 0)

    def setup(self):
        from cfgpp_amd.unet_config import CONFIGS
        self.cfg = cfg = CONFIGS[self.name]
        self.sd = self._weights(cfg)
        H, W = self.hw
        g = torch.Generator().manual_seed(1000 + self.seed)
        inp = {"z": torch.randn(ZR, 4, H, W, generator=g),
               "ehs": (torch.randn(R, 77, cfg.cross_attention_dim, generator=g) * 0.5).half().float()}
        if cfg.addition_embed:
            inp["te"] = (torch.randn(R, cfg.addition_pooled_dim, generator=g) * 0.5).half().float()
            # original size, crop top-left, target size: six different values, and different between the uc and the c rows
            inp["ti"] = torch.tensor([[128.0, 96.0, 8.0, 24.0, 112.0, 136.0]] * ZR + [[96.0, 128.0, 16.0, 0.0, 120.0, 104.0]] * ZR)
        if cfg.in_channels != cfg.out_channels:
            inp["cond"] = torch.cat([(torch.rand(ZR, 1, H, W, generator=g) < 0.5).float(), torch.randn(ZR, 4, H, W, generator=g)], 1).half().float()
        if cfg.time_cond_proj_dim:
            from cfgpp_amd.lcm import guidance_scale_embedding
            inp["w_emb"] = torch.tensor(guidance_scale_embedding(L.GUIDANCE, cfg.time_cond_proj_dim), dtype=torch.float64)
        self.more_inputs(inp)
        self.inputs = inp
        self.base_cfg = replace(cfg, time_cond_proj_dim=0)
        self._refs = {}

    def more_inputs(self, inp):
        pass

    def ref_args(self):
        return ()

    def ref(self, emulate=False):
        if emulate not in self._refs:
            self._refs[emulate] = ref_class(self.kind, emulate)(self.base_cfg, self.oracle_sd(self.sd, self.inputs), *self.ref_args())
        return self._refs[emulate]

    def outputs(self, sd, inputs, t):
        assert sd is self.sd, "the geometry cases fault the forward, not the weights"
        ref = self.ref(bool(inputs.get("emulate")))
        ref.spatial = inputs.get("spatial")
        fn = _model_of(inputs, "inpaint condition")
        if fn is not None:
            inputs = dict(inputs, cond=fn(inputs["cond"]))
        try:
            yield ref(self.sample(inputs), t, inputs["ehs"], self.ack(inputs))["sample"]
        finally:
            ref.spatial = None

    def sites(self):
        ref = self.ref()
        ref.seen = []
        try:
            ref(self.sample(self.inputs), 500.0, self.inputs["ehs"], self.ack(self.inputs))
            seen = ref.seen
        finally:
            ref.seen = None
        return seen + (["inpaint condition"] if "cond" in self.inputs else [])


class GeoFreeU(GeoUNet):
    kind = "freeu"

    def ref_args(self):
        return (FREEU,)


class GeoRegions(GeoUNet):
    """the right third of the map is the last region, the rest is split into horizontal bands of the others: under either fault model
    bands turn into stripes, at every level down to 2 x 6 and 5 x 3 (left / right stripes alone leave the deepest map's fault at 4.1 T,
    this map at 4.9 T and more - the mid block is a small share of eps).  The contexts are tests/region_ref.py's, loudly different per
    region."""
    kind = "regions"

    def more_inputs(self, inp):
        import region_ref as RR
        H, W = self.hw
        y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        inp["ids"] = torch.where(x >= 2 * W // 3, N_REGIONS - 1, y * (N_REGIONS - 1) // H)[None]
        inp["ehs"] = RR.region_context(R, N_REGIONS, self.cfg.cross_attention_dim)

    def ref_args(self):
        return (self.inputs["ids"], N_REGIONS)


class GeoControlNet(L.ControlNetEngine):
    """loud_cases.ControlNetEngine at the case's (H, W) with the hint at (8 H, 8 W), synth weights"""

    def __init__(self, case):
        self.case, self.hw = case, tuple(case.hw)
        super().__init__("controlnet", case.weights, case.seed)

    def _weights(self, which):
        sd = L.synth_weights(which, 0)
        if self.weights == "hint10" and isinstance(which, tuple):
            sd = {k: (v.float() * HINT_GAIN).half().float() if k.startswith(HINT_KEY) else v for k, v in sd.items()}
        return sd

    def setup(self):
        from cfgpp_amd.unet_config import CONFIGS
        self.cfg = cfg = CONFIGS[self.case.cfg]
        self.sd = self._weights(("controlnet", cfg))
        self.usd = self._weights(cfg)
        H, W = self.hw
        g = torch.Generator().manual_seed(2000 + self.seed)
        self.inputs = {"z": torch.randn(ZR, 4, H, W, generator=g),
                       "img": torch.rand(ZR, 3, 8 * H, 8 * W, generator=g),
                       "ehs": (torch.randn(R, 77, cfg.cross_attention_dim, generator=g) * self._ctx_scale("controlnet")).half().float()}
        self._refs = {}

    def ref(self, emulate=False):
        if emulate not in self._refs:
            unet = type("Fp16UNetRef", (Fp16Acts, UNetRef), {}) if emulate else UNetRef
            self._refs[emulate] = (ref_class("controlnet", emulate)(self.cfg, self.sd), unet(self.cfg, self.usd))
        return self._refs[emulate]

    def handoff_sites(self):
        return [f"{n} handed to the UNet" for n in self.output_names()[:-1]]

    def outputs(self, sd, inputs, t):
        from controlnet_ref import controlled_unet, image_rows
        assert sd is self.sd, "the geometry cases fault the forward, not the weights"
        cn, unet = self.ref(bool(inputs.get("emulate")))
        zz = inputs["z"][torch.arange(R) % ZR]
        cn.spatial = inputs.get("spatial")
        try:
            down, mid = cn(zz, t, inputs["ehs"], image_rows(inputs["img"], R, ZR), CN_SCALE, None)
        finally:
            cn.spatial = None
        for r in down:
            yield r
        yield mid
        res = list(down) + [mid]
        for i, site in enumerate(self.handoff_sites()):
            fn = _model_of(inputs, site)
            if fn is not None:
                res[i] = fn(res[i])
        yield controlled_unet(unet, zz, t, inputs["ehs"], None, res[:-1], res[-1])

    def sites(self):
        from controlnet_ref import image_rows
        cn, _ = self.ref()
        cn.seen = []
        try:
            cn(self.inputs["z"][torch.arange(R) % ZR], 500.0, self.inputs["ehs"], image_rows(self.inputs["img"], R, ZR), CN_SCALE, None)
            seen = cn.seen
        finally:
            cn.seen = None
        return seen + self.handoff_sites()


_ENGINES = {}
_CLS = {"unet": GeoUNet, "freeu": GeoFreeU, "regions": GeoRegions, "controlnet": GeoControlNet}


def engine(case):
    if case not in _ENGINES:
        _ENGINES[case] = _CLS[case.engine](case)
    return _ENGINES[case]


_SITES = {}


def sites(case):
    """the sites of the case's forward, in order (one recording forward, kept)"""
    if case not in _SITES:
        _SITES[case] = tuple(engine(case).sites())
    return _SITES[case]


def spatial_faults(case, kinds=KINDS):
    return [spatial_fault(s, k) for k in kinds for s in sites(case)]


def expected_sites(case):
    """the sites a case's config has, counted from the config and not from the mixin: {group: count}"""
    from cfgpp_amd.unet_config import CONFIGS
    cfg = CONFIGS[case.cfg]
    Lv, n, attn = cfg.num_levels, cfg.layers_per_block, cfg.level_has_attn
    control = case.engine == "controlnet"
    out = {"conv_in / conv_out": 1 if control else 2,
           "downsamplers": Lv - 1,
           "upsamplers": 0 if control else Lv - 1,
           "transformers": sum(attn) * n + 1 + (0 if control else sum(attn) * (n + 1)),
           "up-path concatenations": 0 if control else Lv * (n + 1)}
    if cfg.in_channels != cfg.out_channels:
        out["inpaint condition"] = 1
    if control:
        out["hint"] = 2                                       # the image, the embedding's output
        out["residuals handed over"] = Lv * n + Lv + 1        # conv_in, every resnet, every downsampler; the mid block
    if case.engine == "freeu":
        out["freeu pairs"] = 2 * (n + 1)
    if case.engine == "regions":
        out["region maps"] = len({lvl for lvl in range(Lv) if attn[lvl]} | {Lv - 1})
    return out


def site_group(site):
    if site.startswith("region map"):
        return "region maps"
    if site in ("conv_in", "conv_out"):
        return "conv_in / conv_out"
    if site.endswith("downsamplers.0.conv"):
        return "downsamplers"
    if site.endswith("upsamplers.0.conv"):
        return "upsamplers"
    if site.endswith(" tokens"):
        return "transformers"
    if site.endswith(" concat"):
        return "up-path concatenations"
    if site.endswith(" freeu pair"):
        return "freeu pairs"
    if site.endswith(" handed to the UNet"):
        return "residuals handed over"
    if site in ("hint image", "controlnet_cond_embedding.conv_out"):
        return "hint"
    return site


# ------------------------------------------------------------------------------------------------------------------ room and bounds
_EMULATED = {}


def emulated(case, t):
    """rel-L2 of the fp16-activation emulation against the fp32 oracle, the largest over the outputs the GPU test asserts on"""
    if (case, t) not in _EMULATED:
        e = engine(case)
        outs = e.outputs(e.sd, dict(e.inputs, emulate=True), t)
        _EMULATED[(case, t)] = max(L.rel_l2(o, b) for o, b in zip(outs, e.base(t)))
    return _EMULATED[(case, t)]


def bound(case, t):
    """the GPU test's bound on every output of ``case`` at ``t``: T; for a case of RELAXED max(T, 2 x emulated) - from the oracle
    alone, never from the engine"""
    return max(T, 2.0 * emulated(case, t)) if case in RELAXED else T


# ------------------------------------------------------------------------------------------------------------------ effects, explain
_CHANGES = {}


def change(case, site, kind, t=500.0):
    """the oracle's outputs with the fault ``kind`` at ``site`` minus its outputs without, one tensor per output (computed once)"""
    key = (case, site, kind, t)
    if key not in _CHANGES:
        _CHANGES[key] = engine(case).change(spatial_fault(site, kind), t)
    return _CHANGES[key]


def effect(case, site, kind, t=500.0):
    """rel-L2 of that change, the largest over the outputs the GPU test asserts on"""
    return max(float(d.norm() / (b.norm() + 1e-30)) for d, b in zip(change(case, site, kind, t), engine(case).base(t)))


def fault_table(case, t, kinds=KINDS):
    """[(label, flat oracle change)] of every spatial fault of ``case`` at ``t``: the table loud_cases.explain ranks"""
    return [(f"{k}: {s}", L.flat(change(case, s, k, t))) for k in kinds for s in sites(case)]


def suspects(case, t, got, top=3):
    """the ``top`` spatial faults whose oracle change is most collinear with the residual of ``got`` (the outputs in the engine's order)"""
    e = engine(case)
    res = [g.detach().float().cpu() - b for g, b in zip(got, e.base(t))]
    rows = L.explain(res, fault_table(case, t), top)
    return "; ".join(f"{label} (cos {c:+.2f}, |res|/|change| {r:.2g})" for label, c, r in rows)


def extremes(cases, kind, t=500.0):
    """over ``cases`` (one engine): the quietest and the loudest site of ``kind``, each site at the case where it is loudest"""
    best = {}
    for c in cases:
        for s in sites(c):
            best[s] = max(best.get(s, 0.0), effect(c, s, kind, t))
    r = sorted((v, n) for n, v in best.items())
    return {"sites": len(r), "min": [r[0][1], r[0][0]], "max": [r[-1][1], r[-1][0]]}


if __name__ == "__main__":      # PYTHONPATH=. python tests/geometry_cases.py: the CPU tables of profiles/latent_geometry/README.md
    print("| Latent | Sites | Largest `pitch` effect | `transpose` effect |\n|---|---|---|---|")
    for c in SQUARE:
        tr = [effect(c, s, "transpose") for s in sites(c)]
        print(f"| {case_id(c)} | {len(sites(c))} | {max(effect(c, s, 'pitch') for s in sites(c)):g} | {min(tr):.3f} .. {max(tr):.3f} |")
    groups = {}
    for c in LOUD + FEATURES:
        groups.setdefault(engine_key(c), []).append(c)
    print("\n| Engine | Kind | Sites | Quietest site | Loudest site |\n|---|---|---|---|---|")
    for key, cs in groups.items():
        for kind in KINDS:
            x = extremes(cs, kind)
            print(f"| {key[0]} {key[1]} | {kind} | {x['sites']} | {x['min'][0]}: {x['min'][1]:.3f} = {x['min'][1] / T:.0f} T | {x['max'][0]}: {x['max'][1]:.3f} |")
    print("\n| Case | For | Emulated at t = 500 | 981 | 1 | Bound |\n|---|---|---|---|---|---|")
    for c in all_cases():
        print(f"| {case_id(c)} | {c.what} | " + " | ".join(f"{emulated(c, t):.2e}" for t in TS) + f" | {max(bound(c, t) for t in TS):g} |")
