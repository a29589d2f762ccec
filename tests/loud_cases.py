"""Loud weights for the engine tests, the fault models that prove them loud, and ``explain`` (numpy / torch on the CPU, no HIP).

Shared by tests/test_loud_cases_cpu.py (conditions A and B below on the fp32 oracle, the silent keys, the recorded gap of the
synth weights) and tests/test_gpu_loud_engines.py (the HIP engines on the same weights and inputs against the same oracle).

Why.  The engine tests compare a whole output with the fp32 oracle at a tolerance T (2.5e-3 for a UNet / ControlNet forward, 1e-2
for a VAE pass).  With ``synth_state_dict`` / ``synth_vae_state_dict`` a large part of every net moves the output by less than T:
almost every bias and norm beta, and in the UNets whole cross-attentions (a softmax over 77 random tokens at scale 0.5 is nearly
flat).  An engine that lost, swapped or mis-laid-out such a parameter would still pass.  ``loud_state_dict`` rescales the same
seeded tensors (same keys, same shapes) until every parameter is audible:

    norm gamma 1 + 0.5 n, norm beta 0.5 n, every other bias x 15, to_q / to_k weights x 2 (tiny_xl, ControlNet: x 1.5; VAE: x 3), context drawn at scale 1.5,
    and per engine what RECIPES adds (the reasons stand there)

UNet and ControlNet weights are rounded through fp16 like the synth weights they come from (oracle and engine read the same bits);
the VAE's are not, like ``synth_vae_state_dict`` - there the engine's fp16 storage is part of what T covers (condition B).

Faults, applied to the oracle's copy of the state dict (``weight_faults``):
    drop       weights and biases -> 0, norm gammas -> 1
    swap       a key exchanged with its nearest sibling of the same shape: norm1 / norm2 (norm3 / norm2), to_k / to_v, to_q / to_out.0,
               conv1 / conv2, the resnets j / j + 1 of a level
    transpose  every square 2-D weight, every conv weight with O == I: O and I exchanged
    taps       every 3 x 3 conv weight with kh and kw reversed (`flip`) and with kh and kw exchanged (`khkw`): an OIHW repack into the
               wrong tap order
    halves     GEGLU ff.net.0.proj: value and gate halves of weight and bias exchanged
and to its inputs (``input_faults``): context / latent / text_embeds / hint rows permuted, t replaced by the neighbouring step of a
50-step schedule (20 apart), time_ids crop and size exchanged, the inpaint mask and masked-image channels exchanged, a ControlNet
residual added one skip off, the VAE's scaling_factor not applied, the moments' halves exchanged.

``effect`` is the rel-L2 of the oracle's output change, per output the GPU test asserts on (a UNet's eps; every ControlNet
residual and the controlled eps; the image; moments, z and the posterior mean), the largest of them: the GPU test asserts
``< T`` on each, so a fault is caught when one of them moves.

    Condition A: every fault has effect >= 4 T at one of the tested t.  An honest engine lies within T of the oracle, a faulty one at
                 least 4T - T = 3T away; the factor 3 is the allowance for the fault's effect in the fp16 engine differing from its
                 effect in the fp32 oracle.
    Condition B: the oracle with weights rounded to fp16 stays within T / 4 of the oracle with the weights as given.
    Silent keys: drop effect < 1e-5.  Exactly the VAE attentions' to_k.bias (it shifts every score of a row equally; softmax is
                 invariant): SILENT.

``explain`` ranks the faults of a table by how collinear their oracle change is with a HIP-minus-oracle residual.
"""
from __future__ import annotations

from collections import OrderedDict, namedtuple
from dataclasses import replace

import torch

T_UNET = 2.5e-3             # tests/test_gpu_unet.py, tests/test_gpu_controlnet.py: EPS_REL
T_VAE = 1e-2                # tests/test_gpu_vae.py
SILENT_BELOW = 1e-5
TS = (500.0, 981.0, 1.0)    # 500 first: the sweep tries the others only for what is not loud there
UNETS = ("tiny_sd", "tiny_xl", "tiny_sd2", "tiny_sd_inpaint", "tiny_sd_lcm")
ENGINES = UNETS + ("controlnet", "vae_dec", "vae_enc")
KINDS = ("drop", "swap", "transpose", "taps", "halves", "input")
HW = 16                     # UNet latents
ZR = 2                      # latent rows; UNet rows = 2 * ZR, row r reads latent r % ZR
VAE_HW = (8, 16)            # the smallest latent the VAE engine accepts (H * W = 128)
VAE_SCALE = 0.18215
CN_SCALE = 0.7
GUIDANCE = 8.5

# the only keys that may be silent, and why: Engine.silent_reason() checks the reason
SILENT = {"vae_dec": ("decoder.mid_block.attentions.0.to_k.bias",), "vae_enc": ("encoder.mid_block.attentions.0.to_k.bias",)}

# ``extra``: (substring of the key, factor) applied on top, to what the common rules leave below 4 T in that engine
Recipe = namedtuple("Recipe", "gamma beta bias qk ctx extra")
RECIPES = {
    # to_q / to_k x 2 with the context at 1.5 puts the cross-attention logits at std 8 (max 44): peaked enough to be heard,
    # and the oracle with every activation rounded through fp16 stays at 1.2e-3 of the fp32 oracle (synth weights: 8e-4).
    # (x 3 gave logits of std 17, max 99, and an fp16 engine cannot hold that: 7e-3 on the MI355X.)  The deepest level is a small
    # share of eps next to the skips: x 4 on the upsampler conv that carries it up makes the mid block and its neighbours loud;
    # the feed-forward biases (one addend among 8 c / c channels) x 2, conv1.bias and time_emb_proj.bias (two addends of one sum) x 1.5.
    "unet": Recipe(gamma=0.5, beta=0.5, bias=15.0, qk=2.0, ctx=1.5,
                   extra=(("up_blocks.0.upsamplers.0.conv.weight", 4.0), (".ff.net.0.proj.bias", 2.0), (".ff.net.2.bias", 2.0),
                          (".conv1.bias", 1.5), (".time_emb_proj.bias", 1.5))),
    # tiny_xl runs two transformer blocks per attention: at x 2 its fp16-activation emulation stands at 1.9e-3 and the HIP engine
    # measured 2.74e-3 > T; at x 1.5 the emulation gives 1.2e-3
    "tiny_xl": Recipe(gamma=0.5, beta=0.5, bias=15.0, qk=1.5, ctx=1.5,
                      extra=(("up_blocks.0.upsamplers.0.conv.weight", 4.0), (".ff.net.0.proj.bias", 2.0), (".ff.net.2.bias", 2.0),
                             (".conv1.bias", 1.5), (".time_emb_proj.bias", 1.5))),
    # the hint's embedding enters as one addend of conv_in's output: x 10 at its last conv lifts the whole stack
    "controlnet": Recipe(gamma=0.5, beta=0.5, bias=15.0, qk=1.5, ctx=1.5,
                         extra=(("controlnet_cond_embedding.conv_out.", 10.0), ("controlnet_cond_embedding.conv_in.bias", 3.0), (".ff.net.0.proj.bias", 2.0), (".ff.net.2.bias", 2.0),
                                (".conv1.bias", 1.5), (".time_emb_proj.bias", 1.5))),
    # The VAE's residual stream is never normalised between resnets, so it grows and a late resnet's branch is a small share of
    # it: the stream is damped where it is born (decoder.conv_in) and at every upsampler conv, which makes every branch behind
    # them louder at once (making biases louder instead only moves the quiet spot: they drown the gammas).  conv2.bias of
    # neighbouring resnets add into the same stream, so exchanging two shows only through the resnet between them: x 1.25.
    # to_q.bias: x 2 (512 channels into one softmax over 128 tokens).
    "vae": Recipe(gamma=0.5, beta=0.5, bias=15.0, qk=3.0, ctx=None,
                  extra=(("upsamplers.0.conv.weight", 0.5), ("decoder.conv_in.weight", 0.3), (".conv2.bias", 1.25), (".to_q.bias", 2.0))),
}
Fault = namedtuple("Fault", "kind name apply")      # apply(sd, inputs) -> (sd, inputs), fresh shallow copies


# ------------------------------------------------------------------------------------------------------------------ weights
def is_norm(key):
    return "norm" in key


def loudify(sd, recipe, round_fp16):
    """the loud version of a synth state dict: norm gamma 1 + 0.1 n -> 1 + gamma n, beta 0.05 n -> beta n, bias 0.02 n -> bias * 0.02 n"""
    out = OrderedDict()
    for k, v in sd.items():
        v = v.float()
        leaf = k.rsplit(".", 1)[-1]
        if is_norm(k):
            v = 1.0 + (v - 1.0) * (recipe.gamma / 0.1) if leaf == "weight" else v * (recipe.beta / 0.05)
        elif leaf == "bias":
            v = v * recipe.bias
        elif ".to_q." in k or ".to_k." in k:
            v = v * recipe.qk
        for part, factor in recipe.extra:
            if part in k:
                v = v * factor
        out[k] = v.half().float() if round_fp16 else v
    return out


def synth_weights(which, seed=0):
    """the project's synth weights of ``which``: a UNetConfig, "vae", or ("controlnet", cfg)"""
    if which == "vae":
        from cfgpp_amd.vae import synth_vae_state_dict
        return synth_vae_state_dict(seed)
    if isinstance(which, tuple):
        from cfgpp_amd.controlnet import synth_controlnet_state_dict
        return synth_controlnet_state_dict(which[1], seed)
    from cfgpp_amd.weights import synth_state_dict
    return synth_state_dict(which, seed)


def loud_state_dict(which, seed=0):
    """``which``: a UNetConfig, "vae", or ("controlnet", cfg) - the synth weights of the same seed, rescaled (RECIPES)"""
    sd = synth_weights(which, seed)
    if which == "vae":
        return loudify(sd, RECIPES["vae"], round_fp16=False)
    recipe = RECIPES["controlnet"] if isinstance(which, tuple) else RECIPES.get(which.name, RECIPES["unet"])
    return loudify(sd, recipe, round_fp16=True)


# ------------------------------------------------------------------------------------------------------------------ weight faults
def _with(sd, **changes):
    out = dict(sd)
    out.update(changes)
    return out


def _on_sd(fn):
    return lambda sd, inputs: (fn(sd), inputs)


def drop_value(key, v):
    return torch.ones_like(v) if (is_norm(key) and key.endswith(".weight")) else torch.zeros_like(v)


_SIBLINGS = ((".norm1.", ".norm2."), (".norm3.", ".norm2."), (".to_k.", ".to_v."), (".to_q.", ".to_out.0."), (".conv1.", ".conv2."))


def swap_pairs(sd, keys):
    """unordered pairs (a, b) of ``keys`` to exchange: the name siblings above, and resnets.j / resnets.j+1 of one block"""
    pairs = []
    for k in keys:
        for a, b in _SIBLINGS:
            if a in k:
                o = k.replace(a, b)
                if o in sd and sd[o].shape == sd[k].shape:
                    pairs.append((k, o))
        if ".resnets." in k:
            head, rest = k.split(".resnets.", 1)
            j, tail = rest.split(".", 1)
            o = f"{head}.resnets.{int(j) + 1}.{tail}"
            if o in sd and sd[o].shape == sd[k].shape:
                pairs.append((k, o))
    return pairs


def weight_faults(sd, keys, kind):
    """the faults of ``kind`` on ``keys`` of ``sd``"""
    out = []
    if kind == "drop":
        for k in keys:
            out.append(Fault(kind, k, _on_sd(lambda s, k=k: _with(s, **{k: drop_value(k, s[k])}))))
    elif kind == "swap":
        for a, b in swap_pairs(sd, keys):
            out.append(Fault(kind, f"{a} <-> {b}", _on_sd(lambda s, a=a, b=b: _with(s, **{a: s[b], b: s[a]}))))
    elif kind == "transpose":
        for k in keys:
            v = sd[k]
            if k.endswith(".weight") and v.dim() in (2, 4) and v.shape[0] == v.shape[1]:
                out.append(Fault(kind, k, _on_sd(lambda s, k=k: _with(s, **{k: s[k].transpose(0, 1).contiguous()}))))
    elif kind == "taps":
        for k in keys:
            v = sd[k]
            if v.dim() == 4 and tuple(v.shape[2:]) == (3, 3):
                out.append(Fault(kind, k + " flip", _on_sd(lambda s, k=k: _with(s, **{k: s[k].flip(2, 3).contiguous()}))))
                out.append(Fault(kind, k + " khkw", _on_sd(lambda s, k=k: _with(s, **{k: s[k].transpose(2, 3).contiguous()}))))
    elif kind == "halves":
        for k in keys:
            if k.endswith(".ff.net.0.proj.weight"):
                b = k[:-len("weight")] + "bias"

                def fn(s, k=k, b=b):
                    return _with(s, **{k: torch.cat(s[k].chunk(2, 0)[::-1], 0), b: torch.cat(s[b].chunk(2, 0)[::-1], 0)})
                out.append(Fault(kind, k, _on_sd(fn)))
    else:
        raise ValueError(kind)
    return out


def _on_inputs(**fns):
    def apply(sd, inputs):
        new = dict(inputs)
        for name, fn in fns.items():
            new[name] = fn(inputs[name])
        return sd, new
    return apply


def _swap_halves(x):
    h = x.shape[0] // 2
    return torch.cat([x[h:], x[:h]])


def rel_l2(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def neighbour_t(t):
    """the next timestep of a 50-step schedule (1, 21, ..., 981)"""
    return t - 20.0 if t > 20.0 else t + 20.0


# ------------------------------------------------------------------------------------------------------------------ engines
class Engine:
    """one engine / config of the table: its weights (``weights`` = "loud" or "synth"), inputs, oracle and faults.
    ``outputs(sd, inputs, t)`` yields the tensors the GPU test compares, in its order."""

    T = T_UNET
    ts = TS

    def __init__(self, name, weights="loud", seed=0):
        self.name, self.weights, self.seed = name, weights, seed
        self._base = {}
        self.setup()
        self.keys = list(self.sd)

    # -- to be provided ---------------------------------------------------------------------------------------------------
    def setup(self):
        raise NotImplementedError

    def outputs(self, sd, inputs, t):
        raise NotImplementedError

    def input_faults(self):
        return []

    def output_names(self):
        return ["out"]

    # -- shared --------------------------------------------------------------------------------------------------------------
    def _weights(self, which):
        return loud_state_dict(which, self.seed) if self.weights == "loud" else synth_weights(which, self.seed)

    def _ctx_scale(self, recipe="unet"):
        return RECIPES[recipe].ctx if self.weights == "loud" else 0.5

    def base(self, t):
        if t not in self._base:
            self._base[t] = list(self.outputs(self.sd, self.inputs, t))
        return self._base[t]

    def faults(self, kind):
        return self.input_faults() if kind == "input" else weight_faults(self.sd, self.keys, kind)

    def change(self, fault, t):
        """the oracle's outputs under ``fault`` minus its outputs without, one tensor per output"""
        sd, inputs = fault.apply(self.sd, self.inputs)
        return [o - b for o, b in zip(self.outputs(sd, inputs, t), self.base(t))]

    def effect(self, fault, t, stop_at=None):
        """max over the outputs of rel-L2(change); with ``stop_at`` the later (more expensive) outputs are not computed once one
        output has reached it"""
        sd, inputs = fault.apply(self.sd, self.inputs)
        worst = 0.0
        for o, b in zip(self.outputs(sd, inputs, t), self.base(t)):
            worst = max(worst, rel_l2(o, b))
            if stop_at is not None and worst >= stop_at:
                break
        return worst

    def loudest(self, fault, stop_at=None):
        """max over the tested t of ``effect``, trying t = 500 first and the others only while below ``stop_at``"""
        worst = 0.0
        for t in self.ts:
            worst = max(worst, self.effect(fault, t, stop_at))
            if stop_at is not None and worst >= stop_at:
                break
        return worst

    def rounding_effect(self, t):
        """condition B: the oracle on fp16-rounded weights against the oracle on the weights as given"""
        sd16 = {k: v.half().float() for k, v in self.sd.items()}
        return max(rel_l2(o, b) for o, b in zip(self.outputs(sd16, self.inputs, t), self.base(t)))

    def silent_reason(self, key, t):
        """the reason a to_k.bias may be silent: adding one constant to all of it changes nothing.  (Any vector added to to_k.bias
        shifts a row's scores by q . b, equally for every key; a constant is the instance checked.)"""
        sd = _with(self.sd, **{key: self.sd[key] + 0.5})
        return max(rel_l2(o, b) for o, b in zip(self.outputs(sd, self.inputs, t), self.base(t)))


class UNetEngine(Engine):
    def setup(self):
        from cfgpp_amd.unet_config import CONFIGS
        self.cfg = cfg = CONFIGS[self.name]
        self.sd = self._weights(cfg)
        R = 2 * ZR
        g = torch.Generator().manual_seed(1000 + self.seed)
        inp = {"z": torch.randn(ZR, 4, HW, HW, generator=g),
               "ehs": (torch.randn(R, 77, cfg.cross_attention_dim, generator=g) * self._ctx_scale()).half().float()}
        if cfg.addition_embed:
            inp["te"] = (torch.randn(R, cfg.addition_pooled_dim, generator=g) * 0.5).half().float()
            # original size, crop top-left, target size: all different, and different between the uc and the c rows
            inp["ti"] = torch.tensor([[128.0, 96.0, 8.0, 24.0, 112.0, 128.0]] * ZR + [[96.0, 128.0, 16.0, 0.0, 128.0, 104.0]] * ZR)
        if cfg.in_channels != cfg.out_channels:       # inpaint: mask (1) then the masked image's latent (4), diffusers' order
            inp["cond"] = torch.cat([(torch.rand(ZR, 1, HW, HW, generator=g) < 0.5).float(), torch.randn(ZR, 4, HW, HW, generator=g)], 1).half().float()
        if cfg.time_cond_proj_dim:
            from cfgpp_amd.lcm import guidance_scale_embedding
            inp["w_emb"] = torch.tensor(guidance_scale_embedding(GUIDANCE, cfg.time_cond_proj_dim), dtype=torch.float64)
        self.inputs = inp
        self.base_cfg = replace(cfg, time_cond_proj_dim=0)
        self._ref = None

    def oracle_sd(self, sd, inputs):
        """a guidance-embedded UNet as the plain UNet that computes the same: linear_1(sinusoid + cond_proj w) = W1 sinusoid +
        (b1 + W1 cond_proj w), exact by linearity (tests/test_gpu_lcm_net.py)"""
        if not self.cfg.time_cond_proj_dim:
            return sd
        out = {k: v for k, v in sd.items() if k != "time_embedding.cond_proj.weight"}
        w1, wc = sd["time_embedding.linear_1.weight"].double(), sd["time_embedding.cond_proj.weight"].double()
        out["time_embedding.linear_1.bias"] = (sd["time_embedding.linear_1.bias"].double() + w1 @ (wc @ inputs["w_emb"])).float()
        return out

    def sample(self, inputs):
        rows = torch.arange(2 * ZR) % ZR
        x = inputs["z"][rows]
        if "cond" in inputs:
            x = torch.cat([x, inputs["cond"][rows]], 1)
        return x

    def ack(self, inputs):
        return {"text_embeds": inputs["te"], "time_ids": inputs["ti"]} if "te" in inputs else None

    def outputs(self, sd, inputs, t):
        from oracle.unet_ref import UNetRef
        if sd is self.sd and inputs.get("w_emb") is self.inputs.get("w_emb"):     # input faults: the oracle of the unchanged weights
            if self._ref is None:
                self._ref = UNetRef(self.base_cfg, self.oracle_sd(sd, inputs))
            ref = self._ref
        else:
            ref = UNetRef(self.base_cfg, self.oracle_sd(sd, inputs))
        yield ref(self.sample(inputs), _t_of(inputs, t), inputs["ehs"], self.ack(inputs))["sample"]

    def input_faults(self):
        f = [Fault("input", "context rows: uc / c exchanged", _on_inputs(ehs=_swap_halves)),
             Fault("input", "context rows: neighbours exchanged", _on_inputs(ehs=lambda x: x[[1, 0, 3, 2]])),
             Fault("input", "latent rows exchanged", _on_inputs(z=lambda x: x.flip(0))),
             Fault("input", "t of the neighbouring step", lambda sd, inputs: (sd, dict(inputs, t_shift=True)))]
        if "te" in self.inputs:
            f += [Fault("input", "text_embeds rows: uc / c exchanged", _on_inputs(te=_swap_halves)),
                  Fault("input", "time_ids rows: uc / c exchanged", _on_inputs(ti=_swap_halves)),
                  Fault("input", "time_ids: crop and original size exchanged", _on_inputs(ti=lambda x: x[:, [2, 3, 0, 1, 4, 5]]))]
        if "cond" in self.inputs:
            f += [Fault("input", "mask and masked-image channels exchanged", _on_inputs(cond=lambda x: torch.cat([x[:, 1:], x[:, :1]], 1))),
                  Fault("input", "condition rows exchanged", _on_inputs(cond=lambda x: x.flip(0)))]
        if "w_emb" in self.inputs:
            from cfgpp_amd.lcm import guidance_scale_embedding
            other = torch.tensor(guidance_scale_embedding(GUIDANCE - 0.5, self.cfg.time_cond_proj_dim), dtype=torch.float64)
            f.append(Fault("input", "guidance embedding of another scale", _on_inputs(w_emb=lambda x: other)))
        return f


def _t_of(inputs, t):
    """the `t of the neighbouring step` fault marks the inputs; the oracle is then called at that t"""
    return neighbour_t(t) if inputs.get("t_shift") else t


class ControlNetEngine(Engine):
    """the tiny ControlNet of tests/controlnet_ref.py on tiny_sd: the faults are on the ControlNet's state dict; the controlled
    UNet (loud weights too) is the last output"""

    def setup(self):
        from cfgpp_amd.unet_config import CONFIGS
        self.cfg = cfg = CONFIGS["tiny_sd"]
        self.sd = self._weights(("controlnet", cfg))
        self.usd = self._weights(cfg)
        R = 2 * ZR
        g = torch.Generator().manual_seed(2000 + self.seed)
        self.inputs = {"z": torch.randn(ZR, 4, HW, HW, generator=g),
                       "img": torch.rand(ZR, 3, 8 * HW, 8 * HW, generator=g),
                       "ehs": (torch.randn(R, 77, cfg.cross_attention_dim, generator=g) * self._ctx_scale("controlnet")).half().float()}
        self._unet = None

    def output_names(self):
        from cfgpp_amd.controlnet import num_down_residuals
        n = num_down_residuals(self.cfg)
        return [f"residual {i}" for i in range(n)] + ["mid residual", "controlled eps"]

    def outputs(self, sd, inputs, t):
        from controlnet_ref import ControlNetRef, controlled_unet, image_rows
        from oracle.unet_ref import UNetRef
        t = _t_of(inputs, t)
        R = 2 * ZR
        zz = inputs["z"][torch.arange(R) % ZR]
        down, mid = ControlNetRef(self.cfg, sd)(zz, t, inputs["ehs"], image_rows(inputs["img"], R, ZR), CN_SCALE, None)
        for r in down:
            yield r
        yield mid
        if self._unet is None:
            self._unet = UNetRef(self.cfg, self.usd)
        down = list(down)
        shift = inputs.get("residual_shift")
        if shift:
            i, j = shift
            down[j] = down[j] + down[i]
            down[i] = torch.zeros_like(down[i])
        yield controlled_unet(self._unet, zz, t, inputs["ehs"], None, down, mid)

    def residual_shifts(self):
        """(i, j = i +/- 1) where residual i fits skip j"""
        from cfgpp_amd.controlnet import _skip_channels
        ch = _skip_channels(self.cfg)
        hw = [HW]
        for i in range(self.cfg.num_levels):
            hw += [hw[-1]] * self.cfg.layers_per_block
            if i != self.cfg.num_levels - 1:
                hw.append(hw[-1] // 2)
        out = []
        for i in range(len(ch)):
            for j in (i - 1, i + 1):
                if 0 <= j < len(ch) and ch[i] == ch[j] and hw[i] == hw[j]:
                    out.append((i, j))
        return out

    def input_faults(self):
        f = [Fault("input", "context rows: uc / c exchanged", _on_inputs(ehs=_swap_halves)),
             Fault("input", "latent rows exchanged", _on_inputs(z=lambda x: x.flip(0))),
             Fault("input", "hint rows exchanged", _on_inputs(img=lambda x: x.flip(0))),
             Fault("input", "t of the neighbouring step", lambda sd, inputs: (sd, dict(inputs, t_shift=True)))]
        for i, j in self.residual_shifts():
            f.append(Fault("input", f"residual {i} added at skip {j}", lambda sd, inputs, ij=(i, j): (sd, dict(inputs, residual_shift=ij))))
        return f


class VAEEngine(Engine):
    T = T_VAE
    ts = (None,)

    def setup(self):
        full = self._weights("vae")
        dec = self.name == "vae_dec"
        self.full_sd = full
        self.sd = OrderedDict((k, v) for k, v in full.items() if k.startswith(("decoder.", "post_quant_conv.")) == dec)
        g = torch.Generator().manual_seed(3000 + self.seed)
        h, w = VAE_HW
        if dec:
            self.inputs = {"z": torch.randn(1, 4, h, w, generator=g) * VAE_SCALE * 1.5, "scale": VAE_SCALE}
        else:
            self.inputs = {"img": torch.rand(1, 3, 8 * h, 8 * w, generator=g) * 2 - 1, "noise": torch.randn(1, 4, h, w, generator=g), "halves": False}

    def output_names(self):
        return ["image"] if self.name == "vae_dec" else ["moments", "z", "posterior mean"]

    def outputs(self, sd, inputs, t):
        from oracle.vae_ref import VAERef
        ref = VAERef(VAE_SCALE, device="cpu", dtype=torch.float32, state_dict=sd)
        if self.name == "vae_dec":
            yield ref.decode_raw(inputs["z"] / inputs["scale"]).float()
            return
        mean, logvar = ref.encode_moments(inputs["img"])
        if inputs["halves"]:
            mean, logvar = logvar, mean
        yield torch.cat([mean, logvar], 1)
        yield (mean + torch.exp(0.5 * logvar) * inputs["noise"]) * VAE_SCALE
        yield mean * VAE_SCALE

    def input_faults(self):
        if self.name == "vae_dec":
            return [Fault("input", "scaling_factor not applied", _on_inputs(scale=lambda s: 1.0))]
        return [Fault("input", "mean / logvar halves exchanged", _on_inputs(halves=lambda s: True))]


_CACHE = {}


def engine(name, weights="loud", seed=0):
    """the (cached) Engine of ``name`` in ENGINES"""
    key = (name, weights, seed)
    if key not in _CACHE:
        cls = UNetEngine if name in UNETS else ControlNetEngine if name == "controlnet" else VAEEngine
        _CACHE[key] = cls(name, weights, seed)
    return _CACHE[key]


def effect(name, fault, t=None, weights="loud"):
    """rel-L2 of the oracle's output change under ``fault`` (the largest over the tested t when ``t`` is None)"""
    e = engine(name, weights)
    return e.loudest(fault) if (t is None and e.ts != (None,)) else e.effect(fault, t)


def sweep(name, kind, weights="loud", stop_at=None, all_t=True):
    """[(fault name, effect)] for every fault of ``kind``; with ``all_t`` the largest over the tested t (each fault goes to the next t
    only while below ``stop_at``), otherwise at t = 500 alone"""
    e = engine(name, weights)
    return [(f.name, e.loudest(f, stop_at) if all_t else e.effect(f, e.ts[0], stop_at)) for f in e.faults(kind)]


# ------------------------------------------------------------------------------------------------------------------ explain
def flat(tensors):
    return torch.cat([x.detach().double().cpu().reshape(-1) for x in tensors])


def change_table(name, t, kinds=("drop", "input"), weights="loud"):
    """[(label, flat oracle change)] of every fault of ``kinds`` at ``t``: the table ``explain`` ranks"""
    e = engine(name, weights)
    return [(f"{f.kind}: {f.name}", flat(e.change(f, t))) for k in kinds for f in e.faults(k)]


def explain(residual, table, top=3):
    """the ``top`` faults of ``table`` whose oracle change is most collinear with ``residual`` (HIP minus oracle; a tensor or a list
    of tensors in the table's layout): [(label, cosine, |residual| / |change|)], largest |cosine| first.  A norm ratio near 1 with
    a cosine near 1 names the fault; a cosine near -1 with ratio 1 means the engine did what the fault UNdoes."""
    r = flat(residual if isinstance(residual, (list, tuple)) else [residual])
    rn = float(r.norm()) + 1e-300
    rows = []
    for label, d in table:
        dn = float(d.norm())
        if d.numel() != r.numel():
            raise ValueError(f"explain: the residual has {r.numel()} elements, the change of `{label}` {d.numel()}: another layout")
        if dn == 0.0:
            continue
        rows.append((label, float(r @ d) / (rn * dn), rn / dn))
    rows.sort(key=lambda x: -abs(x[1]))
    return rows[:top]


# ------------------------------------------------------------------------------------------------------------------ records
def quiet_count(name, kind):
    """the gap the loud weights close: how many faults of ``kind`` the SYNTH weights leave below T and below 4 T (t = 500)"""
    e = engine(name, "synth")
    r = sweep(name, kind, "synth", stop_at=4 * e.T, all_t=False)
    return {"faults": len(r), "below_T": sum(v < e.T for _, v in r), "below_4T": sum(v < 4 * e.T for _, v in r)} if r else None


def quiet_counts(name):
    out = {"keys": len(engine(name, "synth").keys)}
    for kind in KINDS:
        c = quiet_count(name, kind)
        if c:
            out[kind] = c
    return out


def loud_extremes(name):
    """per fault kind the quietest and the loudest fault of the LOUD weights (largest over the tested t), silent keys apart"""
    e = engine(name)
    out = {}
    for kind in KINDS:
        r = sorted((v, n) for n, v in sweep(name, kind) if n not in SILENT.get(name, ()))
        if r:
            out[kind] = {"faults": len(r), "min": [r[0][1], r[0][0]], "max": [r[-1][1], r[-1][0]]}
    return out


if __name__ == "__main__":      # python tests/loud_cases.py: rewrite profiles/loud_weights/quiet_keys.json
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    d = os.path.join(root, "profiles", "loud_weights")
    os.makedirs(d, exist_ok=True)
    quiet = {"what": "faults of the synth weights whose oracle effect is below T / below 4 T at t = 500 (tests/loud_cases.py: quiet_counts)",
             "T": {n: engine(n, "synth").T for n in ENGINES}, "engines": {n: quiet_counts(n) for n in ENGINES}}
    with open(os.path.join(d, "quiet_keys.json"), "w") as f:
        json.dump(quiet, f, indent=1)
        f.write("\n")
