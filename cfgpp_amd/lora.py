"""LoRA adapters for the UNet: parsing of the published file layouts into ``{unet weight key: (up, down, alpha)}`` and the
bookkeeping that turns a list of ``(adapter, scale)`` into ONE device merge per touched weight
(include/cfgpp.h: cfgpp_unet_lora - ``W = fp16(base + up @ down)`` written into the repacked weights the kernels read).

Accepted namings, all resolved against ``unet_config.param_shapes(cfg)``:

* PEFT / diffusers      ``[unet.]<module>.lora_A.weight`` (down) / ``lora_B.weight`` (up)
* older diffusers       ``<module>.lora.down.weight`` / ``lora.up.weight``, and the attention-processor form
                        ``<attn>.processor.to_q_lora.down.weight``
* kohya                 ``lora_unet_<module path with "_" for ".">.lora_down.weight`` / ``.lora_up.weight`` / ``.alpha`` where
                        the module path is the diffusers one

Everything else is refused with an error that names the key - never skipped: the SGM block naming
(``lora_unet_input_blocks_...``), LoHa / LoKr factors, DoRA magnitudes, modules the UNet does not have, and text-encoder
entries unless the caller passes ``ignore_text_encoder=True`` (the text encoders take no adapter here).
"""
from __future__ import annotations

import re
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch

from .unet_config import UNetConfig, param_shapes


class LoraError(ValueError):
    pass


class ParsedLora(dict):
    """``{unet weight key: (up [O, r] fp32, down [r, I*kh*kw] fp32, alpha or None)}``; ``report`` lists what was set aside
    on request (``ignore_text_encoder=True``: the text-encoder keys)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.report: Dict[str, List[str]] = {"ignored_text_encoder": []}


_TE_PREFIXES = ("lora_te", "text_encoder", "te1_", "te2_")
_SGM = re.compile(r"^lora_unet_(input_blocks|middle_block|output_blocks|time_embed|label_emb|out)_")
# (suffix pattern, role) tried in order on the key with its "unet." prefix removed
_SUFFIXES = (
    (re.compile(r"^(?P<m>.+)\.lora_A(\.[A-Za-z0-9_]+)?\.weight$"), "down"),
    (re.compile(r"^(?P<m>.+)\.lora_B(\.[A-Za-z0-9_]+)?\.weight$"), "up"),
    (re.compile(r"^(?P<m>.+)\.processor\.(?P<p>to_q|to_k|to_v|to_out)_lora\.(?P<r>down|up)\.weight$"), None),
    (re.compile(r"^(?P<m>.+)\.lora\.(?P<r>down|up)\.weight$"), None),
    (re.compile(r"^(?P<m>.+)\.lora_linear_layer\.(?P<r>down|up)\.weight$"), None),
    (re.compile(r"^(?P<m>.+)\.lora_(?P<r>down|up)\.weight$"), None),
    (re.compile(r"^(?P<m>.+)\.alpha$"), "alpha"),
)


def _load(src) -> Dict[str, torch.Tensor]:
    if isinstance(src, dict):
        return src
    from .weights import load_safetensors_iter
    return dict(load_safetensors_iter(str(src)))


def _modules(cfg: UNetConfig) -> Dict[str, tuple]:
    """module name -> weight shape, for every matrix parameter of the UNet"""
    return {k[: -len(".weight")]: s for k, s in param_shapes(cfg).items() if k.endswith(".weight") and len(s) in (2, 4)}


def parse_lora(src, cfg: UNetConfig, ignore_text_encoder: bool = False) -> ParsedLora:
    """``src``: a state dict or the path of a safetensors file.  See the module docstring for what is accepted."""
    sd = _load(src)
    mods = _modules(cfg)
    under = {m.replace(".", "_"): m for m in mods}
    parts: Dict[str, dict] = {}
    out = ParsedLora()
    for key in sd:
        low = key.lower()
        if any(key.startswith(p) for p in _TE_PREFIXES):
            if not ignore_text_encoder:
                raise LoraError(f"LoRA key {key}: text-encoder adapters are not supported (pass ignore_text_encoder=True to apply "
                                "the UNet part only)")
            out.report["ignored_text_encoder"].append(key)
            continue
        if "hada_" in low or "lokr_" in low:
            raise LoraError(f"LoRA key {key}: LoHa / LoKr factors are not supported (plain low-rank up / down only)")
        if "dora_scale" in low or "lora_magnitude_vector" in low:
            raise LoraError(f"LoRA key {key}: DoRA magnitudes are not supported")
        if _SGM.match(key):
            raise LoraError(f"LoRA key {key}: SGM block naming (input_blocks / middle_block / output_blocks) is not supported; "
                            "convert the file to the diffusers module names")
        k = key[len("unet."):] if key.startswith("unet.") else key
        role = mod = None
        for pat, r in _SUFFIXES:
            m = pat.match(k)
            if m:
                gd = m.groupdict()
                role = r or gd["r"]
                mod = gd["m"]
                if gd.get("p"):
                    mod += "." + ("to_out.0" if gd["p"] == "to_out" else gd["p"])
                break
        if role is None:
            raise LoraError(f"LoRA key {key}: not a LoRA tensor name this loader knows")
        if mod.startswith("lora_unet_"):
            u = mod[len("lora_unet_"):]
            if u not in under:
                raise LoraError(f"LoRA key {key}: no UNet module matches '{u}' (config {cfg.name})")
            mod = under[u]
        elif mod not in mods:
            raise LoraError(f"LoRA key {key}: the UNet has no matrix '{mod}.weight' (config {cfg.name})")
        parts.setdefault(mod, {})[role] = (key, sd[key])
    for mod, p in parts.items():
        wkey = mod + ".weight"
        if "up" not in p or "down" not in p:
            have = ", ".join(v[0] for v in p.values())
            raise LoraError(f"LoRA adapter for {wkey} is incomplete (found only: {have})")
        up, down = p["up"][1].detach().float().cpu(), p["down"][1].detach().float().cpu()
        shape = mods[mod]
        O, K = int(shape[0]), 1
        for d in shape[1:]:
            K *= int(d)
        r = int(down.shape[0])
        if up.dim() == 4:               # conv adapter: up [O, r, 1, 1], down [r, I, k, k] - flattened in OIHW order
            if tuple(up.shape[2:]) != (1, 1):
                raise LoraError(f"LoRA adapter for {wkey}: up kernel {tuple(up.shape)} (1 x 1 expected)")
        up, down = up.reshape(up.shape[0], -1), down.reshape(r, -1)
        if tuple(up.shape) != (O, r) or tuple(down.shape) != (r, K):
            raise LoraError(f"LoRA adapter for {wkey}: up {tuple(p['up'][1].shape)} / down {tuple(p['down'][1].shape)} do not fit the "
                            f"weight {tuple(shape)} at rank {r}")
        alpha = float(p["alpha"][1]) if "alpha" in p else None
        out[wkey] = (up.contiguous(), down.contiguous(), alpha)
    return out


def merged_delta(parsed: Dict[str, tuple], scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """``{key: scale * alpha / r * up @ down}`` in float64 (host reference of what the engine merges)"""
    out = {}
    for k, (up, down, alpha) in parsed.items():
        r = up.shape[1]
        out[k] = (float(scale) * (r if alpha is None else alpha) / r) * (up.double() @ down.double())
    return out


def merge_into_state_dict(sd: Dict[str, torch.Tensor], adapters, cfg: UNetConfig) -> Dict[str, torch.Tensor]:
    """a copy of UNet state dict ``sd`` with the adapters merged on the host: ``fp16(W + sum of deltas)`` as fp32 tensors"""
    out = dict(sd)
    acc: Dict[str, torch.Tensor] = {}
    for src, scale in adapters:
        p = src if isinstance(src, ParsedLora) else parse_lora(src, cfg)
        for k, d in merged_delta(p, scale).items():
            acc[k] = acc[k] + d if k in acc else d
    for k, d in acc.items():
        w = sd[k]
        out[k] = (w.double() + d.reshape(w.shape)).to(torch.float16).to(torch.float32)
    return out


class LoraState:
    """The adapters currently merged into one engine.  ``sink(key, up, down)`` performs the merge for one weight
    (``HipUNet.lora``; ``up is None`` restores the base).  ``set`` folds every adapter's ``scale * alpha / rank`` into ``up`` in
    fp32 and concatenates the adapters of a weight along the rank axis: one sink call per touched weight, however many
    adapters; weights the previous set touched and this one does not are restored.  ``epoch`` counts the changes - the solvers
    put it into their context-cache key, because the cached cross-attention K / V^T are functions of attn2.to_k / to_v."""

    def __init__(self, cfg: UNetConfig, sink: Callable):
        self.cfg = cfg
        self.sink = sink
        self.epoch = 0
        self.keys: Tuple[str, ...] = ()
        self.adapters: List[Tuple[ParsedLora, float]] = []

    def parse(self, adapters: Iterable, ignore_text_encoder: bool = False) -> List[Tuple[ParsedLora, float]]:
        out = []
        if isinstance(adapters, (dict, str)):              # one adapter, scale 1
            adapters = [adapters]
        for item in adapters or ():
            src, scale = item if isinstance(item, (tuple, list)) else (item, 1.0)
            p = src if isinstance(src, ParsedLora) else parse_lora(src, self.cfg, ignore_text_encoder=ignore_text_encoder)
            out.append((p, float(scale)))
        return out

    def set(self, adapters: Iterable, ignore_text_encoder: bool = False):
        parsed = self.parse(adapters, ignore_text_encoder)
        ups: Dict[str, list] = {}
        downs: Dict[str, list] = {}
        for p, scale in parsed:
            for key, (up, down, alpha) in p.items():
                r = int(up.shape[1])
                s = torch.tensor(scale * (r if alpha is None else alpha) / r, dtype=torch.float32)
                ups.setdefault(key, []).append(up.to(torch.float32) * s)
                downs.setdefault(key, []).append(down.to(torch.float32))
        touched, ok = [], False
        try:
            for key in ups:
                touched.append(key)
                self.sink(key, torch.cat(ups[key], dim=1).contiguous(), torch.cat(downs[key], dim=0).contiguous())
            for key in self.keys:
                if key not in ups:
                    self.sink(key, None, None)
            ok = True
        finally:
            # whatever happened, the weights may differ from what the solvers cached against; after a failure every weight
            # that may hold an adapter stays listed, so that the next set() restores it
            self.epoch += 1
            self.keys = tuple(ups) if ok else tuple(dict.fromkeys(list(self.keys) + touched))
        self.adapters = parsed
        return self

    def rescale(self, scale: float):
        """the same adapters, every one at ``scale``"""
        return self.set([(p, float(scale)) for p, _ in self.adapters])


def parse_cli(specs: Optional[Iterable[str]]) -> List[Tuple[str, float]]:
    """``--lora PATH[:SCALE]`` (repeatable) -> ``[(path, scale)]``"""
    out = []
    for s in specs or ():
        path, scale = s, 1.0
        head, sep, tail = s.rpartition(":")
        if sep and head:
            try:
                path, scale = head, float(tail)
            except ValueError:
                pass
        out.append((path, scale))
    return out
