"""CPU mock engine with image tokens: ``tests/mock_engine.MockEngine`` driving ``tests/ip_adapter_ref.IPUNetRef``, with the
IP-Adapter methods of ``cfgpp_amd.hip_engine.HipEngine`` (set_ip_adapter / ip_adapter / set_image_embeds) - TEST INFRASTRUCTURE
ONLY, injected with ``get_solver(..., engine=...)``."""
from __future__ import annotations

import torch

from cfgpp_amd.ip_adapter import assemble_embeds, resolve
from ip_adapter_ref import IPUNetRef
from mock_engine import MockEngine


class IPMockEngine(MockEngine):
    def __init__(self, cfg, sd, latent_hw=(16, 16), adapter=None):
        self.cfg, self.sd = cfg, sd
        self.net = IPUNetRef(cfg, sd, {})
        super().__init__(self._unet, latent_hw)
        self.image_calls = []               # (embeds rows [2B, E] | None, scale) of every set_image_embeds
        self._ip = None
        if adapter is not None:
            self.set_ip_adapter(adapter)

    def _unet(self, z, t, ehs, te, ti):
        kw = None if te is None else dict(text_embeds=te.float(), time_ids=ti.float())
        return self.net(z, t, ehs.float(), kw)["sample"].half()

    def set_ip_adapter(self, spec):
        self._ip = resolve(spec, self.cfg)
        self.net.ip = {} if self._ip is None else {k: v.float() for k, v in self._ip.items()}
        self.net.set_image(None, 0.0)
        return self

    @property
    def ip_adapter(self):
        return self._ip

    def set_image_embeds(self, embeds, negative=None, scale=1.0):
        if embeds is None or float(scale) == 0.0:
            self.net.set_image(None, 0.0)
            self.image_calls.append((None, 0.0))
            return
        if self._ip is None:
            raise ValueError("no IP-Adapter is loaded")
        rows = assemble_embeds(embeds, negative, self.B)
        self.net.set_image(rows.float(), scale)
        self.image_calls.append((rows.clone(), float(scale)))
