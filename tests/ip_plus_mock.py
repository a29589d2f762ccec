"""CPU mock engine for Resampler ("plus") IP-Adapters: ``tests/ip_adapter_mock.IPMockEngine`` driving
``tests/ip_plus_ref.IPPlusUNetRef``, with ``HipEngine.set_image_embeds``'s handling of the two adapter kinds - TEST INFRASTRUCTURE
ONLY, injected with ``get_solver(..., engine=...)``."""
from __future__ import annotations

from cfgpp_amd.ip_adapter import assemble_embeds, assemble_hidden
from ip_adapter_mock import IPMockEngine
from ip_plus_ref import IPPlusUNetRef


class _EitherRef(IPPlusUNetRef):
    """the Resampler for [R, S, E] hidden states, the Linear projection for [R, E] embeds"""

    def image_tokens(self, embeds, fp64=None):
        if embeds.dim() == 3:
            return super().image_tokens(embeds, fp64)
        return super(IPPlusUNetRef, self).image_tokens(embeds)


class IPPlusMockEngine(IPMockEngine):
    def __init__(self, cfg, sd, latent_hw=(16, 16), adapter=None):
        super().__init__(cfg, sd, latent_hw, None)
        self.net = _EitherRef(cfg, sd, {})
        if adapter is not None:
            self.set_ip_adapter(adapter)

    def set_image_embeds(self, embeds, negative=None, scale=1.0):
        if embeds is None or float(scale) == 0.0:
            self.net.set_image(None, 0.0)
            self.image_calls.append((None, 0.0))
            return
        if self._ip is None:
            raise ValueError("no IP-Adapter is loaded")
        rows = (assemble_hidden if self._ip.seq_input else assemble_embeds)(embeds, negative, self.B)
        self.net.set_image(rows.float(), scale)
        self.image_calls.append((rows.clone(), float(scale)))
