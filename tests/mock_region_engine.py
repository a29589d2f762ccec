"""CPU stand-in for ``HipEngine`` with regional prompts, in the style of tests/mock_engine.py and used ONLY by tests: the solver's
region path (context stacking, map building, the order of the engine calls, the refusals) runs on the CPU, and with a state dict
the UNet is the fp32 oracle of tests/region_ref.py."""
from __future__ import annotations

import torch

from mock_engine import MockEngine


class RegionCalls:
    """mixin for any mock engine (tests/lcm_mock.py, tests/sde_mock.py, ..): records ``set_regions`` and the context it follows"""
    _regions = 0

    @property
    def regions(self):
        return self._regions

    def set_context(self, uc, c, text_embeds=None, time_ids=None):
        self.__dict__.setdefault("order", []).append("context")
        super().set_context(uc, c, text_embeds, time_ids)

    def set_regions(self, ids, n_regions=0):
        self.__dict__.setdefault("order", []).append("regions")
        self.__dict__.setdefault("region_calls", []).append((None if ids is None else torch.as_tensor(ids).clone(), int(n_regions) if ids is not None else 0))
        self._regions = int(n_regions) if ids is not None else 0
        return self


class RegionMockEngine(MockEngine):
    """records every ``set_regions`` / ``set_context`` call; ``cfg`` / ``sd`` None: the UNet is a cheap deterministic function of
    (z, t, context) - enough for the host tests, which compare calls, not images"""

    def __init__(self, cfg=None, sd=None, latent_hw=(8, 8)):
        self.ref = None
        if cfg is not None:
            from region_ref import RegionUNetRef
            self.ref = RegionUNetRef(cfg, sd)
        super().__init__(self._unet, latent_hw)
        self.region_calls = []          # (ids or None, n_regions) in call order
        self.order = []                 # "context" / "regions" in call order
        self._regions = 0
        self._ids = None

    @property
    def regions(self):
        return self._regions

    def set_context(self, uc, c, text_embeds=None, time_ids=None):
        self.order.append("context")
        super().set_context(uc, c, text_embeds, time_ids)

    def set_regions(self, ids, n_regions=0):
        self.order.append("regions")
        self.region_calls.append((None if ids is None else torch.as_tensor(ids).clone(), int(n_regions) if ids is not None else 0))
        self._ids = None if ids is None else torch.as_tensor(ids).long()
        self._regions = int(n_regions) if ids is not None else 0
        return self

    def _unet(self, z, t, ehs, te, ti):
        if self.ref is None:
            return (z.float() * 0.9 + 0.01 * ehs.float().mean() + 1e-4 * t).half()
        ids = self._ids
        if ids is not None and ids.shape[0] > 1:
            ids = torch.cat([ids, ids], 0)                  # rows [uc_1..uc_B, c_1..c_B]: both halves use the same map
        self.ref.set_regions(ids, self._regions)
        ack = None if te is None else {"text_embeds": te.float(), "time_ids": ti.float()}
        return self.ref(z.float(), t, ehs.float(), ack)["sample"].half()
