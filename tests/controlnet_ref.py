"""CPU restatement of diffusers ``ControlNetModel`` (one net, non-guess mode) and of ``UNet2DConditionModel.forward`` with
``down_block_additional_residuals`` / ``mid_block_additional_residual`` - TEST INFRASTRUCTURE ONLY, on the primitives of
``oracle.unet_ref.UNetRef`` (fp32 torch ops; the latent, the sinusoids and the control image rounded through fp16 as the fp16
engine and pipeline do)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.unet_ref import UNetRef, timestep_embedding


def _emb(net: UNetRef, R, timestep, added_cond_kwargs):
    cfg = net.cfg
    t = torch.as_tensor(timestep, dtype=torch.float32).reshape(-1)
    if t.numel() == 1:
        t = t.expand(R)
    temb = timestep_embedding(t, cfg.block_out_channels[0])
    if net.round_io:
        temb = temb.half().float()
    emb = net._lin("time_embedding.linear_2", F.silu(net._lin("time_embedding.linear_1", temb)))
    if cfg.addition_embed:
        te = added_cond_kwargs["text_embeds"].float()
        ti = added_cond_kwargs["time_ids"].float()
        tproj = timestep_embedding(ti.flatten(), cfg.addition_time_embed_dim)
        if net.round_io:
            tproj = tproj.half().float()
        add = torch.cat([te, tproj.reshape(te.shape[0], -1)], dim=-1)
        emb = emb + net._lin("add_embedding.linear_2", F.silu(net._lin("add_embedding.linear_1", add)))
    return emb


def _down(net: UNetRef, x, emb, ctx):
    cfg = net.cfg
    skips = [x]
    for i in range(cfg.num_levels):
        for j in range(cfg.layers_per_block):
            x = net._resnet(f"down_blocks.{i}.resnets.{j}", x, emb)
            if cfg.level_has_attn[i]:
                x = net._transformer(f"down_blocks.{i}.attentions.{j}", x, ctx, cfg.transformer_depth[i], cfg.num_heads[i])
            skips.append(x)
        if i != cfg.num_levels - 1:
            x = net._conv(f"down_blocks.{i}.downsamplers.0.conv", x, stride=2)
            skips.append(x)
    return x, skips


def _mid(net: UNetRef, x, emb, ctx):
    cfg = net.cfg
    x = net._resnet("mid_block.resnets.0", x, emb)
    x = net._transformer("mid_block.attentions.0", x, ctx, cfg.transformer_depth[-1], cfg.num_heads[-1])
    return net._resnet("mid_block.resnets.1", x, emb)


class ControlNetRef(UNetRef):
    """``__call__(sample, t, ehs, image, scale, added_cond_kwargs) -> (down_block_res_samples, mid_block_res_sample)``, each
    already ``* scale``; ``image`` [R, 3, 8H, 8W] holds one row per UNet row."""

    def embed(self, image):
        q = "controlnet_cond_embedding."
        x = image.float().half().float()
        x = F.silu(self._conv(q + "conv_in", x))
        i = 0
        while (q + f"blocks.{i}.weight") in self.sd:
            x = F.silu(self._conv(q + f"blocks.{i}", x, stride=1 if i % 2 == 0 else 2))
            i += 1
        return self._conv(q + "conv_out", x)

    @torch.no_grad()
    def __call__(self, sample, timestep, encoder_hidden_states, image, scale=1.0, added_cond_kwargs=None):
        x = sample.float()
        if self.round_io:
            x = x.half().float()
        ctx = encoder_hidden_states.float()
        emb = _emb(self, x.shape[0], timestep, added_cond_kwargs)
        x = self._conv("conv_in", x) + self.embed(image)
        x, skips = _down(self, x, emb, ctx)
        x = _mid(self, x, emb, ctx)
        down = [self._conv(f"controlnet_down_blocks.{k}", s, pad=0) * scale for k, s in enumerate(skips)]
        return down, self._conv("controlnet_mid_block", x, pad=0) * scale


@torch.no_grad()
def controlled_unet(net: UNetRef, sample, timestep, encoder_hidden_states, added_cond_kwargs=None,
                    down_block_additional_residuals=None, mid_block_additional_residual=None):
    """UNet2DConditionModel.forward with ControlNet residuals: every skip gets its residual after the whole down path, the mid
    block runs on the un-added last down output, its output gets the mid residual"""
    cfg = net.cfg
    x = sample.float()
    if net.round_io:
        x = x.half().float()
    ctx = encoder_hidden_states.float()
    emb = _emb(net, x.shape[0], timestep, added_cond_kwargs)
    x = net._conv("conv_in", x)
    x, skips = _down(net, x, emb, ctx)
    if down_block_additional_residuals is not None:
        skips = [s + r for s, r in zip(skips, down_block_additional_residuals)]
    x = _mid(net, x, emb, ctx)
    if mid_block_additional_residual is not None:
        x = x + mid_block_additional_residual
    L = cfg.num_levels
    for i in range(L):
        lvl = L - 1 - i
        for j in range(cfg.layers_per_block + 1):
            x = torch.cat([x, skips.pop()], dim=1)
            x = net._resnet(f"up_blocks.{i}.resnets.{j}", x, emb)
            if cfg.level_has_attn[lvl]:
                x = net._transformer(f"up_blocks.{i}.attentions.{j}", x, ctx, cfg.transformer_depth[lvl], cfg.num_heads[lvl])
        if i != L - 1:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            x = net._conv(f"up_blocks.{i}.upsamplers.0.conv", x)
    x = F.silu(net._gn("conv_norm_out", x))
    return net._conv("conv_out", x)


def image_rows(image, R, B):
    """the pipeline's image batch for UNet rows [uc_1..uc_B, c_1..c_B]: row r uses image row (r % B) % image_rows"""
    idx = (torch.arange(R) % B) % image.shape[0]
    return image[idx]
