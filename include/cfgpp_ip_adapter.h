/* libcfgpp_hip.so - IP-Adapter extension of the C ABI in include/cfgpp.h (same library, same conventions: device pointers, work
 * enqueued on `stream`, 0 on success, < 0 with a message in cfgpp_last_error()).
 *
 * Kept in its own header: include/cfgpp.h is the drop-in boundary for the reference's seam and stays at its size; what is
 * declared here has no counterpart in the reference at all.
 */
#ifndef CFGPP_IP_ADAPTER_H
#define CFGPP_IP_ADAPTER_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- IP-Adapter: image prompts (diffusers `load_ip_adapter` with ip-adapter_sd15 / ip-adapter_sdxl / ip-adapter_sdxl_vit-h: one
 * adapter, the Linear + LayerNorm ImageProjection; the Resampler "plus" variants load through the same cfgpp_unet_ip_load and take
 * their image context through include/cfgpp_ip_plus.h; not the FaceID variants).  No reference counterpart: the reference conditions
 * on text only. */

/* Load one adapter tensor into a FINALIZED UNet engine (not a ControlNet), converted to the engine's dtypes and uploaded; `host`,
 * dtype, shape as cfgpp_unet_load_tensor.  Keys (cross = cross_attention_dim):
 *   image_proj.proj.weight [n_img * cross, embed_dim], image_proj.proj.bias [n_img * cross]     1 <= n_img <= 32, embed_dim % 64 == 0
 *   image_proj.norm.weight / .bias [cross]
 *   <block>.attn2.to_k_ip.weight, <block>.attn2.to_v_ip.weight [C, cross]   for every transformer block, by its diffusers name
 *                                                                          (e.g. "down_blocks.1.attentions.0.transformer_blocks.0")
 * - diffusers `unet.encoder_hid_proj` (ImageProjection) and the to_k_ip / to_v_ip of every IPAdapterAttnProcessor2_0, whose numbered
 * checkpoint keys ("ip_adapter.<2i+1>.to_k_ip.weight") the binding maps to block names.  key == NULL drops the adapter and frees its
 * memory.  The UNet's own weights do not move: tile pins, LoRA bases and captured graphs stay valid; LoRA merges are independent of
 * the adapter's weights.  A load deactivates the adapter until the next cfgpp_unet_image_context.  Unknown key or wrong shape:
 * error naming the key, nothing changed.  The adapter's bytes count in cfgpp_unet_device_bytes.  Synchronises the device. */
int cfgpp_unet_ip_load(cfgpp_unet* u, const char* key, const void* host, int dtype, const long* shape, int ndim);

/* Image conditioning for the next forwards.  image_embeds: fp16 [rows][embed_dim] (DEVICE), the CLIP image embeddings, uc rows first
 * then c rows - the row order of `ehs`; rows must equal the rows of the current text context (call cfgpp_unet_set_context first).
 * Replaces, once per job instead of per step:
 *   ImageProjection.forward:  tokens = LayerNorm(proj(image_embeds).reshape(rows, n_img, cross))          (unet.encoder_hid_proj)
 *   IPAdapterAttnProcessor2_0.__call__:  ip_key = to_k_ip(tokens), ip_value = to_v_ip(tokens)             per cross-attention
 * by one GEMM + LayerNorm and one head-scatter GEMM per block that writes the block's image K / V^T into key slots [96, 96 + n_img)
 * of the buffers that hold the text K / V^T in slots [0, 77) (slots [96, 128) are cleared first).  While active, every
 * cross-attention of the forward computes
 *   hidden_states = SDPA(q, k_text, v_text) + scale * SDPA(q, ip_key, ip_value)                          (same processor)
 * in the launch that computed the text attention alone (head dims padded to 64: all of SDXL, SD1.5's first level; other head dims
 * add one small launch per block), so a forward launches what it launched without the adapter.  image_embeds == NULL or scale == 0
 * deactivates: the next forward is bit-identical to an engine that never had an adapter.  The embeds are identified BY ADDRESS: a
 * call with the same image_embeds and rows only changes `scale` and launches nothing - after rewriting the buffer in place pass
 * NULL once.  A later cfgpp_unet_set_context with the same rows keeps the image slots (the text projection writes slots < 77 only).
 * Missing adapter tensors: error naming them.  cfgpp_sample_graph_ddim keys its graph on (active, n_img, scale).  A ControlNet
 * attached to this UNet sees the text only. */
/* (Named like cfgpp_unet_image_condition: in these headers "_set_" marks the development switches of cfgpp_debug.h.) */
int cfgpp_unet_image_context(cfgpp_unet* u, const void* image_embeds, int rows, int embed_dim, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_IP_ADAPTER_H */
