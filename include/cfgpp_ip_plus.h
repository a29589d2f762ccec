/* libcfgpp_hip.so - IP-Adapter "plus" extension of the C ABI (same library, same conventions as include/cfgpp.h: device pointers,
 * work enqueued on `stream`, 0 on success, < 0 with a message in cfgpp_last_error()).
 *
 * Kept in its own header, like include/cfgpp_ip_adapter.h: include/cfgpp.h is the drop-in boundary for the reference's seam and
 * stays at its size; what is declared here has no counterpart in the reference at all.
 */
#ifndef CFGPP_IP_PLUS_H
#define CFGPP_IP_PLUS_H
#include "cfgpp_ip_adapter.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- IP-Adapter Plus: the Resampler image projection (ip-adapter-plus_sd15, ip-adapter-plus-face_sd15, ip-adapter-plus_sdxl_vit-h,
 * ip-adapter-plus-face_sdxl_vit-h).  A Perceiver Resampler turns the CLIP image tower's penultimate hidden states [rows, seq, embed]
 * into n_q image tokens; everything behind the projection (the image K / V^T slots, the decoupled cross-attention, graph keying) is
 * that of include/cfgpp_ip_adapter.h.
 *
 * cfgpp_unet_ip_load takes these further keys, same conventions (finalized UNet, not a ControlNet, error naming the key and shape,
 * nothing changed on error), the published checkpoint naming under "image_proj.":
 *   latents [1, n_q, D] (or [n_q, D])                       1 <= n_q <= 32
 *   proj_in.weight [D, E], proj_in.bias [D]                 E = the tower's hidden size
 *   proj_out.weight [cross, D], proj_out.bias [cross]       cross = the UNet's cross_attention_dim
 *   norm_out.weight / .bias [cross]
 *   layers.<i>.0.norm1 / .norm2 .weight / .bias [D]         0 <= i < depth, 1 <= depth <= 8
 *   layers.<i>.0.to_q.weight [inner, D], .to_kv.weight [2 * inner, D], .to_out.weight [D, inner]       heads = inner / 64
 *   layers.<i>.1.0.weight / .bias [D], layers.<i>.1.1.weight [ff_inner, D], layers.<i>.1.3.weight [D, ff_inner]
 * D, E, inner and ff_inner are multiples of 64; every layer has layer 0's shapes.  Matrices are kept in fp16, biases, norms and the
 * latents in fp32.  An adapter has ONE kind: after a drop (key == NULL) the first image_proj.* tensor fixes it (Linear + LayerNorm:
 * image_proj.proj.* / image_proj.norm.*; Resampler: the keys above) and a tensor of the other kind is refused by name until the
 * next drop. */

/* Image conditioning of a Resampler adapter for the next forwards.  hidden: fp16 [rows][seq][embed_dim] (DEVICE), the tower's
 * penultimate hidden states, uc rows first then c rows; 1 <= seq <= 1024, embed_dim = E.  Computes, once per job,
 *   x   = proj_in(hidden);  lat = latents for every row
 *   per layer:  q = to_q(norm2(lat));  k, v = to_kv over norm1(x) followed by norm2(lat)
 *               lat += to_out(softmax(q k^T / 8) v)                      heads of 64, one softmax over all seq + n_q keys
 *               lat += W2(GELU_erf(W1(LayerNorm(lat))))
 *   tokens = LayerNorm(proj_out(lat))                                    [rows][n_q][cross]
 * every GEMM on the implicit-GEMM launcher with bias / residual in its epilogue, the attention in one launch per layer reading the
 * GEMMs' token-major outputs (csrc/resampler.hip), activations in fp16 between launches; then the per-block to_k_ip / to_v_ip
 * head-scatter of cfgpp_unet_image_context.  Scratch is adapter memory (counted in cfgpp_unet_device_bytes, freed by the drop),
 * allocated on the first call from (max_rows, seq) and again only when a longer seq arrives.
 * Otherwise exactly cfgpp_unet_image_context: rows must equal the text context's; hidden is identified BY ADDRESS together with
 * (rows, seq) - a call that changes only `scale` launches nothing; hidden == NULL or scale == 0 deactivates and the next forward
 * is bit-identical to an engine that never had an adapter; the image slots are cleared before they are written; missing adapter
 * tensors are named; cfgpp_sample_graph_ddim keys its graph on (active, n_img, scale).
 * On a Linear adapter this call is an error that names cfgpp_unet_image_context, and cfgpp_unet_image_context on a Resampler
 * adapter is an error that names this call. */
int cfgpp_unet_image_context_seq(cfgpp_unet* u, const void* hidden, int rows, int seq, int embed_dim, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_IP_PLUS_H */
