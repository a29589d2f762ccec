/* libcfgpp_hip.so - soft regional prompts: the weighted continuation of include/cfgpp_regions.h (same library, same conventions: 0
 * on success, < 0 with a message in cfgpp_last_error()).  Kept in its own header for the reason given there.
 */
#ifndef CFGPP_REGIONS_SOFT_H
#define CFGPP_REGIONS_SOFT_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Soft regions: R = n_regions = 2 .. 4 prompts of 77 tokens stacked along the token axis of the context as for
 * cfgpp_unet_set_regions, and a WEIGHT per region and latent pixel instead of one id.  While on, every cross-attention of the UNet
 * computes, for the query at pixel p,
 *     o = sum_r w_r(p) * softmax(q K[77 r : 77 r + 77]) V[77 r : 77 r + 77]
 * in ONE launch per block (cfgpp_op_attention_region_soft: every region's softmax complete over its own 77 keys, an MFMA kernel for
 * every head dim the engine configs reach, a term with w_r(p) == 0 not evaluated).  One-hot weights are the hard partition of
 * cfgpp_unet_set_regions.  Self-attention, resnets and the time / added-condition embeddings are untouched.
 *
 * cfgpp_unet_enable_region_weights: before cfgpp_unet_finalize, after cfgpp_unet_set_max_tokens(> 77).  It makes finalize allocate,
 * next to the per-level id maps, one fp32 buffer per level, max_rows x 4 x q_tok_pad, counted in cfgpp_unet_device_bytes.  Without
 * the call nothing is allocated and cfgpp_unet_set_region_weights is refused by name. */
int cfgpp_unet_enable_region_weights(cfgpp_unet* u);

/* w_host is a HOST fp32 [map_rows][n_regions][sample_h][sample_w], map_rows = 1 (one map for every row) or the context's row count.
 * The weights of UNet level l are the nearest downsample w_l[r][y][x] = w_0[r][y << l][x << l] (no area averaging); the level maps are
 * made on the host and copied, once per call.  Nothing is allocated.  Refused by name: a non-finite or negative weight (with row,
 * region and pixel), a pixel whose weights sum outside 1 +- 1e-4, n_regions outside 2 .. 4, max_tokens < 77 * n_regions, an engine
 * that was not enabled, a ControlNet-mode engine, an engine with an IP-Adapter loaded.  (NULL, 0, 0) turns the weights off.
 *
 * Soft weights and the hard id map are exclusive: a successful call of one clears the other.  While on, cfgpp_unet_forward refuses
 * a context whose tokens != 77 * n_regions and a row count the map was not set for, and cfgpp_sample_graph_ddim refuses by name. */
int cfgpp_unet_set_region_weights(cfgpp_unet* u, const float* w_host, int map_rows, int n_regions);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_REGIONS_SOFT_H */
