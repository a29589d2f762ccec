/* libcfgpp_hip.so - regional-prompt extension of the C ABI in include/cfgpp.h (same library, same conventions: 0 on success, < 0
 * with a message in cfgpp_last_error()).
 *
 * Kept in its own header, like include/cfgpp_long_prompt.h: include/cfgpp.h is the drop-in boundary for the reference's seam and
 * stays at its size (40 entry points, its cap); the reference conditions the whole image on one prompt and has no counterpart.
 */
#ifndef CFGPP_REGIONS_H
#define CFGPP_REGIONS_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Regional prompts ("attention couple"): R = n_regions = 2 .. 4 prompts of 77 tokens, stacked along the token axis of the context
 * ([rows, 77 R, D]: region r's keys are tokens [77 r, 77 r + 77)), and a region id per latent pixel.  While on, every
 * cross-attention of the UNet computes, for the query at pixel p of region r, softmax(q K[77 r : 77 r + 77]) V[77 r : 77 r + 77] -
 * the cross-attention of region r's prompt alone at that pixel - in ONE launch per block (cfgpp_op_attention_region: the head's
 * K / V^T of all regions resident in LDS, the mask a per-row key range inside the softmax).  Self-attention, resnets and the time /
 * added-condition embeddings are untouched.
 *
 * ids_host is a HOST uint8 [map_rows][sample_h][sample_w] with ids < n_regions (refused with the id and n_regions otherwise) and
 * map_rows = 1 (one map for every row) or the context's row count.  The map of UNet level l (and of the mid block, at the deepest
 * level) is the nearest downsample id_l[y][x] = id_0[y << l][x << l]; the level maps are made on the host and copied, once per
 * call, into per-level device buffers that cfgpp_unet_finalize allocates when max_tokens > 77 (max_rows x q_tok_pad bytes each,
 * counted in cfgpp_unet_device_bytes).  Nothing is allocated here.  (NULL, 0, 0) turns regions off: the plain engine, bit for bit
 * and launch for launch, as if the call had never been made.
 *
 * On a finalized engine only.  Needs max_tokens >= 77 * n_regions (cfgpp_unet_set_max_tokens before finalize; refused with both
 * numbers).  While on, cfgpp_unet_forward refuses a context whose tokens != 77 * n_regions with both numbers, and
 * cfgpp_sample_graph_ddim refuses by name (a region-masked step is not captured: run the eager loop).  A ControlNet-mode engine and
 * an engine with an IP-Adapter loaded refuse the call by name. */
int cfgpp_unet_set_regions(cfgpp_unet* u, const unsigned char* ids_host, int map_rows, int n_regions);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_REGIONS_H */
