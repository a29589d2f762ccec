/* libcfgpp_hip.so - CLIP image tower extension of the C ABI (same library, same conventions as include/cfgpp.h: device pointers,
 * work enqueued on `stream`, 0 on success, < 0 with a message in cfgpp_last_error()).
 *
 * Kept in its own header, like include/cfgpp_ip_adapter.h: include/cfgpp.h is the drop-in boundary for the reference's seam and
 * stays at its size; the reference conditions on text only and has no image tower at all.
 *
 * What it is for: an IP-Adapter consumer hands the UNet image EMBEDDINGS (cfgpp_unet_image_context: the pooled, projected
 * `image_embeds`; cfgpp_unet_image_context_seq: the penultimate hidden states).  This engine computes both from a picture -
 * `transformers.CLIPVisionModelWithProjection` (ViT-L/14, ViT-H/14, ViT-bigG/14 at 224 px) on the library's own kernels
 * (cfgpp_amd/csrc/vision.hip), so that an image-prompted job needs neither Python nor torch.
 */
#ifndef CFGPP_VISION_H
#define CFGPP_VISION_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct cfgpp_vision cfgpp_vision;

/* Geometry: hidden = heads * d with d in {64, 80, 104}; hidden and intermediate multiples of 64; image_size a multiple of
 * patch_size; tokens T = 1 + (image_size / patch_size)^2 <= 320; act 0 = quick_gelu, 1 = gelu (erf); proj_dim > 0 and a multiple of
 * 4; max_batch = images per cfgpp_vision_encode call.  Anything else is refused by name (NULL + cfgpp_last_error()). */
cfgpp_vision* cfgpp_vision_create(int hidden, int layers, int heads, int intermediate, int act, int proj_dim, int image_size,
                                  int patch_size, int max_batch, int device_id);
void cfgpp_vision_destroy(cfgpp_vision* v);
/* Keys: the `transformers` CLIPVisionModelWithProjection state dict, unchanged: "vision_model.embeddings.class_embedding",
 * "vision_model.embeddings.patch_embedding.weight", "vision_model.embeddings.position_embedding.weight",
 * "vision_model.pre_layrnorm.weight" / ".bias" (the spelling is the library's), "vision_model.encoder.layers.<i>.layer_norm1 /
 * layer_norm2 / self_attn.{q,k,v,out}_proj / mlp.fc1 / mlp.fc2 .weight / .bias", "vision_model.post_layernorm.weight" / ".bias",
 * "visual_projection.weight"; the "vision_model." prefix may be absent.  host: HOST memory, dtype 0 = fp32, 1 = fp16. */
int cfgpp_vision_load_tensor(cfgpp_vision* v, const char* key, const void* host, int dtype, const long* shape, int ndim);
int cfgpp_vision_finalize(cfgpp_vision* v);
/* img: DEVICE fp32 [N][3][H][W] in [0, 1], any H, W >= 1, any N >= 1 -> pixels_out: DEVICE fp16 [N][3][S][S], S = image_size:
 * short side to S with the antialiased bicubic filter of torch (separable, horizontal pass first, fp32 between the passes,
 * a = -0.5, support 2 * max(scale, 1), weights normalised by their sum), clamp to [0, 1], centre crop, (x - mean) / std of CLIP.
 * One launch; only the S x S crop window is computed. */
int cfgpp_vision_preprocess(cfgpp_vision* v, const float* img, int N, int H, int W, void* pixels_out, void* stream);
/* pixels: DEVICE fp16 [N][3][S][S], 1 <= N <= max_batch.  layer: -1 = no hidden output, k in [0, layers] = hidden_states[k] of
 * `transformers` (hidden_states[0]: the token stream after pre_layrnorm; [layers]: after the last layer, before post_layernorm).
 * hidden_out: DEVICE fp16 [N][T][hidden] or NULL (required when layer >= 0); embeds_out: DEVICE fp32 [N][proj_dim] or NULL -
 * image_embeds = visual_projection(post_layernorm(hidden_states[layers][:, 0])). */
int cfgpp_vision_encode(cfgpp_vision* v, const void* pixels, int N, int layer, void* hidden_out, float* embeds_out, void* stream);
/* floating-point operations of one encode of N images (GEMMs and attention; 2 per multiply-add) */
double cfgpp_vision_flops(cfgpp_vision* v, int N);
double cfgpp_vision_device_bytes(cfgpp_vision* v);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_VISION_H */
