/* libcfgpp_hip.so - C ABI of the MI355X-native CFG++ sampling hot path.
 *
 * The reference (CFGpp-diffusion/CFGpp) has no FFI of its own: its hot path is
 * the pure-Python seam
 *     self.unet(z_in, t_in, encoder_hidden_states=..., added_cond_kwargs=...)['sample']
 *         latent_diffusion.py:146,149,155      latent_sdxl.py:170,174,181
 * plus the per-step elementwise sampler arithmetic
 *         latent_diffusion.py:660-666 (and 179-180, 283-286, 479-490, 708-710, 855-866, 907-908)
 *         latent_sdxl.py:738-744 (and 317-318, 453-456, 904-919, 972-973).
 * This header declares what a binding for that seam calls instead.  Each entry
 * point cites the reference lines it replaces.
 *
 * Conventions: plain C types only; every data pointer is a DEVICE pointer owned
 * by the caller (PyTorch-ROCm tensor storage) unless the name says `host`; all
 * work is enqueued asynchronously on the hipStream_t passed as `void* stream`
 * and nothing synchronises (one exception: the tile-tuning passes of the first
 * forward at a batch size: the engine times every implicit-GEMM launch of its plan in place once per candidate tile and
 * pins the fastest - a few extra forwards and host syncs, results bit-identical across candidates; environment
 * CFGPP_AUTOTUNE=0 of the Python binding, or cfgpp_unet_tuning(set = 1), skips them); return 0 on success, < 0 on error
 * with a message in cfgpp_last_error() (thread-local).  Not thread-safe: one host thread drives the library; several
 * engines may run concurrently on different streams (the K-split workspace is per stream).  ONE DEVICE PER PROCESS (the
 * torchrun layout, one rank per GPU): cfgpp_unet_create / cfgpp_vae_create refuse a device other than the first one the
 * process used.
 *
 * This header is the whole drop-in boundary.  Single-kernel test hooks (cfgpp_op_*) and the development / A-B switches of
 * the launcher live in cfgpp_amd/csrc/cfgpp_debug.h: exported by the same library, bound only by tests/ and scripts/.
 */
#ifndef CFGPP_H
#define CFGPP_H
#ifdef __cplusplus
extern "C" {
#endif

const char* cfgpp_last_error(void);

/* Provenance of this binary (no reference counterpart): "cfgpp-build:<digest of the kernel sources + flags it was compiled
 * from>:<git HEAD when it was linked>[+local]".  cfgpp_amd/build.py names every object file by the same digests, so a stale
 * object cannot be linked; bench.py, smoke() and the real-size GPU tests print this string next to their numbers. */
const char* cfgpp_build_id(void);

/* ---- fused sampler step (K12) ------------------------------------------- */

/* Generalised DDIM update on n fp32 latent elements, in place:
 *     eps_hat = eps_uc + lam*(eps_c - eps_uc)
 *     z0t = (z - c1*A)/c2 ;  z = c3*z0t + c4*B ;  A,B in {eps_hat, eps_uc}
 * replaces latent_diffusion.py:660-666 (CFG++: tweedie_uc=0, renoise_uc=1),
 * :280-286 (CFG: 0,0), :177-180 (inversion CFG: 0,0 with coefficients swapped),
 * :905-908 (inversion CFG++: 1,0) and latent_sdxl.py:738-744, 450-456, 315-318, 970-973.
 * eps_is_half=1: eps are fp16 (the autocast UNet output) and every eps product is
 * rounded to fp16 exactly as torch promotion does.  n must be a multiple of 4.
 * Divisors (c2 here; s of cfgpp_kdiff_input mode 0; sigma_item and two_r of cfgpp_step_kdiff) are positive on this
 * path, and their SIGN selects how the quotient is formed: c > 0 is an IEEE division (torch-CPU); c < 0 means the
 * caller passes c = -fl32(1/divisor) and the kernel multiplies by -c - torch's GPU `div` with a CPU-scalar divisor
 * (`/ at.sqrt()`, `/ sigma.item()`, `/ (2*r)`), which is `a * (1/b)` with the reciprocal taken once in fp32. */
int cfgpp_step_ddim(void* z, void* z0t_out, const void* eps_uc, const void* eps_c, int eps_is_half,
                    float lam, float c1, float c2, float c3, float c4,
                    int tweedie_uc, int renoise_uc, long n, void* stream);

/* The same update on n fp16 latent elements (z, z0t_out and both eps fp16), every op rounded to
 * fp16: the reference's inversion / edit paths, whose latent starts as the fp16 `vae.encode(...)`
 * sample and therefore stays fp16 through `inversion()` and the regeneration loop
 * (latent_diffusion.py:168-180,527-541,901-908; latent_sdxl.py:307-318,966-1011). */
int cfgpp_step_ddim_h(void* z, void* z0t_out, const void* eps_uc, const void* eps_c,
                      float lam, float c1, float c2, float c3, float c4,
                      int tweedie_uc, int renoise_uc, long n, void* stream);

/* Inpainting with an ordinary (4-channel) UNet: the fp32-latent / fp16-eps update of cfgpp_step_ddim (eps_is_half = 1) on
 * B x 4 x hw elements, blended in the same pass with the forward-noised source latent (diffusers
 * StableDiffusionInpaintPipeline.__call__, `num_channels_unet == 4` branch: init_latents_proper =
 * scheduler.add_noise(image_latents, noise, t_next); latents = (1 - init_mask) * init_latents_proper + init_mask * latents):
 *     z = mask ? z_new : a*src + b*noise          z0t_out = mask ? z0t : src
 * mask: uint8 [B][hw], 0 = keep, nonzero = repaint (binarized by the caller); src fp16 [B][4][hw]; noise fp32 [B][4][hw];
 * (a, b) = (sqrt(at_prev), sqrt(1 - at_prev)) of the step, (1, 0) on the last one.  The two products and the sum are
 * rounded separately (torch's `a*src.float() + b*noise`).  hw must be a multiple of 4.  An all-ones mask gives the bits
 * of cfgpp_step_ddim. */
int cfgpp_step_ddim_masked(void* z, void* z0t_out, const void* eps_uc, const void* eps_c, float lam, float c1, float c2,
                           float c3, float c4, int tweedie_uc, int renoise_uc, const void* mask, const void* src,
                           const void* noise, float a, float b, int B, long hw, void* stream);

/* k-diffusion UNet input scaling on fp16 latents: mode 0: xc = x / s
 * (latent_diffusion.py:229-230, s = sqrt(sigma^2+1)); mode 1: xc = x * s (latent_sdxl.py:901). */
int cfgpp_kdiff_input(const void* x, void* xc, float s, int mode, long n, void* stream);

/* Euler / DPM-Solver++(2M) update on fp16 latents, in place.
 * coef[9] = {lam, sigma, c_out_h, sigma_item, sigma_next, neg_exp_mh_h, expm1_mh_h, two_r, exp_mh_h}
 * variant 0 = CFG (latent_diffusion.py:477-490, 329-333), 1 = CFG++ SD1.5 (:853-866, 706-710),
 * 2 = CFG++ SDXL (latent_sdxl.py:901-919).  xl_form: denoised = x + c_out*eps instead of x - eps*sigma.
 * euler_branch=1 selects x' = den + ((x - d_from)/sigma)*sigma_next.  den_out receives `denoised`. */
int cfgpp_step_kdiff(void* x, void* den_out, void* old, const void* eps_uc, const void* eps_c,
                     const float* coef_host, int variant, int xl_form, int euler_branch, int write_old,
                     long n, void* stream);

/* denoised = x - eps_hat*sigma and uncond_denoised = x - eps_uc*sigma on fp16 latents
 * (kdiffusion_x_to_denoised, latent_diffusion.py:235-241); used by the 2-stage DPM++(2S) samplers. */
int cfgpp_kdiff_denoise(const void* x, const void* eps_uc, const void* eps_c, float lam, float sigma,
                        void* den, void* uden, long n, void* stream);
/* fp16 linear combinations with torch's rounding order (out may alias x):
 * mode 0: out = x*a - y*b            (latent_diffusion.py:428,435,804)
 * mode 1: out = (y - z*b) + x*a      (latent_diffusion.py:811)
 * mode 2: out = x + y*a              (ancestral noise, latent_diffusion.py:379,438,755,814) */
int cfgpp_lincomb(void* out, const void* x, const void* y, const void* z, float a, float b, int mode, long n, void* stream);

/* ---- UNet engine (replaces `self.unet(...)`) ------------------------------ */

typedef struct cfgpp_unet_config {
    int in_channels, out_channels;
    int num_levels;               /* 4 for SD1.5, 3 for SDXL */
    int block_out_channels[4];
    int layers_per_block;         /* 2 */
    int level_has_attn[4];        /* CrossAttn{Down,Up}Block2D per level (down order) */
    int transformer_depth[4];     /* transformer layers per attention, per level */
    int num_heads[4];             /* heads per level (SD1.5: 8 everywhere; SDXL: C/64) */
    int cross_attention_dim;      /* 768 / 2048 */
    int addition_embed;           /* 0 none, 1 = "text_time" (SDXL) */
    int addition_time_embed_dim;  /* 256 */
    int addition_pooled_dim;      /* 1280 */
    int norm_groups;              /* 32 */
    int sample_h, sample_w;       /* latent size this context is built for */
    int max_rows;                 /* max UNet batch rows (2 * chains) */
} cfgpp_unet_config;

typedef struct cfgpp_unet cfgpp_unet;

/* `pipe.unet` construction (latent_diffusion.py:63-67, latent_sdxl.py:40,50). */
cfgpp_unet* cfgpp_unet_create(const cfgpp_unet_config* cfg, int device_id);
void cfgpp_unet_destroy(cfgpp_unet* u);

/* Load one state-dict entry by its diffusers key (e.g.
 * "down_blocks.0.resnets.0.conv1.weight").  `host` points to HOST memory,
 * dtype 0 = fp32, 1 = fp16; conv weights OIHW, linear weights [out,in].
 * The library copies; returns -3 for an unknown key. */
int cfgpp_unet_load_tensor(cfgpp_unet* u, const char* key, const void* host, int dtype,
                           const long* shape, int ndim);
/* Number of parameters still missing (0 = complete), names via cfgpp_last_error(). */
int cfgpp_unet_missing(cfgpp_unet* u);
/* Repack all weights into MFMA-friendly device layouts and build the launch plan. */
int cfgpp_unet_finalize(cfgpp_unet* u);

/* Conditioning for the next forwards: ehs [rows][tokens][cross_dim] fp16, tokens = 77 (or 77 * j, see
 * include/cfgpp_long_prompt.h) (uc rows first,
 * then c rows: the `torch.cat([uc, c])` of latent_diffusion.py:152); SDXL:
 * text_embeds [cond_rows][1280] fp16, time_ids [cond_rows][6] fp32, cond_rows = rows or 1
 * (1 = broadcast, the lambda==1.0 Lightning case of latent_sdxl.py:249-252).
 * Precomputes the step-invariant cross-attention K/V of every block. */
int cfgpp_unet_set_context(cfgpp_unet* u, const void* ehs, int rows, int tokens,
                           const void* text_embeds, const void* time_ids, int cond_rows, void* stream);

/* Inpaint UNets (in_channels > out_channels, e.g. SD1.5 / SDXL inpainting: 9 = 4 latent + 1 mask + 4 masked-image latent):
 * the step-invariant extra input channels, replacing the per-step
 *     latent_model_input = torch.cat([latent_model_input, mask, masked_image_latents], dim=1)
 * of diffusers StableDiffusionInpaintPipeline.__call__ / StableDiffusionXLInpaintPipeline.__call__.
 * cond: fp16 [cond_rows][in_ch - out_ch][H][W] (DEVICE), copied on `stream` into an engine-owned buffer whose address never
 * changes (a captured cfgpp_sample_graph_ddim graph stays valid when the condition changes).  Row r of the UNet batch reads
 * condition row (r % z_rows) % cond_rows: cond_rows must be z_rows or 1.  Error on an engine with in_ch == out_ch; a forward
 * of an inpaint engine before this call is an error. */
int cfgpp_unet_image_condition(cfgpp_unet* u, const void* cond, int cond_rows, void* stream);

/* eps[rows][out_ch][H][W] (fp16) = UNet(z[(row % z_rows)], t).  z: [z_rows][out_ch][H][W] (the latent channels; an inpaint
 * UNet takes the rest from cfgpp_unet_image_condition), fp32 (z_is_half=0) or fp16.  rows = 2*z_rows reproduces
 * cat([zt]*2) / chunk(2) of latent_diffusion.py:153-156: eps_uc = eps[0:z_rows], eps_c = eps[z_rows:]. */
int cfgpp_unet_forward(cfgpp_unet* u, const void* z, int z_is_half, int z_rows, float t,
                       void* eps_out, int rows, void* stream);

/* Whole-loop hipGraph replay: the reference's DDIM loops when callback_fn is None (latent_diffusion.py:653-674, 272-294,
 * 160-182, 888-910; latent_sdxl.py:730-752, 838-858) as ONE captured step - the UNet forward at `rows` plus the fused
 * generalised DDIM update of cfgpp_step_ddim / cfgpp_step_ddim_h - replayed n_steps times on `stream`.
 * host_steps[n_steps][5] = {t, c1, c2, c3, c4} per step: exactly the values the eager loop would pass to
 * cfgpp_unet_forward and cfgpp_step_ddim (HOST memory, copied before the call returns); they live in a device table
 * indexed by a device step counter, so one graph serves every step and every later call with the same buffers (the
 * engine keeps the most recent graph; other buffers / flags / batch re-capture).  z, z0t: [z_rows][out_ch][H][W] fp32 or
 * fp16 (z updated in place, z0t written every step); eps: [rows][out_ch][H][W] fp16 scratch for the UNet output;
 * eps_uc / eps_c point into it (the same pointer for the lambda == 1 Lightning form).  The first call at a batch runs one
 * eager forward (tile tuning, see above) and captures on an engine-owned stream - `stream` may be the legacy default
 * stream.  One host sync per call (the table upload), none per step.  Latents are bit-identical to the eager loop. */
int cfgpp_sample_graph_ddim(cfgpp_unet* u, void* z, void* z0t, int z_is_half, int z_rows, void* eps, const void* eps_uc,
                            const void* eps_c, int rows, const float* host_steps, int n_steps, float lam, int tweedie_uc,
                            int renoise_uc, void* stream);

/* Same forward with a HIP event between every launch (on `stream`): per kernel family
 * k = 0 implicit-GEMM conv/linear, 1 attention, 2 GroupNorm/LayerNorm, 3 small ops:
 * elapsed ms, algorithmic FLOPs and launch counts.  Used by bench.py's roofline block. */
int cfgpp_unet_profile(cfgpp_unet* u, const void* z, int z_is_half, int z_rows, float t, void* eps_out, int rows,
                       void* stream, double* out_ms, double* out_flops, int* out_launches,
                       char* detail /* optional: one text line per launch */, long detail_cap);

/* Export (set = 0) / import (set = 1) the per-launch tile configs pinned by the in-situ tuning at batch `rows`
 * (one int per implicit-GEMM launch, plan order); returns the number of slots.  A profiled run imports what the
 * un-profiled run chose, so PMC passes see the same kernels without timing passes of their own.  Pins are kept per
 * (rows, shared CFG prefix or not): export returns those of the mode the engine last ran in, an import (which may come
 * before any forward) installs the list for both modes of that batch. */
int cfgpp_unet_tuning(cfgpp_unet* u, int rows, int* hints, int cap, int set);

/* ---- ControlNet (diffusers ControlNetModel with StableDiffusionControlNetPipeline / StableDiffusionXLControlNetPipeline:
 * one net, non-guess mode).  No reference counterpart: the reference README points its users to other front ends for it. */

/* A ControlNet is a cfgpp_unet made by cfgpp_unet_create with out_channels = 0 (it has no conv_out: its outputs are residuals)
 * and in_channels = the latent channels - diffusers `ControlNetModel.from_pretrained(...)`.  It holds conv_in, the time
 * (+ add_embedding) embedding, the down blocks and the mid block from the same diffusers keys as the UNet, no up path, plus
 * `controlnet_cond_embedding.{conv_in,blocks.0-5,conv_out}` (ControlNetConditioningEmbedding with diffusers' default
 * conditioning_embedding_out_channels (16, 32, 96, 256)) and the 1x1 zero convolutions `controlnet_down_blocks.N` (one per
 * skip connection) and `controlnet_mid_block`.  load_tensor / missing / finalize / set_context / destroy work on it
 * unchanged; cfgpp_unet_image_condition sets its control image (the pipeline's prepared `image`, step-invariant):
 * fp16 [image_rows][3][8H][8W] in [0, 1], no normalisation (do_normalize=False), embedded once per job
 * (`controlnet_cond = self.controlnet_cond_embedding(controlnet_cond)`) into an engine-owned buffer whose address never changes.
 * Row r of the UNet batch uses image row (r % z_rows) % image_rows: the uncond and cond halves see the same image, as the
 * pipeline's torch.cat([image] * 2) does.  Detach a ControlNet from every UNet before destroying it. */

/* Attach ControlNet cn to UNet u (cn = NULL detaches).  While one is attached with scale != 0, cfgpp_unet_forward first runs
 * cn's forward on the same stream with the same z, t and rows (ControlNetModel.forward: `down_block_res_samples` and
 * `mid_block_res_sample`, each `* conditioning_scale`), then the UNet, whose skip connections and mid-block output receive
 * them (UNet2DConditionModel.forward: `down_block_additional_residuals` / `mid_block_additional_residual`) in one launch after
 * the mid block.  scale == 0 or no ControlNet: nothing extra is launched.  cn must match u's levels, channels, latent size
 * and max_rows; cn's context (set_context) must be set for the same rows, and a forward before its control image is set is an
 * error.  cfgpp_sample_graph_ddim refuses an engine with a ControlNet attached.  Synchronises the device. */
int cfgpp_unet_attach_control(cfgpp_unet* u, cfgpp_unet* cn, float scale);

/* LoRA: merge a low-rank update into one matrix of a FINALIZED engine, in place on the device, in the repacked layout the
 * kernels read: W(key) = fp16(float(base) + up x down), the product accumulated in fp32 and rounded once, `base` being the
 * weight finalize uploaded (saved device-to-device on the first merge into `key`, counted in cfgpp_unet_device_bytes, kept
 * until destroy - so every call starts from the same base and repeated merges do not drift).  key: a diffusers weight name of
 * the UNet (e.g. "down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_k.weight"); up [O][rank], down [rank][I * kh * kw]
 * (the checkpoint's own OIHW flattening), both fp32 on the device, with the adapters' scales (alpha / rank, user scale) folded
 * in by the caller and several adapters concatenated along the rank axis.  rank == 0 restores the base bit for bit.  Weight
 * addresses do not move: tile pins and captured graphs stay valid; after a change of attn2.to_k / to_v call
 * cfgpp_unet_set_context again (the cross-attention K / V^T are computed there).  Works on a ControlNet-mode engine too.
 * Refused (error naming the key, weight unchanged): conv_in.weight / conv_out.weight (fp32 small-kernel path), 1-D parameters,
 * unknown keys, rank < 0, an engine that is not finalized.  The entry point receives pointers and a rank only: the CALLER
 * guarantees that up holds O * rank and down rank * I * kh * kw floats for this key's weight (the Python binding checks the
 * shapes against the UNet's parameter table and refuses a mismatch by key).  Asynchronous on `stream`; up / down must stay
 * valid until the launch ran (stream-ordered allocations freed after the call are fine). */
int cfgpp_unet_lora(cfgpp_unet* u, const char* key, const float* up, const float* down, int rank, void* stream);

/* ---- IP-Adapter image prompts: two further entry points on a finalized UNet engine - load the adapter, set the image context -
 * are declared in include/cfgpp_ip_adapter.h, an extension header of this boundary, exported by the same library. */

/* Algorithmic FLOPs (2*MAC over conv/linear/attention matmuls) of one forward at `rows`.  When the most recent forward shared
 * the CFG prefix (rows == 2 * z_rows on a net without add_embedding: the ops before the first cross-attention ran once for
 * both halves), those ops count once - the figure is the work that was done. */
double cfgpp_unet_flops(cfgpp_unet* u, int rows);
/* Bytes of device memory held (weights + activations). */
double cfgpp_unet_device_bytes(cfgpp_unet* u);

/* ---- VAE engine: decoder (replaces `self.vae.decode(z / scale).sample`) and encoder ------
 * latent_diffusion.py:123-129 (scale 0.18215), latent_sdxl.py:155-164 (vae.config.scaling_factor).
 * Weights by diffusers AutoencoderKL keys (post_quant_conv.*, decoder.*).  img fp32 [B][3][8h][8w]. */
typedef struct cfgpp_vae cfgpp_vae;
cfgpp_vae* cfgpp_vae_create(int latent_h, int latent_w, int max_batch, float scaling_factor, int device_id);
void cfgpp_vae_destroy(cfgpp_vae* v);
int cfgpp_vae_load_tensor(cfgpp_vae* v, const char* key, const void* host, int dtype, const long* shape, int ndim);
int cfgpp_vae_finalize(cfgpp_vae* v);
int cfgpp_vae_decode(cfgpp_vae* v, const void* z, void* img, int B, void* stream);
/* decode + `(img / 2 + 0.5).clamp(0, 1)` of the solvers' sample() (latent_diffusion.py:676-677,
 * latent_sdxl.py:274-275) in the decoder's last kernel: img[B][3][8h][8w] fp32 in [0, 1]. */
int cfgpp_vae_decode_image(cfgpp_vae* v, const void* z, void* img, int B, void* stream);
/* Encoder (replaces `self.vae.encode(x).latent_dist.sample() * scale`, latent_diffusion.py:117-121,
 * latent_sdxl.py:150-153); available when every encoder.* and quant_conv.* tensor was loaded.
 * img [B][3][8h][8w] f32, noise [B][4][h][w] f32 or NULL (posterior mean), z [B][4][h][w] f32,
 * moments [B][8][h][w] f32 or NULL (mean | logvar clamped to [-30, 20]). */
int cfgpp_vae_encode(cfgpp_vae* v, const void* img, const void* noise, void* z, void* moments, int B, void* stream);
double cfgpp_vae_flops(cfgpp_vae* v, int B);
double cfgpp_vae_encode_flops(cfgpp_vae* v, int B);
double cfgpp_vae_device_bytes(cfgpp_vae* v);

/* ---- CLIP text transformer -------------------------------------------------------------------------
 * Replaces `self.text_encoder(tokens)` of the reference (latent_diffusion.py:105-113: last_hidden_state;
 * latent_sdxl.py:76-93: hidden_states[-2] / [-(clip_skip+2)] and the second tower's projected pooled output).  Once per
 * prompt, off the per-step path.  Geometry: hidden = heads * 64 (CLIP-L 768 / 12, OpenCLIP-bigG 1280 / 20), 77 tokens,
 * act 0 = quick_gelu, 1 = gelu, proj_dim 0 = no text_projection.  Keys of cfgpp_text_load_tensor = the `transformers`
 * CLIPTextModel(WithProjection) state dict ("text_model.embeddings.token_embedding.weight", ...,
 * "text_model.encoder.layers.<i>.self_attn.q_proj.weight", ..., "text_model.final_layer_norm.bias", "text_projection.weight").
 * Pinned against `transformers` on the MI355X (tests/test_gpu_text.py); the path `--model_dir` checkpoints take. */
typedef struct cfgpp_text cfgpp_text;
cfgpp_text* cfgpp_text_create(int vocab, int hidden, int layers, int heads, int intermediate, int act, int proj_dim,
                              int max_batch, int device_id);
void cfgpp_text_destroy(cfgpp_text* t);
int cfgpp_text_load_tensor(cfgpp_text* t, const char* key, const void* host, int dtype, const long* shape, int ndim);
int cfgpp_text_finalize(cfgpp_text* t);
/* ids: HOST int32 [B][77]; eos_pos: HOST int32 [B] (row that is pooled) or NULL; layer: -1 = last_hidden_state (final
 * LayerNorm applied), k in [0, layers] = hidden_states[k]; hidden_out: DEVICE fp16 [B][77][hidden]; pooled_out: DEVICE fp32
 * [B][proj_dim] or NULL. */
int cfgpp_text_encode(cfgpp_text* t, const int* ids, const int* eos_pos, int B, int layer, void* hidden_out, float* pooled_out,
                      void* stream);
double cfgpp_text_device_bytes(cfgpp_text* t);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_H */
