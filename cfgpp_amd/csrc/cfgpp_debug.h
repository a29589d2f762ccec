/* libcfgpp_hip.so - test hooks and development switches.  NOT part of the drop-in boundary (include/cfgpp.h is):
 *   * cfgpp_op_*  : single kernels behind the C ABI so that tests/hip_ops.py can compare each one with an fp32 reference
 *                   and scripts/ can time / profile it alone;
 *   * cfgpp_*_set_* / cfgpp_igemm_force_* / cfgpp_igemm_timeline* : process-global A/B switches and diagnostics of the
 *                   launcher (measurement runs only: the defaults are what ships, nothing on the product path changes them).
 * Same conventions as include/cfgpp.h (device pointers, `void* stream`, int return + cfgpp_last_error()). */
#ifndef CFGPP_DEBUG_H
#define CFGPP_DEBUG_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- single ops, exposed for parity tests and micro-benchmarks ------------- */
int cfgpp_op_softmax_rows(void* s, long rows, int ncols, void* stream);
int cfgpp_op_conv_in_ex(const void* z, int z_is_half, void* out, const float* w, const float* bias,
                        int R, int zB, int Cin, int H, int W, int Cout, const float* pre_w, const float* pre_b,
                        float in_scale, void* stream);
/* stats: scratch of N*(1024*G*2 + G*2) floats (per-block {mean, M2} + mean/rstd); deterministic, no atomics */
int cfgpp_op_groupnorm(const void* src0, const void* src1, void* dst, const float* gamma, const float* beta,
                       float* stats, int N, int H, int W, int C0, int C1, int G, float eps, int silu,
                       int dst_padded, void* stream);
/* GroupNorm with the statistics taken from the PRODUCERS of src0 / src1 (round 5): gst0 / gst1 = [N*H*W / 32][C0 or C1][2] fp32
 * {mean, M2} per 32-pixel block and channel, written by the LDS-staged store epilogues of the implicit GEMM (IGemmArgs::gstat);
 * a finalize launch (N x G workgroups, Chan's parallel variance in a fixed order) + the apply launch.  stats: >= N*G*2 floats. */
int cfgpp_op_groupnorm_pre(const void* src0, const void* src1, void* dst, const float* gamma, const float* beta,
                           const float* gst0, const float* gst1, float* stats, int N, int H, int W, int C0, int C1, int G,
                           float eps, int silu, int dst_padded, void* stream);
/* test hook: the next cfgpp_op_igemm launches write those statistics of their output into buf (NULL = off);
 * cfgpp_op_igemm_gstat_written(): did the last one (0 for K-split launches / generic epilogues)? */
void cfgpp_op_igemm_set_gstat(void* buf);
int cfgpp_op_igemm_gstat_written(void);
/* 1 (default): the engines' GroupNorms take the producers' statistics whenever the producer wrote them; 0: always their own pass (A/B) */
void cfgpp_groupnorm_set_prestats(int on);
int cfgpp_groupnorm_prestats_enabled(void);
/* Shared CFG prefix of the UNet forward (csrc/unet.hip).  1 (default): a call with rows == 2 * z_rows on a net without
 * add_embedding whose first level has attention runs the plan ops between conv_in and the first cross-attention - whose inputs
 * are the same for rows r and r + z_rows - on z_rows rows, then one fan-out launch copies the three live tensors onto the upper
 * rows; 0: every op at `rows` (A/B).  Process-global, read by every forward / profile / graph capture. */
void cfgpp_unet_set_share_prefix(int on);
int cfgpp_unet_share_prefix_enabled(void);
/* number of plan ops a forward at (rows, z_rows) runs at rows / 2 as things stand (0: the call does not share - switch off,
 * rows != 2 * z_rows, or the net does not qualify: SDXL) */
int cfgpp_unet_shared_prefix_ops(cfgpp_unet* u, int rows, int z_rows);
/* development / A-B switch of the GroupNorm form: 0 auto, 1 always the two-launch form, 2 the one-launch
 * slab-in-registers kernel whenever the slab fits (csrc/norm_kernels.hip). */
void cfgpp_groupnorm_set_mode(int mode);
/* LayerNorm over the last axis: C % 8 == 0 and C <= 2048 (16-byte loads, the rows of a wave held in registers) */
int cfgpp_op_layernorm(const void* x, void* y, const float* gamma, const float* beta, long rows, int C,
                       float eps, void* stream);
/* development / A-B switch: token rows each wave of the LayerNorm kernel keeps in flight (0 = by row count, 1 / 2 / 4);
 * the result does not depend on it. */
void cfgpp_layernorm_set_rows_per_wave(int rpw);
/* test hooks: what the last call of each op in csrc/norm_kernels.hip dispatched, host-side records zeroed at entry to the op (a
 * refused call reports zeros).
 *   groupnorm (cfgpp_op_groupnorm / cfgpp_op_groupnorm_pre): out8 = {form (0 nothing launched, 1 slab kernel, 2 two launches,
 *     3 producer statistics), NT, MAXCH, gs, cpp of the slab instance (0 otherwise), pix_per_block and nblk of the stats launch
 *     (form 2), pix_per_block of the apply launch (forms 2 and 3)};
 *   layernorm: out2 = {MAXV, RPW} of the layernorm_kernel instance;  softmax_rows: out1 = {MAXC}. */
void cfgpp_groupnorm_last_launch(int* out8);
void cfgpp_layernorm_last_launch(int* out2);
void cfgpp_softmax_last_launch(int* out1);
/* V^T contract of cfgpp_op_attention: vt is [B*heads][dp][tok_pad] with the keys of every 32-key block
 * permuted - key k lives in column (k & ~12) | ((k & 4) << 1) | ((k & 8) >> 1) (bits 2 and 3 swapped), which is
 * how the QKV projection (cfgpp_op_igemm_heads) writes it; and when d % 32 != 0, row d of every matrix holds
 * ones (softmax denominator through the PV MFMA): call prepare_vt once on the zero-initialised buffer. */
int cfgpp_op_attention_prepare_vt(void* vt, int BH, int d, int tok_pad, void* stream);
int cfgpp_op_attention(const void* q, const void* k, const void* vt, void* o, int B, int heads, int d,
                       int nq, int nk, int q_tok_pad, int k_tok_pad, void* stream);
/* A/B switch for head dims padded to 64: 1 (default) the LDS-DMA kernel, 0 the register-staged kernel */
void cfgpp_attention_set_dma(int mode);
/* A/B knob of the LDS-DMA attention kernel: the workgroups sharing a CU start `sleeps` x 64 cycles apart per dispatch slot
 * (0 = together, the default) so that their QK^T / softmax / PV phases interleave instead of coinciding */
void cfgpp_attention_set_stagger(int sleeps);
/* A/B switch: 1 (default) attention with <= 128 keys and head dims padded to 64 (the 77-token cross-attention) runs the
 * resident-K/V single-pass kernel, 0 the flash loop */
void cfgpp_attention_set_cross(int on);
/* The UNet's cross-attention op.  Scope of xattn64_long_kernel (last_launch kernel 6: K / V^T resident in LDS, up to five 64-key
 * tiles, xqb blocks of 128 queries per workgroup, online softmax over the resident tiles): head dims padded to 64 with 129 <= nk <=
 * 320 keys (a text context of 2 .. 4 chunks of 77 tokens).  With the default switches the part of that scope where it measured
 * >= 3 % faster than the flash loop takes it: d = 40 / 48 at every key count, d = 56 / 64 at nk <= 192.  Every other shape (the rest of the scope, nk <= 128,
 * nk > 320, other head dims) is cfgpp_op_attention: same launch, same bits, same record.  Slots [nk, k_tok_pad) may hold anything
 * finite. */
int cfgpp_op_attention_cross(const void* q, const void* k, const void* vt, void* o, int B, int heads, int d,
                             int nq, int nk, int q_tok_pad, int k_tok_pad, void* stream);
/* A/B switch of cfgpp_op_attention_cross: 1 (default) the resident-K/V kernel for its measured classes, 0 the flash loop
 * everywhere, 2 the resident-K/V kernel for its whole scope (the kernel's tests, the A/B measurement) */
void cfgpp_attention_set_cross_long(int mode);
/* test hook: what the last cfgpp_op_attention call dispatched, a host-side record: out4 = {kernel (0 nothing launched: the call
 * was refused, 1 attn_kernel, 2 attn64_kernel, 3 xattn64_kernel, 4 xattn64_kernel IP form, 5 attn_ip_add_kernel, 6 xattn64_long_kernel,
 * 7 xattn64_region_kernel, 8 attn_region_rows_kernel, 9 attn_region_soft_kernel), D16 (16-wide k-steps of QK^T), ONES (1: the denominator comes
 * from the ones row of V^T), xqb (128-query blocks per workgroup of xattn64_kernel, 0 for the flash kernels)} */
void cfgpp_attention_last_launch(int* out4);
/* zero key slots [slot0, slot0 + n) of k [BH][tok_pad][dp] and of rows < d of vt [BH][dp][tok_pad] (the ones row stays) */
int cfgpp_op_attention_clear_slots(void* k, void* vt, int BH, int d, int tok_pad, int slot0, int n, void* stream);
/* Decoupled cross-attention of an IP-Adapter (diffusers IPAdapterAttnProcessor2_0.__call__: a second SDPA call over the image
 * tokens and `hidden_states + scale * ip_hidden_states`): o = fp16(softmax(q K_text) V_text + ip_scale * softmax(q K_img) V_img).
 * Buffers as cfgpp_op_attention, k_tok_pad >= 128: keys [0, nk_text) (nk_text <= 96) are text, keys [96, 96 + n_img)
 * (1 <= n_img <= 32) image tokens, all other slots pads that enter neither softmax; V^T permutation and ones row as above.
 * Head dims padded to 64: one launch (last_launch kernel 4 = xattn64_kernel, IP form).  Other head dims, or the A/B switches off:
 * cfgpp_op_attention over the text keys, then the image branch added in a second launch (kernel 5), rounding O_text to fp16
 * in between.  ip_scale == 0: the text-only call.  Refused, nothing launched: nk_text > 96, n_img > 32, k_tok_pad < 128. */
int cfgpp_op_attention_ip(const void* q, const void* k, const void* vt, void* o, int B, int heads, int d, int nq, int nk_text,
                          int n_img, float ip_scale, int q_tok_pad, int k_tok_pad, void* stream);
/* Regional cross-attention (include/cfgpp_regions.h): n_regions = 2 .. 4 prompts of 77 tokens in key slots [77 r, 77 r + 77) of
 * buffers laid out as for cfgpp_op_attention_cross (nk = 77 * n_regions); ids is a DEVICE uint8 [map_rows][q_tok_pad] with map_rows
 * = 1 or B and zero pads (never read past q_tok_pad), and query p of batch row b answers with softmax(q K_own) V_own over the 77
 * keys of region ids[b][p] alone.  Slots [77 * n_regions, k_tok_pad) may hold anything finite.  last_launch kernel 7
 * (xattn64_region_kernel: head dims padded to 64, K / V^T resident, online softmax started per lane at its first own key) or
 * kernel 8 (attn_region_rows_kernel: every other head dim, and dp = 64 under set_dma(0) / set_cross(0); one thread per row).
 * Refused by name, nothing launched: n_regions outside 2 .. 4, k_tok_pad < round_up(77 * n_regions, 64), map_rows not 1 or B,
 * null ids. */
int cfgpp_op_attention_region(const void* q, const void* k, const void* vt, void* o, int B, int heads, int d, int nq, int n_regions,
                              const void* ids, int map_rows, int q_tok_pad, int k_tok_pad, void* stream);
/* Soft regional cross-attention: buffers as for cfgpp_op_attention_region; w is a DEVICE fp32 [map_rows][n_regions][q_tok_pad] with
 * map_rows = 1 or B and zero pads, and query p of batch row b answers with
 *   o = fp16( sum_r w[b][r][p] / l_r * O_r ),   O_r = P_r V_r,  P_r = fp16(2^(s - m_r)),  l_r = sum of those fp16 P_r
 * over the regions r (ascending) with w != 0: every region's softmax is complete over its own keys [77 r, 77 r + 77) - scores from q
 * pre-scaled by d^-1/2 log2(e) and rounded to fp16, m_r their exact maximum - the sum runs in fp32 and the store is the one fp16
 * rounding.  A term with w == 0 is not evaluated: the keys and values of such a region, and the slots [77 * n_regions, k_tok_pad),
 * may hold anything finite.  One-hot weights give the hard partition of cfgpp_op_attention_region.  last_launch kernel 9
 * (attn_region_soft_kernel: an MFMA instance for every head dim cfgpp_op_attention has one for, regions streamed through LDS two
 * 64-key tiles at a time, a region no query of the workgroup weighs is skipped by a workgroup-wide vote), xqb 0.  Refused by name,
 * nothing launched: a head dim without an instance, n_regions outside 2 .. 4, k_tok_pad < 64 (n_regions + 1), map_rows not 1 or B,
 * null w. */
int cfgpp_op_attention_region_soft(const void* q, const void* k, const void* vt, void* o, int B, int heads, int d, int nq, int n_regions,
                                   const void* w, int map_rows, int q_tok_pad, int k_tok_pad, void* stream);
/* Perceiver attention of the IP-Adapter "plus" Resampler (include/cfgpp_ip_plus.h; csrc/resampler.hip), head dim 64:
 *   o[r][j][h*64 ..] = fp16( softmax_k(q[r][j][h] . k[r][k][h] / 8) v[r][k][h] ),  ONE softmax over the S keys of kv_x followed by the
 *   n_q keys of kv_l.
 * Token-major fp16 operands as the to_q / to_kv GEMMs store them, inner = heads * 64: q, o [rows][n_q][inner]; kv_x [rows][S][2 * inner]
 * and kv_l [rows][n_q][2 * inner] with K in columns [0, inner) and V in [inner, 2 * inner).  One kernel instance, one wave per (row,
 * head), 32-key tiles.  Refused by name, nothing launched: n_q outside 1 .. 32, S outside 1 .. 1024, a null operand. */
int cfgpp_op_perceiver_attention(const void* q, const void* kv_x, const void* kv_l, void* o, int rows, int heads, int n_q, int S,
                                 void* stream);
/* Self-attention of the CLIP image tower (include/cfgpp_vision.h; csrc/vision.hip), non-causal, head dims 64 / 80 / 104:
 *   o[r][t][h*d ..] = fp16( softmax_k(q[r][t][h] . k[r][k][h] / sqrt(d)) v[r][k][h] )        t, k over the T tokens of row r
 * Token-major fp16 operands as ONE fused QKV GEMM stores them, hidden = heads * d: qkv [rows][T][3 * hidden] with Q in columns
 * [0, hidden), K in [hidden, 2 hidden), V in [2 hidden, 3 hidden); o [rows][T][hidden].  One wave per (row, head, block of 32
 * queries), 32-key tiles; d = 104 zero-fills the upper half of its seventh 16-wide k-step on load (no padded buffer).  Refused by
 * name, nothing launched: d outside {64, 80, 104}, T outside 1 .. 320, a null operand.  cfgpp_op_attention is untouched by it. */
int cfgpp_op_attention_vit(const void* qkv, void* o, int rows, int heads, int d, int T, void* stream);
/* test hook: what the last cfgpp_op_attention_vit call (or a tower's attention launch) issued, a host-side record zeroed at entry
 * (a refused call reports zeros): out3 = {head dim of the instance, blocks of 32 queries per (row, head), 32-key tiles per block} */
void cfgpp_vit_attention_last_launch(int* out3);
/* the image front end of the tower, alone (cfgpp_vision_preprocess without an engine): img fp32 [N][3][H][W] in [0, 1] ->
 * pixels_out fp16 [N][3][S][S] */
int cfgpp_op_vit_preprocess(const float* img, int N, int H, int W, int S, void* pixels_out, void* stream);
/* the im2col rows of the tower's patch convolution: pixels fp16 [N][3][S][S] -> rows fp16 [N * (S / patch)^2][Kp],
 * rows[n * G * G + py * G + px][c * patch^2 + dy * patch + dx] = pixels[n][c][patch * py + dy][patch * px + dx], columns
 * 3 * patch^2 .. Kp - 1 zero.  Refused: S % patch != 0, Kp < 3 * patch^2. */
int cfgpp_op_vit_patch_rows(const void* pixels, void* rows, int N, int S, int patch, int Kp, void* stream);
/* The small kernels of the CLIP text tower (csrc/text.hip), the image tower (csrc/vision.hip) and the Resampler (csrc/resampler.hip),
 * each through the launcher its engine's plan calls (same checks, same launch geometry).  fp16 operands unless said otherwise; every
 * row width H is read and written in 16-byte units (H % 8 == 0).  Refused by name, nothing launched: a null operand, H % 8 != 0,
 * a count below 1, and what each entry says.
 *   text_embed      x[b * 77 + t][:] = fp16(float(tok[id]) + float(pos[t])), id = ids[b][t] clamped to [0, vocab); ids: DEVICE int32 [B][77]
 *   text_attention  causal self-attention over 77 tokens, head dim 64: qkv [B][77][3 H] (Q | K | V column blocks, head h at columns
 *                   64 h of each) -> out [B][77][H]; refused: H != 64 heads
 *   text_pool       out[b][:] = float(h[b][eos[b]][:]) with eos[b] clamped to [0, 77); h [B][77][H], eos: DEVICE int32 [B], out fp32 [B][H]
 *   act_inplace     x = fp16(act(x)) over n values (csrc/small_kernels.hip; the MLP activation of both towers): act 0 quick_gelu
 *                   x sigmoid(1.702 x), 1 gelu x / 2 (1 + erff(x / sqrt 2)); refused: n % 8 != 0, act outside {0, 1}
 *   vit_assemble    x[n][0] = cls + pos[0], x[n][1 + p] = patch[n][p] + pos[1 + p] (fp32 sum, rounded once); patch [N][T - 1][H],
 *                   cls [H], pos [T][H], x [N][T][H]; refused: T < 2
 *   vit_cls_rows    dst[n][:] = x[n][0][:]; x [N][T][H], dst [N][H]
 *   gelu_inplace    x = fp16(gelu(x)) over n values by common.h's gelu_erf_f (the Resampler's feed-forward; NOT act_inplace's erff)
 *   broadcast_rows  dst[r][:] = fp16(src[:]) for r < rows; src fp32 [n], dst [rows][n]; refused: n % 8 != 0 */
int cfgpp_op_text_embed(const int* ids, const void* tok, const void* pos, void* x, int B, int H, int vocab, void* stream);
int cfgpp_op_text_attention(const void* qkv, void* out, int B, int heads, int H, void* stream);
int cfgpp_op_text_pool(const void* h, const int* eos, float* out, int B, int H, void* stream);
int cfgpp_op_act_inplace(void* x, long n, int act, void* stream);
int cfgpp_op_vit_assemble(const void* patch, const void* cls, const void* pos, void* x, int N, int T, int H, void* stream);
int cfgpp_op_vit_cls_rows(const void* x, void* dst, int N, int T, int H, void* stream);
int cfgpp_op_gelu_inplace(void* x, long n, void* stream);
int cfgpp_op_broadcast_rows(const float* src, void* dst, long n, int rows, void* stream);
/* the [rows][n_img][cross_attention_dim] fp16 image tokens the last cfgpp_unet_image_context / cfgpp_unet_image_context_seq computed
 * (the output of the image projection, before the per-block to_k_ip / to_v_ip), copied to host_fp16_out.  rows must be the rows of
 * that call.  Error when no tokens were computed since the adapter was loaded.  Synchronises the device. */
int cfgpp_unet_ip_tokens(cfgpp_unet* u, void* host_fp16_out, int rows);
int cfgpp_op_conv_in(const void* z, int z_is_half, void* out, const float* w, const float* bias,
                     int R, int zB, int Cin, int H, int W, int Cout, void* stream);
/* conv_in of an inpaint UNet: input channels 0..Cz-1 from z (row r % zB), Cz..Cz+Cc-1 from the fp16 condition
 * [cond_rows][Cc][H][W] (row (r % zB) % cond_rows), Cz + Cc <= 16; w [9*(Cz+Cc)][Cout] fp32 (k = tap*Cin + ci).
 * cond = NULL is cfgpp_op_conv_in. */
int cfgpp_op_conv_in_cond(const void* z, int z_is_half, const void* cond, int cond_rows, int Cc, void* out, const float* w,
                          const float* bias, int R, int zB, int Cz, int H, int W, int Cout, void* stream);
/* conv_in_cond plus an fp16 addend in the output's layout [add_rows][H+2][W+2][Cout] (row (r % zB) % add_rows), added to the
 * fp16-rounded conv result and rounded again: the ControlNet's `sample = conv_in(sample) + controlnet_cond` (diffusers
 * ControlNetModel.forward).  addend = NULL is cfgpp_op_conv_in_cond bit for bit. */
int cfgpp_op_conv_in_add(const void* z, int z_is_half, const void* cond, int cond_rows, int Cc, const void* addend, int add_rows,
                         void* out, const float* w, const float* bias, int R, int zB, int Cz, int H, int W, int Cout, void* stream);
/* ControlNet conditioning-embedding convolution (diffusers ControlNetConditioningEmbedding conv_in / blocks.N): 3x3, pad 1,
 * stride 1 or 2, Ci, Co <= 256, w [9][Ci][Co] fp32 (tap-major), fp32 accumulation, fp16 output, silu = 1: F.silu after the fp16
 * rounding (rounded again).  in_kind 0: dense NHWC fp16 [R][Hi][Wi][Ci]; 1 / 2: NCHW fp16 / fp32 [R][Ci][Hi][Wi].  out_pad 0: dense
 * NHWC fp16 [R][Ho][Wo][Co]; 1: halo-padded NHWC [R][Ho+2][Wo+2][Co] (interior written).  Ho = (Hi - 1) / stride + 1. */
int cfgpp_op_cn_conv3x3(const void* in, int in_kind, void* out, int out_pad, const float* w, const float* bias, int R, int Ci, int Co,
                        int Hi, int Wi, int stride, int silu, void* stream);
/* the ControlNet residual add of the controlled UNet on n <= 32 tensor pairs in one launch: dst[i] = half(float(dst[i]) +
 * float(half(float(src[i]) * scale))) - torch's fp16 `s + r * scale` - over the interior of halo-padded NHWC fp16 tensors,
 * hwc[3 * i ..] = {H, W, C} of pair i (C % 8 == 0), `rows` rows.  dst / src: HOST arrays of device pointers (the table is
 * uploaded synchronously: test hook). */
int cfgpp_op_residual_add(void* const* dst, const void* const* src, const int* hwc, int n, int rows, float scale, void* stream);
/* halo-padded NHWC fp16 [rows][H+2][W+2][C] -> dense fp32 NCHW, each value multiplied by scale and rounded to fp16 first */
int cfgpp_op_residual_nchw(const void* src, float* out, int rows, int H, int W, int C, float scale, void* stream);
/* ControlNet test hook: residual i (0 .. n_down - 1 the down-block residuals in diffusers' order, n_down the mid-block
 * residual) of the last ControlNet forward, multiplied by `scale` and rounded to fp16 as the controlled UNet adds it, into a
 * dense fp32 NCHW buffer out [rows][C][H][W].  Returns the number of residuals when out is NULL. */
int cfgpp_controlnet_residual(cfgpp_unet* cn, int i, float scale, float* out, int rows, int* hwc_out, void* stream);

/* FreeU on one (hidden, skip) pair as the UNet's plan runs it (include/cfgpp_freeu.h; csrc/freeu_kernel.hip), in place on halo-padded
 * NHWC fp16 tensors [rows][H+2][W+2][C_h] / [..][C_s], ONE launch: hidden[:, :C_h / 2] = fp16(float(h) * b); skip = fp16(v + (s - 1) /
 * (H W) * low(v)), low = the four frequencies {-1, 0} x {-1, 0} of the plane as fp32 sums against host-made fp32 twiddles.  Only
 * interiors are read and written.  Either pointer may be NULL: that half of the job is not run.  Refused by name, nothing
 * launched: H or W < 2 (or > 1024), C_h / 2 or C_s not a multiple of 8, non-finite b / s, both pointers NULL.  (The twiddle table of
 * a plane size is uploaded synchronously on its first use: test hook.) */
int cfgpp_op_freeu(void* hidden, int C_h, void* skip, int C_s, int rows, int H, int W, float b, float s, void* stream);
/* test hook: what the last FreeU launch (cfgpp_op_freeu or a forward's) issued, a host-side record zeroed at entry (a refused call
 * reports zeros): out5 = {path (0 nothing launched, 1 skip slab resident in LDS, 2 two-phase: planes over 4096 pixels are re-read
 * from memory, 3 hidden half only), channels per skip slab, skip workgroups, hidden workgroups, dynamic LDS bytes} */
void cfgpp_freeu_last_launch(int* out5);

/* the CURRENT weight of matrix parameter `key` (base, or base + the adapters merged by cfgpp_unet_lora), read back from the
 * repacked device layout and un-repacked to checkpoint order: host_fp16_out holds [O][I][kh][kw] / [O][I] fp16.  Same keys and
 * refusals as cfgpp_unet_lora.  Synchronises the device. */
int cfgpp_unet_read_weight(cfgpp_unet* u, const char* key, void* host_fp16_out);

/* the raw words of the LCM noise generator (include/cfgpp_lcm.h; csrc/lcm_kernels.hip): out [n][4] uint32 on the device, 16-byte
 * aligned, out[i] = Philox4x32-10 of counter (ctr_host4[0] + i mod 2^32, ctr_host4[1], ctr_host4[2], ctr_host4[3]) under key
 * (key_host2[0], key_host2[1]); both arrays are host memory, read before the call returns.  1 <= n <= 2^24. */
int cfgpp_op_philox_raw(void* out, const unsigned* ctr_host4, const unsigned* key_host2, long n, void* stream);

/* per-launch timing of the VAE decoder (a diagnostic: scripts and HipVAE.profile; the UNet's twin cfgpp_unet_profile feeds the
 * benchmark and stays in include/cfgpp.h): one decode (image post-processing included) with a HIP event between every launch of the decoder plan; `detail` receives one
 * line per launch: index \t family (0 igemm, 1 attention GEMMs, 2 norm / softmax, 3 small) \t description \t us \t GFLOP */
int cfgpp_vae_profile(cfgpp_vae* v, const void* z, void* img, int B, void* stream, char* detail, long detail_cap);

/* quant_conv (1x1, 8->8) + DiagonalGaussian posterior on the encoder's 8-channel conv_out (fp32 NCHW). */
int cfgpp_op_vae_posterior(const float* conv_out, const float* qw, const float* qb, const float* noise, float* z,
                           float* moments, int B, int HW, float scale, void* stream);
int cfgpp_op_conv_out(const void* x, void* out, int out_is_half, const void* w, const float* bias,
                      int R, int H, int W, int C, int Cout, void* stream);
/* the same with `* post_scale + post_shift` and an optional clamp to [0, 1] applied to the fp32 result (the VAE
 * decoder's conv_out with the sampler's `(img / 2 + 0.5).clamp(0, 1)` folded in) */
int cfgpp_op_conv_out_ex(const void* x, void* out, int out_is_half, const void* w, const float* bias,
                         int R, int H, int W, int C, int Cout, float post_scale, float post_shift, int clamp01, void* stream);
/* A/B switch: 1 (default) conv_out on maps of >= 128 x 128 pixels runs the LDS-tiled kernel, 0 the wave-per-pixel kernel */
void cfgpp_conv_out_set_tiled(int on);
/* test hook: what the last cfgpp_op_conv_out / cfgpp_op_conv_out_ex call dispatched, a host-side record zeroed at entry (a refused
 * call reports zeros): out4 = {kernel (0 wave per pixel, 1 LDS-tiled), CO of the instance (3, 4 or 8), out_is_half, workgroups} */
void cfgpp_conv_out_last_launch(int* out4);
int cfgpp_op_sinusoid(const float* vals, float scalar, float* out, int count, int dim, int out_ld, int out_off,
                      void* stream);
/* out[m][n] = act_out(sum_k act_in(x[m][k]) W[n][k] + bias[n] + addend[m][n]); x fp32 with row stride ldx (0: one row for every
 * m), read in 16-byte units: x 16-byte aligned, K % 8 == 0 and ldx % 4 == 0 (refused otherwise); W [N][K] fp16; out fp32, row
 * stride ldo >= N, columns [N, ldo) untouched; bias / addend may be NULL */
int cfgpp_op_skinny_gemm(const float* x, int ldx, const void* w, const float* bias, const float* addend, int add_ld,
                         float* out, int ldo, int M, int N, int K, int silu_in, int silu_out, void* stream);
/* out[r][out_off + c] = float(in[r][c]), in [rows][cols] fp16 dense; refused: a null pointer, rows or cols <= 0, out_ld < out_off + cols */
int cfgpp_op_f16_to_f32_rows(const void* in, float* out, int rows, int cols, int out_ld, int out_off, void* stream);
/* the fan-out that ends the shared CFG prefix, alone: rows [0, h) of each p[k] ([>= 2h][row_elems[k]] fp16, 16-byte aligned,
 * row_elems[k] % 8 == 0) are copied onto rows [h, 2h); nseg <= 3.  p / row_elems: HOST arrays. */
int cfgpp_op_fanout_rows(void* const* p, const long* row_elems, int nseg, int h, void* stream);

/* Generic implicit GEMM (conv3x3 / conv1x1 / linear), see cfgpp_amd/csrc/igemm.h.
 * a0/a1: activation sources (C0/C1 channels), amode 0 linear rows, 1 halo-padded NHWC,
 * 2 padded stride-2, 3 padded nearest-2x upsample; w [N][taps*(C0+C1)] fp16 with K order channel-block major,
 * tap minor: k = (cb*taps + tap)*64 + c, cb = 64-channel block of the concatenated input;
 * epi 0 store (+bias +temb +resid), 1 GEGLU (packed weights).  omode/rmode: 0 linear, 1 padded.
 * amode 4 ("2x2 phase"): the upsample + conv3x3 of amode 3 as four 2x2 convolutions over the source map, one per output parity:
 * taps = 4, one source, H x W still the (even) OUTPUT size and M = rows * H * W, w = the folded weights of cfgpp_op_fold_upsample
 * ([4 phases][N][4 * C0]), epi 0 into a padded output (omode 1), no temb / resid, N % 8 == 0.  Rows are computed phase-outermost
 * (phase = 2 py + px, n, i, j): tap (a, b) reads padded source pixel (n, i + py + a, j + px + b), the row lands on padded output
 * pixel (n, 2i + py + 1, 2j + px + 1).  Tiles: every family but the one-wave-per-SIMD configs 24 - 26 / 28 and the 64 x 160 wave
 * tiles on 32-deep K-tiles (20 / 27), which report "did not run"; never K-split. */
int cfgpp_op_igemm(const void* a0, const void* a1, int C0, int C1, int taps, int amode, int H, int W,
                   const void* w, int M, int N, const float* bias, const float* temb, int temb_ld,
                   const void* resid, int rmode, int rld, void* out, int omode, int old_, int epi,
                   void* stream);
/* cfgpp_op_igemm plus ashift (amode 2: 0 = pad 1, 1 = pad (0,1,0,1)), out_scale (multiplies the accumulator before the bias) and
 * cfg_hint (the tuner's pin: bits 0-5 tile config, bits 6-7 tile walk) */
int cfgpp_op_igemm_ex(const void* a0, const void* a1, int C0, int C1, int taps, int amode, int H, int W,
                      const void* w, int M, int N, const float* bias, const float* temb, int temb_ld,
                      const void* resid, int rmode, int rld, void* out, int omode, int old_, int epi,
                      int ashift, float out_scale, int cfg_hint, void* stream);
/* w9: a conv3x3 weight in the repacked layout [O][I/64][9][64] fp16 (I % 64 == 0) -> w4 [4][O][I/64][4][64]: per output parity
 * (py, px) the 2x2 kernel whose taps are sums of 1, 2, 2 or 4 of the 3x3 taps (1-D: p = 0: a0 <- {t0}, a1 <- {t1, t2}; p = 1: a0 <-
 * {t0, t1}, a1 <- {t2}), summed in fp32 (t ascending, then s ascending) and rounded once */
int cfgpp_op_fold_upsample(const void* w9, void* w4, int O, int I, void* stream);
/* nearest-2x upsample + conv3x3 (+bias) of a padded Hs x Ws x C source into a padded 2Hs x 2Ws x N output, dispatched as the
 * engines' plan builder does: the 2x2 phase form (amode 4, reads w4) when the switch below is on and the source map is at least
 * 8 x 8, else the 9-tap amode-3 launch (reads w9) */
int cfgpp_op_upsample_conv3x3(const void* src, int C, int Hs, int Ws, const void* w9, const void* w4, int rows, int N,
                              const float* bias, void* out, void* stream);
/* 1 (default): plans built from now on run their upsampler convolutions in the 2x2 phase form; 0: the 9-tap form (A/B).  Read
 * when a plan is built (finalize), not per forward. */
void cfgpp_igemm_set_upsample_phase(int on);
/* test hooks: the A-operand mode of the last implicit-GEMM launch; 1 when that launch ran the tile config it was asked for (forced
 * or pinned), 0 when the config does not support the launch and another tile ran (cfgpp_igemm_last_launch says which).  A forced
 * config whose wave tiles have no GEGLU epilogue (3, 5, 7 - 9, 11 and their register-staged forms) refuses a GEGLU launch. */
int cfgpp_igemm_last_amode(void);
int cfgpp_igemm_last_config_ran(void);
/* QKV / KV projection with head-major scatter (EPI_HEADS) */
int cfgpp_op_igemm_heads(const void* a, int K, const void* w, int M, int N, const float* bias, int rows_per_batch,
                         void* hq, void* hk, void* hvt, int part0, int part_width, int head_dim, int heads,
                         int q_tok_pad, int tok_pad, void* stream);
/* the same with vt_linear: 1 = V^T columns in natural key order (the VAE), 0 = the attention kernel's permuted order */
int cfgpp_op_igemm_heads_ex(const void* a, int K, const void* w, int M, int N, const float* bias, int rows_per_batch,
                            void* hq, void* hk, void* hvt, int part0, int part_width, int head_dim, int heads,
                            int q_tok_pad, int tok_pad, int vt_linear, void* stream);
/* test hook: what the last implicit-GEMM launch ISSUED, after every fallback of the launcher - a host-side record, zeroed at the
 * entry of every launch (a refused call reports zeros).  out16 = {kernel family (1 igemm_kernel, 2 tile32_kernel, 3 igemm16_kernel,
 * 4 big4_kernel, 5 big4p_kernel), BM, BN, LDS stages, AMODE as instantiated, operand staging (1 LDS-DMA, 0 registers), grid,
 * ksplit (1 = whole tiles), n_major as finally set, walk_bn (0 = 1-D walk), par_nb, dynamic LDS bytes, producer statistics written,
 * epilogue variant (0 generic, 1 staged store, 2 staged GEGLU, 3 staged heads), waves along M, waves along N} */
void cfgpp_igemm_last_launch(int* out16);
/* 0 = heuristic, 1 = 128x128, 2 = 256x64, 3 = 64x64, 4 = 256x256, 5 = 256x320, 6 = 256x128, 7 = 128x160, 8 = 128x320,
 * 10 = 256x320 (waves along M); 9 / 11 = 128x160 on a 3- / 4-stage LDS ring, 12 = 128x128 and 14 = 256x128 on 3 stages;
 * 15 / 16 / 17 = 256x128 (8 waves) / 128x128 / 256x64 (4 waves) on 32-deep K-tiles and three stages, 2 - 3 workgroups per CU;
 * 13 / 20 = 256x256 / 256x320 on 32-deep K-tiles and FOUR stages (tile32_kernel);
 * 18 / 19 = 128x160 as 8 waves of 32x80 on the 16x16x32 MFMA, 3 / 4 stages (plain-store launches with N % 160 == 0);
 * 21..23 = register-staged 1..3 */
void cfgpp_igemm_force_config(int cfg);
void cfgpp_igemm_set_tail_split(int on);  /* 1 = K-split tiny grids with long K into fp32 partials + reduce (default 1); 2 = the
                                           * round-1 slice count (rounded up: a second partial round of workgroups), for A/B */
/* 8-wave 16x16x32-MFMA 128x160 tile for plain-store launches whose 128x160 grid is 200..256 tiles: 0 = off, 3 / 4 (default 4) =
 * on with that many LDS stages.  Rule-based (the tile sums k in a different order than the others, so the tuner never picks it). */
void cfgpp_igemm_set_mf16(int mode);
/* 1 (default): the rule also takes token-major linears; 0: convolutions only - the in-situ tuner then picks the linears' tile (A/B) */
void cfgpp_igemm_set_mf16_linear(int on);
/* 1 (default since round 3, validated on hardware): QKV / Q / KV projections (head-major epilogue) may use that tile too; 0: off */
void cfgpp_igemm_set_mf16_heads(int on);
/* A/B knob of that rule: also take grids of exactly 2 .. n full rounds of 256 tiles (default 2: the M = 16384 x N = 640 class;
 * 1 = one round of 200 .. 256 tiles only) */
void cfgpp_igemm_set_mf16_rounds(int n);
/* tile of the rule-based K-split launches: 14 (default) = 256x128 on 3 stages, 1 = 128x128 on 2 stages, 12 = 128x128 on 3 stages */
void cfgpp_igemm_set_split_tile(int cfg);
/* diagnostics: with a forced config, K-split every tile of a plain-store launch this many ways (0 = off) */
void cfgpp_igemm_force_split(int s);
/* big-tile K-split rule (M x N too small for 8-wave tiles to fill the chip, K long): least K-tiles (of 64) per slice for the
 * rule to fire; 0 = rule off (default - see csrc/igemm_kernel.hip).  Rule-based, so results never depend on tile tuning. */
void cfgpp_igemm_set_big_split(int min_kt);
/* tile walk of the implicit GEMM: -1 (default) by operand bytes / the tuner's pin, 0 always M-major, 1 always N-major; the
 * result does not depend on it */
void cfgpp_igemm_set_n_major(int mode);
/* 1 (default): launches whose round-by-round byte count says so take the XCD-blocked 2-D tile walk (IGemmArgs::walk_bn,
 * csrc/igemm_kernel.hip walk_plan); 0: the 1-D M- / N-major walks only (A/B).  Results do not depend on it. */
void cfgpp_igemm_set_blocked_walk(int on);
/* host-only probe of that choice (tests; no GPU): token GEMM M x N x K on BM x BN tiles, smem bytes of LDS per workgroup, the 1-D
 * default (n_major); out5 = {blocks along M (0: the 1-D walk stays), along N, tiles per block along M, along N, inner order} */
void cfgpp_igemm_walk_plan_probe(int M, int N, int K, int BM, int BN, int smem, int n_major, int* out5);
/* in-situ tuning candidates: bit c set = tile config c may be pinned (c = 1 .. 27; 24 - 26 = the one-wave-per-SIMD tiles of
 * big4_kernel.hip), bit 31 = the tile-walk stage runs.  Default 0xf1ffffff: everything but 25 / 26 / 27, which lose in situ
 * (profiles/r05/ab/) */
void cfgpp_igemm_set_tune_mask(unsigned mask);
/* all switches that change what the tuner measures or may pin (mask, big tiles, tail split, walk, staging, forced config),
 * folded into one word: pins are persisted only by a process whose word is still the default (cfgpp_amd/tune_cache.py) */
unsigned cfgpp_igemm_tuner_state(void);
/* 1 (default): on the first cfgpp_unet_forward / cfgpp_vae_decode at a batch size the engine times every igemm
 * launch of its plan in place (HIP events, a few extra forwards, one host sync) per candidate tile config and pins
 * the fastest; results are bit-identical across candidates, K-split launches stay rule-based.  0: fixed heuristic. */
void cfgpp_igemm_set_autotune(int on);
void cfgpp_igemm_set_big_tiles(int on);  /* 1 = allow the 8-wave 256x256 / 256x320 tiles (default) */
void cfgpp_igemm_set_staged_epilogue(int on); /* 1 = LDS-transposed row-coalesced store epilogue (default) */
void cfgpp_igemm_set_staging(int glds);   /* 1 = global_load_lds tiles (default), 0 = register staging */
/* diagnostics: per-workgroup timeline of ONE implicit-GEMM launch.  Arms the `target`-th launch (0-based) after this call:
 * every workgroup writes 16 x uint64 into buf[grid][16] (device memory, cap_blocks records): s_memtime at {entry, first
 * K-tile landed, k-loop done, stores done}, s_memrealtime (100 MHz) at {entry, exit}, HW_ID | XCC_ID << 32, s_memtime after
 * the first K-tile, s_memtime {before the first LDS-DMA is issued, after the prologue's DMAs are issued}.  buf = NULL disarms.  cfgpp_igemm_timeline_info: {tile id, grid, threads, BM, BN, LDS stages, K-split,
 * N-major walk, M, N, K, epilogue} of the recorded launch (scripts/igemm_timeline.py). */
void cfgpp_igemm_timeline(void* buf, long cap_blocks, int target);
void cfgpp_igemm_timeline_info(int* out12);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_DEBUG_H */
