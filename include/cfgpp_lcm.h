/* libcfgpp_hip.so - latent-consistency (LCM) extension of the C ABI in include/cfgpp.h (same library, same conventions: 0 on
 * success, < 0 with a message in cfgpp_last_error(); `stream` is a hipStream_t; nothing here allocates or synchronises).
 *
 * Kept in its own header, like include/cfgpp_vpred.h and include/cfgpp_freeu.h: include/cfgpp.h is the drop-in boundary for the
 * reference's seam and stays at its size; the reference has no few-step consistency sampler.
 *
 * ---- the generator (ours; NOT torch's device stream) -------------------------------------------------------------------------
 * Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
 * key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.  For element group q (elements 4q .. 4q+3) of chain b's row:
 *     key     = (seed_b & 0xffffffff, seed_b >> 32)              seed_b: the chain's 64-bit seed
 *     counter = (q, 0, draw, stream_id)                          draw: step / noise-draw index; stream_id 0: LCM renoise, 1: ancestral
 * The four outputs r0 .. r3 make two Box-Muller pairs, (r0, r1) -> elements 4q, 4q+1 and (r2, r3) -> elements 4q+2, 4q+3:
 *     u1 = ((r_even >> 8) + 1) * 2^-24   in (0, 1]               u2 = (r_odd >> 8) * 2^-24   in [0, 1)       both exact in fp32
 *     rho = fl(sqrtf(fl(-2 * logf(u1))))                         (s, c) = sincospif(fl(2 * u2))              2 * u2 is exact
 *     element 4q (4q+2) = fl(rho * c)                            element 4q+1 (4q+3) = fl(rho * s)
 * logf, sqrtf and sincospif are the ACCURATE device functions (OCML __ocml_log_f32, correctly rounded sqrt, __ocml_sincospi_f32),
 * never the fast intrinsics (__logf, __sinf, __cosf); csrc/lcm_kernels.hip is compiled without fma contraction and without fast-math.
 * The integer part is exact (known-answer vectors in tests/test_lcm_cpu.py); u1 >= 2^-24, so |value| <= sqrt(48 ln 2) < 5.78.
 * A chain's values depend on (seed_b, q, draw, stream_id) only: not on the batch it runs in, not on the row index, not on the launch.
 *
 * ---- rounding contract of the step (ours; no fma contraction) ----------------------------------------------------------------
 * fl() is one fp32 rounding, h() the RNE rounding to fp16 of a value that has ALREADY been rounded to fp32.  The model output m is
 * fp16; the guidance mix is the step kernels' (include/cfgpp.h):  m_hat = h(m_uc + h(lam * h(m_c - m_uc))).
 */
#ifndef CFGPP_LCM_H
#define CFGPP_LCM_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out[b][i], b < B, i < row_elems = the normals defined above for seed seeds_host[b] (host memory, read before the call returns).
 * out_is_half == 0: float; != 0: fp16, h() of the fp32 value.  row_elems % 4 == 0, 4 <= row_elems < 2^34, 1 <= B; out 16-byte
 * (fp16: 8-byte) aligned.  One Philox block per 4-element group, one 16-byte (8-byte) store per group. */
int cfgpp_philox_normal(void* out, int out_is_half, const unsigned long long* seeds_host, int B, long row_elems, unsigned draw,
                        unsigned stream_id, void* stream);

/* One LCM (multistep consistency) step, in place on the fp32 latent z [B][row_elems]; den_out [B][row_elems] fp32 receives the
 * boundary-conditioned x0 estimate ("denoised").  m_uc / m_c: the UNet's fp16 outputs; m_uc == m_c is the single-forward case
 * (m_hat is then that tensor, bit for bit).
 *     coef_host[8] (host memory, read before the call returns):
 *       pred_v == 0 (epsilon model):  {c1, c2, c_out, c_skip, c3, c4, -, -}    c1, c2 as cfgpp_step_ddim's, the sign of c2 included
 *       pred_v != 0 (v model):        {s_v, a_z, c_out, c_skip, c3, c4, -, -}  s_v, a_z as cfgpp_step_ddim_v's
 *       entries 6 and 7 are reserved and ignored.
 *     x0   = div(fl(z - h(fl(m_hat * c1))), c2)              pred_v == 0: cfgpp_step_ddim's expression with eps_is_half = 1
 *                                                            (div: c2 > 0 IEEE division, c2 < 0 multiply by -c2)
 *     x0   = fl(fl(a_z * z) - h(fl(s_v * m_hat)))            pred_v != 0: cfgpp_step_ddim_v's expression
 *     den  = fl(fl(c_out * x0) + fl(c_skip * z))
 *     z    = last ? den : fl(fl(c3 * den) + fl(c4 * noise))
 * c_skip / c_out: the consistency boundary scalings; c3 = sqrt(alpha_prev), c4 = sqrt(1 - alpha_prev) of the NEXT timestep.
 * noise: a device fp32 tensor [B][row_elems], or NULL: the values cfgpp_philox_normal(.., seeds_host, B, row_elems, draw, 0, ..)
 * would have written as fp32, generated in registers (no launch, no memory traffic of their own); seeds_host may be NULL when
 * noise is given or last != 0.  last != 0 draws and reads no noise.  Same size rules as cfgpp_philox_normal; 16-byte loads and
 * stores, no atomics. */
int cfgpp_step_lcm(void* z, void* den_out, const void* m_uc, const void* m_c, float lam, const float* coef_host, int pred_v, int last,
                   const void* noise, const unsigned long long* seeds_host, int B, long row_elems, unsigned draw, void* stream);

/* ---- guidance-embedded UNets (the distilled LCM checkpoints: UNet2DConditionModel with time_cond_proj_dim = dim) ---------------
 * Before cfgpp_unet_finalize, like cfgpp_unet_set_max_tokens (cfgpp_unet_config is ABI and stays as it is): the engine then expects
 * the extra parameter time_embedding.cond_proj.weight [block_out_channels[0]][dim] (no bias) and computes
 *     emb = linear_2(silu(linear_1(sinusoid(t) + cond_proj(w_emb))))
 * in fp32 like the rest of the time MLP.  dim: a multiple of 8 in 8 .. 4096.  Errors by name: after finalize, a second call, a
 * ControlNet-mode engine. */
int cfgpp_unet_set_time_cond(cfgpp_unet* u, int dim);

/* Once per job: w_emb_host[dim] (host memory, read before the call returns) is diffusers' get_guidance_scale_embedding of the job's
 * guidance scale, one vector for every row.  Two skinny-GEMM launches on `stream` compute
 *     time_add = linear_1.weight x (cond_proj.weight x w_emb)                       fp32 accumulation, fp16 weights
 * into an engine-owned buffer whose address never changes (a captured graph stays valid, like the image condition's); every later
 * forward's linear_1 launch takes it as its addend, which lands before the SiLU: by linearity that is linear_1(sinusoid + cond_proj
 * (w_emb)), and a forward of such an engine runs exactly the launches of a plain one.  The time path stays one row, so the shared CFG
 * prefix is unaffected.  A forward (profile, graph capture) of such an engine before this call is an error by name; so is this call
 * on an engine without cfgpp_unet_set_time_cond or before finalize, and a non-finite w_emb. */
int cfgpp_unet_guidance_embedding(cfgpp_unet* u, const float* w_emb_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_LCM_H */
