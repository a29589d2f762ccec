/* libcfgpp_hip.so - v-prediction extension of the C ABI in include/cfgpp.h (same library, same conventions: 0 on success, < 0 with
 * a message in cfgpp_last_error(); `stream` is a hipStream_t; nothing here allocates or synchronises).
 *
 * Kept in its own header, like include/cfgpp_ip_adapter.h, include/cfgpp_long_prompt.h and include/cfgpp_freeu.h: include/cfgpp.h is
 * the drop-in boundary for the reference's seam and stays at its size; the reference runs epsilon models only.
 *
 * A v-prediction UNet returns v = a*eps - s*x0 at the noise level of its input z = a*x0 + s*eps (a = sqrt(alpha), s = sqrt(1-alpha)):
 *     x0 = a*z - s*v          eps = a*v + s*z
 * Guidance is applied to v; both maps are affine in v with the same z, so that is the same guidance as on eps.
 *
 * Rounding contract (ours; csrc/vpred_kernels.hip is compiled without fma contraction).  fl() is one fp32 rounding, h() the RNE
 * rounding to fp16 of a value that has ALREADY been rounded to fp32 - what torch does for an fp16 result.  v is fp16;
 *     v_hat = h(v_uc + h(lam * h(v_c - v_uc)))                                    the step kernels' guidance mix (include/cfgpp.h)
 * The coefficients arrive as fp32; the host (cfgpp_amd/coeffs.py: ddim_v_coeffs_pinned) pre-rounds to fp16 the ones torch-CPU would
 * round, exactly as it does for cfgpp_step_ddim.
 */
#ifndef CFGPP_VPRED_H
#define CFGPP_VPRED_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The generalised DDIM update for a v-prediction model, in place on z[n]; z0t_out[n] receives the x0 estimate.  The v-form twin of
 * cfgpp_step_ddim: no division, so alpha_t = 0 (a zero-terminal-SNR schedule's first step) is an ordinary input.
 *     coef_host[6] = {a_z, s_v, a_v, s_z, c3, c4}  (host memory, read before the call returns)
 *     A = tweedie_uc ? v_uc : v_hat ;  B = renoise_uc ? v_uc : v_hat
 *   fp32 latent (z_is_half == 0; z, z0t_out float):
 *     z0t  = fl(fl(a_z*z) - h(fl(s_v*A)))
 *     epsB = fl(h(fl(a_v*B)) + fl(s_z*z))
 *     z    = fl(fl(c3*z0t) + fl(c4*epsB))
 *   fp16 latent (z_is_half != 0; z, z0t_out fp16 - the inversion / edit flow): every operation rounds to fp16
 *     z0t  = h(h(a_z*z) - h(s_v*A)) ;  epsB = h(h(a_v*B) + h(s_z*z)) ;  z = h(h(c3*z0t) + h(c4*epsB))
 * Forward step from alpha_t to alpha_prev: a_z = a_v = sqrt(alpha_t), s_v = s_z = sqrt(1-alpha_t), c3 = sqrt(alpha_prev),
 * c4 = sqrt(1-alpha_prev); an inversion swaps the two levels, as it does for cfgpp_step_ddim.
 * row_scale: NULL, or float[n / row_elems] on the device (cfgpp_cfg_rescale): sample b's v_hat is replaced by h(fl(f_b * v_hat))
 * wherever v_hat is used (v_uc is never scaled); the factor stays fp32.  This is our contract, not a claim about torch's bits.
 * n % 4 == 0 and row_elems % 4 == 0 (row_elems > 0 and n % row_elems == 0 when row_scale is given); v_uc / v_c fp16 [n]. */
int cfgpp_step_ddim_v(void* z, void* z0t_out, const void* v_uc, const void* v_c, int z_is_half, float lam, const float* coef_host,
                      int tweedie_uc, int renoise_uc, const float* row_scale, long row_elems, long n, void* stream);

/* v -> eps for the k-diffusion loops, both CFG halves in one launch:  eps = h(h(a*v) + h(s*x)),  all tensors fp16 [n] (x_is_half
 * must be nonzero: the Karras-sigma loops keep fp16 latents).  x is the scaled UNet input (xc of cfgpp_kdiff_input),
 * a = 1/sqrt(sigma^2+1), s = sigma/sqrt(sigma^2+1).  eps_*_out may be v_* (in place), and the two halves may alias each other when the
 * caller passed one conditioning only.  After it cfgpp_step_kdiff / cfgpp_kdiff_denoise / cfgpp_lincomb run unchanged.  n % 4 == 0. */
int cfgpp_v_to_eps(void* eps_uc_out, void* eps_c_out, const void* v_uc, const void* v_c, const void* x, int x_is_half, float a, float s,
                   long n, void* stream);

/* diffusers' rescale_noise_cfg reduced to one factor per sample:  row_scale_out[b] = f_b, b < B,
 *     f_b = phi * std(v_c[b]) / std(v_hat[b]) + (1 - phi),      evaluated as fl(1 + fl(phi * fl(r_b - 1))), r_b = sqrt(M2_c / M2_hat)
 * std unbiased over the row_elems values of sample b; v_hat recomputed with the rounding above.  fp32 two-pass sums (mean, then
 * M2 = sum (x - mean)^2) by one workgroup per sample with a fixed reduction tree: no atomics, the same bits on every run.
 * f_b = 1 where M2_hat == 0.  1 <= B, row_elems % 4 == 0, 4 <= row_elems; v_uc / v_c fp16 [B][row_elems]. */
int cfgpp_cfg_rescale(const void* v_uc, const void* v_c, float lam, float phi, float* row_scale_out, int B, long row_elems, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_VPRED_H */
