/* libcfgpp_hip.so - two-stage stochastic (DPM-Solver++ SDE, k-diffusion's sample_dpmpp_sde at r = 1/2) extension of the C ABI in
 * include/cfgpp.h (same library, same conventions as include/cfgpp_sde.h: 0 on success, < 0 with a message in cfgpp_last_error();
 * `stream` is a hipStream_t; nothing here allocates or synchronises; host arrays are read before the call returns).
 *
 * Kept in its own header, like include/cfgpp_sde.h: include/cfgpp.h is the drop-in boundary for the reference's seam.  The latent
 * is fp32 and one launch per UNet call does the guidance mix, the denoised estimates from the stage's base latent, the linear
 * combination, up to two noise terms (drawn in registers) and the next UNet call's fp16 input.  The job's first UNet input is
 * cfgpp_sde_input (include/cfgpp_sde.h).
 *
 * For r = 1/2 both stages of a step are linear in their inputs, so the kernel evaluates ONE fixed expression with host-made
 * coefficients (cfgpp_amd/dpmpp_sde.py: dpmpp_sde_coeffs); stage A, stage B, CFG and CFG++ are rows of one coefficient function:
 *     out = a_x x + a_d den + a_u uden + c_1 n1 + c_2 n2,      den / uden taken from `base` (x in stage A, stage A's out in stage B)
 *
 * ---- rounding contract (ours; no fma contraction) ------------------------------------------------------------------------------
 * fl() is one fp32 rounding, h() the RNE rounding to fp16 of a value that has ALREADY been rounded to fp32.  The model output m
 * (epsilon) is fp16; the guidance mix is the step kernels' (include/cfgpp.h):
 *     m_hat = h(m_uc + h(lam * h(m_c - m_uc)))          m_uc == m_c (the same pointer): m_hat is that tensor, bit for bit
 *     den   = fl(base - fl(sigma_b * m_hat))
 *     uden  = fl(base - fl(sigma_b * m_uc))             only where the a_u term is on
 *     last:      out = den
 *     otherwise: acc = fl(a_x * x)
 *                then, each only if its bit of `terms` is set, in this order:
 *                CFGPP_STAGE_D:   acc = fl(acc + fl(a_d * den))
 *                CFGPP_STAGE_U:   acc = fl(acc + fl(a_u * uden))
 *                CFGPP_STAGE_N1:  acc = fl(acc + fl(c_1 * n1))
 *                CFGPP_STAGE_N2:  acc = fl(acc + fl(c_2 * n2))
 *                out = acc
 *     den_out = den;   xc_out (if non-NULL) = h(fl(out * s_in))
 * A skipped term is not evaluated: its tensor is not read and its coefficient plays no part (no 0 * NaN).  With last != 0 x is
 * read only where it is base.
 *
 * ---- noise -------------------------------------------------------------------------------------------------------------------
 * The generator of include/cfgpp_lcm.h (Philox4x32-10 + Box-Muller, counter (q, 0, draw, stream_id)) with stream_id 3; 0, 1 and 2
 * stay the LCM renoise, the ancestral noise and the 2M / 3M SDE step noise.  n1 is the draw `draw1`, n2 the draw `draw2`.  The two
 * noise terms of a step cover overlapping intervals: stage A needs the path increment over [sigma, sigma_mid], stage B the one
 * over [sigma, sigma_next].  A host passes the SAME draw1 / draw2 (2 i, 2 i + 1 at step i) to both stages; stage A adds c_1 n1,
 * stage B c_1 n1 + c_2 n2 with c_1 : c_2 = sqrt(sigma - sigma_mid) : sqrt(sigma_mid - sigma_next), so both are normalised
 * increments of ONE Brownian path and nothing is kept between the stages: a counter-based generator draws n1 again for nothing.
 */
#ifndef CFGPP_DPMPP_SDE_H
#define CFGPP_DPMPP_SDE_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the bits of `terms` */
#define CFGPP_STAGE_D 1
#define CFGPP_STAGE_U 2
#define CFGPP_STAGE_N1 4
#define CFGPP_STAGE_N2 8

/* One stage of a DPM-Solver++ SDE step (CFG or CFG++) on fp32 latents [B][row_elems], by the expression sequence above.
 *     x, base, out, den_out, noise1, noise2: fp32 [B][row_elems]              m_uc, m_c, xc_out: fp16 [B][row_elems]
 *     coef_host[7] = {sigma_b, a_x, a_d, a_u, c_1, c_2, s_in}                 (host memory; every entry finite, used or not)
 *     terms: a mask of CFGPP_STAGE_*: which of the a_d, a_u, c_1, c_2 terms are added        last != 0: out = den, nothing else
 * base may be x (stage A).  out may be x (stage B in place; with base == x also stage A or the last step in place): every thread
 * reads its own elements before it writes them.  out must not be base when base is not x.  den_out must be neither x nor out; it
 * may be base where base is not x (stage B: the host lets D2 overwrite stage A's latent, which nothing reads afterwards, and keeps
 * stage A's den for its callback).  xc_out may be NULL.
 * noise1 / noise2: a device tensor each, or NULL: the values cfgpp_philox_normal(.., seeds_host, B, row_elems, draw1 | draw2, 3,
 * ..) would have written as fp32, generated in registers.  A term that is off, and every term with last != 0, draws and reads no
 * noise; where nothing is drawn seeds_host may be NULL.
 * Size rules are cfgpp_philox_normal's: row_elems % 4 == 0, 4 <= row_elems < 2^34, 1 <= B; more chains than one launch carries keys
 * for (32) take further launches keyed by their own seeds.  16-byte loads and stores (8-byte for fp16), no atomics.
 * Errors by name: a null pointer, out == base != x, den_out == x, den_out == out, B, row_elems, terms outside 0 .. 15, a non-finite
 * coefficient or lam, a noise term that has neither its tensor nor seeds_host. */
int cfgpp_step_sde_stage(const void* x, const void* base, void* out, void* den_out, void* xc_out, const void* m_uc, const void* m_c,
                         float lam, const float* coef_host, int terms, int last, const void* noise1, const void* noise2,
                         const unsigned long long* seeds_host, int B, long row_elems, unsigned draw1, unsigned draw2, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_DPMPP_SDE_H */
