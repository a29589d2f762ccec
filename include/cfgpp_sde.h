/* libcfgpp_hip.so - stochastic multistep (DPM-Solver++ 2M / 3M SDE) extension of the C ABI in include/cfgpp.h (same library, same
 * conventions as include/cfgpp_lcm.h: 0 on success, < 0 with a message in cfgpp_last_error(); `stream` is a hipStream_t; nothing here
 * allocates or synchronises; host arrays are read before the call returns).
 *
 * Kept in its own header, like include/cfgpp_lcm.h: include/cfgpp.h is the drop-in boundary for the reference's seam, and the
 * reference has no stochastic multistep sampler, so there is no reference arithmetic to mirror: the latent is fp32 and one launch
 * per sampling step does the guidance mix, both denoised estimates, the multistep combination, the noise (drawn in registers), the
 * history write and the next step's fp16 UNet input.
 *
 * The update of both solvers is linear in its inputs, so the kernel evaluates ONE fixed expression with host-made coefficients
 * (cfgpp_amd/sde.py: sde_coeffs); "2M midpoint", "2M heun", "3M", CFG and CFG++ are rows of one coefficient function.
 *
 * ---- rounding contract (ours; no fma contraction) ------------------------------------------------------------------------------
 * fl() is one fp32 rounding, h() the RNE rounding to fp16 of a value that has ALREADY been rounded to fp32.  The model output m
 * (epsilon) is fp16; the guidance mix is the step kernels' (include/cfgpp.h):
 *     m_hat = h(m_uc + h(lam * h(m_c - m_uc)))          m_uc == m_c (the same pointer): m_hat is that tensor, bit for bit
 *     den   = fl(x - fl(sigma * m_hat))                 uden = fl(x - fl(sigma * m_uc))         (uden: only where it is used)
 *     last:      x' = den
 *     otherwise: acc = fl(a_x * x)
 *                acc = fl(acc + fl(a_d * den))
 *                cfgpp:        acc = fl(acc + fl(a_u * uden))
 *                n_hist >= 1:  acc = fl(acc + fl(a_1 * hist1))
 *                n_hist == 2:  acc = fl(acc + fl(a_2 * hist2))
 *                a_n != 0:     acc = fl(acc + fl(a_n * noise))
 *                x' = acc
 *     den_out = den;   hist_out (if non-NULL) = cfgpp ? uden : den;   xc_out (if non-NULL) = h(fl(x' * s_in_next))
 * A skipped term is not evaluated: its tensor is not read and its coefficient plays no part (no 0 * NaN).
 *
 * ---- noise -------------------------------------------------------------------------------------------------------------------
 * The generator of include/cfgpp_lcm.h (Philox4x32-10 + Box-Muller, counter (q, 0, draw, stream_id)) with stream_id 2; 0 and 1 stay
 * the LCM renoise and the ancestral noise.  The intervals of successive steps do not overlap, so independent standard normals per
 * step (draw = step index) have exactly the law of a Brownian path's increments over them.
 */
#ifndef CFGPP_SDE_H
#define CFGPP_SDE_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* xc[i] = h(fl(x[i] * s_in)), i < n: the fp16 UNet input of step 0 of a job (every later step's comes out of cfgpp_step_sde).
 * x fp32, xc fp16, 1 <= n; x 16-byte and xc 8-byte aligned; s_in finite. */
int cfgpp_sde_input(const void* x, void* xc, float s_in, long n, void* stream);

/* One DPM-Solver++ 2M / 3M SDE step (CFG or CFG++), in place on the fp32 latent x [B][row_elems], by the expression sequence above.
 *     x, den_out, hist1, hist2, hist_out, noise: fp32 [B][row_elems]          m_uc, m_c, xc_out: fp16 [B][row_elems]
 *     coef_host[8] = {sigma, a_x, a_d, a_u, a_1, a_2, a_n, s_in_next}         (host memory; every entry finite, used or not)
 *     cfgpp != 0: the a_u term is added and the history holds uden            n_hist in 0 .. 2: how many history terms are added
 *     last != 0: x' = den, no combination, no noise
 * hist1 / hist2: the previous / the one-before-previous history value; needed (non-NULL) for n_hist >= 1 / == 2, else not read.
 * hist_out and xc_out may be NULL.  hist_out may be the same buffer as hist2 (or hist1): every thread reads its own elements before
 * it writes them, so a host can rotate its history buffers without a copy.  den_out must not be x.
 * noise: a device tensor, or NULL: the values cfgpp_philox_normal(.., seeds_host, B, row_elems, draw, 2, ..) would have written as
 * fp32, generated in registers.  last != 0 or a_n == 0 draws and reads no noise, and seeds_host may then be NULL.
 * Size rules are cfgpp_philox_normal's: row_elems % 4 == 0, 4 <= row_elems < 2^34, 1 <= B; more chains than one launch carries keys
 * for (32) take further launches keyed by their own seeds.  16-byte loads and stores (8-byte for fp16), no atomics.
 * Errors by name: a null pointer, B, row_elems, n_hist outside 0 .. 2, a history pointer missing for n_hist, a non-finite
 * coefficient or lam, den_out == x, a step that needs noise and has neither noise nor seeds_host. */
int cfgpp_step_sde(void* x, void* den_out, void* xc_out, const void* hist1, const void* hist2, void* hist_out, const void* m_uc,
                   const void* m_c, float lam, const float* coef_host, int cfgpp, int n_hist, int last, const void* noise,
                   const unsigned long long* seeds_host, int B, long row_elems, unsigned draw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_SDE_H */
