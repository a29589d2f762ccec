/* libcfgpp_hip.so - FreeU extension of the C ABI in include/cfgpp.h (same library, same conventions: 0 on success, < 0 with a
 * message in cfgpp_last_error()).
 *
 * Kept in its own header, like include/cfgpp_ip_adapter.h and include/cfgpp_long_prompt.h: include/cfgpp.h is the drop-in boundary
 * for the reference's seam and stays at its size; the reference has no counterpart for this (its users reach FreeU through
 * diffusers' UNet2DConditionModel.enable_freeu).
 */
#ifndef CFGPP_FREEU_H
#define CFGPP_FREEU_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* diffusers' enable_freeu(s1, s2, b1, b2) (enable != 0) / disable_freeu() (enable == 0) on a finalized UNet engine.  While it is on,
 * every forward edits the pair (hidden, skip) that each of the three resnets of up_blocks.0 (b1, s1) and up_blocks.1 (b2, s2)
 * concatenates, before the resnet reads it (apply_freeu / fourier_filter with threshold 1, FreeU "v1"):
 *     hidden[:, :C / 2] *= b                                  one fp16 rounding of h * b
 *     skip = Re(ifft2(mask * fft2(skip))), mask = s on the frequencies {-1, 0} x {-1, 0} and 1 elsewhere      fp32 sums, one rounding
 * as ONE extra launch per affected resnet (six per forward) on the tensors in place; the GroupNorm that follows takes its own
 * statistics where a tensor changed.  Off (the state after finalize) is the plain engine: the same launches, the same bits; values
 * (1, 1, 1, 1) run the kernel and reproduce those bits too.  Any time after cfgpp_unet_finalize; allocates nothing (the twiddle
 * tables of both levels are built by finalize); takes effect with the next forward / cfgpp_sample_graph_ddim, which never replays a
 * graph captured under another state.  Refused by name: an engine that is not finalized, a ControlNet-mode engine (out_channels =
 * 0: it has no up path), a non-finite value while enabling, a latent so small that up_blocks.0 runs on planes under 2 x 2. */
int cfgpp_unet_set_freeu(cfgpp_unet* u, float s1, float s2, float b1, float b2, int enable);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_FREEU_H */
