/* libcfgpp_hip.so - long-prompt extension of the C ABI in include/cfgpp.h (same library, same conventions: 0 on success, < 0 with
 * a message in cfgpp_last_error()).
 *
 * Kept in its own header, like include/cfgpp_ip_adapter.h: include/cfgpp.h is the drop-in boundary for the reference's seam and
 * stays at its size (40 entry points, its cap); the reference cuts every prompt at 77 tokens and has no counterpart for this.
 */
#ifndef CFGPP_LONG_PROMPT_H
#define CFGPP_LONG_PROMPT_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The longest text context the engine accepts: 77 * j tokens with j = 1 .. 4 (77, the default, 154, 231, 308) - a prompt's
 * 75-id chunks, each encoded as a 77-token CLIP context and concatenated along the token axis (cfgpp_amd/prompt.py).  Before
 * cfgpp_unet_finalize only, refused afterwards: finalize sizes the cross-attention K / V^T buffers of every block for it -
 * max(128, round_up(max_tokens, 64)) key slots, counted in cfgpp_unet_device_bytes - and nothing is allocated later.
 * cfgpp_unet_set_context then takes tokens = 77 * j <= max_tokens (anything else is refused with both numbers), and an engine built
 * for more computes, on a 77-token context, the bits of a default engine - also after a longer context: the key slots behind the
 * current context keep what the longer one wrote, finite values that every attention kernel on the path masks or never loads.
 * Head dims padded to 64 run contexts of 154 .. 308 tokens on a kernel of their own (xattn64_long_kernel: K / V^T resident in LDS).
 * A ControlNet-mode engine takes the same call, and must be given the max_tokens of the UNet it is attached to.  An engine with
 * max_tokens > 77 refuses an IP-Adapter by name: its image slots sit at key 96 of the 128-slot buffers. */
int cfgpp_unet_set_max_tokens(cfgpp_unet* u, int max_tokens);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_LONG_PROMPT_H */
