/* libcfgpp_hip.so - MultiDiffusion panorama extension of the C ABI in include/cfgpp.h (same library, same conventions: 0 on
 * success, < 0 with a message in cfgpp_last_error(); `stream` is a hipStream_t; nothing here allocates or synchronises).
 *
 * Kept in its own header, like include/cfgpp_lcm.h and include/cfgpp_vpred.h: include/cfgpp.h is the drop-in boundary for the
 * reference's seam and stays at its size; the reference has no sampler for latents larger than the UNet's window.
 *
 * MultiDiffusion (Bar-Tal et al., "MultiDiffusion: Fusing Diffusion Paths for Controlled Image Generation", ICML'23; diffusers'
 * StableDiffusionPanoramaPipeline): the panorama latent [B][C][Hp][Wp] is cut into V overlapping windows of the UNet's size
 * h x w ("views"); every view takes an ordinary denoising step and the results are averaged where views overlap.
 *
 * ---- view geometry (latent units) --------------------------------------------------------------------------------------------
 *     nbh = Hp > h ? (Hp - h) / stride + 1 : 1
 *     nbw = Wp > w ? (circular ? Wp / stride : (Wp - w) / stride + 1) : 1            V = nbh * nbw
 *     view v: y0 = (v / nbw) * stride, x0 = (v % nbw) * stride; it covers rows y0 .. y0 + h - 1 and columns x0 .. x0 + w - 1,
 *     the columns taken mod Wp when circular.
 * Refused by name (nothing is left uncovered, nothing is read out of bounds): Hp < h, Wp < w; stride, w or Wp not a multiple of 4
 * (16-byte vectors); stride > h or stride > w; (Hp - h) % stride != 0; (Wp - w) % stride != 0 without circular; Wp % stride != 0
 * with circular; V % chunk_views != 0.
 *
 * ---- buffers -------------------------------------------------------------------------------------------------------------------
 *     z_pano, z0t_pano   fp32 [B][C][Hp][Wp]
 *     z_views            fp32 [V * B][C][h][w], row = v * B + b.  Chunk k = rows k * Vc * B .. (k + 1) * Vc * B - 1, Vc = chunk_views:
 *                        a contiguous slice, which is what cfgpp_unet_forward takes as `z` with z_rows = Vc * B
 *     eps                fp16 [V / Vc][2 * Vc * B][C][h][w]: chunk k is that forward's eps_out - the Vc * B unconditional rows first,
 *                        then the Vc * B conditional rows, each in the order of the chunk's z rows
 * All 16-byte aligned.
 *
 * ---- rounding contract of the step (ours; no fma contraction) ------------------------------------------------------------------
 * fl() is one fp32 rounding.  For a panorama element p with covering views v_1 < v_2 < .. < v_n (ascending view index) let
 * (z0_i, zn_i) be cfgpp_step_ddim's results (eps_is_half = 1: include/cfgpp.h) for the inputs z = z_pano[p] and view v_i's eps_uc /
 * eps_c at the element's window-local position.  Then
 *     sum  = zn_1;  sum = fl(sum + zn_2);  ..  fl(sum + zn_n)             z_pano[p]   = sum / float(n)      IEEE division
 *     sum0 = z0_1;  ..                                                     z0t_pano[p] = sum0 / float(n)
 * n = 1 divides by 1: the result is cfgpp_step_ddim's, bit for bit.
 */
#ifndef CFGPP_PANORAMA_H
#define CFGPP_PANORAMA_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct cfgpp_pano_views {
    int B, C;            /* chains, latent channels */
    int Hp, Wp;          /* panorama latent size */
    int h, w;            /* window (the UNet's latent size) */
    int stride;          /* distance between view origins, both directions */
    int circular;        /* != 0: views wrap around the panorama's width */
    int chunk_views;     /* Vc: views per UNet forward */
} cfgpp_pano_views;

/* z_views[v * B + b][c][y][x] = z_pano[b][c][y0_v + y][(x0_v + x) mod Wp]: the windows of the panorama, one launch.  Once per job,
 * and again when the caller has edited z_pano (cfgpp_step_ddim_views keeps z_views current itself). */
int cfgpp_views_gather(const cfgpp_pano_views* views, const void* z_pano, void* z_views, void* stream);

/* One DDIM / DDIM-CFG++ step of every view, the overlap average and the next step's UNet inputs, in ONE launch.  lam, c1 .. c4,
 * tweedie_uc, renoise_uc: as cfgpp_step_ddim's (the sign of c2 included).  A thread owns four consecutive panorama columns: it reads
 * z_pano there, finds the covering views arithmetically, evaluates the update above per view, writes z_pano (in place) and
 * z0t_pano, and scatters the new z_pano value into every covering view's slot of z_views - each element of z_views has exactly one
 * source, so there are no conflicts and no atomics.  16-byte loads and stores (8-byte for eps). */
int cfgpp_step_ddim_views(const cfgpp_pano_views* views, void* z_pano, void* z0t_pano, void* z_views, const void* eps, float lam,
                          float c1, float c2, float c3, float c4, int tweedie_uc, int renoise_uc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_PANORAMA_H */
