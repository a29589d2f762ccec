/* libcfgpp_hip.so - image-to-image / latent hires-fix extension of the C ABI in include/cfgpp.h (same library, same conventions as
 * include/cfgpp_sde.h: 0 on success, < 0 with a message in cfgpp_last_error(); `stream` is a hipStream_t; nothing here allocates,
 * synchronises or uses atomics; host arrays are read before the call returns).
 *
 * Kept in its own header, like include/cfgpp_sde.h: include/cfgpp.h is the drop-in boundary for the reference's seam, and the
 * reference starts every job from noise.  An image-to-image job starts from a source latent z, possibly of a smaller size (latent
 * hires fix), forward-noised to the first timestep / sigma the loop runs:  x = a * resample(z) + s * n.  That start is ONE launch
 * - the resample, the noise (given, or drawn in registers), both products, the sum and the cast - and the sampling loops and step
 * kernels run on its output unchanged.
 *
 * ---- resample ------------------------------------------------------------------------------------------------------------------
 * mode 0 identity (h0 == h, w0 == w), 1 nearest-exact, 2 bilinear, 3 bicubic (Keys' kernel, A = -0.75): the conventions of torch's
 * F.interpolate(size=(h, w), align_corners=False) without antialiasing.  Upscaling only, h0 <= h and w0 <= w (there torch's
 * antialiased bilinear kernel coincides with the plain one; its antialiased bicubic is another kernel, A = -0.5, and is not built).
 * Source coordinates are exact integer rationals: for output index d of an axis of `out` elements over `in` source elements
 *     coordinate = num / den,   num = (2 d + 1) in - out,   den = 2 out;        q = floor(num / den),  t = (num - q den) / den
 *     nearest-exact: tap min(floor((2 d + 1) in / (2 out)), in - 1)
 *     bilinear:      num < 0: q = 0, t = 0;   taps q, min(q + 1, in - 1);   weights 1 - t, t
 *     bicubic:       taps clamp(q - 1 + k, 0, in - 1), k = 0 .. 3;   weights W2(t + 1), W1(t), W1(1 - t), W2(2 - t),
 *                    W1(u) = ((A + 2) u - (A + 3)) u u + 1,   W2(u) = ((A u - 5 A) u + 8 A) u - 4 A
 * Tap indices are exact.  Each weight is evaluated in fp64 from the exact integers (1 - t as (den - rem) / den) and rounded ONCE to
 * fp32.  torch's fp32 kernels carry the coordinate itself in fp32, so they agree with this to a few ulp, not bit for bit.
 *
 * ---- rounding contract (ours; no fma contraction) ------------------------------------------------------------------------------
 * fl() is one fp32 rounding, h() the RNE rounding to fp16 of a value that has ALREADY been rounded to fp32.  v is the source value
 * as fp32 (an fp16 source converts exactly).  The resample is separable, rows inside columns, as torch's CPU kernel nests it; with
 * the taps of an axis in ascending k:
 *     identity, nearest-exact:   r = v[tap_y][tap_x]                                   (no arithmetic)
 *     row(j)  = fl(wx_0 v[j][x_0]);   row(j) = fl(row(j) + fl(wx_k v[j][x_k])),  k = 1 ..        (j: a y tap)
 *     r       = fl(wy_0 row(y_0));    r      = fl(r      + fl(wy_k row(y_k))),   k = 1 ..
 *     both terms:   x' = fl(fl(a r) + fl(s n))        a == 0:   x' = fl(s n)        s == 0:   x' = fl(a r)
 *     x = x' (fp32 x)   or   h(x') (fp16 x)
 * A term whose coefficient is 0 is not evaluated: its tensor is not read (no 0 * NaN) and may be NULL.  Mode 0 with an fp32 x is
 * therefore torch's  a * z.float() + s * noise  bit for bit (cfgpp_amd/inpaint.py: _prepare_job).
 *
 * ---- noise -------------------------------------------------------------------------------------------------------------------
 * The generator of include/cfgpp_lcm.h (Philox4x32-10 + Box-Muller, counter (q, 0, draw, stream_id)) with stream_id 4, draw 0; 0 .. 3
 * stay the LCM renoise, the ancestral noise, the 2M / 3M SDE step noise and the DPM++ SDE path increments.  Keyed per chain, so
 * chain b of a batch starts where chain b alone starts.
 */
#ifndef CFGPP_IMG2IMG_H
#define CFGPP_IMG2IMG_H
#include "cfgpp.h"
#ifdef __cplusplus
extern "C" {
#endif

/* x[b] = a * resample(src[src_rows == 1 ? 0 : b]) + s * n[b], b < B, by the expression sequence above.
 *     x:     [B][C][h][w], fp32 (x_half == 0, 16-byte aligned) or fp16 (x_half != 0, 8-byte aligned)
 *     src:   [src_rows][C][h0][w0], fp32 or fp16 (src_half); src_rows is 1 (broadcast to every chain) or B; must not overlap x
 *     noise: fp32 [B][C][h][w] (16-byte aligned), or NULL: the values cfgpp_philox_normal(.., seeds_host, B, C h w, 0, 4, ..) would have
 *            written as fp32, generated in registers
 * a == 0: src is not read and may be NULL.  s == 0: no noise is read or drawn; noise and seeds_host may both be NULL.
 * Size rules: C h w % 4 == 0 (a thread owns one Philox group of 4 consecutive elements of a chain's row; for w % 4 != 0 a group
 * straddles image rows and planes, so every element is indexed on its own); 1 <= h0 <= h <= 2048, 1 <= w0 <= w <= 2048 (the
 * coordinate integers stay exact); 1 <= B, 1 <= C.  More chains than one launch carries keys for (32) take further launches keyed by
 * their own seeds.  16-byte stores (8-byte for fp16), no atomics.
 * Errors by name: a null pointer that is needed, a misaligned x or noise, B, C, a size that is no upscaling ("downscaling is not
 * built"), mode outside 0 .. 3, mode 0 with another source size, src_rows other than 1 or B, C h w no multiple of 4, a or s not
 * finite or both 0, s != 0 with neither noise nor seeds_host. */
int cfgpp_img2img_start(void* x, const void* src, const void* noise, const unsigned long long* seeds_host, float a, float s, int B,
                        int src_rows, int C, int h0, int w0, int h, int w, int mode, int x_half, int src_half, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFGPP_IMG2IMG_H */
