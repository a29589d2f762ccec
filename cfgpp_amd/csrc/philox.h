// The counter-based normal generator of include/cfgpp_lcm.h, shared by the kernels that draw noise in registers (lcm_kernels.hip,
// sde_kernels.hip, dpmpp_sde_kernels.hip, img2img_kernels.hip): ONE definition, so that a draw inside a step kernel is the instruction sequence of cfgpp_philox_normal's fill and
// gives the same bits.  Every file that includes this is built with -ffp-contract=off and without fast-math (cfgpp_amd/build.py).
//
// Philox4x32-10 keyed by the chain's 64-bit seed, counter (q, 0, draw, stream_id) with q the 4-element group inside the chain's row;
// the four outputs are two Box-Muller pairs.  stream_id 0: LCM renoise, 1: ancestral noise, 2: the 2M / 3M SDE solvers' step noise,
// 3: the path increments of the two-stage DPM++ SDE solver (two draws per step, both read by both stages), 4: the forward noise of an
// img2img / hires-fix start (include/cfgpp_img2img.h; draw 0).
#pragma once
#include "common.h"

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// Philox4x32-10: c <- ten rounds of {hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)}, the key bumped between rounds
static __device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c[0]), lo0 = PHILOX_M0 * c[0];
        const uint32_t hi1 = __umulhi(PHILOX_M1, c[2]), lo1 = PHILOX_M1 * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
}

// one Box-Muller pair from two words: (rho cos(2 pi u2), rho sin(2 pi u2))
static __device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& x, float& y) {
    const float u1 = __fmul_rn((float)((ra >> 8) + 1u), 0x1p-24f);      // (0, 1], exact
    const float t2 = __fmul_rn((float)(rb >> 8), 0x1p-23f);              // 2 u2 in [0, 2), exact
    const float rho = __fsqrt_rn(__fmul_rn(-2.0f, logf(u1)));
    float s, c;
    sincospif(t2, &s, &c);
    x = __fmul_rn(rho, c);
    y = __fmul_rn(rho, s);
}

// the four normals of group q of a chain's row
static __device__ __forceinline__ void philox_normal4(uint32_t q, uint32_t draw, uint32_t stream_id, uint32_t k0, uint32_t k1, float (&n)[4]) {
    uint32_t c[4] = {q, 0u, draw, stream_id};
    philox4x32_10(c, k0, k1);
    box_muller(c[0], c[1], n[0], n[1]);
    box_muller(c[2], c[3], n[2], n[3]);
}

// The launch shape of the kernels that draw per chain: grid (blocks over a row's 4-element groups, chain), the chains' keys as kernel
// arguments (seeds_host is consumed before the launcher returns, nothing is uploaded).  Larger batches take more launches.
constexpr int PHILOX_ROWS = 32;       // chains per launch
struct PhiloxKeys {
    uint32_t k[PHILOX_ROWS][2];
};

static inline void philox_fill_keys(PhiloxKeys& keys, const unsigned long long* seeds, int rows) {
    for (int r = 0; r < PHILOX_ROWS; ++r) {
        const unsigned long long s = (seeds && r < rows) ? seeds[r] : 0ull;
        keys.k[r][0] = (uint32_t)(s & 0xffffffffull);
        keys.k[r][1] = (uint32_t)(s >> 32);
    }
}

static inline int philox_row_grid(long row4) {
    long g = (row4 + 255) / 256;
    if (g > 1024) g = 1024;
    return (int)g;
}
