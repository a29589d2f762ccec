// Latent-consistency (LCM) sampling (include/cfgpp_lcm.h): the counter-based normal generator and the fused consistency step that
// draws its renoising noise from it in registers.
//
// Generator (csrc/philox.h, shared with sde_kernels.hip): Philox4x32-10 keyed by the chain's 64-bit seed, counter (q, 0, draw,
// stream_id) with q the 4-element group inside the chain's row; the four outputs are two Box-Muller pairs.  A chain's noise therefore depends on its seed and its position in its own
// row only: chain b of a batch reproduces chain b run alone.  The definition and the known-answer vectors are in the header.
//
// Rounding contract: as in step_kernels.hip / vpred_kernels.hip every rounding is explicit and this file is built with
// -ffp-contract=off; logf / sqrtf / sincospif are the accurate OCML functions, so the step's in-register draw and
// cfgpp_philox_normal's fill are the same instruction sequence and the same bits.
//
// The grid is (blocks over a row's 4-element groups, chain): the seed is uniform in a workgroup and is read from the kernel
// arguments (seeds_host is consumed before the launcher returns, nothing is uploaded).
//
// HBM-bound: per element 4 B z in + 2+2 B model out in + 4 B den out + 4 B z out = 16 B, cfgpp_step_ddim's traffic; the Philox
// block + two logf / sincospif pairs per 4 elements ride under it (measured: profiles/lcm/README.md).
#include "common.h"
#include "step_math.h"
#include "philox.h"
#include "../../include/cfgpp_lcm.h"
#include "cfgpp_debug.h"

namespace {

constexpr int LCM_ROWS = PHILOX_ROWS;  // chains per launch (their keys travel as kernel arguments); larger batches take more launches
using Keys = PhiloxKeys;

template <bool OUT_HALF>
__global__ void __launch_bounds__(256)
philox_normal_kernel(void* __restrict__ out_, Keys keys, uint32_t draw, uint32_t stream_id, long row4) {
    const int b = blockIdx.y;
    const uint32_t k0 = keys.k[b][0], k1 = keys.k[b][1];
    const long stride = (long)gridDim.x * blockDim.x;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < row4; q += stride) {
        float n[4];
        philox_normal4((uint32_t)q, draw, stream_id, k0, k1, n);
        const long i = (long)b * row4 + q;
        if (OUT_HALF) {
            half4_t o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (half_t)n[j];
            reinterpret_cast<half4_t*>(out_)[i] = o;
        } else {
            reinterpret_cast<float4*>(out_)[i] = make_float4(n[0], n[1], n[2], n[3]);
        }
    }
}

struct LcmCoef {
    float k0, k1, c_out, c_skip, c3, c4;      // k0 / k1: (c1, c2) of the epsilon form, (s_v, a_z) of the v form
};

// NOISE: 0 the last step (no noise), 1 a caller-supplied fp32 tensor, 2 drawn in registers.  m_uc / m_c may be the same tensor.
template <bool PRED_V, int NOISE>
__global__ void __launch_bounds__(256)
lcm_step_kernel(float* __restrict__ z, float* __restrict__ den_out, const half_t* m_uc, const half_t* m_c, float lam, LcmCoef k,
                const float* __restrict__ noise, Keys keys, uint32_t draw, long row4) {
    const int b = blockIdx.y;
    const uint32_t k0 = keys.k[b][0], k1 = keys.k[b][1];
    const long stride = (long)gridDim.x * blockDim.x;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < row4; q += stride) {
        const long i = (long)b * row4 + q;
        const float4 zv = reinterpret_cast<const float4*>(z)[i];
        const half4_t ua = reinterpret_cast<const half4_t*>(m_uc)[i];
        const half4_t ub = reinterpret_cast<const half4_t*>(m_c)[i];
        const float zi[4] = {zv.x, zv.y, zv.z, zv.w};
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (NOISE == 1) {
            const float4 nv = reinterpret_cast<const float4*>(noise)[i];
            nz[0] = nv.x; nz[1] = nv.y; nz[2] = nv.z; nz[3] = nv.w;
        } else if (NOISE == 2) {
            philox_normal4((uint32_t)q, draw, 0u, k0, k1, nz);
        }
        float dn[4], zn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float hat = cfg_mix_h((float)ua[j], (float)ub[j], lam);
            float x0;
            if (PRED_V) x0 = __fsub_rn(__fmul_rn(k.k1, zi[j]), h_round(__fmul_rn(k.k0, hat)));
            else        x0 = div_as_ref(__fsub_rn(zi[j], h_round(__fmul_rn(hat, k.k0))), k.k1);
            dn[j] = __fadd_rn(__fmul_rn(k.c_out, x0), __fmul_rn(k.c_skip, zi[j]));
            zn[j] = NOISE == 0 ? dn[j] : __fadd_rn(__fmul_rn(k.c3, dn[j]), __fmul_rn(k.c4, nz[j]));
        }
        reinterpret_cast<float4*>(den_out)[i] = make_float4(dn[0], dn[1], dn[2], dn[3]);
        reinterpret_cast<float4*>(z)[i] = make_float4(zn[0], zn[1], zn[2], zn[3]);
    }
}

// out[4 i ..] = Philox4x32-10 of counter (c0 + i, c1, c2, c3) under key (k0, k1): the raw words, for the known-answer test
__global__ void __launch_bounds__(256)
philox_raw_kernel(uint32_t* __restrict__ out, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t c[4] = {c0 + (uint32_t)i, c1, c2, c3};
    philox4x32_10(c, k0, k1);
    reinterpret_cast<uint4*>(out)[i] = make_uint4(c[0], c[1], c[2], c[3]);
}

inline int row_grid(long row4) { return philox_row_grid(row4); }
inline void fill_keys(Keys& keys, const unsigned long long* seeds, int rows) { philox_fill_keys(keys, seeds, rows); }

}  // namespace

extern "C" {

int cfgpp_philox_normal(void* out, int out_is_half, const unsigned long long* seeds_host, int B, long row_elems, unsigned draw,
                        unsigned stream_id, void* stream) {
    CFGPP_REQUIRE(out && seeds_host, "cfgpp_philox_normal: null pointer");
    CFGPP_REQUIRE(B >= 1, "cfgpp_philox_normal: B=%d", B);
    CFGPP_REQUIRE(row_elems >= 4 && (row_elems % 4) == 0 && row_elems < (1L << 34),
                  "cfgpp_philox_normal: row_elems=%ld must be a multiple of 4 in 4 .. 2^34 - 4", row_elems);
    const long row4 = row_elems / 4;
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += LCM_ROWS) {
        const int rows = B - b0 < LCM_ROWS ? B - b0 : LCM_ROWS;
        Keys keys;
        fill_keys(keys, seeds_host + b0, rows);
        const dim3 grid(row_grid(row4), rows);
        if (out_is_half)
            hipLaunchKernelGGL(philox_normal_kernel<true>, grid, dim3(256), 0, s, (void*)((half_t*)out + (long)b0 * row_elems), keys,
                               (uint32_t)draw, (uint32_t)stream_id, row4);
        else
            hipLaunchKernelGGL(philox_normal_kernel<false>, grid, dim3(256), 0, s, (void*)((float*)out + (long)b0 * row_elems), keys,
                               (uint32_t)draw, (uint32_t)stream_id, row4);
        CFGPP_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

int cfgpp_step_lcm(void* z, void* den_out, const void* m_uc, const void* m_c, float lam, const float* coef_host, int pred_v, int last,
                   const void* noise, const unsigned long long* seeds_host, int B, long row_elems, unsigned draw, void* stream) {
    CFGPP_REQUIRE(z && den_out && m_uc && m_c && coef_host, "cfgpp_step_lcm: null pointer");
    CFGPP_REQUIRE(B >= 1, "cfgpp_step_lcm: B=%d", B);
    CFGPP_REQUIRE(row_elems >= 4 && (row_elems % 4) == 0 && row_elems < (1L << 34),
                  "cfgpp_step_lcm: row_elems=%ld must be a multiple of 4 in 4 .. 2^34 - 4", row_elems);
    CFGPP_REQUIRE(last || noise || seeds_host, "cfgpp_step_lcm: a step that is not the last needs noise or seeds_host");
    const LcmCoef k{coef_host[0], coef_host[1], coef_host[2], coef_host[3], coef_host[4], coef_host[5]};
    const long row4 = row_elems / 4;
    const int mode = last ? 0 : (noise ? 1 : 2);
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += LCM_ROWS) {
        const int rows = B - b0 < LCM_ROWS ? B - b0 : LCM_ROWS;
        Keys keys;
        fill_keys(keys, mode == 2 ? seeds_host + b0 : nullptr, rows);
        const long off = (long)b0 * row_elems;
        float* zp = (float*)z + off;
        float* dp = (float*)den_out + off;
        const half_t* up = (const half_t*)m_uc + off;
        const half_t* cp = (const half_t*)m_c + off;
        const float* np = noise ? (const float*)noise + off : nullptr;
        const dim3 grid(row_grid(row4), rows);
#define CFGPP_LCM_LAUNCH(V, N) \
        hipLaunchKernelGGL((lcm_step_kernel<V, N>), grid, dim3(256), 0, s, zp, dp, up, cp, lam, k, np, keys, (uint32_t)draw, row4)
        if (pred_v) {
            if (mode == 0) CFGPP_LCM_LAUNCH(true, 0); else if (mode == 1) CFGPP_LCM_LAUNCH(true, 1); else CFGPP_LCM_LAUNCH(true, 2);
        } else {
            if (mode == 0) CFGPP_LCM_LAUNCH(false, 0); else if (mode == 1) CFGPP_LCM_LAUNCH(false, 1); else CFGPP_LCM_LAUNCH(false, 2);
        }
#undef CFGPP_LCM_LAUNCH
        CFGPP_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

int cfgpp_op_philox_raw(void* out, const unsigned* ctr_host4, const unsigned* key_host2, long n, void* stream) {
    CFGPP_REQUIRE(out && ctr_host4 && key_host2, "cfgpp_op_philox_raw: null pointer");
    CFGPP_REQUIRE(n >= 1 && n <= (1L << 24), "cfgpp_op_philox_raw: n=%ld", n);
    hipLaunchKernelGGL(philox_raw_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t*)out, ctr_host4[0],
                       ctr_host4[1], ctr_host4[2], ctr_host4[3], key_host2[0], key_host2[1], n);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
