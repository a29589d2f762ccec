// DPM-Solver++ SDE sampling (include/cfgpp_dpmpp_sde.h): one stage of the two-stage stochastic step, a sibling of sde_step_kernel.
//
// One launch per UNet call: guidance mix, den / uden from the stage's base latent, the linear combination with host-made
// coefficients, up to two noise terms drawn in registers from the generator of csrc/philox.h (stream id 3) and the next UNet call's
// fp16 input.  Both stages of a step pass the same two draw indices, so stage B draws stage A's normals again instead of reading
// them back: the two noise terms of a step are increments of ONE Brownian path without a stored tensor.
//
// Rounding contract: as in sde_kernels.hip every rounding is explicit and this file is built with -ffp-contract=off and without
// fast-math; the in-register draw is philox_normal4, the instruction sequence of cfgpp_philox_normal's fill, hence the same bits.
//
// The grid is sde_kernels.hip's: (blocks over a row's 4-element groups, chain), the chain's key read from the kernel arguments.
// out may alias x (and base where base is x): no __restrict__ on them; each thread loads everything it needs of a group before it
// stores anything of that group.
//
// HBM-bound and, at the product's sizes, launch-bound: per element stage A (base is x) moves 4 B x + 2+2 B model out in, 4 B out +
// 4 B den + 2 B UNet input out = 18 B, stage B 4 B more for its base = 22 B (measured: profiles/dpmpp_sde/README.md).
#include "common.h"
#include "step_math.h"
#include "philox.h"
#include "../../include/cfgpp_dpmpp_sde.h"

namespace {

constexpr uint32_t STAGE_STREAM = 3u;      // csrc/philox.h: the stream id of this solver's path increments

struct StageCoef {
    float sigma, a_x, a_d, a_u, c_1, c_2, s_in;
};

// n1 / n2: 0 no such term, 1 a caller-supplied fp32 tensor, 2 drawn in registers
struct StageFlags {
    int d, u, n1, n2, last, single, base_is_x;      // single: m_uc == m_c, m_hat is that tensor
};

__global__ void __launch_bounds__(256)
sde_stage_kernel(const float* x, const float* base, float* out, float* den_out, half_t* xc_out, const half_t* m_uc, const half_t* m_c,
                 float lam, StageCoef k, StageFlags f, const float* noise1, const float* noise2, PhiloxKeys keys, uint32_t draw1,
                 uint32_t draw2, long row4) {
    const int b = blockIdx.y;
    const uint32_t k0 = keys.k[b][0], k1 = keys.k[b][1];
    const long stride = (long)gridDim.x * blockDim.x;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < row4; q += stride) {
        const long i = (long)b * row4 + q;
        const float4 bv = reinterpret_cast<const float4*>(base)[i];
        float4 xv = bv;
        if (!f.base_is_x && !f.last) xv = reinterpret_cast<const float4*>(x)[i];
        const half4_t ua = reinterpret_cast<const half4_t*>(m_uc)[i];
        half4_t ub = ua;
        if (!f.single) ub = reinterpret_cast<const half4_t*>(m_c)[i];
        const float bi[4] = {bv.x, bv.y, bv.z, bv.w};
        const float xi[4] = {xv.x, xv.y, xv.z, xv.w};
        float na[4] = {0.f, 0.f, 0.f, 0.f}, nb[4] = {0.f, 0.f, 0.f, 0.f};
        if (f.n1 == 1) {
            const float4 v = reinterpret_cast<const float4*>(noise1)[i];
            na[0] = v.x; na[1] = v.y; na[2] = v.z; na[3] = v.w;
        } else if (f.n1 == 2) {
            philox_normal4((uint32_t)q, draw1, STAGE_STREAM, k0, k1, na);
        }
        if (f.n2 == 1) {
            const float4 v = reinterpret_cast<const float4*>(noise2)[i];
            nb[0] = v.x; nb[1] = v.y; nb[2] = v.z; nb[3] = v.w;
        } else if (f.n2 == 2) {
            philox_normal4((uint32_t)q, draw2, STAGE_STREAM, k0, k1, nb);
        }
        float dn[4], xn[4];
        half4_t xc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float uc = (float)ua[j];
            const float hat = f.single ? uc : cfg_mix_h(uc, (float)ub[j], lam);
            dn[j] = __fsub_rn(bi[j], __fmul_rn(k.sigma, hat));
            if (f.last) {
                xn[j] = dn[j];
            } else {
                float acc = __fmul_rn(k.a_x, xi[j]);
                if (f.d) acc = __fadd_rn(acc, __fmul_rn(k.a_d, dn[j]));
                if (f.u) acc = __fadd_rn(acc, __fmul_rn(k.a_u, __fsub_rn(bi[j], __fmul_rn(k.sigma, uc))));
                if (f.n1) acc = __fadd_rn(acc, __fmul_rn(k.c_1, na[j]));
                if (f.n2) acc = __fadd_rn(acc, __fmul_rn(k.c_2, nb[j]));
                xn[j] = acc;
            }
            xc[j] = (half_t)h_round(__fmul_rn(xn[j], k.s_in));
        }
        reinterpret_cast<float4*>(den_out)[i] = make_float4(dn[0], dn[1], dn[2], dn[3]);
        reinterpret_cast<float4*>(out)[i] = make_float4(xn[0], xn[1], xn[2], xn[3]);
        if (xc_out) reinterpret_cast<half4_t*>(xc_out)[i] = xc;
    }
}

inline bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" {

int cfgpp_step_sde_stage(const void* x, const void* base, void* out, void* den_out, void* xc_out, const void* m_uc, const void* m_c,
                         float lam, const float* coef_host, int terms, int last, const void* noise1, const void* noise2,
                         const unsigned long long* seeds_host, int B, long row_elems, unsigned draw1, unsigned draw2, void* stream) {
    CFGPP_REQUIRE(x && base && out && den_out && m_uc && m_c && coef_host, "cfgpp_step_sde_stage: null pointer");
    CFGPP_REQUIRE(out != base || base == x, "cfgpp_step_sde_stage: out must not be base when base is not x");
    CFGPP_REQUIRE(den_out != x, "cfgpp_step_sde_stage: den_out must not be x");
    CFGPP_REQUIRE(den_out != out, "cfgpp_step_sde_stage: den_out must not be out");
    CFGPP_REQUIRE(B >= 1, "cfgpp_step_sde_stage: B=%d", B);
    CFGPP_REQUIRE(row_elems >= 4 && (row_elems % 4) == 0 && row_elems < (1L << 34),
                  "cfgpp_step_sde_stage: row_elems=%ld must be a multiple of 4 in 4 .. 2^34 - 4", row_elems);
    CFGPP_REQUIRE(terms >= 0 && terms <= 15, "cfgpp_step_sde_stage: terms=%d (a mask of CFGPP_STAGE_*, 0 .. 15)", terms);
    for (int j = 0; j < 7; ++j) CFGPP_REQUIRE(finite_f(coef_host[j]), "cfgpp_step_sde_stage: coef[%d] is not finite", j);
    CFGPP_REQUIRE(finite_f(lam), "cfgpp_step_sde_stage: lam is not finite");
    const StageCoef k{coef_host[0], coef_host[1], coef_host[2], coef_host[3], coef_host[4], coef_host[5], coef_host[6]};
    const int n1 = (last || !(terms & CFGPP_STAGE_N1)) ? 0 : (noise1 ? 1 : 2);
    const int n2 = (last || !(terms & CFGPP_STAGE_N2)) ? 0 : (noise2 ? 1 : 2);
    const bool draws = n1 == 2 || n2 == 2;
    CFGPP_REQUIRE(!draws || seeds_host, "cfgpp_step_sde_stage: a noise term needs its noise tensor or seeds_host");
    const StageFlags f{(terms & CFGPP_STAGE_D) != 0, (terms & CFGPP_STAGE_U) != 0, n1, n2, last != 0, m_uc == m_c, base == x};
    const long row4 = row_elems / 4;
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += PHILOX_ROWS) {
        const int rows = B - b0 < PHILOX_ROWS ? B - b0 : PHILOX_ROWS;
        PhiloxKeys keys;
        philox_fill_keys(keys, draws ? seeds_host + b0 : nullptr, rows);
        const long off = (long)b0 * row_elems;
        const float* xp = (const float*)x + off;
        const float* bp = (const float*)base + off;
        float* op = (float*)out + off;
        float* dp = (float*)den_out + off;
        half_t* cp = xc_out ? (half_t*)xc_out + off : nullptr;
        const half_t* up = (const half_t*)m_uc + off;
        const half_t* mp = (const half_t*)m_c + off;
        const float* p1 = (n1 == 1) ? (const float*)noise1 + off : nullptr;
        const float* p2 = (n2 == 1) ? (const float*)noise2 + off : nullptr;
        hipLaunchKernelGGL(sde_stage_kernel, dim3(philox_row_grid(row4), rows), dim3(256), 0, s, xp, bp, op, dp, cp, up, mp, lam, k, f, p1,
                           p2, keys, (uint32_t)draw1, (uint32_t)draw2, row4);
        CFGPP_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
