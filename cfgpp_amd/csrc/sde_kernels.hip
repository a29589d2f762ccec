// DPM-Solver++ 2M / 3M SDE sampling (include/cfgpp_sde.h): the fused stochastic multistep step and the job's first UNet input.
//
// One launch per sampling step: guidance mix, den / uden, the linear multistep combination with host-made coefficients, the noise
// drawn in registers from the generator of csrc/philox.h (stream id 2), the history write and the next step's fp16 UNet input.
//
// Rounding contract: as in lcm_kernels.hip every rounding is explicit and this file is built with -ffp-contract=off and without
// fast-math; the in-register draw is philox_normal4, the instruction sequence of cfgpp_philox_normal's fill, hence the same bits.
//
// The grid is lcm_kernels.hip's: (blocks over a row's 4-element groups, chain), the chain's key read from the kernel arguments.
// x, hist1, hist2 and hist_out may alias (x is updated in place, hist_out may be hist2): no __restrict__ on them; each thread loads
// everything it needs of a group before it stores anything of that group.
//
// HBM-bound and, at the product's sizes, launch-bound: per element at most 4 B x + 2+2 B model out + 4+4 B history in, 4 B x +
// 4 B den + 4 B history + 2 B UNet input out = 30 B (measured: profiles/sde/README.md).
#include "common.h"
#include "step_math.h"
#include "philox.h"
#include "../../include/cfgpp_sde.h"

namespace {

struct SdeCoef {
    float sigma, a_x, a_d, a_u, a_1, a_2, a_n, s_in;
};

struct SdeFlags {
    int cfgpp, n_hist, last, single;      // single: m_uc == m_c, m_hat is that tensor
};

// NOISE: 0 no noise term (the last step, a_n == 0), 1 a caller-supplied fp32 tensor, 2 drawn in registers
template <int NOISE>
__global__ void __launch_bounds__(256)
sde_step_kernel(float* x, float* den_out, half_t* xc_out, const float* hist1, const float* hist2, float* hist_out, const half_t* m_uc,
                const half_t* m_c, float lam, SdeCoef k, SdeFlags f, const float* noise, PhiloxKeys keys, uint32_t draw, long row4) {
    const int b = blockIdx.y;
    const uint32_t k0 = keys.k[b][0], k1 = keys.k[b][1];
    const long stride = (long)gridDim.x * blockDim.x;
    const bool need_u = f.cfgpp != 0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < row4; q += stride) {
        const long i = (long)b * row4 + q;
        const float4 xv = reinterpret_cast<const float4*>(x)[i];
        const half4_t ua = reinterpret_cast<const half4_t*>(m_uc)[i];
        half4_t ub = ua;
        if (!f.single) ub = reinterpret_cast<const half4_t*>(m_c)[i];
        const float xi[4] = {xv.x, xv.y, xv.z, xv.w};
        float h1[4] = {0.f, 0.f, 0.f, 0.f}, h2[4] = {0.f, 0.f, 0.f, 0.f}, nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (!f.last && f.n_hist >= 1) {
            const float4 v = reinterpret_cast<const float4*>(hist1)[i];
            h1[0] = v.x; h1[1] = v.y; h1[2] = v.z; h1[3] = v.w;
        }
        if (!f.last && f.n_hist == 2) {
            const float4 v = reinterpret_cast<const float4*>(hist2)[i];
            h2[0] = v.x; h2[1] = v.y; h2[2] = v.z; h2[3] = v.w;
        }
        if (NOISE == 1) {
            const float4 v = reinterpret_cast<const float4*>(noise)[i];
            nz[0] = v.x; nz[1] = v.y; nz[2] = v.z; nz[3] = v.w;
        } else if (NOISE == 2) {
            philox_normal4((uint32_t)q, draw, 2u, k0, k1, nz);
        }
        float dn[4], un[4], xn[4];
        half4_t xc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float uc = (float)ua[j];
            const float hat = f.single ? uc : cfg_mix_h(uc, (float)ub[j], lam);
            dn[j] = __fsub_rn(xi[j], __fmul_rn(k.sigma, hat));
            un[j] = need_u ? __fsub_rn(xi[j], __fmul_rn(k.sigma, uc)) : dn[j];
            if (f.last) {
                xn[j] = dn[j];
            } else {
                float acc = __fmul_rn(k.a_x, xi[j]);
                acc = __fadd_rn(acc, __fmul_rn(k.a_d, dn[j]));
                if (f.cfgpp) acc = __fadd_rn(acc, __fmul_rn(k.a_u, un[j]));
                if (f.n_hist >= 1) acc = __fadd_rn(acc, __fmul_rn(k.a_1, h1[j]));
                if (f.n_hist == 2) acc = __fadd_rn(acc, __fmul_rn(k.a_2, h2[j]));
                if (NOISE != 0) acc = __fadd_rn(acc, __fmul_rn(k.a_n, nz[j]));
                xn[j] = acc;
            }
            xc[j] = (half_t)h_round(__fmul_rn(xn[j], k.s_in));
        }
        reinterpret_cast<float4*>(den_out)[i] = make_float4(dn[0], dn[1], dn[2], dn[3]);
        reinterpret_cast<float4*>(x)[i] = make_float4(xn[0], xn[1], xn[2], xn[3]);
        if (hist_out) reinterpret_cast<float4*>(hist_out)[i] = make_float4(un[0], un[1], un[2], un[3]);      // un == dn without cfgpp
        if (xc_out) reinterpret_cast<half4_t*>(xc_out)[i] = xc;
    }
}

// xc = h(fl(x * s)): whole 4-element groups by 16-byte loads / 8-byte stores, the up-to-3 trailing elements one by one
__global__ void __launch_bounds__(256)
sde_input_kernel(const float* __restrict__ x, half_t* __restrict__ xc, float s, long n) {
    const long n4 = n / 4;
    const long stride = (long)gridDim.x * blockDim.x;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long q = t; q < n4; q += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[q];
        half4_t o;
        o[0] = (half_t)h_round(__fmul_rn(v.x, s));
        o[1] = (half_t)h_round(__fmul_rn(v.y, s));
        o[2] = (half_t)h_round(__fmul_rn(v.z, s));
        o[3] = (half_t)h_round(__fmul_rn(v.w, s));
        reinterpret_cast<half4_t*>(xc)[q] = o;
    }
    const long e = 4 * n4 + t;
    if (e < n) xc[e] = (half_t)h_round(__fmul_rn(x[e], s));
}

inline bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" {

int cfgpp_sde_input(const void* x, void* xc, float s_in, long n, void* stream) {
    CFGPP_REQUIRE(x && xc, "cfgpp_sde_input: null pointer");
    CFGPP_REQUIRE(n >= 1 && n < (1L << 40), "cfgpp_sde_input: n=%ld", n);
    CFGPP_REQUIRE(finite_f(s_in), "cfgpp_sde_input: s_in is not finite");
    const long groups = n / 4 > 0 ? n / 4 : 1;
    hipLaunchKernelGGL(sde_input_kernel, dim3(philox_row_grid(groups)), dim3(256), 0, (hipStream_t)stream, (const float*)x, (half_t*)xc,
                       s_in, n);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

int cfgpp_step_sde(void* x, void* den_out, void* xc_out, const void* hist1, const void* hist2, void* hist_out, const void* m_uc,
                   const void* m_c, float lam, const float* coef_host, int cfgpp, int n_hist, int last, const void* noise,
                   const unsigned long long* seeds_host, int B, long row_elems, unsigned draw, void* stream) {
    CFGPP_REQUIRE(x && den_out && m_uc && m_c && coef_host, "cfgpp_step_sde: null pointer");
    CFGPP_REQUIRE(den_out != x, "cfgpp_step_sde: den_out must not be x");
    CFGPP_REQUIRE(B >= 1, "cfgpp_step_sde: B=%d", B);
    CFGPP_REQUIRE(row_elems >= 4 && (row_elems % 4) == 0 && row_elems < (1L << 34),
                  "cfgpp_step_sde: row_elems=%ld must be a multiple of 4 in 4 .. 2^34 - 4", row_elems);
    CFGPP_REQUIRE(n_hist >= 0 && n_hist <= 2, "cfgpp_step_sde: n_hist=%d (0 .. 2)", n_hist);
    CFGPP_REQUIRE(n_hist < 1 || hist1, "cfgpp_step_sde: n_hist=%d needs hist1", n_hist);
    CFGPP_REQUIRE(n_hist < 2 || hist2, "cfgpp_step_sde: n_hist=%d needs hist2", n_hist);
    for (int j = 0; j < 8; ++j) CFGPP_REQUIRE(finite_f(coef_host[j]), "cfgpp_step_sde: coef[%d] is not finite", j);
    CFGPP_REQUIRE(finite_f(lam), "cfgpp_step_sde: lam is not finite");
    const SdeCoef k{coef_host[0], coef_host[1], coef_host[2], coef_host[3], coef_host[4], coef_host[5], coef_host[6], coef_host[7]};
    const int mode = (last || k.a_n == 0.f) ? 0 : (noise ? 1 : 2);
    CFGPP_REQUIRE(mode != 2 || seeds_host, "cfgpp_step_sde: a step with a noise term needs noise or seeds_host");
    const SdeFlags f{cfgpp != 0, n_hist, last != 0, m_uc == m_c};
    const long row4 = row_elems / 4;
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += PHILOX_ROWS) {
        const int rows = B - b0 < PHILOX_ROWS ? B - b0 : PHILOX_ROWS;
        PhiloxKeys keys;
        philox_fill_keys(keys, mode == 2 ? seeds_host + b0 : nullptr, rows);
        const long off = (long)b0 * row_elems;
        float* xp = (float*)x + off;
        float* dp = (float*)den_out + off;
        half_t* cp = xc_out ? (half_t*)xc_out + off : nullptr;
        const float* h1 = hist1 ? (const float*)hist1 + off : nullptr;
        const float* h2 = hist2 ? (const float*)hist2 + off : nullptr;
        float* ho = hist_out ? (float*)hist_out + off : nullptr;
        const half_t* up = (const half_t*)m_uc + off;
        const half_t* mp = (const half_t*)m_c + off;
        const float* np = (mode == 1) ? (const float*)noise + off : nullptr;
        const dim3 grid(philox_row_grid(row4), rows);
#define CFGPP_SDE_LAUNCH(N) \
        hipLaunchKernelGGL((sde_step_kernel<N>), grid, dim3(256), 0, s, xp, dp, cp, h1, h2, ho, up, mp, lam, k, f, np, keys, (uint32_t)draw, row4)
        if (mode == 0) CFGPP_SDE_LAUNCH(0); else if (mode == 1) CFGPP_SDE_LAUNCH(1); else CFGPP_SDE_LAUNCH(2);
#undef CFGPP_SDE_LAUNCH
        CFGPP_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
