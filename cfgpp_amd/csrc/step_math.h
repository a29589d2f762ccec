// The rounding primitives of the fused sampler steps (step_kernels.hip, vpred_kernels.hip, lcm_kernels.hip, sde_kernels.hip, pano_kernels.hip): ONE
// definition, so that a step kernel in another file evaluates the same instruction sequence and gives the same bits.  Every file
// that includes this is built with -ffp-contract=off (cfgpp_amd/build.py).
#pragma once
#include "common.h"

// RNE to fp16 of a value that has ALREADY been rounded to fp32 (torch computes the fp16 result of an
// op in fp32 and then rounds: two roundings).  The empty asm makes the fp32 value opaque so the compiler
// cannot fuse mul+convert into v_fma_mixlo_f16, which rounds the exact product ONCE and differs on ties.
static __device__ __forceinline__ float h_round(float x) {
    asm volatile("" : "+v"(x));
    return (float)(half_t)x;
}

// eps_hat = eps_uc + lam*(eps_c - eps_uc) with fp16 rounding after each op
static __device__ __forceinline__ float cfg_mix_h(float uc, float c, float lam) {
    float d = h_round(__fsub_rn(c, uc));
    float e = h_round(__fmul_rn(d, lam));
    return h_round(__fadd_rn(uc, e));
}
static __device__ __forceinline__ float cfg_mix_f(float uc, float c, float lam) {
    return __fadd_rn(uc, __fmul_rn(__fsub_rn(c, uc), lam));
}

// `x / c` as the reference's backend evaluates it.  c > 0: IEEE division (torch-CPU, and every tensor / tensor division).
// c < 0: the host passes c = -fl32(1 / divisor) and the kernel MULTIPLIES by -c: torch's GPU `div` with a CPU 0-dim
// scalar (or python number) divisor - which is what `/ at.sqrt()`, `/ sigma.item()`, `/ (2*r)` and `/ (sigma**2+1)**0.5`
// are in the reference - computes `a * (1/b)` with the reciprocal taken once on the host in fp32
// (ATen BinaryDivTrueKernel.cu, `iter.is_cpu_scalar(2)`): up to 1 ulp away from the true quotient.  Every divisor on
// this path is positive, so the sign is free to carry the choice (cfgpp_amd/coeffs.py: `divisor()`).
static __device__ __forceinline__ float div_as_ref(float x, float c) {
    return c < 0.f ? __fmul_rn(x, -c) : __fdiv_rn(x, c);
}

// One element of the generalised DDIM update on an fp32 latent with fp16 eps (ddim_step_kernel<EPS_HALF = true>):
//     hat = cfg_mix_h(uc, cc);  A = tweedie_uc ? uc : hat;  B = renoise_uc ? uc : hat
//     z0  = div_as_ref(z - h(A * c1), c2);   zn = c3 * z0 + h(B * c4)
static __device__ __forceinline__ void ddim_update_h(float z, float uc, float cc, float lam, float c1, float c2, float c3, float c4,
                                                     int tweedie_uc, int renoise_uc, float& z0, float& zn) {
    const float hat = cfg_mix_h(uc, cc, lam);
    const float A = tweedie_uc ? uc : hat;
    const float B = renoise_uc ? uc : hat;
    const float pa = h_round(__fmul_rn(A, c1));
    const float pb = h_round(__fmul_rn(B, c4));
    z0 = div_as_ref(__fsub_rn(z, pa), c2);
    zn = __fadd_rn(__fmul_rn(c3, z0), pb);
}
