// The fused sampler arithmetic of v-prediction models (include/cfgpp_vpred.h): the v-form twin of step_kernels.hip's generalised
// DDIM update, the v -> eps conversion in front of the k-diffusion step kernels, and the per-sample factor of diffusers'
// rescale_noise_cfg.
//
// With a = sqrt(alpha), s = sqrt(1-alpha) a v-prediction UNet returns v = a*eps - s*x0, so
//     x0 = a*z - s*v          eps = a*v + s*z
// and the DDIM update needs no division: alpha_t = 0 (zero terminal SNR) is an ordinary input.
//
// Rounding contract: as in step_kernels.hip every rounding is explicit (fp16 roundings of the products with v, fp32 latent, NO fma
// contraction: this file is built with -ffp-contract=off); the coefficients arrive as fp32 and the host (cfgpp_amd/coeffs.py)
// pre-rounds to fp16 the ones torch-CPU would round.
//
// HBM-bound: per element 4 B z in + 2+2 B v in + 4 B z0t out + 4 B z out = 16 B, the eps kernel's traffic.
#include "common.h"
#include "step_math.h"
#include "../../include/cfgpp_vpred.h"

namespace {

struct VCoef {
    float a_z, s_v, a_v, s_z, c3, c4;
};

// Z_HALF = false: fp32 latent; true: fp16 latent, every operation rounded to fp16.  row4 = row_elems / 4 (only read with row_scale).
template <bool Z_HALF>
__global__ void __launch_bounds__(256)
ddim_v_step_kernel(void* __restrict__ z_, void* __restrict__ z0t_, const half_t* __restrict__ v_uc, const half_t* __restrict__ v_c,
                   float lam, VCoef k, int tweedie_uc, int renoise_uc, const float* __restrict__ row_scale, long row4, long n4) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n4; i += stride) {
        const half4_t ua = reinterpret_cast<const half4_t*>(v_uc)[i];
        const half4_t ub = reinterpret_cast<const half4_t*>(v_c)[i];
        const float f = row_scale ? row_scale[i / row4] : 1.f;      // row_elems % 4 == 0: the four elements share a sample
        float zi[4];
        if (Z_HALF) {
            const half4_t zv = reinterpret_cast<const half4_t*>(z_)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) zi[j] = (float)zv[j];
        } else {
            const float4 zv = reinterpret_cast<const float4*>(z_)[i];
            zi[0] = zv.x; zi[1] = zv.y; zi[2] = zv.z; zi[3] = zv.w;
        }
        float z0[4], zn[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float uc = (float)ua[j], cc = (float)ub[j];
            float hat = cfg_mix_h(uc, cc, lam);
            if (row_scale) hat = h_round(__fmul_rn(f, hat));
            const float A = tweedie_uc ? uc : hat;
            const float B = renoise_uc ? uc : hat;
            const float sA = h_round(__fmul_rn(k.s_v, A));
            const float aB = h_round(__fmul_rn(k.a_v, B));
            float az = __fmul_rn(k.a_z, zi[j]);
            float sz = __fmul_rn(k.s_z, zi[j]);
            if (Z_HALF) {
                az = h_round(az); sz = h_round(sz);
                const float x0 = h_round(__fsub_rn(az, sA));
                const float eb = h_round(__fadd_rn(aB, sz));
                z0[j] = x0;
                zn[j] = h_round(__fadd_rn(h_round(__fmul_rn(k.c3, x0)), h_round(__fmul_rn(k.c4, eb))));
            } else {
                const float x0 = __fsub_rn(az, sA);
                const float eb = __fadd_rn(aB, sz);
                z0[j] = x0;
                zn[j] = __fadd_rn(__fmul_rn(k.c3, x0), __fmul_rn(k.c4, eb));
            }
        }
        if (Z_HALF) {
            half4_t o0, o1;
#pragma unroll
            for (int j = 0; j < 4; ++j) { o0[j] = (half_t)z0[j]; o1[j] = (half_t)zn[j]; }
            reinterpret_cast<half4_t*>(z0t_)[i] = o0;
            reinterpret_cast<half4_t*>(z_)[i] = o1;
        } else {
            reinterpret_cast<float4*>(z0t_)[i] = make_float4(z0[0], z0[1], z0[2], z0[3]);
            reinterpret_cast<float4*>(z_)[i] = make_float4(zn[0], zn[1], zn[2], zn[3]);
        }
    }
}

// eps = h(h(a*v) + h(s*x)) for both halves; outputs may be the inputs (each thread reads its four elements before it writes them)
__global__ void __launch_bounds__(256)
v_to_eps_kernel(half_t* eps_uc, half_t* eps_c, const half_t* v_uc, const half_t* v_c, const half_t* __restrict__ x, float a, float s,
                long n4) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n4; i += stride) {
        const half4_t ua = reinterpret_cast<const half4_t*>(v_uc)[i];
        const half4_t ub = reinterpret_cast<const half4_t*>(v_c)[i];
        const half4_t xv = reinterpret_cast<const half4_t*>(x)[i];
        half4_t o0, o1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float sx = h_round(__fmul_rn(s, (float)xv[j]));
            o0[j] = (half_t)h_round(__fadd_rn(h_round(__fmul_rn(a, (float)ua[j])), sx));
            o1[j] = (half_t)h_round(__fadd_rn(h_round(__fmul_rn(a, (float)ub[j])), sx));
        }
        reinterpret_cast<half4_t*>(eps_uc)[i] = o0;
        reinterpret_cast<half4_t*>(eps_c)[i] = o1;
    }
}

// ---- rescale_noise_cfg: one factor per sample ---------------------------------------------------------------------------------
constexpr int RS_THREADS = 1024;                    // one workgroup per sample: 16 waves
constexpr int RS_WAVES = RS_THREADS / CFGPP_WAVE;

// sum of (p, q) over the workgroup, the same value in every thread: xor-shuffle tree inside a wave, then the 16 wave sums in index
// order.  A fixed tree: the result does not depend on timing.
__device__ __forceinline__ void block_sum2(float& p, float& q, float (*sm)[RS_WAVES]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        p = __fadd_rn(p, __shfl_xor(p, o));
        q = __fadd_rn(q, __shfl_xor(q, o));
    }
    const int w = threadIdx.x / CFGPP_WAVE;
    __syncthreads();                                // the previous round's readers are done with sm
    if ((threadIdx.x & (CFGPP_WAVE - 1)) == 0) { sm[0][w] = p; sm[1][w] = q; }
    __syncthreads();
    p = 0.f; q = 0.f;
#pragma unroll
    for (int k = 0; k < RS_WAVES; ++k) { p = __fadd_rn(p, sm[0][k]); q = __fadd_rn(q, sm[1][k]); }
}

// Two passes over the row (it stays in L2: at most 2 x 128 KiB per sample): means of v_c and v_hat, then M2 = sum (x - mean)^2 -
// no E[x^2] - E[x]^2 cancellation.  A thread keeps four independent partial sums (one per element of its half4), combined pairwise.
__global__ void __launch_bounds__(RS_THREADS)
cfg_rescale_kernel(const half_t* __restrict__ v_uc, const half_t* __restrict__ v_c, float lam, float phi, float* __restrict__ out,
                   long row4) {
    __shared__ float sm[2][RS_WAVES];
    const half4_t* pu = reinterpret_cast<const half4_t*>(v_uc) + (long)blockIdx.x * row4;
    const half4_t* pc = reinterpret_cast<const half4_t*>(v_c) + (long)blockIdx.x * row4;
    float sc[4] = {0.f, 0.f, 0.f, 0.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
    for (long i = threadIdx.x; i < row4; i += RS_THREADS) {
        const half4_t a = pu[i], b = pc[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            sc[j] = __fadd_rn(sc[j], (float)b[j]);
            sh[j] = __fadd_rn(sh[j], cfg_mix_h((float)a[j], (float)b[j], lam));
        }
    }
    float tc = __fadd_rn(__fadd_rn(sc[0], sc[1]), __fadd_rn(sc[2], sc[3]));
    float th = __fadd_rn(__fadd_rn(sh[0], sh[1]), __fadd_rn(sh[2], sh[3]));
    block_sum2(tc, th, sm);
    const float cnt = (float)(4 * row4);            // exact: row_elems <= 2^24 is checked by the launcher
    const float mc = __fdiv_rn(tc, cnt), mh = __fdiv_rn(th, cnt);
#pragma unroll
    for (int j = 0; j < 4; ++j) { sc[j] = 0.f; sh[j] = 0.f; }
    for (long i = threadIdx.x; i < row4; i += RS_THREADS) {
        const half4_t a = pu[i], b = pc[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dc = __fsub_rn((float)b[j], mc);
            const float dh = __fsub_rn(cfg_mix_h((float)a[j], (float)b[j], lam), mh);
            sc[j] = __fadd_rn(sc[j], __fmul_rn(dc, dc));
            sh[j] = __fadd_rn(sh[j], __fmul_rn(dh, dh));
        }
    }
    tc = __fadd_rn(__fadd_rn(sc[0], sc[1]), __fadd_rn(sc[2], sc[3]));
    th = __fadd_rn(__fadd_rn(sh[0], sh[1]), __fadd_rn(sh[2], sh[3]));
    block_sum2(tc, th, sm);
    if (threadIdx.x == 0) {
        // std_c / std_hat = sqrt(M2_c / M2_hat): the 1 / (n - 1) of the unbiased estimate cancels
        float f = 1.f;
        if (th > 0.f) f = __fadd_rn(1.f, __fmul_rn(phi, __fsub_rn(__fsqrt_rn(__fdiv_rn(tc, th)), 1.f)));
        out[blockIdx.x] = f;
    }
}

inline int grid_for(long items) {
    long g = (items + 255) / 256;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

extern "C" {

int cfgpp_step_ddim_v(void* z, void* z0t_out, const void* v_uc, const void* v_c, int z_is_half, float lam, const float* coef_host,
                      int tweedie_uc, int renoise_uc, const float* row_scale, long row_elems, long n, void* stream) {
    CFGPP_REQUIRE(n > 0 && (n % 4) == 0, "cfgpp_step_ddim_v: n=%ld must be a positive multiple of 4", n);
    CFGPP_REQUIRE(z && z0t_out && v_uc && v_c && coef_host, "cfgpp_step_ddim_v: null pointer");
    CFGPP_REQUIRE(row_elems >= 0 && (row_elems % 4) == 0, "cfgpp_step_ddim_v: row_elems=%ld must be a multiple of 4", row_elems);
    CFGPP_REQUIRE(!row_scale || (row_elems > 0 && (n % row_elems) == 0),
                  "cfgpp_step_ddim_v: row_scale needs row_elems > 0 dividing n (row_elems=%ld, n=%ld)", row_elems, n);
    const VCoef k{coef_host[0], coef_host[1], coef_host[2], coef_host[3], coef_host[4], coef_host[5]};
    const long n4 = n / 4, row4 = row_scale ? row_elems / 4 : n4;
    hipStream_t s = (hipStream_t)stream;
    if (z_is_half)
        hipLaunchKernelGGL(ddim_v_step_kernel<true>, dim3(grid_for(n4)), dim3(256), 0, s, z, z0t_out, (const half_t*)v_uc,
                           (const half_t*)v_c, lam, k, tweedie_uc, renoise_uc, row_scale, row4, n4);
    else
        hipLaunchKernelGGL(ddim_v_step_kernel<false>, dim3(grid_for(n4)), dim3(256), 0, s, z, z0t_out, (const half_t*)v_uc,
                           (const half_t*)v_c, lam, k, tweedie_uc, renoise_uc, row_scale, row4, n4);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

int cfgpp_v_to_eps(void* eps_uc_out, void* eps_c_out, const void* v_uc, const void* v_c, const void* x, int x_is_half, float a, float s,
                   long n, void* stream) {
    CFGPP_REQUIRE(n > 0 && (n % 4) == 0, "cfgpp_v_to_eps: n=%ld must be a positive multiple of 4", n);
    CFGPP_REQUIRE(eps_uc_out && eps_c_out && v_uc && v_c && x, "cfgpp_v_to_eps: null pointer");
    CFGPP_REQUIRE(x_is_half, "cfgpp_v_to_eps: an fp32 x is not supported (the Karras-sigma loops keep fp16 latents)");
    const long n4 = n / 4;
    hipLaunchKernelGGL(v_to_eps_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, (half_t*)eps_uc_out, (half_t*)eps_c_out,
                       (const half_t*)v_uc, (const half_t*)v_c, (const half_t*)x, a, s, n4);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

int cfgpp_cfg_rescale(const void* v_uc, const void* v_c, float lam, float phi, float* row_scale_out, int B, long row_elems, void* stream) {
    CFGPP_REQUIRE(v_uc && v_c && row_scale_out, "cfgpp_cfg_rescale: null pointer");
    CFGPP_REQUIRE(B >= 1 && B <= 65535, "cfgpp_cfg_rescale: B=%d", B);
    CFGPP_REQUIRE(row_elems >= 4 && (row_elems % 4) == 0 && row_elems <= (1L << 24),
                  "cfgpp_cfg_rescale: row_elems=%ld must be a multiple of 4 in 4 .. 2^24", row_elems);
    hipLaunchKernelGGL(cfg_rescale_kernel, dim3(B), dim3(RS_THREADS), 0, (hipStream_t)stream, (const half_t*)v_uc, (const half_t*)v_c,
                       lam, phi, row_scale_out, row_elems / 4);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
