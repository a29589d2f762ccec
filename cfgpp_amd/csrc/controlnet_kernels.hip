// ControlNet kernels (diffusers ControlNetModel / StableDiffusion(XL)ControlNetPipeline, one net, non-guess mode):
//   * the conditioning-embedding convolutions (controlnet_cond_embedding.conv_in / blocks.N): 3x3, pad 1, stride 1 or 2,
//     a few dozen channels at the full image size - too narrow for the implicit GEMM (64-channel blocks) and too wide for
//     conv_in_kernel (<= 16 input channels).  Once per job, so a plain direct convolution;
//   * the multi-tensor scaled residual add of the controlled UNet: every skip connection and the mid-block output
//     get `+ residual * conditioning_scale` in ONE launch that walks a device table.
// Built with -ffp-contract=off: the residual add is torch's fp16 `s + r * scale`, bit for bit.
#include <algorithm>

#include "common.h"
#include "../../include/cfgpp.h"
#include "cfgpp_debug.h"

namespace {

// One output (row, y, x, co) per thread, output channel fastest: the lanes of a wave share an input pixel (one broadcast
// load) and read consecutive weights (w [tap][ci][co] fp32).  fp32 accumulation; the result is rounded to fp16, then
// SiLU (silu = 1) is applied and rounded again - torch's conv2d then F.silu on fp16 tensors.
// in_kind 0: dense NHWC fp16 [R][Hi][Wi][Ci]; 1 / 2: NCHW fp16 / fp32 [R][Ci][Hi][Wi] (the control image; fp32 values are
// rounded to fp16 first, as the pipeline hands the net an fp16 image).  out_pad 0: dense NHWC [R][Ho][Wo][Co]; 1: halo-padded
// NHWC [R][Ho+2][Wo+2][Co] (interior only; the halo is not touched).
template <int KIND>
__global__ void __launch_bounds__(256)
cn_conv3x3_kernel(const void* __restrict__ in_, half_t* __restrict__ out, const float* __restrict__ w, const float* __restrict__ bias,
                  int Ci, int Co, int Hi, int Wi, int Ho, int Wo, int stride, int silu, int out_pad, long total) {
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int co = (int)(idx % Co);
        long p = idx / Co;
        const int xo = (int)(p % Wo); p /= Wo;
        const int yo = (int)(p % Ho);
        const int r = (int)(p / Ho);
        float acc = bias ? bias[co] : 0.f;
        for (int ky = 0; ky < 3; ++ky) {
            const int y = yo * stride + ky - 1;
            if (y < 0 || y >= Hi) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int x = xo * stride + kx - 1;
                if (x < 0 || x >= Wi) continue;
                const float* wp = w + (long)(ky * 3 + kx) * Ci * Co + co;
                if (KIND == 0) {
                    const half_t* ip = (const half_t*)in_ + (((long)r * Hi + y) * Wi + x) * Ci;
                    for (int ci = 0; ci < Ci; ++ci) acc += wp[(long)ci * Co] * (float)ip[ci];
                } else {
                    const long plane = (long)Hi * Wi, base = (long)r * Ci * plane + (long)y * Wi + x;
                    for (int ci = 0; ci < Ci; ++ci) {
                        const float v = KIND == 1 ? (float)((const half_t*)in_)[base + ci * plane]
                                                  : (float)(half_t)((const float*)in_)[base + ci * plane];
                        acc += wp[(long)ci * Co] * v;
                    }
                }
            }
        }
        half_t h = (half_t)acc;
        if (silu) {
            const float v = (float)h;
            h = (half_t)(v / (1.0f + expf(-v)));
        }
        const long o = out_pad ? (((long)r * (Ho + 2) + yo + 1) * (Wo + 2) + xo + 1) * Co : (((long)r * Ho + yo) * Wo + xo) * Co;
        out[o + co] = h;
    }
}

// blockIdx.y = table entry; dst = half(float(dst) + float(half(float(src) * scale))) - torch's fp16 `s + r * scale` - over the
// interior pixels of `rows`
// rows, 8 channels per thread (C % 8 == 0, 16-byte aligned rows).  The halo is neither read nor written.
__global__ void __launch_bounds__(256)
cn_residual_add_kernel(const CnAddEntry* __restrict__ tab, int rows, float scale) {
    const CnAddEntry e = tab[blockIdx.y];
    const int C8 = e.C >> 3;
    const long n = (long)rows * e.H * e.W * C8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c8 = (int)(i % C8);
        long p = i / C8;
        const int x = (int)(p % e.W); p /= e.W;
        const int y = (int)(p % e.H);
        const int r = (int)(p / e.H);
        const long off = (((long)r * (e.H + 2) + y + 1) * (e.W + 2) + x + 1) * e.C + (long)c8 * 8;
        half8_t d = *(const half8_t*)(e.dst + off);
        const half8_t s = *(const half8_t*)(e.src + off);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            // torch rounds the product to fp32, then to fp16; the empty asm keeps the compiler from fusing mul + convert into
            // v_fma_mixlo_f16, which rounds the exact product once (step_kernels.hip: h_round)
            float p = __fmul_rn((float)s[k], scale);
            asm volatile("" : "+v"(p));
            d[k] = (half_t)__fadd_rn((float)d[k], (float)(half_t)p);
        }
        *(half8_t*)(e.dst + off) = d;
    }
}

// residual (halo-padded NHWC fp16) * scale, rounded to fp16, as dense fp32 NCHW - the test hook's view of one residual
__global__ void __launch_bounds__(256)
cn_residual_nchw_kernel(const half_t* __restrict__ src, float* __restrict__ out, int H, int W, int C, float scale, long total) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        long p = i / W;
        const int y = (int)(p % H); p /= H;
        const int c = (int)(p % C);
        const int r = (int)(p / C);
        const half_t v = src[(((long)r * (H + 2) + y + 1) * (W + 2) + x + 1) * C + c];
        float q = __fmul_rn((float)v, scale);
        asm volatile("" : "+v"(q));
        out[i] = (float)(half_t)q;
    }
}

inline int grid_for(long total) { return (int)std::min<long>(std::max<long>(cdiv(total, 256), 1), 1L << 20); }

}  // namespace

// engine-internal launcher of the residual add (unet.hip): tab = n device entries, max_n8 = the largest entry's
// rows * H * W * C / 8 at max rows (sizes the grid)
int cn_residual_add_launch(const CnAddEntry* tab, int n, long max_n8, int rows, float scale, hipStream_t s) {
    if (n <= 0) return 0;
    dim3 grid((unsigned)std::min<long>(std::max<long>(cdiv(max_n8, 256), 1), 2048), (unsigned)n);
    hipLaunchKernelGGL(cn_residual_add_kernel, grid, dim3(256), 0, s, tab, rows, scale);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" {

int cfgpp_op_cn_conv3x3(const void* in, int in_kind, void* out, int out_pad, const float* w, const float* bias, int R, int Ci, int Co,
                        int Hi, int Wi, int stride, int silu, void* stream) {
    CFGPP_REQUIRE(in && out && w && R > 0 && Hi > 0 && Wi > 0, "cn_conv3x3: bad args");
    CFGPP_REQUIRE(Ci >= 1 && Ci <= 256 && Co >= 1 && Co <= 256, "cn_conv3x3: Ci=%d Co=%d (1 .. 256)", Ci, Co);
    CFGPP_REQUIRE(stride == 1 || stride == 2, "cn_conv3x3: stride %d (1 or 2)", stride);
    CFGPP_REQUIRE(in_kind >= 0 && in_kind <= 2, "cn_conv3x3: in_kind %d", in_kind);
    const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
    const long total = (long)R * Ho * Wo * Co;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(grid_for(total));
    if (in_kind == 0)
        hipLaunchKernelGGL(cn_conv3x3_kernel<0>, grid, dim3(256), 0, s, in, (half_t*)out, w, bias, Ci, Co, Hi, Wi, Ho, Wo, stride, silu, out_pad, total);
    else if (in_kind == 1)
        hipLaunchKernelGGL(cn_conv3x3_kernel<1>, grid, dim3(256), 0, s, in, (half_t*)out, w, bias, Ci, Co, Hi, Wi, Ho, Wo, stride, silu, out_pad, total);
    else
        hipLaunchKernelGGL(cn_conv3x3_kernel<2>, grid, dim3(256), 0, s, in, (half_t*)out, w, bias, Ci, Co, Hi, Wi, Ho, Wo, stride, silu, out_pad, total);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

int cfgpp_op_residual_add(void* const* dst, const void* const* src, const int* hwc, int n, int rows, float scale, void* stream) {
    CFGPP_REQUIRE(dst && src && hwc && n > 0 && n <= 32 && rows > 0, "residual_add: bad args (n=%d, at most 32)", n);
    static CnAddEntry* d_tab = nullptr;      // test hook: one table for the process
    if (!d_tab) CFGPP_HIP_CHECK(hipMalloc(&d_tab, 32 * sizeof(CnAddEntry)));
    CnAddEntry h[32];
    long max_n8 = 0;
    for (int i = 0; i < n; ++i) {
        CFGPP_REQUIRE(dst[i] && src[i] && hwc[3 * i + 2] % 8 == 0, "residual_add: entry %d: null pointer or C %% 8 != 0", i);
        h[i] = CnAddEntry{(half_t*)dst[i], (const half_t*)src[i], hwc[3 * i], hwc[3 * i + 1], hwc[3 * i + 2], 0};
        max_n8 = std::max(max_n8, (long)rows * hwc[3 * i] * hwc[3 * i + 1] * (hwc[3 * i + 2] / 8));
    }
    hipStream_t s = (hipStream_t)stream;
    CFGPP_HIP_CHECK(hipStreamSynchronize(s));            // the previous call's launch may still read the table
    CFGPP_HIP_CHECK(hipMemcpy(d_tab, h, n * sizeof(CnAddEntry), hipMemcpyHostToDevice));
    return cn_residual_add_launch(d_tab, n, max_n8, rows, scale, s);
}

int cfgpp_op_residual_nchw(const void* src, float* out, int rows, int H, int W, int C, float scale, void* stream) {
    CFGPP_REQUIRE(src && out && rows > 0 && H > 0 && W > 0 && C > 0, "residual_nchw: bad args");
    const long total = (long)rows * C * H * W;
    hipLaunchKernelGGL(cn_residual_nchw_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const half_t*)src, out, H, W, C,
                       scale, total);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
