// Image-to-image / latent hires-fix start (include/cfgpp_img2img.h): x = a * resample(src) + s * n in ONE launch - the resample of
// the source latent (identity, nearest-exact, bilinear, bicubic; torch's align_corners=False conventions on exact integer-rational
// coordinates), the noise (a caller's tensor, or drawn in registers from the generator of csrc/philox.h, stream id 4, draw 0), both
// products, the sum and the cast to the loop's latent dtype.
//
// Rounding contract: the header's; as in sde_kernels.hip every rounding is explicit and this file is built with -ffp-contract=off
// and without fast-math; the in-register draw is philox_normal4, the instruction sequence of cfgpp_philox_normal's fill, hence the
// same bits.
//
// The grid is sde_kernels.hip's: (blocks over a row's 4-element groups, chain), the chain's key read from the kernel arguments.  A
// thread owns one Philox group: 4 consecutive elements of the chain's row [C][h][w].  For w % 4 != 0 a group straddles image rows
// and planes, so (c, y, x) is derived per element, never per group.  Source taps are scalar gathers (2 or 4 B), every index clamped
// into its plane; the output goes out as one 16-byte (fp32) or 8-byte (fp16) store per group.
//
// Launch-bound at latent sizes (SD1.5 b8: 131 072 elements, SDXL b2: 131 072): the axis weights are recomputed per element in fp64
// rather than tabulated - a table would be a second launch or an upload (measured: profiles/img2img/README.md).
#include "common.h"
#include "step_math.h"
#include "philox.h"
#include "../../include/cfgpp_img2img.h"

namespace {

constexpr int I2I_MAX_SIDE = 2048;        // 2 out in < 2^24: the coordinate integers are exact in int32 (and in fp32 / fp64)
constexpr double CUBIC_A = -0.75;

struct I2IGeom {
    int C, h0, w0, h, w;
    int src_rows, x_half;
    int b0;                               // first chain of this launch (the source row of chain b is b0 + b, or 0)
};

// the taps of one output index along one axis: ntaps(MODE) of them, ascending, indices already inside [0, in)
constexpr int ntaps(int mode) { return mode <= 1 ? 1 : (mode == 2 ? 2 : 4); }
template <int MODE>
struct Taps {
    int i[ntaps(MODE)];
    float w[ntaps(MODE)];
};

static __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static __device__ __forceinline__ double cubic1(double u) { return ((CUBIC_A + 2.0) * u - (CUBIC_A + 3.0)) * u * u + 1.0; }
static __device__ __forceinline__ double cubic2(double u) { return ((CUBIC_A * u - 5.0 * CUBIC_A) * u + 8.0 * CUBIC_A) * u - 4.0 * CUBIC_A; }

template <int MODE>
static __device__ __forceinline__ void axis_taps(int d, int in, int out, Taps<MODE>& t) {
    const int den = 2 * out;
    if constexpr (MODE == 0) {
        t.i[0] = d; t.w[0] = 1.f;
    } else if constexpr (MODE == 1) {     // nearest-exact: floor((d + 0.5) in / out)
        const int q = ((2 * d + 1) * in) / den;
        t.i[0] = q < in - 1 ? q : in - 1; t.w[0] = 1.f;
    } else if constexpr (MODE == 2) {     // bilinear: a negative coordinate is 0
        const int num = (2 * d + 1) * in - out;
        int q = 0, rem = 0;
        if (num > 0) { q = num / den; rem = num - q * den; }
        t.i[0] = clampi(q, 0, in - 1);
        t.i[1] = clampi(q + 1, 0, in - 1);
        t.w[0] = (float)((double)(den - rem) / (double)den);
        t.w[1] = (float)((double)rem / (double)den);
    } else {                              // bicubic: floor division, the coordinate is not clamped (its taps are)
        const int num = (2 * d + 1) * in - out;
        int q = num / den, rem = num - q * den;
        if (rem < 0) { rem += den; q -= 1; }
        const double tt = (double)rem / (double)den, omt = (double)(den - rem) / (double)den;
#pragma unroll
        for (int k = 0; k < 4; ++k) t.i[k] = clampi(q - 1 + k, 0, in - 1);
        t.w[0] = (float)cubic2(tt + 1.0);
        t.w[1] = (float)cubic1(tt);
        t.w[2] = (float)cubic1(omt);
        t.w[3] = (float)cubic2(omt + 1.0);
    }
}

template <bool SRC_HALF>
static __device__ __forceinline__ float src_at(const void* p, long i) {
    return SRC_HALF ? (float)reinterpret_cast<const half_t*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}

// r of the header for element e of a chain's row; row_base: the source offset of (source row, channel 0)
template <bool SRC_HALF, int MODE>
static __device__ __forceinline__ float resample_at(const void* src, long row_base, long e, const I2IGeom& g) {
    constexpr int NT = ntaps(MODE);
    const int hw = g.h * g.w;
    const int c = (int)(e / hw);
    const int rem = (int)(e - (long)c * hw);
    const int y = rem / g.w, xx = rem - y * g.w;
    const long plane = row_base + (long)c * g.h0 * g.w0;
    Taps<MODE> ty, tx;
    axis_taps<MODE>(y, g.h0, g.h, ty);
    axis_taps<MODE>(xx, g.w0, g.w, tx);
    if constexpr (NT == 1) {
        return src_at<SRC_HALF>(src, plane + (long)ty.i[0] * g.w0 + tx.i[0]);
    } else {
        float r = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const long line = plane + (long)ty.i[j] * g.w0;
            float row = __fmul_rn(tx.w[0], src_at<SRC_HALF>(src, line + tx.i[0]));
#pragma unroll
            for (int k = 1; k < NT; ++k) row = __fadd_rn(row, __fmul_rn(tx.w[k], src_at<SRC_HALF>(src, line + tx.i[k])));
            const float term = __fmul_rn(ty.w[j], row);
            r = j == 0 ? term : __fadd_rn(r, term);
        }
        return r;
    }
}

// NOISE: 0 no noise term (s == 0), 1 a caller-supplied fp32 tensor, 2 drawn in registers.  MODE: the resample (a template
// parameter, so that the tap arrays have a fixed size and stay in registers).  use_src: a != 0.
template <int NOISE, bool SRC_HALF, int MODE>
__global__ void __launch_bounds__(256)
img2img_start_kernel(void* __restrict__ x, const void* __restrict__ src, const float* __restrict__ noise, float a, float s, I2IGeom g,
                     int use_src, PhiloxKeys keys, long row4) {
    const int b = blockIdx.y;
    const uint32_t k0 = keys.k[b][0], k1 = keys.k[b][1];
    const long stride = (long)gridDim.x * blockDim.x;
    const long src_row = g.src_rows == 1 ? 0 : (long)(g.b0 + b);
    const long row_base = src_row * g.C * g.h0 * g.w0;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < row4; q += stride) {
        const long i = (long)b * row4 + q;            // the group's index in this launch's slice of x / noise
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (NOISE == 1) {
            const float4 v = reinterpret_cast<const float4*>(noise)[i];
            nz[0] = v.x; nz[1] = v.y; nz[2] = v.z; nz[3] = v.w;
        } else if (NOISE == 2) {
            philox_normal4((uint32_t)q, 0u, 4u, k0, k1, nz);
        }
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.f;
            if (use_src) acc = __fmul_rn(a, resample_at<SRC_HALF, MODE>(src, row_base, 4 * q + j, g));
            if (NOISE != 0) {
                const float sn = __fmul_rn(s, nz[j]);
                acc = use_src ? __fadd_rn(acc, sn) : sn;
            }
            o[j] = acc;
        }
        if (g.x_half) {
            half4_t ov;
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = (half_t)h_round(o[j]);
            reinterpret_cast<half4_t*>(x)[i] = ov;
        } else {
            reinterpret_cast<float4*>(x)[i] = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

inline bool finite_f(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" {

int cfgpp_img2img_start(void* x, const void* src, const void* noise, const unsigned long long* seeds_host, float a, float s, int B,
                        int src_rows, int C, int h0, int w0, int h, int w, int mode, int x_half, int src_half, void* stream) {
    CFGPP_REQUIRE(x, "cfgpp_img2img_start: null pointer (x)");
    CFGPP_REQUIRE(B >= 1 && C >= 1, "cfgpp_img2img_start: B=%d C=%d", B, C);
    CFGPP_REQUIRE(mode >= 0 && mode <= 3, "cfgpp_img2img_start: mode=%d (0 identity, 1 nearest-exact, 2 bilinear, 3 bicubic)", mode);
    CFGPP_REQUIRE(h0 >= 1 && w0 >= 1 && h >= 1 && w >= 1 && h <= I2I_MAX_SIDE && w <= I2I_MAX_SIDE,
                  "cfgpp_img2img_start: source %d x %d, target %d x %d: sides in 1 .. %d", h0, w0, h, w, I2I_MAX_SIDE);
    CFGPP_REQUIRE(h0 <= h && w0 <= w, "cfgpp_img2img_start: source %d x %d is larger than the target %d x %d: downscaling is not built",
                  h0, w0, h, w);
    CFGPP_REQUIRE(mode != 0 || (h0 == h && w0 == w), "cfgpp_img2img_start: mode 0 (identity) with source %d x %d for target %d x %d", h0,
                  w0, h, w);
    CFGPP_REQUIRE(src_rows == 1 || src_rows == B, "cfgpp_img2img_start: src_rows=%d (1 or B=%d)", src_rows, B);
    const long row_elems = (long)C * h * w;
    CFGPP_REQUIRE((row_elems % 4) == 0 && row_elems < (1L << 34), "cfgpp_img2img_start: C h w = %ld must be a multiple of 4 below 2^34",
                  row_elems);
    CFGPP_REQUIRE(finite_f(a) && finite_f(s), "cfgpp_img2img_start: a or s is not finite");
    CFGPP_REQUIRE(a != 0.f || s != 0.f, "cfgpp_img2img_start: a == 0 and s == 0: nothing to write");
    CFGPP_REQUIRE(a == 0.f || src, "cfgpp_img2img_start: a != 0 needs src");
    const int nmode = s == 0.f ? 0 : (noise ? 1 : 2);
    CFGPP_REQUIRE(nmode != 2 || seeds_host, "cfgpp_img2img_start: s != 0 needs noise or seeds_host");
    CFGPP_REQUIRE(((uintptr_t)x % (x_half ? 8 : 16)) == 0, "cfgpp_img2img_start: x must be %d-byte aligned", x_half ? 8 : 16);
    CFGPP_REQUIRE(nmode != 1 || ((uintptr_t)noise % 16) == 0, "cfgpp_img2img_start: noise must be 16-byte aligned");
    const long row4 = row_elems / 4;
    const int use_src = a != 0.f;
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += PHILOX_ROWS) {
        const int rows = B - b0 < PHILOX_ROWS ? B - b0 : PHILOX_ROWS;
        PhiloxKeys keys;
        philox_fill_keys(keys, nmode == 2 ? seeds_host + b0 : nullptr, rows);
        const long off = (long)b0 * row_elems;
        void* xp = x_half ? (void*)((half_t*)x + off) : (void*)((float*)x + off);
        const float* np = nmode == 1 ? (const float*)noise + off : nullptr;
        const I2IGeom g{C, h0, w0, h, w, src_rows, x_half != 0, b0};
        const dim3 grid(philox_row_grid(row4), rows);
#define CFGPP_I2I_LAUNCH(N, SH, M) \
        hipLaunchKernelGGL((img2img_start_kernel<N, SH, M>), grid, dim3(256), 0, st, xp, src, np, a, s, g, use_src, keys, row4)
#define CFGPP_I2I_MODE(N, SH) \
        do { if (mode == 0) CFGPP_I2I_LAUNCH(N, SH, 0); else if (mode == 1) CFGPP_I2I_LAUNCH(N, SH, 1); \
             else if (mode == 2) CFGPP_I2I_LAUNCH(N, SH, 2); else CFGPP_I2I_LAUNCH(N, SH, 3); } while (0)
        if (src_half) {
            if (nmode == 0) CFGPP_I2I_MODE(0, true); else if (nmode == 1) CFGPP_I2I_MODE(1, true); else CFGPP_I2I_MODE(2, true);
        } else {
            if (nmode == 0) CFGPP_I2I_MODE(0, false); else if (nmode == 1) CFGPP_I2I_MODE(1, false); else CFGPP_I2I_MODE(2, false);
        }
#undef CFGPP_I2I_MODE
#undef CFGPP_I2I_LAUNCH
        CFGPP_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
