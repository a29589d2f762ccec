// FreeU (diffusers UNet2DConditionModel.enable_freeu / utils.torch_utils.apply_freeu, fourier_filter with threshold = 1) on the
// pair (hidden, skip) an up-path resnet concatenates, in place on halo-padded NHWC fp16, ONE launch:
//   * hidden[:, :C_h / 2] *= b                      - one fp16 rounding of float(h) * b;
//   * skip = Re(ifft2(mask * fft2(skip)))           - mask = s on the 2 x 2 block of frequencies {-1, 0} x {-1, 0}, 1 elsewhere.
// The filter needs no FFT: only four frequencies are scaled, so per plane (row, channel), with ty = 2 pi y / H, tx = 2 pi x / W,
//   A = sum v      B = sum v e^{+i ty}      C = sum v e^{+i tx}      D = sum v e^{+i (ty + tx)}
//   out[y, x] = v[y, x] + (s - 1) / (H W) * (A + Re(B e^{-i ty}) + Re(C e^{-i tx}) + Re(D e^{-i (ty + tx)}))
// (the mask is not Hermitian-symmetric - frequency -1 is scaled, +1 is not - and `.real` drops the imaginary part that leaves:
// the formula above is that real part).  Seven real fp32 sums per plane; cos / sin of ty and tx come from a table the HOST
// computed in double and rounded to fp32 (no device sincos), the diagonal twiddle is their fp32 product.
//
// Work split: one workgroup per (row, slab of CS = 8 * LPP channels) of the skip - lane l % LPP of a pixel holds 8 channels, a
// 16-byte load - followed by grid-stride workgroups over the scaled half of the hidden.  Resident path: the slab's H x W x CS
// values stay in LDS between the reduce and the apply (SDXL's 64 x 64 x 8 = 64 KiB), the skip is read once; planes that do not
// fit at CS = 8 take the two-phase path, which re-reads the slab from memory.  Only interiors are read and written.
#include <algorithm>
#include <cmath>
#include <map>
#include <utility>
#include <vector>

#include "freeu.h"
#include "../../include/cfgpp.h"
#include "cfgpp_debug.h"

namespace {

constexpr int FREEU_THREADS = 256;
constexpr int FREEU_LDS_PLANE_CAP = 64 * 1024;      // bytes of one resident slab (two workgroups per CU)
constexpr int FREEU_NSUM = 7;

// blocks [0, nskip): skip slabs; [nskip, gridDim.x): the hidden half.  tw = [cos ty (H) | sin ty (H) | cos tx (W) | sin tx (W)].
template <int LPP, bool RESIDENT>
__global__ void __launch_bounds__(FREEU_THREADS)
freeu_kernel(half_t* __restrict__ hidden, int C_h, half_t* __restrict__ skip, int C_s, int rows, int H, int W, float b, float k,
             const float* __restrict__ tw, int nskip) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x;
    if ((int)blockIdx.x >= nskip) {
        // ---- hidden[:, :C_h / 2] *= b over the interior pixels, 8 channels per thread ----
        const int C8 = C_h >> 4;                    // 16-byte chunks of the scaled half
        const long n = (long)rows * H * W * C8;
        const long nb = (long)gridDim.x - nskip;
        for (long i = ((long)blockIdx.x - nskip) * FREEU_THREADS + t; i < n; i += nb * FREEU_THREADS) {
            const int c8 = (int)(i % C8);
            long p = i / C8;
            const int x = (int)(p % W); p /= W;
            const int y = (int)(p % H);
            const int r = (int)(p / H);
            half_t* q = hidden + (((long)r * (H + 2) + y + 1) * (W + 2) + x + 1) * C_h + (long)c8 * 8;
            half8_t v = *(const half8_t*)q;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (half_t)((float)v[j] * b);
            *(half8_t*)q = v;
        }
        return;
    }
    // ---- skip low-pass: this workgroup owns row r, channels [c0, c0 + 8 * LPP) ----
    constexpr int CS = 8 * LPP, PSTEP = FREEU_THREADS / LPP;
    const int HW = H * W;
    const int nslab = C_s / CS;
    // blocks b and b + 8 share an XCD: hand them neighbouring slabs, whose pixels share cache lines (a permutation of the block ids)
    int L = (int)blockIdx.x;
    if (nskip % 8 == 0) L = (L % 8) * (nskip / 8) + L / 8;
    const int r = L / nslab, c0 = (L % nslab) * CS;
    half8_t* plane = (half8_t*)smem;                                            // RESIDENT: [HW][LPP] chunks
    float* tws = (float*)(smem + (RESIDENT ? (size_t)HW * CS * sizeof(half_t) : 0));   // 2 H + 2 W twiddles
    float* red = tws + 2 * H + 2 * W;                                           // [4 waves][LPP][7][8]
    for (int i = t; i < 2 * H + 2 * W; i += FREEU_THREADS) tws[i] = tw[i];
    __syncthreads();
    const float *cy = tws, *sy = tws + H, *cx = tws + 2 * H, *sx = tws + 2 * H + W;
    const int l = t % LPP, p0 = t / LPP;
    half_t* base = skip + (long)r * (H + 2) * (W + 2) * C_s + c0 + l * 8;
    float acc[FREEU_NSUM][8];
#pragma unroll
    for (int m = 0; m < FREEU_NSUM; ++m)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[m][j] = 0.f;
    for (int p = p0; p < HW; p += PSTEP) {
        const int y = p / W, x = p - y * W;
        const half8_t raw = *(const half8_t*)(base + ((long)(y + 1) * (W + 2) + x + 1) * C_s);
        if (RESIDENT) plane[p * LPP + l] = raw;
        const float wy_c = cy[y], wy_s = sy[y], wx_c = cx[x], wx_s = sx[x];
        const float wd_c = wy_c * wx_c - wy_s * wx_s, wd_s = wy_s * wx_c + wy_c * wx_s;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = (float)raw[j];
            acc[0][j] += v;
            acc[1][j] += v * wy_c; acc[2][j] += v * wy_s;
            acc[3][j] += v * wx_c; acc[4][j] += v * wx_s;
            acc[5][j] += v * wd_c; acc[6][j] += v * wd_s;
        }
    }
    // lanes of a wave that hold the same chunk (lane % LPP), then the four waves in a fixed order: deterministic
#pragma unroll
    for (int off = LPP; off < 64; off <<= 1)
#pragma unroll
        for (int m = 0; m < FREEU_NSUM; ++m)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[m][j] += __shfl_xor(acc[m][j], off);
    const int wave = t >> 6, lane = t & 63;
    if (lane < LPP) {
#pragma unroll
        for (int m = 0; m < FREEU_NSUM; ++m)
#pragma unroll
            for (int j = 0; j < 8; ++j) red[((wave * LPP + lane) * FREEU_NSUM + m) * 8 + j] = acc[m][j];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < FREEU_NSUM; ++m)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float s = red[((0 * LPP + l) * FREEU_NSUM + m) * 8 + j];
#pragma unroll
            for (int w = 1; w < FREEU_THREADS / 64; ++w) s += red[((w * LPP + l) * FREEU_NSUM + m) * 8 + j];
            acc[m][j] = s;
        }
    // ---- apply: every thread rewrites the pixels it read (its own LDS entries: no barrier needed) ----
    for (int p = p0; p < HW; p += PSTEP) {
        const int y = p / W, x = p - y * W;
        half_t* q = base + ((long)(y + 1) * (W + 2) + x + 1) * C_s;
        const half8_t raw = RESIDENT ? plane[p * LPP + l] : *(const half8_t*)q;
        const float wy_c = cy[y], wy_s = sy[y], wx_c = cx[x], wx_s = sx[x];
        const float wd_c = wy_c * wx_c - wy_s * wx_s, wd_s = wy_s * wx_c + wy_c * wx_s;
        half8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float low = acc[0][j] + (acc[1][j] * wy_c + acc[2][j] * wy_s) + (acc[3][j] * wx_c + acc[4][j] * wx_s) +
                              (acc[5][j] * wd_c + acc[6][j] * wd_s);
            o[j] = (half_t)((float)raw[j] + k * low);
        }
        *(half8_t*)q = k == 0.f ? raw : o;          // s = 1: the input's bits (-0 stays -0, a non-finite sum cannot leak in)
    }
}

int g_last[5] = {0, 0, 0, 0, 0};

template <int LPP>
int launch_lpp(bool resident, dim3 grid, size_t smem, hipStream_t st, half_t* hidden, int C_h, half_t* skip, int C_s, int rows, int H, int W,
               float b, float k, const float* tw, int nskip) {
    if (resident) {
        static bool attr = false;           // once per instance, on the first (eager) launch: never inside a stream capture
        if (!attr) {
            CFGPP_HIP_CHECK(hipFuncSetAttribute((const void*)freeu_kernel<LPP, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                FREEU_LDS_PLANE_CAP + 16384));       // + twiddles (H + W <= 1028) + partial sums
            attr = true;
        }
        hipLaunchKernelGGL((freeu_kernel<LPP, true>), grid, dim3(FREEU_THREADS), smem, st, hidden, C_h, skip, C_s, rows, H, W, b, k, tw, nskip);
    } else {
        hipLaunchKernelGGL((freeu_kernel<LPP, false>), grid, dim3(FREEU_THREADS), smem, st, hidden, C_h, skip, C_s, rows, H, W, b, k, tw, nskip);
    }
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

void freeu_twiddles(int H, int W, float* out) {
    const double two_pi = 6.283185307179586476925286766559;
    for (int y = 0; y < H; ++y) { out[y] = (float)std::cos(two_pi * y / H); out[H + y] = (float)std::sin(two_pi * y / H); }
    for (int x = 0; x < W; ++x) { out[2 * H + x] = (float)std::cos(two_pi * x / W); out[2 * H + W + x] = (float)std::sin(two_pi * x / W); }
}

// engine-internal launcher (unet.hip) and the body of cfgpp_op_freeu.  tw: device table of freeu_twiddles(H, W).
int freeu_launch(half_t* hidden, int C_h, half_t* skip, int C_s, int rows, int H, int W, float b, float s, const float* tw,
                 hipStream_t st) {
    for (int& v : g_last) v = 0;
    CFGPP_REQUIRE(hidden || skip, "freeu: both tensors are null");
    CFGPP_REQUIRE(rows > 0, "freeu: rows=%d", rows);
    CFGPP_REQUIRE(H >= 2 && W >= 2 && H <= 1024 && W <= 1024, "freeu: plane %d x %d (2 .. 1024 each way: the closed form of the filter does not hold for a "
                  "one-pixel axis)", H, W);
    CFGPP_REQUIRE(!hidden || (C_h > 0 && C_h % 16 == 0), "freeu: C_h=%d (the scaled half C_h / 2 must be a multiple of 8)", C_h);
    CFGPP_REQUIRE(!skip || (C_s > 0 && C_s % 8 == 0), "freeu: C_s=%d (a multiple of 8)", C_s);
    CFGPP_REQUIRE(std::isfinite(b) && std::isfinite(s), "freeu: non-finite scale (b=%f, s=%f)", (double)b, (double)s);
    CFGPP_REQUIRE(!skip || tw, "freeu: no twiddle table");
    const int HW = H * W;
    int cs = 0, nskip = 0;
    bool resident = false;
    if (skip) {
        // the widest slab (best coalescing) that still gives every CU a workgroup, resident if it fits; else the narrowest that fits
        resident = (long)HW * 8 * (long)sizeof(half_t) <= FREEU_LDS_PLANE_CAP;
        for (int c : {64, 32, 16, 8}) {
            if (C_s % c) continue;
            if (resident && (long)HW * c * (long)sizeof(half_t) > FREEU_LDS_PLANE_CAP) continue;
            cs = c;
            if ((long)rows * (C_s / c) >= 256) break;
        }
        nskip = rows * (C_s / cs);
    }
    int nhid = 0;
    if (hidden) nhid = (int)std::min<long>(std::max<long>(cdiv((long)rows * HW * (C_h / 16), FREEU_THREADS), 1), 2048);
    const int lpp = skip ? cs / 8 : 1;
    const size_t smem = skip ? (resident ? (size_t)HW * cs * sizeof(half_t) : 0) + (size_t)(2 * H + 2 * W) * sizeof(float) +
                                   (size_t)(FREEU_THREADS / 64) * lpp * FREEU_NSUM * 8 * sizeof(float)
                             : 0;
    const float k = (s - 1.0f) / (float)HW;
    const dim3 grid((unsigned)(nskip + nhid));
    int e = 0;
    switch (lpp) {
        case 8: e = launch_lpp<8>(resident, grid, smem, st, hidden, C_h, skip, C_s, rows, H, W, b, k, tw, nskip); break;
        case 4: e = launch_lpp<4>(resident, grid, smem, st, hidden, C_h, skip, C_s, rows, H, W, b, k, tw, nskip); break;
        case 2: e = launch_lpp<2>(resident, grid, smem, st, hidden, C_h, skip, C_s, rows, H, W, b, k, tw, nskip); break;
        default: e = launch_lpp<1>(resident, grid, smem, st, hidden, C_h, skip, C_s, rows, H, W, b, k, tw, nskip); break;
    }
    if (e) return e;
    g_last[0] = !skip ? 3 : resident ? 1 : 2; g_last[1] = cs; g_last[2] = nskip; g_last[3] = nhid; g_last[4] = (int)smem;
    return 0;
}

extern "C" {

int cfgpp_op_freeu(void* hidden, int C_h, void* skip, int C_s, int rows, int H, int W, float b, float s, void* stream) {
    for (int& v : g_last) v = 0;
    CFGPP_REQUIRE(H >= 2 && W >= 2 && H <= 1024 && W <= 1024, "freeu: plane %d x %d (2 .. 1024 each way: the closed form of the filter does not hold for a "
                  "one-pixel axis)", H, W);
    // test hook: one device table per plane size, kept for the process (the engine builds its own at finalize)
    static std::map<std::pair<int, int>, float*> tabs;
    float*& tw = tabs[std::make_pair(H, W)];
    if (!tw) {
        std::vector<float> h((size_t)2 * H + 2 * W);
        freeu_twiddles(H, W, h.data());
        CFGPP_HIP_CHECK(hipMalloc(&tw, h.size() * sizeof(float)));
        CFGPP_HIP_CHECK(hipMemcpy(tw, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return freeu_launch((half_t*)hidden, C_h, (half_t*)skip, C_s, rows, H, W, b, s, tw, (hipStream_t)stream);
}

void cfgpp_freeu_last_launch(int* out5) { for (int i = 0; i < 5; ++i) out5[i] = g_last[i]; }

}  // extern "C"
