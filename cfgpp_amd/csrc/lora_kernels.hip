// LoRA weight merge on the device (cfgpp_unet_lora, unet.hip): W = fp16(float(base) + up x down), written straight into the
// REPACKED layout the forward kernels read - the kernel owns the address map of every layout the Builder produces
// (engine_base.h), so there is no checkpoint-order temporary and no second repack pass.
//
//   up   [O][rank] fp32, down [rank][I * taps] fp32 in the checkpoint's own OIHW flattening (column = i * taps + tap)
//   base / dst: the parameter's O rows of I * taps fp16 in the repacked layout (dst: first row of the parameter inside its
//               possibly row-concatenated matrix; base: the copy finalize's upload left, saved by the engine)
//
// A workgroup (4 waves) owns a 32 x 128 tile of the DESTINATION: wave w rows 8w .. 8w + 7, lane l columns 2l, 2l + 1 - a wave
// stores 256 contiguous bytes per row.  The rank axis is walked in chunks of 32 through LDS: down_s[r][col] is staged by
// destination column (the conv3x3 gather happens on the way in, from the small L2-resident `down`), up_s[r][row] by
// destination row (the GEGLU interleave likewise), so the inner loop is two 16-byte broadcast reads of `up`, one 8-byte read
// of `down` (32 lanes x 8 B = one 256-B bank row: conflict-free) and 16 FMAs.  fp32 accumulation in a fixed order: the same
// inputs give the same bits; one rounding at the end.
#include "common.h"

namespace {

constexpr int LORA_BO = 32, LORA_BK = 128, LORA_RC = 32, LORA_UP_LD = 36;      // 36 floats: rows stay 16-byte aligned

// KIND: 0 rows and columns as in the checkpoint, 1 conv3x3 columns [I/64][tap][64], 2 GEGLU rows (per 64: 32 value rows f,
// then the 32 gate rows O/2 + f)
template <int KIND>
__global__ __launch_bounds__(256) void lora_merge_kernel(const half_t* __restrict__ base, half_t* __restrict__ dst,
                                                         const float* __restrict__ up, const float* __restrict__ down, int rank,
                                                         int O, int Kc, int taps, int vec2) {
    __shared__ __attribute__((aligned(16))) float up_s[LORA_RC][LORA_UP_LD];
    __shared__ __attribute__((aligned(16))) float down_s[LORA_RC][LORA_BK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.y * LORA_BO, k0 = blockIdx.x * LORA_BK;

    // staging coordinates: `up` by (rank index fast, 8 rows per pass), `down` by (column fast, 2 rank indices per pass)
    const int u_r = tid & 31, u_row = tid >> 5;
    const int d_col = tid & 127, d_r = tid >> 7;
    long u_src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = p0 + u_row + 8 * i;
        long o = p;
        if (KIND == 2) { const int w = p & 63; o = (long)(p >> 6) * 32 + (w & 31) + (w >= 32 ? O / 2 : 0); }
        u_src[i] = p < O ? o * rank : -1;
    }
    long d_src = -1;
    {
        const int k = k0 + d_col;
        if (k < Kc) {
            d_src = k;
            if (KIND == 1) { const int q = k >> 6; d_src = ((long)(q / taps) * 64 + (k & 63)) * taps + q % taps; }
        }
    }

    float acc[8][2];
#pragma unroll
    for (int i = 0; i < 8; ++i) { acc[i][0] = 0.f; acc[i][1] = 0.f; }

    for (int r0 = 0; r0 < rank; r0 += LORA_RC) {
        const bool u_live = r0 + u_r < rank;
#pragma unroll
        for (int i = 0; i < 4; ++i) up_s[u_r][u_row + 8 * i] = (u_live && u_src[i] >= 0) ? up[u_src[i] + r0 + u_r] : 0.f;
#pragma unroll
        for (int i = 0; i < LORA_RC / 2; ++i) {
            const int r = r0 + d_r + 2 * i;
            down_s[d_r + 2 * i][d_col] = (d_src >= 0 && r < rank) ? down[(long)r * Kc + d_src] : 0.f;
        }
        __syncthreads();
        const int rn = min(LORA_RC, rank - r0);
#pragma unroll 4
        for (int r = 0; r < rn; ++r) {
            const float2 d = *reinterpret_cast<const float2*>(&down_s[r][2 * lane]);
            const float4 a = *reinterpret_cast<const float4*>(&up_s[r][8 * wave]);
            const float4 b = *reinterpret_cast<const float4*>(&up_s[r][8 * wave + 4]);
            const float uu[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) { acc[i][0] = fmaf(uu[i], d.x, acc[i][0]); acc[i][1] = fmaf(uu[i], d.y, acc[i][1]); }
        }
        __syncthreads();
    }

    const int k = k0 + 2 * lane;
    if (k >= Kc) return;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = p0 + 8 * wave + i;
        if (p >= O) break;
        const long off = (long)p * Kc + k;
        if (vec2) {                                        // Kc even: both columns are in range and the pair is 4-byte aligned
            const half2_t w = *reinterpret_cast<const half2_t*>(base + off);
            half2_t o;
            o.x = (half_t)((float)w.x + acc[i][0]); o.y = (half_t)((float)w.y + acc[i][1]);
            *reinterpret_cast<half2_t*>(dst + off) = o;
        } else {
            dst[off] = (half_t)((float)base[off] + acc[i][0]);
            if (k + 1 < Kc) dst[off + 1] = (half_t)((float)base[off + 1] + acc[i][1]);
        }
    }
}

// Folded weights of the 2x2 phase form of `nearest-2x upsample -> conv3x3` (IGemmArgs::amode 4).  Output pixel y = 2i + p reads,
// through tap t (dy = t - 1), source row i + floor((p + t - 1) / 2); with the 2-tap index a reading source row i + p - 1 + a:
// p = 0: a = 0 <- {t = 0}, a = 1 <- {t = 1, 2};  p = 1: a = 0 <- {t = 0, 1}, a = 1 <- {t = 2}.  2-D is the outer product, so a folded
// weight is the sum of 1, 2, 2 or 4 taps: summed in fp32 in a fixed order (t ascending, then s ascending), rounded ONCE to fp16.
//   w9 [O][I/64][9][64]  (SLOT_CONV3)   ->   w4 [4 phases = 2 py + px][O][I/64][4 taps = 2 a + b][64]
// One thread per 8 consecutive channels of one folded tap.
__global__ __launch_bounds__(256) void fold_upsample_kernel(const half_t* __restrict__ w9, half_t* __restrict__ w4, long O, long CB) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;          // ((((phase * O + o) * CB + cb) * 4 + tap) * 8 + c8
    if (idx >= 4 * O * CB * 32) return;
    const int c8 = (int)(idx & 7), tap = (int)((idx >> 3) & 3);
    const long r = idx >> 5, cb = r % CB, po = r / CB, o = po % O;
    const int phase = (int)(po / O);
    const int py = phase >> 1, px = phase & 1, a = tap >> 1, b = tap & 1;
    // taps [lo, hi] of one axis: (p, a) = (0, 0) -> 0..0, (0, 1) -> 1..2, (1, 0) -> 0..1, (1, 1) -> 2..2
    const int t0 = a == 0 ? 0 : 1 + py, t1 = a == 0 ? py : 2;
    const int s0 = b == 0 ? 0 : 1 + px, s1 = b == 0 ? px : 2;
    const half_t* src = w9 + ((o * CB + cb) * 9) * 64 + c8 * 8;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    for (int t = t0; t <= t1; ++t)
        for (int s = s0; s <= s1; ++s) {
            const half8_t v = *reinterpret_cast<const half8_t*>(src + (t * 3 + s) * 64);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[k] += (float)v[k];
        }
    half8_t out;
#pragma unroll
    for (int k = 0; k < 8; ++k) out[k] = (half_t)acc[k];
    *reinterpret_cast<half8_t*>(w4 + idx * 8) = out;
}

}  // namespace

// engine-internal launcher (engine_base.h; cfgpp_op_fold_upsample): w9 = a conv3x3 weight in the repacked layout, w4 = 16 * O * I halfs
int igemm_fold_upsample_launch(const half_t* w9, half_t* w4, long O, long I, hipStream_t s) {
    CFGPP_REQUIRE(w9 && w4 && O > 0 && I > 0 && I % 64 == 0 && O * I < (1L << 34), "fold_upsample: bad args (O=%ld, I=%ld: a multiple of 64)", O, I);
    const long n = 4 * O * (I / 64) * 32;
    hipLaunchKernelGGL(fold_upsample_kernel, dim3((unsigned)cdiv(n, 256L)), dim3(256), 0, s, w9, w4, O, I / 64);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

// engine-internal launcher (unet.hip).  kind: 0 plain, 1 conv3x3 repack (I % 64 == 0), 2 GEGLU interleave (O % 64 == 0)
int lora_merge_launch(const half_t* base, half_t* dst, const float* up, const float* down, int rank, int kind, long O, long I,
                      int taps, hipStream_t s) {
    const long Kc = I * taps;
    CFGPP_REQUIRE(base && dst && up && down && rank > 0 && O > 0 && Kc > 0 && O < (1L << 30) && Kc < (1L << 30), "lora_merge: bad args");
    CFGPP_REQUIRE(kind != 1 || I % 64 == 0, "lora_merge: conv3x3 repack with %ld input channels (a multiple of 64)", I);
    CFGPP_REQUIRE(kind != 2 || O % 64 == 0, "lora_merge: GEGLU interleave with %ld rows (a multiple of 64)", O);
    const dim3 grid((unsigned)cdiv(Kc, LORA_BK), (unsigned)cdiv(O, LORA_BO));
    CFGPP_REQUIRE(grid.y <= 65535u, "lora_merge: %ld rows", O);
    const int vec2 = Kc % 2 == 0 ? 1 : 0;
    if (kind == 1) hipLaunchKernelGGL(lora_merge_kernel<1>, grid, dim3(256), 0, s, base, dst, up, down, rank, (int)O, (int)Kc, taps, vec2);
    else if (kind == 2) hipLaunchKernelGGL(lora_merge_kernel<2>, grid, dim3(256), 0, s, base, dst, up, down, rank, (int)O, (int)Kc, taps, vec2);
    else hipLaunchKernelGGL(lora_merge_kernel<0>, grid, dim3(256), 0, s, base, dst, up, down, rank, (int)O, (int)Kc, taps, vec2);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}
