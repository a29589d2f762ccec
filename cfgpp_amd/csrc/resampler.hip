// Perceiver attention of the IP-Adapter "plus" Resampler (include/cfgpp_ip_plus.h) and the two small launches its executor in
// unet.hip needs beside the implicit GEMM and the LayerNorm: the erf GELU of the feed-forward and the broadcast of the learned
// latents.  Once per job, not per step.  No reference counterpart: the reference conditions on text only.
//
//   O[r, j, h*64 + :] = softmax_k( q[r, j, h] . k[r, k, h] / 8 ) v[r, k, h]        k over S image-token keys, THEN n_q latent keys
//
// Operands are token-major, exactly as the to_q / to_kv GEMMs store them (EPI_STORE, no head scatter, no permute launch):
//   q    [rows][n_q][inner]                  inner = heads * 64
//   kv_x [rows][S  ][2 * inner]              K in columns [0, inner), V in [inner, 2 inner)     to_kv(norm1(x))
//   kv_l [rows][n_q][2 * inner]              the same of the latents                             to_kv(norm2(latents))
//   o    [rows][n_q][inner]
// The two key sources are never concatenated: key g of the joint softmax is row g of kv_x for g < S and row g - S of kv_l otherwise.
//
// One wave per (row, head): n_q <= 32 queries are ONE 32-wide MFMA column block, so a (row, head) is a chain of 32-key tiles with
// nothing to share between waves; at the shipped geometries that is rows * heads = 80 .. 192 waves of 9 tiles each, a few
// microseconds beside the GEMMs around it.  Per 32-key tile (KT):
//   * S^T = K Q^T, four v_mfma_f32_32x32x16_f16 (A = 32 keys x 16 dims, B = 16 dims x 32 queries): both operands are 16-byte global
//     loads of the lane's own row - lane l holds key / query l % 32 and dims 16 ks + 8 (l / 32) .. + 7.  Q is loaded once.
//     Lane l then holds, for query l % 32, the scores of keys 8 (reg / 4) + 4 (l / 32) + reg % 4.
//   * scores * (1/8 * log2 e) in fp32 (the Resampler's q * 64^-1/4 and k * 64^-1/4, applied once), pad keys -inf, online softmax in
//     registers: running max per query (one __shfl_xor 32), P = exp2(s - m) rounded to fp16, the denominator summed from the
//     rounded P, O and l rescaled by exp2(m_old - m_new) on every tile.
//   * O^T += V^T P^T, four MFMAs (2 halves of the head dim x 2 k-steps of 16 keys).  B = the lane's own registers 8 tt .. 8 tt + 7
//     as fp16; A = V^T from LDS, where the tile was staged transposed with the keys in cfgpp_vt_pos order (bits 2 and 3 of the key
//     index swapped), which makes the lane's 8 k-slots one 16-byte read.  Pad keys stage zeros (0 x garbage must not make NaN).
//   * the next tile's K rows and V chunks are in flight while this one is computed.
// Pad queries (n_q .. 31) read zeros and store nothing.
#include "common.h"

namespace {

constexpr int KT = 32;              // keys per tile
constexpr int VT_LD = KT + 8;       // halfs per V^T row in LDS: 80 bytes, so the 16-byte reads of 8 consecutive rows spread over the banks

struct PerceiverArgs {
    const half_t* q; const half_t* kvx; const half_t* kvl;
    half_t* o;
    int heads, nq, S;
    float scale_log2e;              // 1/8 * log2(e)
};

__global__ void __launch_bounds__(64)
perceiver_attn_kernel(const PerceiverArgs a) {
    __shared__ __attribute__((aligned(16))) half_t vt[64 * VT_LD];
    const int lane = threadIdx.x, j = lane & 31, hi = lane >> 5;
    const int r = blockIdx.x / a.heads, h = blockIdx.x - r * a.heads;
    const long inner = (long)a.heads * 64, ldkv = 2 * inner;
    const int nk = a.S + a.nq;
    const int ntiles = (nk + KT - 1) / KT;
    const half8_t z8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // K row of joint key g (this head's 64 columns; V sits `inner` columns further); null for a pad
    auto key_row = [&](int g) -> const half_t* {
        if (g < a.S) return a.kvx + ((long)r * a.S + g) * ldkv + h * 64;
        if (g < nk) return a.kvl + ((long)r * a.nq + (g - a.S)) * ldkv + h * 64;
        return nullptr;
    };

    half8_t qf[4];
    {
        const half_t* qp = a.q + ((long)r * a.nq + j) * inner + h * 64 + 8 * hi;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = j < a.nq ? *reinterpret_cast<const half8_t*>(qp + 16 * ks) : z8;
    }

    half8_t kf[4], vr[4];
    auto load_tile = [&](int t0) {
        const half_t* kp = key_row(t0 + j);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kf[ks] = kp ? *reinterpret_cast<const half8_t*>(kp + 16 * ks + 8 * hi) : z8;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i;                    // chunk c: key c / 8 of the tile, dims 8 (c % 8) .. + 7
            const half_t* vp = key_row(t0 + (c >> 3));
            vr[i] = vp ? *reinterpret_cast<const half8_t*>(vp + inner + 8 * (c & 7)) : z8;
        }
    };

    float m = -INFINITY, l = 0.f;
    f32x16 oacc[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[dt][i] = 0.f;

    load_tile(0);
    for (int t = 0; t < ntiles; ++t) {
        const int t0 = t * KT;
        __syncthreads();                                    // the previous tile's V^T reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = lane + 64 * i, col = cfgpp_vt_pos(c >> 3), d0 = 8 * (c & 7);
#pragma unroll
            for (int e = 0; e < 8; ++e) vt[(d0 + e) * VT_LD + col] = vr[i][e];
        }
        half8_t kc[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kc[ks] = kf[ks];
        __syncthreads();
        if (t + 1 < ntiles) load_tile(t0 + KT);

        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kc[ks], qf[ks], s, 0, 0, 0);

        float mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = t0 + 8 * (i >> 2) + 4 * hi + (i & 3);
            s[i] = key < nk ? s[i] * a.scale_log2e : -INFINITY;
            mt = fmaxf(mt, s[i]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32));                 // finite: every tile holds at least one real key
        const float mn = fmaxf(m, mt);
        const float alpha = __builtin_amdgcn_exp2f(m - mn); // first tile: exp2(-inf) = 0
        m = mn;
        half8_t pf[2];
        float ls = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const half_t p = (half_t)__builtin_amdgcn_exp2f(s[i] - mn);
            pf[i >> 3][i & 7] = p;
            ls += (float)p;
        }
        l = l * alpha + ls;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
            for (int i = 0; i < 16; ++i) oacc[dt][i] *= alpha;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const half8_t vf = *reinterpret_cast<const half8_t*>(&vt[(32 * dt + j) * VT_LD + 16 * tt + 8 * hi]);
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[tt], oacc[dt], 0, 0, 0);
            }
        }
    }
    l += __shfl_xor(l, 32);
    if (j >= a.nq) return;
    const float inv = 1.0f / l;
    half_t* op = a.o + ((long)r * a.nq + j) * inner + h * 64 + 4 * hi;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            half4_t o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (half_t)(oacc[dt][4 * g + e] * inv);
            *reinterpret_cast<half4_t*>(op + 32 * dt + 8 * g) = o;
        }
}

// x = fp16(gelu_erf(x)) in place, 8 values per thread (the Resampler's feed-forward: nn.GELU() between two bias-free Linears)
__global__ void __launch_bounds__(256) gelu_inplace_kernel(half_t* x, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    half8_t v = *reinterpret_cast<const half8_t*>(x + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (half_t)gelu_erf_f((float)v[e]);
    *reinterpret_cast<half8_t*>(x + i * 8) = v;
}

// dst[r][i] = fp16(src[i]) for r < rows: the learned latents, one copy per batch row (n % 8 == 0)
__global__ void __launch_bounds__(256) broadcast_rows_kernel(const float* src, half_t* dst, long n8, int rows) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8 * rows) return;
    const long c = i % n8;
    half8_t v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (half_t)src[c * 8 + e];
    *reinterpret_cast<half8_t*>(dst + i * 8) = v;
}

}  // namespace

int perceiver_attn_launch(const half_t* q, const half_t* kvx, const half_t* kvl, half_t* o, int rows, int heads, int nq, int S, hipStream_t s) {
    CFGPP_REQUIRE(q && kvx && kvl && o, "perceiver_attention: null operand");
    CFGPP_REQUIRE(rows >= 1 && heads >= 1 && (long)rows * heads < (1L << 30), "perceiver_attention: rows=%d heads=%d", rows, heads);
    CFGPP_REQUIRE(nq >= 1 && nq <= 32, "perceiver_attention: n_q=%d (1 .. 32 queries per row and head)", nq);
    CFGPP_REQUIRE(S >= 1 && S <= 1024, "perceiver_attention: S=%d (1 .. 1024 image-token keys)", S);
    PerceiverArgs a;
    a.q = q; a.kvx = kvx; a.kvl = kvl; a.o = o; a.heads = heads; a.nq = nq; a.S = S;
    a.scale_log2e = 0.125f * 1.4426950408889634f;
    hipLaunchKernelGGL(perceiver_attn_kernel, dim3(rows * heads), dim3(64), 0, s, a);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

int gelu_inplace_launch(half_t* x, long n, hipStream_t s) {
    CFGPP_REQUIRE(x && n > 0 && n % 8 == 0, "gelu: n=%ld (a positive multiple of 8)", n);
    hipLaunchKernelGGL(gelu_inplace_kernel, dim3(cdiv(n / 8, 256)), dim3(256), 0, s, x, n / 8);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

int broadcast_rows_launch(const float* src, half_t* dst, long n, int rows, hipStream_t s) {
    CFGPP_REQUIRE(src && dst && n > 0 && n % 8 == 0 && rows >= 1, "broadcast_rows: n=%ld rows=%d", n, rows);
    hipLaunchKernelGGL(broadcast_rows_kernel, dim3(cdiv(n / 8 * rows, 256)), dim3(256), 0, s, src, dst, n / 8, rows);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

// the Resampler's GELU and latent broadcast on their own.  gelu_erf_f (common.h) is the Abramowitz-Stegun erfc with hardware rcp / exp2,
// not the erff of act_inplace (small_kernels.hip, the towers' act 1): another function in the last bits, so it keeps its kernel.
extern "C" int cfgpp_op_gelu_inplace(void* x, long n, void* stream) { return gelu_inplace_launch((half_t*)x, n, (hipStream_t)stream); }

extern "C" int cfgpp_op_broadcast_rows(const float* src, void* dst, long n, int rows, void* stream) {
    return broadcast_rows_launch(src, (half_t*)dst, n, rows, (hipStream_t)stream);
}

extern "C" int cfgpp_op_perceiver_attention(const void* q, const void* kv_x, const void* kv_l, void* o, int rows, int heads, int n_q,
                                            int S, void* stream) {
    return perceiver_attn_launch((const half_t*)q, (const half_t*)kv_x, (const half_t*)kv_l, (half_t*)o, rows, heads, n_q, S,
                                 (hipStream_t)stream);
}
