// CLIP image tower on the engine's kernels (include/cfgpp_vision.h): `CLIPVisionModelWithProjection(pixel_values)` of `transformers`,
// the part of an IP-Adapter job that turns `ip_adapter_image=` into `image_embeds` / penultimate hidden states.  Runs once per job,
// off the per-step path.  No reference counterpart: the reference conditions on text only.  The twin of text.hip and built from the
// same parts - igemm linear layers (bias / residual epilogues), cfgpp_op_layernorm, cfgpp_op_skinny_gemm for the pooled projection.
// New here:
//   vit_preprocess_kernel   [N,3,H,W] fp32 in [0,1] -> fp16 pixel values [N,3,S,S]: antialiased bicubic resize of the short side to S,
//                           clamp, centre crop, CLIP mean / std, ONE launch (the two separable passes are evaluated per output pixel in
//                           torch's order: every input row's horizontal sum in fp32, then the vertical sum of those; the
//                           weights themselves in fp64, rounded to fp32 once)
//   vit_patch_rows_kernel   the im2col rows [N * P^2][Kp] of the patch convolution (stride = kernel = patch, no bias), K = 3 patch^2
//                           zero-padded to Kp (a multiple of 64: the implicit GEMM's K granule); a launch of its own, NOT fused with the
//                           preprocess store, because cfgpp_vision_encode takes pixel values as its input
//   vit_assemble_kernel     row 0 = class_embedding + pos[0], row 1 + p = patch[p] + pos[1 + p]
//   vit_attn_kernel         non-causal self-attention over T <= 320 tokens, head dims 64 / 80 / 104, reading the fused QKV GEMM's
//                           token-major output in place (the pattern of resampler.hip: no head scatter, no permute launch)
//
// vit_attn_kernel<D>: one wave per (row, head, block of 32 queries); the block is ONE 32-wide MFMA column block, so the wave walks a
// chain of 32-key tiles with nothing to share between waves.  qkv [rows][T][3 * hidden] (Q | K | V column blocks, head h at columns
// h * D of each), o [rows][T][hidden].  Per 32-key tile:
//   * S^T = K Q^T, DK = ceil(D / 16) v_mfma_f32_32x32x16_f16: lane l holds key / query l % 32 and dims 16 ks + 8 (l / 32) .. + 7, one
//     16-byte global load each.  Chunks at dims >= D are ZEROS on load (D = 104: the upper half of the seventh k-step) - no padded
//     buffer, the neighbouring head's columns are never read.  Q is loaded once.
//   * scores * (D^-1/2 * log2 e) in fp32, pad keys -inf, online softmax in registers: running max per query (one __shfl_xor 32),
//     P = exp2(s - m) rounded to fp16, the denominator summed from the ROUNDED P, O and l rescaled by exp2(m_old - m_new) per tile.
//   * O^T += V^T P^T, 2 * DT MFMAs (DT = ceil(D / 32) blocks of 32 output dims x 2 k-steps of 16 keys): B = the lane's own P registers,
//     A = V^T from LDS, staged transposed with the keys in cfgpp_vt_pos order so that the lane's 8 k-slots are one 16-byte read.  Pad
//     keys stage zeros (0 x garbage must not make NaN); LDS rows D .. 32 DT - 1 are zeroed once and produce output dims nobody stores.
//   * the next tile's K rows and V chunks are in flight while this one is computed.
// Pad queries (>= T, last block) read zeros and store nothing.
#include "engine_base.h"
#include "../../include/cfgpp_vision.h"

struct cfgpp_vision : EngineBase {
    int hidden = 0, layers = 0, heads = 0, d = 0, inter = 0, act = 0, proj = 0, S = 0, ps = 0, G = 0, T = 0, K = 0, Kp = 0, device = 0;
    bool finalized = false;
    // per-call state read by the plan's closures
    const half_t* in_pixels = nullptr;
    int out_layer = -1; half_t* out_hidden = nullptr; float* out_embeds = nullptr;
    // device buffers
    half_t *cls = nullptr, *pos = nullptr, *wpatch = nullptr, *wproj = nullptr;
    half_t *rows = nullptr, *patch = nullptr, *x = nullptr, *h = nullptr, *qkv = nullptr, *att = nullptr, *ff = nullptr;
    half_t *cls_x = nullptr, *cls_h = nullptr;
    float* pool_in = nullptr;
};

namespace {

constexpr int MAX_TOKENS = 320;
constexpr int KT = 32;              // keys per tile
constexpr int VT_LD = KT + 8;       // halfs per V^T row in LDS: 80 bytes, so the 16-byte reads of 8 consecutive rows spread over the banks

int g_last[3] = {0, 0, 0};          // cfgpp_vit_attention_last_launch

struct VitAttnArgs {
    const half_t* qkv;
    half_t* o;
    int heads, T, qblocks;
    float scale_log2e;              // D^-1/2 * log2(e)
};

template <int D>
__global__ void __launch_bounds__(64)
vit_attn_kernel(const VitAttnArgs a) {
    constexpr int DK = (D + 15) / 16, DT = (D + 31) / 32, DCH = D / 8, NV = (KT * DCH + 63) / 64;
    __shared__ __attribute__((aligned(16))) half_t vt[32 * DT * VT_LD];
    const int lane = threadIdx.x, j = lane & 31, hi = lane >> 5;
    const int qb = blockIdx.x % a.qblocks, rh = blockIdx.x / a.qblocks;
    const int r = rh / a.heads, h = rh - r * a.heads;
    const long hidden = (long)a.heads * D, ld = 3 * hidden;
    const int T = a.T;
    const int ntiles = (T + KT - 1) / KT;
    const half8_t z8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const half_t* base = a.qkv + (long)r * T * ld + h * D;       // Q of token 0; K sits `hidden` columns further, V 2 * hidden

    for (int i = lane; i < 32 * DT * VT_LD / 8; i += 64) *reinterpret_cast<half8_t*>(&vt[8 * i]) = z8;

    half8_t qf[DK];
    {
        const int q = qb * 32 + j;
        const half_t* qp = base + (long)q * ld + 8 * hi;
#pragma unroll
        for (int ks = 0; ks < DK; ++ks) qf[ks] = (q < T && 16 * ks + 8 * hi < D) ? *reinterpret_cast<const half8_t*>(qp + 16 * ks) : z8;
    }

    half8_t kf[DK], vr[NV];
    auto load_tile = [&](int t0) {
        const int key = t0 + j;
        const half_t* kp = base + (long)key * ld + hidden + 8 * hi;
#pragma unroll
        for (int ks = 0; ks < DK; ++ks) kf[ks] = (key < T && 16 * ks + 8 * hi < D) ? *reinterpret_cast<const half8_t*>(kp + 16 * ks) : z8;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;                    // chunk c: key c / DCH of the tile, dims 8 (c % DCH) .. + 7
            const int kk = t0 + c / DCH;
            vr[i] = (c < KT * DCH && kk < T) ? *reinterpret_cast<const half8_t*>(base + (long)kk * ld + 2 * hidden + 8 * (c % DCH)) : z8;
        }
    };

    float m = -INFINITY, l = 0.f;
    f32x16 oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[dt][i] = 0.f;

    load_tile(0);
    for (int t = 0; t < ntiles; ++t) {
        const int t0 = t * KT;
        __syncthreads();                                    // the previous tile's V^T reads (first tile: the zero fill) are done
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < KT * DCH) {
                const int col = cfgpp_vt_pos(c / DCH), d0 = 8 * (c % DCH);
#pragma unroll
                for (int e = 0; e < 8; ++e) vt[(d0 + e) * VT_LD + col] = vr[i][e];
            }
        }
        half8_t kc[DK];
#pragma unroll
        for (int ks = 0; ks < DK; ++ks) kc[ks] = kf[ks];
        __syncthreads();
        if (t + 1 < ntiles) load_tile(t0 + KT);

        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < DK; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kc[ks], qf[ks], s, 0, 0, 0);

        float mt = -INFINITY;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = t0 + 8 * (i >> 2) + 4 * hi + (i & 3);
            s[i] = key < T ? s[i] * a.scale_log2e : -INFINITY;
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
        for (int dt = 0; dt < DT; ++dt) {
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
    const int q = qb * 32 + j;
    if (q >= T) return;
    const float inv = 1.0f / l;
    half_t* op = a.o + ((long)r * T + q) * hidden + h * D + 4 * hi;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (32 * dt + 8 * g + 4 * hi >= D) continue;   // D % 8 == 0: a group of 4 dims is stored whole or not at all
            half4_t o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (half_t)(oacc[dt][4 * g + e] * inv);
            *reinterpret_cast<half4_t*>(op + 32 * dt + 8 * g) = o;
        }
}

int vit_attn_launch(const half_t* qkv, half_t* o, int rows, int heads, int d, int T, hipStream_t s) {
    g_last[0] = g_last[1] = g_last[2] = 0;
    CFGPP_REQUIRE(qkv && o, "vit_attention: null operand");
    CFGPP_REQUIRE(d == 64 || d == 80 || d == 104, "vit_attention: head dim %d (64, 80 or 104)", d);
    CFGPP_REQUIRE(T >= 1 && T <= MAX_TOKENS, "vit_attention: T=%d (1 .. %d tokens)", T, MAX_TOKENS);
    CFGPP_REQUIRE(rows >= 1 && heads >= 1 && (long)rows * heads * ((T + 31) / 32) < (1L << 30), "vit_attention: rows=%d heads=%d", rows, heads);
    VitAttnArgs a;
    a.qkv = qkv; a.o = o; a.heads = heads; a.T = T; a.qblocks = (T + 31) / 32;
    a.scale_log2e = (float)(1.4426950408889634 / std::sqrt((double)d));
    const dim3 grid(rows * heads * a.qblocks);
    if (d == 64) hipLaunchKernelGGL(vit_attn_kernel<64>, grid, dim3(64), 0, s, a);
    else if (d == 80) hipLaunchKernelGGL(vit_attn_kernel<80>, grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL(vit_attn_kernel<104>, grid, dim3(64), 0, s, a);
    CFGPP_HIP_CHECK(hipGetLastError());
    g_last[0] = d; g_last[1] = a.qblocks; g_last[2] = (T + KT - 1) / KT;
    return 0;
}

// ---- image front end ----------------------------------------------------------------------------------------------------------
// torch's antialiased bicubic (upsample_bicubic2d_aa, a = -0.5), one axis: output index i of an axis resized from `in` to `out`
// samples reads input [xmin, xmin + xsize) with weights aa_weight(k) / sum_k aa_weight(k)
struct AaAxis { double center, invscale; int xmin, xsize; };

// Window and weights are evaluated in fp64 and each normalised weight is rounded to fp32 once: torch evaluates them in fp32, where
// the sample position scale * (i + 0.5) alone carries an error of ~1e-5 of a pixel at a few hundred pixels - more than the whole fp32
// accumulation the tests' bound is derived from (tests/test_vision_cpu.py measures torch at 1.2e-5 from the fp64 value).
__device__ __forceinline__ double aa_filter(double x) {
    x = fabs(x);
    if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1.0;
    if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    return 0.0;
}
__device__ __forceinline__ AaAxis aa_axis(int i, int in, int out) {
    const double scale = (double)in / (double)out;
    const double support = scale >= 1.0 ? 2.0 * scale : 2.0;
    AaAxis a;
    a.invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
    a.center = scale * ((double)i + 0.5);
    a.xmin = max((int)(a.center - support + 0.5), 0);
    a.xsize = min((int)(a.center + support + 0.5), in) - a.xmin;
    return a;
}
__device__ __forceinline__ double aa_weight(const AaAxis& a, int k) { return aa_filter(((double)(k + a.xmin) - a.center + 0.5) * a.invscale); }

struct PreArgs {
    const float* img; half_t* out;
    int N, H, W, S, nh, nw, top, left;
    float mean[3], istd[3];
};

__global__ void __launch_bounds__(256)
vit_preprocess_kernel(const PreArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)a.N * 3 * a.S * a.S;
    if (idx >= total) return;
    const int ox = (int)(idx % a.S), oy = (int)((idx / a.S) % a.S);
    const int c = (int)((idx / ((long)a.S * a.S)) % 3);
    const long n = idx / ((long)3 * a.S * a.S);
    const AaAxis ay = aa_axis(oy + a.top, a.H, a.nh), ax = aa_axis(ox + a.left, a.W, a.nw);
    double ty = 0.0, tx = 0.0;
    for (int k = 0; k < ay.xsize; ++k) ty += aa_weight(ay, k);
    for (int k = 0; k < ax.xsize; ++k) tx += aa_weight(ax, k);
    const double ity = 1.0 / ty, itx = 1.0 / tx;
    const float* plane = a.img + (n * 3 + c) * (long)a.H * a.W;
    float acc = 0.f;
    for (int yy = 0; yy < ay.xsize; ++yy) {
        const float* row = plane + (long)(ay.xmin + yy) * a.W + ax.xmin;
        float hsum = 0.f;                                   // the horizontal pass's fp32 value at (input row, output column)
        for (int xx = 0; xx < ax.xsize; ++xx) hsum += (float)(aa_weight(ax, xx) * itx) * row[xx];
        acc += (float)(aa_weight(ay, yy) * ity) * hsum;
    }
    acc = fminf(fmaxf(acc, 0.0f), 1.0f);
    a.out[idx] = (half_t)((acc - a.mean[c]) * a.istd[c]);
}

int vit_preprocess_launch(const float* img, int N, int H, int W, int S, half_t* out, hipStream_t s) {
    CFGPP_REQUIRE(img && out, "vision_preprocess: null operand");
    CFGPP_REQUIRE(N >= 1 && H >= 1 && W >= 1 && S >= 1 && (long)N * 3 * S * S < (1L << 31) && (long)N * 3 * H * W < (1L << 40),
                  "vision_preprocess: N=%d H=%d W=%d S=%d", N, H, W, S);
    PreArgs a;
    a.img = img; a.out = out; a.N = N; a.H = H; a.W = W; a.S = S;
    // short side to S: Python's `max(size, round(H * size / min(H, W)))` (round half to even, as nearbyint in the default mode)
    const double sc = (double)S / (double)std::min(H, W);
    a.nh = std::max(S, (int)std::nearbyint(H * sc)); a.nw = std::max(S, (int)std::nearbyint(W * sc));
    a.top = (a.nh - S) / 2; a.left = (a.nw - S) / 2;
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, sd[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    for (int c = 0; c < 3; ++c) { a.mean[c] = mean[c]; a.istd[c] = 1.0f / sd[c]; }
    hipLaunchKernelGGL(vit_preprocess_kernel, dim3(cdiv((long)N * 3 * S * S, 256)), dim3(256), 0, s, a);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

// rows[(n * G * G + py * G + px)][c * ps * ps + dy * ps + dx] = pix[n][c][ps * py + dy][ps * px + dx]; columns K .. Kp - 1 = 0
__global__ void __launch_bounds__(256)
vit_patch_rows_kernel(const half_t* __restrict__ pix, half_t* __restrict__ rows, long total, int S, int ps, int G, int K, int Kp) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int k = (int)(idx % Kp);
    const long rp = idx / Kp;
    half_t v = (half_t)0.f;
    if (k < K) {
        const int p = (int)(rp % (G * G)); const long n = rp / (G * G);
        const int py = p / G, px = p - py * G;
        const int c = k / (ps * ps), rem = k - c * ps * ps, dy = rem / ps, dx = rem - dy * ps;
        v = pix[((n * 3 + c) * S + py * ps + dy) * (long)S + px * ps + dx];
    }
    rows[idx] = v;
}

int vit_patch_rows_launch(const half_t* pix, half_t* rows, int N, int S, int ps, int Kp, hipStream_t s) {
    CFGPP_REQUIRE(pix && rows, "vision_patch_rows: null operand");
    CFGPP_REQUIRE(N >= 1 && ps >= 1 && S >= ps && S % ps == 0 && Kp >= 3 * ps * ps, "vision_patch_rows: N=%d S=%d patch=%d Kp=%d", N, S, ps, Kp);
    const int G = S / ps;
    const long total = (long)N * G * G * Kp;
    CFGPP_REQUIRE(total < (1L << 38), "vision_patch_rows: %ld elements", total);
    hipLaunchKernelGGL(vit_patch_rows_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, pix, rows, total, S, ps, G, 3 * ps * ps, Kp);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

// x[n][0] = class_embedding + pos[0]; x[n][1 + p] = patch[n][p] + pos[1 + p]      (fp32 sum of fp16 values, rounded once; H % 8 == 0)
__global__ void __launch_bounds__(128)
vit_assemble_kernel(const half_t* __restrict__ patch, const half_t* __restrict__ cls, const half_t* __restrict__ pos,
                    half_t* __restrict__ x, int H, int T) {
    const int row = blockIdx.x;                       // n * T + t
    const int t = row % T, n = row / T;
    const half_t* src = t == 0 ? cls : patch + ((long)n * (T - 1) + (t - 1)) * H;
    const half_t* pe = pos + (long)t * H;
    for (int c = threadIdx.x * 8; c < H; c += 128 * 8) {
        const half8_t u = *reinterpret_cast<const half8_t*>(src + c);
        const half8_t b = *reinterpret_cast<const half8_t*>(pe + c);
        half8_t o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (half_t)((float)u[k] + (float)b[k]);
        *reinterpret_cast<half8_t*>(x + (long)row * H + c) = o;
    }
}

int vit_assemble_launch(const half_t* patch, const half_t* cls, const half_t* pos, half_t* x, int N, int T, int H, hipStream_t s) {
    CFGPP_REQUIRE(patch && cls && pos && x, "vit_assemble: null operand");
    CFGPP_REQUIRE(N >= 1 && T >= 2 && (long)N * T < (1L << 31) && H >= 8 && H % 8 == 0,
                  "vit_assemble: N=%d T=%d H=%d (a class token and at least one patch; H a positive multiple of 8)", N, T, H);
    hipLaunchKernelGGL(vit_assemble_kernel, dim3(N * T), dim3(128), 0, s, patch, cls, pos, x, H, T);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

// the class-token rows: dst[n][:] = x[n][0][:]
__global__ void __launch_bounds__(128)
vit_cls_rows_kernel(const half_t* __restrict__ x, half_t* __restrict__ dst, int H, int T) {
    const int n = blockIdx.x;
    for (int c = threadIdx.x * 8; c < H; c += 128 * 8)
        *reinterpret_cast<half8_t*>(dst + (long)n * H + c) = *reinterpret_cast<const half8_t*>(x + (long)n * T * H + c);
}

int vit_cls_rows_launch(const half_t* x, half_t* dst, int N, int T, int H, hipStream_t s) {
    CFGPP_REQUIRE(x && dst, "vit_cls_rows: null operand");
    CFGPP_REQUIRE(N >= 1 && T >= 1 && H >= 8 && H % 8 == 0, "vit_cls_rows: N=%d T=%d H=%d (H a positive multiple of 8)", N, T, H);
    hipLaunchKernelGGL(vit_cls_rows_kernel, dim3(N), dim3(128), 0, s, x, dst, H, T);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

const char* VM = "vision_model.";

void vision_param_table(cfgpp_vision* t) {
    const long H = t->hidden, I = t->inter;
    const std::string vm = VM;
    expect(t, vm + "embeddings.class_embedding", {H}, true);
    expect(t, vm + "embeddings.patch_embedding.weight", {H, 3, t->ps, t->ps}, true);
    expect(t, vm + "embeddings.position_embedding.weight", {t->T, H}, true);
    expect_norm(t, vm + "pre_layrnorm", H);
    for (int l = 0; l < t->layers; ++l) {
        const std::string p = vm + "encoder.layers." + std::to_string(l);
        expect_norm(t, p + ".layer_norm1", H); expect_norm(t, p + ".layer_norm2", H);
        for (const char* n : {"q_proj", "k_proj", "v_proj", "out_proj"}) expect_linear(t, p + ".self_attn." + n, H, H, true);
        expect_linear(t, p + ".mlp.fc1", I, H, true);
        expect_linear(t, p + ".mlp.fc2", H, I, true);
    }
    expect_norm(t, vm + "post_layernorm", H);
    expect(t, "visual_projection.weight", {t->proj, H}, true);
}

}  // namespace

extern "C" {

void cfgpp_vit_attention_last_launch(int* out3) { if (out3) { out3[0] = g_last[0]; out3[1] = g_last[1]; out3[2] = g_last[2]; } }

int cfgpp_op_attention_vit(const void* qkv, void* o, int rows, int heads, int d, int T, void* stream) {
    return vit_attn_launch((const half_t*)qkv, (half_t*)o, rows, heads, d, T, (hipStream_t)stream);
}

int cfgpp_op_vit_preprocess(const float* img, int N, int H, int W, int S, void* pixels_out, void* stream) {
    return vit_preprocess_launch(img, N, H, W, S, (half_t*)pixels_out, (hipStream_t)stream);
}

int cfgpp_op_vit_patch_rows(const void* pixels, void* rows, int N, int S, int patch, int Kp, void* stream) {
    return vit_patch_rows_launch((const half_t*)pixels, (half_t*)rows, N, S, patch, Kp, (hipStream_t)stream);
}

int cfgpp_op_vit_assemble(const void* patch, const void* cls, const void* pos, void* x, int N, int T, int H, void* stream) {
    return vit_assemble_launch((const half_t*)patch, (const half_t*)cls, (const half_t*)pos, (half_t*)x, N, T, H, (hipStream_t)stream);
}

int cfgpp_op_vit_cls_rows(const void* x, void* dst, int N, int T, int H, void* stream) {
    return vit_cls_rows_launch((const half_t*)x, (half_t*)dst, N, T, H, (hipStream_t)stream);
}

cfgpp_vision* cfgpp_vision_create(int hidden, int layers, int heads, int intermediate, int act, int proj_dim, int image_size,
                                  int patch_size, int max_batch, int device_id) {
    if (hidden <= 0 || layers <= 0 || heads <= 0 || intermediate <= 0 || proj_dim <= 0 || image_size <= 0 || patch_size <= 0 || max_batch <= 0) {
        cfgpp_set_error("vision_create: non-positive geometry (hidden=%d layers=%d heads=%d intermediate=%d proj_dim=%d image=%d patch=%d "
                        "max_batch=%d)", hidden, layers, heads, intermediate, proj_dim, image_size, patch_size, max_batch);
        return nullptr;
    }
    const int d = hidden / heads;
    if (hidden != heads * d || (d != 64 && d != 80 && d != 104)) {
        cfgpp_set_error("vision_create: unsupported head dim: hidden=%d over heads=%d (hidden must be heads x 64, 80 or 104)", hidden, heads);
        return nullptr;
    }
    if (hidden % 64 != 0 || intermediate % 64 != 0) {
        cfgpp_set_error("vision_create: hidden=%d and intermediate=%d must be multiples of 64", hidden, intermediate);
        return nullptr;
    }
    if (image_size % patch_size != 0) {
        cfgpp_set_error("vision_create: image_size=%d is not a multiple of patch_size=%d", image_size, patch_size);
        return nullptr;
    }
    const int G = image_size / patch_size;
    if (1 + G * G > MAX_TOKENS) {
        cfgpp_set_error("vision_create: %d tokens (image_size=%d, patch_size=%d): towers beyond %d tokens are not supported", 1 + G * G,
                        image_size, patch_size, MAX_TOKENS);
        return nullptr;
    }
    if (act != 0 && act != 1) { cfgpp_set_error("vision_create: activation %d (0 quick_gelu | 1 gelu)", act); return nullptr; }
    if (proj_dim % 4 != 0) { cfgpp_set_error("vision_create: proj_dim=%d must be a multiple of 4", proj_dim); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id || device_id < 0 || hipSetDevice(device_id) != hipSuccess) {
        cfgpp_set_error("vision_create: no HIP device %d - the HIP path has no CPU fallback", device_id);
        return nullptr;
    }
    if (cfgpp_claim_device(device_id)) return nullptr;
    cfgpp_vision* t = new cfgpp_vision();
    t->hidden = hidden; t->layers = layers; t->heads = heads; t->d = d; t->inter = intermediate; t->act = act; t->proj = proj_dim;
    t->S = image_size; t->ps = patch_size; t->G = G; t->T = 1 + G * G; t->K = 3 * patch_size * patch_size; t->Kp = round_up(t->K, 64);
    t->max_rows = max_batch; t->device = device_id;
    vision_param_table(t);
    return t;
}

void cfgpp_vision_destroy(cfgpp_vision* t) { delete t; }

int cfgpp_vision_load_tensor(cfgpp_vision* t, const char* key, const void* host, int dtype, const long* shape, int ndim) {
    CFGPP_REQUIRE(t && key && host && shape && ndim >= 0 && !t->finalized, "vision_load_tensor: bad state/args");
    CFGPP_REQUIRE(dtype == 0 || dtype == 1, "vision_load_tensor: dtype %d (0 fp32 | 1 fp16)", dtype);
    std::string k = key;
    if (k.size() >= 12 && k.compare(k.size() - 12, 12, "position_ids") == 0) return 0;
    auto it = t->params.find(k);
    if (it == t->params.end()) it = t->params.find(std::string(VM) + k);      // a bare CLIPVisionTransformer's keys carry no prefix
    if (it == t->params.end()) { cfgpp_set_error("vision_load_tensor: unknown key %s", key); return -3; }
    HostParam& p = it->second;
    long n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i];
    CFGPP_REQUIRE(n == p.numel(), "vision_load_tensor: %s has %ld elements, expected %ld", key, n, p.numel());
    if (p.is_matrix) {
        p.h.resize(n);
        if (dtype == 0) { const float* s = (const float*)host; for (long i = 0; i < n; ++i) p.h[i] = (half_t)s[i]; }
        else std::memcpy(p.h.data(), host, n * sizeof(half_t));
    } else {
        p.f.resize(n);
        if (dtype == 0) std::memcpy(p.f.data(), host, n * sizeof(float));
        else { const half_t* s = (const half_t*)host; for (long i = 0; i < n; ++i) p.f[i] = (float)s[i]; }
    }
    p.loaded = true;
    return 0;
}

int cfgpp_vision_finalize(cfgpp_vision* t) {
    CFGPP_REQUIRE(t && !t->finalized, "vision_finalize: bad state");
    {
        int n = 0; std::string names;
        for (auto& kv : t->params) if (!kv.second.loaded) { if (n++ < 4) names += kv.first + " "; }
        CFGPP_REQUIRE(n == 0, "vision_finalize: %d parameters not loaded (%s...)", n, names.c_str());
    }
    const int H = t->hidden, I = t->inter, R = t->max_rows, T = t->T, PP = t->G * t->G, K = t->K, Kp = t->Kp;
    const std::string vm = VM;
    Builder B{t};
    Plan P{t, &B, &t->plan};
    {
        HostParam* c = B.get(vm + "embeddings.class_embedding");
        if (c) { t->cls = B.upload(c->h); B.drop(vm + "embeddings.class_embedding"); }
        HostParam* w = B.get(vm + "embeddings.patch_embedding.weight");
        if (w) {                                        // [H][3 * ps * ps] -> [H][Kp], columns K .. Kp - 1 zero
            std::vector<half_t> r((size_t)H * Kp, (half_t)0.f);
            for (long o = 0; o < H; ++o) std::memcpy(&r[(size_t)o * Kp], &w->h[(size_t)o * K], (size_t)K * sizeof(half_t));
            t->wpatch = B.upload(r); B.drop(vm + "embeddings.patch_embedding.weight");
        }
    }
    t->pos = B.linear(vm + "embeddings.position_embedding.weight");
    CFGPP_REQUIRE(B.ok, "vision_finalize: %s", B.err.c_str());
    const size_t rows = (size_t)R * T;
    t->rows = (half_t*)t->dmalloc((size_t)R * PP * Kp * sizeof(half_t));
    t->patch = (half_t*)t->dmalloc((size_t)R * PP * H * sizeof(half_t));
    t->x = (half_t*)t->dmalloc(rows * H * sizeof(half_t));
    t->h = (half_t*)t->dmalloc(rows * H * sizeof(half_t));
    t->qkv = (half_t*)t->dmalloc(rows * 3 * H * sizeof(half_t));
    t->att = (half_t*)t->dmalloc(rows * H * sizeof(half_t));
    t->ff = (half_t*)t->dmalloc(rows * I * sizeof(half_t));
    t->cls_x = (half_t*)t->dmalloc((size_t)R * H * sizeof(half_t));
    t->cls_h = (half_t*)t->dmalloc((size_t)R * H * sizeof(half_t));
    t->pool_in = (float*)t->dmalloc((size_t)R * H * sizeof(float));
    CFGPP_REQUIRE(t->rows && t->patch && t->x && t->h && t->qkv && t->att && t->ff && t->cls_x && t->cls_h && t->pool_in,
                  "vision_finalize: hipMalloc failed");
    cfgpp_vision* tt = t;
    // hidden_states[k] snapshot: the residual stream as it stands when layer k is about to run (k = 0: after pre_layrnorm, k = L: after the last layer)
    auto snapshot = [&](int k) {
        t->plan.push_back([tt, k, H, T](hipStream_t s, int r) {
            if (tt->out_layer != k || !tt->out_hidden) return 0;
            CFGPP_HIP_CHECK(hipMemcpyAsync(tt->out_hidden, tt->x, (size_t)r * T * H * sizeof(half_t), hipMemcpyDeviceToDevice, s));
            return 0;
        });
    };
    t->plan.push_back([tt](hipStream_t s, int r) { return vit_patch_rows_launch(tt->in_pixels, tt->rows, r, tt->S, tt->ps, tt->Kp, s); });
    P.linear(t->rows, Kp, t->patch, H, t->wpatch, nullptr, nullptr, PP);
    t->plan.push_back([tt, H, T](hipStream_t s, int r) { return vit_assemble_launch(tt->patch, tt->cls, tt->pos, tt->h, r, T, H, s); });
    {
        const float* g = B.f32(vm + "pre_layrnorm.weight"); const float* b = B.f32(vm + "pre_layrnorm.bias");
        P.layernorm(t->h, t->x, g, b, T, H);
    }
    for (int l = 0; l < t->layers && B.ok; ++l) {
        const std::string p = vm + "encoder.layers." + std::to_string(l);
        snapshot(l);
        const float* g1 = B.f32(p + ".layer_norm1.weight"); const float* b1 = B.f32(p + ".layer_norm1.bias");
        const float* g2 = B.f32(p + ".layer_norm2.weight"); const float* b2 = B.f32(p + ".layer_norm2.bias");
        std::vector<float> bq;
        for (const char* n : {"q_proj", "k_proj", "v_proj"}) {
            HostParam* hp = B.get(p + ".self_attn." + n + ".bias");
            if (hp) bq.insert(bq.end(), hp->f.begin(), hp->f.end());
        }
        const float* bqkv = B.upload(bq);
        const half_t* wqkv = B.concat({p + ".self_attn.q_proj.weight", p + ".self_attn.k_proj.weight", p + ".self_attn.v_proj.weight"});
        const half_t* wo = B.linear(p + ".self_attn.out_proj.weight"); const float* bo = B.f32(p + ".self_attn.out_proj.bias");
        const half_t* w1 = B.linear(p + ".mlp.fc1.weight"); const float* bf1 = B.f32(p + ".mlp.fc1.bias");
        const half_t* w2 = B.linear(p + ".mlp.fc2.weight"); const float* bf2 = B.f32(p + ".mlp.fc2.bias");
        if (!B.ok) break;
        P.layernorm(t->x, t->h, g1, b1, T, H);
        P.linear(t->h, H, t->qkv, 3 * H, wqkv, bqkv, nullptr, T);
        t->attn_macs_per_row += 2.0 * (double)t->heads * T * T * t->d;
        t->plan.push_back([tt, T](hipStream_t s, int r) { return vit_attn_launch(tt->qkv, tt->att, r, tt->heads, tt->d, T, s); });
        t->tag(1, 2.0 * (double)t->heads * T * T * t->d, "vit_attn heads=" + std::to_string(t->heads) + " T=" + std::to_string(T) + " d=" + std::to_string(t->d));
        P.linear(t->att, H, t->x, H, wo, bo, t->x, T);                  // x += out_proj(att)   (residual in place)
        P.layernorm(t->x, t->h, g2, b2, T, H);
        P.linear(t->h, H, t->ff, I, w1, bf1, nullptr, T);
        t->plan.push_back([tt, I, T](hipStream_t s, int r) { return act_inplace_launch(tt->ff, (long)r * T * I, tt->act, s); });
        P.linear(t->ff, I, t->x, H, w2, bf2, t->x, T);                   // x += fc2(act(fc1(ln2(x))))
    }
    CFGPP_REQUIRE(B.ok, "vision_finalize: %s", B.err.c_str());
    snapshot(t->layers);
    {
        // image_embeds = visual_projection(post_layernorm(x[:, 0])): the class-token rows only
        const float* gf = B.f32(vm + "post_layernorm.weight"); const float* bf = B.f32(vm + "post_layernorm.bias");
        t->wproj = B.linear("visual_projection.weight");
        t->macs_per_row += (double)H * t->proj;
        t->plan.push_back([tt, gf, bf, H, T](hipStream_t s, int r) {
            if (!tt->out_embeds) return 0;
            int e = vit_cls_rows_launch(tt->x, tt->cls_x, r, T, H, s);
            if (e) return e;
            e = cfgpp_op_layernorm(tt->cls_x, tt->cls_h, gf, bf, r, H, 1e-5f, s);
            if (e) return e;
            e = cfgpp_op_f16_to_f32_rows(tt->cls_h, tt->pool_in, r, H, H, 0, s);
            if (e) return e;
            return cfgpp_op_skinny_gemm(tt->pool_in, H, tt->wproj, nullptr, nullptr, 0, tt->out_embeds, tt->proj, r, tt->proj, H, 0, 0, s);
        });
    }
    CFGPP_REQUIRE(B.ok, "vision_finalize: %s", B.err.c_str());
    CFGPP_HIP_CHECK(hipDeviceSynchronize());
    t->plan_kind.resize(t->plan.size(), 3); t->plan_macs.resize(t->plan.size(), 0.0); t->plan_desc.resize(t->plan.size());
    t->finalized = true;
    return 0;
}

int cfgpp_vision_preprocess(cfgpp_vision* t, const float* img, int N, int H, int W, void* pixels_out, void* stream) {
    CFGPP_REQUIRE(t && img && pixels_out, "vision_preprocess: null engine / operand");
    CFGPP_REQUIRE(N >= 1 && H >= 1 && W >= 1, "vision_preprocess: N=%d H=%d W=%d (all >= 1)", N, H, W);
    return vit_preprocess_launch(img, N, H, W, t->S, (half_t*)pixels_out, (hipStream_t)stream);
}

int cfgpp_vision_encode(cfgpp_vision* t, const void* pixels, int N, int layer, void* hidden_out, float* embeds_out, void* stream) {
    CFGPP_REQUIRE(t && t->finalized && pixels, "vision_encode: engine not finalized or null pixels");
    CFGPP_REQUIRE(N > 0 && N <= t->max_rows, "vision_encode: N=%d images (1 .. max_batch=%d)", N, t->max_rows);
    CFGPP_REQUIRE(layer >= -1 && layer <= t->layers, "vision_encode: layer %d outside [-1, %d]", layer, t->layers);
    CFGPP_REQUIRE(layer < 0 || hidden_out, "vision_encode: layer %d asks for hidden states, hidden_out is NULL", layer);
    CFGPP_REQUIRE(hidden_out || embeds_out, "vision_encode: no output requested");
    hipStream_t s = (hipStream_t)stream;
    t->in_pixels = (const half_t*)pixels;
    t->out_layer = layer; t->out_hidden = layer >= 0 ? (half_t*)hidden_out : nullptr; t->out_embeds = embeds_out;
    for (auto& op : t->plan) { int e = op(s, N); if (e) return e; }
    return 0;
}

double cfgpp_vision_flops(cfgpp_vision* t, int N) { return t ? 2.0 * (t->macs_per_row + t->attn_macs_per_row) * N : 0.0; }
double cfgpp_vision_device_bytes(cfgpp_vision* t) { return t ? t->dev_bytes : 0.0; }

}  // extern "C"
