// K6/K7: fused (flash-style) attention for the SD / SDXL UNet on gfx950.
//
//   O[b, q, h*d + :] = softmax(Q K^T * scale) V      Q,K: [B*heads][tok_pad][dp]   V^T: [B*heads][dp][tok_pad]
//
// Layout contract (written by the QKV GEMM epilogue, EPI_HEADS): head-major, head
// dim zero-padded to dp = round_up(d, 32), V stored TRANSPOSED with the keys of every
// 32-key block PERMUTED (bits 2 and 3 of the key index swapped: cfgpp_vt_pos in common.h) so
// that every MFMA operand is ONE contiguous 16-byte LDS read and no cross-lane shuffles are needed
// (the 8 k-slots a lane feeds to a PV MFMA are its accumulator registers 8*tt .. 8*tt+7 = keys
// 16*tt + 8*b + 4*hi + r, which the permutation makes consecutive):
//   * S^T = K Q^T with v_mfma_f32_32x32x16_f16 (A = K rows = keys, B = Q^T cols =
//     queries): each lane ends up holding 16 scores of ONE query per 32-key tile.
//   * Online softmax entirely in registers (one __shfl_xor(…,32) for the row max); Q is pre-scaled by
//     d^-1/2*log2(e) so scores feed v_exp_f32 directly; the O rescale is skipped (exactly) on tiles
//     where no query's running max grows; key masking only on a partial last tile.
//   * The loop is VALU-bound, not MFMA-bound, at small d (150 VALU vs 14 MFMA per 64-key tile at d = 40), so
//     two thirds of the softmax VALU is moved into the MFMAs: (i) the accumulator of S^T is INITIALISED with
//     -m (a persistent 16-register vector, rewritten only when a running max grows), so scores come out as
//     s - m and feed v_exp_f32 without a subtract; (ii) when d is not a multiple of 32 the first padding row
//     of V^T holds ONES (written once at engine build, cfgpp_op_attention_prepare_vt), so row d of O^T
//     accumulates sum_k P[k][q] - the softmax denominator - inside the PV MFMAs (no v_add chain, and the
//     denominator sums exactly the fp16 P values the numerator uses).
//   * O^T += V^T P^T: the B operand (P^T) is exactly the lane's own 8 consecutive
//     accumulator registers converted to fp16 (the MFMA k-slot <-> key assignment is
//     free as long as A and B agree), the A operand is one ds_read_b128 from the permuted V^T.
//   * 4 waves x 32 queries per workgroup, 64-key tiles.
//   * dp = 64 (d = 40: SD1.5 64x64 level, d = 64: every SDXL level - > 90 % of the attention time):
//     attn64_kernel.  K and V^T tiles are both [64 rows][128 B]; they go HBM -> LDS by LDS-DMA
//     (global_load_lds_dwordx4: no VGPR staging, no ds_write pass - the VGPR -> LDS store path was what
//     saturated the CU's LDS pipe: PMC showed 33 % of the LDS cycles as bank conflicts of the old 2 x
//     ds_read_b64 V reads and 47 % of the wave time parked) into unpadded rows with the igemm's XOR swizzle
//     applied to the per-lane SOURCE chunk, on a 2-stage ring (32 KB: FOUR workgroups per CU since round 4; rounds 2-3: 3 stages, three), one
//     raw s_barrier per tile, counted vmcnt.
//   * other head dims (80, 160): attn_kernel, register-staged double buffering, padded LDS rows.
// At most 128 keys with dp = 64 (the 77 text tokens of cross-attention) take xattn64_kernel below: K / V^T resident, one pass.
// softmax statistics and accumulation are fp32; P is rounded to fp16 for the PV
// product (same as the reference's SDPA flash path under fp16 autocast).
#include "common.h"

namespace {

// Deferred re-referencing of the online softmax: the scores leave the MFMA as s - m_ref (log2 domain); as long as no
// query of the wave exceeds m_ref by more than RESCALE_THR the reference stays and P = 2^(s - m_ref) <= 2^THR = 32
// (exact in fp16 / fp32: a floating-point scale; O and the denominator carry the same factor and it cancels in O / l).
// On random data a NEW running max appears in ~2/3 of the tiles of a 32-query wave, but it beats the old one by < 2;
// re-referencing only on a jump > 5 removes ~50 VALU instructions from 2/3 of the tiles.  The rare branch is covered
// by tests/test_gpu_configs.py::test_attention_online_softmax_rescale_branch (a key that jumps by ~100) and, for every
// kernel that has the branch, by the planted late keys of tests/test_gpu_attention.py.
constexpr float RESCALE_THR = 5.0f;

struct AttnArgs {
    const half_t* q; const half_t* k; const half_t* vt;
    half_t* o;
    int heads, d;         // real head dim
    int nq, nk_valid;     // real query / key counts
    int q_tok_pad, k_tok_pad;
    int o_ld;             // heads*d
    int nqb;              // query blocks (of 128 queries) per batch*head; grid = nqb * B * heads workgroups
    float scale_log2e;    // d^-0.5 * log2(e)
    int stagger;          // > 0: the co-resident workgroups of a CU start phase-shifted by this many 64-cycle sleeps (A/B knob)
};

// Workgroup -> (query block, batch*head).  Workgroup b runs on XCD b % 8 (observed dispatch order; speed only, never
// correctness), and every XCD has its own 4 MiB L2.  All query blocks of one (batch, head) read the same K / V^T
// (1 MB at N = 4096): with the natural order they are spread over all 8 XCDs and every L2 has to hold the K / V^T
// of EVERY head in flight (24 heads x 1 MB >> 4 MiB), so K / V^T tiles keep coming from HBM / Infinity Cache
// (~4 GB of fabric traffic per launch instead of 128 MB).  The remap hands each XCD a contiguous range of
// (batch*head, query block) pairs: the ~3 heads an XCD works on at a time stay L2-resident.
__device__ __forceinline__ void attn_block_map(int nqb, int& qb, int& bh) {
    const int T = gridDim.x, bid = blockIdx.x;
    const int q = T >> 3, r = T & 7, xcd = bid & 7, idx = bid >> 3;
    const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    bh = w / nqb; qb = w - bh * nqb;
}

template <int D16, int DT, bool ONES, int QT>
__global__ void __launch_bounds__(256)
attn_kernel(const AttnArgs a) {
    constexpr int DP = DT * 32;                  // padded head dim (row pitch of Q/K, rows of V^T)
    constexpr int KPITCH = DP * 2 + 16;          // bytes per K row in LDS
    constexpr int VPITCH = 64 * 2 + 16;          // bytes per V^T row in LDS (64 keys)
    constexpr int CH = (64 * DP / 8) / 256;      // 16-B chunks per thread per tile (K and V each)
    constexpr int STAGE = 64 * KPITCH + DP * VPITCH;
    static_assert((64 * DP / 8) % 256 == 0, "tile/loader mismatch");
    extern __shared__ __attribute__((aligned(16))) char smem[];     // 2 stages of (K tile | V^T tile)

    // QT query sub-tiles of 32 per wave: every K / V^T fragment read from LDS feeds QT MFMAs.  Measured with
    // QT = 2 (240-256 VGPRs, 2 waves/SIMD): +2 % at d = 40, -11 % at d = 64 (N = 4096), so QT = 1 ships.
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    int qb, bh;
    attn_block_map(a.nqb, qb, bh);
    const int q0 = qb * (128 * QT) + wid * (32 * QT);
    const half_t* Qb = a.q + (long)bh * a.q_tok_pad * DP;
    const half_t* Kb = a.k + (long)bh * a.k_tok_pad * DP;
    const half_t* Vb = a.vt + (long)bh * DP * a.k_tok_pad;

    // Q^T fragments (B operand): lane = query q0+qt*32+l31, 8 consecutive d at ks*16 + hi*8, pre-multiplied by
    // d^-1/2 * log2(e) so that the scores come out of the MFMA ready for exp2.
    half8_t qf[QT][D16];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int ks = 0; ks < D16; ++ks) {
            const half8_t raw = *reinterpret_cast<const half8_t*>(Qb + (long)(q0 + qt * 32 + l31) * DP + ks * 16 + hi * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[qt][ks][j] = (half_t)((float)raw[j] * a.scale_log2e);
        }

    f32x16 oacc[QT][DT];
    // negm = -m_ref broadcast over the 16 accumulator registers (C operand of the first S^T MFMA);
    // m_ref = 0 until the first tile (which always takes the "max grew" path) sets it.
    f32x16 negm[QT];
    float l_run[QT];                 // only used when !ONES
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        l_run[qt] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[qt][r] = 0.f;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[qt][i][r] = 0.f;
    }

    const int ntiles = (a.nk_valid + 63) >> 6;
    const int tail = a.nk_valid & 63;            // != 0: the last tile is partially masked

    half8_t rk[CH], rv[CH];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int c = tid + j * 256;
            const int kr = c / (DP / 8), kc = c - kr * (DP / 8);
            rk[j] = *reinterpret_cast<const half8_t*>(Kb + (long)(t * 64 + kr) * DP + kc * 8);
            const int vr = c >> 3, vc = c & 7;
            rv[j] = *reinterpret_cast<const half8_t*>(Vb + (long)vr * a.k_tok_pad + t * 64 + vc * 8);
        }
    };
    auto store_tile = [&](int stage) {
        char* Ks = smem + stage * STAGE;
        char* Vs = Ks + 64 * KPITCH;
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int c = tid + j * 256;
            const int kr = c / (DP / 8), kc = c - kr * (DP / 8);
            *reinterpret_cast<half8_t*>(Ks + kr * KPITCH + kc * 16) = rk[j];
            const int vr = c >> 3, vc = c & 7;
            *reinterpret_cast<half8_t*>(Vs + vr * VPITCH + vc * 16) = rv[j];
        }
    };

    load_tile(0);
    store_tile(0);
    __syncthreads();
    if (ntiles > 1) load_tile(1);
    for (int t = 0; t < ntiles; ++t) {
        const char* Ks = smem + (t & 1) * STAGE;
        const char* Vs = Ks + 64 * KPITCH;

        // ---- S^T - m = K Q^T + (-m) for two 32-key sub-tiles (log2 domain) ----
        f32x16 s[QT][2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int ks = 0; ks < D16; ++ks) {
                const half8_t kf = *reinterpret_cast<const half8_t*>(Ks + (kt * 32 + l31) * KPITCH + (ks * 16 + hi * 8) * 2);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
                    s[qt][kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[qt][ks], ks == 0 ? negm[qt] : s[qt][kt], 0, 0, 0);
            }
        }
        if (tail != 0 && t == ntiles - 1) {      // wave-uniform: mask keys >= nk_valid of a partial last tile (nk % 64 != 0)
            const int kbase = t * 64 + 4 * hi;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = kbase + kt * 32 + (r & 3) + 8 * (r >> 2);
                        s[qt][kt][r] = key < a.nk_valid ? s[qt][kt][r] : -INFINITY;
                    }
        }
        // ---- online softmax: per query = per lane column; keys across 32 registers and the two half-waves ----
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            float mx = s[qt][0][0];                  // tile max RELATIVE to m_ref
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[qt][kt][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            if (t == 0 || !__all(mx <= RESCALE_THR)) {   // (rare after the first tile) re-reference: exact
                const float delta = t == 0 ? mx : fmaxf(mx, 0.f);
                const float alpha = __builtin_amdgcn_exp2f(-delta);         // O = 0 on the first tile: alpha irrelevant
                l_run[qt] *= alpha;
#pragma unroll
                for (int i = 0; i < DT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[qt][i][r] *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) negm[qt][r] -= delta;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[qt][kt][r] -= delta;
            }
            float psum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(s[qt][kt][r]);
                    s[qt][kt][r] = pv;
                    if constexpr (!ONES) psum += pv;
                }
            if constexpr (!ONES) l_run[qt] += psum;
        }

        // ---- O^T += V^T P^T ----
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                half8_t pf[QT];
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[qt][j] = (half_t)s[qt][kt][8 * tt + j];
                // k-slot j = b*4 + r  <->  key = kt*32 + 8*(2*tt + b) + 4*hi + r  <->  V^T column kt*32 + 16*tt + 8*hi + j
                const int kpos0 = kt * 32 + 16 * tt + 8 * hi;
#pragma unroll
                for (int i = 0; i < DT; ++i) {
                    const half8_t vf = *reinterpret_cast<const half8_t*>(Vs + (i * 32 + l31) * VPITCH + kpos0 * 2);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt)
                        oacc[qt][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[qt], oacc[qt][i], 0, 0, 0);
                }
            }
        // ---- stage tile t+1 (registers -> the other LDS stage), prefetch tile t+2 ----
        if (t + 1 < ntiles) store_tile((t + 1) & 1);
        __syncthreads();
        if (t + 2 < ntiles) load_tile(t + 2);
    }

    // ---- finalize: O = O^T / l, store token-major ----
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        float l_tot;
        if constexpr (ONES) {
            // row d of O^T (the ones row of V^T) = sum_k P[k][q]: register (d%32 / 8) * 4 of tile d/32, half-wave 0
            const int dr = a.d & 31;                                   // multiple of 8 by contract
            float lv = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) if (dr == 8 * g) lv = oacc[qt][DT - 1][4 * g];
            l_tot = __shfl(lv, l31);
        } else {
            l_tot = l_run[qt] + __shfl_xor(l_run[qt], 32);
        }
        const float inv_l = 1.0f / l_tot;
        const int q = q0 + qt * 32 + l31;
        if (q < a.nq) {
            const int b = bh / a.heads, head = bh - b * a.heads;
            half_t* orow = a.o + ((long)b * a.nq + q) * a.o_ld + head * a.d;
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int dd = i * 32 + 8 * g + 4 * hi;
                    if (dd < a.d) {
                        half4_t o;
#pragma unroll
                        for (int k = 0; k < 4; ++k) o[k] = (half_t)(oacc[qt][i][4 * g + k] * inv_l);
                        *reinterpret_cast<half4_t*>(orow + dd) = o;
                    }
                }
        }
    }
}

// ---- dp = 64 ------------------------------------------------------------------------------------
// K tile  : LDS [64 keys  ][64 halfs], row = key,   16-B chunk c = 8 head dims
// V^T tile: LDS [64 d-rows][64 keys ], row = d,     16-B chunk c = 8 (permuted) keys
// physical chunk = logical chunk ^ ((row >> 1) & 7); one DMA piece = 8 rows x 128 B = 64 lanes x 16 B.
template <int D16, bool ONES, int NST, int WPE = 3>        // NST = LDS ring stages (shipped: 2 = 32 KB); WPE = waves per SIMD the
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))      // register allocation targets (4: <= 128 VGPRs, with NST = 2 four workgroups / CU)
attn64_kernel(const AttnArgs a) {
    constexpr int DP = 64, DT = 2;
    constexpr int TILE = 64 * 128;               // bytes of one K or V^T tile
    constexpr int STAGE = 2 * TILE;
    constexpr int PPW = 4;                       // DMA pieces per wave per tile: 8 (K) + 8 (V^T) over 4 waves
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    int qb, bh;
    attn_block_map(a.nqb, qb, bh);
    const int q0 = qb * 128 + wid * 32;
    const half_t* Qb = a.q + (long)bh * a.q_tok_pad * DP;
    const half_t* Kb = a.k + (long)bh * a.k_tok_pad * DP;
    const half_t* Vb = a.vt + (long)bh * DP * a.k_tok_pad;

    // DMA source addressing: lane -> (row r8 = lane >> 3 of the piece, physical chunk pc = lane & 7); the wave's
    // pieces are K rows [16 * wid, 16 * wid + 16) and V^T rows [16 * wid, 16 * wid + 16) of the tile
    const int r8 = lane >> 3, pc = lane & 7;
    // (32-bit element offsets from the wave-uniform bases Kb / Vb: half the registers of per-lane 64-bit pointers, and the loads can
    // take the scalar-base + vector-offset form)
    int koff[2], voff[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int row = wid * 16 + h * 8 + r8;
        const int lc = pc ^ ((row >> 1) & 7);
        koff[h] = row * DP + lc * 8;                               // + t * 64 * DP per tile
        voff[h] = row * a.k_tok_pad + lc * 8;                      // + t * 64 per tile
    }
    auto dma_tile = [&](int t, int stage) {
        char* Ks = smem + stage * STAGE;
        char* Vs = Ks + TILE;
        const half_t* Kt = Kb + (long)t * 64 * DP;                 // (wave-uniform)
        const half_t* Vt = Vb + (long)t * 64;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Kt + koff[h]),
                                             (__attribute__((address_space(3))) void*)(Ks + (wid * 16 + h * 8) * 128), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Vt + voff[h]),
                                             (__attribute__((address_space(3))) void*)(Vs + (wid * 16 + h * 8) * 128), 16, 0, 0);
        }
    };

    const int ntiles = (a.nk_valid + 63) >> 6;
    const int tail = a.nk_valid & 63;
    if (a.stagger > 0) {
        // Workgroups that share a CU run the same code from the same instant: their QK^T / softmax / PV phases coincide
        // and the matrix and vector pipes take turns instead of overlapping (PMC: both busy 19 % of the time).  Dispatch
        // slot s of a CU (observed order: block b -> XCD b % 8, then one block per CU, then the second slot ...) starts s
        // thirds of a tile late; blocks that start later inherit the offset of the block whose slot they take.
        const int slot = ((blockIdx.x >> 3) >> 5) % 3;
        for (int i = 0; i < slot * a.stagger; ++i) __builtin_amdgcn_s_sleep(1);
    }
#pragma unroll
    for (int t = 0; t < NST - 1; ++t) if (t < ntiles) dma_tile(t, t);

    // Q^T fragments (B operand), pre-multiplied by d^-1/2 * log2(e); ordinary loads, issued after the first DMAs
    half8_t qf[D16];
#pragma unroll
    for (int ks = 0; ks < D16; ++ks) {
        const half8_t raw = *reinterpret_cast<const half8_t*>(Qb + (long)(q0 + l31) * DP + ks * 16 + hi * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[ks][j] = (half_t)((float)raw[j] * a.scale_log2e);
    }

    f32x16 oacc[DT];
    f32x16 negm;
    float l_run = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) negm[r] = 0.f;
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;

    const int fsw = (l31 >> 1) & 7;
    const int frow = l31 * 128;
    for (int t = 0; t < ntiles; ++t) {
        // tile t landed once at most the NST-2 younger tiles' pieces are outstanding; the barrier makes every wave's pieces
        // visible and tells that everyone is done reading tile t-1, whose stage tile t+NST-1 is about to overwrite
        if (NST > 2 && t + 1 < ntiles) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((NST - 2) * PPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");           // (the barrier intrinsic alone does not order the LDS reads below)
        if (t + NST - 1 < ntiles) dma_tile(t + NST - 1, (t + NST - 1) % NST);
        const char* Ks = smem + (t % NST) * STAGE;
        const char* Vs = Ks + TILE;

        // ---- S^T - m = K Q^T + (-m) for two 32-key sub-tiles (log2 domain) ----
        f32x16 s[2];
        {
            // register-lean form (<= 128 VGPRs: four waves per SIMD): one 32-key sub-tile's K fragments at a time; the other waves of
            // the SIMD cover the LDS latency
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
                for (int k0 = 0; k0 < D16; k0 += 2) {    // two fragments (8 registers) in flight at a time
                    half8_t kf1[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        if (k0 + u < D16) kf1[u] = *reinterpret_cast<const half8_t*>(Ks + kt * 32 * 128 + frow + (((((k0 + u) << 1) | hi) ^ fsw) << 4));
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        if (k0 + u < D16) s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf1[u], qf[k0 + u], k0 + u == 0 ? negm : s[kt], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);   // later fragments are not hoisted above these MFMAs (registers)
                }
            }
        }
        // wave-uniform: mask keys >= nk_valid of a partial last tile.  With the default switches this kernel sees nk > 128 only
        // (<= 128 keys, the 77 text tokens included, go to xattn64_kernel), so the mask runs when nk % 64 != 0: 144 tokens of a
        // 12 x 12 map, or any shape under cfgpp_attention_set_cross(0)
        if (tail != 0 && t == ntiles - 1) {
            const int kbase = t * 64 + 4 * hi;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kbase + kt * 32 + (r & 3) + 8 * (r >> 2);
                    s[kt][r] = key < a.nk_valid ? s[kt][r] : -INFINITY;
                }
        }
        // ---- online softmax: per query = per lane column; keys across 32 registers and the two half-waves ----
        float mx = s[0][0];                      // tile max RELATIVE to m_ref
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kt][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        if (t == 0 || !__all(mx <= RESCALE_THR)) {   // (rare after the first tile) re-reference: exact
            const float delta = t == 0 ? mx : fmaxf(mx, 0.f);
            const float alpha = __builtin_amdgcn_exp2f(-delta);
            l_run *= alpha;
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
#pragma unroll
            for (int r = 0; r < 16; ++r) negm[r] -= delta;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kt][r] -= delta;
        }
        float psum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(s[kt][r]);
                s[kt][r] = pv;
                if constexpr (!ONES) psum += pv;
            }
        if constexpr (!ONES) l_run += psum;

        // ---- O^T += V^T P^T ----
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                half8_t pf;
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[j] = (half_t)s[kt][8 * tt + j];
                const int lc = kt * 4 + 2 * tt + hi;               // logical 16-B chunk of the (permuted) key axis
#pragma unroll
                for (int i = 0; i < DT; ++i) {
                    const half8_t vf = *reinterpret_cast<const half8_t*>(Vs + i * 32 * 128 + frow + ((lc ^ fsw) << 4));
                    oacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[i], 0, 0, 0);
                }
            }
    }

    // ---- finalize: O = O^T / l, store token-major ----
    // (lane-derived indices are re-derived here from an opaque copy of the lane id: kept live across the key loop they are what
    //  the register-lean instantiations spilled)
    int lane_f = threadIdx.x & 63;
    asm volatile("" : "+v"(lane_f));
    const int l31_f = lane_f & 31, hi_f = lane_f >> 5;
    float l_tot;
    if constexpr (ONES) {
        const int dr = a.d & 31;
        float lv = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) if (dr == 8 * g) lv = oacc[DT - 1][4 * g];
        l_tot = __shfl(lv, l31_f);
    } else {
        l_tot = l_run + __shfl_xor(l_run, 32);
    }
    const float inv_l = 1.0f / l_tot;
    const int q = qb * 128 + wid * 32 + l31_f;
    if (q < a.nq) {
        const int b = bh / a.heads, head = bh - b * a.heads;
        half_t* orow = a.o + ((long)b * a.nq + q) * a.o_ld + head * a.d;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int dd = i * 32 + 8 * g + 4 * hi_f;
                if (dd < a.d) {
                    half4_t o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = (half_t)(oacc[i][4 * g + k] * inv_l);
                    *reinterpret_cast<half4_t*>(orow + dd) = o;
                }
            }
    }
}

// ---- cross-attention, dp = 64, <= 128 keys (the 77 text tokens) ----------------------------------------------------------
// With 77 keys the flash loop above is two tiles of latency per 128 queries: every workgroup loads its own copy of K / V^T
// (32 KB) for 16 KB of Q and 16 KB of O, waits for it twice and runs the online-softmax bookkeeping for nothing
// (100-160 TF/s in the per-launch tables of rounds 1-2).  Here a workgroup loads the head's K and V^T ONCE (both 64-key tiles, by
// LDS-DMA, the layouts of attn64_kernel) and then walks XQB blocks of 128 queries with no barrier and no running maximum: all
// 96 scores of a query (three 32-key sub-tiles; keys >= nk_valid masked) are in registers, softmax is a single pass, and the
// kernel is what it should be - a stream of Q in and O out.
//
// IP = true: decoupled cross-attention (IP-Adapter; diffusers IPAdapterAttnProcessor2_0).  Keys [0, nk_valid) with nk_valid <= 96
// are the text (sub-tiles 0 - 2), keys [96, 96 + n_img) the image tokens (sub-tile 3): the same resident K / V^T, the same walk,
// and after the text pass a SECOND complete softmax over sub-tile 3 - its own mask, maximum, fp16-rounded P, accumulators (the
// registers of the text scores, dead by then) and denominator (the sum of its own rounded P, or the ones row of V^T met by its
// own P; in this form the text group's denominator is summed from the rounded P as well, in the text-only form from the fp32 P) -
//     o = fp16( O_text / l_text + ip_scale * O_img / l_img )                  one rounding, one launch.
template <int D16, bool ONES, bool IP = false>
__global__ void __launch_bounds__(256)
xattn64_kernel(const AttnArgs a, int xqb /* 128-query blocks per workgroup */, int nxb /* workgroups per batch*head */,
               int n_img /* IP: image tokens, 1 .. 32 */, float ip_scale) {
    constexpr int DP = 64, DT = 2, TILE = 64 * 128;
    constexpr int NTXT = IP ? 3 : 4;                                   // 32-key sub-tiles the first softmax may cover
    extern __shared__ __attribute__((aligned(16))) char smem[];      // K tile 0 | V^T tile 0 | K tile 1 | V^T tile 1
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    int xb, bh;
    {   // XCD-contiguous (batch*head, chunk) order as attn_block_map
        const int T = gridDim.x, bid = blockIdx.x;
        const int q = T >> 3, r = T & 7, xcd = bid & 7, idx = bid >> 3;
        const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        bh = w / nxb; xb = w - bh * nxb;
    }
    const half_t* Qb = a.q + (long)bh * a.q_tok_pad * DP;
    const half_t* Kb = a.k + (long)bh * a.k_tok_pad * DP;
    const half_t* Vb = a.vt + (long)bh * DP * a.k_tok_pad;
    const int ntiles = IP ? 2 : (a.nk_valid + 63) >> 6;      // 1 or 2
    {
        const int r8 = lane >> 3, pc = lane & 7;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (t < ntiles) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int row = wid * 16 + h * 8 + r8;
                    const int lc = pc ^ ((row >> 1) & 7);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Kb + (long)(t * 64 + row) * DP + lc * 8),
                                                     (__attribute__((address_space(3))) void*)(smem + t * 2 * TILE + (wid * 16 + h * 8) * 128), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Vb + (long)row * a.k_tok_pad + t * 64 + lc * 8),
                                                     (__attribute__((address_space(3))) void*)(smem + t * 2 * TILE + TILE + (wid * 16 + h * 8) * 128), 16, 0, 0);
                }
            }
        }
    }
    const int fsw = (l31 >> 1) & 7;
    const int frow = l31 * 128;
    const int nsub = (a.nk_valid + 31) >> 5;                 // 32-key sub-tiles with at least one valid key (1 .. 4)
    const int b = bh / a.heads, head = bh - b * a.heads;
    // first block's Q while the DMA is in flight
    half8_t qf[D16];
    int q0 = (xb * xqb) * 128 + wid * 32;
#pragma unroll
    for (int ks = 0; ks < D16; ++ks) qf[ks] = *reinterpret_cast<const half8_t*>(Qb + (long)(q0 + l31) * DP + ks * 16 + hi * 8);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int blk = 0; blk < xqb; ++blk) {
        half8_t qs[D16];
#pragma unroll
        for (int ks = 0; ks < D16; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) qs[ks][j] = (half_t)((float)qf[ks][j] * a.scale_log2e);
        const int qrow = q0 + l31;
        // next block's Q (clamped: the last block re-reads itself)
        const int q0n = blk + 1 < xqb ? q0 + 128 : q0;
#pragma unroll
        for (int ks = 0; ks < D16; ++ks) qf[ks] = *reinterpret_cast<const half8_t*>(Qb + (long)(q0n + l31) * DP + ks * 16 + hi * 8);
        // ---- S^T = K Q^T for up to four 32-key sub-tiles ----
        f32x16 s[NTXT];
#pragma unroll
        for (int st = 0; st < NTXT; ++st) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[st][r] = 0.f;
            if (st < nsub) {
                const char* Ks = smem + (st >> 1) * 2 * TILE + (st & 1) * 32 * 128;
#pragma unroll
                for (int ks = 0; ks < D16; ++ks) {
                    const half8_t kf = *reinterpret_cast<const half8_t*>(Ks + frow + ((((ks << 1) | hi) ^ fsw) << 4));
                    s[st] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qs[ks], s[st], 0, 0, 0);
                }
            }
        }
        // ---- softmax over all keys at once (log2 domain); keys >= nk_valid masked ----
        float mx = -INFINITY;
#pragma unroll
        for (int st = 0; st < NTXT; ++st) {
            if (st < nsub) {
                if (st == nsub - 1 && (a.nk_valid & 31) != 0) {      // (wave-uniform) only the last sub-tile has invalid keys
                    const int nv = (a.nk_valid & 31) - 4 * hi;         // valid keys of this sub-tile, seen from this half-wave
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[st][r] = ((r & 3) + 8 * (r >> 2)) < nv ? s[st][r] : -INFINITY;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[st][r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float psum = 0.f;
#pragma unroll
        for (int st = 0; st < NTXT; ++st) {
            if (st < nsub) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(s[st][r] - mx);
                    s[st][r] = pv;
                    if constexpr (!ONES) psum += IP ? (float)(half_t)pv : pv;     // IP form: the denominator of the P the MFMAs see
                }
            }
        }
        // ---- O^T = V^T P^T ----
        f32x16 oacc[DT];
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
#pragma unroll
        for (int st = 0; st < NTXT; ++st) {
            if (st < nsub) {
                const char* Vs = smem + (st >> 1) * 2 * TILE + TILE;
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    half8_t pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (half_t)s[st][8 * tt + j];
                    const int lc = (st & 1) * 4 + 2 * tt + hi;
#pragma unroll
                    for (int i = 0; i < DT; ++i) {
                        const half8_t vf = *reinterpret_cast<const half8_t*>(Vs + i * 32 * 128 + frow + ((lc ^ fsw) << 4));
                        oacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[i], 0, 0, 0);
                    }
                }
            }
        }
        float l_tot;
        if constexpr (ONES) {
            const int dr = a.d & 31;
            float lv = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) if (dr == 8 * g) lv = oacc[DT - 1][4 * g];
            l_tot = __shfl(lv, l31);
        } else {
            l_tot = psum + __shfl_xor(psum, 32);
        }
        const float inv_l = 1.0f / l_tot;
        if constexpr (IP) {
            // ---- the image keys: sub-tile 3 = rows 32 .. 63 of K tile 1, columns 32 .. 63 of V^T tile 1 ----
            __builtin_amdgcn_sched_barrier(0);       // the text pass is over: its score registers are free for what follows
            f32x16 si;
#pragma unroll
            for (int r = 0; r < 16; ++r) si[r] = 0.f;
            {
                const char* Ks = smem + 2 * TILE + 32 * 128;
#pragma unroll
                for (int ks = 0; ks < D16; ++ks) {
                    const half8_t kf = *reinterpret_cast<const half8_t*>(Ks + frow + ((((ks << 1) | hi) ^ fsw) << 4));
                    si = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qs[ks], si, 0, 0, 0);
                }
            }
            if (n_img < 32) {                                          // (wave-uniform)
                const int nv = n_img - 4 * hi;
#pragma unroll
                for (int r = 0; r < 16; ++r) si[r] = ((r & 3) + 8 * (r >> 2)) < nv ? si[r] : -INFINITY;
            }
            float mi = si[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mi = fmaxf(mi, si[r]);
            mi = fmaxf(mi, __shfl_xor(mi, 32));
            float pisum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(si[r] - mi);
                si[r] = pv;
                if constexpr (!ONES) pisum += (float)(half_t)pv;
            }
            f32x16 oi[DT];
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oi[i][r] = 0.f;
            {
                const char* Vs = smem + 2 * TILE + TILE;
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    half8_t pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (half_t)si[8 * tt + j];
                    const int lc = 4 + 2 * tt + hi;
#pragma unroll
                    for (int i = 0; i < DT; ++i) {
                        const half8_t vf = *reinterpret_cast<const half8_t*>(Vs + i * 32 * 128 + frow + ((lc ^ fsw) << 4));
                        oi[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oi[i], 0, 0, 0);
                    }
                }
            }
            float li;
            if constexpr (ONES) {
                const int dr = a.d & 31;
                float lv = 0.f;
#pragma unroll
                for (int g = 0; g < 4; ++g) if (dr == 8 * g) lv = oi[DT - 1][4 * g];
                li = __shfl(lv, l31);
            } else {
                li = pisum + __shfl_xor(pisum, 32);
            }
            const float wi = ip_scale / li;
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[i][r] = oacc[i][r] * inv_l + wi * oi[i][r];
        }
        if (qrow < a.nq) {
            half_t* orow = a.o + ((long)b * a.nq + qrow) * a.o_ld + head * a.d;
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int dd = i * 32 + 8 * g + 4 * hi;
                    if (dd < a.d) {
                        half4_t o;
#pragma unroll
                        for (int k = 0; k < 4; ++k) o[k] = (half_t)(IP ? oacc[i][4 * g + k] : oacc[i][4 * g + k] * inv_l);
                        *reinterpret_cast<half4_t*>(orow + dd) = o;
                    }
                }
        }
        q0 = q0n;
    }
}

// ---- cross-attention, dp = 64, 129 .. 320 keys (long prompts: 2 .. 4 chunks of 77 text tokens) --------------------------
// The flash loop reloads the head's K / V^T (48 - 80 KB) for every 128 queries and pays a pipeline prologue and a barrier per
// tile.  Here, as in xattn64_kernel, a workgroup loads K and V^T ONCE - ntiles = ceil(nk / 64) <= 5 tiles of (K | V^T), 16 KB each,
// by LDS-DMA in the layouts of attn64_kernel (source-side XOR swizzle, permuted V^T keys); the K half-tile of a 32-key sub-tile that
// lies wholly beyond nk_valid is not loaded (V^T rows span the whole 64-key tile and are loaded whole; such a sub-tile is never
// multiplied) - and after one wait and one barrier walks xqb blocks of 128 queries with no further barrier, the next block's Q
// prefetched.  The scores of 320 keys do not fit in registers, so inside a query block the resident tiles are walked with the
// online softmax of attn64_kernel: scores in the log2 domain from the pre-scaled fp16 Q, the accumulator of S^T initialised with
// -m_ref, P rounded to fp16 from the accumulator registers into the PV MFMA, the denominator through the ones row of V^T
// (d % 32 != 0) or an fp32 sum.  The running maximum uses the DEFERRED RE-REFERENCE of the flash loop (RESCALE_THR), not an exact
// running max.  Keys >= nk_valid are masked in the last partial 32-key sub-tile; nothing read from slots >= nk_valid reaches the
// result as long as it is finite (masked P = 0 meets it in the PV product).
// LDS: ntiles x 16 KB (48 KB at 154 keys: three workgroups per CU; 64 KB at 231, 80 KB at 308: two).
// Registers (gfx950, register allocation aimed at three waves per SIMD, what 48 KB of LDS allows): <3, ONES> 135 VGPRs,
// <4, ONES> 144, <4, fp32 sum> 142; no AGPRs, no scratch, 3 waves / SIMD.  The 128 that a fourth wave would need are not reached
// (the prefetched raw Q next to the scaled Q costs 16 registers) and would buy nothing: LDS caps a CU at three workgroups.
template <int D16, bool ONES>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
xattn64_long_kernel(const AttnArgs a, int xqb /* 128-query blocks per workgroup */, int nxb /* workgroups per batch*head */) {
    constexpr int DP = 64, DT = 2, TILE = 64 * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // (K tile t | V^T tile t) for t = 0 .. ntiles - 1
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    int xb, bh;
    {   // XCD-contiguous (batch*head, chunk) order as attn_block_map
        const int T = gridDim.x, bid = blockIdx.x;
        const int q = T >> 3, r = T & 7, xcd = bid & 7, idx = bid >> 3;
        const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        bh = w / nxb; xb = w - bh * nxb;
    }
    const half_t* Qb = a.q + (long)bh * a.q_tok_pad * DP;
    const half_t* Kb = a.k + (long)bh * a.k_tok_pad * DP;
    const half_t* Vb = a.vt + (long)bh * DP * a.k_tok_pad;
    const int ntiles = (a.nk_valid + 63) >> 6;               // 3 .. 5
    const int nsub = (a.nk_valid + 31) >> 5;                 // 32-key sub-tiles with at least one valid key
    {
        const int r8 = lane >> 3, pc = lane & 7;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            if (t < ntiles) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int row = wid * 16 + h * 8 + r8;
                    const int lc = pc ^ ((row >> 1) & 7);
                    if (t * 64 + wid * 16 < nsub * 32)         // (wave-uniform) K rows of a sub-tile with a valid key
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Kb + (long)(t * 64 + row) * DP + lc * 8),
                                                         (__attribute__((address_space(3))) void*)(smem + t * 2 * TILE + (wid * 16 + h * 8) * 128), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Vb + (long)row * a.k_tok_pad + t * 64 + lc * 8),
                                                     (__attribute__((address_space(3))) void*)(smem + t * 2 * TILE + TILE + (wid * 16 + h * 8) * 128), 16, 0, 0);
                }
            }
        }
    }
    const int fsw = (l31 >> 1) & 7;
    const int frow = l31 * 128;
    const int b = bh / a.heads, head = bh - b * a.heads;
    const int tailv = a.nk_valid & 31;                       // != 0: the last sub-tile is partially masked
    // first block's Q while the DMA is in flight
    half8_t qf[D16];
    int q0 = (xb * xqb) * 128 + wid * 32;
#pragma unroll
    for (int ks = 0; ks < D16; ++ks) qf[ks] = *reinterpret_cast<const half8_t*>(Qb + (long)(q0 + l31) * DP + ks * 16 + hi * 8);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int blk = 0; blk < xqb; ++blk) {
        half8_t qs[D16];
#pragma unroll
        for (int ks = 0; ks < D16; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) qs[ks][j] = (half_t)((float)qf[ks][j] * a.scale_log2e);
        const int qrow = q0 + l31;
        // next block's Q (clamped: the last block re-reads itself)
        const int q0n = blk + 1 < xqb ? q0 + 128 : q0;
#pragma unroll
        for (int ks = 0; ks < D16; ++ks) qf[ks] = *reinterpret_cast<const half8_t*>(Qb + (long)(q0n + l31) * DP + ks * 16 + hi * 8);

        f32x16 oacc[DT];
        f32x16 negm;                 // -m_ref over the 16 accumulator registers (C operand of the first S^T MFMA of a sub-tile)
        float l_run = 0.f;           // only used when !ONES
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[r] = 0.f;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;

        for (int t = 0; t < ntiles; ++t) {
            const char* Ks = smem + t * 2 * TILE;
            const char* Vs = Ks + TILE;
            const int nkt = nsub - 2 * t >= 2 ? 2 : 1;       // (wave-uniform) sub-tiles of this tile with a valid key
            // ---- S^T - m = K Q^T + (-m) for up to two 32-key sub-tiles (log2 domain) ----
            f32x16 s[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                if (kt < nkt) {
#pragma unroll
                    for (int ks = 0; ks < D16; ++ks) {
                        const half8_t kf = *reinterpret_cast<const half8_t*>(Ks + kt * 32 * 128 + frow + ((((ks << 1) | hi) ^ fsw) << 4));
                        s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qs[ks], ks == 0 ? negm : s[kt], 0, 0, 0);
                    }
                    if (tailv != 0 && 2 * t + kt == nsub - 1) {          // (wave-uniform) the one sub-tile with invalid keys
                        const int nv = tailv - 4 * hi;                   // its valid keys, seen from this half-wave
#pragma unroll
                        for (int r = 0; r < 16; ++r) s[kt][r] = ((r & 3) + 8 * (r >> 2)) < nv ? s[kt][r] : -INFINITY;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[kt][r] = -INFINITY;   // no valid key: neither loaded nor multiplied
                }
            }
            // ---- online softmax (deferred re-reference, as attn64_kernel) ----
            float mx = s[0][0];                      // tile max RELATIVE to m_ref
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kt][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            if (t == 0 || !__all(mx <= RESCALE_THR)) {   // (rare after the first tile) re-reference: exact
                const float delta = t == 0 ? mx : fmaxf(mx, 0.f);
                const float alpha = __builtin_amdgcn_exp2f(-delta);         // O = 0 on the first tile: alpha irrelevant
                l_run *= alpha;
#pragma unroll
                for (int i = 0; i < DT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) negm[r] -= delta;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[kt][r] -= delta;
            }
            float psum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(s[kt][r]);
                    s[kt][r] = pv;
                    if constexpr (!ONES) psum += pv;
                }
            if constexpr (!ONES) l_run += psum;
            // ---- O^T += V^T P^T ----
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                if (kt < nkt) {
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) {
                        half8_t pf;
#pragma unroll
                        for (int j = 0; j < 8; ++j) pf[j] = (half_t)s[kt][8 * tt + j];
                        const int lc = kt * 4 + 2 * tt + hi;               // logical 16-B chunk of the (permuted) key axis
#pragma unroll
                        for (int i = 0; i < DT; ++i) {
                            const half8_t vf = *reinterpret_cast<const half8_t*>(Vs + i * 32 * 128 + frow + ((lc ^ fsw) << 4));
                            oacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[i], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // ---- finalize: O = O^T / l, store token-major ----
        float l_tot;
        if constexpr (ONES) {
            const int dr = a.d & 31;
            float lv = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) if (dr == 8 * g) lv = oacc[DT - 1][4 * g];
            l_tot = __shfl(lv, l31);
        } else {
            l_tot = l_run + __shfl_xor(l_run, 32);
        }
        const float inv_l = 1.0f / l_tot;
        if (qrow < a.nq) {
            half_t* orow = a.o + ((long)b * a.nq + qrow) * a.o_ld + head * a.d;
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int dd = i * 32 + 8 * g + 4 * hi;
                    if (dd < a.d) {
                        half4_t o;
#pragma unroll
                        for (int k = 0; k < 4; ++k) o[k] = (half_t)(oacc[i][4 * g + k] * inv_l);
                        *reinterpret_cast<half4_t*>(orow + dd) = o;
                    }
                }
        }
        q0 = q0n;
    }
}

// ---- regional cross-attention, dp = 64: R = 2 .. 4 prompts of 77 tokens, every query attends to ONE of them ---------------
// Keys [77 r, 77 r + 77) of the resident K / V^T are region r's prompt; ids [map_rows][q_tok_pad] (uint8, pads 0) names the region
// of every query, and a query's result is softmax(q K_own) V_own over its own 77 keys - nothing else reaches it.  The frame is
// xattn64_long_kernel's: ceil(77 R / 64) = 3 .. 5 tiles of (K | V^T) loaded once by LDS-DMA, xqb query blocks per workgroup, the
// next block's Q (and region ids) prefetched, the XCD remap.  In the S^T accumulator layout a lane owns one query and its registers
// run over the keys, so the mask is a per-lane compare: register r of sub-tile kt of tile t holds key t*64 + kt*32 + (r&3) + 8(r>>2)
// + 4 hi, kept when (unsigned)(key - 77 rid) < 77, else -inf.  That mask covers the slots behind the context as well.
//
// Softmax: the ONLINE form is kept (choice, after reading the loop: an exact two-pass softmax over resident K doubles the QK^T
// MFMAs and their LDS reads, 3 .. 5 tiles x 8 MFMAs per query block; the online form adds one register of per-lane state).  What
// the long kernel's loop cannot do is start: a row of region r >= 1 has no own key in tile 0, its tile maximum there is -inf, and
// the unconditional "t == 0" re-reference would give delta = -inf, alpha = +inf, NaN accumulators.  Here every lane carries
// `seen` (an own key has been met).  Until then m_ref = 0, every P is exp2(-inf) = 0 and the accumulators stay 0.  The re-reference
// branch is taken when a lane meets its first own key (delta = its tile maximum, alpha = 1: nothing accumulated yet) or, as in the
// flash loop, when a seen lane's tile maximum exceeds RESCALE_THR (delta = max(mx, 0), alpha = 2^-delta); lanes that are neither
// get delta = 0, alpha = 1 - exact.  Tiles after a row's own keys have mx = -inf: no branch, P = 0.  Every tile with a valid key is
// multiplied for every wave: no wave-uniform skip of tiles without own keys (not measured, so not built).
// A region id >= n_regions (refused by the engine) is clamped to n_regions - 1.
// LDS: 48 KB (R = 2), 64 KB (R = 3), 80 KB (R = 4), as the long kernel at the same key counts: three / two / two workgroups per CU.
// Registers (gfx950, allocation aimed at three waves per SIMD): <3, ONES> 141 VGPRs, <4, ONES> 151, <4, fp32 sum> 151 (the long
// kernel's 135 / 144 / 142 plus the mask base, `seen` and the prefetched ids); no AGPRs, no scratch, 3 waves / SIMD.
template <int D16, bool ONES>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
xattn64_region_kernel(const AttnArgs a, int xqb /* 128-query blocks per workgroup */, int nxb /* workgroups per batch*head */,
                      const unsigned char* __restrict__ ids, int ids_bstride /* 0 (one map for all rows) or q_tok_pad */, int n_regions) {
    constexpr int DP = 64, DT = 2, TILE = 64 * 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];      // (K tile t | V^T tile t) for t = 0 .. ntiles - 1
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    int xb, bh;
    {   // XCD-contiguous (batch*head, chunk) order as attn_block_map
        const int T = gridDim.x, bid = blockIdx.x;
        const int q = T >> 3, r = T & 7, xcd = bid & 7, idx = bid >> 3;
        const int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        bh = w / nxb; xb = w - bh * nxb;
    }
    const half_t* Qb = a.q + (long)bh * a.q_tok_pad * DP;
    const half_t* Kb = a.k + (long)bh * a.k_tok_pad * DP;
    const half_t* Vb = a.vt + (long)bh * DP * a.k_tok_pad;
    const int ntiles = (a.nk_valid + 63) >> 6;               // 3 .. 5 (nk_valid = 77 * n_regions)
    const int nsub = (a.nk_valid + 31) >> 5;                 // 32-key sub-tiles with at least one valid key
    {
        const int r8 = lane >> 3, pc = lane & 7;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            if (t < ntiles) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int row = wid * 16 + h * 8 + r8;
                    const int lc = pc ^ ((row >> 1) & 7);
                    if (t * 64 + wid * 16 < nsub * 32)         // (wave-uniform) K rows of a sub-tile with a valid key
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Kb + (long)(t * 64 + row) * DP + lc * 8),
                                                         (__attribute__((address_space(3))) void*)(smem + t * 2 * TILE + (wid * 16 + h * 8) * 128), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Vb + (long)row * a.k_tok_pad + t * 64 + lc * 8),
                                                     (__attribute__((address_space(3))) void*)(smem + t * 2 * TILE + TILE + (wid * 16 + h * 8) * 128), 16, 0, 0);
                }
            }
        }
    }
    const int fsw = (l31 >> 1) & 7;
    const int frow = l31 * 128;
    const int b = bh / a.heads, head = bh - b * a.heads;
    const unsigned char* idb = ids + (long)b * ids_bstride;  // q0 + l31 < nqb * 128 <= q_tok_pad: every read is inside the row
    // first block's Q and region ids while the DMA is in flight
    half8_t qf[D16];
    int q0 = (xb * xqb) * 128 + wid * 32;
#pragma unroll
    for (int ks = 0; ks < D16; ++ks) qf[ks] = *reinterpret_cast<const half8_t*>(Qb + (long)(q0 + l31) * DP + ks * 16 + hi * 8);
    int ridf = idb[q0 + l31];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int blk = 0; blk < xqb; ++blk) {
        half8_t qs[D16];
#pragma unroll
        for (int ks = 0; ks < D16; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) qs[ks][j] = (half_t)((float)qf[ks][j] * a.scale_log2e);
        const int qrow = q0 + l31;
        // the lane's own keys seen from its half-wave: key - own0 in [0, 77) with key = t*64 + kt*32 + (r&3) + 8(r>>2) + 4 hi
        const int own0 = 77 * min(ridf, n_regions - 1) - 4 * hi;
        // next block's Q and region ids (clamped: the last block re-reads itself)
        const int q0n = blk + 1 < xqb ? q0 + 128 : q0;
#pragma unroll
        for (int ks = 0; ks < D16; ++ks) qf[ks] = *reinterpret_cast<const half8_t*>(Qb + (long)(q0n + l31) * DP + ks * 16 + hi * 8);
        ridf = idb[q0n + l31];

        f32x16 oacc[DT];
        f32x16 negm;                 // -m_ref over the 16 accumulator registers (C operand of the first S^T MFMA of a sub-tile)
        float l_run = 0.f;           // only used when !ONES
        bool seen = false;           // this lane's query has met an own key: m_ref is a real reference
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[r] = 0.f;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;

        for (int t = 0; t < ntiles; ++t) {
            const char* Ks = smem + t * 2 * TILE;
            const char* Vs = Ks + TILE;
            const int nkt = nsub - 2 * t >= 2 ? 2 : 1;       // (wave-uniform) sub-tiles of this tile with a valid key
            // ---- S^T - m = K Q^T + (-m) for up to two 32-key sub-tiles (log2 domain), foreign keys masked ----
            f32x16 s[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                if (kt < nkt) {
#pragma unroll
                    for (int ks = 0; ks < D16; ++ks) {
                        const half8_t kf = *reinterpret_cast<const half8_t*>(Ks + kt * 32 * 128 + frow + ((((ks << 1) | hi) ^ fsw) << 4));
                        s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qs[ks], ks == 0 ? negm : s[kt], 0, 0, 0);
                    }
                    const int rel0 = t * 64 + kt * 32 - own0;
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        s[kt][r] = (unsigned)(rel0 + ((r & 3) + 8 * (r >> 2))) < 77u ? s[kt][r] : -INFINITY;
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[kt][r] = -INFINITY;   // no valid key: neither loaded nor multiplied
                }
            }
            // ---- online softmax (deferred re-reference), started per lane at the first tile with an own key ----
            float mx = s[0][0];                      // tile max RELATIVE to m_ref (-inf: no own key in this tile)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kt][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const bool own_here = mx > -INFINITY;
            if (!__all(seen ? mx <= RESCALE_THR : !own_here)) {   // a first own key, or (rare) a jump: re-reference, exact
                const float delta = seen ? fmaxf(mx, 0.f) : own_here ? mx : 0.f;
                const float alpha = seen ? __builtin_amdgcn_exp2f(-delta) : 1.0f;      // not seen: O = 0, l = 0
                seen = seen || own_here;
                l_run *= alpha;
#pragma unroll
                for (int i = 0; i < DT; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) negm[r] -= delta;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[kt][r] -= delta;
            }
            float psum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(s[kt][r]);
                    s[kt][r] = pv;
                    if constexpr (!ONES) psum += pv;
                }
            if constexpr (!ONES) l_run += psum;
            // ---- O^T += V^T P^T ----
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                if (kt < nkt) {
#pragma unroll
                    for (int tt = 0; tt < 2; ++tt) {
                        half8_t pf;
#pragma unroll
                        for (int j = 0; j < 8; ++j) pf[j] = (half_t)s[kt][8 * tt + j];
                        const int lc = kt * 4 + 2 * tt + hi;               // logical 16-B chunk of the (permuted) key axis
#pragma unroll
                        for (int i = 0; i < DT; ++i) {
                            const half8_t vf = *reinterpret_cast<const half8_t*>(Vs + i * 32 * 128 + frow + ((lc ^ fsw) << 4));
                            oacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[i], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // ---- finalize: O = O^T / l, store token-major ----
        float l_tot;
        if constexpr (ONES) {
            const int dr = a.d & 31;
            float lv = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) if (dr == 8 * g) lv = oacc[DT - 1][4 * g];
            l_tot = __shfl(lv, l31);
        } else {
            l_tot = l_run + __shfl_xor(l_run, 32);
        }
        const float inv_l = 1.0f / l_tot;
        if (qrow < a.nq) {
            half_t* orow = a.o + ((long)b * a.nq + qrow) * a.o_ld + head * a.d;
#pragma unroll
            for (int i = 0; i < DT; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int dd = i * 32 + 8 * g + 4 * hi;
                    if (dd < a.d) {
                        half4_t o;
#pragma unroll
                        for (int k = 0; k < 4; ++k) o[k] = (half_t)(oacc[i][4 * g + k] * inv_l);
                        *reinterpret_cast<half4_t*>(orow + dd) = o;
                    }
                }
        }
        q0 = q0n;
    }
}

// Regional cross-attention for every other head dim (dp != 64: SD1.5's d = 80 / 160, the tiny nets' d = 32) and for dp = 64 under
// cfgpp_attention_set_dma(0) / set_cross(0): a correctness path in the mould of attn_ip_add_kernel.  One thread per (batch*head,
// query) runs the complete softmax over its region's 77 keys in fp32 with the rounding points of the MFMA kernels (q * d^-1/2 *
// log2(e) to fp16, P to fp16, the denominator summed from the rounded P, V^T read through cfgpp_vt_pos) and stores fp16(O / l).
// The 77 scores live in registers (256 VGPRs + 62 AGPRs, no scratch, one wave per SIMD: not a hot path); neighbouring threads of a
// region read the same K rows.  A region id >= n_regions is clamped.
__global__ void __launch_bounds__(256)
attn_region_rows_kernel(const AttnArgs a, int dp, const unsigned char* __restrict__ ids, int ids_bstride, int n_regions) {
    const int q = blockIdx.x * 256 + threadIdx.x, bh = blockIdx.y;
    if (q >= a.nq) return;
    const int b = bh / a.heads, head = bh - b * a.heads;
    const int key0 = 77 * min((int)ids[(long)b * ids_bstride + q], n_regions - 1);
    const half_t* Qr = a.q + ((long)bh * a.q_tok_pad + q) * dp;
    const half_t* Kr = a.k + ((long)bh * a.k_tok_pad + key0) * dp;
    const half_t* Vr = a.vt + (long)bh * dp * a.k_tok_pad;
    float sc[77];
#pragma unroll
    for (int k = 0; k < 77; ++k) sc[k] = 0.f;
    for (int d0 = 0; d0 < a.d; d0 += 8) {
        const half8_t raw = *reinterpret_cast<const half8_t*>(Qr + d0);
        float qs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) qs[j] = (float)(half_t)((float)raw[j] * a.scale_log2e);
#pragma unroll
        for (int k = 0; k < 77; ++k) {
            const half8_t kf = *reinterpret_cast<const half8_t*>(Kr + (long)k * dp + d0);
#pragma unroll
            for (int j = 0; j < 8; ++j) sc[k] += qs[j] * (float)kf[j];
        }
    }
    float m = sc[0];
#pragma unroll
    for (int k = 1; k < 77; ++k) m = fmaxf(m, sc[k]);
    float l = 0.f;
#pragma unroll
    for (int k = 0; k < 77; ++k) {
        sc[k] = (float)(half_t)__builtin_amdgcn_exp2f(sc[k] - m);
        l += sc[k];
    }
    const float inv_l = 1.0f / l;
    half_t* orow = a.o + ((long)b * a.nq + q) * a.o_ld + head * a.d;
    for (int d0 = 0; d0 < a.d; d0 += 4) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 77; ++k) {
            const int col = cfgpp_vt_pos(key0 + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += sc[k] * (float)Vr[(long)(d0 + j) * a.k_tok_pad + col];
        }
        half4_t o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (half_t)(acc[j] * inv_l);
        *reinterpret_cast<half4_t*>(orow + d0) = o;
    }
}

// ---- soft regional cross-attention, every padded head dim: R = 2 .. 4 prompts of 77 tokens BLENDED per query ----------------------
//     o = fp16( sum_r  w_r(q) / l_r  *  O_r ),    O_r = P_r V_r,  P_r = fp16(2^(s - m_r)) over keys [77 r, 77 r + 77) alone
// w is fp32 [map_rows][n_regions][q_tok_pad] (pads 0).  Every region's softmax is COMPLETE (77 keys, its own maximum, its own
// denominator), so nothing is re-referenced across regions and a lane carries no "own key met" state.  The frame is attn_kernel's
// (S^T layout: a lane owns a query; K / V^T tiles through padded LDS rows; P from the accumulator registers into the PV MFMA): keys
// [77 r, 77 r + 77) lie inside the two 64-key tiles r and r + 1 (77 r >> 6 == r and (77 r + 76) >> 6 == r + 1 for r = 0 .. 3), which
// are staged together (at dp = 160: 2 x 44.5 KB; the K / V^T of four regions would not fit, so regions are STREAMED through the one
// stage).  All 128 scores of the two tiles stay in registers (keys outside the region -inf; a 32-key sub-tile without a key of the
// region is neither multiplied nor exponentiated: r = 0, 1, 3 have three live sub-tiles, r = 2 four), the maximum is exact, the
// denominator is the ones row of V^T met by the rounded P (d % 32 != 0) or the fp32 sum of the ROUNDED P.
// Region skipping is a WORKGROUP vote: the tile loads sit behind __syncthreads, so the decision is taken from one LDS word per wave
// that every wave reads after a barrier - all four waves see the same four words, take the same branches and meet the same number of
// barriers.  A region in which no query of the workgroup's 128 has w != 0 is not loaded.  Inside an evaluated region a lane with
// w_r == 0 keeps its total as it is (a select, not a multiply by 0: the region's keys and values may hold junk that overflows).
// The vote words are the first 16 bytes of the DYNAMIC LDS (a static __shared__ would shift the 16-byte alignment of the tiles).
template <int D16, int DT, bool ONES>
__global__ void __launch_bounds__(256)
attn_region_soft_kernel(const AttnArgs a, const float* __restrict__ w, int w_bstride /* 0 (one map for all rows) or n_regions * q_tok_pad */,
                        int n_regions) {
    constexpr int DP = DT * 32;
    constexpr int KPITCH = DP * 2 + 16;          // bytes per K row in LDS
    constexpr int VPITCH = 64 * 2 + 16;          // bytes per V^T row in LDS (64 keys)
    constexpr int CH = (64 * DP / 8) / 256;      // 16-B chunks per thread per tile (K and V each)
    constexpr int STAGE = 64 * KPITCH + DP * VPITCH;
    static_assert((64 * DP / 8) % 256 == 0 && STAGE % 16 == 0, "tile/loader mismatch");
    extern __shared__ __attribute__((aligned(16))) char smem[];     // votes (16 B) | tile r (K | V^T) | tile r + 1 (K | V^T)
    int* vote = reinterpret_cast<int*>(smem);
    char* tiles = smem + 16;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    int qb, bh;
    attn_block_map(a.nqb, qb, bh);
    const int q0 = qb * 128 + wid * 32;
    const int b = bh / a.heads, head = bh - b * a.heads;
    const half_t* Qb = a.q + (long)bh * a.q_tok_pad * DP;
    const half_t* Kb = a.k + (long)bh * a.k_tok_pad * DP;
    const half_t* Vb = a.vt + (long)bh * DP * a.k_tok_pad;

    // the lane's query's weights (q0 + l31 < nqb * 128 <= q_tok_pad: inside the row), and the workgroup's vote
    const float* wq = w + (long)b * w_bstride + q0 + l31;
    float wv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wv[r] = r < n_regions ? wq[(long)r * a.q_tok_pad] : 0.f;
    int mine = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) mine |= __any(wv[r] != 0.f) ? (1 << r) : 0;
    if (lane == 0) vote[wid] = mine;
    __syncthreads();
    const int live = __builtin_amdgcn_readfirstlane(vote[0] | vote[1] | vote[2] | vote[3]);     // the same in every wave

    half8_t qf[D16];
#pragma unroll
    for (int ks = 0; ks < D16; ++ks) {
        const half8_t raw = *reinterpret_cast<const half8_t*>(Qb + (long)(q0 + l31) * DP + ks * 16 + hi * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[ks][j] = (half_t)((float)raw[j] * a.scale_log2e);
    }
    f32x16 otot[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) otot[i][rr] = 0.f;

#pragma unroll 1
    for (int r = 0; r < 4; ++r) {
        if (!((live >> r) & 1)) continue;        // WORKGROUP-uniform (see above): every wave skips, or none does
        const float wr = r == 0 ? wv[0] : r == 1 ? wv[1] : r == 2 ? wv[2] : wv[3];
        __syncthreads();                         // every wave is done with the previous region's tiles
        {
            half8_t rk[2][CH], rv[2][CH];
#pragma unroll
            for (int tl = 0; tl < 2; ++tl)
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const int c = tid + j * 256;
                    const int kr = c / (DP / 8), kc = c - kr * (DP / 8);
                    rk[tl][j] = *reinterpret_cast<const half8_t*>(Kb + (long)((r + tl) * 64 + kr) * DP + kc * 8);
                    const int vr = c >> 3, vc = c & 7;
                    rv[tl][j] = *reinterpret_cast<const half8_t*>(Vb + (long)vr * a.k_tok_pad + (r + tl) * 64 + vc * 8);
                }
#pragma unroll
            for (int tl = 0; tl < 2; ++tl) {
                char* Ks = tiles + tl * STAGE;
                char* Vs = Ks + 64 * KPITCH;
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const int c = tid + j * 256;
                    const int kr = c / (DP / 8), kc = c - kr * (DP / 8);
                    *reinterpret_cast<half8_t*>(Ks + kr * KPITCH + kc * 16) = rk[tl][j];
                    const int vr = c >> 3, vc = c & 7;
                    *reinterpret_cast<half8_t*>(Vs + vr * VPITCH + vc * 16) = rv[tl][j];
                }
            }
        }
        __syncthreads();

        // ---- S^T = K Q^T for the region's 32-key sub-tiles (log2 domain), keys outside [77 r, 77 r + 77) masked ----
        // register rr of sub-tile st holds key r * 64 + st * 32 + (rr & 3) + 8 (rr >> 2) + 4 hi
        const int own0 = 77 * r;
        f32x16 s[4];
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int lo = r * 64 + st * 32;
            if (lo < own0 + 77 && lo + 32 > own0) {              // (workgroup-uniform) the sub-tile holds a key of the region
                const char* Ks = tiles + (st >> 1) * STAGE;
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) s[st][rr] = 0.f;
#pragma unroll
                for (int ks = 0; ks < D16; ++ks) {
                    const half8_t kf = *reinterpret_cast<const half8_t*>(Ks + ((st & 1) * 32 + l31) * KPITCH + (ks * 16 + hi * 8) * 2);
                    s[st] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s[st], 0, 0, 0);
                }
                const int rel0 = lo + 4 * hi - own0;
#pragma unroll
                for (int rr = 0; rr < 16; ++rr)
                    s[st][rr] = (unsigned)(rel0 + ((rr & 3) + 8 * (rr >> 2))) < 77u ? s[st][rr] : -INFINITY;
            } else {
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) s[st][rr] = -INFINITY;
            }
        }
        // ---- the region's complete softmax: exact maximum over its 77 keys, P rounded to fp16 ----
        float mx = -INFINITY;
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int lo = r * 64 + st * 32;
            if (lo < own0 + 77 && lo + 32 > own0) {              // (workgroup-uniform) a dead sub-tile enters neither the maximum ..
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) mx = fmaxf(mx, s[st][rr]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float psum = 0.f;
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int lo = r * 64 + st * 32;
            if (lo < own0 + 77 && lo + 32 > own0) {              // .. nor the exponentials (its P is never read: the PV loop skips it too)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const float pv = __builtin_amdgcn_exp2f(s[st][rr] - mx);
                    s[st][rr] = pv;
                    if constexpr (!ONES) psum += (float)(half_t)pv;
                }
            }
        }
        // ---- O_r^T = V_r^T P^T ----
        f32x16 oacc[DT];
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) oacc[i][rr] = 0.f;
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int lo = r * 64 + st * 32;
            if (lo < own0 + 77 && lo + 32 > own0) {
                const char* Vs = tiles + (st >> 1) * STAGE + 64 * KPITCH;
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    half8_t pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (half_t)s[st][8 * tt + j];
                    const int kpos0 = (st & 1) * 32 + 16 * tt + 8 * hi;
#pragma unroll
                    for (int i = 0; i < DT; ++i) {
                        const half8_t vf = *reinterpret_cast<const half8_t*>(Vs + (i * 32 + l31) * VPITCH + kpos0 * 2);
                        oacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[i], 0, 0, 0);
                    }
                }
            }
        }
        // ---- total += (w_r / l_r) O_r for the lanes whose query has w_r != 0 ----
        float l_r;
        if constexpr (ONES) {
            const int dr = a.d & 31;                                   // multiple of 8 by contract
            float lv = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) if (dr == 8 * g) lv = oacc[DT - 1][4 * g];
            l_r = __shfl(lv, l31);
        } else {
            l_r = psum + __shfl_xor(psum, 32);
        }
        const bool on = wr != 0.f;
        const float coef = on ? wr / l_r : 0.f;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) otot[i][rr] = on ? fmaf(coef, oacc[i][rr], otot[i][rr]) : otot[i][rr];
    }

    // ---- store token-major: one rounding ----
    const int q = q0 + l31;
    if (q < a.nq) {
        half_t* orow = a.o + ((long)b * a.nq + q) * a.o_ld + head * a.d;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int dd = i * 32 + 8 * g + 4 * hi;
                if (dd < a.d) {
                    half4_t o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = (half_t)otot[i][4 * g + k];
                    *reinterpret_cast<half4_t*>(orow + dd) = o;
                }
            }
    }
}

template <int D16, int DT, bool ONES>
int launch_attn_region_soft(const AttnArgs& a, dim3 grid, hipStream_t s, const float* w, int w_bstride, int n_regions) {
    constexpr int DP = DT * 32;
    constexpr int smem = 16 + 2 * (64 * (DP * 2 + 16) + DP * (64 * 2 + 16));
    static bool attr_set = false;
    auto kern = attn_region_soft_kernel<D16, DT, ONES>;
    if (!attr_set) {
        CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), smem, s, a, w, w_bstride, n_regions);
    return 0;
}

template <int D16, bool ONES, int NST, int WPE = 3>
int launch_attn64(const AttnArgs& a, dim3 grid, hipStream_t s) {
    constexpr int smem = NST * 2 * 64 * 128;
    static bool attr_set = false;
    auto kern = attn64_kernel<D16, ONES, NST, WPE>;
    if (!attr_set) {
        CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), smem, s, a);
    return 0;
}

// sets row d of every V^T matrix to 1.0 (see the kernel header); vt [BH][dp][tok_pad]
__global__ void attn_ones_row_kernel(half_t* vt, int BH, int d, int dp, int tok_pad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)BH * tok_pad) return;
    const long bh = i / tok_pad, k = i - bh * tok_pad;
    vt[(bh * dp + d) * tok_pad + k] = (half_t)1.0f;
}

// Image branch of the decoupled cross-attention for the head dims without a fused instance (dp != 64: SD1.5's d = 80 / 160, the tiny
// nets' d = 32; correctness path).  o already holds fp16(O_text) from a launch of the kernels above over the text keys; one thread
// per (batch*head, query) runs the complete softmax over the image keys [96, 96 + n_img) in fp32 with the rounding points of the
// MFMA kernels (q * d^-1/2 * log2(e) to fp16, P to fp16, the denominator summed from the rounded P) and stores
//     o = fp16( float(o) + ip_scale * O_img / l_img ).
// K rows / V^T columns are the same for every thread of a block (uniform loads); n_img <= 32 scores live in registers.
__global__ void __launch_bounds__(256)
attn_ip_add_kernel(const AttnArgs a, int dp, int n_img, float ip_scale) {
    const int q = blockIdx.x * 256 + threadIdx.x, bh = blockIdx.y;
    if (q >= a.nq) return;
    const half_t* Qr = a.q + ((long)bh * a.q_tok_pad + q) * dp;
    const half_t* Ki = a.k + ((long)bh * a.k_tok_pad + 96) * dp;
    const half_t* Vi = a.vt + (long)bh * dp * a.k_tok_pad + 96;
    float sc[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) sc[k] = 0.f;
    for (int d0 = 0; d0 < a.d; d0 += 8) {
        const half8_t raw = *reinterpret_cast<const half8_t*>(Qr + d0);
        float qs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) qs[j] = (float)(half_t)((float)raw[j] * a.scale_log2e);
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (k < n_img) {
                const half8_t kf = *reinterpret_cast<const half8_t*>(Ki + (long)k * dp + d0);
#pragma unroll
                for (int j = 0; j < 8; ++j) sc[k] += qs[j] * (float)kf[j];
            }
    }
    float m = sc[0];
#pragma unroll
    for (int k = 1; k < 32; ++k) if (k < n_img) m = fmaxf(m, sc[k]);
    float l = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        sc[k] = k < n_img ? (float)(half_t)__builtin_amdgcn_exp2f(sc[k] - m) : 0.f;
        l += sc[k];
    }
    const float wi = ip_scale / l;
    const int b = bh / a.heads, head = bh - b * a.heads;
    half_t* orow = a.o + ((long)b * a.nq + q) * a.o_ld + head * a.d;
    for (int d0 = 0; d0 < a.d; d0 += 4) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (k < n_img) {
                const int col = cfgpp_vt_pos(k);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] += sc[k] * (float)Vi[(long)(d0 + j) * a.k_tok_pad + col];
            }
        half4_t o = *reinterpret_cast<const half4_t*>(orow + d0);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (half_t)((float)o[j] + wi * acc[j]);
        *reinterpret_cast<half4_t*>(orow + d0) = o;
    }
}

// zeroes key slots [slot0, slot0 + n) of every K matrix (all dp columns) and of rows < d of every V^T matrix - the ones row (row d)
// and the zero rows above it stay as they are.  One thread per (bh, 8 halfs): slot0, n and tok_pad are multiples of 8.
__global__ void attn_clear_slots_kernel(half_t* k, half_t* vt, int BH, int d, int dp, int tok_pad, int slot0, int n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per_k = (long)n * dp / 8, per_v = (long)d * n / 8;
    if (i >= (long)BH * (per_k + per_v)) return;
    const long bh = i / (per_k + per_v), r = i - bh * (per_k + per_v);
    const half8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < per_k) {
        *reinterpret_cast<half8_t*>(k + (bh * tok_pad + slot0) * dp + r * 8) = z;
    } else {
        const long e = r - per_k, row = e / (n / 8), c = e - row * (n / 8);
        *reinterpret_cast<half8_t*>(vt + (bh * dp + row) * tok_pad + slot0 + c * 8) = z;
    }
}

template <int D16, int DT, bool ONES, int QT>
int launch_attn(const AttnArgs& a, dim3 grid, hipStream_t s) {
    constexpr int DP = DT * 32;
    constexpr int smem = 2 * (64 * (DP * 2 + 16) + DP * (64 * 2 + 16));
    static bool attr_set = false;
    auto kern = attn_kernel<D16, DT, ONES, QT>;
    if (!attr_set) {
        CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), smem, s, a);
    return 0;
}

}  // namespace

static int g_attn_dma = 1;       // dp = 64: 1 = LDS-DMA kernel, 0 = register-staged kernel (A/B switch).  (A software-pipelined form
                                 // with two score tiles live was built and measured in round 3 - correct, 8 % slower: fewer resident waves -
                                 // and removed in round 4; profiles/r03/ab/attention_variants_alone.txt.  Round 4's woven form - QK^T of
                                 // tile t+1 and PV of tile t-1 issued between slices of tile t's softmax, two workgroups per CU - was +6..11 %
                                 // alone, neutral per forward and no better in matrix-pipe utilisation: commit 926a7ad)
static int g_attn_cross = 1;     // dp = 64, <= 128 keys: 1 = the resident-K/V cross-attention kernel, 0 = the flash loop (A/B switch)
static int g_attn_cross_long = 1;   // dp = 64, 129 .. 320 keys through cfgpp_op_attention_cross: 0 = the flash loop, 1 = xattn64_long_kernel for the classes
                                    // it measured >= 3 % faster in (d <= 48, or nk <= 192: see cfgpp_op_attention_cross), 2 = for every shape in its scope (tests, A/B)
static int g_attn_stagger = 0;   // attn64_kernel: phase shift between the workgroups of a CU, in 64-cycle sleeps per slot (0 = off)
// what the last cfgpp_op_attention / cfgpp_op_attention_ip call dispatched (host-side record, test hook): {kernel, D16, ONES, xqb};
// kernel 0 = nothing launched (refused), 1 = attn_kernel, 2 = attn64_kernel, 3 = xattn64_kernel, 4 = xattn64_kernel IP form,
// 5 = attn_ip_add_kernel (the last launch of the two-pass form), 6 = xattn64_long_kernel (cfgpp_op_attention_cross); xqb = 0 for the
// flash kernels and for 5
static int g_attn_last[4] = {0, 0, 0, 0};
static void attn_note(int kernel, int d16, int ones, int xqb) {
    g_attn_last[0] = kernel; g_attn_last[1] = d16; g_attn_last[2] = ones; g_attn_last[3] = xqb;
}

extern "C" {

void cfgpp_attention_set_dma(int mode) { g_attn_dma = mode ? 1 : 0; }
void cfgpp_attention_set_stagger(int sleeps) { g_attn_stagger = sleeps > 0 ? sleeps : 0; }
void cfgpp_attention_set_cross(int on) { g_attn_cross = on ? 1 : 0; }
void cfgpp_attention_set_cross_long(int mode) { g_attn_cross_long = mode < 0 ? 0 : mode > 2 ? 2 : mode; }
void cfgpp_attention_last_launch(int* out4) { for (int i = 0; i < 4; ++i) out4[i] = g_attn_last[i]; }

// V^T contract: when d is not a multiple of 32, row d of every [dp][tok_pad] matrix must hold ones (softmax
// denominator through the PV MFMA).  Call once after allocating / zeroing the buffer; the QKV epilogue never
// writes rows >= d.
int cfgpp_op_attention_prepare_vt(void* vt, int BH, int d, int tok_pad, void* stream) {
    CFGPP_REQUIRE(vt && BH > 0 && d > 0 && tok_pad > 0, "attention_prepare_vt: bad args");
    if (d % 32 == 0) return 0;
    CFGPP_REQUIRE(d % 8 == 0, "attention: head dim %d (not a multiple of 32) must be a multiple of 8", d);
    const int dp = (d + 31) / 32 * 32;
    hipLaunchKernelGGL(attn_ones_row_kernel, dim3(cdiv((long)BH * tok_pad, 256)), dim3(256), 0, (hipStream_t)stream, (half_t*)vt, BH, d, dp, tok_pad);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

// Zero the key slots [slot0, slot0 + n) of k [BH][tok_pad][dp] and vt [BH][dp][tok_pad] without touching the ones row of vt (the
// image-token slots of the cross-attention buffers, before a new set of image tokens is projected into them).
int cfgpp_op_attention_clear_slots(void* k, void* vt, int BH, int d, int tok_pad, int slot0, int n, void* stream) {
    CFGPP_REQUIRE(k && vt && BH > 0 && d > 0 && d % 8 == 0, "attention_clear_slots: bad args (d=%d)", d);
    CFGPP_REQUIRE(slot0 >= 0 && n > 0 && slot0 % 8 == 0 && n % 8 == 0 && tok_pad % 8 == 0 && slot0 + n <= tok_pad,
                  "attention_clear_slots: slots [%d, %d) of %d (multiples of 8)", slot0, slot0 + n, tok_pad);
    const int dp = (d + 31) / 32 * 32;
    const long total = (long)BH * ((long)n * dp / 8 + (long)d * n / 8);
    hipLaunchKernelGGL(attn_clear_slots_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (half_t*)k, (half_t*)vt, BH, d, dp, tok_pad, slot0, n);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

// q [B*heads][q_tok_pad][dp], k [B*heads][k_tok_pad][dp], vt [B*heads][dp][k_tok_pad], all fp16, dp = round_up(d,32),
// pads zero EXCEPT the ones row of vt (above).  o [B][nq][heads*d] fp16.  q_tok_pad % 128 == 0, k_tok_pad % 64 == 0.
int cfgpp_op_attention(const void* q, const void* k, const void* vt, void* o, int B, int heads, int d,
                       int nq, int nk, int q_tok_pad, int k_tok_pad, void* stream) {
    attn_note(0, 0, 0, 0);
    CFGPP_REQUIRE(q && k && vt && o, "attention: null pointer");
    CFGPP_REQUIRE(d > 0 && d <= 160 && (d % 32 == 0 || d % 8 == 0), "attention: head dim %d unsupported (multiple of 8, <= 160)", d);
    CFGPP_REQUIRE(q_tok_pad % 128 == 0 && q_tok_pad >= nq, "attention: q_tok_pad=%d (nq=%d) must be a multiple of 128", q_tok_pad, nq);
    CFGPP_REQUIRE(k_tok_pad % 64 == 0 && k_tok_pad >= nk, "attention: k_tok_pad=%d (nk=%d) must be a multiple of 64", k_tok_pad, nk);
    AttnArgs a;
    a.q = (const half_t*)q; a.k = (const half_t*)k; a.vt = (const half_t*)vt; a.o = (half_t*)o;
    a.heads = heads; a.d = d; a.nq = nq; a.nk_valid = nk; a.q_tok_pad = q_tok_pad; a.k_tok_pad = k_tok_pad;
    a.o_ld = heads * d;
    a.scale_log2e = (1.0f / sqrtf((float)d)) * 1.4426950408889634f;
    a.nqb = cdiv(nq, 128);
    a.stagger = g_attn_stagger;
    dim3 grid(a.nqb * B * heads);
    hipStream_t s = (hipStream_t)stream;
    const int d16 = (d + 15) / 16, dt = (d + 31) / 32;
    const bool ones = (d % 32) != 0;
    if (dt == 2 && g_attn_dma && g_attn_cross && nk <= 128 && k_tok_pad >= 64 * ((nk + 63) >> 6)) {
        // cross-attention (77 text tokens): K / V^T resident per workgroup, single-pass softmax, XQB query blocks per workgroup
        const int BH = B * heads;
        int xqb = 1;
        while (xqb < 8 && a.nqb % (xqb * 2) == 0 && (long)BH * (a.nqb / (xqb * 2)) >= 512) xqb *= 2;
        const int nxb = a.nqb / xqb;
        static bool attr_set = false;
        if (!attr_set) {
            CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_kernel<3, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 64 * 128));
            CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_kernel<4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 64 * 128));
            CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_kernel<4, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 64 * 128));
            attr_set = true;
        }
        const dim3 xg(BH * nxb);
        if (d16 == 3) hipLaunchKernelGGL((xattn64_kernel<3, true>), xg, dim3(256), 4 * 64 * 128, s, a, xqb, nxb, 0, 0.f);
        else if (ones) hipLaunchKernelGGL((xattn64_kernel<4, true>), xg, dim3(256), 4 * 64 * 128, s, a, xqb, nxb, 0, 0.f);
        else hipLaunchKernelGGL((xattn64_kernel<4, false>), xg, dim3(256), 4 * 64 * 128, s, a, xqb, nxb, 0, 0.f);
        CFGPP_HIP_CHECK(hipGetLastError());
        attn_note(3, d16, ones, xqb);
        return 0;
    }
    if (dt == 2 && g_attn_dma) {                   // dp = 64 (d = 40, 48, 56, 64): LDS-DMA kernel
        int rc;        // (a 2-stage ring was measured within 1 % of the 3-stage one and is not built)
        // four workgroups per CU: two-stage ring (32 KB), <= 128 VGPRs (the three-per-CU form on a 3-stage ring of rounds 2-3 measured
        // 3 - 9 % slower alone and 0.3 - 1 % per forward, profiles/r04/ab/attention_occupancy_call9.txt / _call10.txt)
        if (d16 == 3) rc = launch_attn64<3, true, 2, 4>(a, grid, s);
        else rc = ones ? launch_attn64<4, true, 2, 4>(a, grid, s) : launch_attn64<4, false, 2, 4>(a, grid, s);
        if (rc) return -1;
        CFGPP_HIP_CHECK(hipGetLastError());
        attn_note(2, d16, ones, 0);
        return 0;
    }
#define ATTN_CASE(D16_, DT_) \
    if (d16 == D16_ && dt == DT_) { if (ones ? launch_attn<D16_, DT_, true, 1>(a, grid, s) : launch_attn<D16_, DT_, false, 1>(a, grid, s)) return -1; } else
    ATTN_CASE(1, 1) ATTN_CASE(2, 1) ATTN_CASE(3, 2) ATTN_CASE(4, 2) ATTN_CASE(5, 3) ATTN_CASE(6, 3)
    ATTN_CASE(8, 4) ATTN_CASE(10, 5)
    { cfgpp_set_error("attention: no kernel instance for head dim %d", d); return -2; }
#undef ATTN_CASE
    CFGPP_HIP_CHECK(hipGetLastError());
    attn_note(1, d16, ones, 0);
    return 0;
}

// Cross-attention of the UNet: cfgpp_op_attention, except where xattn64_long_kernel (record: kernel 6) is taken.  Its scope is
// dp = 64 with 129 .. 320 keys (a text context of 2 .. 4 chunks of 77 tokens); what SHIPS (mode 1, the default) is the part of
// that scope where the interleaved per-launch A/B against the flash loop on the MI355X gave >= 3 % (the in-situ tuner's threshold
// for a pin; profiles/long_prompt/launch_ab.jsonl, run-to-run spreads <= 3 %): D16 = 3 (d = 40, 48) at every key count (-11.9 %
// at 154 keys, -3.9 % at 231, -3.4 % at 308) and D16 = 4 (d = 56, 64) at up to three resident tiles, nk <= 192 (-3.2 % at
// Nq = 4096, -7.2 % at 1024).  Not shipped: D16 = 4 at four / five tiles (+11 .. +16 %: two 64 - 80 KB workgroups per CU hide less
// latency than the flash loop's four).  Mode 2 takes the whole scope.  Every other shape is forwarded: same launch, same bits,
// same record.
int cfgpp_op_attention_cross(const void* q, const void* k, const void* vt, void* o, int B, int heads, int d,
                             int nq, int nk, int q_tok_pad, int k_tok_pad, void* stream) {
    const int dt = (d + 31) / 32;
    const bool scope = dt == 2 && g_attn_dma && g_attn_cross && nk >= 129 && nk <= 320;
    const bool measured = (d + 15) / 16 == 3 || nk <= 192;
    if (!(scope && (g_attn_cross_long == 2 || (g_attn_cross_long == 1 && measured))))
        return cfgpp_op_attention(q, k, vt, o, B, heads, d, nq, nk, q_tok_pad, k_tok_pad, stream);
    attn_note(0, 0, 0, 0);
    CFGPP_REQUIRE(q && k && vt && o, "attention_cross: null pointer");
    CFGPP_REQUIRE(B > 0 && heads > 0 && nq > 0, "attention_cross: B=%d heads=%d nq=%d", B, heads, nq);
    CFGPP_REQUIRE(d % 8 == 0, "attention_cross: head dim %d unsupported (multiple of 8)", d);
    CFGPP_REQUIRE(q_tok_pad % 128 == 0 && q_tok_pad >= nq, "attention_cross: q_tok_pad=%d (nq=%d) must be a multiple of 128", q_tok_pad, nq);
    CFGPP_REQUIRE(k_tok_pad % 64 == 0 && k_tok_pad >= nk, "attention_cross: k_tok_pad=%d (nk=%d) must be a multiple of 64", k_tok_pad, nk);
    AttnArgs a;
    a.q = (const half_t*)q; a.k = (const half_t*)k; a.vt = (const half_t*)vt; a.o = (half_t*)o;
    a.heads = heads; a.d = d; a.nq = nq; a.nk_valid = nk; a.q_tok_pad = q_tok_pad; a.k_tok_pad = k_tok_pad;
    a.o_ld = heads * d;
    a.scale_log2e = (1.0f / sqrtf((float)d)) * 1.4426950408889634f;
    a.nqb = cdiv(nq, 128);
    a.stagger = 0;
    const int d16 = (d + 15) / 16, BH = B * heads;
    const bool ones = (d % 32) != 0;
    int xqb = 1;        // the walk of cfgpp_op_attention's cross-attention branch
    while (xqb < 8 && a.nqb % (xqb * 2) == 0 && (long)BH * (a.nqb / (xqb * 2)) >= 512) xqb *= 2;
    const int nxb = a.nqb / xqb;
    constexpr int kMaxSmem = 5 * 2 * 64 * 128;
    static bool attr_set = false;
    if (!attr_set) {
        CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_long_kernel<3, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxSmem));
        CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_long_kernel<4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxSmem));
        CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_long_kernel<4, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxSmem));
        attr_set = true;
    }
    const int smem = ((nk + 63) >> 6) * 2 * 64 * 128;      // <= k_tok_pad * 256 bytes: every tile the DMA reads lies inside the buffers
    const dim3 xg(BH * nxb);
    hipStream_t s = (hipStream_t)stream;
    if (d16 == 3) hipLaunchKernelGGL((xattn64_long_kernel<3, true>), xg, dim3(256), smem, s, a, xqb, nxb);
    else if (ones) hipLaunchKernelGGL((xattn64_long_kernel<4, true>), xg, dim3(256), smem, s, a, xqb, nxb);
    else hipLaunchKernelGGL((xattn64_long_kernel<4, false>), xg, dim3(256), smem, s, a, xqb, nxb);
    CFGPP_HIP_CHECK(hipGetLastError());
    attn_note(6, d16, ones, xqb);
    return 0;
}

// Decoupled cross-attention (IP-Adapter): o = fp16( softmax(q K_text) V_text + ip_scale * softmax(q K_img) V_img ).  Buffers as
// cfgpp_op_attention with k_tok_pad >= 128: keys [0, nk_text), nk_text <= 96, are the text, keys [96, 96 + n_img), n_img <= 32, the
// image tokens; every other slot is a pad that enters neither softmax.  The V^T permutation and the ones row hold for the image
// columns as for the text ones.  dp = 64 with the default switches: ONE launch of xattn64_kernel<.., IP = true> (record: kernel 4).
// Every other head dim, or dp = 64 under cfgpp_attention_set_dma(0) / set_cross(0): cfgpp_op_attention over the text keys (O_text
// rounded to fp16), then attn_ip_add_kernel (record: kernel 5).  ip_scale == 0 is the text-only call: cfgpp_op_attention, its record.
int cfgpp_op_attention_ip(const void* q, const void* k, const void* vt, void* o, int B, int heads, int d, int nq, int nk_text,
                          int n_img, float ip_scale, int q_tok_pad, int k_tok_pad, void* stream) {
    attn_note(0, 0, 0, 0);
    CFGPP_REQUIRE(q && k && vt && o, "attention_ip: null pointer");
    CFGPP_REQUIRE(B > 0 && heads > 0 && nq > 0, "attention_ip: B=%d heads=%d nq=%d", B, heads, nq);
    CFGPP_REQUIRE(nk_text >= 1 && nk_text <= 96, "attention_ip: nk_text=%d (1 .. 96 text keys; the image keys start at slot 96)", nk_text);
    CFGPP_REQUIRE(n_img >= 1 && n_img <= 32, "attention_ip: n_img=%d (1 .. 32 image tokens)", n_img);
    CFGPP_REQUIRE(k_tok_pad >= 128 && k_tok_pad % 64 == 0, "attention_ip: k_tok_pad=%d must be a multiple of 64 and >= 128", k_tok_pad);
    CFGPP_REQUIRE(d > 0 && d <= 160 && d % 8 == 0, "attention_ip: head dim %d unsupported (multiple of 8, <= 160)", d);
    CFGPP_REQUIRE(q_tok_pad % 128 == 0 && q_tok_pad >= nq, "attention_ip: q_tok_pad=%d (nq=%d) must be a multiple of 128", q_tok_pad, nq);
    if (ip_scale == 0.f) return cfgpp_op_attention(q, k, vt, o, B, heads, d, nq, nk_text, q_tok_pad, k_tok_pad, stream);
    AttnArgs a;
    a.q = (const half_t*)q; a.k = (const half_t*)k; a.vt = (const half_t*)vt; a.o = (half_t*)o;
    a.heads = heads; a.d = d; a.nq = nq; a.nk_valid = nk_text; a.q_tok_pad = q_tok_pad; a.k_tok_pad = k_tok_pad;
    a.o_ld = heads * d;
    a.scale_log2e = (1.0f / sqrtf((float)d)) * 1.4426950408889634f;
    a.nqb = cdiv(nq, 128);
    a.stagger = 0;
    hipStream_t s = (hipStream_t)stream;
    const int d16 = (d + 15) / 16, dt = (d + 31) / 32, BH = B * heads;
    const bool ones = (d % 32) != 0;
    if (dt == 2 && g_attn_dma && g_attn_cross) {
        int xqb = 1;        // the walk of cfgpp_op_attention's cross-attention branch
        while (xqb < 8 && a.nqb % (xqb * 2) == 0 && (long)BH * (a.nqb / (xqb * 2)) >= 512) xqb *= 2;
        const int nxb = a.nqb / xqb;
        static bool attr_set = false;
        if (!attr_set) {
            CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_kernel<3, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 64 * 128));
            CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_kernel<4, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 64 * 128));
            CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_kernel<4, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 64 * 128));
            attr_set = true;
        }
        const dim3 xg(BH * nxb);
        if (d16 == 3) hipLaunchKernelGGL((xattn64_kernel<3, true, true>), xg, dim3(256), 4 * 64 * 128, s, a, xqb, nxb, n_img, ip_scale);
        else if (ones) hipLaunchKernelGGL((xattn64_kernel<4, true, true>), xg, dim3(256), 4 * 64 * 128, s, a, xqb, nxb, n_img, ip_scale);
        else hipLaunchKernelGGL((xattn64_kernel<4, false, true>), xg, dim3(256), 4 * 64 * 128, s, a, xqb, nxb, n_img, ip_scale);
        CFGPP_HIP_CHECK(hipGetLastError());
        attn_note(4, d16, ones, xqb);
        return 0;
    }
    int e = cfgpp_op_attention(q, k, vt, o, B, heads, d, nq, nk_text, q_tok_pad, k_tok_pad, stream);
    if (e) return e;
    hipLaunchKernelGGL(attn_ip_add_kernel, dim3(cdiv(nq, 256), BH), dim3(256), 0, s, a, dt * 32, n_img, ip_scale);
    CFGPP_HIP_CHECK(hipGetLastError());
    attn_note(5, d16, ones, 0);
    return 0;
}

// Regional cross-attention: n_regions = 2 .. 4 prompts of 77 tokens in key slots [77 r, 77 r + 77) of buffers laid out as for
// cfgpp_op_attention_cross (nk = 77 * n_regions); ids is a DEVICE uint8 [map_rows][q_tok_pad] (map_rows = 1: one map for every batch
// row, or B; pads 0) and query p of row b answers with softmax(q K_own) V_own over the 77 keys of region ids[b][p] alone.  Slots
// [77 * n_regions, k_tok_pad) may hold anything finite.  Head dims padded to 64 with the default switches: xattn64_region_kernel
// (record: kernel 7, with its xqb).  Every other head dim, or dp = 64 under cfgpp_attention_set_dma(0) / set_cross(0):
// attn_region_rows_kernel (record: kernel 8, xqb 0).
int cfgpp_op_attention_region(const void* q, const void* k, const void* vt, void* o, int B, int heads, int d, int nq, int n_regions,
                              const void* ids, int map_rows, int q_tok_pad, int k_tok_pad, void* stream) {
    attn_note(0, 0, 0, 0);
    CFGPP_REQUIRE(q && k && vt && o, "attention_region: null pointer");
    CFGPP_REQUIRE(ids, "attention_region: null ids (a device uint8 [map_rows][q_tok_pad] region map)");
    CFGPP_REQUIRE(B > 0 && heads > 0 && nq > 0, "attention_region: B=%d heads=%d nq=%d", B, heads, nq);
    CFGPP_REQUIRE(n_regions >= 2 && n_regions <= 4, "attention_region: n_regions=%d (2 .. 4 regions of 77 keys)", n_regions);
    CFGPP_REQUIRE(map_rows == 1 || map_rows == B, "attention_region: map_rows=%d (1 or B=%d)", map_rows, B);
    CFGPP_REQUIRE(d > 0 && d <= 160 && d % 8 == 0, "attention_region: head dim %d unsupported (multiple of 8, <= 160)", d);
    CFGPP_REQUIRE(q_tok_pad % 128 == 0 && q_tok_pad >= nq, "attention_region: q_tok_pad=%d (nq=%d) must be a multiple of 128", q_tok_pad, nq);
    const int nk = 77 * n_regions, need = (nk + 63) / 64 * 64;
    CFGPP_REQUIRE(k_tok_pad % 64 == 0 && k_tok_pad >= need, "attention_region: k_tok_pad=%d must be a multiple of 64 and >= %d (n_regions=%d: %d keys)",
                  k_tok_pad, need, n_regions, nk);
    AttnArgs a;
    a.q = (const half_t*)q; a.k = (const half_t*)k; a.vt = (const half_t*)vt; a.o = (half_t*)o;
    a.heads = heads; a.d = d; a.nq = nq; a.nk_valid = nk; a.q_tok_pad = q_tok_pad; a.k_tok_pad = k_tok_pad;
    a.o_ld = heads * d;
    a.scale_log2e = (1.0f / sqrtf((float)d)) * 1.4426950408889634f;
    a.nqb = cdiv(nq, 128);
    a.stagger = 0;
    hipStream_t s = (hipStream_t)stream;
    const int d16 = (d + 15) / 16, dt = (d + 31) / 32, BH = B * heads;
    const bool ones = (d % 32) != 0;
    const unsigned char* idp = (const unsigned char*)ids;
    const int ids_bstride = map_rows == 1 ? 0 : q_tok_pad;
    if (dt == 2 && g_attn_dma && g_attn_cross) {
        int xqb = 1;        // the walk of cfgpp_op_attention's cross-attention branch
        while (xqb < 8 && a.nqb % (xqb * 2) == 0 && (long)BH * (a.nqb / (xqb * 2)) >= 512) xqb *= 2;
        const int nxb = a.nqb / xqb;
        constexpr int kMaxSmem = 5 * 2 * 64 * 128;
        static bool attr_set = false;
        if (!attr_set) {
            CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_region_kernel<3, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxSmem));
            CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_region_kernel<4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxSmem));
            CFGPP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(xattn64_region_kernel<4, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxSmem));
            attr_set = true;
        }
        const int smem = ((nk + 63) >> 6) * 2 * 64 * 128;      // <= k_tok_pad * 256 bytes: every tile the DMA reads lies inside the buffers
        const dim3 xg(BH * nxb);
        if (d16 == 3) hipLaunchKernelGGL((xattn64_region_kernel<3, true>), xg, dim3(256), smem, s, a, xqb, nxb, idp, ids_bstride, n_regions);
        else if (ones) hipLaunchKernelGGL((xattn64_region_kernel<4, true>), xg, dim3(256), smem, s, a, xqb, nxb, idp, ids_bstride, n_regions);
        else hipLaunchKernelGGL((xattn64_region_kernel<4, false>), xg, dim3(256), smem, s, a, xqb, nxb, idp, ids_bstride, n_regions);
        CFGPP_HIP_CHECK(hipGetLastError());
        attn_note(7, d16, ones, xqb);
        return 0;
    }
    hipLaunchKernelGGL(attn_region_rows_kernel, dim3(cdiv(nq, 256), BH), dim3(256), 0, s, a, dt * 32, idp, ids_bstride, n_regions);
    CFGPP_HIP_CHECK(hipGetLastError());
    attn_note(8, d16, ones, 0);
    return 0;
}

// Soft regional cross-attention: buffers as for cfgpp_op_attention_region; w is a DEVICE fp32 [map_rows][n_regions][q_tok_pad]
// (map_rows = 1 or B, pads 0) and query p of row b answers with fp16( sum_r w[b][r][p] * softmax(q K_r) V_r ), every region's softmax
// complete over its own 77 keys; a term with w == 0 is not evaluated.  attn_region_soft_kernel for every head dim cfgpp_op_attention
// has an instance for (record: kernel 9, xqb 0); the other head dims are refused by name.  The A/B switches do not reach it.
int cfgpp_op_attention_region_soft(const void* q, const void* k, const void* vt, void* o, int B, int heads, int d, int nq, int n_regions,
                                   const void* w, int map_rows, int q_tok_pad, int k_tok_pad, void* stream) {
    attn_note(0, 0, 0, 0);
    CFGPP_REQUIRE(q && k && vt && o, "attention_region_soft: null pointer");
    CFGPP_REQUIRE(w, "attention_region_soft: null weights (a device fp32 [map_rows][n_regions][q_tok_pad] map)");
    CFGPP_REQUIRE(B > 0 && heads > 0 && nq > 0, "attention_region_soft: B=%d heads=%d nq=%d", B, heads, nq);
    CFGPP_REQUIRE(n_regions >= 2 && n_regions <= 4, "attention_region_soft: n_regions=%d (2 .. 4 regions of 77 keys)", n_regions);
    CFGPP_REQUIRE(map_rows == 1 || map_rows == B, "attention_region_soft: map_rows=%d (1 or B=%d)", map_rows, B);
    CFGPP_REQUIRE(d > 0 && d <= 160 && d % 8 == 0, "attention_region_soft: head dim %d unsupported (multiple of 8, <= 160)", d);
    CFGPP_REQUIRE(q_tok_pad % 128 == 0 && q_tok_pad >= nq, "attention_region_soft: q_tok_pad=%d (nq=%d) must be a multiple of 128", q_tok_pad, nq);
    // region r is read as the two 64-key tiles r and r + 1: 64 (n_regions + 1) == round_up(77 n_regions, 64) slots for 2 .. 4 regions
    const int nk = 77 * n_regions, need = 64 * (n_regions + 1);
    CFGPP_REQUIRE(k_tok_pad % 64 == 0 && k_tok_pad >= need, "attention_region_soft: k_tok_pad=%d must be a multiple of 64 and >= %d (n_regions=%d: %d keys)",
                  k_tok_pad, need, n_regions, nk);
    AttnArgs a;
    a.q = (const half_t*)q; a.k = (const half_t*)k; a.vt = (const half_t*)vt; a.o = (half_t*)o;
    a.heads = heads; a.d = d; a.nq = nq; a.nk_valid = nk; a.q_tok_pad = q_tok_pad; a.k_tok_pad = k_tok_pad;
    a.o_ld = heads * d;
    a.scale_log2e = (1.0f / sqrtf((float)d)) * 1.4426950408889634f;
    a.nqb = cdiv(nq, 128);
    a.stagger = 0;
    hipStream_t s = (hipStream_t)stream;
    const int d16 = (d + 15) / 16, dt = (d + 31) / 32;
    const bool ones = (d % 32) != 0;
    const dim3 grid(a.nqb * B * heads);
    const float* wp = (const float*)w;
    const int w_bstride = map_rows == 1 ? 0 : n_regions * q_tok_pad;
#define SOFT_CASE(D16_, DT_, ONES_) \
    if (d16 == D16_ && dt == DT_ && ones == ONES_) { if (launch_attn_region_soft<D16_, DT_, ONES_>(a, grid, s, wp, w_bstride, n_regions)) return -1; } else
    SOFT_CASE(1, 1, true) SOFT_CASE(2, 1, true) SOFT_CASE(2, 1, false) SOFT_CASE(3, 2, true) SOFT_CASE(4, 2, true) SOFT_CASE(4, 2, false)
    SOFT_CASE(5, 3, true) SOFT_CASE(6, 3, true) SOFT_CASE(6, 3, false) SOFT_CASE(8, 4, true) SOFT_CASE(8, 4, false)
    SOFT_CASE(10, 5, true) SOFT_CASE(10, 5, false)
    { cfgpp_set_error("attention_region_soft: no kernel instance for head dim %d", d); return -2; }
#undef SOFT_CASE
    CFGPP_HIP_CHECK(hipGetLastError());
    attn_note(9, d16, ones, 0);
    return 0;
}

}  // extern "C"
