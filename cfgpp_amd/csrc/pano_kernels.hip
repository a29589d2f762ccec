// MultiDiffusion panoramas (include/cfgpp_panorama.h): the window gather and the fused per-step kernel - every covering view's DDIM /
// DDIM-CFG++ update, the overlap average and the scatter of the new latent into the views' UNet input slots, in one launch.
//
// Rounding contract: the per-view update is step_kernels.hip's (step_math.h: ddim_update_h, one definition); the sum over the covering
// views runs in ascending view index, one fp32 rounding per add, and the mean is an IEEE division by float(count).  This file is built
// with -ffp-contract=off.
//
// Work split: a thread owns FOUR consecutive panorama columns of one (chain, channel, row).  stride, w and Wp are multiples of 4, so
// the four columns share their covering views and never straddle a window edge or the wrap: every access is one 16-byte vector
// (8 bytes of fp16 eps).  The covering views follow from the coordinates:
//     rows     iy in [floor((y - h) / stride) + 1, y / stride]  clipped to [0, nbh)
//     columns  ix in [floor((x - w) / stride) + 1, x / stride]  clipped to [0, nbw), and with circular padding the negative ix of
//              that range are the views nbw + ix, which come AFTER the non-negative ones in view order
// Each element of z_views is written by exactly one thread (its panorama element's owner): no conflicts, no atomics.
//
// HBM traffic at count covering views per element: 4 B z in + count * (2 + 2) B eps in + 4 + 4 B out + count * 4 B scatter.
#include "common.h"
#include "step_math.h"
#include "../../include/cfgpp_panorama.h"

namespace {

struct Geom {
    int B, C, Hp, Wp, h, w, stride, circ, Vc, nbh, nbw;
};

// floor(a / s) + 1 for a that may be negative (s > 0)
__host__ __device__ __forceinline__ int floor_div_p1(int a, int s) {
    return a >= 0 ? a / s + 1 : -((-a + s - 1) / s) + 1;
}

// the covering views of panorama position (y, x): rows iy0 .. iy1; columns a0 .. a1 and then (circular only) b0 .. b1
// (__host__ too: plain index arithmetic, so a host program can walk it)
struct Cover {
    int iy0, iy1, a0, a1, b0, b1;
};
__host__ __device__ __forceinline__ Cover cover_of(const Geom& g, int y, int x) {
    Cover c;
    c.iy0 = max(0, floor_div_p1(y - g.h, g.stride));
    c.iy1 = min(g.nbh - 1, y / g.stride);
    const int lo = floor_div_p1(x - g.w, g.stride);
    c.a0 = max(0, lo);
    c.a1 = min(g.nbw - 1, x / g.stride);
    c.b0 = 0; c.b1 = -1;
    if (g.circ && lo < 0) { c.b0 = g.nbw + lo; c.b1 = g.nbw - 1; }      // w <= Wp: b0 > a1, no view twice
    return c;
}

template <typename F>
__host__ __device__ __forceinline__ void for_each_view(const Geom& g, const Cover& c, int y, int x, F&& f) {
    for (int iy = c.iy0; iy <= c.iy1; ++iy) {
        const int ly = y - iy * g.stride;
        for (int ix = c.a0; ix <= c.a1; ++ix) f(iy * g.nbw + ix, ly, x - ix * g.stride);
        for (int ix = c.b0; ix <= c.b1; ++ix) f(iy * g.nbw + ix, ly, x - ix * g.stride + g.Wp);
    }
}

__global__ void __launch_bounds__(256)
views_gather_kernel(Geom g, const float* __restrict__ z_pano, float* __restrict__ z_views, long n4) {
    const int w4 = g.w / 4;
    const long tstride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += tstride) {
        long r = i;
        const int lx = (int)(r % w4) * 4; r /= w4;
        const int ly = (int)(r % g.h); r /= g.h;
        const int c = (int)(r % g.C); r /= g.C;
        const int b = (int)(r % g.B);
        const int v = (int)(r / g.B);
        const int y = (v / g.nbw) * g.stride + ly;
        int x = (v % g.nbw) * g.stride + lx;
        if (x >= g.Wp) x -= g.Wp;                                          // circular only: x0 < Wp, lx < w <= Wp
        const long src = (((long)b * g.C + c) * g.Hp + y) * g.Wp + x;
        reinterpret_cast<float4*>(z_views)[i] = *reinterpret_cast<const float4*>(z_pano + src);
    }
}

__global__ void __launch_bounds__(256)
ddim_step_views_kernel(Geom g, float* __restrict__ z_pano, float* __restrict__ z0t_pano, float* __restrict__ z_views,
                       const half_t* __restrict__ eps, float lam, float c1, float c2, float c3, float c4, int tweedie_uc,
                       int renoise_uc, long n4) {
    const int W4 = g.Wp / 4;
    const long win = (long)g.h * g.w;                       // elements of one window channel
    const long half_rows = (long)g.Vc * g.B;                // uc rows of a chunk; the c rows follow
    const long tstride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += tstride) {
        long r = i;
        const int x = (int)(r % W4) * 4; r /= W4;
        const int y = (int)(r % g.Hp); r /= g.Hp;
        const int c = (int)(r % g.C);
        const int b = (int)(r / g.C);
        const float4 zv = reinterpret_cast<const float4*>(z_pano)[i];
        const float zi[4] = {zv.x, zv.y, zv.z, zv.w};
        const Cover cov = cover_of(g, y, x);
        float s0[4] = {0.f, 0.f, 0.f, 0.f}, sn[4] = {0.f, 0.f, 0.f, 0.f};
        int count = 0;
        for_each_view(g, cov, y, x, [&](int v, int ly, int lx) {
            const int k = v / g.Vc, vi = v - k * g.Vc;
            const long row_uc = (long)k * 2 * half_rows + (long)vi * g.B + b;
            const long off = (long)ly * g.w + lx;
            const half4_t ua = *reinterpret_cast<const half4_t*>(eps + (row_uc * g.C + c) * win + off);
            const half4_t ub = *reinterpret_cast<const half4_t*>(eps + ((row_uc + half_rows) * g.C + c) * win + off);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float z0, zn;
                ddim_update_h(zi[j], (float)ua[j], (float)ub[j], lam, c1, c2, c3, c4, tweedie_uc, renoise_uc, z0, zn);
                s0[j] = count ? __fadd_rn(s0[j], z0) : z0;
                sn[j] = count ? __fadd_rn(sn[j], zn) : zn;
            }
            ++count;
        });
        const float cnt = (float)count;                     // >= 1: the geometry leaves nothing uncovered
        float o0[4], on[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { o0[j] = __fdiv_rn(s0[j], cnt); on[j] = __fdiv_rn(sn[j], cnt); }
        const float4 znew = make_float4(on[0], on[1], on[2], on[3]);
        reinterpret_cast<float4*>(z0t_pano)[i] = make_float4(o0[0], o0[1], o0[2], o0[3]);
        reinterpret_cast<float4*>(z_pano)[i] = znew;
        for_each_view(g, cov, y, x, [&](int v, int ly, int lx) {
            const long dst = ((((long)v * g.B + b) * g.C + c) * g.h + ly) * g.w + lx;
            *reinterpret_cast<float4*>(z_views + dst) = znew;
        });
    }
}

inline int grid_for(long items) {
    long gr = (items + 255) / 256;
    if (gr > 2048) gr = 2048;
    if (gr < 1) gr = 1;
    return (int)gr;
}

// every refusal of include/cfgpp_panorama.h; fills the derived view counts
int make_geom(const cfgpp_pano_views* p, const char* who, Geom& g) {
    CFGPP_REQUIRE(p, "%s: null views", who);
    CFGPP_REQUIRE(p->B >= 1 && p->C >= 1 && p->h >= 1 && p->w >= 1 && p->stride >= 1 && p->chunk_views >= 1,
                  "%s: B=%d C=%d h=%d w=%d stride=%d chunk_views=%d must all be positive", who, p->B, p->C, p->h, p->w, p->stride, p->chunk_views);
    CFGPP_REQUIRE(p->Hp >= p->h && p->Wp >= p->w, "%s: the panorama %d x %d is smaller than the window %d x %d", who, p->Hp, p->Wp, p->h, p->w);
    CFGPP_REQUIRE(p->stride % 4 == 0 && p->w % 4 == 0 && p->Wp % 4 == 0,
                  "%s: stride=%d, w=%d and Wp=%d must be multiples of 4 (16-byte vectors)", who, p->stride, p->w, p->Wp);
    CFGPP_REQUIRE(p->stride <= p->h && p->stride <= p->w, "%s: stride=%d exceeds the window %d x %d", who, p->stride, p->h, p->w);
    CFGPP_REQUIRE((p->Hp - p->h) % p->stride == 0, "%s: (Hp - h) = %d is not a multiple of stride=%d", who, p->Hp - p->h, p->stride);
    const bool circ = p->circular != 0 && p->Wp > p->w;       // Wp == w is one column of views that covers everything: no wrap
    if (p->circular)
        CFGPP_REQUIRE(p->Wp % p->stride == 0, "%s: circular, and Wp=%d is not a multiple of stride=%d", who, p->Wp, p->stride);
    else
        CFGPP_REQUIRE((p->Wp - p->w) % p->stride == 0, "%s: (Wp - w) = %d is not a multiple of stride=%d", who, p->Wp - p->w, p->stride);
    g.B = p->B; g.C = p->C; g.Hp = p->Hp; g.Wp = p->Wp; g.h = p->h; g.w = p->w; g.stride = p->stride; g.circ = circ ? 1 : 0;
    g.Vc = p->chunk_views;
    g.nbh = p->Hp > p->h ? (p->Hp - p->h) / p->stride + 1 : 1;
    g.nbw = p->Wp > p->w ? (circ ? p->Wp / p->stride : (p->Wp - p->w) / p->stride + 1) : 1;
    const long V = (long)g.nbh * g.nbw;
    CFGPP_REQUIRE(V % g.Vc == 0, "%s: chunk_views=%d does not divide the %ld views", who, g.Vc, V);
    CFGPP_REQUIRE(V * p->B * p->C * p->h * p->w < (1L << 40), "%s: %ld views are too many", who, V);
    return 0;
}

}  // namespace

extern "C" {

int cfgpp_views_gather(const cfgpp_pano_views* views, const void* z_pano, void* z_views, void* stream) {
    Geom g;
    if (int rc = make_geom(views, "cfgpp_views_gather", g)) return rc;
    CFGPP_REQUIRE(z_pano && z_views, "cfgpp_views_gather: null pointer");
    const long n4 = (long)g.nbh * g.nbw * g.B * g.C * g.h * (g.w / 4);
    hipLaunchKernelGGL(views_gather_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, g, (const float*)z_pano,
                       (float*)z_views, n4);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

int cfgpp_step_ddim_views(const cfgpp_pano_views* views, void* z_pano, void* z0t_pano, void* z_views, const void* eps, float lam,
                          float c1, float c2, float c3, float c4, int tweedie_uc, int renoise_uc, void* stream) {
    Geom g;
    if (int rc = make_geom(views, "cfgpp_step_ddim_views", g)) return rc;
    CFGPP_REQUIRE(z_pano && z0t_pano && z_views && eps, "cfgpp_step_ddim_views: null pointer");
    const long n4 = (long)g.B * g.C * g.Hp * (g.Wp / 4);
    hipLaunchKernelGGL(ddim_step_views_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, g, (float*)z_pano,
                       (float*)z0t_pano, (float*)z_views, (const half_t*)eps, lam, c1, c2, c3, c4, tweedie_uc, renoise_uc, n4);
    CFGPP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
