// MSWNet baseline (the reference's Extended_Baseline_Comparison.py:479-548): what its MultiScaleBlock needs beyond the shared kernels.
//
// 1. MaxPool2d(3, stride 1, padding 1) (branch4's first layer, :490) over NHWC views:
//      runet_maxpool3s1_fwd   padding counts as -inf; winner byte k = dy * 3 + dx, the first maximum in row-major window order, a NaN wins over
//                             everything (ATen's CPU rule: `v > max || isnan(v)`)
//      runet_maxpool3s1_bwd   a GATHER: every dx element sums, in row-major order of the windows, the dy of those of its <= 9 covering windows
//                             whose winner byte points at it (no atomics, no scatter)
//
// 2. The multi-scale stem, enc1 = MultiScaleBlock(3, 64) on the strided NCHW image:
//      t = cat(conv1x1(x), conv3x3(x), conv5x5(x), conv1x1(maxpool3(x)))   16 channels each, 1728 multiply-adds per pixel
//      y = t * scale + shift (the four BatchNorms), e = relu(y)
//    recomputed per pixel from an image tile with a 2-pixel halo in LDS, so the 64-channel pre-BatchNorm tensor never touches HBM:
//      runet_ms_stem_stats       per-block (count, mean, M2) partials of t (exact two-pass form) for runet_bn_stats_finalize, one partials array
//                                per branch
//      runet_ms_stem_fwd         x, scale / shift -> e [n, h, w, 64]
//      runet_ms_stem_bwd_reduce  x, de -> the BatchNorm-backward sums (dgamma [64] | dbeta [64])
//      runet_ms_stem_bwd_apply   x, de, sums -> dt [n, h, w, 64], the gradient of the four convolutions' outputs
//    t and y come from ONE routine (branch_t / bn_pre: explicit FMAs in a fixed order) in all four kernels, so the backward's ReLU decision
//    (y > 0) is the forward's, bit for bit.  Weights in their physical (HWIO) layouts w1 [1][1][3][16], w3 [3][3][3][16], w5 [5][5][3][16],
//    w4 [1][1][3][16]; in LDS back to back (1728 floats) with the biases (64) and the per-channel vectors, read at wave-uniform addresses
//    (broadcasts).  A block owns an 8 x 32 pixel tile, a thread one pixel, looping over the four branches with 16 accumulators; a 32-lane half
//    of a wave reads 32 consecutive floats of one tile row at every tap: no bank conflicts.  Sums: in-wave butterfly, the block's four waves
//    in order through LDS, the blocks' partial rows in index order.  No float atomics; the block count depends on the shape only.
#include "runet_common.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;

// =============================================================================================================== 3x3 stride-1 max-pool
template <int V>
struct Vec;
template <>
struct Vec<1> {
    typedef float f;
    typedef unsigned char b;
};
template <>
struct Vec<4> {
    typedef f32x4 f;
    typedef unsigned int b;
};
template <int V>
__device__ __forceinline__ float lane_of(const typename Vec<V>::f& v, int e);
template <>
__device__ __forceinline__ float lane_of<1>(const float& v, int) { return v; }
template <>
__device__ __forceinline__ float lane_of<4>(const f32x4& v, int e) { return v[e]; }

template <int V>
__global__ __launch_bounds__(TPB) void mp3s1_fwd_kernel(const float* __restrict__ x, const int ldx, float* __restrict__ y, const int ldy,
                                                        unsigned char* __restrict__ idx, const long P, const int H, const int W, const int C) {
    const int G = C / V;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < P * G; i += (long)gridDim.x * TPB) {
        const long p = i / G;
        const int c = (int)(i - p * G) * V;
        const int rem = (int)(p % ((long)H * W));
        const int yy = rem / W, xx = rem - yy * W;
        float m[V];
        unsigned int k[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            m[e] = -INFINITY;
            k[e] = (yy == 0 ? 3u : 0u) + (xx == 0 ? 1u : 0u);      // ATen starts at the window's first valid element
        }
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int iy = yy + ky - 1, ix = xx + kx - 1;
                if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
                const typename Vec<V>::f v = *reinterpret_cast<const typename Vec<V>::f*>(x + (p + (long)(ky - 1) * W + (kx - 1)) * ldx + c);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float f = lane_of<V>(v, e);
                    if (f > m[e] || f != f) {
                        m[e] = f;
                        k[e] = (unsigned)(ky * 3 + kx);
                    }
                }
            }
#pragma unroll
        for (int e = 0; e < V; ++e) y[p * ldy + c + e] = m[e];
        if (idx) {
#pragma unroll
            for (int e = 0; e < V; ++e) idx[p * C + c + e] = (unsigned char)k[e];
        }
    }
}

template <int V>
__global__ __launch_bounds__(TPB) void mp3s1_bwd_kernel(const float* __restrict__ dy, const int lddy, const unsigned char* __restrict__ idx,
                                                        float* __restrict__ dx, const int lddx, const long P, const int H, const int W, const int C,
                                                        const int accumulate) {
    const int G = C / V;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < P * G; i += (long)gridDim.x * TPB) {
        const long p = i / G;
        const int c = (int)(i - p * G) * V;
        const int rem = (int)(p % ((long)H * W));
        const int yy = rem / W, xx = rem - yy * W;
        float s[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.f;
#pragma unroll
        for (int oy = -1; oy <= 1; ++oy)
#pragma unroll
            for (int ox = -1; ox <= 1; ++ox) {
                const int wy = yy + oy, wx = xx + ox;          // the window centred here covers (yy, xx) at position (1 - oy, 1 - ox)
                if (wy < 0 || wy >= H || wx < 0 || wx >= W) continue;
                const unsigned int kk = (unsigned)((1 - oy) * 3 + (1 - ox));
                const long q = p + (long)oy * W + ox;
                const typename Vec<V>::b bytes = *reinterpret_cast<const typename Vec<V>::b*>(idx + q * C + c);
                const typename Vec<V>::f g = *reinterpret_cast<const typename Vec<V>::f*>(dy + q * lddy + c);
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if ((((unsigned int)bytes >> (8 * e)) & 0xffu) == kk) s[e] += lane_of<V>(g, e);
            }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float* o = dx + p * lddx + c + e;
            *o = accumulate ? *o + s[e] : s[e];
        }
    }
}


// =============================================================================================================== multi-scale stem
constexpr int TH = 8, TW = 32;             // pixel tile of a block: thread t owns pixel (t / 32, t % 32)
constexpr int HALO = 2;
constexpr int IH = TH + 2 * HALO, IW = TW + 2 * HALO;
constexpr int CB = 16, NB = 4, CT = CB * NB;       // channels per branch, branches, channels of t
constexpr int NW1 = 3 * CB, NW3 = 27 * CB, NW5 = 75 * CB, NW = 2 * NW1 + NW3 + NW5;      // 1728

struct Src {
    const float* x;
    long sn, sc, sh, sw;
    int h, w, tiles_x, tiles_y;
};
struct Wts {
    const float *w1, *w3, *w5, *w4, *b1, *b3, *b5, *b4;
};
struct Smem {
    float w[NW];            // w1 | w3 | w5 | w4
    float bias[CT];
    float sc[CT], sh[CT], va[CT], vb[CT];      // scale, shift and two more per-channel vectors (mean / invstd, or the BatchNorm-backward coefficients)
    float img[3][IH][IW];   // the image tile with its halo; zero outside the image (the convolutions' padding)
};
struct Tile {
    int n, y0, x0, ty, tx;
    bool valid;
    long p;                 // pixel index over all images
    int cnt;                // pixels of the tile inside the image
};

__device__ __forceinline__ void fill(float* dst, const float* __restrict__ src, const int n) {
    for (int i = threadIdx.x; i < n; i += TPB) dst[i] = src[i];
}
__device__ __forceinline__ void load_weights(Smem& s, const Wts& k) {
    fill(s.w, k.w1, NW1);
    fill(s.w + NW1, k.w3, NW3);
    fill(s.w + NW1 + NW3, k.w5, NW5);
    fill(s.w + NW1 + NW3 + NW5, k.w4, NW1);
    fill(s.bias, k.b1, CB);
    fill(s.bias + CB, k.b3, CB);
    fill(s.bias + 2 * CB, k.b5, CB);
    fill(s.bias + 3 * CB, k.b4, CB);
}
__device__ __forceinline__ Tile load_tile(Smem& s, const Src& src) {
    Tile t;
    const int per = src.tiles_x * src.tiles_y;
    t.n = blockIdx.x / per;
    const int r = blockIdx.x - t.n * per;
    t.y0 = (r / src.tiles_x) * TH;
    t.x0 = (r % src.tiles_x) * TW;
    t.ty = threadIdx.x / TW;
    t.tx = threadIdx.x % TW;
    const int gy = t.y0 + t.ty, gx = t.x0 + t.tx;
    t.valid = gy < src.h && gx < src.w;
    t.p = ((long)t.n * src.h + gy) * src.w + gx;
    const int vh = src.h - t.y0 < TH ? src.h - t.y0 : TH, vw = src.w - t.x0 < TW ? src.w - t.x0 : TW;
    t.cnt = vh * vw;
    const float* base = src.x + (long)t.n * src.sn;
    for (int i = threadIdx.x; i < 3 * IH * IW; i += TPB) {
        const int ci = i / (IH * IW), q = i - ci * (IH * IW);
        const int ry = q / IW, rx = q - ry * IW;
        const int iy = t.y0 - HALO + ry, ix = t.x0 - HALO + rx;
        float v = 0.f;
        if (iy >= 0 && iy < src.h && ix >= 0 && ix < src.w) v = base[(long)ci * src.sc + (long)iy * src.sh + (long)ix * src.sw];
        s.img[ci][ry][rx] = v;
    }
    return t;
}
// the 3x3 stride-1 max-pool of the thread's pixel (padding = -inf: only taps inside the image take part; runet_maxpool3s1_fwd's rule)
__device__ __forceinline__ void pool3(const Smem& s, const Src& src, const Tile& t, float (&m)[3]) {
    const int gy = t.y0 + t.ty, gx = t.x0 + t.tx;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) m[ci] = -INFINITY;
#pragma unroll
    for (int ky = -1; ky <= 1; ++ky)
#pragma unroll
        for (int kx = -1; kx <= 1; ++kx) {
            const bool in = gy + ky >= 0 && gy + ky < src.h && gx + kx >= 0 && gx + kx < src.w;
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const float v = s.img[ci][t.ty + HALO + ky][t.tx + HALO + kx];
                if (in && (v > m[ci] || v != v)) m[ci] = v;
            }
        }
    if (!t.valid) m[0] = m[1] = m[2] = 0.f;       // a thread outside the image: no -inf into the (unused) arithmetic
}

template <int B>
struct Br {
    static constexpr int K = B == 1 ? 3 : B == 2 ? 5 : 1;
    static constexpr int WOFF = B == 0 ? 0 : B == 1 ? NW1 : B == 2 ? NW1 + NW3 : NW1 + NW3 + NW5;
};
// t[0 : 16) of branch B at the thread's pixel: bias, then the taps in (ky, kx, ci) order, one FMA each - the ONE definition of t
template <int B>
__device__ __forceinline__ void branch_t(const Smem& s, const Tile& tl, const float (&pool)[3], float (&t)[CB]) {
    constexpr int K = Br<B>::K, R = K / 2;
#pragma unroll
    for (int j = 0; j < CB; ++j) t[j] = s.bias[B * CB + j];
#pragma unroll 1
    for (int ky = 0; ky < K; ++ky)      // rolled: a fully unrolled 5x5 lets the scheduler hoist hundreds of LDS reads and spill
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const float v = B == 3 ? pool[ci] : s.img[ci][tl.ty + HALO - R + ky][tl.tx + HALO - R + kx];
                const float* wr = s.w + Br<B>::WOFF + ((ky * K + kx) * 3 + ci) * CB;
#pragma unroll
                for (int j = 0; j < CB; ++j) t[j] = __builtin_fmaf(wr[j], v, t[j]);
            }
}

// acc[N] summed over the block in a fixed order -> dst[0 : N) (LDS or global); red: LDS [WAVES][N].  Ends with a barrier: red and dst may be
// read / reused at once.
template <int N>
__device__ __forceinline__ void block_sum(const float (&acc)[N], float* red, float* dst) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float t = wave_sum(acc[j]);
        if (lane == 0) red[wave * N + j] = t;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < N; j += TPB) {
        float t = red[j];
        for (int wv = 1; wv < WAVES; ++wv) t += red[wv * N + j];
        dst[j] = t;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- statistics
// part[branch][block][16][3] = (count, mean, M2) of t over the block's pixels: the block's mean, then the squares of the deviations from it
template <int B>
__device__ __forceinline__ void stats_branch(const Smem& s, const Tile& tl, const float (&pool)[3], float* red, float* bsum, float* bm2,
                                             float* __restrict__ part, const int nparts) {
    float t[CB], acc[CB];
    branch_t<B>(s, tl, pool, t);
#pragma unroll
    for (int j = 0; j < CB; ++j) acc[j] = tl.valid ? t[j] : 0.f;
    block_sum<CB>(acc, red, bsum);
#pragma unroll
    for (int j = 0; j < CB; ++j) {
        const float d = t[j] - bsum[j] / (float)tl.cnt;
        acc[j] = tl.valid ? d * d : 0.f;
    }
    block_sum<CB>(acc, red, bm2);
    if (threadIdx.x < CB) {
        float* o = part + (((long)B * nparts + blockIdx.x) * CB + threadIdx.x) * 3;
        o[0] = (float)tl.cnt;
        o[1] = bsum[threadIdx.x] / (float)tl.cnt;
        o[2] = bm2[threadIdx.x];
    }
    __syncthreads();        // bsum / bm2 are rewritten by the next branch
}
__global__ __launch_bounds__(TPB) void ms_stats_kernel(const Src src, const Wts k, float* __restrict__ part, const int nparts) {
    __shared__ Smem s;
    __shared__ float red[WAVES * CB], bsum[CB], bm2[CB];
    load_weights(s, k);
    const Tile tl = load_tile(s, src);
    __syncthreads();
    float pool[3];
    pool3(s, src, tl, pool);
    stats_branch<0>(s, tl, pool, red, bsum, bm2, part, nparts);
    stats_branch<1>(s, tl, pool, red, bsum, bm2, part, nparts);
    stats_branch<2>(s, tl, pool, red, bsum, bm2, part, nparts);
    stats_branch<3>(s, tl, pool, red, bsum, bm2, part, nparts);
}

// ---------------------------------------------------------------------------------------------------------------- forward
template <int B>
__device__ __forceinline__ void fwd_branch(const Smem& s, const Tile& tl, const float (&pool)[3], float* __restrict__ e, const int lde) {
    float t[CB];
    branch_t<B>(s, tl, pool, t);
    if (!tl.valid) return;
    float* o = e + tl.p * lde + B * CB;
#pragma unroll
    for (int q = 0; q < CB / 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(bn_pre(t[4 * q + r], s.sc[B * CB + 4 * q + r], s.sh[B * CB + 4 * q + r]), 0.f);
        *reinterpret_cast<f32x4*>(o + 4 * q) = v;
    }
}
__global__ __launch_bounds__(TPB) void ms_fwd_kernel(const Src src, const Wts k, const float* __restrict__ scale, const float* __restrict__ shift,
                                                     float* __restrict__ e, const int lde) {
    __shared__ Smem s;
    load_weights(s, k);
    fill(s.sc, scale, CT);
    fill(s.sh, shift, CT);
    const Tile tl = load_tile(s, src);
    __syncthreads();
    float pool[3];
    pool3(s, src, tl, pool);
    fwd_branch<0>(s, tl, pool, e, lde);
    fwd_branch<1>(s, tl, pool, e, lde);
    fwd_branch<2>(s, tl, pool, e, lde);
    fwd_branch<3>(s, tl, pool, e, lde);
}

// ---------------------------------------------------------------------------------------------------------------- backward
// g = de masked by the forward's ReLU decision (y > 0), for the thread's 16 channels of branch B
template <int B>
__device__ __forceinline__ void masked_grad(const Smem& s, const Tile& tl, const float (&t)[CB], const float* __restrict__ de, const int ldde,
                                            float (&g)[CB]) {
#pragma unroll
    for (int q = 0; q < CB / 4; ++q) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (tl.valid) v = *reinterpret_cast<const f32x4*>(de + tl.p * ldde + B * CB + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 4 * q + r;
            g[j] = bn_pre(t[j], s.sc[B * CB + j], s.sh[B * CB + j]) > 0.f ? v[r] : 0.f;
        }
    }
}
// row[128] of the block = sum g * xhat [64] | sum g [64]   (va = mean, vb = invstd)
template <int B>
__device__ __forceinline__ void reduce_branch(const Smem& s, const Tile& tl, const float (&pool)[3], const float* __restrict__ de, const int ldde,
                                              float* red, float* __restrict__ row) {
    float t[CB], g[CB], a[CB], b[CB];
    branch_t<B>(s, tl, pool, t);
    masked_grad<B>(s, tl, t, de, ldde, g);
#pragma unroll
    for (int j = 0; j < CB; ++j) {
        a[j] = g[j] * ((t[j] - s.va[B * CB + j]) * s.vb[B * CB + j]);      // g is 0 for a thread outside the image
        b[j] = g[j];
    }
    block_sum<CB>(a, red, row + B * CB);
    block_sum<CB>(b, red, row + CT + B * CB);
}
__global__ __launch_bounds__(TPB) void ms_bwd_reduce_kernel(const Src src, const Wts k, const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ de, const int ldde, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, float* __restrict__ part) {
    __shared__ Smem s;
    __shared__ float red[WAVES * CB];
    load_weights(s, k);
    fill(s.sc, scale, CT);
    fill(s.sh, shift, CT);
    fill(s.va, mean, CT);
    fill(s.vb, invstd, CT);
    const Tile tl = load_tile(s, src);
    __syncthreads();
    float pool[3];
    pool3(s, src, tl, pool);
    float* row = part + (long)blockIdx.x * (2 * CT);
    reduce_branch<0>(s, tl, pool, de, ldde, red, row);
    reduce_branch<1>(s, tl, pool, de, ldde, red, row);
    reduce_branch<2>(s, tl, pool, de, ldde, red, row);
    reduce_branch<3>(s, tl, pool, de, ldde, red, row);
}

// dt = runet_bn_bwd_apply's formula on g (va = ca, vb = cb of bn_bwd_coef)
template <int B>
__device__ __forceinline__ void apply_branch(const Smem& s, const Tile& tl, const float (&pool)[3], const float* __restrict__ de, const int ldde,
                                             float* __restrict__ dt, const int lddt) {
    float t[CB], g[CB];
    branch_t<B>(s, tl, pool, t);
    masked_grad<B>(s, tl, t, de, ldde, g);
    if (!tl.valid) return;
    float* o = dt + tl.p * lddt + B * CB;
#pragma unroll
    for (int q = 0; q < CB / 4; ++q) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = B * CB + 4 * q + r;
            v[r] = bn_bwd_dx(g[4 * q + r], s.sc[j], t[4 * q + r], s.va[j], s.vb[j]);
        }
        *reinterpret_cast<f32x4*>(o + 4 * q) = v;
    }
}
__global__ __launch_bounds__(TPB) void ms_bwd_apply_kernel(const Src src, const Wts k, const float* __restrict__ scale, const float* __restrict__ shift,
                                                           const float* __restrict__ de, const int ldde, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ sums, const float inv_m,
                                                           float* __restrict__ dt, const int lddt) {
    __shared__ Smem s;
    load_weights(s, k);
    fill(s.sc, scale, CT);
    fill(s.sh, shift, CT);
    if (threadIdx.x < CT) {
        const int j = threadIdx.x;
        float ca, cb;
        bn_bwd_coef(scale[j], mean[j], invstd[j], sums[j], sums[CT + j], inv_m, ca, cb);
        s.va[j] = ca;
        s.vb[j] = cb;
    }
    const Tile tl = load_tile(s, src);
    __syncthreads();
    float pool[3];
    pool3(s, src, tl, pool);
    apply_branch<0>(s, tl, pool, de, ldde, dt, lddt);
    apply_branch<1>(s, tl, pool, de, ldde, dt, lddt);
    apply_branch<2>(s, tl, pool, de, ldde, dt, lddt);
    apply_branch<3>(s, tl, pool, de, ldde, dt, lddt);
}

inline long n_tiles(int n, int h, int w) { return (long)n * cdiv(h, TH) * cdiv(w, TW); }
inline bool shape_ok(int n, int h, int w) {
    return n > 0 && h > 0 && w > 0 && (long)h * w <= 0x7fffffffL && n_tiles(n, h, w) <= 0x7fffffffL / (NB * CB * 3);
}
inline Src make_src(const float* x, long sn, long sc, long sh, long sw, int h, int w) { return Src{x, sn, sc, sh, sw, h, w, cdiv(w, TW), cdiv(h, TH)}; }
}  // namespace

#define MS_WTS_OK (w1 && w3 && w5 && w4 && b1 && b3 && b5 && b4)

extern "C" int runet_maxpool3s1_fwd(const float* x, int ldx, float* y, int ldy, unsigned char* idx, int n_img, int h, int w, int c, void* stream) {
    RUNET_REQUIRE(x && y, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w > 0 && c > 0 && (long)h * w <= 0x7fffffffL, "empty shape");
    RUNET_REQUIRE(ldx >= c && ldy >= c, "a pixel stride below the channel count");
    const long P = (long)n_img * h * w;
    if (c % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && RUNET_ALIGNED16(x) && RUNET_ALIGNED16(y))
        hipLaunchKernelGGL(mp3s1_fwd_kernel<4>, dim3(ew_grid(P * (c / 4), 16384)), dim3(TPB), 0, (hipStream_t)stream, x, ldx, y, ldy, idx, P, h, w, c);
    else
        hipLaunchKernelGGL(mp3s1_fwd_kernel<1>, dim3(ew_grid(P * c, 16384)), dim3(TPB), 0, (hipStream_t)stream, x, ldx, y, ldy, idx, P, h, w, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_maxpool3s1_bwd(const float* dy, int lddy, const unsigned char* idx, float* dx, int lddx, int n_img, int h, int w, int c,
                                    int accumulate, void* stream) {
    RUNET_REQUIRE(dy && idx && dx, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w > 0 && c > 0 && (long)h * w <= 0x7fffffffL, "empty shape");
    RUNET_REQUIRE(lddy >= c && lddx >= c, "a pixel stride below the channel count");
    const long P = (long)n_img * h * w;
    if (c % 4 == 0 && lddy % 4 == 0 && RUNET_ALIGNED16(dy) && ((uintptr_t)idx % 4) == 0)
        hipLaunchKernelGGL(mp3s1_bwd_kernel<4>, dim3(ew_grid(P * (c / 4), 16384)), dim3(TPB), 0, (hipStream_t)stream, dy, lddy, idx, dx, lddx, P, h, w, c,
                           accumulate);
    else
        hipLaunchKernelGGL(mp3s1_bwd_kernel<1>, dim3(ew_grid(P * c, 16384)), dim3(TPB), 0, (hipStream_t)stream, dy, lddy, idx, dx, lddx, P, h, w, c, accumulate);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_ms_stem_parts(int n_img, int h, int w_) {
    if (!shape_ok(n_img, h, w_)) return -1;
    return (int)n_tiles(n_img, h, w_);
}

extern "C" long runet_ms_stem_workspace_floats(int n_img, int h, int w_) {
    if (!shape_ok(n_img, h, w_)) return -1;
    return n_tiles(n_img, h, w_) * (2 * CT);
}

extern "C" int runet_ms_stem_stats(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* w3,
                                   const float* w5, const float* w4, const float* b1, const float* b3, const float* b5, const float* b4, float* part,
                                   long part_floats, void* stream) {
    RUNET_REQUIRE(x && MS_WTS_OK && part, "null pointer");
    RUNET_REQUIRE(shape_ok(n_img, h, w_), "empty shape");
    const long nb = n_tiles(n_img, h, w_);
    RUNET_REQUIRE(part_floats >= nb * NB * CB * 3, "partials buffer too small (4 branches x runet_ms_stem_parts rows of 16 x 3 floats)");
    hipLaunchKernelGGL(ms_stats_kernel, dim3((unsigned)nb), dim3(TPB), 0, (hipStream_t)stream, make_src(x, sn, sc, sh, sw, h, w_),
                       Wts{w1, w3, w5, w4, b1, b3, b5, b4}, part, (int)nb);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_ms_stem_fwd(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* w3,
                                 const float* w5, const float* w4, const float* b1, const float* b3, const float* b5, const float* b4,
                                 const float* scale, const float* shift, float* e, int lde, void* stream) {
    RUNET_REQUIRE(x && MS_WTS_OK && scale && shift && e, "null pointer");
    RUNET_REQUIRE(shape_ok(n_img, h, w_), "empty shape");
    RUNET_REQUIRE(lde >= CT && lde % 4 == 0 && RUNET_ALIGNED16(e), "the output's pixel stride must be a multiple of 4 floats, at least 64, its pointer 16-byte aligned");
    hipLaunchKernelGGL(ms_fwd_kernel, dim3((unsigned)n_tiles(n_img, h, w_)), dim3(TPB), 0, (hipStream_t)stream, make_src(x, sn, sc, sh, sw, h, w_),
                       Wts{w1, w3, w5, w4, b1, b3, b5, b4}, scale, shift, e, lde);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_ms_stem_bwd_reduce(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* w3,
                                        const float* w5, const float* w4, const float* b1, const float* b3, const float* b5, const float* b4,
                                        const float* scale, const float* shift, const float* de, int ldde, const float* mean, const float* invstd,
                                        float* workspace, long workspace_floats, float* sums, void* stream) {
    RUNET_REQUIRE(x && MS_WTS_OK && scale && shift && de && mean && invstd && workspace && sums, "null pointer");
    RUNET_REQUIRE(shape_ok(n_img, h, w_), "empty shape");
    RUNET_REQUIRE(ldde >= CT && ldde % 4 == 0 && RUNET_ALIGNED16(de), "the gradient's pixel stride must be a multiple of 4 floats, at least 64, its pointer 16-byte aligned");
    const long nb = n_tiles(n_img, h, w_);
    RUNET_REQUIRE(workspace_floats >= nb * 2 * CT, "workspace too small (runet_ms_stem_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ms_bwd_reduce_kernel, dim3((unsigned)nb), dim3(TPB), 0, st, make_src(x, sn, sc, sh, sw, h, w_),
                       Wts{w1, w3, w5, w4, b1, b3, b5, b4}, scale, shift, de, ldde, mean, invstd, workspace);
    sum_parts<16>(workspace, (int)nb, 2 * CT, sums, st);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_ms_stem_bwd_apply(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* w3,
                                       const float* w5, const float* w4, const float* b1, const float* b3, const float* b5, const float* b4,
                                       const float* scale, const float* shift, const float* de, int ldde, const float* mean, const float* invstd,
                                       const float* sums, long m_total, float* dt, int lddt, void* stream) {
    RUNET_REQUIRE(x && MS_WTS_OK && scale && shift && de && mean && invstd && sums && dt, "null pointer");
    RUNET_REQUIRE(shape_ok(n_img, h, w_), "empty shape");
    RUNET_REQUIRE(ldde >= CT && ldde % 4 == 0 && RUNET_ALIGNED16(de), "the gradient's pixel stride must be a multiple of 4 floats, at least 64, its pointer 16-byte aligned");
    RUNET_REQUIRE(lddt >= CT && lddt % 4 == 0 && RUNET_ALIGNED16(dt), "the output's pixel stride must be a multiple of 4 floats, at least 64, its pointer 16-byte aligned");
    const float inv_m = 1.0f / (float)(m_total > 0 ? m_total : (long)n_img * h * w_);
    hipLaunchKernelGGL(ms_bwd_apply_kernel, dim3((unsigned)n_tiles(n_img, h, w_)), dim3(TPB), 0, (hipStream_t)stream, make_src(x, sn, sc, sh, sw, h, w_),
                       Wts{w1, w3, w5, w4, b1, b3, b5, b4}, scale, shift, de, ldde, mean, invstd, sums, inv_m, dt, lddt);
    RUNET_CHECK_LAUNCH();
}
