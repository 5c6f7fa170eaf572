// WaterNet baseline (the reference's Extended_Baseline_Comparison.py:378-473): its front end, WaterIndexModule (:378-393) + torch.cat (:458),
//   Conv2d(3, 16, 1) -> BatchNorm2d(16) -> ReLU -> Conv2d(16, 4, 1) -> Sigmoid, then cat([x, idx]),
// as four streaming kernels over the RGB image.  The chain is 112 multiply-adds per pixel on 3 input floats, so every 16-channel tensor of the
// reference's order (the 1x1 convolution's output, the activation, their gradients) is recomputed from the pixel in registers and never
// touches HBM:
//   runet_water_index_stats       z = W1 x + b1 per pixel -> per-block (count, mean, M2) partials for runet_bn_stats_finalize
//   runet_water_index_fwd         x, scale / shift -> the 8-channel NHWC row [R, G, B, s0..s3, 0] enc1's first convolution reads
//   runet_water_index_bwd_reduce  g (gradient of channels 3..6) -> dW2, db2 and the BatchNorm-backward sums (dgamma | dbeta)
//   runet_water_index_bwd_apply   the BatchNorm-backward dz -> dW1, db1 (no input gradient: the input is the image)
// Notation: z = W1 x + b1 (16), y = z * scale + shift, a = relu(y), u = W2 a + b2 (4), s = sigmoid(u).  z and y are evaluated by the same
// explicit FMAs in all four kernels, so the backward's ReLU decision (y > 0) is the forward's, bit for bit.
// Weights in their physical (HWIO) layouts: w1 [3][16], w2 [16][4]; the gradients come back in the same layouts.
// A block owns PPB consecutive pixels (pixel index = (n * h + y) * w + x), a thread every TPB-th of them: neighbouring lanes read neighbouring
// addresses of each colour plane.  Sums: per-thread serial, in-wave butterfly, the block's four waves in order through LDS, the blocks'
// partial rows in index order (sum_parts<16> of runet_common.h).  No float atomics; the block count depends on the shape only: bitwise reproducible.
#include "runet_common.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int PPT = 8;                 // pixels per thread of the reducing kernels
constexpr int PPB = TPB * PPT;         // pixels per block
constexpr int C1 = 16, C2 = 4;
constexpr int W_RED = 2 * C1 + C1 * C2 + C2;      // bwd_reduce: dgamma [16] | dbeta [16] | dW2 [16][4] | db2 [4]
constexpr int W_APP = 3 * C1 + C1;                // bwd_apply:  dW1 [3][16] | db1 [16]

// the NCHW input through its four strides (in floats)
struct Src {
    const float* x;
    long sn, sc, sh, sw;
    int hw, w;
};
__device__ __forceinline__ void load_rgb(const Src& s, const long p, float (&v)[3]) {
    const long n = p / s.hw;
    const int rem = (int)(p - n * s.hw);
    const int y = rem / s.w, xx = rem - y * s.w;
    const float* b = s.x + n * s.sn + (long)y * s.sh + (long)xx * s.sw;
    v[0] = b[0]; v[1] = b[s.sc]; v[2] = b[2 * s.sc];
}

// coefficients of one launch in LDS (read with uniform addresses: broadcasts)
struct Coef {
    float w1[3 * C1], b1[C1], sc[C1], sh[C1], w2[C1 * C2], b2[C2], mu[C1], is[C1], ca[C1], cb[C1];
};
__device__ __forceinline__ void fill(float* dst, const float* __restrict__ src, const int n) {
    for (int i = threadIdx.x; i < n; i += TPB) dst[i] = src[i];
}

__device__ __forceinline__ void conv1(const Coef& k, const float (&v)[3], float (&z)[C1]) {
#pragma unroll
    for (int j = 0; j < C1; ++j)
        z[j] = __builtin_fmaf(k.w1[2 * C1 + j], v[2], __builtin_fmaf(k.w1[C1 + j], v[1], __builtin_fmaf(k.w1[j], v[0], k.b1[j])));
}
// y = BatchNorm(z), s = sigmoid(W2 relu(y) + b2)
__device__ __forceinline__ void tail(const Coef& k, const float (&z)[C1], float (&y)[C1], float (&s)[C2]) {
    float u[C2];
#pragma unroll
    for (int q = 0; q < C2; ++q) u[q] = k.b2[q];
#pragma unroll
    for (int j = 0; j < C1; ++j) {
        y[j] = bn_pre(z[j], k.sc[j], k.sh[j]);
        const float a = fmaxf(y[j], 0.f);
#pragma unroll
        for (int q = 0; q < C2; ++q) u[q] = __builtin_fmaf(k.w2[j * C2 + q], a, u[q]);
    }
#pragma unroll
    for (int q = 0; q < C2; ++q) s[q] = sigmoidf_(u[q]);
}
// da = W2^T (g * s * (1 - s)), masked by the ReLU decision; du is returned for the caller's own sums
__device__ __forceinline__ void back_to_a(const Coef& k, const float (&y)[C1], const float (&s)[C2], const float (&g)[C2], float (&du)[C2],
                                          float (&da)[C1]) {
#pragma unroll
    for (int q = 0; q < C2; ++q) du[q] = g[q] * s[q] * (1.f - s[q]);
#pragma unroll
    for (int j = 0; j < C1; ++j) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < C2; ++q) t = __builtin_fmaf(k.w2[j * C2 + q], du[q], t);
        da[j] = y[j] > 0.f ? t : 0.f;
    }
}

// acc[N] summed over the block in a fixed order -> row[0 : N); red: LDS [WAVES][N]
template <int N>
__device__ __forceinline__ void block_sum_store(float (&acc)[N], float* red, float* __restrict__ row) {
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
        row[j] = t;
    }
}

// ------------------------------------------------------------------------------------------------------------------ statistics
// Two passes over the block's pixels, which stay in registers: the block's mean of z, then the squares of the deviations from it (the exact
// two-pass form; nothing is derived from the input's covariance).  part[block][16][3] = (count, mean, M2).
__global__ __launch_bounds__(TPB) void wi_stats_kernel(const Src src, const long P, const float* __restrict__ w1, const float* __restrict__ b1,
                                                       float* __restrict__ part) {
    __shared__ Coef k;
    __shared__ float red[WAVES * C1];
    __shared__ float bmean[C1], bm2[C1];
    fill(k.w1, w1, 3 * C1);
    fill(k.b1, b1, C1);
    const long p0 = (long)blockIdx.x * PPB;
    const int cnt = (int)(P - p0 < PPB ? P - p0 : PPB);
    float v[PPT][3];
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int o = i * TPB + threadIdx.x;
        if (o < cnt) load_rgb(src, p0 + o, v[i]);
        else v[i][0] = v[i][1] = v[i][2] = 0.f;
    }
    __syncthreads();
    float acc[C1], z[C1];
#pragma unroll
    for (int j = 0; j < C1; ++j) acc[j] = 0.f;
#pragma unroll
    for (int i = 0; i < PPT; ++i)
        if (i * TPB + (int)threadIdx.x < cnt) {
            conv1(k, v[i], z);
#pragma unroll
            for (int j = 0; j < C1; ++j) acc[j] += z[j];
        }
    block_sum_store<C1>(acc, red, bmean);
    __syncthreads();
    float mu[C1];
#pragma unroll
    for (int j = 0; j < C1; ++j) {
        mu[j] = bmean[j] / (float)cnt;
        acc[j] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < PPT; ++i)
        if (i * TPB + (int)threadIdx.x < cnt) {
            conv1(k, v[i], z);
#pragma unroll
            for (int j = 0; j < C1; ++j) {
                const float d = z[j] - mu[j];
                acc[j] = __builtin_fmaf(d, d, acc[j]);
            }
        }
    block_sum_store<C1>(acc, red, bm2);      // red was last read in front of the barrier above
    __syncthreads();
    if (threadIdx.x < C1) {
        float* o = part + ((long)blockIdx.x * C1 + threadIdx.x) * 3;
        o[0] = (float)cnt; o[1] = bmean[threadIdx.x] / (float)cnt; o[2] = bm2[threadIdx.x];
    }
}

// ------------------------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(TPB) void wi_fwd_kernel(const Src src, const long P, const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ scale, const float* __restrict__ shift,
                                                     const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out,
                                                     const int ldo) {
    __shared__ Coef k;
    fill(k.w1, w1, 3 * C1); fill(k.b1, b1, C1); fill(k.sc, scale, C1); fill(k.sh, shift, C1); fill(k.w2, w2, C1 * C2); fill(k.b2, b2, C2);
    __syncthreads();
    for (long p = (long)blockIdx.x * TPB + threadIdx.x; p < P; p += (long)gridDim.x * TPB) {
        float v[3], z[C1], y[C1], s[C2];
        load_rgb(src, p, v);
        conv1(k, v, z);
        tail(k, z, y, s);
        const f32x4 lo = {v[0], v[1], v[2], s[0]};
        const f32x4 hi = {s[1], s[2], s[3], 0.f};
        float* o = out + p * ldo;
        *reinterpret_cast<f32x4*>(o) = lo;
        *reinterpret_cast<f32x4*>(o + 4) = hi;
    }
}

// ------------------------------------------------------------------------------------------------------------------ backward
// part[block][W_RED] = sum da * xhat [16] | sum da [16] | sum a_j du_q [16][4] | sum du [4]
__global__ __launch_bounds__(TPB) void wi_bwd_reduce_kernel(const Src src, const long P, const float* __restrict__ g, const int ldg,
                                                            const float* __restrict__ w1, const float* __restrict__ b1,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const float* __restrict__ w2, const float* __restrict__ b2,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            float* __restrict__ part) {
    __shared__ Coef k;
    __shared__ float red[WAVES * W_RED];
    fill(k.w1, w1, 3 * C1); fill(k.b1, b1, C1); fill(k.sc, scale, C1); fill(k.sh, shift, C1); fill(k.w2, w2, C1 * C2); fill(k.b2, b2, C2);
    fill(k.mu, mean, C1); fill(k.is, invstd, C1);
    __syncthreads();
    const long p0 = (long)blockIdx.x * PPB;
    const int cnt = (int)(P - p0 < PPB ? P - p0 : PPB);
    float acc[W_RED];
#pragma unroll
    for (int j = 0; j < W_RED; ++j) acc[j] = 0.f;
    for (int o = threadIdx.x; o < cnt; o += TPB) {
        const long p = p0 + o;
        float v[3], gv[C2], z[C1], y[C1], s[C2], du[C2], da[C1];
        load_rgb(src, p, v);
#pragma unroll
        for (int q = 0; q < C2; ++q) gv[q] = g[p * ldg + q];
        conv1(k, v, z);
        tail(k, z, y, s);
        back_to_a(k, y, s, gv, du, da);
#pragma unroll
        for (int j = 0; j < C1; ++j) {
            acc[j] = __builtin_fmaf(da[j], (z[j] - k.mu[j]) * k.is[j], acc[j]);
            acc[C1 + j] += da[j];
            const float a = fmaxf(y[j], 0.f);
#pragma unroll
            for (int q = 0; q < C2; ++q) acc[2 * C1 + j * C2 + q] = __builtin_fmaf(a, du[q], acc[2 * C1 + j * C2 + q]);
        }
#pragma unroll
        for (int q = 0; q < C2; ++q) acc[2 * C1 + C1 * C2 + q] += du[q];
    }
    block_sum_store<W_RED>(acc, red, part + (long)blockIdx.x * W_RED);
}

// dz = BatchNorm backward (runet_bn_bwd_apply's formula) of da; part[block][W_APP] = sum x_c dz_j [3][16] | sum dz [16]
__global__ __launch_bounds__(TPB) void wi_bwd_apply_kernel(const Src src, const long P, const float* __restrict__ g, const int ldg,
                                                           const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           const float* __restrict__ w2, const float* __restrict__ b2,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ sums, const float inv_m, float* __restrict__ part) {
    __shared__ Coef k;
    __shared__ float red[WAVES * W_APP];
    fill(k.w1, w1, 3 * C1); fill(k.b1, b1, C1); fill(k.sc, scale, C1); fill(k.sh, shift, C1); fill(k.w2, w2, C1 * C2); fill(k.b2, b2, C2);
    if (threadIdx.x < C1) {
        const int j = threadIdx.x;
        float ca, cb;
        bn_bwd_coef(scale[j], mean[j], invstd[j], sums[j], sums[C1 + j], inv_m, ca, cb);
        k.ca[j] = ca; k.cb[j] = cb;
    }
    __syncthreads();
    const long p0 = (long)blockIdx.x * PPB;
    const int cnt = (int)(P - p0 < PPB ? P - p0 : PPB);
    float acc[W_APP];
#pragma unroll
    for (int j = 0; j < W_APP; ++j) acc[j] = 0.f;
    for (int o = threadIdx.x; o < cnt; o += TPB) {
        const long p = p0 + o;
        float v[3], gv[C2], z[C1], y[C1], s[C2], du[C2], da[C1];
        load_rgb(src, p, v);
#pragma unroll
        for (int q = 0; q < C2; ++q) gv[q] = g[p * ldg + q];
        conv1(k, v, z);
        tail(k, z, y, s);
        back_to_a(k, y, s, gv, du, da);
#pragma unroll
        for (int j = 0; j < C1; ++j) {
            const float dz = bn_bwd_dx(da[j], k.sc[j], z[j], k.ca[j], k.cb[j]);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c * C1 + j] = __builtin_fmaf(v[c], dz, acc[c * C1 + j]);
            acc[3 * C1 + j] += dz;
        }
    }
    block_sum_store<W_APP>(acc, red, part + (long)blockIdx.x * W_APP);
}

// ------------------------------------------------------------------------------------------------------------------ unfused partner
// The element-wise steps of the reference's order that no shared kernel offers (RUNET_NO_FUSED_WATER_INDEX=1): a sigmoid and its backward
// over c channels of NHWC views, and a channel-slice copy.  Views may start at any channel (4-byte accesses).
__global__ __launch_bounds__(TPB) void sigmoid_nhwc_fwd_kernel(const float* __restrict__ u, const int ldu, float* __restrict__ y, const int ldy,
                                                               const long P, const int C) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < P * C; i += (long)gridDim.x * TPB) {
        const long p = i / C;
        const int c = (int)(i - p * C);
        y[p * ldy + c] = sigmoidf_(u[p * ldu + c]);
    }
}
__global__ __launch_bounds__(TPB) void sigmoid_nhwc_bwd_kernel(const float* __restrict__ dy, const int lddy, const float* __restrict__ y, const int ldy,
                                                               float* __restrict__ du, const int lddu, const long P, const int C) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < P * C; i += (long)gridDim.x * TPB) {
        const long p = i / C;
        const int c = (int)(i - p * C);
        const float s = y[p * ldy + c];
        du[p * lddu + c] = dy[p * lddy + c] * s * (1.f - s);
    }
}
__global__ __launch_bounds__(TPB) void copy_nhwc_kernel(const float* __restrict__ x, const int ldx, float* __restrict__ y, const int ldy, const long P,
                                                        const int C) {
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < P * C; i += (long)gridDim.x * TPB) {
        const long p = i / C;
        const int c = (int)(i - p * C);
        y[p * ldy + c] = x[p * ldx + c];
    }
}
inline long n_blocks(long P) { return (P + PPB - 1) / PPB; }
inline bool shape_ok(int n, int h, int w) { return n > 0 && h > 0 && w > 0 && (long)h * w <= 0x7fffffffL && n_blocks((long)n * h * w) <= 0x7fffffffL / W_RED; }
}  // namespace

extern "C" int runet_water_index_parts(int n_img, int h, int w_) {
    if (!shape_ok(n_img, h, w_)) return -1;
    return (int)n_blocks((long)n_img * h * w_);
}

extern "C" long runet_water_index_workspace_floats(int n_img, int h, int w_) {
    if (!shape_ok(n_img, h, w_)) return -1;
    return n_blocks((long)n_img * h * w_) * W_RED;
}

extern "C" int runet_water_index_stats(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* b1,
                                       float* part, long part_floats, void* stream) {
    RUNET_REQUIRE(x && w1 && b1 && part, "null pointer");
    RUNET_REQUIRE(shape_ok(n_img, h, w_), "empty shape");
    const long P = (long)n_img * h * w_, nb = n_blocks(P);
    RUNET_REQUIRE(part_floats >= nb * C1 * 3, "partials buffer too small (runet_water_index_parts rows of 16 x 3 floats)");
    const Src src{x, sn, sc, sh, sw, h * w_, w_};
    hipLaunchKernelGGL(wi_stats_kernel, dim3((unsigned)nb), dim3(TPB), 0, (hipStream_t)stream, src, P, w1, b1, part);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_water_index_fwd(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* w1, const float* b1,
                                     const float* scale, const float* shift, const float* w2, const float* b2, float* out, int ldo, void* stream) {
    RUNET_REQUIRE(x && w1 && b1 && scale && shift && w2 && b2 && out, "null pointer");
    RUNET_REQUIRE(shape_ok(n_img, h, w_), "empty shape");
    RUNET_REQUIRE(ldo >= 8 && ldo % 4 == 0 && RUNET_ALIGNED16(out), "the output's pixel stride must be a multiple of 4 floats, at least 8, its pointer 16-byte aligned");
    const long P = (long)n_img * h * w_;
    long blocks = (P + TPB - 1) / TPB;
    if (blocks > 8192) blocks = 8192;
    const Src src{x, sn, sc, sh, sw, h * w_, w_};
    hipLaunchKernelGGL(wi_fwd_kernel, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, src, P, w1, b1, scale, shift, w2, b2, out, ldo);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_water_index_bwd_reduce(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* g, int ldg,
                                            const float* w1, const float* b1, const float* scale, const float* shift, const float* w2,
                                            const float* b2, const float* mean, const float* invstd, float* workspace, long workspace_floats,
                                            float* out, void* stream) {
    RUNET_REQUIRE(x && g && w1 && b1 && scale && shift && w2 && b2 && mean && invstd && workspace && out, "null pointer");
    RUNET_REQUIRE(shape_ok(n_img, h, w_), "empty shape");
    RUNET_REQUIRE(ldg >= 4, "the gradient's pixel stride must cover its 4 channels");
    const long P = (long)n_img * h * w_, nb = n_blocks(P);
    RUNET_REQUIRE(workspace_floats >= nb * W_RED, "workspace too small (runet_water_index_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    const Src src{x, sn, sc, sh, sw, h * w_, w_};
    hipLaunchKernelGGL(wi_bwd_reduce_kernel, dim3((unsigned)nb), dim3(TPB), 0, st, src, P, g, ldg, w1, b1, scale, shift, w2, b2, mean, invstd, workspace);
    sum_parts<16>(workspace, (int)nb, W_RED, out, st);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_water_index_bwd_apply(const float* x, long sn, long sc, long sh, long sw, int n_img, int h, int w_, const float* g, int ldg,
                                           const float* w1, const float* b1, const float* scale, const float* shift, const float* w2,
                                           const float* b2, const float* mean, const float* invstd, const float* sums, long m_total,
                                           float* workspace, long workspace_floats, float* out, void* stream) {
    RUNET_REQUIRE(x && g && w1 && b1 && scale && shift && w2 && b2 && mean && invstd && sums && workspace && out, "null pointer");
    RUNET_REQUIRE(shape_ok(n_img, h, w_), "empty shape");
    RUNET_REQUIRE(ldg >= 4, "the gradient's pixel stride must cover its 4 channels");
    const long P = (long)n_img * h * w_, nb = n_blocks(P);
    RUNET_REQUIRE(workspace_floats >= nb * W_APP, "workspace too small (runet_water_index_workspace_floats)");
    const float inv_m = 1.0f / (float)(m_total > 0 ? m_total : P);
    hipStream_t st = (hipStream_t)stream;
    const Src src{x, sn, sc, sh, sw, h * w_, w_};
    hipLaunchKernelGGL(wi_bwd_apply_kernel, dim3((unsigned)nb), dim3(TPB), 0, st, src, P, g, ldg, w1, b1, scale, shift, w2, b2, mean, invstd, sums, inv_m,
                       workspace);
    sum_parts<16>(workspace, (int)nb, W_APP, out, st);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_sigmoid_nhwc_fwd(const float* u, int ldu, float* y, int ldy, long pixels, int c, void* stream) {
    RUNET_REQUIRE(u && y, "null pointer");
    RUNET_REQUIRE(pixels > 0 && c > 0 && ldu >= c && ldy >= c, "empty shape, or a pixel stride below the channel count");
    hipLaunchKernelGGL(sigmoid_nhwc_fwd_kernel, dim3(ew_grid(pixels * c, 4096)), dim3(TPB), 0, (hipStream_t)stream, u, ldu, y, ldy, pixels, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_sigmoid_nhwc_bwd(const float* dy, int lddy, const float* y, int ldy, float* du, int lddu, long pixels, int c, void* stream) {
    RUNET_REQUIRE(dy && y && du, "null pointer");
    RUNET_REQUIRE(pixels > 0 && c > 0 && lddy >= c && ldy >= c && lddu >= c, "empty shape, or a pixel stride below the channel count");
    hipLaunchKernelGGL(sigmoid_nhwc_bwd_kernel, dim3(ew_grid(pixels * c, 4096)), dim3(TPB), 0, (hipStream_t)stream, dy, lddy, y, ldy, du, lddu, pixels, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_copy_nhwc(const float* x, int ldx, float* y, int ldy, long pixels, int c, void* stream) {
    RUNET_REQUIRE(x && y, "null pointer");
    RUNET_REQUIRE(pixels > 0 && c > 0 && ldx >= c && ldy >= c, "empty shape, or a pixel stride below the channel count");
    hipLaunchKernelGGL(copy_nhwc_kernel, dim3(ew_grid(pixels * c, 4096)), dim3(TPB), 0, (hipStream_t)stream, x, ldx, y, ldy, pixels, c);
    RUNET_CHECK_LAUNCH();
}
