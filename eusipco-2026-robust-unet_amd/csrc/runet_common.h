// Shared helpers for the gfx950 Robust U-Net kernels (internal; the public C ABI is include/runet_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/runet_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define RUNET_OK 0
#define RUNET_EINVAL 1
#define RUNET_ELAUNCH 2

extern "C" void runet_set_error(const char* msg);

#define RUNET_REQUIRE(cond, msg)                                          \
    do {                                                                  \
        if (!(cond)) {                                                    \
            char _b[512];                                                 \
            snprintf(_b, sizeof(_b), "%s: %s (%s)", __func__, msg, #cond); \
            runet_set_error(_b);                                          \
            return RUNET_EINVAL;                                          \
        }                                                                 \
    } while (0)

#define RUNET_CHECK_LAUNCH()                                                   \
    do {                                                                       \
        hipError_t _e = hipGetLastError();                                     \
        if (_e != hipSuccess) {                                                \
            char _b[512];                                                      \
            snprintf(_b, sizeof(_b), "%s: launch failed: %s", __func__, hipGetErrorString(_e)); \
            runet_set_error(_b);                                               \
            return RUNET_ELAUNCH;                                              \
        }                                                                      \
        return RUNET_OK;                                                       \
    } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Environment knobs (measurement and A/B switches).  Callers keep the value in a function-local static: read once per process.
static inline bool env_flag(const char* name) { const char* v = getenv(name); return v && atoi(v) != 0; }                 // set and non-zero
static inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }

// Threads per block of the helpers below that fix a block shape (ew_grid, sum_parts, block_rows_to_part); every kernel file's own TPB.
constexpr int RUNET_TPB = 256;
// blocks of a grid-stride element-wise kernel over `total` work items, at most `cap`
static inline int ew_grid(long total, int cap) {
    long b = (total + RUNET_TPB - 1) / RUNET_TPB;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// NHWC view checks of the entry points: a pixel stride that covers c channels in whole 16-byte groups, and a 16-byte aligned base.  The
// condition is spelled out in RUNET_REQ_LD because RUNET_REQUIRE echoes its text in the error message.
#define RUNET_ALIGNED16(p) (((uintptr_t)(p) % 16) == 0)
#define RUNET_REQ_LD(ld, c, p)                                                        \
    RUNET_REQUIRE((ld) >= (c) && (ld) % 4 == 0 && ((uintptr_t)(p) % 16) == 0,         \
                  "pixel strides must be multiples of 4 floats that cover the channels, tensors 16-byte aligned")

static inline int runet_band_elem_size(int dtype) { return dtype == RUNET_BAND_U8 ? 1 : dtype == RUNET_BAND_F32 ? 4 : 2; }
// The raster checks of the entry points that read band planes (scene_bands.hip, report.hip): a planar [n_bands][h][w] raster read through
// strides (in elements) that cover its extent.  runet_band_elem_size: bytes per element of a RUNET_BAND_* dtype.
#define RUNET_REQ_BANDS()                                                                                                            \
    do {                                                                                                                             \
        RUNET_REQUIRE(dtype >= RUNET_BAND_U8 && dtype <= RUNET_BAND_F32, "dtype must be RUNET_BAND_U8 / U16 / I16 / F32");           \
        RUNET_REQUIRE(n_bands >= 1 && h > 0 && w > 0, "bad shape");                                                                  \
        RUNET_REQUIRE((long)h * w < 2147483648L, "h * w must be below 2^31");                                                        \
        RUNET_REQUIRE(elem_stride >= 1 && row_stride >= (long)(w - 1) * elem_stride + 1, "strides smaller than a row's extent");     \
        RUNET_REQUIRE(n_bands == 1 || band_stride >= (long)(h - 1) * row_stride + (long)(w - 1) * elem_stride + 1,                   \
                      "band stride smaller than a band's extent");                                                                   \
        RUNET_REQUIRE(((uintptr_t)bands % runet_band_elem_size(dtype)) == 0, "bands must be aligned to their element size");                    \
    } while (0)

// gemm.hip (internal launchers behind runet_gemm_batched / runet_gemm_tn_batched)
int runet_gemm_nn_launch(const float* a, int lda, long sa, const float* b, long sb, float* c, int ldc, long sc, int batch, int rows, int k, int n,
                         hipStream_t st);
int runet_gemm_tn_launch(const float* a, int lda, long sa, const float* b, int ldb, long sb, float* c, int batch, int rows, int k, int n, int rps,
                         hipStream_t st);

// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a full workgroup fence, which on gfx9 drains vmcnt too:
// every global load still in flight (register prefetches meant to overlap the next phase) is waited for at the barrier.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// ---- wave / block reductions (wave = 64 lanes) ----
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// LDS histograms private to a wave: one count for `bin` (or none: bin < 0) from every lane of a converged wave.  The lanes that hold the
// first active lane's bin are added by that lane in one atomic: a run of equal keys costs one LDS atomic per wave, not 64 serialised ones on
// one address.
__device__ __forceinline__ void wave_add(unsigned* h, int bin, int lane) {
    const unsigned long long act = __ballot(bin >= 0);
    if (act == 0) return;
    const int leader = __ffsll((long long)act) - 1;
    const int lb = __shfl(bin, leader, 64);
    const unsigned long long same = __ballot(bin == lb);
    if (lane == leader) atomicAdd(&h[lb], (unsigned)__popcll(same));
    else if (bin >= 0 && bin != lb) atomicAdd(&h[bin], 1u);
}

// 16-byte access to four consecutive floats (p 16-byte aligned)
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, const f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
// a thread's VEC (4 or 1) consecutive channels to / from registers: one 16-byte access, or one float
template <int VEC>
__device__ __forceinline__ void load_vec(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const f32x4 t = ld4(p);
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else v[0] = p[0];
}
template <int VEC>
__device__ __forceinline__ void store_vec(float* p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const f32x4 t = {v[0], v[1], v[2], v[3]};
        st4(p, t);
    } else p[0] = v[0];
}

// ---- the two ordered passes of a two-stage reduction (no float atomics: these few lines fix the summation order, so the bits) ----
// In-block row pass: sm holds [rows][width] floats, one row of sums per thread row of the block.  After the barrier thread u adds column u
// over the rows in row order, in double, and writes part[block][u].
__device__ __forceinline__ void block_rows_to_part(const float* sm, int rows, int width, float* __restrict__ part) {
    __syncthreads();
    for (int u = threadIdx.x; u < width; u += RUNET_TPB) {
        double s = 0;
        for (int r = 0; r < rows; ++r) s += sm[r * width + u];
        part[(long)blockIdx.x * width + u] = (float)s;
    }
}
// Final pass, out[u] = sum_k part[k][u]: a block takes CW consecutive outputs x RUNET_TPB / CW part-lanes.  Lane pl adds the partial rows
// pl, pl + lanes, ... in that order, then the lane sums are added in lane order through LDS; double throughout, one cast to float.  The lane
// count is part of the order: a caller that changes its CW changes its bits.  Unnamed namespace: every translation unit keeps its own copy.
namespace {
template <int CW>
__global__ __launch_bounds__(RUNET_TPB) void sum_parts_kernel(const float* __restrict__ part, int nparts, int width, float* __restrict__ out) {
    constexpr int PL = RUNET_TPB / CW;
    __shared__ double red[RUNET_TPB];
    const int cl = threadIdx.x % CW, pl = threadIdx.x / CW;
    const int u = blockIdx.x * CW + cl;
    double s = 0;
    if (u < width) {
#pragma unroll 8                             // eight loads in flight per lane; the adds stay serial, in k order
        for (int k = pl; k < nparts; k += PL) s += part[(long)k * width + u];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (pl == 0 && u < width) {
        for (int j = 1; j < PL; ++j) s += red[j * CW + cl];
        out[u] = (float)s;
    }
}
template <int CW>
inline void sum_parts(const float* part, int nparts, int width, float* out, hipStream_t st) {
    hipLaunchKernelGGL(sum_parts_kernel<CW>, dim3(cdiv(width, CW)), dim3(RUNET_TPB), 0, st, part, nparts, width, out);
}
}  // namespace

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// BatchNorm pieces that several kernels must evaluate BIT-IDENTICALLY (bn_apply_kernel, the backward kernels that recompute the ReLU mask from
// x, the F(4x4) input transforms that take the BatchNorm in their loads): explicit FMAs, so the roundings do not depend on what the compiler
// contracts in each kernel.
__device__ __forceinline__ float bn_pre(const float x, const float scale, const float shift) { return __builtin_fmaf(x, scale, shift); }
// dx = gg * sc + x * ca + cb  with  ca = -sc * k2 * invstd,  cb = sc * (mean * invstd * k2 - k1),  k1 = sum(g) / m,  k2 = sum(g * xhat) / m
__device__ __forceinline__ void bn_bwd_coef(const float sc, const float mean, const float is, const float sum_gx, const float sum_g, const float inv_m,
                                            float& ca, float& cb) {
#pragma clang fp contract(off)
    const float k1 = sum_g * inv_m, k2 = sum_gx * inv_m;
    const float mi = mean * is;
    ca = -sc * k2 * is;
    cb = sc * __builtin_fmaf(mi, k2, -k1);
}
__device__ __forceinline__ float bn_bwd_dx(const float gg, const float sc, const float x, const float ca, const float cb) {
    return __builtin_fmaf(gg, sc, __builtin_fmaf(x, ca, cb));
}

// The full-resolution gradient behind a 2x2 max-pool, rebuilt in registers from the POOLED gradient dy [n, H/2, W/2] (pixel stride lddy) and
// the winner bytes pidx (dense, C per pooled pixel), exactly as runet_maxpool2_bwd(accumulate=0) would write it:
// g(h, w) = pidx[h/2, w/2] == (h&1)*2 + (w&1) ? dy[h/2, w/2] : 0.  W is the full-resolution width, p the pixel inside image n, c the first of
// the thread's 4 channels.  Shared by the BatchNorm-backward POOL instances (norm_act.hip) and rb_bwd1 (attention.hip).
// pooled_grad4_at: the same from the pooled pixel q (over all images) and the position k = (h&1)*2 + (w&1) in its window, for callers that
// visit several channel groups of one pixel.
__device__ __forceinline__ f32x4 pooled_grad4_at(const float* __restrict__ dy, int lddy, const unsigned char* __restrict__ pidx, int C, long q,
                                                 unsigned int k, int c) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(dy + q * lddy + c);
    const unsigned int s = *reinterpret_cast<const unsigned int*>(pidx + q * C + c);
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = (((s >> (8 * e)) & 0xff) == k) ? t[e] : 0.f;
    return g;
}
__device__ __forceinline__ f32x4 pooled_grad4(const float* __restrict__ dy, int lddy, const unsigned char* __restrict__ pidx, int W, int C,
                                              int n, int HW, int p, int c) {
    const int hh = p / W, ww = p - hh * W;
    const long q = (long)n * (HW >> 2) + (long)(hh >> 1) * (W >> 1) + (ww >> 1);
    return pooled_grad4_at(dy, lddy, pidx, C, q, (unsigned)((hh & 1) * 2 + (ww & 1)), c);
}

// GELU, the exact erf form (nn.GELU(), SegFormer-Lite's patch embeddings and MixFFN): ATen's expressions, shared by the BatchNorm + GELU
// kernels (norm_act.hip) and the depthwise convolution + GELU kernels (dwconv.hip).  gelu_grad(g, z) = g * GELU'(z).
__device__ __forceinline__ float gelu_f(const float z) { return z * 0.5f * (1.0f + erff(z * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad(const float g, const float z) {
    const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * z * z) * 0.39894228040143267794f;     // M_2_SQRTPI * M_SQRT1_2 * 0.5
    return g * (cdf + z * pdf);
}

// ATen's align_corners=False source index of a bilinear resize (upsample_bilinear2d): src = max(0, (o + 0.5) * scale - 0.5), scale = in / out;
// the two source taps i0, i1 (i1 clamped to the last row / column) and their weights.  Shared by the planar (runet_bilinear_*) and the NHWC
// (runet_bilinear_nhwc_*) kernels of misc.hip, so both follow the same rule bit for bit.
__device__ __forceinline__ void bilin_src(int o, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
    float src = scale * ((float)o + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}
// the weight with which output o reads input index i (0 when neither tap is i): the tap weight of the gather adjoints
__device__ __forceinline__ float bilin_tap_weight(int o, float scale, int in, int i) {
    int i0, i1;
    float l0, l1;
    bilin_src(o, scale, in, i0, i1, l0, l1);
    return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}
// adjoint (gather) range: the outputs whose two source taps can include input index i lie in [lo, hi] (index 0 also takes the clamped ones)
__device__ __forceinline__ void bilin_adj_range(int i, float scale, int out, int& lo, int& hi) {
    lo = i == 0 ? 0 : max(0, (int)floorf(((float)i - 0.5f) / scale - 0.5f) - 1);
    hi = min(out - 1, (int)ceilf(((float)i + 1.5f) / scale - 0.5f) + 1);
}
// the same for an integer factor S (scale = 1 / S, out = S * in), in integers: src = (o + 0.5) / S - 0.5 in [i - 1, i + 1)  <=>
// S i - S / 2 <= o <= S i + 3 S / 2 - 1 for an even S; an odd S takes the wider S i - S .. S i + 2 S.  Outputs of the range that do not read i
// have tap weight 0, so a wider range gives the same sum.
__device__ __forceinline__ void upsample_adj_range(int i, int S, int out, int& lo, int& hi) {
    lo = max(0, S * i - ((S & 1) ? S : S / 2));
    hi = min(out - 1, S * i + ((S & 1) ? 2 * S : 3 * S / 2 - 1));
}
