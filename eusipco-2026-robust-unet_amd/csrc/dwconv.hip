// Depthwise 3x3 convolution + bias + GELU of SegFormer-Lite's MixFFN (Extended_Baseline_Comparison.py:628-633: nn.Conv2d(hidden, hidden, 3,
// padding=1, groups=hidden) -> nn.GELU()).  NHWC fp32, weights w [3][3][C] (the HWIO memory of the [C, 1, 3, 3] parameter), 4 channels per lane.
// HBM-bound: every pass reads or writes each hidden tensor once, the 3x3 neighbourhood comes from L1 / L2.
//
//   forward      z = b + dwconv(x), a = GELU(z); z is written only when the caller keeps it
//   wgrad        g = da * GELU'(z), written (g may be da itself: each element is read and then written by the same lane), and the per-chunk
//                partial sums of dw [3][3][C] and db [C]; sum_parts<32> (runet_common.h) adds the chunks in order (fixed order, no atomics).
//                z is read, or (z NULL) recomputed from the nine neighbours of x that the dw sums read anyway, with the forward's arithmetic
//                (dwconv_z).  Keeping z measured faster: the model keeps it, the operator-level op recomputes
//   data grad    dx = the adjoint taps of g (a gather: each dx element sums its nine neighbours of g in a fixed order)
#include "runet_common.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int TPB = 256;

// z = b + sum over the in-image taps of w[tap] * x[neighbour], taps in (r, s) order: the forward and the backward's recomputation share it
__device__ __forceinline__ f32x4 dwconv_z(const float* __restrict__ x, int ldx, const float* __restrict__ w, const float* __restrict__ b,
                                          long img, int yh, int xw, int H, int W, int C, int c) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int ih = yh + r - 1;
        if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int iw = xw + s - 1;
            if ((unsigned)iw >= (unsigned)W) continue;
            acc += ld4(w + (r * 3 + s) * C + c) * ld4(x + (img + (long)ih * W + iw) * ldx + c);
        }
    }
    return acc + ld4(b + c);
}

__global__ __launch_bounds__(TPB) void dw3_gelu_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                           const float* __restrict__ b, float* __restrict__ z, int ldz, float* __restrict__ a,
                                                           int lda, int N, int H, int W, int C) {
    const int cv = C >> 2;
    const long total = (long)N * H * W * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % cv) * 4;
        const long p = i / cv;
        const int xw = (int)(p % W);
        const long t = p / W;
        const int yh = (int)(t % H);
        const long img = (t / H) * H * W;
        const f32x4 acc = dwconv_z(x, ldx, w, b, img, yh, xw, H, W, C, c);
        if (z) st4(z + p * ldz + c, acc);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = gelu_f(acc[e]);
        st4(a + p * lda + c, o);
    }
}

// grid (chunks); block = rows x (C/4) lanes, lane (row, col) takes pixels p0 + row, + rows, ... of the chunk; an LDS pass over the rows (in
// order) leaves part[chunk][10][C] = (dw taps 0..8, db)
__global__ __launch_bounds__(TPB) void dw3_gelu_wgrad_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                             const float* __restrict__ b, const float* da, int ldda, const float* __restrict__ z,
                                                             int ldz, float* g, int ldg, float* __restrict__ part, int N, int H, int W, int C,
                                                             long ppc) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int cv = C >> 2, rows = TPB / cv, tid = threadIdx.x;
    const int col = tid % cv, row = tid / cv, c = col * 4;
    const long P = (long)N * H * W;
    const long p0 = blockIdx.x * ppc, p1 = min(P, p0 + ppc);
    f32x4 acc[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row < rows) {
        for (long p = p0 + row; p < p1; p += rows) {
            const int xw = (int)(p % W);
            const long t = p / W;
            const int yh = (int)(t % H);
            const long img = (t / H) * H * W;
            const f32x4 dv = ld4(da + p * ldda + c);
            const f32x4 zv = z ? ld4(z + p * ldz + c) : dwconv_z(x, ldx, w, b, img, yh, xw, H, W, C, c);
            f32x4 gv;
#pragma unroll
            for (int e = 0; e < 4; ++e) gv[e] = gelu_grad(dv[e], zv[e]);
            st4(g + p * ldg + c, gv);
            acc[9] += gv;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int ih = yh + r - 1;
                if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int iw = xw + s - 1;
                    if ((unsigned)iw >= (unsigned)W) continue;
                    acc[r * 3 + s] += gv * ld4(x + (img + (long)ih * W + iw) * ldx + c);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) st4(sm + (row * 10 + k) * C + c, acc[k]);
    }
    block_rows_to_part(sm, rows, 10 * C, part);
}

__global__ __launch_bounds__(TPB) void dw3_dgrad_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ w, float* __restrict__ dx,
                                                        int lddx, int N, int H, int W, int C) {
    const int cv = C >> 2;
    const long total = (long)N * H * W * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % cv) * 4;
        const long p = i / cv;
        const int xw = (int)(p % W);
        const long t = p / W;
        const int yh = (int)(t % H);
        const long img = (t / H) * H * W;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int oh = yh + 1 - r;           // output pixel that read this one through tap (r, s)
            if ((unsigned)oh >= (unsigned)H) continue;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int ow = xw + 1 - s;
                if ((unsigned)ow >= (unsigned)W) continue;
                acc += ld4(w + (r * 3 + s) * C + c) * ld4(g + (img + (long)oh * W + ow) * ldg + c);
            }
        }
        st4(dx + p * lddx + c, acc);
    }
}

int wgrad_chunks(long P, int C) {
    const int rows = TPB / (C / 4);
    const long want = (P + 4L * rows - 1) / (4L * rows);       // at least 4 pixels per lane
    return (int)(want < 256 ? (want < 1 ? 1 : want) : 256);
}
}  // namespace

#define DW_REQ_SHAPE(n, h, w, c)                                                                                             \
    RUNET_REQUIRE((n) > 0 && (h) > 0 && (w) > 0 && (c) >= 4 && (c) % 4 == 0 && (c) <= 1024, "bad shape (c a multiple of 4, at most 1024)")

extern "C" int runet_dwconv3x3_gelu_fwd(const float* x, int ldx, const float* w, const float* b, float* z, int ldz, float* a, int lda, int n_img,
                                        int h, int w_, int c, void* stream) {
    RUNET_REQUIRE(x && w && b && a, "null pointer");
    DW_REQ_SHAPE(n_img, h, w_, c);
    RUNET_REQ_LD(ldx, c, x);
    RUNET_REQ_LD(lda, c, a);
    if (z) RUNET_REQ_LD(ldz, c, z);
    RUNET_REQUIRE(((uintptr_t)w % 16) == 0 && ((uintptr_t)b % 16) == 0, "w and b must be 16-byte aligned");
    hipLaunchKernelGGL(dw3_gelu_fwd_kernel, dim3(ew_grid((long)n_img * h * w_ * (c / 4), 8192)), dim3(TPB), 0, (hipStream_t)stream, x, ldx, w, b, z, ldz,
                       a, lda, n_img, h, w_, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_dwconv3x3_gelu_bwd_workspace_floats(int n_img, int h, int w_, int c) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || c < 4 || c % 4 || c > 1024) return -1;
    return (long)wgrad_chunks((long)n_img * h * w_, c) * 10 * c;
}

extern "C" int runet_dwconv3x3_gelu_bwd_wgrad(const float* x, int ldx, const float* w, const float* b, const float* da, int ldda, const float* z,
                                              int ldz, float* g, int ldg, float* workspace, long workspace_floats, float* dwdb, int n_img, int h,
                                              int w_, int c, void* stream) {
    RUNET_REQUIRE(x && w && b && da && g && workspace && dwdb, "null pointer");
    DW_REQ_SHAPE(n_img, h, w_, c);
    RUNET_REQ_LD(ldx, c, x);
    RUNET_REQ_LD(ldda, c, da);
    if (z) RUNET_REQ_LD(ldz, c, z);
    RUNET_REQUIRE(((uintptr_t)w % 16) == 0 && ((uintptr_t)b % 16) == 0, "w and b must be 16-byte aligned");
    RUNET_REQ_LD(ldg, c, g);
    RUNET_REQUIRE(g == da ? ldg == ldda : true, "g may alias da only with the same pixel stride");
    const long P = (long)n_img * h * w_;
    const int chunks = wgrad_chunks(P, c);
    RUNET_REQUIRE(workspace_floats >= (long)chunks * 10 * c, "workspace too small (runet_dwconv3x3_gelu_bwd_workspace_floats)");
    const long ppc = (P + chunks - 1) / chunks;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(TPB / (c / 4)) * 10 * c * sizeof(float);
    hipLaunchKernelGGL(dw3_gelu_wgrad_kernel, dim3(chunks), dim3(TPB), lds, st, x, ldx, w, b, da, ldda, z, ldz, g, ldg, workspace, n_img, h, w_, c,
                       ppc);
    sum_parts<32>(workspace, chunks, 10 * c, dwdb, st);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_dwconv3x3_bwd_data(const float* g, int ldg, const float* w, float* dx, int lddx, int n_img, int h, int w_, int c, void* stream) {
    RUNET_REQUIRE(g && w && dx, "null pointer");
    DW_REQ_SHAPE(n_img, h, w_, c);
    RUNET_REQ_LD(ldg, c, g);
    RUNET_REQ_LD(lddx, c, dx);
    RUNET_REQUIRE(((uintptr_t)w % 16) == 0, "w must be 16-byte aligned");
    hipLaunchKernelGGL(dw3_dgrad_kernel, dim3(ew_grid((long)n_img * h * w_ * (c / 4), 8192)), dim3(TPB), 0, (hipStream_t)stream, g, ldg, w, dx, lddx,
                       n_img, h, w_, c);
    RUNET_CHECK_LAUNCH();
}
