// Fast-SCNN baseline (the reference's comne.py:305-476): what the shared kernels cannot express.
//
//   depthwise      nn.Conv2d(c, c, 3, stride 1 | 2, padding 1, groups=c, bias=False) (:310-311): forward, weight gradient (chunk partials
//                  plus the ordered final pass sum_parts<32>) and data gradient (a stride-aware gather).  dw3_common.h holds the per-pixel arithmetic.
//   pyramid        PyramidPoolingFastSCNN (:343-371): AdaptiveAvgPool2d to 1 / 2 / 3 / 6 bins in one pass over x, written branch-major as
//                  [n * 1 | n * 4 | n * 9 | n * 36] rows of c floats, so each branch is a dense [n, b, b, c] image for the shared 1x1
//                  convolution and BatchNorm; the gather adjoint (with the concat's direct slice added); the four F.interpolate calls into
//                  four channel slices of the concat buffer in one launch, and their gather adjoint.
//   fusion         FeatureFusionModule (:421-427): relu(bn(low) + interpolate(bn(high))).  The BatchNorm affine commutes with the
//                  interpolation (its weights sum to 1), so the high branch's raw convolution output is interpolated in registers and the
//                  upsampled tensor never exists.  runet_relu_mask_nhwc is the ReLU's backward for the high branch's gather.
//   head           F.interpolate(logits, size of the input) -> sigmoid (:474-476) for an integer factor s, and its gather adjoint.
//
// All HBM-bound: NHWC fp32, 16-byte accesses along the channels.  Every sum has a fixed order (per-thread serial, LDS in row order, partials
// in index order; no float atomics), so results are bitwise reproducible.  Source-index rule: bilin_src of runet_common.h.
#include "dw3_common.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int TPB = 256;

// ---------------------------------------------------------------------------------------------------------------- depthwise 3x3
__global__ __launch_bounds__(TPB) void dw3_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w, float* __restrict__ y,
                                                      int ldy, int N, int H, int W, int Ho, int Wo, int C, int stride) {
    const int cv = C >> 2;
    const long total = (long)N * Ho * Wo * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % cv) * 4;
        const long p = i / cv;
        const int ow = (int)(p % Wo);
        const long t = p / Wo;
        const int oh = (int)(t % Ho);
        const float* xi = x + (t / Ho) * H * W * (long)ldx + c;
        f32x4 wv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wv[k] = ld4(w + k * C + c);
        st4(y + p * ldy + c, dw3_point([&](int ih, int iw) { return ld4(xi + ((long)ih * W + iw) * ldx); }, wv, oh, ow, H, W, stride));
    }
}

// grid (chunks of output pixels); block = rows x (C/4) lanes, lane (row, col) takes output pixels p0 + row, + rows, ... of the chunk; an LDS
// pass over the rows (in order) leaves part[chunk][9][C]
__global__ __launch_bounds__(TPB) void dw3_wgrad_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ dy, int lddy,
                                                        float* __restrict__ part, int N, int H, int W, int Ho, int Wo, int C, int stride, long ppc) {
    extern __shared__ __attribute__((aligned(16))) float sm[];       // [rows][9][C]
    const int cv = C >> 2, rows = TPB / cv, tid = threadIdx.x;
    const int col = tid % cv, row = tid / cv, c = col * 4;
    const long P = (long)N * Ho * Wo;
    const long p0 = blockIdx.x * ppc, p1 = min(P, p0 + ppc);
    if (row < rows) {
        f32x4 acc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (long p = p0 + row; p < p1; p += rows) {
            const int ow = (int)(p % Wo);
            const long t = p / Wo;
            const int oh = (int)(t % Ho);
            const float* xi = x + (t / Ho) * H * W * (long)ldx + c;
            const f32x4 dv = ld4(dy + p * lddy + c);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int ih = oh * stride + r - 1;
                if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int iw = ow * stride + s - 1;
                    if ((unsigned)iw >= (unsigned)W) continue;
                    acc[r * 3 + s] += dv * ld4(xi + ((long)ih * W + iw) * ldx);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) st4(sm + (row * 9 + k) * C + c, acc[k]);
    }
    block_rows_to_part(sm, rows, 9 * C, part);
}

// dx[ih][iw] = sum over the taps (r, s), in that order, of w[r][s] * dy[oh][ow] for the outputs with oh * stride + r - 1 == ih (a gather)
__global__ __launch_bounds__(TPB) void dw3_dgrad_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ w, float* __restrict__ dx,
                                                        int lddx, int N, int H, int W, int Ho, int Wo, int C, int stride) {
    const int cv = C >> 2;
    const long total = (long)N * H * W * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % cv) * 4;
        const long p = i / cv;
        const int iw = (int)(p % W);
        const long t = p / W;
        const int ih = (int)(t % H);
        const float* gi = dy + (t / H) * Ho * Wo * (long)lddy + c;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int th = ih + 1 - r;
            if (th < 0 || th % stride) continue;
            const int oh = th / stride;
            if (oh >= Ho) continue;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int tw = iw + 1 - s;
                if (tw < 0 || tw % stride) continue;
                const int ow = tw / stride;
                if (ow >= Wo) continue;
                acc += ld4(w + (r * 3 + s) * C + c) * ld4(gi + ((long)oh * Wo + ow) * lddy);
            }
        }
        st4(dx + p * lddx + c, acc);
    }
}

int dw3_chunks(long P, int C) {
    const int rows = TPB / (C / 4);
    const long want = (P + 4L * rows - 1) / (4L * rows);       // at least 4 pixels per lane
    return (int)(want < 256 ? (want < 1 ? 1 : want) : 256);
}

// ---------------------------------------------------------------------------------------------------------------- pyramid pooling
// rows of the branch-major buffers: branch j (b = BINS[j] bins) starts at row N * OFF[j], image n at + n * b * b, cell (by, bx) at + by * b + bx
__device__ __forceinline__ void pyr_row(long row, long N, int& j, int& b, long& n, int& by, int& bx) {
    long rem;
    if (row < N) { j = 0; b = 1; rem = row; }
    else if (row < 5 * N) { j = 1; b = 2; rem = row - N; }
    else if (row < 14 * N) { j = 2; b = 3; rem = row - 5 * N; }
    else { j = 3; b = 6; rem = row - 14 * N; }
    n = rem / (b * b);
    const int cell = (int)(rem % (b * b));
    by = cell / b;
    bx = cell % b;
}
// ATen's adaptive window: [floor(i * in / b), ceil((i + 1) * in / b))
__device__ __forceinline__ void pyr_win(int i, int in, int b, int& lo, int& hi) {
    lo = (i * in) / b;
    hi = ((i + 1) * in + b - 1) / b;
}

// one block per output row (image, branch, cell): lane (row, col) sums the window pixels row, row + rows, ... of its channel quad, the rows are
// added in order through LDS
__global__ __launch_bounds__(TPB) void pyramid_pool_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ pooled, int ldp, long N,
                                                               int H, int W, int C) {
    __shared__ __attribute__((aligned(16))) float sm[4 * TPB];       // [rows][C], rows * C <= 4 * TPB
    const int cv = C >> 2, rows = TPB / cv, tid = threadIdx.x;
    const int col = tid % cv, row = tid / cv, c = col * 4;
    int j, b, by, bx, y0, y1, x0, x1;
    long n;
    pyr_row(blockIdx.x, N, j, b, n, by, bx);
    pyr_win(by, H, b, y0, y1);
    pyr_win(bx, W, b, x0, x1);
    const int ww = x1 - x0, area = (y1 - y0) * ww;
    if (row < rows) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const float* xi = x + n * H * W * (long)ldx + c;
        for (int k = row; k < area; k += rows) acc += ld4(xi + ((long)(y0 + k / ww) * W + x0 + k % ww) * ldx);
        st4(sm + row * C + c, acc);
    }
    __syncthreads();
    for (int u = tid; u < C; u += TPB) {
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += sm[r * C + u];
        pooled[(long)blockIdx.x * ldp + u] = s / (float)area;
    }
}

// dx = direct (optional) + for the four levels in order, the cells (row-major) whose window holds the pixel: dpooled / window area
__global__ __launch_bounds__(TPB) void pyramid_pool_bwd_kernel(const float* __restrict__ dpooled, int ldp, const float* __restrict__ direct, int ldd,
                                                               float* __restrict__ dx, int lddx, long N, int H, int W, int C) {
    const int cv = C >> 2;
    const long total = N * H * W * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % cv) * 4;
        const long p = i / cv;
        const int xw = (int)(p % W);
        const long t = p / W;
        const int yh = (int)(t % H);
        const long n = t / H;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (direct) acc = ld4(direct + p * ldd + c);
        long base = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = j == 0 ? 1 : j == 1 ? 2 : j == 2 ? 3 : 6;
            const float* dp = dpooled + (base + n * b * b) * ldp + c;
            for (int by = 0; by < b; ++by) {
                int y0, y1;
                pyr_win(by, H, b, y0, y1);
                if (yh < y0 || yh >= y1) continue;
                for (int bx = 0; bx < b; ++bx) {
                    int x0, x1;
                    pyr_win(bx, W, b, x0, x1);
                    if (xw < x0 || xw >= x1) continue;
                    acc += ld4(dp + (long)(by * b + bx) * ldp) / (float)((y1 - y0) * (x1 - x0));
                }
            }
            base += N * b * b;
        }
        st4(dx + p * lddx + c, acc);
    }
}

// y[n][h][w][j * CQ + 0:CQ] = bilinear resize of branch j's [n][b][b][CQ] image to h x w: thread per (pixel, branch, channel quad)
__global__ __launch_bounds__(TPB) void pyramid_upsample_fwd_kernel(const float* __restrict__ a, int lda, float* __restrict__ y, int ldy, long N, int H,
                                                                   int W, int CQ) {
    const int cv = CQ >> 2;
    const long total = N * H * W * 4 * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % cv) * 4;
        long p = i / cv;
        const int j = (int)(p & 3);
        p >>= 2;
        const int ox = (int)(p % W);
        const long t = p / W;
        const int oy = (int)(t % H);
        const long n = t / H;
        const int b = j == 0 ? 1 : j == 1 ? 2 : j == 2 ? 3 : 6;
        const long off = j == 0 ? 0 : j == 1 ? 1 : j == 2 ? 5 : 14;
        const float* ap = a + (N * off + n * b * b) * lda + c;
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        bilin_src(oy, (float)b / (float)H, b, y0, y1, ly0, ly1);
        bilin_src(ox, (float)b / (float)W, b, x0, x1, lx0, lx1);
        const f32x4 q00 = ld4(ap + (long)(y0 * b + x0) * lda), q01 = ld4(ap + (long)(y0 * b + x1) * lda);
        const f32x4 q10 = ld4(ap + (long)(y1 * b + x0) * lda), q11 = ld4(ap + (long)(y1 * b + x1) * lda);
        st4(y + p * ldy + j * CQ + c, ly0 * (lx0 * q00 + lx1 * q01) + ly1 * (lx0 * q10 + lx1 * q11));
    }
}

// da[row] = the adjoint in gather form: the outputs (rows, then columns) whose source taps include the row's cell; thread per (row, channel quad)
__global__ __launch_bounds__(TPB) void pyramid_upsample_bwd_kernel(const float* __restrict__ dy, int lddy, float* __restrict__ da, int lda, long N,
                                                                   int H, int W, int CQ) {
    const int cv = CQ >> 2;
    const long total = N * 50 * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % cv) * 4;
        const long row = i / cv;
        int j, b, by, bx;
        long n;
        pyr_row(row, N, j, b, n, by, bx);
        const float sh = (float)b / (float)H, sw = (float)b / (float)W;
        const float* gp = dy + n * H * W * (long)lddy + j * CQ + c;
        int oy_lo, oy_hi, ox_lo, ox_hi;
        bilin_adj_range(by, sh, H, oy_lo, oy_hi);
        bilin_adj_range(bx, sw, W, ox_lo, ox_hi);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            const float wy = bilin_tap_weight(oy, sh, b, by);
            if (wy == 0.f) continue;
            f32x4 r = {0.f, 0.f, 0.f, 0.f};
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const float wx = bilin_tap_weight(ox, sw, b, bx);
                if (wx != 0.f) r += wx * ld4(gp + ((long)oy * W + ox) * lddy);
            }
            acc += wy * r;
        }
        st4(da + row * lda + c, acc);
    }
}

// ---------------------------------------------------------------------------------------------------------------- feature fusion
// y = relu((t_low * s_l + h_l) + (bilinear_S(t_high) * s_h + h_h)): thread per (output pixel, channel quad)
__global__ __launch_bounds__(TPB) void ffm_fwd_kernel(const float* __restrict__ tl, int ldl, const float* __restrict__ th, int ldh,
                                                      const float* __restrict__ sl, const float* __restrict__ hl, const float* __restrict__ sh,
                                                      const float* __restrict__ hh, float* __restrict__ y, int ldy, long N, int H, int W, int S, int C) {
    const int cv = C >> 2, Ho = S * H, Wo = S * W;
    const float inv = 1.f / (float)S;
    const long total = N * Ho * Wo * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % cv) * 4;
        const long p = i / cv;
        const int ox = (int)(p % Wo);
        const long r = p / Wo;
        const int oy = (int)(r % Ho);
        const float* xp = th + (r / Ho) * H * W * (long)ldh + c;
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        bilin_src(oy, inv, H, y0, y1, ly0, ly1);
        bilin_src(ox, inv, W, x0, x1, lx0, lx1);
        const f32x4 a = ld4(xp + ((long)y0 * W + x0) * ldh), b = ld4(xp + ((long)y0 * W + x1) * ldh);
        const f32x4 d = ld4(xp + ((long)y1 * W + x0) * ldh), e = ld4(xp + ((long)y1 * W + x1) * ldh);
        const f32x4 v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * d + lx1 * e);
        const f32x4 lo = ld4(tl + p * ldl + c);
        const f32x4 s0 = ld4(sl + c), h0 = ld4(hl + c), s1 = ld4(sh + c), h1 = ld4(hh + c);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = fmaxf(bn_pre(lo[q], s0[q], h0[q]) + bn_pre(v[q], s1[q], h1[q]), 0.f);
        st4(y + p * ldy + c, o);
    }
}

__global__ __launch_bounds__(TPB) void relu_mask_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy,
                                                        float* __restrict__ g, int ldg, long P, int C) {
    const int cv = C >> 2;
    const long total = P * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % cv) * 4;
        const long p = i / cv;
        const f32x4 d = ld4(dy + p * lddy + c), a = ld4(y + p * ldy + c);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = a[q] > 0.f ? d[q] : 0.f;
        st4(g + p * ldg + c, o);
    }
}

// ---------------------------------------------------------------------------------------------------------------- head
// prob[n][S h][S w] = sigmoid(bilinear_S(z)); thread per output
__global__ __launch_bounds__(TPB) void up_sigmoid_fwd_kernel(const float* __restrict__ z, float* __restrict__ prob, long N, int H, int W, int S) {
    const int Ho = S * H, Wo = S * W;
    const float inv = 1.f / (float)S;
    const long total = N * Ho * Wo;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int ox = (int)(i % Wo);
        const long r = i / Wo;
        const int oy = (int)(r % Ho);
        const float* zp = z + (r / Ho) * H * W;
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        bilin_src(oy, inv, H, y0, y1, ly0, ly1);
        bilin_src(ox, inv, W, x0, x1, lx0, lx1);
        const float* r0 = zp + (long)y0 * W;
        const float* r1 = zp + (long)y1 * W;
        prob[i] = sigmoidf_(ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (lx0 * r1[x0] + lx1 * r1[x1]));
    }
}
// dz[n][iy][ix] = sum over the outputs whose taps include (iy, ix) of wy * wx * dprob * prob * (1 - prob): gather form, rows then columns
__global__ __launch_bounds__(TPB) void up_sigmoid_bwd_kernel(const float* __restrict__ dprob, const float* __restrict__ prob, float* __restrict__ dz,
                                                             long N, int H, int W, int S) {
    const int Ho = S * H, Wo = S * W;
    const float inv = 1.f / (float)S;
    const long total = N * H * W;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int ix = (int)(i % W);
        const long r = i / W;
        const int iy = (int)(r % H);
        const long plane = (r / H) * Ho * Wo;
        int oy_lo, oy_hi, ox_lo, ox_hi;
        upsample_adj_range(iy, S, Ho, oy_lo, oy_hi);
        upsample_adj_range(ix, S, Wo, ox_lo, ox_hi);
        float acc = 0.f;
        for (int oy = oy_lo; oy <= oy_hi; ++oy) {
            const float wy = bilin_tap_weight(oy, inv, H, iy);
            if (wy == 0.f) continue;
            float row = 0.f;
            for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                const float wx = bilin_tap_weight(ox, inv, W, ix);
                if (wx != 0.f) {
                    const long q = plane + (long)oy * Wo + ox;
                    const float pr = prob[q];
                    row += wx * (dprob[q] * pr * (1.f - pr));
                }
            }
            acc += wy * row;
        }
        dz[i] = acc;
    }
}
}  // namespace

#define FS_REQ_SHAPE(n, h, w, c)                                                                                             \
    RUNET_REQUIRE((n) > 0 && (h) > 0 && (w) > 0 && (c) >= 4 && (c) % 4 == 0 && (c) <= 1024, "bad shape (c a multiple of 4, at most 1024)")
#define FS_REQ_STRIDE(s) RUNET_REQUIRE((s) == 1 || (s) == 2, "stride must be 1 or 2")
#define FS_REQ_PLANE(n, h, w, s) RUNET_REQUIRE((n) > 0 && (h) > 0 && (w) > 0 && (s) >= 1 && (s) <= 32 && (long)(n) * (h) * (w) * (s) * (s) < (1L << 40), "bad shape (factor s in 1..32)")

extern "C" int runet_dw3_fwd(const float* x, int ldx, const float* w, float* y, int ldy, int n_img, int h, int w_, int c, int stride, void* stream) {
    RUNET_REQUIRE(x && w && y, "null pointer");
    FS_REQ_SHAPE(n_img, h, w_, c);
    FS_REQ_STRIDE(stride);
    RUNET_REQ_LD(ldx, c, x);
    RUNET_REQ_LD(ldy, c, y);
    RUNET_REQUIRE(((uintptr_t)w % 16) == 0, "w must be 16-byte aligned");
    const int ho = (h + stride - 1) / stride, wo = (w_ + stride - 1) / stride;
    hipLaunchKernelGGL(dw3_fwd_kernel, dim3(ew_grid((long)n_img * ho * wo * (c / 4), 8192)), dim3(TPB), 0, (hipStream_t)stream, x, ldx, w, y, ldy, n_img, h,
                       w_, ho, wo, c, stride);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_dw3_wgrad_workspace_floats(int n_img, int h, int w_, int c, int stride) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || c < 4 || c % 4 || c > 1024 || (stride != 1 && stride != 2)) return -1;
    const long P = (long)n_img * ((h + stride - 1) / stride) * ((w_ + stride - 1) / stride);
    return (long)dw3_chunks(P, c) * 9 * c;
}

extern "C" int runet_dw3_wgrad(const float* x, int ldx, const float* dy, int lddy, float* workspace, long workspace_floats, float* dw, int n_img, int h,
                               int w_, int c, int stride, void* stream) {
    RUNET_REQUIRE(x && dy && workspace && dw, "null pointer");
    FS_REQ_SHAPE(n_img, h, w_, c);
    FS_REQ_STRIDE(stride);
    RUNET_REQ_LD(ldx, c, x);
    RUNET_REQ_LD(lddy, c, dy);
    const int ho = (h + stride - 1) / stride, wo = (w_ + stride - 1) / stride;
    const long P = (long)n_img * ho * wo;
    const int chunks = dw3_chunks(P, c);
    RUNET_REQUIRE(workspace_floats >= (long)chunks * 9 * c, "workspace too small (runet_dw3_wgrad_workspace_floats)");
    const long ppc = (P + chunks - 1) / chunks;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)(TPB / (c / 4)) * 9 * c * sizeof(float);
    hipLaunchKernelGGL(dw3_wgrad_kernel, dim3(chunks), dim3(TPB), lds, st, x, ldx, dy, lddy, workspace, n_img, h, w_, ho, wo, c, stride, ppc);
    sum_parts<32>(workspace, chunks, 9 * c, dw, st);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_dw3_dgrad(const float* dy, int lddy, const float* w, float* dx, int lddx, int n_img, int h, int w_, int c, int stride,
                               void* stream) {
    RUNET_REQUIRE(dy && w && dx, "null pointer");
    FS_REQ_SHAPE(n_img, h, w_, c);
    FS_REQ_STRIDE(stride);
    RUNET_REQ_LD(lddy, c, dy);
    RUNET_REQ_LD(lddx, c, dx);
    RUNET_REQUIRE(((uintptr_t)w % 16) == 0, "w must be 16-byte aligned");
    const int ho = (h + stride - 1) / stride, wo = (w_ + stride - 1) / stride;
    hipLaunchKernelGGL(dw3_dgrad_kernel, dim3(ew_grid((long)n_img * h * w_ * (c / 4), 8192)), dim3(TPB), 0, (hipStream_t)stream, dy, lddy, w, dx, lddx,
                       n_img, h, w_, ho, wo, c, stride);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_pyramid_pool_fwd(const float* x, int ldx, float* pooled, int ldp, int n_img, int h, int w_, int c, void* stream) {
    RUNET_REQUIRE(x && pooled, "null pointer");
    FS_REQ_SHAPE(n_img, h, w_, c);
    RUNET_REQUIRE((long)n_img * 50 < (1L << 31) && (long)h * w_ < (1L << 31), "shape too large");
    RUNET_REQ_LD(ldx, c, x);
    RUNET_REQ_LD(ldp, c, pooled);
    hipLaunchKernelGGL(pyramid_pool_fwd_kernel, dim3(n_img * 50), dim3(TPB), 0, (hipStream_t)stream, x, ldx, pooled, ldp, (long)n_img, h, w_, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_pyramid_pool_bwd(const float* dpooled, int ldp, const float* direct, int ldd, float* dx, int lddx, int n_img, int h, int w_,
                                      int c, void* stream) {
    RUNET_REQUIRE(dpooled && dx, "null pointer");
    FS_REQ_SHAPE(n_img, h, w_, c);
    RUNET_REQ_LD(ldp, c, dpooled);
    RUNET_REQ_LD(lddx, c, dx);
    if (direct) RUNET_REQ_LD(ldd, c, direct);
    hipLaunchKernelGGL(pyramid_pool_bwd_kernel, dim3(ew_grid((long)n_img * h * w_ * (c / 4), 8192)), dim3(TPB), 0, (hipStream_t)stream, dpooled, ldp, direct,
                       ldd, dx, lddx, (long)n_img, h, w_, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_pyramid_upsample_fwd(const float* a, int lda, float* y, int ldy, int n_img, int h, int w_, int cq, void* stream) {
    RUNET_REQUIRE(a && y, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0 && cq >= 4 && cq % 4 == 0 && cq <= 256, "bad shape (cq a multiple of 4, at most 256)");
    RUNET_REQ_LD(lda, cq, a);
    RUNET_REQ_LD(ldy, 4 * cq, y);
    hipLaunchKernelGGL(pyramid_upsample_fwd_kernel, dim3(ew_grid((long)n_img * h * w_ * cq, 8192)), dim3(TPB), 0, (hipStream_t)stream, a, lda, y, ldy,
                       (long)n_img, h, w_, cq);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_pyramid_upsample_bwd(const float* dy, int lddy, float* da, int lda, int n_img, int h, int w_, int cq, void* stream) {
    RUNET_REQUIRE(dy && da, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0 && cq >= 4 && cq % 4 == 0 && cq <= 256, "bad shape (cq a multiple of 4, at most 256)");
    RUNET_REQ_LD(lddy, 4 * cq, dy);
    RUNET_REQ_LD(lda, cq, da);
    hipLaunchKernelGGL(pyramid_upsample_bwd_kernel, dim3(ew_grid((long)n_img * 50 * (cq / 4), 8192)), dim3(TPB), 0, (hipStream_t)stream, dy, lddy, da, lda,
                       (long)n_img, h, w_, cq);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_ffm_fwd(const float* t_low, int ldl, const float* t_high, int ldh, const float* scale_low, const float* shift_low,
                             const float* scale_high, const float* shift_high, float* y, int ldy, int n_img, int h, int w_, int s, int c,
                             void* stream) {
    RUNET_REQUIRE(t_low && t_high && scale_low && shift_low && scale_high && shift_high && y, "null pointer");
    FS_REQ_SHAPE(n_img, h, w_, c);
    RUNET_REQUIRE(s >= 1 && s <= 32, "the factor s must be in 1..32");
    RUNET_REQ_LD(ldl, c, t_low);
    RUNET_REQ_LD(ldh, c, t_high);
    RUNET_REQ_LD(ldy, c, y);
    RUNET_REQUIRE(((uintptr_t)scale_low % 16) == 0 && ((uintptr_t)shift_low % 16) == 0 && ((uintptr_t)scale_high % 16) == 0 &&
                      ((uintptr_t)shift_high % 16) == 0, "coefficient vectors must be 16-byte aligned");
    hipLaunchKernelGGL(ffm_fwd_kernel, dim3(ew_grid((long)n_img * h * w_ * s * s * (c / 4), 8192)), dim3(TPB), 0, (hipStream_t)stream, t_low, ldl, t_high,
                       ldh, scale_low, shift_low, scale_high, shift_high, y, ldy, (long)n_img, h, w_, s, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_relu_mask_nhwc(const float* dy, int lddy, const float* y, int ldy, float* g, int ldg, long pixels, int c, void* stream) {
    RUNET_REQUIRE(dy && y && g, "null pointer");
    RUNET_REQUIRE(pixels > 0 && c >= 4 && c % 4 == 0, "bad shape (c a positive multiple of 4)");
    RUNET_REQ_LD(lddy, c, dy);
    RUNET_REQ_LD(ldy, c, y);
    RUNET_REQ_LD(ldg, c, g);
    hipLaunchKernelGGL(relu_mask_kernel, dim3(ew_grid(pixels * (c / 4), 8192)), dim3(TPB), 0, (hipStream_t)stream, dy, lddy, y, ldy, g, ldg, pixels, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_up_sigmoid_fwd(const float* z, float* prob, int n_img, int h, int w_, int s, void* stream) {
    RUNET_REQUIRE(z && prob, "null pointer");
    FS_REQ_PLANE(n_img, h, w_, s);
    hipLaunchKernelGGL(up_sigmoid_fwd_kernel, dim3(ew_grid((long)n_img * h * w_ * s * s, 8192)), dim3(TPB), 0, (hipStream_t)stream, z, prob, (long)n_img, h,
                       w_, s);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_up_sigmoid_bwd(const float* dprob, const float* prob, float* dz, int n_img, int h, int w_, int s, void* stream) {
    RUNET_REQUIRE(dprob && prob && dz, "null pointer");
    FS_REQ_PLANE(n_img, h, w_, s);
    hipLaunchKernelGGL(up_sigmoid_bwd_kernel, dim3(ew_grid((long)n_img * h * w_, 8192)), dim3(TPB), 0, (hipStream_t)stream, dprob, prob, dz, (long)n_img, h,
                       w_, s);
    RUNET_CHECK_LAUNCH();
}
