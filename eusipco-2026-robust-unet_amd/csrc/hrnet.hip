// HRNet-Water baseline (the reference's Extended_Baseline_Comparison.py:554-616): the two places where the model, written in the reference's
// order, streams a tensor through HBM that a commuted order never needs.
//
//   head     Conv3x3 144->64, BatchNorm, ReLU, Upsample x2, Conv1x1 64->1, Sigmoid (:598-602).  Bilinear weights sum to 1, so the 1x1
//            convolution (bias included) commutes with the interpolation: the 64 -> 1 contraction runs at half resolution straight from
//            the 3x3 convolution's raw output (runet_hr_head_fwd: BatchNorm + ReLU in registers, the activated tensor is never written) and
//            only the one-channel logit plane is upsampled (runet_up2_sigmoid_fwd).  The full-resolution 64-channel map, its gradient and
//            the half-resolution activation and its gradient never exist: the backward goes dprob -> dz (runet_up2_sigmoid_bwd) ->
//            (dw, db, BatchNorm sums) in one pass over t (runet_hr_head_bwd_reduce) -> dt (runet_hr_head_bwd_apply).
//   fusion   Conv1x1, BatchNorm, Upsample x2 / x4, no activation (:588-595).  The BatchNorm affine commutes with the interpolation the same
//            way: runet_bn_bilinear_nhwc_fwd interpolates the raw convolution output into the concat slice and applies scale / shift as
//            one FMA per output; runet_bilinear_nhwc_bwd_sums gathers the slice gradient back and takes the BatchNorm-backward sums of the
//            gathered gradient in the same pass (runet_bn_bwd_apply with act = NULL finishes).
//
// All HBM-bound: 16-byte accesses along the channels, per-channel coefficients in registers.  Every sum has a fixed order (per-thread
// serial, LDS in row order, partials in index order; no float atomics), so results are bitwise reproducible.
// Source-index rule: bilin_src of runet_common.h (ATen align_corners=False) with scale 1/2 and 1/4, both exact in fp32.
#include "runet_common.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int TPB = 256;
constexpr int MAX_PARTS = 1024;      // blocks of a partial reduction (rows of the caller's workspace)

// blocks of a (channel quad x pixel row) streaming kernel over P pixels of C channels: ~`elems` elements per block, at most `cap` blocks
inline int pixel_chunks(long P, int C, long elems, int cap, long& ppc) {
    long chunks = (P * C + elems - 1) / elems;
    if (chunks > cap) chunks = cap;
    if (chunks < 1) chunks = 1;
    ppc = (P + chunks - 1) / chunks;
    return (int)((P + ppc - 1) / ppc);
}

// ------------------------------------------------------------------------------------------------------------------ head, forward
// z[p] = b + sum_c w[c] * relu(t[p][c] * scale[c] + shift[c]).  L lanes share a pixel (L = the power of two >= C / 4, at most 64: 16 lanes x
// float4 for C = 64), each owns the channel quads lane, lane + L, ...; the L partial sums meet in an in-wave butterfly.
__global__ __launch_bounds__(TPB) void hr_head_fwd_kernel(const float* __restrict__ t, int ldt, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const float* __restrict__ w,
                                                          const float* __restrict__ b, float* __restrict__ z, long P, int C, int L) {
    const int cv = C >> 2, lane = threadIdx.x & (L - 1), ppb = TPB / L;
    const bool own = lane < cv;
    float sc[4], sh[4], wv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = lane * 4 + q;
        sc[q] = own ? scale[c] : 0.f; sh[q] = own ? shift[c] : 0.f; wv[q] = own ? w[c] : 0.f;
    }
    const float bias = b[0];
    for (long base = (long)blockIdx.x * ppb; base < P; base += (long)gridDim.x * ppb) {      // block-uniform bound: every lane reaches the shuffles
        const long p = base + threadIdx.x / L;
        float acc = 0.f;
        if (p < P && own) {
            const float* tp = t + p * ldt;
            const f32x4 v = ld4(tp + lane * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_fmaf(wv[q], fmaxf(bn_pre(v[q], sc[q], sh[q]), 0.f), acc);
            for (int j = lane + L; j < cv; j += L) {                                       // C > 256 only
                const f32x4 u = ld4(tp + j * 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc = __builtin_fmaf(w[j * 4 + q], fmaxf(bn_pre(u[q], scale[j * 4 + q], shift[j * 4 + q]), 0.f), acc);
            }
        }
        for (int o = L >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0 && p < P) z[p] = acc + bias;
    }
}

// ------------------------------------------------------------------------------------------------------------------ x2 + sigmoid
// prob[n][2h][2w] = sigmoid(bilinear x2 (z)); a thread makes four neighbouring outputs of a row (one 16-byte store when 2w is a multiple of 4)
__global__ __launch_bounds__(TPB) void up2_sigmoid_fwd_kernel(const float* __restrict__ z, float* __restrict__ prob, long N, int H, int W) {
    const int Ho = 2 * H, Wo = 2 * W, G = (Wo + 3) >> 2;
    const bool vec = (Wo & 3) == 0;
    const long total = N * Ho * G;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int g = (int)(i % G);
        const long r = i / G;
        const int oy = (int)(r % Ho);
        const float* zp = z + (r / Ho) * H * W;
        int y0, y1;
        float ly0, ly1;
        bilin_src(oy, 0.5f, H, y0, y1, ly0, ly1);
        const float* r0 = zp + (long)y0 * W;
        const float* r1 = zp + (long)y1 * W;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ox = min(4 * g + e, Wo - 1);
            int x0, x1;
            float lx0, lx1;
            bilin_src(ox, 0.5f, W, x0, x1, lx0, lx1);
            v[e] = sigmoidf_(ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (lx0 * r1[x0] + lx1 * r1[x1]));
        }
        float* o = prob + r * Wo + 4 * g;
        if (vec) {
            const f32x4 s = {v[0], v[1], v[2], v[3]};
            st4(o, s);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * g + e < Wo) o[e] = v[e];
        }
    }
}
// dz[n][iy][ix] = sum over the outputs whose taps include (iy, ix) of wy * wx * dprob * prob * (1 - prob): the adjoint in gather form, fixed
// order (rows, then columns); a thread makes four neighbouring dz of a row
__global__ __launch_bounds__(TPB) void up2_sigmoid_bwd_kernel(const float* __restrict__ dprob, const float* __restrict__ prob,
                                                              float* __restrict__ dz, long N, int H, int W) {
    const int Ho = 2 * H, Wo = 2 * W, G = (W + 3) >> 2;
    const bool vec = (W & 3) == 0;
    const long total = N * H * G;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int g = (int)(i % G);
        const long r = i / G;
        const int iy = (int)(r % H);
        const long plane = (r / H) * Ho * Wo;
        int oy_lo, oy_hi;
        upsample_adj_range(iy, 2, Ho, oy_lo, oy_hi);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ix = min(4 * g + e, W - 1);
            int ox_lo, ox_hi;
            upsample_adj_range(ix, 2, Wo, ox_lo, ox_hi);
            float acc = 0.f;
            for (int oy = oy_lo; oy <= oy_hi; ++oy) {
                const float wy = bilin_tap_weight(oy, 0.5f, H, iy);
                if (wy == 0.f) continue;
                float row = 0.f;
                for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                    const float wx = bilin_tap_weight(ox, 0.5f, W, ix);
                    if (wx != 0.f) {
                        const long q = plane + (long)oy * Wo + ox;
                        const float pr = prob[q];
                        row += wx * (dprob[q] * pr * (1.f - pr));
                    }
                }
                acc += wy * row;
            }
            v[e] = acc;
        }
        float* o = dz + r * W + 4 * g;
        if (vec) {
            const f32x4 s = {v[0], v[1], v[2], v[3]};
            st4(o, s);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * g + e < W) o[e] = v[e];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ head, backward
// Layout of the streaming kernels below (as norm_act.hip): a thread owns one channel quad (its coefficients live in registers) and every
// `rows`-th pixel of its block's pixel range.
// One pass over t and dz: per channel  sum g * xhat | sum g | sum dz * relu(y)  and the scalar  sum dz,  with y = t * scale + shift and
// g = dz * w * (y > 0).  part[block][3C + 1] in the order of the final result (dgamma | dbeta | dw | db).
__global__ __launch_bounds__(TPB) void hr_head_bwd_reduce_partial(const float* __restrict__ dz, const float* __restrict__ t, int ldt,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  const float* __restrict__ w, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, long P, int C, long ppc,
                                                                  float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float sm[];       // [rows][3C + 1]
    const int cv = C >> 2, rows = TPB / cv, tid = threadIdx.x;
    const int col = tid % cv, row = tid / cv, width = 3 * C + 1;
    const long p0 = (long)blockIdx.x * ppc;
    const long p1 = p0 + ppc < P ? p0 + ppc : P;
    if (row < rows) {
        float sc[4], sh[4], wv[4], mu[4], is[4], sgx[4], sg[4], sa[4], sd = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = col * 4 + q;
            sc[q] = scale[c]; sh[q] = shift[c]; wv[q] = w[c]; mu[q] = mean[c]; is[q] = invstd[c];
            sgx[q] = 0.f; sg[q] = 0.f; sa[q] = 0.f;
        }
        auto take = [&](const float d, const f32x4 v) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float y = bn_pre(v[q], sc[q], sh[q]);
                const float g = y > 0.f ? d * wv[q] : 0.f;
                sa[q] += d * fmaxf(y, 0.f);
                sg[q] += g;
                sgx[q] += g * (v[q] - mu[q]) * is[q];
            }
            if (col == 0) sd += d;
        };
        long p = p0 + row;
        for (; p + rows < p1; p += 2 * rows) {               // two pixels' loads in flight per thread; same summation order
            const float d0 = dz[p], d1 = dz[p + rows];
            const f32x4 v0 = ld4(t + p * ldt + col * 4);
            const f32x4 v1 = ld4(t + (p + rows) * ldt + col * 4);
            take(d0, v0); take(d1, v1);
        }
        for (; p < p1; p += rows) take(dz[p], ld4(t + p * ldt + col * 4));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = col * 4 + q;
            sm[row * width + c] = sgx[q]; sm[row * width + C + c] = sg[q]; sm[row * width + 2 * C + c] = sa[q];
        }
        if (col == 0) sm[row * width + 3 * C] = sd;
    }
    block_rows_to_part(sm, rows, width, part);
}
// dt = BatchNorm backward (runet_bn_bwd_apply's formula) of g = dz * w * (y > 0), g recomputed; sums = (dgamma | dbeta) as the reduce left them
__global__ __launch_bounds__(TPB) void hr_head_bwd_apply_kernel(const float* __restrict__ dz, const float* __restrict__ t, int ldt,
                                                                const float* __restrict__ w, float* __restrict__ dt, int lddt, long P, int C,
                                                                long ppc, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                const float* __restrict__ sums, float inv_m) {
    const int cv = C >> 2, rows = TPB / cv, tid = threadIdx.x;
    const int col = tid % cv, row = tid / cv;
    if (row >= rows) return;
    const long p0 = (long)blockIdx.x * ppc;
    const long p1 = p0 + ppc < P ? p0 + ppc : P;
    float sc[4], sh[4], wv[4], ca[4], cb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = col * 4 + q;
        sc[q] = scale[c]; sh[q] = shift[c]; wv[q] = w[c];
        bn_bwd_coef(sc[q], mean[c], invstd[c], sums[c], sums[C + c], inv_m, ca[q], cb[q]);
    }
    for (long p = p0 + row; p < p1; p += rows) {
        const float d = dz[p];
        const f32x4 v = ld4(t + p * ldt + col * 4);
        f32x4 r;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float g = bn_pre(v[q], sc[q], sh[q]) > 0.f ? d * wv[q] : 0.f;
            r[q] = bn_bwd_dx(g, sc[q], v[q], ca[q], cb[q]);
        }
        st4(dt + p * lddt + col * 4, r);
    }
}

// ------------------------------------------------------------------------------------------------------------------ fusion branches
// y[n][S h][S w][0:C] = scale * bilinear_S(x) + shift: thread per (output pixel, channel quad), one 16-byte store
template <int S>
__global__ __launch_bounds__(TPB) void bn_bilinear_nhwc_fwd_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy,
                                                                   const float* __restrict__ scale, const float* __restrict__ shift, long N,
                                                                   int H, int W, int C) {
    const int cv = C >> 2, Ho = S * H, Wo = S * W;
    const float inv = 1.f / (float)S;
    const long total = N * Ho * Wo * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int c = (int)(i % cv) * 4;
        const long p = i / cv;
        const int ox = (int)(p % Wo);
        const long r = p / Wo;
        const int oy = (int)(r % Ho);
        const float* xp = x + (r / Ho) * H * W * (long)ldx + c;
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        bilin_src(oy, inv, H, y0, y1, ly0, ly1);
        bilin_src(ox, inv, W, x0, x1, lx0, lx1);
        const f32x4 a = ld4(xp + ((long)y0 * W + x0) * ldx);
        const f32x4 b = ld4(xp + ((long)y0 * W + x1) * ldx);
        const f32x4 d = ld4(xp + ((long)y1 * W + x0) * ldx);
        const f32x4 e = ld4(xp + ((long)y1 * W + x1) * ldx);
        const f32x4 sc = ld4(scale + c);
        const f32x4 sh = ld4(shift + c);
        const f32x4 v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * d + lx1 * e);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = bn_pre(v[q], sc[q], sh[q]);
        st4(y + p * ldy + c, o);
    }
}
// g[n][h][w][0:C] = the adjoint (gather form, fixed order) of the slice gradient dy [n][S h][S w][0:C], and in the same pass the
// BatchNorm-backward partial sums of g against x: part[block][2C] = (sum g * xhat | sum g)
template <int S>
__global__ __launch_bounds__(TPB) void bilinear_nhwc_bwd_sums_partial(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx,
                                                                      const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                      float* __restrict__ g, int ldg, long P, int H, int W, int C, long ppc,
                                                                      float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float sm[];       // [rows][2C]
    const int cv = C >> 2, rows = TPB / cv, tid = threadIdx.x;
    const int col = tid % cv, row = tid / cv, Ho = S * H, Wo = S * W;
    const float inv = 1.f / (float)S;
    const long p0 = (long)blockIdx.x * ppc;
    const long p1 = p0 + ppc < P ? p0 + ppc : P;
    if (row < rows) {
        float mu[4], is[4], sgx[4], sg[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            mu[q] = mean[col * 4 + q]; is[q] = invstd[col * 4 + q];
            sgx[q] = 0.f; sg[q] = 0.f;
        }
        for (long p = p0 + row; p < p1; p += rows) {
            const int ix = (int)(p % W);
            const long r = p / W;
            const int iy = (int)(r % H);
            const float* gp = dy + (r / H) * Ho * Wo * (long)lddy + col * 4;
            const f32x4 xv = ld4(x + p * ldx + col * 4);
            int oy_lo, oy_hi, ox_lo, ox_hi;
            upsample_adj_range(iy, S, Ho, oy_lo, oy_hi);
            upsample_adj_range(ix, S, Wo, ox_lo, ox_hi);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int oy = oy_lo; oy <= oy_hi; ++oy) {
                const float wy = bilin_tap_weight(oy, inv, H, iy);
                if (wy == 0.f) continue;
                f32x4 rsum = {0.f, 0.f, 0.f, 0.f};
                for (int ox = ox_lo; ox <= ox_hi; ++ox) {
                    const float wx = bilin_tap_weight(ox, inv, W, ix);
                    if (wx != 0.f) rsum += wx * ld4(gp + ((long)oy * Wo + ox) * lddy);
                }
                acc += wy * rsum;
            }
            st4(g + p * ldg + col * 4, acc);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sg[q] += acc[q];
                sgx[q] += acc[q] * (xv[q] - mu[q]) * is[q];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sm[row * 2 * C + col * 4 + q] = sgx[q];
            sm[row * 2 * C + C + col * 4 + q] = sg[q];
        }
    }
    block_rows_to_part(sm, rows, 2 * C, part);
}
}  // namespace

#define REQ_HR_C(C) RUNET_REQUIRE((C) >= 4 && (C) <= 1024 && (C) % 4 == 0, "channels must be a multiple of 4, at most 1024")

extern "C" int runet_hr_head_fwd(const float* t, int ldt, const float* scale, const float* shift, const float* w, const float* b, float* z, int n_img,
                                 int h, int w_, int c, void* stream) {
    RUNET_REQUIRE(t && scale && shift && w && b && z, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty shape");
    REQ_HR_C(c);
    RUNET_REQUIRE(ldt >= c && ldt % 4 == 0 && RUNET_ALIGNED16(t), "pixel strides must be multiples of 4 floats that cover the channels, pointers 16-byte aligned");
    int L = 1;
    while (L < c / 4 && L < 64) L <<= 1;
    const long P = (long)n_img * h * w_;
    long blocks = (P + TPB / L - 1) / (TPB / L);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(hr_head_fwd_kernel, dim3((int)blocks), dim3(TPB), 0, (hipStream_t)stream, t, ldt, scale, shift, w, b, z, P, c, L);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_up2_sigmoid_fwd(const float* z, float* prob, int n_img, int h, int w_, void* stream) {
    RUNET_REQUIRE(z && prob, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty shape");
    RUNET_REQUIRE(RUNET_ALIGNED16(prob), "pointers 16-byte aligned");
    hipLaunchKernelGGL(up2_sigmoid_fwd_kernel, dim3(ew_grid((long)n_img * 2 * h * ((2 * w_ + 3) / 4), 4096)), dim3(TPB), 0, (hipStream_t)stream, z, prob,
                       (long)n_img, h, w_);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_up2_sigmoid_bwd(const float* dprob, const float* prob, float* dz, int n_img, int h, int w_, void* stream) {
    RUNET_REQUIRE(dprob && prob && dz, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty shape");
    RUNET_REQUIRE(RUNET_ALIGNED16(dz), "pointers 16-byte aligned");
    hipLaunchKernelGGL(up2_sigmoid_bwd_kernel, dim3(ew_grid((long)n_img * h * ((w_ + 3) / 4), 4096)), dim3(TPB), 0, (hipStream_t)stream, dprob, prob, dz,
                       (long)n_img, h, w_);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_hr_head_bwd_workspace_floats(int n_img, int h, int w_, int c) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || c < 4 || c > 1024 || c % 4) return -1;
    return (long)MAX_PARTS * (3 * c + 1);
}

extern "C" int runet_hr_head_bwd_reduce(const float* dz, const float* t, int ldt, const float* scale, const float* shift, const float* w,
                                        const float* mean, const float* invstd, float* workspace, long workspace_floats, float* out, int n_img,
                                        int h, int w_, int c, void* stream) {
    RUNET_REQUIRE(dz && t && scale && shift && w && mean && invstd && workspace && out, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty shape");
    REQ_HR_C(c);
    RUNET_REQUIRE(ldt >= c && ldt % 4 == 0 && RUNET_ALIGNED16(t), "pixel strides must be multiples of 4 floats that cover the channels, pointers 16-byte aligned");
    const int width = 3 * c + 1, rows = TPB / (c / 4);
    const long P = (long)n_img * h * w_;
    long ppc;
    const int chunks = pixel_chunks(P, c, 16384, MAX_PARTS, ppc);
    RUNET_REQUIRE(workspace_floats >= (long)chunks * width, "workspace too small (runet_hr_head_bwd_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(hr_head_bwd_reduce_partial, dim3(chunks), dim3(TPB), (size_t)rows * width * sizeof(float), st, dz, t, ldt, scale, shift, w, mean,
                       invstd, P, c, ppc, workspace);
    sum_parts<16>(workspace, chunks, width, out, st);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_hr_head_bwd_apply(const float* dz, const float* t, int ldt, const float* w, float* dt, int lddt, int n_img, int h, int w_, int c,
                                       const float* mean, const float* invstd, const float* scale, const float* shift, const float* sums,
                                       long m_total, void* stream) {
    RUNET_REQUIRE(dz && t && w && dt && mean && invstd && scale && shift && sums, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty shape");
    REQ_HR_C(c);
    RUNET_REQUIRE(ldt >= c && ldt % 4 == 0 && lddt >= c && lddt % 4 == 0 && RUNET_ALIGNED16(t) && RUNET_ALIGNED16(dt),
                  "pixel strides must be multiples of 4 floats that cover the channels, pointers 16-byte aligned");
    const long P = (long)n_img * h * w_;
    const float inv_m = 1.0f / (float)(m_total > 0 ? m_total : P);
    long ppc;
    const int chunks = pixel_chunks(P, c, 8192, 8192, ppc);
    hipLaunchKernelGGL(hr_head_bwd_apply_kernel, dim3(chunks), dim3(TPB), 0, (hipStream_t)stream, dz, t, ldt, w, dt, lddt, P, c, ppc, mean, invstd, scale,
                       shift, sums, inv_m);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_bn_bilinear_nhwc_fwd(const float* x, int ldx, float* y, int ldy, const float* scale, const float* shift, int n_img, int h, int w_,
                                          int s, int c, void* stream) {
    RUNET_REQUIRE(x && y && scale && shift, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty shape");
    RUNET_REQUIRE(s == 2 || s == 4, "the scale factor must be 2 or 4");
    REQ_HR_C(c);
    RUNET_REQUIRE(ldx >= c && ldy >= c && ldx % 4 == 0 && ldy % 4 == 0 && RUNET_ALIGNED16(x) && RUNET_ALIGNED16(y) && RUNET_ALIGNED16(scale) && RUNET_ALIGNED16(shift),
                  "pixel strides must be multiples of 4 floats that cover the channels, pointers 16-byte aligned");
    const int grid = ew_grid((long)n_img * s * h * s * w_ * (c / 4), 4096);
    hipStream_t st = (hipStream_t)stream;
    if (s == 2) hipLaunchKernelGGL(bn_bilinear_nhwc_fwd_kernel<2>, dim3(grid), dim3(TPB), 0, st, x, ldx, y, ldy, scale, shift, (long)n_img, h, w_, c);
    else hipLaunchKernelGGL(bn_bilinear_nhwc_fwd_kernel<4>, dim3(grid), dim3(TPB), 0, st, x, ldx, y, ldy, scale, shift, (long)n_img, h, w_, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_bilinear_nhwc_bwd_sums_workspace_floats(int n_img, int h, int w_, int c) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || c < 4 || c > 1024 || c % 4) return -1;
    return (long)MAX_PARTS * 2 * c;
}

extern "C" int runet_bilinear_nhwc_bwd_sums(const float* dy, int lddy, const float* x, int ldx, const float* mean, const float* invstd, float* g, int ldg,
                                            float* workspace, long workspace_floats, float* sums, int n_img, int h, int w_, int s, int c,
                                            void* stream) {
    RUNET_REQUIRE(dy && x && mean && invstd && g && workspace && sums, "null pointer");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty shape");
    RUNET_REQUIRE(s == 2 || s == 4, "the scale factor must be 2 or 4");
    REQ_HR_C(c);
    RUNET_REQUIRE(lddy >= c && ldx >= c && ldg >= c && lddy % 4 == 0 && ldx % 4 == 0 && ldg % 4 == 0 && RUNET_ALIGNED16(dy) && RUNET_ALIGNED16(x) && RUNET_ALIGNED16(g),
                  "pixel strides must be multiples of 4 floats that cover the channels, pointers 16-byte aligned");
    const int rows = TPB / (c / 4);
    const long P = (long)n_img * h * w_;
    long ppc;
    const int chunks = pixel_chunks(P, 1, rows, MAX_PARTS, ppc);         // one pixel per thread while the blocks last: the gather is the heavy part
    RUNET_REQUIRE(workspace_floats >= (long)chunks * 2 * c, "workspace too small (runet_bilinear_nhwc_bwd_sums_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)rows * 2 * c * sizeof(float);
    if (s == 2) hipLaunchKernelGGL(bilinear_nhwc_bwd_sums_partial<2>, dim3(chunks), dim3(TPB), lds, st, dy, lddy, x, ldx, mean, invstd, g, ldg, P, h, w_, c, ppc, workspace);
    else hipLaunchKernelGGL(bilinear_nhwc_bwd_sums_partial<4>, dim3(chunks), dim3(TPB), lds, st, dy, lddy, x, ldx, mean, invstd, g, ldg, P, h, w_, c, ppc, workspace);
    sum_parts<16>(workspace, chunks, 2 * c, sums, st);
    RUNET_CHECK_LAUNCH();
}
