// ENet baseline (comne.py:482-608): the initial block, the bottleneck's tail and the k2-s2 one-channel transposed-convolution head.
//
//   initial  t = (Conv2d 3 -> 13, 3x3 stride 2 padding 1 | MaxPool2d(2)) of the NCHW image in one pass over its 3 x 3 x 3 patches, with the
//            BatchNorm partials (count, mean, M2) of the 16 channels per 256-pixel block; the weight gradient of the 13-column convolution
//            from per-chunk partial slabs
//   tail     out = relu(mask * (t3 * scale3 + shift3) + id), id = idn or idn * scale_d + shift_d (the downsample block's BatchNorm on the raw
//            1x1 convolution of the pooled input): one pass for BatchNorm-apply, Dropout2d, add and ReLU.  Backward in two passes over
//            g = dout where out > 0: the (dgamma | dbeta) sums of one or both BatchNorms (chunk partials -> block_rows_to_part -> sum_parts<16>),
//            then dt3 and either dt_d or g itself.
//   head     prob[n, 2i + a, 2j + b] = sigmoid(bias + sum_c x[n, i, j, c] * w[a][b][c]) and its backward: dx, and (dw [2][2][c] | db) through
//            the same two-stage ordered reduction.
// Layout: a thread owns 4 consecutive channels of a pixel (16-byte accesses), c / 4 threads share a pixel, the remaining thread rows of a
// block walk the block's pixel chunk.  No float atomics; chunk counts depend on the shape only: bitwise reproducible.
#include "runet_common.h"
#include "../../include/runet_hip.h"

namespace {

constexpr int TPB = RUNET_TPB;
constexpr int MAX_PARTS = 1024;      // blocks of a partial reduction (rows of the caller's workspace)

// blocks of a (channel quad x pixel row) streaming kernel over P pixels of C channels: ~`elems` elements per block, at most `cap` blocks
inline int tail_chunks(long P, int C, long elems, int cap, long& ppc) {
    long chunks = (P * C + elems - 1) / elems;
    if (chunks > cap) chunks = cap;
    if (chunks < 1) chunks = 1;
    ppc = (P + chunks - 1) / chunks;
    return (int)((P + ppc - 1) / ppc);
}

// ------------------------------------------------------------------------------------------------------------------ tail, forward
template <bool DOWN>
__global__ __launch_bounds__(TPB) void enet_tail_fwd_kernel(const float* __restrict__ t3, int ldt, const float* __restrict__ idn, int ldi,
                                                            const float* __restrict__ scale3, const float* __restrict__ shift3,
                                                            const float* __restrict__ scale_d, const float* __restrict__ shift_d,
                                                            const float* __restrict__ mask_nc, float* __restrict__ out, int ldo, long P, int HW,
                                                            int C) {
    const int cv = C >> 2;
    const long total = P * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const long p = i / cv;
        const int c = (int)(i - p * cv) * 4;
        const f32x4 tv = ld4(t3 + p * ldt + c), iv = ld4(idn + p * ldi + c), s3 = ld4(scale3 + c), h3 = ld4(shift3 + c);
        f32x4 m = {1.f, 1.f, 1.f, 1.f}, sd = m, hd = m;
        if (mask_nc) m = ld4(mask_nc + (p / HW) * C + c);
        if constexpr (DOWN) { sd = ld4(scale_d + c); hd = ld4(shift_d + c); }
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v = bn_pre(tv[q], s3[q], h3[q]);
            if (mask_nc) v *= m[q];
            const float id = DOWN ? bn_pre(iv[q], sd[q], hd[q]) : iv[q];
            const float r = v + id;
            o[q] = r > 0.f ? r : 0.f;
        }
        st4(out + p * ldo + c, o);
    }
}

// ------------------------------------------------------------------------------------------------------------------ tail, backward sums
// part[block][(2 | 4) C] = (sum g m xhat3 | sum g m [| sum g xhat_d | sum g]) over the block's pixel chunk
template <bool DOWN>
__global__ __launch_bounds__(TPB) void enet_tail_bwd_partial(const float* __restrict__ dout, int lddo, const float* __restrict__ out, int ldo,
                                                             const float* __restrict__ t3, int ldt, const float* __restrict__ idn, int ldi,
                                                             const float* __restrict__ mean3, const float* __restrict__ invstd3,
                                                             const float* __restrict__ mean_d, const float* __restrict__ invstd_d,
                                                             const float* __restrict__ mask_nc, long P, int HW, int C, long ppc,
                                                             float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float sm[];       // [rows][width]
    constexpr int NV = DOWN ? 4 : 2;
    const int cv = C >> 2, rows = TPB / cv, tid = threadIdx.x, width = NV * C;
    const int col = tid % cv, row = tid / cv, c = col * 4;
    const long p0 = (long)blockIdx.x * ppc;
    const long p1 = p0 + ppc < P ? p0 + ppc : P;
    if (row < rows) {
        float acc[NV][4];
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[v][q] = 0.f;
        const f32x4 mu3 = ld4(mean3 + c), is3 = ld4(invstd3 + c);
        f32x4 mud = mu3, isd = is3;
        if constexpr (DOWN) { mud = ld4(mean_d + c); isd = ld4(invstd_d + c); }
        for (long p = p0 + row; p < p1; p += rows) {
            const f32x4 dv = ld4(dout + p * lddo + c), ov = ld4(out + p * ldo + c), tv = ld4(t3 + p * ldt + c);
            f32x4 m = {1.f, 1.f, 1.f, 1.f}, iv = m;
            if (mask_nc) m = ld4(mask_nc + (p / HW) * C + c);
            if constexpr (DOWN) iv = ld4(idn + p * ldi + c);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float g = ov[q] > 0.f ? dv[q] : 0.f;
                const float gm = mask_nc ? g * m[q] : g;
                acc[0][q] += gm * ((tv[q] - mu3[q]) * is3[q]);
                acc[1][q] += gm;
                if constexpr (DOWN) {
                    acc[2][q] += g * ((iv[q] - mud[q]) * isd[q]);
                    acc[3][q] += g;
                }
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int q = 0; q < 4; ++q) sm[row * width + v * C + c + q] = acc[v][q];
    }
    block_rows_to_part(sm, rows, width, part);
}

// ------------------------------------------------------------------------------------------------------------------ tail, backward apply
template <bool DOWN>
__global__ __launch_bounds__(TPB) void enet_tail_bwd_apply_kernel(const float* __restrict__ dout, int lddo, const float* __restrict__ out, int ldo,
                                                                  const float* __restrict__ t3, int ldt, const float* __restrict__ idn, int ldi,
                                                                  const float* __restrict__ mean3, const float* __restrict__ invstd3,
                                                                  const float* __restrict__ scale3, const float* __restrict__ mean_d,
                                                                  const float* __restrict__ invstd_d, const float* __restrict__ scale_d,
                                                                  const float* __restrict__ mask_nc, const float* __restrict__ sums, float inv_m,
                                                                  float* __restrict__ dt3, int lddt, float* __restrict__ did, int lddi, long P,
                                                                  int HW, int C) {
    const int cv = C >> 2;
    const long total = P * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const long p = i / cv;
        const int c = (int)(i - p * cv) * 4;
        const f32x4 dv = ld4(dout + p * lddo + c), ov = ld4(out + p * ldo + c), tv = ld4(t3 + p * ldt + c), s3 = ld4(scale3 + c);
        const f32x4 mu3 = ld4(mean3 + c), is3 = ld4(invstd3 + c), sgx3 = ld4(sums + c), sg3 = ld4(sums + C + c);
        f32x4 m = {1.f, 1.f, 1.f, 1.f}, iv = m, sd = m, mud = m, isd = m, sgxd = m, sgd = m;
        if (mask_nc) m = ld4(mask_nc + (p / HW) * C + c);
        if constexpr (DOWN) {
            iv = ld4(idn + p * ldi + c); sd = ld4(scale_d + c); mud = ld4(mean_d + c); isd = ld4(invstd_d + c);
            sgxd = ld4(sums + 2 * C + c); sgd = ld4(sums + 3 * C + c);
        }
        f32x4 o3, od;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float g = ov[q] > 0.f ? dv[q] : 0.f;
            const float gm = mask_nc ? g * m[q] : g;
            float ca, cb;
            bn_bwd_coef(s3[q], mu3[q], is3[q], sgx3[q], sg3[q], inv_m, ca, cb);
            o3[q] = bn_bwd_dx(gm, s3[q], tv[q], ca, cb);
            if constexpr (DOWN) {
                bn_bwd_coef(sd[q], mud[q], isd[q], sgxd[q], sgd[q], inv_m, ca, cb);
                od[q] = bn_bwd_dx(g, sd[q], iv[q], ca, cb);
            } else od[q] = g;
        }
        st4(dt3 + p * lddt + c, o3);
        st4(did + p * lddi + c, od);
    }
}

// ------------------------------------------------------------------------------------------------------------------ head, forward
// one thread per input pixel: the four taps' dot products over the channels in channel order, two 8-byte stores
__global__ __launch_bounds__(TPB) void enet_head_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ prob, long P, int H, int W, int C) {
    const float b = bias[0];
    for (long p = (long)blockIdx.x * TPB + threadIdx.x; p < P; p += (long)gridDim.x * TPB) {
        float z[4] = {b, b, b, b};
        const float* xp = x + p * ldx;
        for (int c = 0; c < C; c += 4) {
            const f32x4 xv = ld4(xp + c);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 wv = ld4(w + t * C + c);
#pragma unroll
                for (int q = 0; q < 4; ++q) z[t] = __builtin_fmaf(xv[q], wv[q], z[t]);
            }
        }
        const int j = (int)(p % W);
        const long r = p / W;                         // n * H + i
        float* o = prob + (2 * r) * (2L * W) + 2 * j;
        *reinterpret_cast<float2*>(o) = make_float2(sigmoidf_(z[0]), sigmoidf_(z[1]));
        *reinterpret_cast<float2*>(o + 2L * W) = make_float2(sigmoidf_(z[2]), sigmoidf_(z[3]));
    }
}

// ------------------------------------------------------------------------------------------------------------------ head, backward
// dz = dprob p (1 - p); dx = sum_ab dz_ab w_ab; part[block][4 C + 1] = (sum dz_ab x | sum dz) over the block's pixel chunk
__global__ __launch_bounds__(TPB) void enet_head_bwd_partial(const float* __restrict__ dprob, const float* __restrict__ prob,
                                                             const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                             float* __restrict__ dx, int lddx, long P, int H, int W, int C, long ppc,
                                                             float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float sm[];       // [rows][4 C + 1]
    const int cv = C >> 2, rows = TPB / cv, tid = threadIdx.x, width = 4 * C + 1;
    const int col = tid % cv, row = tid / cv, c = col * 4;
    const long p0 = (long)blockIdx.x * ppc;
    const long p1 = p0 + ppc < P ? p0 + ppc : P;
    if (row < rows) {
        float acc[4][4], sdz = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[t][q] = 0.f;
        f32x4 wv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) wv[t] = ld4(w + t * C + c);
        for (long p = p0 + row; p < p1; p += rows) {
            const int j = (int)(p % W);
            const long r = p / W;
            const long o = (2 * r) * (2L * W) + 2 * j;
            const float2 d0 = *reinterpret_cast<const float2*>(dprob + o), d1 = *reinterpret_cast<const float2*>(dprob + o + 2L * W);
            const float2 q0 = *reinterpret_cast<const float2*>(prob + o), q1 = *reinterpret_cast<const float2*>(prob + o + 2L * W);
            const float dz[4] = {d0.x * q0.x * (1.f - q0.x), d0.y * q0.y * (1.f - q0.y), d1.x * q1.x * (1.f - q1.x), d1.y * q1.y * (1.f - q1.y)};
            const f32x4 xv = ld4(x + p * ldx + c);
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    g[q] = __builtin_fmaf(dz[t], wv[t][q], g[q]);
                    acc[t][q] = __builtin_fmaf(dz[t], xv[q], acc[t][q]);
                }
            }
            st4(dx + p * lddx + c, g);
            sdz += (dz[0] + dz[1]) + (dz[2] + dz[3]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) sm[row * width + t * C + c + q] = acc[t][q];
        if (col == 0) sm[row * width + 4 * C] = sdz;
    }
    block_rows_to_part(sm, rows, width, part);
}

// ------------------------------------------------------------------------------------------------------------------ initial block
// One thread per output pixel: the 3 x 3 x 3 patch of the NCHW image (zero padding on the top / left edge; H and W are even, so the bottom /
// right taps are always inside) feeds the 13 convolution outputs, taps in (r, s, channel) order, and its lower-right 2 x 2 x 3 corner is the
// pool window.  The tile's 16-channel outputs pass through LDS for the BatchNorm partials: 16 row-lanes per channel, two passes (mean, then
// M2 about it), the lane sums added in lane order.
constexpr int INI_TILE = 256;        // output pixels per block = threads per block
constexpr int INI_W = 3 * 3 * 3 * 13;

__device__ __forceinline__ void initial_patch(const float* __restrict__ x, long sn, long sc, long sh, long sw, long p, int Ho, int Wo, int H, int W,
                                              float (&v)[27]) {
    const int j = (int)(p % Wo);
    const long r = p / Wo;
    const int i = (int)(r % Ho);
    const float* xb = x + (r / Ho) * sn;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int yy = 2 * i - 1 + a;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int xx = 2 * j - 1 + b;
            const bool ok = yy >= 0 && xx >= 0 && yy < H && xx < W;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[(a * 3 + b) * 3 + c] = ok ? xb[c * sc + yy * sh + xx * sw] : 0.f;
        }
    }
}

__global__ __launch_bounds__(INI_TILE) void enet_initial_fwd_kernel(const float* __restrict__ x, long sn, long sc, long sh, long sw,
                                                                    const float* __restrict__ w, float* __restrict__ t, int ldt,
                                                                    float* __restrict__ part, long P, int Ho, int Wo) {
    __shared__ float Wl[INI_W + 1];
    __shared__ float Tl[INI_TILE][17];
    __shared__ float red[16][16];
    const int tid = threadIdx.x;
    for (int i = tid; i < INI_W; i += INI_TILE) Wl[i] = w[i];
    __syncthreads();
    const long p0 = (long)blockIdx.x * INI_TILE, p = p0 + tid;
    const int valid = (int)(P - p0 < INI_TILE ? P - p0 : INI_TILE);
    if (tid < valid) {
        float v[27], o[16];
        initial_patch(x, sn, sc, sh, sw, p, Ho, Wo, 2 * Ho, 2 * Wo, v);
#pragma unroll
        for (int q = 0; q < 13; ++q) o[q] = 0.f;
#pragma unroll
        for (int k = 0; k < 27; ++k)
#pragma unroll
            for (int q = 0; q < 13; ++q) o[q] = __builtin_fmaf(v[k], Wl[k * 13 + q], o[q]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {          // MaxPool2d(2) over patch rows / columns 1..2; a NaN wins, as in ATen
            float m = v[(1 * 3 + 1) * 3 + c];
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const float u = v[((1 + (k >> 1)) * 3 + 1 + (k & 1)) * 3 + c];
                m = (u > m || u != u) ? u : m;
            }
            o[13 + c] = m;
        }
#pragma unroll
        for (int q = 0; q < 16; q += 4) {
            const f32x4 ov = {o[q], o[q + 1], o[q + 2], o[q + 3]};
            st4(t + p * ldt + q, ov);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) Tl[tid][q] = o[q];
    }
    __syncthreads();
    const int c = tid & 15, r = tid >> 4;
    float s = 0.f;
    for (int m = r; m < valid; m += 16) s += Tl[m][c];
    red[r][c] = s;
    __syncthreads();
    float tot = 0.f;
    for (int k = 0; k < 16; ++k) tot += red[k][c];
    const float mean = tot / (float)valid;
    __syncthreads();
    float m2 = 0.f;
    for (int m = r; m < valid; m += 16) {
        const float d = Tl[m][c] - mean;
        m2 = __builtin_fmaf(d, d, m2);
    }
    red[r][c] = m2;
    __syncthreads();
    if (tid < 16) {
        float q = 0.f;
        for (int k = 0; k < 16; ++k) q += red[k][tid];
        float* o = part + ((long)blockIdx.x * 16 + tid) * 3;
        o[0] = (float)valid; o[1] = mean; o[2] = q;
    }
}

// dw[k][o] = sum_p patch[p][k] dt[p][o] (k = 27 taps x channels, o = 13): thread (k, o) walks the block's pixel chunk through LDS tiles of
// 64 pixels; part[block][351], added in block order by sum_parts<16>.
constexpr int INI_WG_TPB = 384, INI_WG_TILE = 64;

__global__ __launch_bounds__(INI_WG_TPB) void enet_initial_wgrad_partial(const float* __restrict__ x, long sn, long sc, long sh, long sw,
                                                                         const float* __restrict__ dt, int lddt, long P, int Ho, int Wo,
                                                                         long ppc, float* __restrict__ part) {
    __shared__ float Xl[INI_WG_TILE][28];
    __shared__ float Gl[INI_WG_TILE][13];
    const int tid = threadIdx.x;
    const int k = tid / 13, o = tid - k * 13;
    const long c0 = (long)blockIdx.x * ppc;
    const long c1 = c0 + ppc < P ? c0 + ppc : P;
    float acc = 0.f;
    for (long p0 = c0; p0 < c1; p0 += INI_WG_TILE) {
        const int valid = (int)(c1 - p0 < INI_WG_TILE ? c1 - p0 : INI_WG_TILE);
        __syncthreads();
        if (tid < valid) {
            float v[27];
            initial_patch(x, sn, sc, sh, sw, p0 + tid, Ho, Wo, 2 * Ho, 2 * Wo, v);
#pragma unroll
            for (int q = 0; q < 27; ++q) Xl[tid][q] = v[q];
        }
        for (int i = tid; i < valid * 13; i += INI_WG_TPB) {
            const int m = i / 13, q = i - m * 13;
            Gl[m][q] = dt[(p0 + m) * lddt + q];
        }
        __syncthreads();
        if (tid < INI_W)
            for (int m = 0; m < valid; ++m) acc = __builtin_fmaf(Xl[m][k], Gl[m][o], acc);
    }
    if (tid < INI_W) part[(long)blockIdx.x * INI_W + tid] = acc;
}

inline int initial_chunks(long P, long& ppc) {
    ppc = (P + MAX_PARTS - 1) / MAX_PARTS;
    if (ppc < 4 * INI_WG_TILE) ppc = 4 * INI_WG_TILE;
    ppc = (ppc + INI_WG_TILE - 1) / INI_WG_TILE * INI_WG_TILE;
    return (int)((P + ppc - 1) / ppc);
}

}  // namespace

#define REQ_ENET_IMAGE(n, h, w) RUNET_REQUIRE((n) > 0 && (h) > 0 && (w) > 0 && (h) % 2 == 0 && (w) % 2 == 0, "bad shape (H and W positive and even)")

extern "C" int runet_enet_initial_parts(int n_img, int h, int w_) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || h % 2 || w_ % 2) return -1;
    return cdiv((long)n_img * (h / 2) * (w_ / 2), INI_TILE);
}

extern "C" int runet_enet_initial_fwd(const float* x, long sn, long sc, long sh, long sw, const float* w, float* t, int ldt, float* part, int n_img,
                                      int h, int w_, void* stream) {
    RUNET_REQUIRE(x && w && t && part, "null pointer");
    REQ_ENET_IMAGE(n_img, h, w_);
    RUNET_REQ_LD(ldt, 16, t);
    const long P = (long)n_img * (h / 2) * (w_ / 2);
    hipLaunchKernelGGL(enet_initial_fwd_kernel, dim3(cdiv(P, INI_TILE)), dim3(INI_TILE), 0, (hipStream_t)stream, x, sn, sc, sh, sw, w, t, ldt, part, P,
                       h / 2, w_ / 2);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_enet_initial_wgrad_workspace_floats(int n_img, int h, int w_) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || h % 2 || w_ % 2) return -1;
    long ppc;
    return (long)initial_chunks((long)n_img * (h / 2) * (w_ / 2), ppc) * INI_W;
}

extern "C" int runet_enet_initial_wgrad(const float* x, long sn, long sc, long sh, long sw, const float* dt, int lddt, float* workspace,
                                        long workspace_floats, float* dw, int n_img, int h, int w_, void* stream) {
    RUNET_REQUIRE(x && dt && workspace && dw, "null pointer");
    REQ_ENET_IMAGE(n_img, h, w_);
    RUNET_REQ_LD(lddt, 16, dt);
    const long P = (long)n_img * (h / 2) * (w_ / 2);
    long ppc;
    const int chunks = initial_chunks(P, ppc);
    RUNET_REQUIRE(workspace_floats >= (long)chunks * INI_W, "workspace too small (runet_enet_initial_wgrad_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(enet_initial_wgrad_partial, dim3(chunks), dim3(INI_WG_TPB), 0, st, x, sn, sc, sh, sw, dt, lddt, P, h / 2, w_ / 2, ppc, workspace);
    sum_parts<16>(workspace, chunks, INI_W, dw, st);
    RUNET_CHECK_LAUNCH();
}

#define REQ_ENET_C(C) RUNET_REQUIRE((C) >= 4 && (C) <= 1024 && (C) % 4 == 0, "channels must be a multiple of 4, at most 1024")
#define REQ_ENET_SHAPE(n, h, w) RUNET_REQUIRE((n) > 0 && (h) > 0 && (w) > 0, "empty shape")

extern "C" int runet_enet_tail_fwd(const float* t3, int ldt, const float* idn, int ldi, const float* scale3, const float* shift3,
                                   const float* scale_d, const float* shift_d, const float* mask_nc, float* out, int ldo, int n_img, int h,
                                   int w_, int c, void* stream) {
    RUNET_REQUIRE(t3 && idn && scale3 && shift3 && out, "null pointer");
    RUNET_REQUIRE((scale_d == nullptr) == (shift_d == nullptr), "scale_d and shift_d come together (the downsample block) or not at all");
    REQ_ENET_SHAPE(n_img, h, w_);
    REQ_ENET_C(c);
    RUNET_REQ_LD(ldt, c, t3);
    RUNET_REQ_LD(ldi, c, idn);
    RUNET_REQ_LD(ldo, c, out);
    RUNET_REQUIRE(RUNET_ALIGNED16(scale3) && RUNET_ALIGNED16(shift3) && RUNET_ALIGNED16(scale_d) && RUNET_ALIGNED16(shift_d) && RUNET_ALIGNED16(mask_nc),
                  "per-channel vectors 16-byte aligned");
    const long P = (long)n_img * h * w_;
    const int grid = ew_grid(P * (c / 4), 4096);
    hipStream_t st = (hipStream_t)stream;
    if (scale_d)
        hipLaunchKernelGGL(enet_tail_fwd_kernel<true>, dim3(grid), dim3(TPB), 0, st, t3, ldt, idn, ldi, scale3, shift3, scale_d, shift_d, mask_nc, out, ldo,
                           P, h * w_, c);
    else
        hipLaunchKernelGGL(enet_tail_fwd_kernel<false>, dim3(grid), dim3(TPB), 0, st, t3, ldt, idn, ldi, scale3, shift3, scale_d, shift_d, mask_nc, out, ldo,
                           P, h * w_, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_enet_tail_bwd_workspace_floats(int n_img, int h, int w_, int c, int downsample) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || c < 4 || c > 1024 || c % 4) return -1;
    long ppc;
    return (long)tail_chunks((long)n_img * h * w_, c, 16384, MAX_PARTS, ppc) * (downsample ? 4 : 2) * c;
}

extern "C" int runet_enet_tail_bwd_reduce(const float* dout, int lddo, const float* out, int ldo, const float* t3, int ldt, const float* idn, int ldi,
                                          const float* mean3, const float* invstd3, const float* mean_d, const float* invstd_d,
                                          const float* mask_nc, float* workspace, long workspace_floats, float* sums, int n_img, int h, int w_,
                                          int c, void* stream) {
    RUNET_REQUIRE(dout && out && t3 && mean3 && invstd3 && workspace && sums, "null pointer");
    RUNET_REQUIRE((mean_d == nullptr) == (invstd_d == nullptr) && (mean_d == nullptr || idn != nullptr),
                  "mean_d, invstd_d and idn come together (the downsample block) or not at all");
    REQ_ENET_SHAPE(n_img, h, w_);
    REQ_ENET_C(c);
    RUNET_REQ_LD(lddo, c, dout);
    RUNET_REQ_LD(ldo, c, out);
    RUNET_REQ_LD(ldt, c, t3);
    if (mean_d) RUNET_REQ_LD(ldi, c, idn);
    RUNET_REQUIRE(RUNET_ALIGNED16(mean3) && RUNET_ALIGNED16(invstd3) && RUNET_ALIGNED16(mean_d) && RUNET_ALIGNED16(invstd_d) && RUNET_ALIGNED16(mask_nc),
                  "per-channel vectors 16-byte aligned");
    const int nv = mean_d ? 4 : 2, width = nv * c, rows = TPB / (c / 4);
    const long P = (long)n_img * h * w_;
    long ppc;
    const int chunks = tail_chunks(P, c, 16384, MAX_PARTS, ppc);
    RUNET_REQUIRE(workspace_floats >= (long)chunks * width, "workspace too small (runet_enet_tail_bwd_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)rows * width * sizeof(float);
    if (mean_d)
        hipLaunchKernelGGL(enet_tail_bwd_partial<true>, dim3(chunks), dim3(TPB), lds, st, dout, lddo, out, ldo, t3, ldt, idn, ldi, mean3, invstd3, mean_d,
                           invstd_d, mask_nc, P, h * w_, c, ppc, workspace);
    else
        hipLaunchKernelGGL(enet_tail_bwd_partial<false>, dim3(chunks), dim3(TPB), lds, st, dout, lddo, out, ldo, t3, ldt, idn, ldi, mean3, invstd3, mean_d,
                           invstd_d, mask_nc, P, h * w_, c, ppc, workspace);
    sum_parts<16>(workspace, chunks, width, sums, st);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_enet_tail_bwd_apply(const float* dout, int lddo, const float* out, int ldo, const float* t3, int ldt, const float* idn, int ldi,
                                         const float* mean3, const float* invstd3, const float* scale3, const float* mean_d, const float* invstd_d,
                                         const float* scale_d, const float* mask_nc, const float* sums, long m_total, float* dt3, int lddt,
                                         float* did, int lddi, int n_img, int h, int w_, int c, void* stream) {
    RUNET_REQUIRE(dout && out && t3 && mean3 && invstd3 && scale3 && sums && dt3 && did, "null pointer");
    RUNET_REQUIRE((mean_d == nullptr) == (invstd_d == nullptr) && (mean_d == nullptr) == (scale_d == nullptr) && (mean_d == nullptr || idn != nullptr),
                  "mean_d, invstd_d, scale_d and idn come together (the downsample block) or not at all");
    REQ_ENET_SHAPE(n_img, h, w_);
    REQ_ENET_C(c);
    RUNET_REQ_LD(lddo, c, dout);
    RUNET_REQ_LD(ldo, c, out);
    RUNET_REQ_LD(ldt, c, t3);
    if (mean_d) RUNET_REQ_LD(ldi, c, idn);
    RUNET_REQ_LD(lddt, c, dt3);
    RUNET_REQ_LD(lddi, c, did);
    RUNET_REQUIRE(RUNET_ALIGNED16(mean3) && RUNET_ALIGNED16(invstd3) && RUNET_ALIGNED16(scale3) && RUNET_ALIGNED16(mean_d) && RUNET_ALIGNED16(invstd_d) &&
                      RUNET_ALIGNED16(scale_d) && RUNET_ALIGNED16(mask_nc) && RUNET_ALIGNED16(sums),
                  "per-channel vectors 16-byte aligned");
    const long P = (long)n_img * h * w_;
    const float inv_m = 1.0f / (float)(m_total > 0 ? m_total : P);
    const int grid = ew_grid(P * (c / 4), 4096);
    hipStream_t st = (hipStream_t)stream;
    if (mean_d)
        hipLaunchKernelGGL(enet_tail_bwd_apply_kernel<true>, dim3(grid), dim3(TPB), 0, st, dout, lddo, out, ldo, t3, ldt, idn, ldi, mean3, invstd3, scale3,
                           mean_d, invstd_d, scale_d, mask_nc, sums, inv_m, dt3, lddt, did, lddi, P, h * w_, c);
    else
        hipLaunchKernelGGL(enet_tail_bwd_apply_kernel<false>, dim3(grid), dim3(TPB), 0, st, dout, lddo, out, ldo, t3, ldt, idn, ldi, mean3, invstd3, scale3,
                           mean_d, invstd_d, scale_d, mask_nc, sums, inv_m, dt3, lddt, did, lddi, P, h * w_, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_enet_head_fwd(const float* x, int ldx, const float* w, const float* bias, float* prob, int n_img, int h, int w_, int c,
                                   void* stream) {
    RUNET_REQUIRE(x && w && bias && prob, "null pointer");
    REQ_ENET_SHAPE(n_img, h, w_);
    REQ_ENET_C(c);
    RUNET_REQ_LD(ldx, c, x);
    RUNET_REQUIRE(RUNET_ALIGNED16(w) && RUNET_ALIGNED16(prob), "w and prob 16-byte aligned");
    const long P = (long)n_img * h * w_;
    hipLaunchKernelGGL(enet_head_fwd_kernel, dim3(ew_grid(P, 8192)), dim3(TPB), 0, (hipStream_t)stream, x, ldx, w, bias, prob, P, h, w_, c);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_enet_head_bwd_workspace_floats(int n_img, int h, int w_, int c) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || c < 4 || c > 1024 || c % 4) return -1;
    long ppc;
    return (long)tail_chunks((long)n_img * h * w_, c, 4096, MAX_PARTS, ppc) * (4 * c + 1);
}

extern "C" int runet_enet_head_bwd(const float* dprob, const float* prob, const float* x, int ldx, const float* w, float* dx, int lddx,
                                   float* workspace, long workspace_floats, float* dw_db, int n_img, int h, int w_, int c, void* stream) {
    RUNET_REQUIRE(dprob && prob && x && w && dx && workspace && dw_db, "null pointer");
    REQ_ENET_SHAPE(n_img, h, w_);
    REQ_ENET_C(c);
    RUNET_REQ_LD(ldx, c, x);
    RUNET_REQ_LD(lddx, c, dx);
    RUNET_REQUIRE(RUNET_ALIGNED16(w) && RUNET_ALIGNED16(dprob) && RUNET_ALIGNED16(prob), "w, dprob and prob 16-byte aligned");
    const int width = 4 * c + 1, rows = TPB / (c / 4);
    const long P = (long)n_img * h * w_;
    long ppc;
    const int chunks = tail_chunks(P, c, 4096, MAX_PARTS, ppc);
    RUNET_REQUIRE(workspace_floats >= (long)chunks * width, "workspace too small (runet_enet_head_bwd_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(enet_head_bwd_partial, dim3(chunks), dim3(TPB), (size_t)rows * width * sizeof(float), st, dprob, prob, x, ldx, w, dx, lddx, P, h,
                       w_, c, ppc, workspace);
    sum_parts<16>(workspace, chunks, width, dw_db, st);
    RUNET_CHECK_LAUNCH();
}
