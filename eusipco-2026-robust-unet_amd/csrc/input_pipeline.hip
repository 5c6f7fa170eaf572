// Device-resident input pipeline (include/runet_hip.h, "device-resident dataset"): PIL's 8-bit resampling passes, the mask's nearest gather,
// and the batch assembly with the training augmentation of train_water_segmentation.py:313-321 (flip, rotation, colour jitter, ToTensor,
// Normalize) from a byte cache.  Everything here is exact against PIL: integer arithmetic where PIL uses integers, single float32 operations
// with no contraction where it uses floats.  Tables (resampling bounds and coefficients, nearest indices, rotation words) are made on the
// host in double precision; the kernels only apply them, and clamp what they read from a table so that a bad table cannot leave the source.
// Byte-streaming, memory-bound kernels: no scratch, the reused tables in LDS, 4- and 16-byte stores where the address allows.
#include "runet_common.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int TPB = 256;
constexpr int PRECISION_BITS = 22;
constexpr int MAX_TAPS = 255;
constexpr int MAX_SIDE = 4096;
constexpr int GS_BLOCKS = 32;                             // runet_batch_gray_sums: blocks per sample

// PIL's clip8: clamp(v >> 22, 0, 255) with an arithmetic shift.  Written as clamp-then-shift (the same value: v < 0 -> 0, v >= 256 << 22 ->
// 255): for two neighbouring shift-then-clamp results that are packed into a word the compiler selects v_ashr_pk_u8_i32 and ORs further
// bytes into its destination's upper half, which on the MI355X was not zero after that instruction (wrong bytes 2 and 3 of the word).
__device__ __forceinline__ unsigned int clip8(int v) {
    v = max(v, 0);
    v = min(v, (256 << PRECISION_BITS) - 1);
    return (unsigned int)v >> PRECISION_BITS;
}

// ---- horizontal pass: dst[y][xx][c] = clip8(2^21 + sum_t coeffs[xx][t] * src[y][xmin(xx) + t][c]) ------------------------------------------
// A block takes RW consecutive outputs of a row band: their coefficient rows are staged once in LDS (row stride ksize is odd, so the RW
// lanes of a tap hit distinct banks) and reused for every row of the band.  Lane = output pixel, all C channels.
constexpr int RW = 64;
constexpr int RROWS = TPB / RW;
template <int C>
__global__ __launch_bounds__(TPB) void resample_rows_kernel(const unsigned char* __restrict__ src, int h, int w_in, const int* __restrict__ bounds,
                                                            const int* __restrict__ coeffs, int ksize, unsigned char* __restrict__ dst, int w_out,
                                                            int band) {
    extern __shared__ int sk[];                             // [RW][ksize]
    const int x0 = blockIdx.x * RW;
    const int nx = min(RW, w_out - x0);
    for (int i = threadIdx.x; i < nx * ksize; i += TPB) sk[i] = coeffs[(long)x0 * ksize + i];
    __syncthreads();
    const int lx = threadIdx.x % RW, ly = threadIdx.x / RW;
    if (lx >= nx) return;
    const int xx = x0 + lx;
    int xmin = bounds[2 * xx], cnt = bounds[2 * xx + 1];
    xmin = min(max(xmin, 0), w_in);
    cnt = min(min(max(cnt, 0), ksize), w_in - xmin);
    const int* k = sk + lx * ksize;
    const int y0 = blockIdx.y * band, y1 = min(h, y0 + band);
    for (int y = y0 + ly; y < y1; y += RROWS) {
        const unsigned char* p = src + ((long)y * w_in + xmin) * C;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) {
            const int kv = k[t];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += kv * (int)p[t * C + c];
        }
        unsigned char* q = dst + ((long)y * w_out + xx) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = (unsigned char)clip8(acc[c]);
    }
}

// ---- vertical pass over rows of `rowbytes` = w * C bytes: dst[yy][i] = clip8(2^21 + sum_t coeffs[yy][t] * src[ymin(yy) + t][i]) -------------
// One output row per blockIdx.y; a lane takes 4 consecutive bytes of it.  The coefficient row is uniform over the block and staged in LDS
// (every lane reads the same word: a broadcast).  Source rows may start at any byte address, so the 4 bytes are read one by one (the lanes
// of a wave still cover 256 consecutive bytes per load); the result is stored as one word when the destination address allows.
__global__ __launch_bounds__(TPB) void resample_cols_kernel(const unsigned char* __restrict__ src, int h_in, long rowbytes, const int* __restrict__ bounds,
                                                            const int* __restrict__ coeffs, int ksize, unsigned char* __restrict__ dst) {
    __shared__ int sk[MAX_TAPS + 1];
    const int yy = blockIdx.y;
    for (int i = threadIdx.x; i < ksize; i += TPB) sk[i] = coeffs[(long)yy * ksize + i];
    __syncthreads();
    int ymin = bounds[2 * yy], cnt = bounds[2 * yy + 1];
    ymin = min(max(ymin, 0), h_in);
    cnt = min(min(max(cnt, 0), ksize), h_in - ymin);
    unsigned char* drow = dst + (long)yy * rowbytes;
    const unsigned int lead = (unsigned int)((4 - ((uintptr_t)drow & 3)) & 3);       // bytes in front of the first aligned word of the row
    // item 0: the `lead` bytes; item j >= 1: the aligned word j - 1 behind them (the last one may be partial)
    const long items = 1 + (rowbytes > lead ? (rowbytes - lead + 3) / 4 : 0);
    for (long j = (long)blockIdx.x * TPB + threadIdx.x; j < items; j += (long)gridDim.x * TPB) {
        const long b0 = j == 0 ? 0 : lead + 4 * (j - 1);
        const int nb = (int)min((long)(j == 0 ? lead : 4), rowbytes - b0);
        if (nb <= 0) continue;
        int acc[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = 1 << (PRECISION_BITS - 1);
        const unsigned char* p = src + (long)ymin * rowbytes + b0;
        if (nb == 4) {
            for (int t = 0; t < cnt; ++t, p += rowbytes) {
                const int kv = sk[t];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += kv * (int)p[e];
            }
            *reinterpret_cast<unsigned int*>(drow + b0) = clip8(acc[0]) | clip8(acc[1]) << 8 | clip8(acc[2]) << 16 | clip8(acc[3]) << 24;
        } else {
            for (int t = 0; t < cnt; ++t, p += rowbytes) {
                const int kv = sk[t];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nb) acc[e] += kv * (int)p[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < nb) drow[b0 + e] = (unsigned char)clip8(acc[e]);
        }
    }
}

// ---- dst[y][x] = src[ytab[y]][xtab[x]] on one plane (the mask's NEAREST resize); a lane takes 4 consecutive bytes of the dense output -------
__global__ __launch_bounds__(TPB) void gather2d_kernel(const unsigned char* __restrict__ src, int sh, int sw, const int* __restrict__ ytab,
                                                       const int* __restrict__ xtab, unsigned char* __restrict__ dst, int dw, long total) {
    for (long i = ((long)blockIdx.x * TPB + threadIdx.x) * 4; i < total; i += (long)gridDim.x * TPB * 4) {
        unsigned int v[4];
        const int n = (int)min(4L, total - i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = 0;
            if (e < n) {
                const long y = (i + e) / dw;
                const int x = (int)(i + e - y * dw);
                const int sy = min(max(ytab[y], 0), sh - 1), sx = min(max(xtab[x], 0), sw - 1);
                v[e] = src[(long)sy * sw + sx];
            }
        }
        if (n == 4) *reinterpret_cast<unsigned int*>(dst + i) = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;       // dst 4-byte aligned (entry)
        else
            for (int e = 0; e < n; ++e) dst[i + e] = (unsigned char)v[e];
    }
}

// ---- the augmentation of one pixel, shared by the sums and the assembly --------------------------------------------------------------------
// geom[b] = {flip, a0, a1, a2, a3, a4, a5, order}: the source of output (x, y) is ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16) in
// the flipped image (PIL's affine_fixed, the words from the host), i.e. column S - 1 - sx of the cached one; outside: fill 0.
struct Geom {
    int flip, a0, a1, a2, a3, a4, a5, order;
};
__device__ __forceinline__ Geom load_geom(const int* __restrict__ geom, int b) {
    const int* g = geom + (long)b * 8;
    return {g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7]};
}
// -> offset of the source pixel inside the sample's plane, or -1 (fill)
__device__ __forceinline__ int source_pixel(const Geom& g, int S, int x, int y) {
    const int sx = (g.a2 + y * g.a1 + x * g.a0) >> 16;      // S <= 4096 keeps every term and the sum inside int32
    const int sy = (g.a5 + y * g.a4 + x * g.a3) >> 16;
    if (sx < 0 || sx >= S || sy < 0 || sy >= S) return -1;
    return sy * S + (g.flip ? S - 1 - sx : sx);
}
__device__ __forceinline__ int gray_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
// Image.blend(degenerate d, image a, f): one float32 multiply, one float32 add, truncation; clamped only for f outside [0, 1]
__device__ __forceinline__ int blend8(int d, int a, float f) {
#pragma clang fp contract(off)                              // the product keeps its own rounding.  __fmul_rn / __fadd_rn are plain operators
    const float prod = f * (float)(a - d);                  // inside the HIP headers, outside this pragma's reach: they fused into one FMA
    const float t = (float)d + prod;
    if (f >= 0.f && f <= 1.f) return (int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
__device__ __forceinline__ void jitter_step(int which, const float* f, int cmean, int& r, int& g, int& b) {
    if (which == 0) {                                       // brightness: against black
        r = blend8(0, r, f[0]); g = blend8(0, g, f[0]); b = blend8(0, b, f[0]);
    } else if (which == 1) {                                // contrast: against the image's mean grey
        r = blend8(cmean, r, f[1]); g = blend8(cmean, g, f[1]); b = blend8(cmean, b, f[1]);
    } else {                                                // saturation: against the pixel's own grey
        const int l = gray_of(r, g, b);
        r = blend8(l, r, f[2]); g = blend8(l, g, f[2]); b = blend8(l, b, f[2]);
    }
}

// sums[b] += sum of L over sample b as it stands in front of its contrast step.  Integer adds only: wave sums, a block sum through LDS, then
// one 64-bit atomic per block on the sample's word; the order of integer adds does not change the result.  At most GS_BLOCKS blocks per sample:
// every atomic of a sample hits the same address, and with one per wave of a 256-block grid they took five times as long as the pixels.
__global__ __launch_bounds__(TPB) void gray_sums_kernel(const unsigned char* __restrict__ images, int M, int S, const int* __restrict__ index, const int* __restrict__ geom,
                                                        const float* __restrict__ factors, unsigned long long* __restrict__ sums) {
    const int b = blockIdx.y;
    const Geom g = load_geom(geom, b);
    const float f[3] = {factors[b * 3], factors[b * 3 + 1], factors[b * 3 + 2]};
    const int m = min(max(index[b], 0), M - 1);
    const int npix = S * S;
    const unsigned char* img = images + (long)m * npix * 3;
    unsigned int acc = 0;                                   // <= 255 * 4096^2 / (GS_BLOCKS * TPB) < 2^20 per lane
    for (int p = blockIdx.x * TPB + threadIdx.x; p < npix; p += gridDim.x * TPB) {
        const int y = p / S, x = p - y * S;
        const int sp = source_pixel(g, S, x, y);
        int r = 0, gg = 0, bb = 0;
        if (sp >= 0) { r = img[(long)sp * 3]; gg = img[(long)sp * 3 + 1]; bb = img[(long)sp * 3 + 2]; }
        for (int k = 0; k < 3; ++k) {
            const int which = (g.order >> (2 * k)) & 3;
            if (which == 1) break;
            jitter_step(which, f, 0, r, gg, bb);
        }
        acc += (unsigned int)gray_of(r, gg, bb);
    }
    unsigned long long s = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ unsigned long long wsum[TPB / 64];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + b, wsum[0] + wsum[1] + wsum[2] + wsum[3]);
}

// out_images[b][c][p] = ((byte / 255) - mean[c]) / std[c] of the augmented pixel, out_masks[b][0][p] = (float)mask byte.  The three
// normalisations are functions of a byte, so each block tabulates them once in LDS (three correctly rounded float32 operations each) and
// the pixels look them up.  A lane takes V consecutive pixels of the plane: V = 4 when S * S is a multiple of 4 (16-byte stores, and without
// augmentation 12 + 4 contiguous source bytes as four words), else V = 1.
template <int V, bool AUG>
__global__ __launch_bounds__(TPB) void assemble_kernel(const unsigned char* __restrict__ images, const unsigned char* __restrict__ masks, int M, int S,
                                                       const int* __restrict__ index, float m0, float m1, float m2, float s0, float s1, float s2,
                                                       const int* __restrict__ geom, const float* __restrict__ factors, const long* __restrict__ sums,
                                                       int mask_follow, float* __restrict__ out_i, float* __restrict__ out_m) {
    __shared__ float lut[3][256];
    {
        const float t = __fdiv_rn((float)threadIdx.x, 255.f);
        lut[0][threadIdx.x] = __fdiv_rn(__fsub_rn(t, m0), s0);
        lut[1][threadIdx.x] = __fdiv_rn(__fsub_rn(t, m1), s1);
        lut[2][threadIdx.x] = __fdiv_rn(__fsub_rn(t, m2), s2);
    }
    __syncthreads();
    const int b = blockIdx.y;
    const int npix = S * S;
    const int m = min(max(index[b], 0), M - 1);
    const unsigned char* img = images + (long)m * npix * 3;
    const unsigned char* msk = masks + (long)m * npix;
    float* oi = out_i + (long)b * 3 * npix;
    float* om = out_m + (long)b * npix;
    Geom g = {};
    float f[3] = {1.f, 1.f, 1.f};
    int cmean = 0;
    if constexpr (AUG) {
        g = load_geom(geom, b);
        f[0] = factors[b * 3]; f[1] = factors[b * 3 + 1]; f[2] = factors[b * 3 + 2];
        cmean = (int)((double)sums[b] / (double)npix + 0.5);                // ImageStat's mean in double, PIL's int(mean + 0.5)
    }
    for (int p0 = (blockIdx.x * TPB + threadIdx.x) * V; p0 < npix; p0 += gridDim.x * TPB * V) {
        float o[3][V], om_v[V];
        if constexpr (!AUG && V == 4) {
            const unsigned int* w = reinterpret_cast<const unsigned int*>(img + (long)p0 * 3);       // 12 p0' bytes in, sample base 4-aligned
            const unsigned int w0 = w[0], w1 = w[1], w2 = w[2], mw = *reinterpret_cast<const unsigned int*>(msk + p0);
            const unsigned int by[12] = {w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, w0 >> 24, w1 & 255, (w1 >> 8) & 255,
                                         (w1 >> 16) & 255, w1 >> 24, w2 & 255, (w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c][e] = lut[c][by[e * 3 + c]];
                om_v[e] = (float)((mw >> (8 * e)) & 255);
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int p = p0 + e;
                int sp = p;
                if constexpr (AUG) {
                    const int y = p / S, x = p - y * S;
                    sp = source_pixel(g, S, x, y);
                }
                int r = 0, gg = 0, bb = 0;
                if (sp >= 0) { r = img[(long)sp * 3]; gg = img[(long)sp * 3 + 1]; bb = img[(long)sp * 3 + 2]; }
                if constexpr (AUG) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) jitter_step((g.order >> (2 * k)) & 3, f, cmean, r, gg, bb);
                }
                o[0][e] = lut[0][r]; o[1][e] = lut[1][gg]; o[2][e] = lut[2][bb];
                const int mp = (AUG && mask_follow) ? sp : p;
                om_v[e] = mp >= 0 ? (float)msk[mp] : 0.f;
            }
        }
        if constexpr (V == 4) {
#pragma unroll
            for (int c = 0; c < 3; ++c) st4(oi + (long)c * npix + p0, f32x4{o[c][0], o[c][1], o[c][2], o[c][3]});
            st4(om + p0, f32x4{om_v[0], om_v[1], om_v[2], om_v[3]});
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) oi[(long)c * npix + p0] = o[c][0];
            om[p0] = om_v[0];
        }
    }
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------- entry points
static const char* resample_check(const void* src, const void* bounds, const void* coeffs, const void* dst, int a, int b, int c, int ksize, int out) {
    if (!(src && bounds && coeffs && dst)) return "null pointer";
    if (!(a > 0 && b > 0 && out > 0 && (c == 1 || c == 3))) return "bad shape (positive sizes, 1 or 3 channels)";
    if (!(ksize >= 1 && ksize <= MAX_TAPS)) return "ksize must be in 1..255";
    if (((uintptr_t)bounds % 4) || ((uintptr_t)coeffs % 4)) return "tables must be 4-byte aligned";
    if ((long)a * b * c >= (1L << 31) || (long)out * (a > b ? a : b) * c >= (1L << 31)) return "an image must stay below 2^31 bytes";
    return nullptr;
}

extern "C" int runet_resample8_rows(const unsigned char* src, int h, int w_in, int c, const int* bounds, const int* coeffs, int ksize,
                                    unsigned char* dst, int w_out, void* stream) {
    const char* why = resample_check(src, bounds, coeffs, dst, h, w_in, c, ksize, w_out);
    RUNET_REQUIRE(why == nullptr, why ? why : "");
    hipStream_t st = (hipStream_t)stream;
    const int gx = cdiv(w_out, RW);
    const int want = cdiv(2048, gx);                        // enough blocks to fill the chip, bands long enough to reuse the staged rows
    const int band = max(RROWS, cdiv(h, min(want, 65535)));
    const dim3 grid(gx, cdiv(h, band));
    const size_t lds = (size_t)RW * ksize * sizeof(int);    // <= 64 * 255 * 4 = 65 280 bytes
    if (c == 3) hipLaunchKernelGGL(resample_rows_kernel<3>, grid, dim3(TPB), lds, st, src, h, w_in, bounds, coeffs, ksize, dst, w_out, band);
    else hipLaunchKernelGGL(resample_rows_kernel<1>, grid, dim3(TPB), lds, st, src, h, w_in, bounds, coeffs, ksize, dst, w_out, band);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_resample8_cols(const unsigned char* src, int h_in, int w, int c, const int* bounds, const int* coeffs, int ksize,
                                    unsigned char* dst, int h_out, void* stream) {
    const char* why = resample_check(src, bounds, coeffs, dst, h_in, w, c, ksize, h_out);
    RUNET_REQUIRE(why == nullptr, why ? why : "");
    RUNET_REQUIRE(h_out <= 65535, "at most 65535 output rows");
    hipStream_t st = (hipStream_t)stream;
    const long rowbytes = (long)w * c;
    const dim3 grid((unsigned)min(1024L, (rowbytes / 4 + 1 + TPB) / TPB), h_out);
    hipLaunchKernelGGL(resample_cols_kernel, grid, dim3(TPB), 0, st, src, h_in, rowbytes, bounds, coeffs, ksize, dst);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_gather2d_u8(const unsigned char* src, int sh, int sw, const int* ytab, const int* xtab, unsigned char* dst, int dh, int dw,
                                 void* stream) {
    RUNET_REQUIRE(src && ytab && xtab && dst, "null pointer");
    RUNET_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0, "bad shape");
    RUNET_REQUIRE((long)sh * sw < (1L << 31) && (long)dh * dw < (1L << 31), "a plane must stay below 2^31 bytes");
    RUNET_REQUIRE(((uintptr_t)ytab % 4) == 0 && ((uintptr_t)xtab % 4) == 0 && ((uintptr_t)dst % 4) == 0,
                  "tables and destination must be 4-byte aligned");
    const long total = (long)dh * dw;
    hipLaunchKernelGGL(gather2d_kernel, dim3(ew_grid((total + 3) / 4, 4096)), dim3(TPB), 0, (hipStream_t)stream, src, sh, sw, ytab, xtab, dst,
                       dw, total);
    RUNET_CHECK_LAUNCH();
}

static const char* batch_check(const void* images, int m, int s, const void* index, int b) {
    if (!(images && index)) return "null pointer";
    if (!(m > 0 && b > 0 && b <= 65535 && s > 0)) return "bad shape (m, s > 0, 1 <= b <= 65535)";
    if (s > MAX_SIDE) return "side length above 4096";
    if (((uintptr_t)images % 4) || ((uintptr_t)index % 4)) return "cache and index must be 4-byte aligned";
    return nullptr;
}

extern "C" int runet_batch_gray_sums(const unsigned char* images, int m, int s, const int* index, int b, const int* geom, const float* factors,
                                     long* sums, void* stream) {
    const char* why = batch_check(images, m, s, index, b);
    RUNET_REQUIRE(why == nullptr, why ? why : "");
    RUNET_REQUIRE(geom && factors && sums, "null pointer");
    RUNET_REQUIRE(((uintptr_t)geom % 4) == 0 && ((uintptr_t)factors % 4) == 0 && ((uintptr_t)sums % 8) == 0,
                  "parameters must be 4-byte, sums 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(sums, 0, (size_t)b * sizeof(long), st) != hipSuccess) {
        runet_set_error("runet_batch_gray_sums: clearing the sums failed");
        return RUNET_ELAUNCH;
    }
    const dim3 grid(ew_grid((long)s * s, GS_BLOCKS), b);
    hipLaunchKernelGGL(gray_sums_kernel, grid, dim3(TPB), 0, st, images, m, s, index, geom, factors, (unsigned long long*)sums);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_batch_assemble(const unsigned char* images, const unsigned char* masks, int m, int s, const int* index, int b, float mean0,
                                    float mean1, float mean2, float std0, float std1, float std2, const int* geom, const float* factors,
                                    const long* sums, int mask_mode, float* out_images, float* out_masks, void* stream) {
    const char* why = batch_check(images, m, s, index, b);
    RUNET_REQUIRE(why == nullptr, why ? why : "");
    RUNET_REQUIRE(masks && out_images && out_masks, "null pointer");
    RUNET_REQUIRE((geom != nullptr) == (factors != nullptr) && (geom != nullptr) == (sums != nullptr),
                  "geom, factors and sums come together or not at all");
    RUNET_REQUIRE(mask_mode == 0 || mask_mode == 1, "mask_mode must be 0 (fixed) or 1 (follow)");
    RUNET_REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, "std must not be zero");
    RUNET_REQUIRE(((uintptr_t)masks % 4) == 0 && RUNET_ALIGNED16(out_images) && RUNET_ALIGNED16(out_masks),
                  "masks must be 4-byte, outputs 16-byte aligned");
    RUNET_REQUIRE(!geom || (((uintptr_t)geom % 4) == 0 && ((uintptr_t)factors % 4) == 0 && ((uintptr_t)sums % 8) == 0),
                  "parameters must be 4-byte, sums 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)s * s;
    const bool v4 = npix % 4 == 0;
    const dim3 grid(ew_grid(v4 ? npix / 4 : npix, 1024), b);
#define RUNET_ASM_LAUNCH(V, AUG)                                                                                                        \
    hipLaunchKernelGGL((assemble_kernel<V, AUG>), grid, dim3(TPB), 0, st, images, masks, m, s, index, mean0, mean1, mean2, std0, std1, \
                       std2, geom, factors, sums, mask_mode, out_images, out_masks)
    if (geom) {
        if (v4) RUNET_ASM_LAUNCH(4, true);
        else RUNET_ASM_LAUNCH(1, true);
    } else {
        if (v4) RUNET_ASM_LAUNCH(4, false);
        else RUNET_ASM_LAUNCH(1, false);
    }
#undef RUNET_ASM_LAUNCH
    RUNET_CHECK_LAUNCH();
}
