// Prediction-side byte kernels (predict_coastline.py:358-363, 387-396, 595-602; Main_Final.py:521 for the probability models): u8 scene ->
// normalised tiles (NHWC-4 for the plain U-Net's stem, planar NCHW for every other model), arg-max of the head's NHWC output or `prob > threshold`
// of a 1-channel probability map stitched into a u8 scene mask, OpenCV's INTER_NEAREST index rule on u8 masks, and the elliptical dilation minus
// the mask with its two pixel counts.  All of them stream bytes: masks are dense [h][w] u8, every lane owns 16 consecutive mask bytes that are
// 16-byte aligned IN MEMORY (a row of a 1531-wide mask starts at any alignment, so groups are cut on addresses, not on columns) and writes them
// with one 16-byte store; only the groups cut by a row end, a tile edge or a core edge fall back to byte stores.
#include "runet_common.h"
#include "../../include/runet_hip.h"
#include <math.h>

namespace {
constexpr int TPB = 256;
constexpr int MAXK = 31;

// 16 mask bytes b[0..16) for the pixels x0 .. x0+15 of a row (row + x0 is 16-byte aligned); only pixels in [lo, hi) belong to the caller
__device__ __forceinline__ void store_group(unsigned char* row, int x0, int lo, int hi, const uint4 v) {
    if (x0 >= lo && x0 + 16 <= hi) {
        *reinterpret_cast<uint4*>(row + x0) = v;
        return;
    }
    const unsigned int wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int x = x0 + j;
        if (x >= lo && x < hi) row[x] = (unsigned char)(wds[j >> 2] >> (8 * (j & 3)));
    }
}

// ---- u8 HWC scene -> [n_tiles][T][T][4] fp32 (PLANAR: [n_tiles][3][T][T]), ToTensor + Normalize in their own order of roundings ----
struct NormCoef { float mean[3], std[3]; };

template <bool PLANAR>
__global__ void scene_to_tiles_kernel(const unsigned char* __restrict__ scene, int h, int w, long row_stride, const int* __restrict__ origins,
                                      int tile, float* __restrict__ out, NormCoef nc) {
#pragma clang fp contract(off)
    const int t = blockIdx.y;
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= tile * tile) return;
    const int ly = p / tile, lx = p - ly * tile;
    const long y = (long)origins[2 * t] + ly, x = (long)origins[2 * t + 1] + lx;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (y >= 0 && y < h && x >= 0 && x < w) {
        const unsigned char* s = scene + y * row_stride + x * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = ((float)s[c] / 255.0f - nc.mean[c]) / nc.std[c];
    }
    if constexpr (PLANAR) {                                      // a wave writes 256 consecutive bytes of each of the three planes
        const long plane = (long)tile * tile;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[((long)t * 3 + c) * plane + p] = v[c];
    } else {
        *reinterpret_cast<f32x4*>(out + ((long)t * tile * tile + p) * 4) = v;
    }
}

// ---- arg-max over the head's 4-float pixels, core of each tile -> scene mask ----
// torch.argmax's order on the CPU: the first maximal index; NaN is greater than everything and the first NaN wins
__device__ __forceinline__ int argmax4(const f32x4 v, int classes) {
    int best = 0;
    float bv = v[0];
#pragma unroll
    for (int c = 1; c < 4; ++c)
        if (c < classes && !(bv != bv) && (v[c] > bv || v[c] != v[c])) { best = c; bv = v[c]; }
    return best;
}

// The two per-pixel rules of the stitch.  `at` = index of the pixel in the network's output counted in pixels (tile, row and column), `to` =
// index of the same pixel in the scene.
struct ArgmaxPx {                                                // four coalesced 16-byte logit reads per lane
    const float* z4;
    int classes;
    __device__ __forceinline__ unsigned char operator()(long at, long to) const {
        return (unsigned char)argmax4(*reinterpret_cast<const f32x4*>(z4 + at * 4), classes);
    }
};
// torch's `prob > threshold` on an fp32 tensor: an ordered compare, so NaN is 0 (land) where arg-max lets NaN win; +Inf is 1, the threshold
// itself 0.  The soft map takes the probability's bits as they are, NaN included.
struct ThresholdPx {                                             // four coalesced dword reads (and soft-map writes) per lane
    const float* prob;
    float* soft;
    float threshold;
    __device__ __forceinline__ unsigned char operator()(long at, long to) const {
        const float p = prob[at];
        if (soft) soft[to] = p;
        return p > threshold ? 1 : 0;
    }
};

// one wave per core row, 256 address-aligned mask bytes per wave: the lanes read their pixels coalesced (px), the mask bytes meet in LDS and
// lanes 0..15 store 16 of them each
template <class Px>
__global__ void stitch_kernel(const Px px, int tile, const int* __restrict__ origins, int halo, unsigned char* __restrict__ mask, int h, int w) {
    __shared__ __attribute__((aligned(16))) unsigned char cls[4][256];
    const int t = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long oy = origins[2 * t], ox = origins[2 * t + 1];
    const int core = tile - 2 * halo;
    const int ly = halo + blockIdx.y * 4 + wave;               // row inside the tile
    const long y = oy + ly;
    const long xlo_l = ox + halo < 0 ? 0 : ox + halo, xhi_l = ox + halo + core > w ? w : ox + halo + core;
    const bool row_ok = ly < halo + core && y >= 0 && y < h && xlo_l < xhi_l;
    int lo = 0, hi = 0, x0 = 0;
    unsigned char* row = nullptr;
    if (row_ok) {
        lo = (int)xlo_l, hi = (int)xhi_l;
        row = mask + y * w;
        const int shift = (int)((uintptr_t)(row + lo) & 15);
        x0 = lo - shift + blockIdx.x * 256;                  // row + x0 is 16-byte aligned
        const long at0 = ((long)t * tile + ly) * tile - ox;  // + x: lo <= x < hi keeps x - ox inside [halo, tile - halo)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = j * 64 + lane, x = x0 + q;
            unsigned char c = 0;
            if (x >= lo && x < hi) c = px(at0 + x, y * w + x);
            cls[wave][q] = c;
        }
    }
    __syncthreads();
    if (row_ok && lane < 16 && x0 + lane * 16 < hi)
        store_group(row, x0 + lane * 16, lo, hi, *reinterpret_cast<const uint4*>(&cls[wave][lane * 16]));
}

// ---- cv2.resize(INTER_NEAREST) of a u8 mask: source index = min((int)floor(x * (1.0 / ((double)dw / sw))), sw - 1), IEEE double ----
__device__ __forceinline__ int nearest_src(int d, double inv_scale, int n_src) {
    const int s = (int)floor((double)d * inv_scale);
    return s < n_src - 1 ? s : n_src - 1;
}

__global__ void resize_nearest_u8_kernel(const unsigned char* __restrict__ src, int sh, int sw, unsigned char* __restrict__ dst, int dh, int dw,
                                         double ifx, double ify) {
    const long total = (long)dh * dw;
    const long i0 = ((long)blockIdx.x * TPB + threadIdx.x) * 16;
    if (i0 >= total) return;
    int y = (int)(i0 / dw), x = (int)(i0 - (long)y * dw);
    const unsigned char* srow = src + (long)nearest_src(y, ify, sh) * sw;
    unsigned int wds[4] = {0u, 0u, 0u, 0u};
    const int n = total - i0 < 16 ? (int)(total - i0) : 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j < n) {
            wds[j >> 2] |= (unsigned int)srow[nearest_src(x, ifx, sw)] << (8 * (j & 3));
            if (++x == dw) {
                x = 0;
                ++y;
                if (y < dh) srow = src + (long)nearest_src(y, ify, sh) * sw;
            }
        }
    }
    if (n == 16) {
        *reinterpret_cast<uint4*>(dst + i0) = make_uint4(wds[0], wds[1], wds[2], wds[3]);
    } else {
        for (int j = 0; j < n; ++j) dst[i0 + j] = (unsigned char)(wds[j >> 2] >> (8 * (j & 3)));
    }
}

// ---- dilate(mask, MORPH_ELLIPSE k x k) - mask, with the water / coastline pixel counts ----
// A block owns DT_H x DT_W output pixels.  Its input (tile + k - 1 halo rows, one 64-column word of halo on each side) is read once, one
// byte per lane, and bit-packed by a wave ballot: 64 pixels = one 64-bit LDS word.  A lane then builds the 16 output pixels of one group from
// 64-bit windows: for structuring-element row i the OR over the span [x - dx_i, x + dx_i] is a few shift-ORs on the whole window.
constexpr int DT_H = 32, DT_W = 256, DT_WORDS = DT_W / 64 + 2, DT_GROUPS = DT_W / 16 + 1;
struct SpanDx { unsigned char dx[MAXK + 1]; };

__global__ void __launch_bounds__(TPB) dilate_diff_kernel(const unsigned char* __restrict__ mask, int h, int w, int k, SpanDx sp,
                                                          unsigned char* __restrict__ coast, unsigned char* __restrict__ dilated,
                                                          int* __restrict__ counts) {
    __shared__ unsigned long long bits[DT_H + MAXK - 1][DT_WORDS];
    __shared__ int red[2][TPB / 64];
    const int r = k >> 1;
    const int tx0 = blockIdx.x * DT_W, ty0 = blockIdx.y * DT_H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rows_ld = DT_H + k - 1;
    for (int item = wave; item < rows_ld * DT_WORDS; item += TPB / 64) {
        const int ry = item / DT_WORDS, wi = item - ry * DT_WORDS;
        const int y = ty0 - r + ry, x = tx0 - 64 + 64 * wi + lane;
        const bool on = y >= 0 && y < h && x >= 0 && x < w && mask[(long)y * w + x] != 0;
        const unsigned long long b = __ballot(on);
        if (lane == 0) bits[ry][wi] = b;
    }
    __syncthreads();
    const int xe = tx0 + DT_W < w ? tx0 + DT_W : w;           // this block's columns are [tx0, xe)
    int n_water = 0, n_coast = 0;
    for (int item = threadIdx.x; item < DT_H * DT_GROUPS; item += TPB) {
        const int ry = item / DT_GROUPS, gi = item - ry * DT_GROUPS;
        const int y = ty0 + ry;
        if (y >= h) break;
        const long roff = (long)y * w;
        const int shift = (int)((uintptr_t)(coast + roff + tx0) & 15);
        const int x0 = tx0 - shift + gi * 16;                 // coast + roff + x0 is 16-byte aligned; x0 > tx0 - 16
        if (x0 >= xe) continue;
        const int rel = x0 - 16 - (tx0 - 64);                 // window = columns [x0 - 16, x0 + 48), 17 <= rel <= 303
        const int wi = rel >> 6, sh = rel & 63;
        unsigned long long acc = 0, centre = 0;
        for (int i = 0; i < k; ++i) {
            const unsigned long long* brow = bits[ry + i];
            unsigned long long a = brow[wi] >> sh;
            if (sh) a |= brow[wi + 1] << (64 - sh);
            if (i == r) centre = a >> 16;
            const int dx = sp.dx[i], n = 2 * dx + 1;
            int cover = 1;                                    // a's bit b = OR of the window's bits [b, b + cover)
            while (cover * 2 <= n) { a |= a >> cover; cover *= 2; }
            a |= a >> (n - cover);
            acc |= a >> (16 - dx);
        }
        unsigned int valid = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) valid |= (unsigned int)(x0 + j >= tx0 && x0 + j < xe) << j;
        const unsigned int m = (unsigned int)centre & valid, d = (unsigned int)acc & valid, c = d & ~m;
        n_water += __popc(m);
        n_coast += __popc(c);
        unsigned int cw[4], dw[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cw[q] = dw[q] = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cw[q] |= ((c >> (4 * q + j)) & 1u) << (8 * j);
                dw[q] |= ((d >> (4 * q + j)) & 1u) << (8 * j);
            }
        }
        store_group(coast + roff, x0, tx0, xe, make_uint4(cw[0], cw[1], cw[2], cw[3]));
        if (dilated) store_group(dilated + roff, x0, tx0, xe, make_uint4(dw[0], dw[1], dw[2], dw[3]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_water += __shfl_xor(n_water, o, 64);
        n_coast += __shfl_xor(n_coast, o, 64);
    }
    if (lane == 0) { red[0][wave] = n_water; red[1][wave] = n_coast; }
    __syncthreads();
    if (threadIdx.x < 2) {
        int s = 0;
        for (int i = 0; i < TPB / 64; ++i) s += red[threadIdx.x][i];
        if (s) atomicAdd(counts + threadIdx.x, s);
    }
}
}  // namespace

// cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)) as column spans: row i holds columns [j1[i], j2[i]).  Host only.
extern "C" int runet_ellipse_spans(int k, int* j1, int* j2) {
    RUNET_REQUIRE(j1 && j2, "null pointer");
    RUNET_REQUIRE(k >= 1 && k <= MAXK && (k & 1), "k must be odd, 1..31");
    const int r = k / 2, c = k / 2;
    for (int i = 0; i < k; ++i) {
        const int dy = i - r;
        const int dx = r ? (int)nearbyint(c * sqrt((r * r - dy * dy) / (double)(r * r))) : 0;      // round half to even
        j1[i] = c - dx > 0 ? c - dx : 0;
        j2[i] = c + dx + 1 < k ? c + dx + 1 : k;
    }
    return RUNET_OK;
}

template <bool PLANAR>
static int scene_to_tiles_launch(const unsigned char* scene, int h, int w, long row_stride, const int* origins, int n_tiles, int tile,
                                 const NormCoef& nc, float* tiles, void* stream) {
    RUNET_REQUIRE(scene && origins && tiles, "null pointer");
    RUNET_REQUIRE(h > 0 && w > 0 && row_stride >= 3L * w, "bad scene shape");
    RUNET_REQUIRE(n_tiles > 0 && n_tiles <= 65535 && tile > 0 && tile <= 8192, "bad tile count / size");
    RUNET_REQUIRE(((uintptr_t)tiles & (PLANAR ? 3 : 15)) == 0, "tiles must be 16-byte aligned (planar: 4-byte)");
    RUNET_REQUIRE(nc.std[0] != 0.f && nc.std[1] != 0.f && nc.std[2] != 0.f, "zero std");
    hipLaunchKernelGGL(scene_to_tiles_kernel<PLANAR>, dim3(cdiv((long)tile * tile, TPB), n_tiles), dim3(TPB), 0, (hipStream_t)stream, scene, h,
                       w, row_stride, origins, tile, tiles, nc);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_scene_to_tiles(const unsigned char* scene, int h, int w, long row_stride, const int* origins, int n_tiles, int tile,
                                    float mean0, float mean1, float mean2, float std0, float std1, float std2, float* tiles, void* stream) {
    return scene_to_tiles_launch<false>(scene, h, w, row_stride, origins, n_tiles, tile, {{mean0, mean1, mean2}, {std0, std1, std2}}, tiles,
                                        stream);
}

extern "C" int runet_scene_to_tiles_nchw(const unsigned char* scene, int h, int w, long row_stride, const int* origins, int n_tiles, int tile,
                                         float mean0, float mean1, float mean2, float std0, float std1, float std2, float* tiles,
                                         void* stream) {
    return scene_to_tiles_launch<true>(scene, h, w, row_stride, origins, n_tiles, tile, {{mean0, mean1, mean2}, {std0, std1, std2}}, tiles,
                                       stream);
}

extern "C" int runet_argmax_stitch(const float* z4, int n_tiles, int tile, int n_classes, const int* origins, int halo, unsigned char* mask,
                                   int h, int w, void* stream) {
    RUNET_REQUIRE(z4 && origins && mask, "null pointer");
    RUNET_REQUIRE(h > 0 && w > 0 && n_tiles > 0 && n_tiles <= 65535 && tile > 0 && tile <= 8192, "bad shape");
    RUNET_REQUIRE(n_classes >= 1 && n_classes <= 4, "1..4 classes");
    RUNET_REQUIRE(halo >= 0 && 2 * halo < tile, "2 * halo must be smaller than the tile");
    RUNET_REQUIRE(((uintptr_t)z4 & 15) == 0, "z4 must be 16-byte aligned");
    const int core = tile - 2 * halo;
    RUNET_REQUIRE(cdiv(core, 4) <= 65535, "core too tall");
    hipLaunchKernelGGL(stitch_kernel<ArgmaxPx>, dim3(cdiv(core + 15, 256), cdiv(core, 4), n_tiles), dim3(TPB), 0, (hipStream_t)stream,
                       ArgmaxPx{z4, n_classes}, tile, origins, halo, mask, h, w);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_threshold_stitch(const float* prob, int n_tiles, int tile, const int* origins, int halo, float threshold,
                                      unsigned char* mask, float* soft, int h, int w, void* stream) {
    RUNET_REQUIRE(prob && origins && mask, "null pointer");
    RUNET_REQUIRE(tile > 0 && tile <= 8192, "tile must be positive (at most 8192)");
    RUNET_REQUIRE(halo >= 0 && halo < tile - halo, "2 * halo must be smaller than the tile");
    RUNET_REQUIRE(h > 0 && w > 0 && (long)h * w <= 2147483647L, "bad scene shape: h * w must fit int32");
    RUNET_REQUIRE(n_tiles > 0 && n_tiles <= 65535, "bad tile count");
    RUNET_REQUIRE(((uintptr_t)prob & 3) == 0 && ((uintptr_t)soft & 3) == 0, "prob and soft must be 4-byte aligned");
    const int core = tile - 2 * halo;
    hipLaunchKernelGGL(stitch_kernel<ThresholdPx>, dim3(cdiv(core + 15, 256), cdiv(core, 4), n_tiles), dim3(TPB), 0, (hipStream_t)stream,
                       ThresholdPx{prob, soft, threshold}, tile, origins, halo, mask, h, w);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_resize_nearest_u8(const unsigned char* src, int sh, int sw, unsigned char* dst, int dh, int dw, void* stream) {
    RUNET_REQUIRE(src && dst, "null pointer");
    RUNET_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0, "bad shape");
    RUNET_REQUIRE(((uintptr_t)dst & 15) == 0, "dst must be 16-byte aligned");
    RUNET_REQUIRE(src != dst, "in-place resize");
    const double ifx = 1.0 / ((double)dw / sw), ify = 1.0 / ((double)dh / sh);
    const long groups = ((long)dh * dw + 15) / 16;
    hipLaunchKernelGGL(resize_nearest_u8_kernel, dim3(cdiv(groups, TPB)), dim3(TPB), 0, (hipStream_t)stream, src, sh, sw, dst, dh, dw, ifx, ify);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_dilate_diff_u8(const unsigned char* mask, int h, int w, int k, unsigned char* coast, unsigned char* dilated, int* counts2,
                                    void* stream) {
    RUNET_REQUIRE(mask && coast && counts2, "null pointer");
    RUNET_REQUIRE(k >= 1 && k <= MAXK && (k & 1), "k must be odd, 1..31");
    RUNET_REQUIRE(h > 0 && w > 0 && cdiv(h, DT_H) <= 65535, "bad shape");
    RUNET_REQUIRE(mask != coast && mask != dilated, "in-place dilation");
    RUNET_REQUIRE(!dilated || (((uintptr_t)dilated ^ (uintptr_t)coast) & 15) == 0, "coast and dilated must share their 16-byte phase");
    int j1[MAXK], j2[MAXK];
    if (runet_ellipse_spans(k, j1, j2)) return RUNET_EINVAL;
    SpanDx sp = {};
    for (int i = 0; i < k; ++i) sp.dx[i] = (unsigned char)(k / 2 - j1[i]);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts2, 0, 2 * sizeof(int), st) != hipSuccess) {
        (void)hipGetLastError();
        runet_set_error("runet_dilate_diff_u8: clearing the counts failed");
        return RUNET_ELAUNCH;
    }
    hipLaunchKernelGGL(dilate_diff_kernel, dim3(cdiv(w, DT_W), cdiv(h, DT_H)), dim3(TPB), 0, st, mask, h, w, k, sp, coast, dilated, counts2);
    RUNET_CHECK_LAUNCH();
}
