// The arrays behind the two report figures of the reference: the analysis report of one extraction (predict_coastline.py:708-835: combined
// overlay, NDWI / RGB histograms) and the error maps of the model comparison (Extended_Baseline_Comparison.py:882-959: denormalised image,
// TP / FP / FN / TN overlay, |prob - mask| and its mean).  The reference computes all of them on the host in numpy; here every array is
// produced on the device, bit for bit (include/runet_hip.h states the rules; tests/report_ref.py restates them in numpy).
//
// Every kernel is one streaming pass.  Counts are integers (LDS histograms private to a wave, merged with integer atomics), minima and maxima
// are integer atomics on order-preserving keys, and the one floating-point sum (the error map's) has a fixed order: nothing depends on the
// order in which waves arrive.
#include "runet_common.h"
#include "../../include/runet_hip.h"

// every floating-point expression below restates a numpy / torch expression operation by operation: no FMA may merge two of them
#pragma clang fp contract(off)

namespace {
constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int MAXBINS = 256;
constexpr int GRID_CAP = 2048;                   // grid-stride kernels: enough waves to stream, few enough global merges
constexpr int STATS_GRID_CAP = 1024;             // ndwi_stats_kernel: every block ends in atomics on the same seven words
constexpr int CHUNK = 4 * TPB;                   // error_overlays: pixels per block, the unit of the error sum's order

// ---- combined overlay ----
// A lane owns 4 consecutive pixels of the dense image: 12 image bytes and 4 + 4 mask bytes in, 12 bytes out, as whole dwords; the last
// pixels of the image (fewer than 4) go byte by byte.
__device__ __forceinline__ unsigned char overlay1(unsigned char v, unsigned char water, unsigned char coast, const unsigned char* tab) {
    if (coast == 1) return 255;
    return water == 1 ? tab[v] : v;
}

__global__ __launch_bounds__(TPB) void overlay_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ water,
                                                       const unsigned char* __restrict__ coast, long n, const unsigned char* __restrict__ table,
                                                       unsigned char* __restrict__ out) {
    __shared__ unsigned char tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += TPB) tab[i] = table[i];
    __syncthreads();
    const long groups = (n + 3) / 4;
    for (long g = (long)blockIdx.x * TPB + threadIdx.x; g < groups; g += (long)gridDim.x * TPB) {
        const long p = 4 * g;
        if (p + 4 <= n) {
            const unsigned int* src = reinterpret_cast<const unsigned int*>(image + 3 * p);
            const unsigned int in[3] = {src[0], src[1], src[2]};
            const unsigned int wm = *reinterpret_cast<const unsigned int*>(water + p);
            const unsigned int cm = *reinterpret_cast<const unsigned int*>(coast + p);
            unsigned int wd[3] = {0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                const int j = q / 3, c = q % 3;
                const unsigned char v = (unsigned char)(in[q >> 2] >> (8 * (q & 3)));
                const unsigned char o = overlay1(v, (unsigned char)(wm >> (8 * j)), (unsigned char)(cm >> (8 * j)), tab + 256 * c);
                wd[q >> 2] |= (unsigned int)o << (8 * (q & 3));
            }
            unsigned int* dst = reinterpret_cast<unsigned int*>(out + 3 * p);
            dst[0] = wd[0];
            dst[1] = wd[1];
            dst[2] = wd[2];
        } else {
            for (long x = p; x < n; ++x)
                for (int c = 0; c < 3; ++c) out[3 * x + c] = overlay1(image[3 * x + c], water[x], coast[x], tab + 256 * c);
        }
    }
}

// ---- NDWI ----
template <typename T>
__device__ __forceinline__ double ndwi1(T g, T n) {
    const double gd = (double)g, nd = (double)n;
    return (gd - nd) / ((gd + nd) + 1e-8);
}
__device__ __forceinline__ bool finite_d(double v) { return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
// order-preserving key of a float64; -0.0 and +0.0 are one value
__device__ __forceinline__ unsigned long long key_d(double v) {
    unsigned long long b = (unsigned long long)__double_as_longlong(v);
    if ((b << 1) == 0) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// class slot of a mask byte: 0 = water (mask == 1), 1 = the rest (mask == 0), -1 = neither
__device__ __forceinline__ int class_of(unsigned char m) { return m == 1 ? 0 : m == 0 ? 1 : -1; }

__global__ void ndwi_stats_init_kernel(unsigned long long* stats) {
    if (threadIdx.x < 8) stats[threadIdx.x] = (threadIdx.x == 3 || threadIdx.x == 5) ? ~0ull : 0ull;
}

// stats = {count water, count rest, non-finite, min key water, max key water, min key rest, max key rest, 0}
template <typename T>
__global__ __launch_bounds__(TPB) void ndwi_stats_kernel(const T* __restrict__ green, const T* __restrict__ nir, int w, long n, long rs, long es,
                                                          const unsigned char* __restrict__ mask, unsigned long long* __restrict__ stats) {
    unsigned long long cnt[2] = {0ull, 0ull}, mn[2] = {~0ull, ~0ull}, mx[2] = {0ull, 0ull}, nf = 0ull;
    for (long p = (long)blockIdx.x * TPB + threadIdx.x; p < n; p += (long)gridDim.x * TPB) {
        const int c = class_of(mask[p]);
        if (c < 0) continue;
        const long y = p / w, off = y * rs + (p - y * w) * es;
        const double x = ndwi1<T>(green[off], nir[off]);
        if (!finite_d(x)) {
            ++nf;
            continue;
        }
        const unsigned long long k = key_d(x);
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (c == q) {
                ++cnt[q];
                mn[q] = k < mn[q] ? k : mn[q];
                mx[q] = k > mx[q] ? k : mx[q];
            }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nf += __shfl_xor(nf, o, 64);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            cnt[q] += __shfl_xor(cnt[q], o, 64);
            const unsigned long long a = __shfl_xor(mn[q], o, 64), b = __shfl_xor(mx[q], o, 64);
            mn[q] = a < mn[q] ? a : mn[q];
            mx[q] = b > mx[q] ? b : mx[q];
        }
    }
    // one set of atomics per block, not per wave: they all land on the same seven words, where they serialise.  A minimum or maximum that
    // would not change the word is not sent (the word only ever moves towards the result, so a stale read can only send one too many).
    __shared__ unsigned long long red[WAVES][7];
    if ((threadIdx.x & 63) == 0) {
        unsigned long long* r = red[threadIdx.x >> 6];
        r[0] = cnt[0], r[1] = cnt[1], r[2] = nf, r[3] = mn[0], r[4] = mx[0], r[5] = mn[1], r[6] = mx[1];
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int i = threadIdx.x;
        const bool is_min = i == 3 || i == 5, is_max = i == 4 || i == 6;
        unsigned long long v = red[0][i];
#pragma unroll
        for (int k = 1; k < WAVES; ++k) {
            const unsigned long long o = red[k][i];
            v = is_min ? (o < v ? o : v) : is_max ? (o > v ? o : v) : v + o;
        }
        if (is_min) {
            if (v < __hip_atomic_load(&stats[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&stats[i], v);
        } else if (is_max) {
            if (v > __hip_atomic_load(&stats[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&stats[i], v);
        } else if (v) {
            atomicAdd(&stats[i], v);
        }
    }
}

// np.histogram's bin of x among bins equal bins whose edges are e[0 .. bins] (numpy 2.x, _histograms_impl.py, the equal-bin path): the guess
// ((x - first) / (last - first)) * bins truncated, bins -> bins - 1, then one step down if x < e[i], one step up if x >= e[i + 1] and i is
// not the last bin.  -1: x outside [first, last] or NaN.
__device__ __forceinline__ int numpy_bin(double x, const double* e, int bins) {
    const double first = e[0], last = e[bins];
    if (!(x >= first && x <= last)) return -1;
    const double f = ((x - first) / (last - first)) * (double)bins;
    int i = f < (double)bins ? (int)f : bins - 1;      // the guess, and numpy's `indices == bins` -> bins - 1
    if (!(f >= 0.0)) i = 0;                              // edges that do not rise (the host builds rising ones) must not index outside e
    if (x < e[i]) --i;
    if (x >= e[i + 1] && i != bins - 1) ++i;
    return i;
}

template <typename T>
__global__ __launch_bounds__(TPB) void ndwi_hist_kernel(const T* __restrict__ green, const T* __restrict__ nir, int w, long n, long rs, long es,
                                                         const unsigned char* __restrict__ mask, const double* __restrict__ edges, int bins,
                                                         unsigned long long* __restrict__ counts) {
    __shared__ unsigned lh[WAVES][2 * MAXBINS];
    __shared__ double ed[2][MAXBINS + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < WAVES * 2 * MAXBINS; i += TPB) (&lh[0][0])[i] = 0u;
    for (int i = threadIdx.x; i < 2 * (bins + 1); i += TPB) ed[i / (bins + 1)][i % (bins + 1)] = edges[i];
    __syncthreads();
    // whole blocks of pixels per step, so that every wave stays converged for wave_add
    for (long p0 = (long)blockIdx.x * TPB; p0 < n; p0 += (long)gridDim.x * TPB) {
        const long p = p0 + threadIdx.x;
        int bin = -1;
        if (p < n) {
            const int c = class_of(mask[p]);
            if (c >= 0) {
                const long y = p / w, off = y * rs + (p - y * w) * es;
                const int i = numpy_bin(ndwi1<T>(green[off], nir[off]), ed[c], bins);
                if (i >= 0) bin = c * bins + i;
            }
        }
        wave_add(lh[wave], bin, lane);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * bins; i += TPB) {
        unsigned s = 0u;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) s += lh[k][i];
        if (s) atomicAdd(&counts[i], (unsigned long long)s);
    }
}

// ---- RGB histogram ----
// A lane owns 4 consecutive pixels = three dwords of the dense image; byte q of them belongs to channel q % 3.
__global__ __launch_bounds__(TPB) void rgb_hist_kernel(const unsigned char* __restrict__ image, long n, unsigned long long* __restrict__ hist) {
    __shared__ unsigned lh[WAVES][3 * 256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < WAVES * 3 * 256; i += TPB) (&lh[0][0])[i] = 0u;
    __syncthreads();
    const long groups = (n + 3) / 4;
    for (long g0 = (long)blockIdx.x * TPB; g0 < groups; g0 += (long)gridDim.x * TPB) {
        const long p = 4 * (g0 + threadIdx.x);
        unsigned int in[3] = {0u, 0u, 0u};
        int valid = 0;                                   // bytes of this lane's group that lie inside the image
        if (p + 4 <= n) {
            const unsigned int* src = reinterpret_cast<const unsigned int*>(image + 3 * p);
            in[0] = src[0];
            in[1] = src[1];
            in[2] = src[2];
            valid = 12;
        } else if (p < n) {
            valid = (int)(3 * (n - p));
            for (int q = 0; q < valid; ++q) in[q >> 2] |= (unsigned int)image[3 * p + q] << (8 * (q & 3));
        }
#pragma unroll
        for (int q = 0; q < 12; ++q) wave_add(lh[wave], q < valid ? (q % 3) * 256 + (int)((in[q >> 2] >> (8 * (q & 3))) & 255u) : -1, lane);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * 256; i += TPB) {
        unsigned s = 0u;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) s += lh[k][i];
        if (s) atomicAdd(&hist[i], (unsigned long long)s);
    }
}

// ---- error overlays ----
struct F3 { float v[3]; };

// Block b of sample blockIdx.y owns the pixels [CHUNK b, CHUNK (b + 1)); thread t takes the pixels CHUNK b + t + TPB j, j = 0..3, so that every
// load and store of a wave is contiguous.  The error sum's order is stated in include/runet_hip.h.
__global__ __launch_bounds__(TPB) void error_overlays_kernel(const float* __restrict__ images, const float* __restrict__ prob,
                                                              const float* __restrict__ masks, long hw, float threshold, F3 mean, F3 sd,
                                                              const double* __restrict__ colours, float* __restrict__ vis,
                                                              double* __restrict__ overlay, float* __restrict__ err,
                                                              unsigned long long* __restrict__ counts, double* __restrict__ part) {
    __shared__ double col[5][3];
    __shared__ double wsum[WAVES];
    __shared__ unsigned cls[5];
    if (threadIdx.x < 15) (&col[0][0])[threadIdx.x] = colours[threadIdx.x];
    if (threadIdx.x < 5) cls[threadIdx.x] = 0u;
    __syncthreads();
    const long s = blockIdx.y;
    const float* img = images + s * 3 * hw;
    const float f04 = 0.4f;
    double acc = 0.0;
    unsigned long long packed = 0ull;                    // five 12-bit class counts
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long p = (long)blockIdx.x * CHUNK + threadIdx.x + TPB * j;
        float e = 0.f;
        if (p < hw) {
            const float pr = prob[s * hw + p], g = masks[s * hw + p];
            const bool pos = pr > threshold;
            const int k = g == 1.f ? (pos ? 0 : 2) : g == 0.f ? (pos ? 1 : 3) : 4;      // TP FP FN TN, none
            packed += 1ull << (12 * k);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float t = img[c * hw + p] * sd.v[c];
                float v = t + mean.v[c];
                v = v < 0.f ? 0.f : v;
                v = v > 1.f ? 1.f : v;
                vis[(s * hw + p) * 3 + c] = v;
                const float dim = f04 * v;
                overlay[(s * hw + p) * 3 + c] = (double)dim + col[k][c];
            }
            e = fabsf(pr - g);
            err[s * hw + p] = e;
        }
        acc += (double)e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        packed += __shfl_xor(packed, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = acc;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const unsigned c = (unsigned)((packed >> (12 * k)) & 0xfffull);
            if (c) atomicAdd(&cls[k], c);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) part[s * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    if (threadIdx.x < 5 && cls[threadIdx.x]) atomicAdd(&counts[s * 5 + threadIdx.x], (unsigned long long)cls[threadIdx.x]);
}

// one wave per sample: lane l adds the block sums l, l + 64, ... in that order, then the lanes fold (32, 16, ..., 1)
__global__ __launch_bounds__(64) void error_sum_kernel(const double* __restrict__ part, int nblk, double* __restrict__ sums) {
    const double* p = part + (long)blockIdx.x * nblk;
    double acc = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 64) acc += p[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (threadIdx.x == 0) sums[blockIdx.x] = acc;
}

template <typename T>
void launch_ndwi(int pass, const void* bands, int w, long n, long bs, long rs, long es, const unsigned char* mask, const double* edges, int bins,
                 unsigned long long* out, hipStream_t s) {
    const T* green = (const T*)bands + bs;               // raster index 1
    const T* nir = (const T*)bands + 3 * bs;             // raster index 3
    if (pass == 1) hipLaunchKernelGGL(ndwi_stats_kernel<T>, dim3(ew_grid(n, STATS_GRID_CAP)), dim3(TPB), 0, s, green, nir, w, n, rs, es, mask, out);
    else hipLaunchKernelGGL(ndwi_hist_kernel<T>, dim3(ew_grid(n, GRID_CAP)), dim3(TPB), 0, s, green, nir, w, n, rs, es, mask, edges, bins, out);
}

void launch_ndwi_dtype(int pass, const void* bands, int dtype, int w, long n, long bs, long rs, long es, const unsigned char* mask,
                       const double* edges, int bins, unsigned long long* out, hipStream_t s) {
    switch (dtype) {
        case RUNET_BAND_U8: launch_ndwi<unsigned char>(pass, bands, w, n, bs, rs, es, mask, edges, bins, out, s); break;
        case RUNET_BAND_U16: launch_ndwi<unsigned short>(pass, bands, w, n, bs, rs, es, mask, edges, bins, out, s); break;
        case RUNET_BAND_I16: launch_ndwi<short>(pass, bands, w, n, bs, rs, es, mask, edges, bins, out, s); break;
        default: launch_ndwi<float>(pass, bands, w, n, bs, rs, es, mask, edges, bins, out, s); break;
    }
}
}  // namespace

#define RUNET_REQ_IMAGE()                                                              \
    do {                                                                               \
        RUNET_REQUIRE(h > 0 && w > 0, "bad shape");                                    \
        RUNET_REQUIRE((long)h * w < 2147483648L, "h * w must be below 2^31");          \
    } while (0)

extern "C" int runet_report_overlay_u8(const unsigned char* image, const unsigned char* water, const unsigned char* coast, int h, int w,
                                       const unsigned char* table, unsigned char* out, void* stream) {
    RUNET_REQUIRE(image && water && coast && table && out, "null pointer");
    RUNET_REQ_IMAGE();
    RUNET_REQUIRE((((uintptr_t)image | (uintptr_t)water | (uintptr_t)coast | (uintptr_t)out) & 3) == 0, "misaligned pointer");
    const long n = (long)h * w;
    hipLaunchKernelGGL(overlay_kernel, dim3(ew_grid((n + 3) / 4, GRID_CAP)), dim3(TPB), 0, (hipStream_t)stream, image, water, coast, n, table, out);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_ndwi_stats(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride, long elem_stride,
                                const unsigned char* mask, long* stats, void* stream) {
    RUNET_REQUIRE(bands && mask && stats, "null pointer");
    RUNET_REQ_BANDS();
    RUNET_REQUIRE(n_bands >= 4, "NDWI needs at least four bands (green = band 1, NIR = band 3)");
    RUNET_REQUIRE(((uintptr_t)stats & 7) == 0, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ndwi_stats_init_kernel, dim3(1), dim3(64), 0, s, (unsigned long long*)stats);
    launch_ndwi_dtype(1, bands, dtype, w, (long)h * w, band_stride, row_stride, elem_stride, mask, nullptr, 0, (unsigned long long*)stats, s);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_ndwi_hist(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride, long elem_stride,
                               const unsigned char* mask, const double* edges, int bins, long* counts, void* stream) {
    RUNET_REQUIRE(bands && mask && edges && counts, "null pointer");
    RUNET_REQ_BANDS();
    RUNET_REQUIRE(n_bands >= 4, "NDWI needs at least four bands (green = band 1, NIR = band 3)");
    RUNET_REQUIRE(bins >= 2 && bins <= MAXBINS, "bins must lie in 2..256");
    RUNET_REQUIRE(((uintptr_t)edges & 7) == 0 && ((uintptr_t)counts & 7) == 0, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)2 * bins * sizeof(long), s) != hipSuccess) {
        (void)hipGetLastError();
        runet_set_error("runet_ndwi_hist: clearing the counts failed");
        return RUNET_ELAUNCH;
    }
    launch_ndwi_dtype(2, bands, dtype, w, (long)h * w, band_stride, row_stride, elem_stride, mask, edges, bins, (unsigned long long*)counts, s);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_rgb_hist_u8(const unsigned char* image, int h, int w, long* hist, void* stream) {
    RUNET_REQUIRE(image && hist, "null pointer");
    RUNET_REQ_IMAGE();
    RUNET_REQUIRE(((uintptr_t)image & 3) == 0 && ((uintptr_t)hist & 7) == 0, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)3 * 256 * sizeof(long), s) != hipSuccess) {
        (void)hipGetLastError();
        runet_set_error("runet_rgb_hist_u8: clearing the histogram failed");
        return RUNET_ELAUNCH;
    }
    const long n = (long)h * w;
    hipLaunchKernelGGL(rgb_hist_kernel, dim3(ew_grid((n + 3) / 4, GRID_CAP)), dim3(TPB), 0, s, image, n, (unsigned long long*)hist);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_error_overlays_workspace_bytes(int n, int h, int w) {
    if (n < 1 || n > 65535 || h <= 0 || w <= 0 || (long)h * w >= 2147483648L) return -1;
    return (long)n * cdiv((long)h * w, CHUNK) * (long)sizeof(double);
}

extern "C" int runet_error_overlays(const float* images, const float* prob, const float* masks, int n, int h, int w, float threshold, float mean0,
                                    float mean1, float mean2, float std0, float std1, float std2, const double* colours, float* vis,
                                    double* overlay, float* err, long* counts, double* sums, void* workspace, long workspace_bytes,
                                    void* stream) {
    RUNET_REQUIRE(images && prob && masks && colours && vis && overlay && err && counts && sums && workspace, "null pointer");
    RUNET_REQUIRE(n >= 1 && n <= 65535, "1..65535 samples");
    RUNET_REQ_IMAGE();
    RUNET_REQUIRE(workspace_bytes >= runet_error_overlays_workspace_bytes(n, h, w), "workspace too small");
    RUNET_REQUIRE((((uintptr_t)images | (uintptr_t)prob | (uintptr_t)masks | (uintptr_t)vis | (uintptr_t)err) & 3) == 0 &&
                      (((uintptr_t)colours | (uintptr_t)overlay | (uintptr_t)counts | (uintptr_t)sums | (uintptr_t)workspace) & 7) == 0,
                  "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)n * 5 * sizeof(long), s) != hipSuccess) {
        (void)hipGetLastError();
        runet_set_error("runet_error_overlays: clearing the counts failed");
        return RUNET_ELAUNCH;
    }
    const long hw = (long)h * w;
    const int nblk = cdiv(hw, CHUNK);
    const F3 mean = {{mean0, mean1, mean2}}, sd = {{std0, std1, std2}};
    hipLaunchKernelGGL(error_overlays_kernel, dim3(nblk, n), dim3(TPB), 0, s, images, prob, masks, hw, threshold, mean, sd, colours, vis, overlay,
                       err, (unsigned long long*)counts, (double*)workspace);
    hipLaunchKernelGGL(error_sum_kernel, dim3(n), dim3(64), 0, s, (const double*)workspace, nblk, sums);
    RUNET_CHECK_LAUNCH();
}
