// Scene ingestion (tif_to_image.py:139-171, predict_coastline.py:514-581): the exact 2nd / 98th percentile of up to three planes of a planar
// multi-band raster, and the float64 stretch to interleaved uint8 RGB, in front of runet_scene_to_tiles.
//
// Percentiles: numpy's "linear" method needs the order statistics of ranks k, k + 1 for each of the two quantiles: four ranks per band.  They
// are found by a most-significant-digit radix select on an order-preserving 32-bit key, 8 bits per pass (1 pass for uint8, 2 for the 16-bit
// types, 4 for float32).  A pass is two launches: band_hist_kernel counts, for every band and every DISTINCT prefix found so far, the next
// digit of the elements that carry the prefix (wave-private LDS histograms, merged with integer atomics: the counts do not depend on arrival
// order); band_scan_kernel (one block) walks each rank's 256 counts, appends the digit of the bucket the rank falls in and keeps the rank
// inside that bucket.  Prefixes of different ranks are distinct or equal, so an element matches at most one of them: one LDS atomic per
// element at the most.  Equal neighbouring keys (nodata runs) are added once per wave, not once per lane.  After the last pass the prefix IS
// the key of the order statistic; the scan decodes it and interpolates by numpy's _lerp in float64.
#include "runet_common.h"
#include "../../include/runet_hip.h"

// every float64 expression below restates a numpy expression operation by operation: no FMA may merge two of them
#pragma clang fp contract(off)

namespace {
constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int SLOTS = 4, BINS = 256, MAXSEL = 3, MAXPASS = 4;
constexpr int HIST_BLOCKS = 512;                 // row-strided blocks per band: enough waves to stream, few enough global merges

struct Sel3 { int i[MAXSEL]; };
struct SelState {
    unsigned prefix[MAXSEL][SLOTS];              // key bits fixed so far (the digits of the passes done)
    unsigned rank[MAXSEL][SLOTS];                // rank inside the set of elements that carry the prefix
    int alias[MAXSEL][SLOTS];                    // the first slot of the band with the same prefix: the histogram this slot reads
};

// ---- order-preserving keys ----
template <typename T> struct KeyOf;
template <> struct KeyOf<unsigned char> {
    static constexpr int PASSES = 1;
    static __device__ __forceinline__ unsigned key(unsigned char v) { return v; }
};
template <> struct KeyOf<unsigned short> {
    static constexpr int PASSES = 2;
    static __device__ __forceinline__ unsigned key(unsigned short v) { return v; }
};
template <> struct KeyOf<short> {
    static constexpr int PASSES = 2;
    static __device__ __forceinline__ unsigned key(short v) { return (unsigned)((int)v + 32768); }
};
template <> struct KeyOf<float> {
    static constexpr int PASSES = 4;
    static __device__ __forceinline__ unsigned key(float v) {
        unsigned b = __float_as_uint(v);
        if ((b << 1) == 0) b = 0;                // -0.0 and +0.0 compare equal: one key
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
};
__device__ __forceinline__ float key_to_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// A block walks the rows blockIdx.x, blockIdx.x + gridDim.x, ...; a lane owns one 16-byte group of a row, cut on addresses when the elements
// are contiguous (one 16-byte load), element by element at a row's ends and for strided elements.
template <typename T>
__global__ __launch_bounds__(TPB) void band_hist_kernel(const T* __restrict__ bands, int h, int w, long bs, long rs, long es, Sel3 sel, int pass,
                                                         int shift, unsigned* __restrict__ hist, const SelState* __restrict__ st,
                                                         int* __restrict__ nonfinite) {
    constexpr int VEC = 16 / (int)sizeof(T);
    __shared__ unsigned lh[WAVES][SLOTS * BINS];
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int used = pass == 0 ? BINS : SLOTS * BINS;
    for (int i = threadIdx.x; i < WAVES * SLOTS * BINS; i += TPB) (&lh[0][0])[i] = 0u;
    unsigned pre[SLOTS] = {0u, 0u, 0u, 0u};
    bool own[SLOTS] = {true, false, false, false};
    unsigned mask = 0u;
    if (pass > 0) {
        mask = ~0u << (shift + 8);
#pragma unroll
        for (int r = 0; r < SLOTS; ++r) {
            pre[r] = st->prefix[b][r];
            own[r] = st->alias[b][r] == r;
        }
    }
    __syncthreads();
    const T* plane = bands + (long)sel.i[b] * bs;
    int nf = 0;
    for (int y = blockIdx.x; y < h; y += gridDim.x) {
        const T* row = plane + (long)y * rs;
        const int mis = es == 1 ? (int)(((uintptr_t)row & 15) / sizeof(T)) : 0;
        const int ngroups = (w + mis + VEC - 1) / VEC;
        for (int g0 = 0; g0 < ngroups; g0 += TPB) {
            const int g = g0 + threadIdx.x;
            const int x0 = g * VEC - mis;
            T v[VEC];
            unsigned valid = 0u;
            if (g < ngroups) {
                if (es == 1 && x0 >= 0 && x0 + VEC <= w) {
                    const uint4 q = *reinterpret_cast<const uint4*>(row + x0);
                    __builtin_memcpy(v, &q, 16);
                    valid = (1u << VEC) - 1u;
                } else {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const int x = x0 + j;
                        v[j] = T(0);
                        if (x >= 0 && x < w) {
                            v[j] = row[(long)x * es];
                            valid |= 1u << j;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                int bin = -1;
                if ((valid >> j) & 1u) {
                    const unsigned key = KeyOf<T>::key(v[j]);
                    const int digit = (int)((key >> shift) & 255u);
                    if (pass == 0) {
                        bin = digit;
                        if constexpr (sizeof(T) == 4) nf += (__float_as_uint((float)v[j]) & 0x7f800000u) == 0x7f800000u;
                    } else {
#pragma unroll
                        for (int r = 0; r < SLOTS; ++r)
                            if (own[r] && (key & mask) == pre[r]) bin = r * BINS + digit;
                    }
                }
                wave_add(lh[wave], bin, lane);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < used; i += TPB) {
        unsigned s = 0u;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) s += lh[k][i];
        if (s) atomicAdd(&hist[(long)b * SLOTS * BINS + i], s);
    }
    if constexpr (sizeof(T) == 4) {
        if (pass == 0) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nf += __shfl_xor(nf, o, 64);
            if (lane == 0 && nf) atomicAdd(nonfinite, nf);
        }
    }
}

// numpy's _lerp(a, b, t) on the two order statistics, decoded from their keys.  diff = subtract(b, a) is taken in the ARRAY's dtype there: int16
// wraps, float32 rounds; a float64 copy of the band (wide) subtracts in float64.
__device__ double lerp_keys(unsigned ka, unsigned kb, double g, int dtype, int wide) {
    double a, b, diff;
    if (dtype == RUNET_BAND_F32) {
        const float fa = key_to_float(ka), fb = key_to_float(kb);
        a = (double)fa;
        b = (double)fb;
        diff = wide ? b - a : (double)(fb - fa);
    } else if (dtype == RUNET_BAND_I16) {
        const int ia = (int)ka - 32768, ib = (int)kb - 32768;
        a = (double)ia;
        b = (double)ib;
        diff = wide ? b - a : (double)(short)(ib - ia);
    } else {
        a = (double)ka;
        b = (double)kb;
        diff = b - a;
    }
    double r = a + diff * g;
    if (g >= 0.5) r = b - diff * (1.0 - g);
    return r;
}

// one block: thread 4 b + r owns rank r of band b
__global__ void band_scan_kernel(const unsigned* __restrict__ hist, SelState* __restrict__ st, int n_sel, int pass, int shift, int last, unsigned n,
                                 unsigned k_lo, unsigned k_hi, double g_lo, double g_hi, int dtype, int wide, double* __restrict__ out) {
    __shared__ unsigned sp[MAXSEL][SLOTS];
    const int b = threadIdx.x / SLOTS, r = threadIdx.x % SLOTS;
    const bool active = b < n_sel;
    unsigned prefix = 0u, rank = 0u;
    if (active) {
        int src = 0;
        if (pass == 0) {
            const unsigned k = (r < 2 ? k_lo : k_hi) + (unsigned)(r & 1);
            rank = k < n - 1u ? k : n - 1u;
        } else {
            prefix = st->prefix[b][r];
            rank = st->rank[b][r];
            src = st->alias[b][r];
        }
        const unsigned* hh = hist + ((long)b * SLOTS + src) * BINS;
        unsigned cum = 0u;
        int d = 0;
        for (; d < BINS - 1; ++d) {
            const unsigned c = hh[d];
            if (rank < cum + c) break;
            cum += c;
        }
        prefix |= (unsigned)d << shift;
        rank -= cum;
        sp[b][r] = prefix;
    }
    __syncthreads();
    if (!active) return;
    int a = r;
    for (int q = r - 1; q >= 0; --q)
        if (sp[b][q] == prefix) a = q;
    st->prefix[b][r] = prefix;
    st->rank[b][r] = rank;
    st->alias[b][r] = a;
    if (last && r == 0) {
        out[2 * b] = lerp_keys(sp[b][0], sp[b][1], g_lo, dtype, wide);
        out[2 * b + 1] = lerp_keys(sp[b][2], sp[b][3], g_hi, dtype, wide);
    }
}

// ---- stretch ----
// min(max((double(v) - p_lo) / (p_hi - p_lo) * 255, 0), 255), the darkening of channel 0 and the cast through the input dtype.  Comparisons
// keep a NaN (np.clip does); a NaN writes 0.
template <bool ISF>
__device__ __forceinline__ unsigned char stretch1(double x, double lo, double den, bool plain, bool dark) {
    double s = plain ? x : (x - lo) / den * 255.0;
    s = s < 0.0 ? 0.0 : s;
    s = s > 255.0 ? 255.0 : s;
    if (dark && s < 100.0) s = s * 0.7;
    if (s != s) return 0;
    return ISF ? (unsigned char)(int)(float)s : (unsigned char)(int)s;
}

// A lane owns 4 consecutive pixels = 12 output bytes, cut so that they start on a 4-byte address: pixel x of a row sits at row + 3 x, and
// x = 3 (4 - row % 4) % 4 is the first aligned one.  Whole groups go out as three dwords, the ends of a row byte by byte.
template <typename T, bool ISF>
__global__ __launch_bounds__(TPB) void band_stretch_kernel(const T* __restrict__ bands, int h, int w, long bs, long rs, long es, Sel3 sel,
                                                            const double* __restrict__ pct, int mode, unsigned char* __restrict__ out, long ors) {
    double lo[3], den[3];
    bool plain[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = pct[2 * c];
        den[c] = pct[2 * c + 1] - lo[c];
        plain[c] = mode == 2 && !(den[c] > 0.0);
    }
    const T* p0 = bands + (long)sel.i[0] * bs;
    const T* p1 = bands + (long)sel.i[1] * bs;
    const T* p2 = bands + (long)sel.i[2] * bs;
    const int g = blockIdx.x * TPB + threadIdx.x;
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        unsigned char* orow = out + (long)y * ors;
        const int xa = (int)(((4u - (unsigned)((uintptr_t)orow & 3)) & 3u) * 3u) & 3;
        const int x0 = xa - 4 + 4 * g;
        if (x0 + 4 <= 0 || x0 >= w) continue;
        unsigned int wd[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = x0 + j;
            if (x >= 0 && x < w) {
                const long off = (long)y * rs + (long)x * es;
                const unsigned char c0 = stretch1<ISF>((double)p0[off], lo[0], den[0], plain[0], mode == 0);
                const unsigned char c1 = stretch1<ISF>((double)p1[off], lo[1], den[1], plain[1], false);
                const unsigned char c2 = stretch1<ISF>((double)p2[off], lo[2], den[2], plain[2], false);
                wd[(3 * j) >> 2] |= (unsigned)c0 << (8 * ((3 * j) & 3));
                wd[(3 * j + 1) >> 2] |= (unsigned)c1 << (8 * ((3 * j + 1) & 3));
                wd[(3 * j + 2) >> 2] |= (unsigned)c2 << (8 * ((3 * j + 2) & 3));
            }
        }
        if (x0 >= 0 && x0 + 4 <= w) {
            unsigned int* o = reinterpret_cast<unsigned int*>(orow + 3L * x0);
            o[0] = wd[0];
            o[1] = wd[1];
            o[2] = wd[2];
        } else {
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                const int x = x0 + q / 3;
                if (x >= 0 && x < w) orow[3L * x0 + q] = (unsigned char)(wd[q >> 2] >> (8 * (q & 3)));
            }
        }
    }
}

template <typename T>
void launch_pass(const void* bands, int h, int w, long bs, long rs, long es, Sel3 sel, int n_sel, int pass, int shift, unsigned* hist,
                 const SelState* st, int* nonfinite, hipStream_t s) {
    hipLaunchKernelGGL(band_hist_kernel<T>, dim3(h < HIST_BLOCKS ? h : HIST_BLOCKS, n_sel), dim3(TPB), 0, s, (const T*)bands, h, w, bs, rs, es, sel,
                       pass, shift, hist, st, nonfinite);
}

template <typename T, bool ISF>
void launch_stretch(const void* bands, int h, int w, long bs, long rs, long es, Sel3 sel, const double* pct, int mode, unsigned char* out, long ors,
                    hipStream_t s) {
    hipLaunchKernelGGL((band_stretch_kernel<T, ISF>), dim3(cdiv(w / 4 + 2, TPB), h < 65535 ? h : 65535), dim3(TPB), 0, s, (const T*)bands, h, w, bs,
                       rs, es, sel, pct, mode, out, ors);
}
}  // namespace

extern "C" long runet_band_percentiles_workspace(int n_sel) {
    if (n_sel < 1 || n_sel > MAXSEL) return -1;
    return (long)MAXPASS * n_sel * SLOTS * BINS * (long)sizeof(unsigned) + (long)sizeof(SelState);
}

// ev (NULL in the product path): passes + 1 events, recorded before the first pass and after each pass's scan
static int band_percentiles_impl(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride, long elem_stride,
                                 int sel0, int sel1, int sel2, int n_sel, long k_lo, double g_lo, long k_hi, double g_hi, int wide_diff,
                                 double* pct, int* nonfinite, void* workspace, long workspace_bytes, void* stream, hipEvent_t* ev) {
    RUNET_REQUIRE(bands && pct && nonfinite && workspace, "null pointer");
    RUNET_REQ_BANDS();
    RUNET_REQUIRE(n_sel >= 1 && n_sel <= MAXSEL, "1..3 selected bands");
    const Sel3 sel = {{sel0, sel1, sel2}};
    for (int i = 0; i < n_sel; ++i) RUNET_REQUIRE(sel.i[i] >= 0 && sel.i[i] < n_bands, "selected band out of range");
    const long n = (long)h * w;
    RUNET_REQUIRE(k_lo >= 0 && k_lo <= k_hi && k_hi < n, "ranks must satisfy 0 <= k_lo <= k_hi < h * w");
    RUNET_REQUIRE(g_lo >= 0.0 && g_lo < 1.0 && g_hi >= 0.0 && g_hi < 1.0, "gammas must lie in [0, 1)");
    RUNET_REQUIRE(workspace_bytes >= runet_band_percentiles_workspace(n_sel), "workspace too small");
    RUNET_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)pct & 7) == 0 && ((uintptr_t)nonfinite & 3) == 0, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const long hist_words = (long)n_sel * SLOTS * BINS;
    unsigned* hist = (unsigned*)workspace;
    SelState* st = (SelState*)(hist + MAXPASS * hist_words);
    if (hipMemsetAsync(workspace, 0, (size_t)runet_band_percentiles_workspace(n_sel), s) != hipSuccess ||
        hipMemsetAsync(nonfinite, 0, sizeof(int), s) != hipSuccess) {
        (void)hipGetLastError();
        runet_set_error("runet_band_percentiles: clearing the workspace failed");
        return RUNET_ELAUNCH;
    }
    const int passes = runet_band_elem_size(dtype) == 1 ? 1 : runet_band_elem_size(dtype) == 2 ? 2 : 4;
    if (ev) (void)hipEventRecord(ev[0], s);
    for (int p = 0; p < passes; ++p) {
        const int shift = 8 * (passes - 1 - p);
        unsigned* hp = hist + p * hist_words;
        switch (dtype) {
            case RUNET_BAND_U8: launch_pass<unsigned char>(bands, h, w, band_stride, row_stride, elem_stride, sel, n_sel, p, shift, hp, st, nonfinite, s); break;
            case RUNET_BAND_U16: launch_pass<unsigned short>(bands, h, w, band_stride, row_stride, elem_stride, sel, n_sel, p, shift, hp, st, nonfinite, s); break;
            case RUNET_BAND_I16: launch_pass<short>(bands, h, w, band_stride, row_stride, elem_stride, sel, n_sel, p, shift, hp, st, nonfinite, s); break;
            default: launch_pass<float>(bands, h, w, band_stride, row_stride, elem_stride, sel, n_sel, p, shift, hp, st, nonfinite, s); break;
        }
        hipLaunchKernelGGL(band_scan_kernel, dim3(1), dim3(64), 0, s, hp, st, n_sel, p, shift, p == passes - 1 ? 1 : 0, (unsigned)n, (unsigned)k_lo,
                           (unsigned)k_hi, g_lo, g_hi, dtype, wide_diff ? 1 : 0, pct);
        if (ev) (void)hipEventRecord(ev[p + 1], s);
    }
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_band_percentiles(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride, long elem_stride,
                                      int sel0, int sel1, int sel2, int n_sel, long k_lo, double g_lo, long k_hi, double g_hi, int wide_diff,
                                      double* pct, int* nonfinite, void* workspace, long workspace_bytes, void* stream) {
    return band_percentiles_impl(bands, dtype, n_bands, h, w, band_stride, row_stride, elem_stride, sel0, sel1, sel2, n_sel, k_lo, g_lo, k_hi, g_hi,
                                 wide_diff, pct, nonfinite, workspace, workspace_bytes, stream, nullptr);
}

// Measurement only (tools/bench_scene.py): the same call with a device event around every pass; SYNCHRONISES the host and writes the passes'
// milliseconds (hist + scan launch each) to the host array pass_ms [4] (unused entries 0).
extern "C" int runet_band_percentiles_timed(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride,
                                            long elem_stride, int sel0, int sel1, int sel2, int n_sel, long k_lo, double g_lo, long k_hi,
                                            double g_hi, int wide_diff, double* pct, int* nonfinite, void* workspace, long workspace_bytes,
                                            void* stream, float* pass_ms) {
    RUNET_REQUIRE(pass_ms, "null pointer");
    hipEvent_t ev[MAXPASS + 1];
    for (int i = 0; i <= MAXPASS; ++i) RUNET_REQUIRE(hipEventCreate(&ev[i]) == hipSuccess, "hipEventCreate failed");
    const int rc = band_percentiles_impl(bands, dtype, n_bands, h, w, band_stride, row_stride, elem_stride, sel0, sel1, sel2, n_sel, k_lo, g_lo, k_hi,
                                         g_hi, wide_diff, pct, nonfinite, workspace, workspace_bytes, stream, ev);
    const int passes = rc ? 0 : (dtype == RUNET_BAND_U8 ? 1 : dtype == RUNET_BAND_F32 ? 4 : 2);
    for (int p = 0; p < MAXPASS; ++p) {
        pass_ms[p] = 0.f;
        if (p < passes && (hipEventSynchronize(ev[p + 1]) != hipSuccess || hipEventElapsedTime(&pass_ms[p], ev[p], ev[p + 1]) != hipSuccess)) {
            (void)hipGetLastError();
            pass_ms[p] = -1.f;
        }
    }
    for (int i = 0; i <= MAXPASS; ++i) (void)hipEventDestroy(ev[i]);
    return rc;
}

extern "C" int runet_band_stretch_u8(const void* bands, int dtype, int n_bands, int h, int w, long band_stride, long row_stride, long elem_stride,
                                     int sel0, int sel1, int sel2, const double* pct, int mode, unsigned char* out, long out_row_stride,
                                     void* stream) {
    RUNET_REQUIRE(bands && pct && out, "null pointer");
    RUNET_REQ_BANDS();
    const Sel3 sel = {{sel0, sel1, sel2}};
    for (int i = 0; i < MAXSEL; ++i) RUNET_REQUIRE(sel.i[i] >= 0 && sel.i[i] < n_bands, "selected band out of range");
    RUNET_REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (water), 1 (rgb) or 2 (display)");
    RUNET_REQUIRE(out_row_stride >= 3L * w, "output row stride smaller than 3 * w");
    RUNET_REQUIRE(((uintptr_t)pct & 7) == 0, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    switch (dtype) {
        case RUNET_BAND_U8: launch_stretch<unsigned char, false>(bands, h, w, band_stride, row_stride, elem_stride, sel, pct, mode, out, out_row_stride, s); break;
        case RUNET_BAND_U16: launch_stretch<unsigned short, false>(bands, h, w, band_stride, row_stride, elem_stride, sel, pct, mode, out, out_row_stride, s); break;
        case RUNET_BAND_I16: launch_stretch<short, false>(bands, h, w, band_stride, row_stride, elem_stride, sel, pct, mode, out, out_row_stride, s); break;
        default: launch_stretch<float, true>(bands, h, w, band_stride, row_stride, elem_stride, sel, pct, mode, out, out_row_stride, s); break;
    }
    RUNET_CHECK_LAUNCH();
}
