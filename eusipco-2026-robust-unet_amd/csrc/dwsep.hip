// Fast-SCNN's DepthwiseSeparableConv (comne.py:305-320: depthwise 3x3, stride 1 | 2 -> pointwise 1x1 -> BatchNorm -> ReLU) with the depthwise
// tensor d kept out of HBM in both passes.  The layers are bound by bytes and launches (no channel count above 128, the largest layer of a
// 16 x 256^2 step is 0.5 GFLOP), so the pointwise product runs on the exact f32-input MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain, no
// narrower format anywhere) and the work of the kernels is to stream x / t / dt once.
//
//   runet_dwsep_fwd        a block takes TM = 64 consecutive output pixels: the whole pointwise weight [cin][cout] goes to LDS, the depthwise
//                          outputs of the tile are computed by dw3_point (dw3_common.h; the 3x3 neighbourhoods come from L1 / L2) into LDS as
//                          the product's A operand, four waves multiply (wave = 16 pixels x all output channels), the raw pointwise output t
//                          leaves through an LDS tile with 16-byte stores, and the tile's BatchNorm partials (count, mean, M2) per channel are
//                          taken from that tile in pixel order - the layout runet_bn_stats_finalize consumes.
//   runet_dwsep_wgrad_pw   dWp [cin][cout] = d^T dt over chunks of pixel tiles: d recomputed by the same dw3_point (bit-equal to the
//                          forward's), dt staged beside it, the chunk partials added in index order by sum_parts<32> (runet_common.h).
//
// LDS rows are padded so that the four k-rows an MFMA operand load touches fall on disjoint banks.  No float atomics, fixed summation order
// everywhere: two runs give the same bits.
#include "dw3_common.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int TPB = 256, TM = 64, ALD = TM + 16;
constexpr int MAXC = 128;
constexpr int MAX_CHUNKS = 128;

__host__ __device__ inline int pad16(int c) { return (c % 32 == 16) ? c : c + 16; }      // row stride = 16 mod 32 floats

// the depthwise output of output pixel p (over all images), channels c..c+3
__device__ __forceinline__ f32x4 dw_at(const float* __restrict__ x, int ldx, const float* __restrict__ wd, long p, int c, int H, int W, int Ho, int Wo,
                                       int C, int stride) {
    const int ow = (int)(p % Wo);
    const long t = p / Wo;
    const int oh = (int)(t % Ho);
    const float* xi = x + (t / Ho) * H * W * (long)ldx + c;
    f32x4 wv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wv[k] = ld4(wd + k * C + c);
    return dw3_point([&](int ih, int iw) { return ld4(xi + ((long)ih * W + iw) * ldx); }, wv, oh, ow, H, W, stride);
}

__global__ __launch_bounds__(TPB) void dwsep_fwd_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ wd, const float* __restrict__ wp,
                                                        float* __restrict__ t, int ldt, float* __restrict__ part, long P, int H, int W, int Ho, int Wo,
                                                        int cin, int cout, int stride) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int wld = pad16(cout), tld = cout + 4;
    float* Wl = sm;                      // [cin][wld]
    float* At = Wl + cin * wld;          // [cin][ALD]: d transposed, At[k][pixel]
    float* Tl = At + cin * ALD;          // [TM][tld]
    const int tid = threadIdx.x;
    const long p0 = (long)blockIdx.x * TM;
    const int valid = (int)min((long)TM, P - p0);
    for (int i = tid; i < cin * cout / 4; i += TPB) {
        const int k = (i * 4) / cout, j = (i * 4) % cout;
        st4(Wl + k * wld + j, ld4(wp + (long)i * 4));
    }
    const int cv = cin >> 2;
    for (int i = tid; i < TM * cv; i += TPB) {
        const int m = i % TM, c = (i / TM) * 4;
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
        if (m < valid) d = dw_at(x, ldx, wd, p0 + m, c, H, W, Ho, Wo, cin, stride);
#pragma unroll
        for (int e = 0; e < 4; ++e) At[(c + e) * ALD + m] = d[e];
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int ntc = cout >> 4;
    f32x4 acc[MAXC / 16];
#pragma unroll
    for (int nt = 0; nt < MAXC / 16; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < cv; ++ks) {
        const float a = At[(4 * ks + lk) * ALD + 16 * wave + li];
        const float* brow = Wl + (4 * ks + lk) * wld + li;
#pragma unroll
        for (int nt = 0; nt < MAXC / 16; ++nt)
            if (nt < ntc) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, brow[16 * nt], acc[nt], 0, 0, 0);
    }
    // C/D map of the 16x16 tile: column = lane & 15, row = 4 * (lane >> 4) + register
#pragma unroll
    for (int nt = 0; nt < MAXC / 16; ++nt)
        if (nt < ntc) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Tl[(16 * wave + 4 * lk + r) * tld + 16 * nt + li] = acc[nt][r];
        }
    __syncthreads();
    const int ov = cout >> 2;
    for (int i = tid; i < valid * ov; i += TPB) {
        const int m = i / ov, c = (i % ov) * 4;
        st4(t + (p0 + m) * ldt + c, ld4(Tl + m * tld + c));
    }
    if (tid < cout) {
        float s = 0.f;
        for (int m = 0; m < valid; ++m) s += Tl[m * tld + tid];
        const float mean = s / (float)valid;
        float m2 = 0.f;
        for (int m = 0; m < valid; ++m) {
            const float d = Tl[m * tld + tid] - mean;
            m2 = __builtin_fmaf(d, d, m2);
        }
        float* o = part + ((long)blockIdx.x * cout + tid) * 3;
        o[0] = (float)valid; o[1] = mean; o[2] = m2;
    }
}

// grid (chunks); a block walks its pixel tiles, accumulating the whole [cin][cout] product in registers: 16 x 16 tile tt = wave + 4 q
__global__ __launch_bounds__(TPB) void dwsep_wgrad_pw_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ wd,
                                                             const float* __restrict__ dt, int lddt, float* __restrict__ part, long P, int H, int W,
                                                             int Ho, int Wo, int cin, int cout, int stride, int tiles, int tpc) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int dld = pad16(cin), gld = pad16(cout);
    float* Dl = sm;                      // [TM][dld]
    float* Gl = Dl + TM * dld;           // [TM][gld]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int cv = cin >> 2, ov = cout >> 2, ntc = cout >> 4, ntiles = (cin >> 4) * ntc;
    constexpr int Q = (MAXC / 16) * (MAXC / 16) / 4;
    f32x4 acc[Q];
    int aoff[Q], boff[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int tt = wave + 4 * q;
        aoff[q] = 16 * (tt / ntc) + li;
        boff[q] = 16 * (tt % ntc) + li;
    }
    const int tile0 = blockIdx.x * tpc, tile1 = min(tiles, tile0 + tpc);
    for (int tile = tile0; tile < tile1; ++tile) {
        const long p0 = (long)tile * TM;
        const int valid = (int)min((long)TM, P - p0);
        __syncthreads();
        for (int i = tid; i < TM * cv; i += TPB) {
            const int m = i / cv, c = (i % cv) * 4;
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
            if (m < valid) d = dw_at(x, ldx, wd, p0 + m, c, H, W, Ho, Wo, cin, stride);
            st4(Dl + m * dld + c, d);
        }
        for (int i = tid; i < TM * ov; i += TPB) {
            const int m = i / ov, c = (i % ov) * 4;
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            if (m < valid) g = ld4(dt + (p0 + m) * lddt + c);
            st4(Gl + m * gld + c, g);
        }
        __syncthreads();
        for (int ks = 0; ks < TM / 4; ++ks) {
            const float* arow = Dl + (4 * ks + lk) * dld;
            const float* brow = Gl + (4 * ks + lk) * gld;
#pragma unroll
            for (int q = 0; q < Q; ++q)
                if (wave + 4 * q < ntiles) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[aoff[q]], brow[boff[q]], acc[q], 0, 0, 0);
        }
    }
    float* o = part + (long)blockIdx.x * cin * cout;
#pragma unroll
    for (int q = 0; q < Q; ++q)
        if (wave + 4 * q < ntiles) {
            const int ci = aoff[q] - li + 4 * lk, co = boff[q];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[(ci + r) * cout + co] = acc[q][r];
        }
}

inline size_t fwd_lds(int cin, int cout) { return (size_t)(cin * pad16(cout) + cin * ALD + TM * (cout + 4)) * sizeof(float); }
inline size_t wgrad_lds(int cin, int cout) { return (size_t)TM * (pad16(cin) + pad16(cout)) * sizeof(float); }

// kernels that may ask for more than the default 64 KB of dynamic LDS say so once (not a stream operation: done before the first launch)
template <class K>
inline bool allow_lds(K kernel, size_t bytes, bool& done) {
    if (done) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    done = true;
    return true;
}

inline void out_hw(int h, int w, int stride, int& ho, int& wo) { ho = (h + stride - 1) / stride; wo = (w + stride - 1) / stride; }
inline int wgrad_chunks(int tiles, int& tpc) {
    tpc = (tiles + MAX_CHUNKS - 1) / MAX_CHUNKS;
    return (tiles + tpc - 1) / tpc;
}
}  // namespace

#define DS_REQ_SHAPE(n, h, w, cin, cout, stride)                                                                                          \
    RUNET_REQUIRE((n) > 0 && (h) > 0 && (w) > 0 && (cin) >= 16 && (cin) % 16 == 0 && (cin) <= MAXC && (cout) >= 16 && (cout) % 16 == 0 && \
                      (cout) <= MAXC && ((stride) == 1 || (stride) == 2) && (long)(n) * (h) * (w) < (1L << 31) * TM,                       \
                  "bad shape (cin and cout multiples of 16, at most 128; stride 1 or 2)")

extern "C" int runet_dwsep_parts(int n_img, int h, int w_, int stride) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || (stride != 1 && stride != 2)) return -1;
    int ho, wo;
    out_hw(h, w_, stride, ho, wo);
    const long tiles = ((long)n_img * ho * wo + TM - 1) / TM;
    return tiles < (1L << 31) ? (int)tiles : -1;
}

extern "C" int runet_dwsep_fwd(const float* x, int ldx, const float* wd, const float* wp, float* t, int ldt, float* part, int n_img, int h, int w_,
                               int cin, int cout, int stride, void* stream) {
    RUNET_REQUIRE(x && wd && wp && t && part, "null pointer");
    DS_REQ_SHAPE(n_img, h, w_, cin, cout, stride);
    RUNET_REQ_LD(ldx, cin, x);
    RUNET_REQ_LD(ldt, cout, t);
    RUNET_REQUIRE(((uintptr_t)wd % 16) == 0 && ((uintptr_t)wp % 16) == 0, "weights must be 16-byte aligned");
    static bool lds_ok = false;
    RUNET_REQUIRE(allow_lds(dwsep_fwd_kernel, fwd_lds(MAXC, MAXC), lds_ok), "the device refused the kernel's LDS size");
    int ho, wo;
    out_hw(h, w_, stride, ho, wo);
    const long P = (long)n_img * ho * wo;
    hipLaunchKernelGGL(dwsep_fwd_kernel, dim3((unsigned)((P + TM - 1) / TM)), dim3(TPB), fwd_lds(cin, cout), (hipStream_t)stream, x, ldx, wd, wp, t, ldt,
                       part, P, h, w_, ho, wo, cin, cout, stride);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_dwsep_wgrad_pw_workspace_floats(int n_img, int h, int w_, int cin, int cout, int stride) {
    const int tiles = runet_dwsep_parts(n_img, h, w_, stride);
    if (tiles < 0 || cin < 16 || cin % 16 || cin > MAXC || cout < 16 || cout % 16 || cout > MAXC) return -1;
    int tpc;
    return (long)wgrad_chunks(tiles, tpc) * cin * cout;
}

extern "C" int runet_dwsep_wgrad_pw(const float* x, int ldx, const float* wd, const float* dt, int lddt, float* workspace, long workspace_floats,
                                    float* dwp, int n_img, int h, int w_, int cin, int cout, int stride, void* stream) {
    RUNET_REQUIRE(x && wd && dt && workspace && dwp, "null pointer");
    DS_REQ_SHAPE(n_img, h, w_, cin, cout, stride);
    RUNET_REQ_LD(ldx, cin, x);
    RUNET_REQ_LD(lddt, cout, dt);
    RUNET_REQUIRE(((uintptr_t)wd % 16) == 0 && ((uintptr_t)workspace % 16) == 0, "wd and the workspace must be 16-byte aligned");
    int ho, wo, tpc;
    out_hw(h, w_, stride, ho, wo);
    const long P = (long)n_img * ho * wo;
    const int tiles = (int)((P + TM - 1) / TM);
    const int chunks = wgrad_chunks(tiles, tpc);
    RUNET_REQUIRE(workspace_floats >= (long)chunks * cin * cout, "workspace too small (runet_dwsep_wgrad_pw_workspace_floats)");
    static bool lds_ok = false;
    RUNET_REQUIRE(allow_lds(dwsep_wgrad_pw_kernel, wgrad_lds(MAXC, MAXC), lds_ok), "the device refused the kernel's LDS size");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(dwsep_wgrad_pw_kernel, dim3(chunks), dim3(TPB), wgrad_lds(cin, cout), st, x, ldx, wd, dt, lddt, workspace, P, h, w_, ho, wo, cin,
                       cout, stride, tiles, tpc);
    sum_parts<32>(workspace, chunks, cin * cout, dwp, st);
    RUNET_CHECK_LAUNCH();
}
