// Exact squared Euclidean distance transform of a batch of byte masks, and the integer / float64 statistics of a distance map that the
// coastline-accuracy scores are made of (boundary.py; include/runet_hip.h states the rules, tests/edt_ref.py restates them in numpy).
//
// The squared distance between two pixels is an integer, so the transform is defined exactly: d2 = min over feature pixels of dx^2 + dy^2.
// It separates: pass 1 finds, along every row, the distance g to the nearest feature of that row; pass 2 takes, along every column, the
// lower envelope of the parabolas (y - y')^2 + g(y')^2 (Meijster, Roerdink, Hesselink 2000).  Pass 1 is the one along rows because a
// row is contiguous: a wave scans it 64 pixels at a time.  Pass 2 gives a column to a thread, so the 64 lanes of a wave walk 64 adjacent
// columns and every load and store of the walk is one contiguous 256 bytes.
//
// Pass 2 works in place on d2.  A column of d2 first holds g, then the envelope's stack, then the result: stack entry q is written at
// row u >= q, after g(u) has been read (and the rows ahead are read before the rows behind are written, see PF), and in the fill from
// the last row upwards the result of row u >= q lands on a stack entry that is either dead (u > q) or popped by this very step
// (u == q).  Only the entries' start rows live in the workspace: 2 bytes per pixel.
//
// "This row has no feature" is the state g = -1; such a row never becomes a parabola and never meets any arithmetic.  Everything is
// integer; the intersections are formed in 64 bits.  Every loop runs at most h or w times.
#include "runet_common.h"
#include "../../include/runet_hip.h"

// the one floating-point chain (the sum of the roots) has a stated order: no FMA, no reassociation
#pragma clang fp contract(off)

namespace {
constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int ROW_GRID_CAP = 16384;              // pass 1: blocks of four waves, a wave per row, grid-stride over the rows
constexpr int COL_TPB = 64;                      // pass 2: one wave per block, so that 10980 columns spread over 172 CUs, not 43
constexpr int PF = 8;                            // pass 2: rows of g read ahead of the row being worked on
constexpr int CHUNK = 4 * TPB;                   // stats: pixels per block, the unit of the root sum's order
constexpr int MAX_TOL = 8;
constexpr int FAR = 1 << 20;                     // pass 1: "no feature to the right" inside the wave scan; compared, never added to

struct Tol { int sq[MAX_TOL]; };

// ---- pass 1: nearest feature along the row ----
// Forward: d2[x] = the last feature column <= x (-1: none), a running maximum carried from chunk to chunk.  Backward: the first feature
// column >= x as a running minimum (x is a feature exactly where the forward value equals x), and g = the smaller of the two gaps.
__global__ __launch_bounds__(TPB) void edt_row_kernel(const unsigned char* __restrict__ mask, long rows, int h, int w, long rs, long is, int invert,
                                                       int* __restrict__ d2) {
    const int lane = threadIdx.x & 63;
    const int chunks = (w + 63) >> 6;
    for (long r = (long)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * WAVES) {
        const long i = r / h, y = r - i * h;
        const unsigned char* src = mask + i * is + y * rs;
        int* dst = d2 + r * w;
        int carry = -1;
        for (int c = 0; c < chunks; ++c) {
            const int x = (c << 6) + lane;
            int v = -1;
            if (x < w && ((src[x] != 0) != (invert != 0))) v = x;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(v, o, 64);
                if (lane >= o) v = t > v ? t : v;
            }
            v = carry > v ? carry : v;
            carry = __shfl(v, 63, 64);
            if (x < w) dst[x] = v;
        }
        carry = FAR;
        for (int c = chunks - 1; c >= 0; --c) {
            const int x = (c << 6) + lane;
            const int left = x < w ? dst[x] : -1;
            int v = left == x ? x : FAR;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_down(v, o, 64);
                if (lane + o < 64) v = t < v ? t : v;
            }
            v = carry < v ? carry : v;
            carry = __shfl(v, 0, 64);
            if (x < w) {
                int g = left >= 0 ? x - left : -1;
                if (v != FAR && (g < 0 || v - x < g)) g = v - x;
                dst[x] = g;
            }
        }
    }
}

// ---- pass 2: lower envelope along the column ----
// floor(a / b) for b > 0
__device__ __forceinline__ long floor_div(long a, long b) {
    const long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// A stack entry is the parabola of row s with root g (packed s | g << 15, both below 2^15) and the first row t it owns (workspace).
// The top entry lives in registers; memory is read again only after a pop.
__global__ __launch_bounds__(COL_TPB) void edt_col_kernel(int* __restrict__ d2, unsigned short* __restrict__ start, long cols, int h, int w) {
    const long id = (long)blockIdx.x * COL_TPB + threadIdx.x;
    if (id >= cols) return;
    const long i = id / w, x = id - i * w;
    int* col = d2 + i * h * w + x;
    unsigned short* tb = start + i * h * w + x;
    int q = -1, ts = 0, tg = 0, tt = 0;
    for (int u0 = 0; u0 < h; u0 += PF) {
        int gbuf[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) gbuf[j] = u0 + j < h ? col[(long)(u0 + j) * w] : -1;
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int u = u0 + j, g = gbuf[j];
            if (g < 0) continue;
            const long fu = (long)g * g;
            // a top entry that loses to u on its own first row owns nothing any more (at most q + 1 <= h pops)
            while (q >= 0) {
                const long a = (long)(tt - ts) * (tt - ts) + (long)tg * tg, b = (long)(tt - u) * (tt - u) + fu;
                if (a <= b) break;
                --q;
                if (q >= 0) {
                    const int e = col[(long)q * w];
                    ts = e & 0x7fff;
                    tg = e >> 15;
                    tt = tb[(long)q * w];
                }
            }
            bool push = false;
            if (q < 0) {
                tt = 0;
                push = true;
            } else {
                // the last row on which ts still wins against u (ties go to ts); u owns the rows after it, if any lie inside the column
                const long sep = floor_div((long)u * u - (long)ts * ts + fu - (long)tg * tg, 2L * (u - ts));
                if (sep + 1 < h) {
                    tt = (int)(sep + 1);
                    push = true;
                }
            }
            if (push) {
                ++q;
                ts = u;
                tg = g;
                col[(long)q * w] = ts | (tg << 15);
                tb[(long)q * w] = (unsigned short)tt;
            }
        }
    }
    if (q < 0) {                                         // no row of the image has a feature
        for (int u = 0; u < h; ++u) col[(long)u * w] = RUNET_EDT_NONE;
        return;
    }
    for (int u = h - 1; u >= 0; --u) {
        col[(long)u * w] = (u - ts) * (u - ts) + tg * tg;
        if (u == tt) {
            --q;
            if (q >= 0) {
                const int e = col[(long)q * w];
                ts = e & 0x7fff;
                tg = e >> 15;
                tt = tb[(long)q * w];
            }
        }
    }
}

// ---- statistics of a distance map ----
// Block b of image blockIdx.x / nblk owns the pixels [CHUNK b, CHUNK (b + 1)); thread t takes the pixels CHUNK b + t + TPB j.  The order of
// the root sum is stated in include/runet_hip.h (the same shape as runet_error_overlays').
__global__ __launch_bounds__(TPB) void edt_stats_kernel(const int* __restrict__ d2, const unsigned char* __restrict__ select, long hw, int nblk,
                                                         Tol tol, int n_tol, unsigned long long* __restrict__ counts, double* __restrict__ part) {
    __shared__ double wsum[WAVES];
    __shared__ unsigned long long red[WAVES][4 + MAX_TOL];
    const long s = blockIdx.x / nblk, b = blockIdx.x - s * nblk;
    double acc = 0.0;
    unsigned long long c_sel = 0, c_none = 0, mx = 0, sum = 0, within[MAX_TOL];
#pragma unroll
    for (int k = 0; k < MAX_TOL; ++k) within[k] = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long p = b * CHUNK + threadIdx.x + TPB * j;
        double e = 0.0;
        if (p < hw && (select == nullptr || select[s * hw + p] != 0)) {
            const int v = d2[s * hw + p];
            ++c_sel;
            if (v == RUNET_EDT_NONE) {
                ++c_none;
            } else {
                const unsigned long long uv = (unsigned long long)(unsigned int)v;
                mx = uv > mx ? uv : mx;
                sum += uv;
#pragma unroll
                for (int k = 0; k < MAX_TOL; ++k) within[k] += (k < n_tol && v <= tol.sq[k]) ? 1ull : 0ull;
                e = __dsqrt_rn((double)v);
            }
        }
        acc += e;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        c_sel += __shfl_xor(c_sel, o, 64);
        c_none += __shfl_xor(c_none, o, 64);
        sum += __shfl_xor(sum, o, 64);
        const unsigned long long m = __shfl_xor(mx, o, 64);
        mx = m > mx ? m : mx;
#pragma unroll
        for (int k = 0; k < MAX_TOL; ++k) within[k] += __shfl_xor(within[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        wsum[wv] = acc;
        red[wv][0] = c_sel, red[wv][1] = c_none, red[wv][2] = mx, red[wv][3] = sum;
#pragma unroll
        for (int k = 0; k < MAX_TOL; ++k) red[wv][4 + k] = within[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    if (threadIdx.x < 4 + n_tol) {
        const int i = threadIdx.x;
        unsigned long long v = red[0][i];
#pragma unroll
        for (int k = 1; k < WAVES; ++k) v = i == 2 ? (red[k][i] > v ? red[k][i] : v) : v + red[k][i];
        unsigned long long* dst = counts + s * (4 + n_tol) + i;
        if (v) {
            if (i == 2) atomicMax(dst, v);
            else atomicAdd(dst, v);
        }
    }
}

// one wave per image: lane l adds the chunk sums l, l + 64, ... in that order, then the lanes fold (32, 16, ..., 1)
__global__ __launch_bounds__(64) void edt_sum_kernel(const double* __restrict__ part, int nblk, double* __restrict__ sums) {
    const double* p = part + (long)blockIdx.x * nblk;
    double acc = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 64) acc += p[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (threadIdx.x == 0) sums[blockIdx.x] = acc;
}

constexpr int MAX_SIDE = 32768;                          // (h - 1)^2 + (w - 1)^2 stays below RUNET_EDT_NONE
constexpr long MAX_BLOCKS = 2147483647L;
}  // namespace

extern "C" long runet_edt_workspace_bytes(int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1 || h > MAX_SIDE || w > MAX_SIDE) return -1;
    const long hw = (long)h * w;
    const long nblk = (hw + CHUNK - 1) / CHUNK;
    if ((long)n * nblk > MAX_BLOCKS || (long)n * ((w + COL_TPB - 1) / COL_TPB + 1) > MAX_BLOCKS) return -1;
    const long starts = ((long)n * hw * (long)sizeof(unsigned short) + 7) / 8 * 8, parts = (long)n * nblk * (long)sizeof(double);
    return starts > parts ? starts : parts;
}

extern "C" int runet_edt_sq_u8(const unsigned char* mask, int n, int h, int w, long row_stride, long image_stride, int invert, int* d2,
                               void* workspace, long workspace_bytes, void* stream) {
    RUNET_REQUIRE(mask && d2 && workspace, "null pointer");
    RUNET_REQUIRE(n >= 1 && h >= 1 && w >= 1, "bad shape");
    RUNET_REQUIRE(h <= MAX_SIDE && w <= MAX_SIDE, "h and w must not exceed 32768");
    RUNET_REQUIRE(row_stride >= w, "row stride smaller than a row");
    RUNET_REQUIRE(n == 1 || image_stride >= (long)(h - 1) * row_stride + w, "image stride smaller than an image's extent");
    const long need = runet_edt_workspace_bytes(n, h, w);
    RUNET_REQUIRE(need >= 0, "batch too large");
    RUNET_REQUIRE(workspace_bytes >= need, "workspace too small");
    RUNET_REQUIRE(((uintptr_t)d2 & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const long rows = (long)n * h, cols = (long)n * w;
    long rb = (rows + WAVES - 1) / WAVES;
    if (rb > ROW_GRID_CAP) rb = ROW_GRID_CAP;
    hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)rb), dim3(TPB), 0, s, mask, rows, h, w, row_stride, image_stride, invert, d2);
    hipLaunchKernelGGL(edt_col_kernel, dim3((unsigned)((cols + COL_TPB - 1) / COL_TPB)), dim3(COL_TPB), 0, s, d2, (unsigned short*)workspace, cols,
                       h, w);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_edt_stats(const int* d2, const unsigned char* select, int n, int h, int w, const int* tol_sq, int n_tol, long* counts,
                               double* sums, void* workspace, long workspace_bytes, void* stream) {
    RUNET_REQUIRE(d2 && counts && sums && workspace, "null pointer");
    RUNET_REQUIRE(n >= 1 && h >= 1 && w >= 1, "bad shape");
    RUNET_REQUIRE(h <= MAX_SIDE && w <= MAX_SIDE, "h and w must not exceed 32768");
    RUNET_REQUIRE(n_tol >= 0 && n_tol <= MAX_TOL, "0..8 tolerances");
    RUNET_REQUIRE(n_tol == 0 || tol_sq, "null pointer");
    const long need = runet_edt_workspace_bytes(n, h, w);
    RUNET_REQUIRE(need >= 0, "batch too large");
    RUNET_REQUIRE(workspace_bytes >= need, "workspace too small");
    RUNET_REQUIRE(((uintptr_t)d2 & 3) == 0 && (((uintptr_t)counts | (uintptr_t)sums | (uintptr_t)workspace) & 7) == 0, "misaligned pointer");
    Tol tol;
    for (int k = 0; k < MAX_TOL; ++k) {
        tol.sq[k] = k < n_tol ? tol_sq[k] : -1;
        RUNET_REQUIRE(k >= n_tol || tol.sq[k] >= 0, "a squared tolerance is not negative");
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)n * (4 + n_tol) * sizeof(long), s) != hipSuccess) {
        (void)hipGetLastError();
        runet_set_error("runet_edt_stats: clearing the counts failed");
        return RUNET_ELAUNCH;
    }
    const long hw = (long)h * w;
    const int nblk = cdiv(hw, CHUNK);
    hipLaunchKernelGGL(edt_stats_kernel, dim3((unsigned)((long)n * nblk)), dim3(TPB), 0, s, d2, select, hw, nblk, tol, n_tol,
                       (unsigned long long*)counts, (double*)workspace);
    hipLaunchKernelGGL(edt_sum_kernel, dim3(n), dim3(64), 0, s, (const double*)workspace, nblk, sums);
    RUNET_CHECK_LAUNCH();
}
