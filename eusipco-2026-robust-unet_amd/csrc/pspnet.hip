// PSPNet baseline (the reference's comne.py:214-299): what the shared kernels cannot express.
//
//   tap planes     final_conv.0 is a 3x3 convolution over cat[x, up(P_1), up(P_2), up(P_3), up(P_6)] (:240, :279).  The convolution and the
//                  bilinear resize are linear and a channel mix commutes with a per-channel resize, so the pyramid half of its input is
//                  multiplied on the 50 cells per image: Z_j[n][cy][cx][r][s][:] = P_j[n][cy][cx][:] . W[r][s][branch j's rows][:] (a small GEMM
//                  through the shared 1x1 convolution), and
//                      t[n][y][x][:] += sum_j sum_(r, s) up(Z_j[..][r][s][:])[y + r - 1][x + s - 1]          (zero outside the map)
//                  which is the zero padding of the concat.  runet_psp_taps_fwd does the sum separably: rows into LDS, then columns.
//                  runet_psp_taps_bwd is the adjoint in gather form, columns first (into a workspace), then rows.
//   head           final_conv.1-4 (:280-283): z = b + sum_c relu(t * scale + shift)[c] * mask[n][c] * w[c]; neither the activated tensor nor
//                  its gradient exists.  One pass over t gives dw, db and the BatchNorm sums, a second one dt (the structure of
//                  runet_hr_head_bwd_*, with the Dropout2d mask and for up to 1024 channels).
//
// NHWC fp32, 16-byte accesses along the channels, every tensor with a pixel stride of its own.  Every sum has a fixed order (per-thread
// serial, LDS in row order, partials in index order; no float atomics), so results are bitwise reproducible.  Source-index rule: bilin_src of
// runet_common.h with scale = b / size, as runet_pyramid_upsample_fwd.
#include "runet_common.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int TPB = 256;
constexpr int MAX_PARTS = 1024;      // blocks of a partial reduction (rows of the caller's workspace)
constexpr int TAP_CHUNK = 128;       // output channels per block of psp_taps_fwd_kernel: U = 12 x 3 x 128 floats = 18 KB of LDS
constexpr int CELLS = 12;            // (branch, column) pairs of one row of the four grids: 1 + 2 + 3 + 6

__device__ __forceinline__ void psp_cell(int cell, int& j, int& b, int& cx) {
    if (cell < 1) { j = 0; b = 1; cx = 0; }
    else if (cell < 3) { j = 1; b = 2; cx = cell - 1; }
    else if (cell < 6) { j = 2; b = 3; cx = cell - 3; }
    else { j = 3; b = 6; cx = cell - 6; }
}
__device__ __forceinline__ int psp_bins(int j) { return j == 0 ? 1 : j == 1 ? 2 : j == 2 ? 3 : 6; }
__device__ __forceinline__ long psp_off(int j) { return j == 0 ? 0 : j == 1 ? 1 : j == 2 ? 5 : 14; }      // cells in front of branch j, per image
__device__ __forceinline__ int psp_cell0(int j) { return j == 0 ? 0 : j == 1 ? 1 : j == 2 ? 3 : 6; }
// rows of the branch-major buffers (fastscnn.hip): branch j starts at row N * off(j), image n at + n * b * b, cell (by, bx) at + by * b + bx
__device__ __forceinline__ void psp_row(long row, long N, int& j, int& b, long& n, int& by, int& bx) {
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

// blocks of a (channel quad x pixel row) streaming kernel over P pixels of C channels: ~`elems` elements per block, at most `cap` blocks
inline int pixel_chunks(long P, int C, long elems, int cap, long& ppc) {
    long chunks = (P * C + elems - 1) / elems;
    if (chunks > cap) chunks = cap;
    if (chunks < 1) chunks = 1;
    ppc = (P + chunks - 1) / chunks;
    return (int)((P + ppc - 1) / ppc);
}

// ------------------------------------------------------------------------------------------------------------------ tap planes, forward
// block (channel chunk, output row y, image n).  Stage 1, rows: U[cell][s][c] = sum_r sum_(the two source rows cy of row y + r - 1)
// wy * Z_j[n][cy][cx][r][s][c] for the 12 (branch, column) cells and the 3 column taps.  Stage 2, columns: a thread per (pixel of the row,
// channel quad) adds, branch by branch and tap by tap, lx0 * U[x0][s] + lx1 * U[x1][s] of column x + s - 1 and accumulates onto t.
__global__ __launch_bounds__(TPB) void psp_taps_fwd_kernel(const float* __restrict__ Z, int ldz, float* __restrict__ t, int ldt, long N, int H,
                                                           int W, int C) {
    __shared__ __attribute__((aligned(16))) float U[CELLS * 3 * TAP_CHUNK];
    const int c0 = blockIdx.x * TAP_CHUNK, y = blockIdx.y;
    const long n = blockIdx.z;
    const int cw = min(TAP_CHUNK, C - c0), qn = cw >> 2;
    for (int i = threadIdx.x; i < CELLS * 3 * qn; i += TPB) {
        const int q = i % qn, cs = i / qn, s = cs % 3, cell = cs / 3;
        int j, b, cx;
        psp_cell(cell, j, b, cx);
        const float* zp = Z + (N * psp_off(j) + n * b * b) * (long)ldz + s * C + c0 + 4 * q;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int yy = y + r - 1;
            if ((unsigned)yy >= (unsigned)H) continue;
            int y0, y1;
            float l0, l1;
            bilin_src(yy, (float)b / (float)H, b, y0, y1, l0, l1);
            acc += l0 * ld4(zp + (long)(y0 * b + cx) * ldz + r * 3 * C) + l1 * ld4(zp + (long)(y1 * b + cx) * ldz + r * 3 * C);
        }
        st4(U + (cell * 3 + s) * TAP_CHUNK + 4 * q, acc);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < W * qn; i += TPB) {
        const int q = i % qn, x = i / qn;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = psp_bins(j), cell0 = psp_cell0(j);
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int xx = x + s - 1;
                if ((unsigned)xx >= (unsigned)W) continue;
                int x0, x1;
                float l0, l1;
                bilin_src(xx, (float)b / (float)W, b, x0, x1, l0, l1);
                acc += l0 * ld4(U + ((cell0 + x0) * 3 + s) * TAP_CHUNK + 4 * q) + l1 * ld4(U + ((cell0 + x1) * 3 + s) * TAP_CHUNK + 4 * q);
            }
        }
        float* tp = t + ((n * H + y) * W + x) * (long)ldt + c0 + 4 * q;
        st4(tp, ld4(tp) + acc);
    }
}

// ------------------------------------------------------------------------------------------------------------------ tap planes, backward
// columns: V[n][y][cell][s][c] = sum over the columns xx (in index order) that read cell's column cx, with x = xx - s + 1 inside the map, of
// wx(xx, cx) * dt[n][y][x][c]; thread per element quad of V
__global__ __launch_bounds__(TPB) void psp_taps_bwd_cols_kernel(const float* __restrict__ dt, int lddt, float* __restrict__ V, long N, int H, int W,
                                                                int C) {
    const int cv = C >> 2;
    const long total = N * H * (CELLS * 3) * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int q = (int)(i % cv);
        const long u = i / cv;
        const int cs = (int)(u % (CELLS * 3)), s = cs % 3, cell = cs / 3;
        const long ny = u / (CELLS * 3);
        int j, b, cx;
        psp_cell(cell, j, b, cx);
        const float sw = (float)b / (float)W;
        int lo, hi;
        bilin_adj_range(cx, sw, W, lo, hi);
        const float* gp = dt + ny * W * (long)lddt + 4 * q;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int xx = lo; xx <= hi; ++xx) {
            const int x = xx - s + 1;
            if ((unsigned)x >= (unsigned)W) continue;
            const float wx = bilin_tap_weight(xx, sw, b, cx);
            if (wx != 0.f) acc += wx * ld4(gp + (long)x * lddt);
        }
        st4(V + i * 4, acc);
    }
}
// rows: dZ_j[n][cy][cx][r][s][c] = sum over the rows yy (in index order) that read row cy, with y = yy - r + 1 inside the map, of
// wy(yy, cy) * V[n][y][cell(j, cx)][s][c]; thread per element quad of dZ (its one owner)
__global__ __launch_bounds__(TPB) void psp_taps_bwd_rows_kernel(const float* __restrict__ V, float* __restrict__ dZ, int lddz, long N, int H, int C) {
    const int cv = C >> 2;
    const long total = N * 50 * 9 * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int q = (int)(i % cv);
        const long u = i / cv;
        const int tap = (int)(u % 9), r = tap / 3, s = tap % 3;
        const long row = u / 9;
        int j, b, by, bx;
        long n;
        psp_row(row, N, j, b, n, by, bx);
        const float sh = (float)b / (float)H;
        int lo, hi;
        bilin_adj_range(by, sh, H, lo, hi);
        const float* vp = V + ((n * H * (CELLS * 3)) + (psp_cell0(j) + bx) * 3 + s) * (long)C + 4 * q;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int yy = lo; yy <= hi; ++yy) {
            const int y = yy - r + 1;
            if ((unsigned)y >= (unsigned)H) continue;
            const float wy = bilin_tap_weight(yy, sh, b, by);
            if (wy != 0.f) acc += wy * ld4(vp + (long)y * (CELLS * 3) * C);
        }
        st4(dZ + row * lddz + tap * C + 4 * q, acc);
    }
}

// ------------------------------------------------------------------------------------------------------------------ cells' gradient
// dP_j = dZ_j . Wtap_j^T: [n b^2, 9 C] x [9 C, CQ], 100 K outputs behind a 4608-deep contraction at the workload - as one GEMM per branch that
// is one to five tiles of a tiled GEMM, each walking the whole contraction.  Here the contraction is split by tap: block (tile of 16 rows
// inside one branch, tap, 128 cells' channels) multiplies dZ[rows][tap][0:C] by wp[k][tap][0:C] through LDS in chunks of 32 (thread: 2 rows x
// 4 channels, the channel chunk walked in order) and writes part[tap][row][k]; the second kernel adds the nine taps in tap order.
constexpr int DP_ROWS = 16, DP_K = 128, DP_CO = 32;
__device__ __forceinline__ void psp_tile(long tile, long N, int& j, long& row0, long& row_end) {
    long cnt = 0;
    for (j = 0; j < 4; ++j) {
        cnt = N * psp_bins(j) * psp_bins(j);
        const long nt = (cnt + DP_ROWS - 1) / DP_ROWS;
        if (tile < nt || j == 3) break;
        tile -= nt;
    }
    row0 = N * psp_off(j) + tile * DP_ROWS;
    row_end = N * psp_off(j) + cnt;
}
__global__ __launch_bounds__(TPB) void psp_taps_dp_partial_kernel(const float* __restrict__ dZ, int lddz, const float* __restrict__ wp, int ldw,
                                                                  float* __restrict__ part, long N, int CQ, int C) {
    __shared__ __attribute__((aligned(16))) float Wt[DP_CO][DP_K + 4];      // [channel of the chunk][k]: a thread's 4 k are one 16-byte read
    __shared__ __attribute__((aligned(16))) float Zt[DP_ROWS][DP_CO];
    int j;
    long row0, row_end;
    psp_tile(blockIdx.x, N, j, row0, row_end);
    const int tap = blockIdx.y, k0 = blockIdx.z * DP_K, tid = threadIdx.x;
    const int kq = tid & 31, rr = tid >> 5;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int co0 = 0; co0 < C; co0 += DP_CO) {
        if (tid < DP_ROWS * (DP_CO / 4)) {
            const int r = tid >> 3, c4 = tid & 7;
            const long row = row0 + r;
            const int co = co0 + 4 * c4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < row_end && co < C) v = ld4(dZ + row * lddz + tap * C + co);
            st4(&Zt[r][4 * c4], v);
        }
#pragma unroll
        for (int i = 0; i < DP_K * (DP_CO / 4) / TPB; ++i) {
            const int idx = tid + i * TPB, k = idx >> 3, c4 = idx & 7;
            const int kk = k0 + k, co = co0 + 4 * c4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (kk < CQ && co < C) v = ld4(wp + (long)(j * CQ + kk) * ldw + tap * C + co);
#pragma unroll
            for (int e = 0; e < 4; ++e) Wt[4 * c4 + e][k] = v[e];
        }
        __syncthreads();
#pragma unroll 8
        for (int c = 0; c < DP_CO; ++c) {
            const f32x4 b = ld4(&Wt[c][4 * kq]);
            acc0 += Zt[2 * rr][c] * b;
            acc1 += Zt[2 * rr + 1][c] * b;
        }
        __syncthreads();
    }
    if (k0 + 4 * kq < CQ) {
        float* pp = part + ((long)tap * 50 * N) * CQ + k0 + 4 * kq;
        if (row0 + 2 * rr < row_end) st4(pp + (row0 + 2 * rr) * CQ, acc0);
        if (row0 + 2 * rr + 1 < row_end) st4(pp + (row0 + 2 * rr + 1) * CQ, acc1);
    }
}
__global__ __launch_bounds__(TPB) void psp_taps_dp_sum_kernel(const float* __restrict__ part, float* __restrict__ da, int lda, long N, int CQ) {
    const int cv = CQ >> 2;
    const long total = N * 50 * cv;
    for (long i = (long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long)gridDim.x * TPB) {
        const int q = (int)(i % cv);
        const long row = i / cv;
        f32x4 acc = ld4(part + row * CQ + 4 * q);
#pragma unroll
        for (int tap = 1; tap < 9; ++tap) acc += ld4(part + ((long)tap * 50 * N + row) * CQ + 4 * q);
        st4(da + row * lda + 4 * q, acc);
    }
}

// ------------------------------------------------------------------------------------------------------------------ head, forward
// z[p] = b + sum_c w[c] * mask[n][c] * relu(t[p][c] * scale[c] + shift[c]).  L lanes (a power of two, at most 64) share a pixel, lane l owns
// the channel quads l, l + L, ... in that order; the L partial sums meet in an in-wave butterfly.
__global__ __launch_bounds__(TPB) void psp_head_fwd_kernel(const float* __restrict__ t, int ldt, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ mask,
                                                           const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ z, long P,
                                                           long HW, int C, int L) {
    const int cv = C >> 2, lane = threadIdx.x & (L - 1), ppb = TPB / L;
    const float bias = b[0];
    for (long base = (long)blockIdx.x * ppb; base < P; base += (long)gridDim.x * ppb) {      // block-uniform bound: every lane reaches the shuffles
        const long p = base + threadIdx.x / L;
        float acc = 0.f;
        if (p < P) {
            const float* tp = t + p * ldt;
            const float* mp = mask ? mask + (p / HW) * C : nullptr;
            for (int k = lane; k < cv; k += L) {
                const f32x4 v = ld4(tp + 4 * k), sc = ld4(scale + 4 * k), sh = ld4(shift + 4 * k), wv = ld4(w + 4 * k);
                const f32x4 mk = mp ? ld4(mp + 4 * k) : f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(wv[e] * mk[e], fmaxf(bn_pre(v[e], sc[e], sh[e]), 0.f), acc);
            }
        }
        for (int o = L >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0 && p < P) z[p] = acc + bias;
    }
}

// ------------------------------------------------------------------------------------------------------------------ head, backward
// A thread owns one channel quad and every `rows`-th pixel of its block's pixel range (hrnet.hip's layout).  One pass over t and dz: per
// channel  sum g * xhat | sum g | sum dz * mask * relu(y)  and the scalar  sum dz,  y = t * scale + shift, g = dz * w * mask * (y > 0).
// part[block][3C + 1] in the order of the final result (dgamma | dbeta | dw | db).
__global__ __launch_bounds__(TPB) void psp_head_bwd_reduce_partial(const float* __restrict__ dz, const float* __restrict__ t, int ldt,
                                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                                   const float* __restrict__ mask, const float* __restrict__ w,
                                                                   const float* __restrict__ mean, const float* __restrict__ invstd, long P, long HW,
                                                                   int C, long ppc, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float sm[];       // [rows][3C + 1]
    const int cv = C >> 2, rows = TPB / cv, tid = threadIdx.x;
    const int col = tid % cv, row = tid / cv, width = 3 * C + 1;
    const long p0 = (long)blockIdx.x * ppc;
    const long p1 = p0 + ppc < P ? p0 + ppc : P;
    if (row < rows) {
        float sgx[4] = {0.f, 0.f, 0.f, 0.f}, sg[4] = {0.f, 0.f, 0.f, 0.f}, sa[4] = {0.f, 0.f, 0.f, 0.f}, sd = 0.f;
        const f32x4 sc = ld4(scale + 4 * col), sh = ld4(shift + 4 * col), wv = ld4(w + 4 * col), mu = ld4(mean + 4 * col), is = ld4(invstd + 4 * col);
        for (long p = p0 + row; p < p1; p += rows) {
            const float d = dz[p];
            const f32x4 v = ld4(t + p * ldt + 4 * col);
            const f32x4 mk = mask ? ld4(mask + (p / HW) * C + 4 * col) : f32x4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y = bn_pre(v[e], sc[e], sh[e]);
                const float dm = d * mk[e];
                const float g = y > 0.f ? dm * wv[e] : 0.f;
                sa[e] += dm * fmaxf(y, 0.f);
                sg[e] += g;
                sgx[e] += g * (v[e] - mu[e]) * is[e];
            }
            if (col == 0) sd += d;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = col * 4 + e;
            sm[row * width + c] = sgx[e]; sm[row * width + C + c] = sg[e]; sm[row * width + 2 * C + c] = sa[e];
        }
        if (col == 0) sm[row * width + 3 * C] = sd;
    }
    block_rows_to_part(sm, rows, width, part);
}
// dt = BatchNorm backward (runet_bn_bwd_apply's formula) of g = dz * w * mask * (y > 0), g recomputed; sums = (dgamma | dbeta) of the reduce
__global__ __launch_bounds__(TPB) void psp_head_bwd_apply_kernel(const float* __restrict__ dz, const float* __restrict__ t, int ldt,
                                                                 const float* __restrict__ mask, const float* __restrict__ w, float* __restrict__ dt,
                                                                 int lddt, long P, long HW, int C, long ppc, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, const float* __restrict__ sums, float inv_m) {
    const int cv = C >> 2, rows = TPB / cv, tid = threadIdx.x;
    const int col = tid % cv, row = tid / cv;
    if (row >= rows) return;
    const long p0 = (long)blockIdx.x * ppc;
    const long p1 = p0 + ppc < P ? p0 + ppc : P;
    float sc[4], sh[4], wv[4], ca[4], cb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = col * 4 + e;
        sc[e] = scale[c]; sh[e] = shift[c]; wv[e] = w[c];
        bn_bwd_coef(sc[e], mean[c], invstd[c], sums[c], sums[C + c], inv_m, ca[e], cb[e]);
    }
    for (long p = p0 + row; p < p1; p += rows) {
        const float d = dz[p];
        const f32x4 v = ld4(t + p * ldt + 4 * col);
        const f32x4 mk = mask ? ld4(mask + (p / HW) * C + 4 * col) : f32x4{1.f, 1.f, 1.f, 1.f};
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float g = bn_pre(v[e], sc[e], sh[e]) > 0.f ? d * mk[e] * wv[e] : 0.f;
            r[e] = bn_bwd_dx(g, sc[e], v[e], ca[e], cb[e]);
        }
        st4(dt + p * lddt + 4 * col, r);
    }
}
}  // namespace

#define PSP_REQ_SHAPE(n_img, h, w_, c) \
    RUNET_REQUIRE((n_img) > 0 && (h) > 0 && (w_) > 0 && (c) > 0, "empty shape")
#define PSP_REQ_C(c) RUNET_REQUIRE((c) % 4 == 0 && (c) <= 1024, "channels must be a multiple of 4, at most 1024")
#define PSP_REQ_VEC(p) RUNET_REQUIRE(RUNET_ALIGNED16(p), "per-channel vectors must be 16-byte aligned")

extern "C" int runet_psp_taps_fwd(const float* z, int ldz, float* t, int ldt, int n_img, int h, int w_, int cout, void* stream) {
    RUNET_REQUIRE(z && t, "null pointer");
    PSP_REQ_SHAPE(n_img, h, w_, cout);
    RUNET_REQUIRE(cout % 4 == 0, "channels must be a multiple of 4");
    RUNET_REQUIRE(h <= 65535 && n_img <= 65535 && (long)n_img * 50 < (1L << 31), "shape too large");
    RUNET_REQ_LD(ldz, 9 * cout, z);
    RUNET_REQ_LD(ldt, cout, t);
    hipLaunchKernelGGL(psp_taps_fwd_kernel, dim3(cdiv(cout, TAP_CHUNK), h, n_img), dim3(TPB), 0, (hipStream_t)stream, z, ldz, t, ldt, (long)n_img, h, w_,
                       cout);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_psp_taps_bwd_workspace_floats(int n_img, int h, int w_, int cout) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || cout <= 0 || cout % 4) return -1;
    return (long)n_img * h * (CELLS * 3) * cout;
}

extern "C" int runet_psp_taps_bwd(const float* dt, int lddt, float* dz, int lddz, float* workspace, long workspace_floats, int n_img, int h, int w_,
                                  int cout, void* stream) {
    RUNET_REQUIRE(dt && dz && workspace, "null pointer");
    PSP_REQ_SHAPE(n_img, h, w_, cout);
    RUNET_REQUIRE(cout % 4 == 0, "channels must be a multiple of 4");
    RUNET_REQUIRE((long)n_img * 50 < (1L << 31), "shape too large");
    RUNET_REQ_LD(lddt, cout, dt);
    RUNET_REQ_LD(lddz, 9 * cout, dz);
    RUNET_REQUIRE(RUNET_ALIGNED16(workspace), "the workspace must be 16-byte aligned");
    RUNET_REQUIRE(workspace_floats >= runet_psp_taps_bwd_workspace_floats(n_img, h, w_, cout), "workspace too small (runet_psp_taps_bwd_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(psp_taps_bwd_cols_kernel, dim3(ew_grid((long)n_img * h * (CELLS * 3) * (cout / 4), 8192)), dim3(TPB), 0, st, dt, lddt, workspace,
                       (long)n_img, h, w_, cout);
    hipLaunchKernelGGL(psp_taps_bwd_rows_kernel, dim3(ew_grid((long)n_img * 50 * 9 * (cout / 4), 8192)), dim3(TPB), 0, st, workspace, dz, lddz,
                       (long)n_img, h, cout);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_psp_taps_dp_workspace_floats(int n_img, int cq) {
    if (n_img <= 0 || cq <= 0 || cq % 4 || cq > 256) return -1;
    return 9L * 50 * n_img * cq;
}

extern "C" int runet_psp_taps_dp(const float* dz, int lddz, const float* wp, int ldw, float* workspace, long workspace_floats, float* da, int lda,
                                 int n_img, int cq, int cout, void* stream) {
    RUNET_REQUIRE(dz && wp && workspace && da, "null pointer");
    RUNET_REQUIRE(n_img > 0 && cq > 0 && cout > 0, "empty shape");
    RUNET_REQUIRE(cq % 4 == 0 && cq <= 256 && cout % 4 == 0, "channels must be a multiple of 4 (cq at most 256)");
    RUNET_REQUIRE((long)n_img * 50 < (1L << 31), "shape too large");
    RUNET_REQ_LD(lddz, 9 * cout, dz);
    RUNET_REQ_LD(ldw, 9 * cout, wp);
    RUNET_REQ_LD(lda, cq, da);
    RUNET_REQUIRE(RUNET_ALIGNED16(workspace), "the workspace must be 16-byte aligned");
    RUNET_REQUIRE(workspace_floats >= runet_psp_taps_dp_workspace_floats(n_img, cq), "workspace too small (runet_psp_taps_dp_workspace_floats)");
    long tiles = 0;
    for (int b : {1, 2, 3, 6}) tiles += ((long)n_img * b * b + DP_ROWS - 1) / DP_ROWS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(psp_taps_dp_partial_kernel, dim3((unsigned)tiles, 9, cdiv(cq, DP_K)), dim3(TPB), 0, st, dz, lddz, wp, ldw, workspace, (long)n_img, cq,
                       cout);
    hipLaunchKernelGGL(psp_taps_dp_sum_kernel, dim3(ew_grid((long)n_img * 50 * (cq / 4), 8192)), dim3(TPB), 0, st, workspace, da, lda, (long)n_img, cq);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_psp_head_fwd(const float* t, int ldt, const float* scale, const float* shift, const float* mask_nc, const float* w, const float* b,
                                  float* z, int n_img, int h, int w_, int c, void* stream) {
    RUNET_REQUIRE(t && scale && shift && w && b && z, "null pointer");
    PSP_REQ_SHAPE(n_img, h, w_, c);
    PSP_REQ_C(c);
    RUNET_REQ_LD(ldt, c, t);
    PSP_REQ_VEC(scale); PSP_REQ_VEC(shift); PSP_REQ_VEC(w); PSP_REQ_VEC(mask_nc);
    int L = 1;
    while (L < c / 4 && L < 64) L <<= 1;
    const long P = (long)n_img * h * w_;
    long blocks = (P + TPB / L - 1) / (TPB / L);
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(psp_head_fwd_kernel, dim3((int)blocks), dim3(TPB), 0, (hipStream_t)stream, t, ldt, scale, shift, mask_nc, w, b, z, P,
                       (long)h * w_, c, L);
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_psp_head_bwd_workspace_floats(int n_img, int h, int w_, int c) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || c < 4 || c > 1024 || c % 4) return -1;
    long ppc;
    return (long)pixel_chunks((long)n_img * h * w_, c, 16384, MAX_PARTS, ppc) * (3 * c + 1);
}

extern "C" int runet_psp_head_bwd_reduce(const float* dz, const float* t, int ldt, const float* scale, const float* shift, const float* mask_nc,
                                         const float* w, const float* mean, const float* invstd, float* workspace, long workspace_floats, float* out,
                                         int n_img, int h, int w_, int c, void* stream) {
    RUNET_REQUIRE(dz && t && scale && shift && w && mean && invstd && workspace && out, "null pointer");
    PSP_REQ_SHAPE(n_img, h, w_, c);
    PSP_REQ_C(c);
    RUNET_REQ_LD(ldt, c, t);
    PSP_REQ_VEC(scale); PSP_REQ_VEC(shift); PSP_REQ_VEC(w); PSP_REQ_VEC(mean); PSP_REQ_VEC(invstd); PSP_REQ_VEC(mask_nc);
    const int width = 3 * c + 1, rows = TPB / (c / 4);
    const long P = (long)n_img * h * w_;
    long ppc;
    const int chunks = pixel_chunks(P, c, 16384, MAX_PARTS, ppc);
    RUNET_REQUIRE(workspace_floats >= (long)chunks * width, "workspace too small (runet_psp_head_bwd_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(psp_head_bwd_reduce_partial, dim3(chunks), dim3(TPB), (size_t)rows * width * sizeof(float), st, dz, t, ldt, scale, shift, mask_nc,
                       w, mean, invstd, P, (long)h * w_, c, ppc, workspace);
    sum_parts<16>(workspace, chunks, width, out, st);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_psp_head_bwd_apply(const float* dz, const float* t, int ldt, const float* mask_nc, const float* w, float* dt, int lddt, int n_img,
                                        int h, int w_, int c, const float* mean, const float* invstd, const float* scale, const float* shift,
                                        const float* sums, long m_total, void* stream) {
    RUNET_REQUIRE(dz && t && w && dt && mean && invstd && scale && shift && sums, "null pointer");
    PSP_REQ_SHAPE(n_img, h, w_, c);
    PSP_REQ_C(c);
    RUNET_REQ_LD(ldt, c, t);
    RUNET_REQ_LD(lddt, c, dt);
    PSP_REQ_VEC(mask_nc);
    const long P = (long)n_img * h * w_;
    const float inv_m = 1.0f / (float)(m_total > 0 ? m_total : P);
    long ppc;
    const int chunks = pixel_chunks(P, c, 8192, 8192, ppc);
    hipLaunchKernelGGL(psp_head_bwd_apply_kernel, dim3(chunks), dim3(TPB), 0, (hipStream_t)stream, dz, t, ldt, mask_nc, w, dt, lddt, P, (long)h * w_, c, ppc,
                       mean, invstd, scale, shift, sums, inv_m);
    RUNET_CHECK_LAUNCH();
}
