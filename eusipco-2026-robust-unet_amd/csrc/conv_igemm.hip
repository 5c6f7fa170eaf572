// Implicit-GEMM convolutions on the fp32 matrix cores of gfx950 (v_mfma_f32_32x32x2_f32).
//
// Replaces the ATen/oneDNN kernels behind every nn.Conv2d / nn.ConvTranspose2d of the reference's
// RobustUNet (/root/reference/Main_Final.py:157,159,172,126,131,205-208,261-270) for forward, data
// gradient and weight gradient, and of the baseline models (strided, dilated, rectangular and large
// kernels, k3 / k4 transposed convolutions, batched GEMMs).  One kernel template serves them all; the
// geometry struct says how a GEMM row (a pixel of the iteration space) maps to source and destination
// pixels.  File layout: the kernels; then the host side - builders that fill the geometry structs, the
// route (tile variant, weight layout, loader) computed from a filled struct, the split-K launcher - and
// last the extern "C" entry points: their own argument checks, then builder -> route -> launch.
//
// Data layout in HBM: activations NHWC fp32 (pixel stride `ld` floats, so a tensor may be a channel
// slice of a wider concat buffer); weights "HWIO": w[tap][cin][cout], cout contiguous.
//
// fwd/dgrad kernel:  out[p][n] = sum_tap sum_k  src[pix(p,tap)][k] * B_tap[k][n]
//   GEMM M = pixels (tile BM), N = output channels (tile BN), K = taps x channels (step 16 channels).
//   A tile (BM x 16) and B tile (16 x BN) are register-staged into double-buffered LDS
//   (global_load_dwordx4 issued one k-step ahead, ds_write after the MFMAs of the current step),
//   one barrier per k-step.  A rows are padded to 20 floats so the ds_read_b128 fragment reads are
//   bank-conflict free; lane (i, h) of a wave reads 4 consecutive k for row i and feeds them to 4
//   MFMAs (the k order inside a group of 8 is permuted identically for A and B).
// wgrad kernel:      dW[tap][ci][co] = sum_p  x[pix(p,tap)][ci] * dy[p][co]
//   GEMM M = cin, N = cout, K = pixels (step 16 pixels); split over pixel ranges (grid.z) into
//   partial slabs that a second kernel sums in a fixed order (bitwise reproducible, no atomics).
#include "runet_common.h"
#include "../../include/runet_hip.h"
#include <algorithm>

namespace {

struct IGemmArgs {
    const float* x; int ldx;      // A source, [Nimg, Hin, Win, ldx]
    const float* w; long w_tap_stride; int w_sk, w_sn;   // B(tap,k,n) = w[tap*w_tap_stride + k*w_sk + n*w_sn]
    const float* bias;            // [Ncols] or nullptr
    float* y; int ldy;            // destination [Nimg, Hout, Wout, ldy]
    int K, Kx, Kvalid, Ncols;     // K: k-loop extent (multiple of 16); x holds Kx channels; rows >= Kvalid of B are zero
    int Nimg, H, W;               // iteration space
    int Hin, Win, a_scale;        // source pixel = (h*a_scale + bh + r*tdh, w*a_scale + bw + s*tdw)
    int KH, KW, tdh, tdw, bh, bw;
    int Hout, Wout, o_scale, o_dh, o_dw;   // destination pixel = (h*o_scale + o_dh, w*o_scale + o_dw)
    int z_taps;                   // >0: blockIdx.z selects one weight tap AND the destination offset (convT k2 fwd)
    int accumulate;               // y += result
    int a_div;                    // >1: source coordinate must be divisible by a_div and is divided by it (data gradient of a strided conv)
    int zmode4;                   // 1: ConvTranspose2d(k4,s2,p1) forward: blockIdx.z = output parity class (ph,pw); taps (a,b) in 2x2 read
                                  //    weight tap (1-ph+2a, 1-pw+2b) of the 4x4 filter at source offset (ph-a, pw-b)
    long zs_x, zs_w, zs_y;        // zbatch: blockIdx.z selects one GEMM of a batch (element strides of x, w and y)
    int zbatch;
};

// SIMPLE: every tap of every row lies inside the source image (plain 1x1 convolutions, the k2-s2 transposed convolution both ways), K a
// multiple of 16 and fully backed by x and w: every address is a per-thread pointer set up once plus a wave-uniform offset per k-step,
// nothing is predicated (rows / columns beyond the problem are clamped
// to valid addresses: their products land in output rows / columns that are never stored).  The general loader recomputes tap geometry,
// bounds and 64-bit addresses every k-step: ~220 VALU instructions (20 of them quarter-rate integer multiplies) per 32 MFMAs, and fp32
// MFMAs share SIMD cycles with VALU work (conv_winograd.hip) - the 1x1 forward / data-gradient launches ran at 52-69 TFLOP/s with it.
// Stats = float* (runet_convt4_igemm_stats, the k4 transposed forward of YOLOSeg's decoder): after the stores, the BatchNorm statistics
// partials of the stored tile, stats[blockIdx.z * gridDim.x + blockIdx.x][Ncols][3] = (count, mean, M2) per column over the tile's rows.
// The main loop and the stores are the same code either way, so y has the same bits.  Without it (the empty pack) the argument list, the
// code and the demangled name are the kernel's as they were.
template <int BM, int BN, int WM, int WN, bool KCONTIG, bool SIMPLE = false, typename... Stats>
__global__ __launch_bounds__(256, 2) void igemm_kernel(IGemmArgs g, Stats... stats_arg) {
    constexpr int LDA = 20;
    constexpr int LDB = BN + 4;
    constexpr int A_ELEMS = BM * LDA;
    constexpr int B_ELEMS = 16 * LDB;
    constexpr int STAGE = A_ELEMS + B_ELEMS;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int WAVES_N = BN / WN;
    static_assert((BM / WM) * WAVES_N == 4, "4 waves per block");
    constexpr int AROWS = BM / 64;
    constexpr int BREGS = (BN >= 64) ? BN / 64 : 1;

    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm0 = (wid / WAVES_N) * WM, wn0 = (wid % WAVES_N) * WN;
    const int li = lane & 31, lh = lane >> 5;

    const long P = (long)g.Nimg * g.H * g.W;
    const long m0 = (long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int HW = g.H * g.W;

    const float* wbase = g.w;
    const float* xb = g.x;
    float* yb = g.y;
    if (g.zbatch) { xb += (long)blockIdx.z * g.zs_x; wbase += (long)blockIdx.z * g.zs_w; yb += (long)blockIdx.z * g.zs_y; }
    int o_dh = g.o_dh, o_dw = g.o_dw;
    const int ph4 = (blockIdx.z >> 1) & 1, pw4 = blockIdx.z & 1;
    if (g.zmode4) { o_dh = ph4; o_dw = pw4; }
    if (g.z_taps > 0) {
        wbase += (long)blockIdx.z * g.w_tap_stride;
        o_dh = blockIdx.z / g.z_taps;   // z_taps = taps per row (2 for the 2x2 transposed conv)
        o_dw = blockIdx.z % g.z_taps;
    }

    // ---- per-thread A staging rows ----
    const int akq = tid & 3;
    long a_img[AROWS];
    int a_h[AROWS], a_w[AROWS];
    bool a_ok[AROWS];
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
        const long p = m0 + (tid >> 2) + 64 * i;
        a_ok[i] = p < P;
        const long pp = a_ok[i] ? p : 0;
        const int n = (int)(pp / HW);
        const int rem = (int)(pp - (long)n * HW);
        const int h = rem / g.W;
        a_img[i] = (long)n * g.Hin * g.Win;
        a_h[i] = h * g.a_scale + g.bh;
        a_w[i] = (rem - h * g.W) * g.a_scale + g.bw;
    }

    const int KC = g.K >> 4;
    const int ntaps = (g.z_taps > 0) ? 1 : g.KH * g.KW;
    const int nks = ntaps * KC;

    f32x4 ra[AROWS];
    f32x4 rb[BREGS];
    int ld_tr = 0, ld_ts = 0, ld_kc = 0, ld_tap = 0;   // counters of the NEXT tile to load

    // SIMPLE: running pointers of this thread's A rows and B float4s
    const float* ap[AROWS];
    const float* bp[BREGS];
    long bstep = 0;
    if constexpr (SIMPLE) {
#pragma unroll
        for (int i = 0; i < AROWS; ++i)                  // a_ok false: pixel 0 (a_img = a_h = a_w = 0 from pp = 0 above)
            ap[i] = xb + (a_img[i] + (long)a_h[i] * g.Win + a_w[i]) * g.ldx + akq * 4;
        if constexpr (!KCONTIG) {
            constexpr int NQ = BN / 4;
            constexpr int KSTEP = 256 / NQ;
#pragma unroll
            for (int i = 0; i < BREGS; ++i) {
                const int nq = tid % NQ;
                int kr = tid / NQ + KSTEP * i, n = n0 + nq * 4;
                kr = kr < 16 ? kr : 15;
                n = n < g.Ncols ? n : g.Ncols - 4;
                bp[i] = wbase + (long)kr * g.w_sk + n;
            }
            bstep = 16L * g.w_sk;
        } else {
#pragma unroll
            for (int i = 0; i < BREGS; ++i) {
                int n = n0 + (tid >> 2) + 64 * i;
                n = n < g.Ncols ? n : g.Ncols - 1;
                bp[i] = wbase + (long)n * g.w_sn + akq * 4;
            }
            bstep = 16;
        }
    }

    auto load_tile = [&]() {
        if constexpr (SIMPLE) {
            // wave-uniform offsets of the tile (tap shift of the source pixel, channel chunk, weight tap): scalar arithmetic only
            const long offa = ((long)(ld_tr * g.tdh) * g.Win + ld_ts * g.tdw) * g.ldx + ld_kc * 16;
            const long offb = (long)ld_tap * g.w_tap_stride + (long)ld_kc * bstep;
#pragma unroll
            for (int i = 0; i < AROWS; ++i) ra[i] = *reinterpret_cast<const f32x4*>(ap[i] + offa);
#pragma unroll
            for (int i = 0; i < BREGS; ++i) rb[i] = *reinterpret_cast<const f32x4*>(bp[i] + offb);
            ++ld_tap;
            if (++ld_ts == g.KW) {
                ld_ts = 0;
                if (++ld_tr == g.KH) { ld_tr = 0; ld_tap = 0; ++ld_kc; }
            }
            return;
        }
        int dh = ld_tr * g.tdh, dw = ld_ts * g.tdw;
        int wtap = ld_tap;
        if (g.zmode4) { dh = ph4 - ld_tr; dw = pw4 - ld_ts; wtap = (1 - ph4 + 2 * ld_tr) * 4 + (1 - pw4 + 2 * ld_ts); }
        const int kofs = ld_kc * 16;
#pragma unroll
        for (int i = 0; i < AROWS; ++i) {
            int ih = a_h[i] + dh, iw = a_w[i] + dw;
            bool ok = a_ok[i] && kofs + akq * 4 < g.Kx;
            if (g.a_div > 1) {
                ok = ok && ih >= 0 && iw >= 0 && (ih % g.a_div) == 0 && (iw % g.a_div) == 0;
                ih /= g.a_div; iw /= g.a_div;
            }
            ok = ok && (unsigned)ih < (unsigned)g.Hin && (unsigned)iw < (unsigned)g.Win;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *reinterpret_cast<const f32x4*>(xb + ((a_img[i] + (long)ih * g.Win + iw) * g.ldx + kofs + akq * 4));
            ra[i] = v;
        }
        const float* wt = wbase + (long)wtap * g.w_tap_stride;
        if constexpr (!KCONTIG) {   // n contiguous: 16 k-rows x BN/4 float4
            constexpr int NQ = BN / 4;
            constexpr int KSTEP = 256 / NQ;
#pragma unroll
            for (int i = 0; i < BREGS; ++i) {
                const int nq = tid % NQ, kr = tid / NQ + KSTEP * i;
                const int k = kofs + kr, n = n0 + nq * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (kr < 16 && k < g.Kvalid && n < g.Ncols) v = *reinterpret_cast<const f32x4*>(wt + (long)k * g.w_sk + n);
                rb[i] = v;
            }
        } else {   // k contiguous: BN n-rows x 4 float4
#pragma unroll
            for (int i = 0; i < BREGS; ++i) {
                const int nr = (tid >> 2) + 64 * i;
                const int n = n0 + nr, k = kofs + akq * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (nr < BN && n < g.Ncols && k < g.Kvalid) v = *reinterpret_cast<const f32x4*>(wt + (long)n * g.w_sn + k);
                rb[i] = v;
            }
        }
        // advance counters: tap fastest (column, then row), then the channel chunk - the 9 shifted reads of one 16-channel
        // chunk touch the same cache lines back to back, so 8 of them are served by L1/L2 instead of the fabric
        ++ld_tap;
        if (++ld_ts == g.KW) {
            ld_ts = 0;
            if (++ld_tr == g.KH) { ld_tr = 0; ld_tap = 0; ++ld_kc; }
        }
    };

    auto store_tile = [&](int buf) {
        float* As = smem + buf * STAGE;
        float* Bs = As + A_ELEMS;
#pragma unroll
        for (int i = 0; i < AROWS; ++i)
            *reinterpret_cast<f32x4*>(As + ((tid >> 2) + 64 * i) * LDA + akq * 4) = ra[i];
        if constexpr (!KCONTIG) {
            constexpr int NQ = BN / 4;
            constexpr int KSTEP = 256 / NQ;
#pragma unroll
            for (int i = 0; i < BREGS; ++i) {
                const int nq = tid % NQ, kr = tid / NQ + KSTEP * i;
                if (kr < 16) *reinterpret_cast<f32x4*>(Bs + kr * LDB + nq * 4) = rb[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < BREGS; ++i) {
                const int nr = (tid >> 2) + 64 * i;
                if (nr < BN) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) Bs[(akq * 4 + e) * LDB + nr] = rb[i][e];
                }
            }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    load_tile();
    store_tile(0);
    __syncthreads();

    int cur = 0;
    for (int ks = 0; ks < nks; ++ks) {
        const bool more = ks + 1 < nks;
        if (more) load_tile();
        const float* As = smem + cur * STAGE;
        const float* Bs = As + A_ELEMS;
        // all fragments of the k-step are read up front (2*TM ds_read_b128 + 4*TN ds_read2_b32), then the MFMA chain runs
        // without LDS waits inside it; the scheduler is told to keep that order (it otherwise sinks each B read to its use)
        f32x4 af[2][TM];
        float bf[2][TN][4];
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
#pragma unroll
            for (int a = 0; a < TM; ++a)
                af[kh][a] = *reinterpret_cast<const f32x4*>(As + (wm0 + a * 32 + li) * LDA + kh * 8 + 4 * lh);
#pragma unroll
            for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int q = 0; q < 4; ++q) bf[kh][b][q] = Bs[(kh * 8 + 4 * lh + q) * LDB + wn0 + b * 32 + li];
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * TM + 4 * TN, 0);     // DS reads first
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kh][a][q], bf[kh][b][q], acc[a][b], 0, 0, 0);
        __builtin_amdgcn_sched_group_barrier(0x8, 8 * TM * TN, 0);            // then the whole MFMA chain
        if (more) store_tile(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // ---- epilogue: D[row = pixel][col = n]; lane holds col (lane&31), rows (r&3)+8*(r>>2)+4*(lane>>5) ----
    const bool same_pix = (g.o_scale == 1 && g.Hout == g.H && g.Wout == g.W);   // plain conv: destination pixel == GEMM row
    int ncol[TN];
    float bv[TN];
#pragma unroll
    for (int b = 0; b < TN; ++b) {
        ncol[b] = n0 + wn0 + b * 32 + li;
        bv[b] = (g.bias != nullptr && ncol[b] < g.Ncols) ? g.bias[ncol[b]] : 0.f;
    }
#pragma unroll
    for (int a = 0; a < TM; ++a) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            // accumulate mode: the old values of 8 rows are all requested before the first add, so the loads overlap
            // instead of one load -> wait -> store per element (8 at a time keeps the register count where it was)
            float* drow[8];
            float old[8][TN];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = half * 8 + i;
                const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
                const long p = m0 + wm0 + a * 32 + row;
                long op = p < P ? p : 0;
                if (!same_pix) {
                    const int nimg = (int)(op / HW);
                    const int rem = (int)(op - (long)nimg * HW);
                    const int h = rem / g.W, w = rem - h * g.W;
                    op = ((long)nimg * g.Hout + (h * g.o_scale + o_dh)) * g.Wout + (w * g.o_scale + o_dw);
                }
                drow[i] = p < P ? yb + op * g.ldy : nullptr;
#pragma unroll
                for (int b = 0; b < TN; ++b) old[i][b] = (g.accumulate && drow[i] && ncol[b] < g.Ncols) ? drow[i][ncol[b]] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (drow[i]) {
#pragma unroll
                    for (int b = 0; b < TN; ++b)
                        if (ncol[b] < g.Ncols) drow[i][ncol[b]] = acc[a][b][half * 8 + i] + bv[b] + old[i][b];
                }
            }
        }
    }
    if constexpr (sizeof...(Stats) > 0) {
        float* const stats = (stats_arg, ...);
        // as conv_x3_kernel's statistics epilogue: a lane holds TM * 16 rows of each of its columns -> two-pass (mean, M2) in registers,
        // Chan-combined with the other lane half (xor 32), then through LDS over the BM / WM waves of the column in wave order.  Fixed
        // order: bitwise reproducible.  (accumulate is 0 here: the stored value is acc + bias.)
        constexpr int WAVES_M = BM / WM;
        float* xch = smem;                                            // [WAVES_M][BN][3]: the stages are dead by now
        lds_barrier();
#pragma unroll
        for (int b = 0; b < TN; ++b) {
            float cnt = 0.f, s1 = 0.f;
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = m0 + wm0 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh < P;
                    cnt += ok ? 1.f : 0.f;
                    s1 += ok ? acc[a][b][r] + bv[b] : 0.f;
                }
            float mean = cnt > 0.f ? s1 / cnt : 0.f, m2 = 0.f;
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = m0 + wm0 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh < P;
                    const float d = acc[a][b][r] + bv[b] - mean;
                    m2 += ok ? d * d : 0.f;
                }
            const float cnt_o = __shfl_xor(cnt, 32, 64), mean_o = __shfl_xor(mean, 32, 64), m2_o = __shfl_xor(m2, 32, 64);
            {
                const float nt = cnt + cnt_o, dlt = mean_o - mean;
                if (nt > 0.f) { m2 = m2 + m2_o + dlt * dlt * (cnt * cnt_o / nt); mean = mean + dlt * (cnt_o / nt); }
                cnt = nt;
            }
            if (lh == 0) {
                float* o = xch + ((wid / WAVES_N) * BN + wn0 + b * 32 + li) * 3;
                o[0] = cnt; o[1] = mean; o[2] = m2;
            }
        }
        lds_barrier();
        for (int cl = tid; cl < BN; cl += 256) {
            const int col = n0 + cl;
            if (col < g.Ncols) {
                float cnt = xch[cl * 3], mean = xch[cl * 3 + 1], m2 = xch[cl * 3 + 2];
#pragma unroll
                for (int wv = 1; wv < WAVES_M; ++wv) {
                    const float* e = xch + (wv * BN + cl) * 3;
                    const float nt = cnt + e[0], dlt = e[1] - mean;
                    if (nt > 0.f) { m2 = m2 + e[2] + dlt * dlt * (cnt * e[0] / nt); mean = mean + dlt * (e[0] / nt); }
                    cnt = nt;
                }
                float* o = stats + (((long)blockIdx.z * gridDim.x + blockIdx.x) * g.Ncols + col) * 3;
                o[0] = cnt; o[1] = mean; o[2] = m2;
            }
        }
    }
}


// ------------------------------------------------------------------------------------------ wgrad
struct WGradArgs {
    const float* x; int ldx;     // [Nimg, Hin, Win, ldx], channels [0, Kci)
    const float* dy; int ldy;    // [Nimg, Hout, Wout, ldy], channels [0, Nco)
    float* out;                  // slabs: [split][ntaps][Kvalid][Nco]
    int Kci, Kvalid, Nco;        // Kci multiple of 16 (padded read width of x); only ci < Kvalid are written
    int Nimg, H, W;              // iteration space (pixels summed over)
    int Hin, Win, a_scale, KH, KW, tdh, tdw, bh, bw;   // x pixel = (h*a_scale + bh + r*tdh, ...)
    int Hout, Wout, o_scale;     // dy pixel = (h*o_scale + o_dh, w*o_scale + o_dw)
    int tap_on_output;           // 1: tap (r,s) offsets the dy pixel (transposed conv), x pixel unshifted
    int o_bh, o_bw;              // base offset of the dy pixel when tap_on_output (k4-s2-p1 transposed conv: -1)
    long pix_per_split;          // multiple of 16
    long tap_bs_x, tap_bs_dy;    // batched form: tap t reads x + t*tap_bs_x and dy + t*tap_bs_dy (no spatial shift)
};

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(WGradArgs g) {
    constexpr int LDA = BM + 4, LDB = BN + 4;
    constexpr int A_ELEMS = 16 * LDA, B_ELEMS = 16 * LDB, STAGE = A_ELEMS + B_ELEMS;
    constexpr int TM = WM / 32, TN = WN / 32, WAVES_N = BN / WN;
    static_assert((BM / WM) * WAVES_N == 4, "4 waves per block");
    constexpr int AQ = BM / 4, BQ = BN / 4;              // float4 per pixel row
    constexpr int AREGS = (16 * AQ + 255) / 256, BREGS = (16 * BQ + 255) / 256;
    constexpr int APSTEP = 256 / AQ, BPSTEP = 256 / BQ;  // pixel rows covered per pass (AQ,BQ <= 64... see launch)

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm0 = (wid / WAVES_N) * WM, wn0 = (wid % WAVES_N) * WN;
    const int li = lane & 31, lh = lane >> 5;

    const int n_tiles = (g.Nco + BN - 1) / BN;
    const int ci0 = (blockIdx.x / n_tiles) * BM, co0 = (blockIdx.x % n_tiles) * BN;
    const int tap = blockIdx.y, tr = tap / g.KW, ts = tap % g.KW;
    const long P = (long)g.Nimg * g.H * g.W;
    const long p_begin = (long)blockIdx.z * g.pix_per_split;
    long p_end = p_begin + g.pix_per_split;
    if (p_end > P) p_end = P;
    const int HW = g.H * g.W;

    int xdh = g.bh, xdw = g.bw, ydh = 0, ydw = 0;
    if (g.tap_on_output) { ydh = tr + g.o_bh; ydw = ts + g.o_bw; } else { xdh += tr * g.tdh; xdw += ts * g.tdw; }

    const float* xb = g.x + (long)tap * g.tap_bs_x;
    const float* dyb = g.dy + (long)tap * g.tap_bs_dy;
    f32x4 ra[AREGS], rb[BREGS];
    auto load_tile = [&](long pk) {   // pk: first pixel of the 16-pixel k-step
#pragma unroll
        for (int i = 0; i < AREGS; ++i) {
            const int cq = tid % AQ, pr = tid / AQ + APSTEP * i;
            const long p = pk + pr;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (pr < 16 && p < p_end && ci0 + cq * 4 < g.Kci) {
                const int n = (int)(p / HW);
                const int rem = (int)(p - (long)n * HW);
                const int h = rem / g.W, w = rem - h * g.W;
                const int ih = h * g.a_scale + xdh, iw = w * g.a_scale + xdw;
                if ((unsigned)ih < (unsigned)g.Hin && (unsigned)iw < (unsigned)g.Win)
                    v = *reinterpret_cast<const f32x4*>(xb + (((long)n * g.Hin + ih) * g.Win + iw) * g.ldx + ci0 + cq * 4);
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < BREGS; ++i) {
            const int cq = tid % BQ, pr = tid / BQ + BPSTEP * i;
            const long p = pk + pr;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (pr < 16 && p < p_end && co0 + cq * 4 < g.Nco) {
                const int n = (int)(p / HW);
                const int rem = (int)(p - (long)n * HW);
                const int h = rem / g.W, w = rem - h * g.W;
                const int oh = h * g.o_scale + ydh, ow = w * g.o_scale + ydw;
                if ((unsigned)oh < (unsigned)g.Hout && (unsigned)ow < (unsigned)g.Wout)
                    v = *reinterpret_cast<const f32x4*>(dyb + (((long)n * g.Hout + oh) * g.Wout + ow) * g.ldy + co0 + cq * 4);
            }
            rb[i] = v;
        }
    };
    auto store_tile = [&](int buf) {
        float* As = smem + buf * STAGE;
        float* Bs = As + A_ELEMS;
#pragma unroll
        for (int i = 0; i < AREGS; ++i) {
            const int cq = tid % AQ, pr = tid / AQ + APSTEP * i;
            if (pr < 16) *reinterpret_cast<f32x4*>(As + pr * LDA + cq * 4) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < BREGS; ++i) {
            const int cq = tid % BQ, pr = tid / BQ + BPSTEP * i;
            if (pr < 16) *reinterpret_cast<f32x4*>(Bs + pr * LDB + cq * 4) = rb[i];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    const int nks = (int)((p_end - p_begin + 15) / 16);
    if (nks > 0) {
        load_tile(p_begin);
        store_tile(0);
    }
    __syncthreads();
    int cur = 0;
    for (int ks = 0; ks < nks; ++ks) {
        const bool more = ks + 1 < nks;
        if (more) load_tile(p_begin + (long)(ks + 1) * 16);
        const float* As = smem + cur * STAGE;
        const float* Bs = As + A_ELEMS;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            float af[TM], bf[TN];
#pragma unroll
            for (int a = 0; a < TM; ++a) af[a] = As[(2 * s + lh) * LDA + wm0 + a * 32 + li];
#pragma unroll
            for (int b = 0; b < TN; ++b) bf[b] = Bs[(2 * s + lh) * LDB + wn0 + b * 32 + li];
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a], bf[b], acc[a][b], 0, 0, 0);
        }
        if (more) store_tile(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    const int ntaps = g.KH * g.KW;
    float* slab = g.out + ((long)blockIdx.z * ntaps + tap) * g.Kvalid * g.Nco;
#pragma unroll
    for (int b = 0; b < TN; ++b) {
        const int co = co0 + wn0 + b * 32 + li;
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ci = ci0 + wm0 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (co < g.Nco && ci < g.Kvalid) slab[(long)ci * g.Nco + co] = acc[a][b][r];
            }
    }
}


// ------------------------------------------------------------------------------------------ wgrad, tile-resident form
// For 3x3 (dilation 1) and 1x1 convolutions: a block keeps a 4x16-pixel tile of dy and the matching x tile (with its
// 1-pixel halo for 3x3) in LDS and accumulates ALL taps from it, so x and dy are read from HBM/L2 once per
// (cin-chunk, cout-chunk) pair instead of once per tap; it then walks `tiles_per_split` tiles with the accumulators in
// registers (9 taps x one 32x32 tile per wave = 144 accumulator registers for 3x3) and writes one partial slab.
// The next tile's global loads are issued before the current tile's MFMAs (register prefetch).
struct WGradTileArgs {
    const float* x; int ldx;
    const float* dy; int ldy;
    float* out;                 // slabs [split][KS*KS][Kvalid][Nco]
    int Kci, Kvalid, Nco;
    int Nimg, H, W;
    int tiles_h, tiles_w, total_tiles, tiles_per_split, co_chunks;
    int dy_up;                  // 1: transposed conv (KS == 1 only): dy pixel of x pixel (h, w) is (2h + z/2, 2w + z%2), z = blockIdx.z
};

template <int KS, int TM, int TN>
__global__ __launch_bounds__(256, 2) void wgrad_tile_kernel(WGradTileArgs g) {
    constexpr int CI = 64 * TM, CO = 64 * TN;
    constexpr int TH = 4, TW = 16, NPX = TH * TW;
    constexpr int HALO = (KS == 3) ? 1 : 0;
    constexpr int HTW = TW + 2 * HALO, HTH = TH + 2 * HALO, NHPX = HTW * HTH;
    constexpr int XQ = CI / 4, YQ = CO / 4;
    constexpr int NXV = (NHPX * XQ + 255) / 256, NYV = (NPX * YQ + 255) / 256;
    constexpr int NT = KS * KS;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;
    float* dys = smem + NHPX * CI;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, li = lane & 31, lh = lane >> 5;
    const int ci0 = (blockIdx.x / g.co_chunks) * CI, co0 = (blockIdx.x % g.co_chunks) * CO;
    const int t_begin = blockIdx.y * g.tiles_per_split;
    const int t_end = min(g.total_tiles, t_begin + g.tiles_per_split);
    const long P = (long)g.Nimg * g.H * g.W;
    const int tiles_per_img = g.tiles_h * g.tiles_w;

    f32x4 rx[NXV], ry[NYV];
    auto prefetch = [&](int t) {
        int n = 0, h0 = 0, w0 = 0;
        if constexpr (KS == 3) {
            n = t / tiles_per_img;
            const int rem = t - n * tiles_per_img;
            const int th = rem / g.tiles_w;
            h0 = th * TH; w0 = (rem - th * g.tiles_w) * TW;
        }
#pragma unroll
        for (int v = 0; v < NXV; ++v) {
            const int idx = tid + 256 * v;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (idx < NHPX * XQ) {
                const int px = idx / XQ, cq = idx % XQ;
                if (ci0 + cq * 4 < g.Kci) {
                    if constexpr (KS == 3) {
                        const int hy = px / HTW, hx = px - hy * HTW;
                        const int ih = h0 - 1 + hy, iw = w0 - 1 + hx;
                        if ((unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)
                            val = *reinterpret_cast<const f32x4*>(g.x + (((long)n * g.H + ih) * g.W + iw) * g.ldx + ci0 + cq * 4);
                    } else {
                        const long p = (long)t * NPX + px;
                        if (p < P) val = *reinterpret_cast<const f32x4*>(g.x + p * g.ldx + ci0 + cq * 4);
                    }
                }
            }
            rx[v] = val;
        }
#pragma unroll
        for (int v = 0; v < NYV; ++v) {
            const int idx = tid + 256 * v;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (idx < NPX * YQ) {
                const int px = idx / YQ, cq = idx % YQ;
                if (co0 + cq * 4 < g.Nco) {
                    if constexpr (KS == 3) {
                        const int oh = h0 + (px >> 4), ow = w0 + (px & 15);
                        if (oh < g.H && ow < g.W)
                            val = *reinterpret_cast<const f32x4*>(g.dy + (((long)n * g.H + oh) * g.W + ow) * g.ldy + co0 + cq * 4);
                    } else {
                        const long p = (long)t * NPX + px;
                        if (p < P) {
                            long q = p;
                            if (g.dy_up) {
                                const int hw = g.H * g.W;
                                const int ni = (int)(p / hw);
                                const int rem = (int)(p - (long)ni * hw);
                                const int hh = rem / g.W, ww = rem - hh * g.W;
                                q = ((long)ni * 2 * g.H + 2 * hh + (blockIdx.z >> 1)) * (2 * g.W) + 2 * ww + (blockIdx.z & 1);
                            }
                            val = *reinterpret_cast<const f32x4*>(g.dy + q * g.ldy + co0 + cq * 4);
                        }
                    }
                }
            }
            ry[v] = val;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int v = 0; v < NXV; ++v) {
            const int idx = tid + 256 * v;
            if (idx < NHPX * XQ) *reinterpret_cast<f32x4*>(xs + idx * 4) = rx[v];
        }
#pragma unroll
        for (int v = 0; v < NYV; ++v) {
            const int idx = tid + 256 * v;
            if (idx < NPX * YQ) *reinterpret_cast<f32x4*>(dys + idx * 4) = ry[v];
        }
    };

    f32x16 acc[NT][TM][TN];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][a][b][r] = 0.f;

    if (t_begin < t_end) prefetch(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        __syncthreads();
        stash();
        __syncthreads();
        if (t + 1 < t_end) prefetch(t + 1);
#pragma unroll 2
        for (int m = 0; m < NPX / 2; ++m) {
            const int p = 2 * m + lh;
            const int ty = p >> 4, tx = p & 15;
            float bf[TN];
#pragma unroll
            for (int b = 0; b < TN; ++b) bf[b] = dys[p * CO + (wc * TN + b) * 32 + li];
#pragma unroll
            for (int r = 0; r < KS; ++r)
#pragma unroll
                for (int q = 0; q < KS; ++q) {
                    float af[TM];
#pragma unroll
                    for (int a = 0; a < TM; ++a) af[a] = xs[((ty + r) * HTW + tx + q) * CI + (wr * TM + a) * 32 + li];
#pragma unroll
                    for (int a = 0; a < TM; ++a)
#pragma unroll
                        for (int b = 0; b < TN; ++b)
                            acc[r * KS + q][a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a], bf[b], acc[r * KS + q][a][b], 0, 0, 0);
                }
        }
    }

#pragma unroll
    for (int t = 0; t < NT; ++t) {
        float* slab = g.out + (((long)blockIdx.y * gridDim.z + blockIdx.z) * NT + t) * g.Kvalid * g.Nco;
#pragma unroll
        for (int b = 0; b < TN; ++b) {
            const int co = co0 + (wc * TN + b) * 32 + li;
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ci = ci0 + (wr * TM + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (co < g.Nco && ci < g.Kvalid) slab[(long)ci * g.Nco + co] = acc[t][a][b][r];
                }
        }
    }
}

struct TilePlan { int tm, tn, ci_chunks, co_chunks, total_tiles, tiles_h, tiles_w, splits, tps; };

// z_taps: taps that ride on grid.z (4 for the k2-s2 transposed convolution, whose splits shrink by as much), else 1
static TilePlan wgrad_tile_plan(int n_img, int h, int w_, int cin_w, int cout, int ks, int z_taps = 1) {
    TilePlan p{};
    if (ks == 3) { p.tm = 1; p.tn = 1; }
    else { p.tm = cin_w > 64 ? 2 : 1; p.tn = cout > 64 ? 2 : 1; }
    p.ci_chunks = cdiv(cin_w, 64 * p.tm);
    p.co_chunks = cdiv(cout, 64 * p.tn);
    if (ks == 3) { p.tiles_h = cdiv(h, 4); p.tiles_w = cdiv(w_, 16); p.total_tiles = n_img * p.tiles_h * p.tiles_w; }
    else { p.tiles_h = p.tiles_w = 0; p.total_tiles = cdiv((long)n_img * h * w_, 64); }
    const int chunks = p.ci_chunks * p.co_chunks;
    int splits = cdiv(640, chunks);                 // ~2.5 blocks per CU in total
    if (splits > p.total_tiles) splits = p.total_tiles;
    if (splits < 1) splits = 1;
    p.tps = cdiv(p.total_tiles, splits);
    p.splits = cdiv(p.total_tiles, p.tps);
    if (z_taps > 1) { p.splits = cdiv(p.splits, z_taps); p.tps = cdiv(p.total_tiles, p.splits); p.splits = cdiv(p.total_tiles, p.tps); }
    return p;
}

template <int KS, int TM, int TN>
static void launch_wgrad_tile(const WGradTileArgs& a, const TilePlan& p, hipStream_t st) {
    constexpr int HALO = (KS == 3) ? 1 : 0;
    const size_t lds = ((size_t)(16 + 2 * HALO) * (4 + 2 * HALO) * 64 * TM + 64 * 64 * TN) * sizeof(float);
    hipLaunchKernelGGL((wgrad_tile_kernel<KS, TM, TN>), dim3(p.ci_chunks * p.co_chunks, p.splits, a.dy_up ? 4 : 1), dim3(256), lds, st, a);
}


// ------------------------------------------------------------------------------------------ wgrad of the RGB stem (cin <= 4)
// dW[3][3][cin_w][cout] = sum_p x4[p + tap][0:cin_w] * dy[p][co].  A 27-deep "GEMM" wastes the matrix cores (the tile kernel pads
// cin to 64), and the op is bound by reading dy once, so this is a plain VALU kernel: a thread owns 4 output channels and every
// 16th pixel of a strip of image rows, keeps the 9 x 4 x 4 partial products in registers, the block reduces them through LDS and
// writes one partial slab; slab_reduce_kernel sums the slabs.
constexpr int STEM_ROWS = 4;     // image rows per block
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ dy, int ldy,
                                                         float* __restrict__ slabs, int H, int W, int cin_w, int cout) {
    __shared__ float red[256 * 16];                       // one tap at a time: [thread][ci 0..3][co 0..3]
    const int cq = cout / 4;                              // column threads
    const int rows = 256 / cq;                            // pixel lanes
    const int tid = threadIdx.x, col = tid % cq, pl = tid / cq;
    const int n = blockIdx.y, r0 = blockIdx.x * STEM_ROWS;
    const int npx = min(STEM_ROWS, H - r0) * W;
    float acc[9][4][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[t][c][q] = 0.f;
    if (pl < rows) {
        for (int i = pl; i < npx; i += rows) {
            const int h = r0 + i / W, w = i % W;
            const f32x4 g = *reinterpret_cast<const f32x4*>(dy + (((long)n * H + h) * W + w) * ldy + col * 4);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s2 = 0; s2 < 3; ++s2) {
                    const int ih = h + r - 1, iw = w + s2 - 1;
                    f32x4 xv = {0.f, 0.f, 0.f, 0.f};
                    if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                        xv = *reinterpret_cast<const f32x4*>(x + (((long)n * H + ih) * W + iw) * ldx);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[r * 3 + s2][c][q] += xv[c] * g[q];
                }
        }
    }
    float* slab = slabs + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 9 * cin_w * cout;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[tid * 16 + c * 4 + q] = (pl < rows) ? acc[t][c][q] : 0.f;
        __syncthreads();
        // 16*cq outputs of this tap: (ci, co) = (c, col*4+q); thread u sums over the pixel lanes
        for (int u = tid; u < 16 * cq; u += 256) {
            const int cc = u / 16, e = u % 16, c = e >> 2, q = e & 3;
            float sacc = 0.f;
            for (int p = 0; p < rows; ++p) sacc += red[(p * cq + cc) * 16 + e];
            if (c < cin_w) slab[((long)t * cin_w + c) * cout + cc * 4 + q] = sacc;
        }
    }
}

// out[i] = sum_k slabs[k][i]: block = 32 float4 columns x 8 split-lanes (fixed summation order: reproducible)
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ out, long n, int nsplit) {
    __shared__ f32x4 red[256];
    const int col = threadIdx.x & 31, kl = threadIdx.x >> 5;
    const long i = ((long)blockIdx.x * 32 + col) * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (i + 4 <= n) {
        for (int k = kl; k < nsplit; k += 8) s += *reinterpret_cast<const f32x4*>(slabs + (long)k * n + i);
    } else if (i < n) {
        for (int k = kl; k < nsplit; k += 8)
            for (int e = 0; e < 4 && i + e < n; ++e) s[e] += slabs[(long)k * n + i + e];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (kl == 0 && i < n) {
#pragma unroll
        for (int j = 1; j < 8; ++j) s += red[j * 32 + col];
        if (i + 4 <= n) *reinterpret_cast<f32x4*>(out + i) = s;
        else for (int e = 0; e < 4 && i + e < n; ++e) out[i + e] = s[e];
    }
}

// wt[tap][co][ci] = w[tap][ci][co]: 32x32 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void transpose_taps_kernel(const float* __restrict__ w, float* __restrict__ wt, int cin, int cout) {
    __shared__ float tile[32][33];
    const long base = (long)blockIdx.z * cin * cout;
    const int ci0 = blockIdx.y * 32, co0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8)
        tile[r][tx] = (ci0 + r < cin && co0 + tx < cout) ? w[base + (long)(ci0 + r) * cout + co0 + tx] : 0.f;
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (co0 + r < cout && ci0 + tx < cin) wt[base + (long)(co0 + r) * cin + ci0 + tx] = tile[tx][r];
}

// The template kernels this file instantiates: all of them and no others, in the order the device object has always carried them (the order
// of first use in the launchers as they once were).  Naming them here, ahead of every launcher, keeps the device code byte for byte the same
// however the host code below is arranged, so a host-side change can be checked by comparing the .text sections of two builds.
#define K(...) reinterpret_cast<const void*>(&__VA_ARGS__)
#define IGEMM_LOADERS(...) K(igemm_kernel<__VA_ARGS__, true>), K(igemm_kernel<__VA_ARGS__, false>)
#define IGEMM_STATS(...) K(igemm_kernel<__VA_ARGS__, false, false, float*>)
const void* const INSTANTIATIONS[] = {
    IGEMM_LOADERS(256, 64, 64, 64, false),
    IGEMM_LOADERS(128, 32, 32, 32, true), IGEMM_LOADERS(256, 64, 64, 64, true), IGEMM_LOADERS(128, 64, 64, 32, true),
    IGEMM_LOADERS(128, 128, 64, 64, true), IGEMM_LOADERS(64, 64, 32, 32, true),
    K(wgrad_tile_kernel<3, 1, 1>), K(wgrad_tile_kernel<1, 2, 2>), K(wgrad_tile_kernel<1, 2, 1>), K(wgrad_tile_kernel<1, 1, 2>), K(wgrad_tile_kernel<1, 1, 1>),
    K(wgrad_kernel<128, 128, 64, 64>), K(wgrad_kernel<64, 64, 32, 32>),
    IGEMM_STATS(128, 32, 32, 32), IGEMM_STATS(256, 64, 64, 64), IGEMM_STATS(128, 64, 64, 32), IGEMM_STATS(128, 128, 64, 64), IGEMM_STATS(64, 64, 32, 32),
    IGEMM_LOADERS(128, 64, 64, 32, false), IGEMM_LOADERS(128, 128, 64, 64, false), IGEMM_LOADERS(64, 64, 32, 32, false), IGEMM_LOADERS(128, 32, 32, 32, false)};
#undef IGEMM_STATS
#undef IGEMM_LOADERS
#undef K

// =========================================================================================================================== host side
// Each geometry, each routing condition and the split-K tail are written once:
//   operands + weight layout + geometry -> IGemmArgs -> igemm_route -> launch_route      (forward, data gradient, GEMM)
//   operands + geometry -> WGradArgs -> launch_wgrad_splitk                              (per-tap weight gradient)

// ------------------------------------------------------------------------------------------ IGemmArgs builders
// The operands: `cin` channels are read from x (K pads them to whole k-steps), rows >= cin_w of the weight are zero, `cout` columns are written.
static IGemmArgs igemm_operands(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int cin, int cin_w, int cout,
                                int accumulate) {
    IGemmArgs a{};
    a.x = x; a.ldx = ldx; a.w = w; a.bias = bias; a.y = y; a.ldy = ldy; a.Nimg = n_img; a.accumulate = accumulate; a.a_div = 1;
    a.K = (cin + 15) / 16 * 16; a.Kx = cin; a.Kvalid = cin_w; a.Ncols = cout;
    return a;
}
// The two weight layouts: [tap][k][n], n contiguous (forward weights "HWIO", and the data gradients' pre-transposed ones), and
// [tap][n][k], k contiguous (a data gradient reading the forward weight in place).  igemm_route tells them apart by w_sn.
static void weights_n_contig(IGemmArgs& a) { a.w_tap_stride = (long)a.Kvalid * a.Ncols; a.w_sk = a.Ncols; a.w_sn = 1; }
static void weights_k_contig(IGemmArgs& a) { a.w_tap_stride = (long)a.Ncols * a.Kx; a.w_sk = 1; a.w_sn = a.Kx; }

// One convolution's spatial parameters, shared by the forward, data-gradient and weight-gradient geometries: input (hin, win), output (ho, wo)
struct Conv2dGeom { int hin, win, ho, wo, kh, kw, stride, pad_h, pad_w, dil_h, dil_w; };
// 'same' padding, stride 1 (runet_conv_igemm, runet_conv_wgrad)
static Conv2dGeom same_conv(int h, int w_, int kh, int kw, int dil) { return {h, w_, h, w_, kh, kw, 1, dil * (kh / 2), dil * (kw / 2), dil, dil}; }

// The geometry builders return grid.z.
// strided / dilated / per-axis padded forward: rows = output pixels, tap (r, s) reads input (h stride - pad_h + r dil_h, ...)
static int geom_conv_fwd(IGemmArgs& a, const Conv2dGeom& c) {
    a.H = c.ho; a.W = c.wo; a.Hin = c.hin; a.Win = c.win; a.a_scale = c.stride; a.KH = c.kh; a.KW = c.kw;
    a.tdh = c.dil_h; a.tdw = c.dil_w; a.bh = -c.pad_h; a.bw = -c.pad_w; a.Hout = c.ho; a.Wout = c.wo; a.o_scale = 1;
    return 1;
}
// its data gradient: rows = input pixels, tap (r, s) reads dy at (h + pad_h - r dil_h) / stride where that divides (a_div)
static int geom_conv_dgrad(IGemmArgs& a, const Conv2dGeom& c) {
    a.H = c.hin; a.W = c.win; a.Hin = c.ho; a.Win = c.wo; a.a_scale = 1; a.KH = c.kh; a.KW = c.kw;
    a.tdh = -c.dil_h; a.tdw = -c.dil_w; a.bh = c.pad_h; a.bw = c.pad_w; a.a_div = c.stride; a.Hout = c.hin; a.Wout = c.win; a.o_scale = 1;
    return 1;
}
// s x s 1x1 GEMMs over the (h, w) low-resolution pixels; blockIdx.z = tap (r, c) picks the weight slab and the destination pixel
// (h s + r, w s + c).  s = 2: the k2-s2 transposed forward.  Any s with k-contiguous weights: the data gradient of a kernel = stride, unpadded
// convolution (SegFormer-Lite's key / value reductions), where each dx pixel has exactly one live tap - the a_div form above would run all s^2
// taps through the matrix loop for every pixel, s^2 - 1 of them dead.
static int geom_z_taps(IGemmArgs& a, int h, int w_, int s) {
    a.H = h; a.W = w_; a.Hin = h; a.Win = w_; a.a_scale = 1; a.KH = 1; a.KW = 1; a.Hout = h * s; a.Wout = w_ * s; a.o_scale = s; a.z_taps = s;
    return s * s;
}
// data gradient of a stride-2 transposed convolution with a k x k kernel and padding `pad`: dx (h, w) reads dy (2h - pad + r, 2w - pad + s).
// k = 2, pad = 0 is "up2" (every tap inside the source); k = 4, pad = 1 is the k4-s2-p1 one.
static int geom_convt_s2_dgrad(IGemmArgs& a, int h, int w_, int k, int pad) {
    a.H = h; a.W = w_; a.Hin = 2 * h; a.Win = 2 * w_; a.a_scale = 2; a.KH = k; a.KW = k; a.tdh = 1; a.tdw = 1; a.bh = -pad; a.bw = -pad;
    a.Hout = h; a.Wout = w_; a.o_scale = 1;
    return 1;
}
// ConvTranspose2d(k4, s2, p1) forward: blockIdx.z = output parity class, 2x2 live taps each (zmode4)
static int geom_convt4_fwd(IGemmArgs& a, int h, int w_) {
    a.H = h; a.W = w_; a.Hin = h; a.Win = w_; a.a_scale = 1; a.KH = 2; a.KW = 2; a.zmode4 = 1; a.Hout = 2 * h; a.Wout = 2 * w_; a.o_scale = 2;
    return 4;
}
// ConvTranspose2d(k3, s2, p1, output_padding 1) forward, parity class (ph, pw): 1, 2 or 4 live taps, tap (rr, ss) reads source (i + ph (1 - rr), j + pw (1 - ss))
static int geom_convt3_class(IGemmArgs& a, int h, int w_, int ph, int pw) {
    a.H = h; a.W = w_; a.Hin = h; a.Win = w_; a.a_scale = 1;
    a.KH = ph ? 2 : 1; a.KW = pw ? 2 : 1; a.tdh = ph ? -1 : 0; a.tdw = pw ? -1 : 0; a.bh = ph; a.bw = pw;
    a.Hout = 2 * h; a.Wout = 2 * w_; a.o_scale = 2; a.o_dh = ph; a.o_dw = pw;
    return 1;
}
// plain batched GEMM: one image row of `rows` pixels, one tap; blockIdx.z = the GEMM of the batch
static int geom_gemm_batch(IGemmArgs& a, int rows, int batch, long stride_a, long stride_b, long stride_c) {
    a.H = 1; a.W = rows; a.Hin = 1; a.Win = rows; a.a_scale = 1; a.KH = 1; a.KW = 1; a.Hout = 1; a.Wout = rows; a.o_scale = 1;
    a.w_tap_stride = 0; a.zbatch = 1; a.zs_x = stride_a; a.zs_w = stride_b; a.zs_y = stride_c;
    return batch;
}

// kernel = stride, no padding, no dilation, input a whole number of kernels: the data gradient takes geom_z_taps.
// RUNET_NO_LIVE_TAP_DGRAD=1 (measurement knob, tools/segformer_step.py --kernels): through the general a_div form instead.
static bool live_tap_dgrad(const Conv2dGeom& c) {
    static const bool off = env_flag("RUNET_NO_LIVE_TAP_DGRAD");
    return c.kh == c.stride && c.kw == c.stride && c.stride > 1 && c.pad_h == 0 && c.pad_w == 0 && c.dil_h == 1 && c.dil_w == 1 &&
           c.hin == c.ho * c.stride && c.win == c.wo * c.stride && !off;
}
// runet_conv2d_general / runet_conv2d_rect after validation: weights and geometry of a forward or a data gradient
static int conv2d_args(IGemmArgs& a, const Conv2dGeom& c, int mode) {
    if (mode == RUNET_CONV_FWD) { weights_n_contig(a); return geom_conv_fwd(a, c); }
    weights_k_contig(a);
    return live_tap_dgrad(c) ? geom_z_taps(a, c.ho, c.wo, c.stride) : geom_conv_dgrad(a, c);
}
// runet_conv_igemm's six modes: FWD / DGRAD(_T) are the stride-1 'same' case of the general forward and data gradient; the _T modes read
// per-tap transposed weights, so they take the n-contiguous layout.  Returns 0 for an unknown mode.
static int conv_igemm_args(IGemmArgs& a, int h, int w_, int kh, int kw, int dil, int mode) {
    switch (mode) {
    case RUNET_CONV_FWD: weights_n_contig(a); return geom_conv_fwd(a, same_conv(h, w_, kh, kw, dil));
    case RUNET_CONV_DGRAD: weights_k_contig(a); return geom_conv_dgrad(a, same_conv(h, w_, kh, kw, dil));
    case RUNET_CONV_DGRAD_T: weights_n_contig(a); return geom_conv_dgrad(a, same_conv(h, w_, kh, kw, dil));
    case RUNET_CONVT_FWD: weights_n_contig(a); return geom_z_taps(a, h, w_, 2);
    case RUNET_CONVT_DGRAD: weights_k_contig(a); return geom_convt_s2_dgrad(a, h, w_, 2, 0);
    case RUNET_CONVT_DGRAD_T: weights_n_contig(a); return geom_convt_s2_dgrad(a, h, w_, 2, 0);
    default: return 0;
    }
}
static int convt4_args(IGemmArgs& a, int h, int w_, int mode) {
    if (mode == RUNET_CONVT_FWD) { weights_n_contig(a); return geom_convt4_fwd(a, h, w_); }
    weights_k_contig(a);
    return geom_convt_s2_dgrad(a, h, w_, 4, 1);
}

// ------------------------------------------------------------------------------------------ the route: tile variant, weight layout, loader
enum IGemmVariant { V_128x32 = 0, V_256x64 = 1, V_128x64 = 2, V_128x128 = 3, V_64x64 = 4 };
template <int BM_, int BN_, int WM_, int WN_> struct Tile { static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_; };
// the one place that maps a variant to its template arguments: f(Tile<BM, BN, WM, WN>{})
template <typename F>
static void with_tile(IGemmVariant v, F&& f) {
    switch (v) {
    case V_128x32: f(Tile<128, 32, 32, 32>{}); break;
    case V_256x64: f(Tile<256, 64, 64, 64>{}); break;
    case V_128x64: f(Tile<128, 64, 64, 32>{}); break;
    case V_128x128: f(Tile<128, 128, 64, 64>{}); break;
    case V_64x64: f(Tile<64, 64, 32, 32>{}); break;
    }
}
static int variant_bm(IGemmVariant v) { return v == V_256x64 ? 256 : v == V_64x64 ? 64 : 128; }
// [k-contiguous weights][SIMPLE loader][tile variant]: the names rocprofv3 prints for the plain (no statistics) instantiations
static const char* const IGEMM_NAMES[2][2][5] = {
    {{"igemm_kernel<128, 32, 32, 32, false, false>", "igemm_kernel<256, 64, 64, 64, false, false>", "igemm_kernel<128, 64, 64, 32, false, false>",
      "igemm_kernel<128, 128, 64, 64, false, false>", "igemm_kernel<64, 64, 32, 32, false, false>"},
     {"igemm_kernel<128, 32, 32, 32, false, true>", "igemm_kernel<256, 64, 64, 64, false, true>", "igemm_kernel<128, 64, 64, 32, false, true>",
      "igemm_kernel<128, 128, 64, 64, false, true>", "igemm_kernel<64, 64, 32, 32, false, true>"}},
    {{"igemm_kernel<128, 32, 32, 32, true, false>", "igemm_kernel<256, 64, 64, 64, true, false>", "igemm_kernel<128, 64, 64, 32, true, false>",
      "igemm_kernel<128, 128, 64, 64, true, false>", "igemm_kernel<64, 64, 32, 32, true, false>"},
     {"igemm_kernel<128, 32, 32, 32, true, true>", "igemm_kernel<256, 64, 64, 64, true, true>", "igemm_kernel<128, 64, 64, 32, true, true>",
      "igemm_kernel<128, 128, 64, 64, true, true>", "igemm_kernel<64, 64, 32, 32, true, true>"}}};

int g_forced_variant = -1;      // tools/igemm_variants.py: time every tile variant on one shape (runet_igemm_force_variant)

// k1: channels read by a plain 1x1 convolution (0 for every other geometry); kc: k-contiguous weights (the data gradients);
// up2: the k2-s2 transposed convolution's data gradient
static IGemmVariant pick_variant(long P, int ncols, int k1, bool kc, bool up2) {
    if (g_forced_variant >= 0) return (IGemmVariant)g_forced_variant;
    if (ncols <= 32) return V_128x32;
    // 1x1 convolutions are short (K / 16 steps per tile) and near the HBM / MFMA balance point: many small tiles hide the prologue and
    // the `+=` epilogue behind other tiles better than few large ones.  Measured on the 32 1x1 launches of the 16 x 256^2 step
    // (tools/igemm_variants.py, profiles/round2_igemm_variants.txt): 64x64 wins for every data gradient and for every forward with
    // K <= 128 (10-30 %); from K = 256 on the forward prefers the large tiles below (weights re-read per tile start to count).
    static const bool old_rules = env_flag("RUNET_IGEMM_OLD_TILES");      // A/B knob
    if (!old_rules && k1 > 0 && (kc || k1 <= 128)) return V_64x64;
    if (!old_rules && up2 && kc && ncols <= 256) return V_64x64;      // same table: 199 -> 175 us (128 -> 256 @ 64^2), 198 -> 184 us (64 -> 128 @ 128^2)
    if (ncols <= 64) return (P >= 256L * 512) ? V_256x64 : V_128x64;
    const long blocks128 = (long)cdiv(P, 128) * cdiv(ncols, 128);
    if (blocks128 >= 512 || (ncols % 128 == 0 && blocks128 >= 256)) return V_128x128;
    if ((long)cdiv(P, 128) * cdiv(ncols, 64) < 256) return V_64x64;      // few pixels (deep levels): smaller tiles keep every CU busy
    return V_128x64;
}

// SIMPLE (see igemm_kernel): every tap of every row inside the source image, no coordinate division, K whole k-steps backed by x and w.
// That is the plain 1x1 convolution (also the s x s 1x1 GEMMs of geom_z_taps) and "up2", the k2-s2 transposed convolution's data gradient
// (source pixel (2h + r, 2w + s)).  RUNET_IGEMM_GENERAL=1 (measurement knob): the general loader everywhere.
struct IGemmRoute { IGemmVariant variant; bool kc, simple; };
static IGemmRoute igemm_route(const IGemmArgs& a) {
    static const bool no_simple = env_flag("RUNET_IGEMM_GENERAL");
    const long P = (long)a.Nimg * a.H * a.W;
    const bool plain1 = a.KH == 1 && a.KW == 1 && a.a_scale == 1 && a.Hin == a.H && a.Win == a.W;
    const bool up2 = a.KH == 2 && a.KW == 2 && a.z_taps == 0 && a.a_scale == 2 && a.tdh == 1 && a.tdw == 1 && a.Hin == 2 * a.H && a.Win == 2 * a.W;
    IGemmRoute r;
    r.kc = a.w_sn != 1;
    r.simple = !no_simple && (plain1 || up2) && a.a_div <= 1 && !a.zmode4 && a.bh == 0 && a.bw == 0 && a.K % 16 == 0 && a.Kx >= a.K && a.Kvalid >= a.K &&
               a.Ncols >= 4 && P > 0;
    r.variant = pick_variant(P, a.Ncols, (plain1 && a.z_taps == 0) ? a.K : 0, r.kc, up2);      // the z_taps GEMMs follow the general tile rules
    return r;
}
static const char* route_name(const IGemmRoute& r) { return IGEMM_NAMES[r.kc][r.simple][r.variant]; }

// Stats = float*: the statistics epilogue (only instantiated for the n-contiguous general loader, the k4 transposed forward)
template <int BM, int BN, int WM, int WN, bool KC, bool SIMPLE, typename... Stats>
static void launch_igemm(const IGemmArgs& a, int gz, hipStream_t st, Stats... stats) {
    const long P = (long)a.Nimg * a.H * a.W;
    dim3 grid(cdiv(P, BM), cdiv(a.Ncols, BN), gz);
    constexpr int LDS_FLOATS = 2 * (BM * 20 + 16 * (BN + 4));
    static_assert(sizeof...(Stats) == 0 || (BM / WM) * BN * 3 <= LDS_FLOATS, "statistics exchange fits the stages");
    hipLaunchKernelGGL((igemm_kernel<BM, BN, WM, WN, KC, SIMPLE, Stats...>), grid, dim3(256), LDS_FLOATS * sizeof(float), st, a, stats...);
}
static void launch_route(const IGemmArgs& a, const IGemmRoute& r, int gz, hipStream_t st) {
    with_tile(r.variant, [&](auto t) {
        using T = decltype(t);
        if (!r.kc && r.simple) launch_igemm<T::BM, T::BN, T::WM, T::WN, false, true>(a, gz, st);
        else if (!r.kc) launch_igemm<T::BM, T::BN, T::WM, T::WN, false, false>(a, gz, st);
        else if (r.simple) launch_igemm<T::BM, T::BN, T::WM, T::WN, true, true>(a, gz, st);
        else launch_igemm<T::BM, T::BN, T::WM, T::WN, true, false>(a, gz, st);
    });
}
static void dispatch_igemm(const IGemmArgs& a, int gz, hipStream_t st) { launch_route(a, igemm_route(a), gz, st); }

// ------------------------------------------------------------------------------------------ the per-tap split-K weight gradient
template <int BM, int BN, int WM, int WN>
static void launch_wgrad(const WGradArgs& a, dim3 grid, hipStream_t st) {
    const size_t lds = 2 * (16 * (BM + 4) + 16 * (BN + 4)) * sizeof(float);      // two stages of wgrad_kernel's A and B tiles
    hipLaunchKernelGGL((wgrad_kernel<BM, BN, WM, WN>), grid, dim3(256), lds, st, a);
}
// 128 x 128 tiles where both channel counts exceed 64, else 64 x 64; grid = (tiles, taps, splits)
static int wgrad_tiles(bool big, int cin_w, int cout) { return big ? cdiv(cin_w, 128) * cdiv(cout, 128) : cdiv(cin_w, 64) * cdiv(cout, 64); }
static void launch_wgrad_tiles(const WGradArgs& a, bool big, int cin_w, int cout, int ntaps, int splits, hipStream_t st) {
    const dim3 grid(wgrad_tiles(big, cin_w, cout), ntaps, splits);
    if (big) launch_wgrad<128, 128, 64, 64>(a, grid, st);
    else launch_wgrad<64, 64, 32, 32>(a, grid, st);
}
// dw[i] = sum over the slabs, in a fixed order
static void reduce_slabs(const float* slabs, float* dw, long wsize, int nsplit, hipStream_t st) {
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(cdiv(wsize, 32 * 4)), dim3(256), 0, st, slabs, dw, wsize, nsplit);
}

struct WGradPlan { bool big; int splits; };
static WGradPlan wgrad_plan(long P, int cin_w, int cout, int ntaps) {
    const bool big = (cin_w > 64 && cout > 64);
    const long base = (long)wgrad_tiles(big, cin_w, cout) * ntaps;
    long want = (768 + base - 1) / base;            // aim for >= 3 blocks per CU
    const long maxs = (P + 255) / 256;              // at least 256 pixels per split
    if (want > maxs) want = maxs;
    if (want > 64) want = 64;
    if (want < 1) want = 1;
    return {big, (int)want};
}
// floats of workspace for `splits` partial slabs of a [ntaps][cin_w][cout] gradient (one slab goes straight to dw)
static long slab_floats(int splits, int ntaps, int cin_w, int cout) { return splits > 1 ? (long)splits * ntaps * cin_w * cout : 0; }
static long wgrad_workspace(long P, int cin_w, int cout, int ntaps) { return slab_floats(wgrad_plan(P, cin_w, cout, ntaps).splits, ntaps, cin_w, cout); }

// The tail of every per-tap weight gradient: `a` has its geometry; P pixels are summed.  Plans the splits, clamps them to the workspace given,
// rounds the pixels of a split to whole k-steps, launches and reduces.
static void launch_wgrad_splitk(WGradArgs a, long P, int cin_w, int cout, int ntaps, float* dw, float* workspace, long workspace_floats, hipStream_t st) {
    const WGradPlan plan = wgrad_plan(P, cin_w, cout, ntaps);
    int splits = plan.splits;
    const long wsize = (long)ntaps * cin_w * cout;
    if (splits > 1 && (workspace == nullptr || workspace_floats < splits * wsize)) {
        splits = workspace ? (int)(workspace_floats / wsize) : 1;
        if (splits < 1) splits = 1;
    }
    long pps = (P + splits - 1) / splits;
    pps = (pps + 15) / 16 * 16;
    splits = cdiv(P, pps);
    a.pix_per_split = pps;
    a.out = (splits > 1) ? workspace : dw;
    launch_wgrad_tiles(a, plan.big, cin_w, cout, ntaps, splits, st);
    if (splits > 1) reduce_slabs(workspace, dw, wsize, splits, st);
}

static WGradArgs wgrad_operands(const float* x, int ldx, const float* dy, int ldy, int n_img, int cin, int cin_w, int cout) {
    WGradArgs a{};
    a.x = x; a.ldx = ldx; a.dy = dy; a.ldy = ldy; a.Kci = cin; a.Kvalid = cin_w; a.Nco = cout; a.Nimg = n_img;
    return a;
}
// weight gradient of geom_conv_fwd's convolution: pixels summed = output pixels, tap (r, s) shifts the x pixel
static long wgrad_geom_conv(WGradArgs& a, const Conv2dGeom& c) {
    a.H = c.ho; a.W = c.wo; a.Hin = c.hin; a.Win = c.win; a.a_scale = c.stride; a.KH = c.kh; a.KW = c.kw;
    a.tdh = c.dil_h; a.tdw = c.dil_w; a.bh = -c.pad_h; a.bw = -c.pad_w;
    a.Hout = c.ho; a.Wout = c.wo; a.o_scale = 1;
    return (long)a.Nimg * c.ho * c.wo;
}
// ... of ConvTranspose2d(k4, s2, p1): pixels summed = input pixels, tap (r, s) shifts the dy pixel (2h - 1 + r, 2w - 1 + s)
static long wgrad_geom_convt4(WGradArgs& a, int h, int w_) {
    a.H = h; a.W = w_; a.Hin = h; a.Win = w_; a.a_scale = 1; a.KH = 4; a.KW = 4;
    a.tap_on_output = 1; a.o_bh = -1; a.o_bw = -1; a.Hout = 2 * h; a.Wout = 2 * w_; a.o_scale = 2;
    return (long)a.Nimg * h * w_;
}

}  // namespace

extern "C" int runet_transpose_taps(const float* w, float* wt, int taps, int cin, int cout, void* stream) {
    RUNET_REQUIRE(w && wt && taps > 0 && cin > 0 && cout > 0, "bad arguments");
    hipLaunchKernelGGL(transpose_taps_kernel, dim3(cdiv(cout, 32), cdiv(cin, 32), taps), dim3(256), 0, (hipStream_t)stream, w, wt, cin, cout);
    RUNET_CHECK_LAUNCH();
}

int g_lowp_forced_variant = -1;      // shared by conv_bf16.hip / conv_fp16.hip (conv_lowp.inc)

extern "C" int runet_igemm_lowp_force_variant(int variant) {
    RUNET_REQUIRE(variant >= -1 && variant <= 2, "variant: -1 (automatic) or 0..2");
    g_lowp_forced_variant = variant;
    return 0;
}

extern "C" int runet_igemm_force_variant(int variant) {
    RUNET_REQUIRE(variant >= -1 && variant <= 4, "variant: -1 (automatic) or 0..4");
    g_forced_variant = variant;
    return 0;
}

// ------------------------------------------------------------------------------------------ 1x1 / 3x3 / k2-s2 transposed (RobustUNet)
// which device kernel runet_conv_igemm launches for a shape: the same builder and route, without operands (ops.py labels its profile rows with it)
extern "C" const char* runet_conv_igemm_kernel_name(int n_img, int h, int w_, int cin, int cout, int kh, int mode) {
    IGemmArgs a = igemm_operands(nullptr, cin, nullptr, nullptr, nullptr, cout, n_img, cin, cin, cout, 0);
    if (!conv_igemm_args(a, h, w_, kh, kh, 1, mode)) return "unknown mode";
    return route_name(igemm_route(a));
}

extern "C" int runet_conv_igemm(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy,
                                 int n_img, int h, int w_, int cin, int cin_w, int cout, int kh, int kw, int dil,
                                 int mode, int accumulate, void* stream) {
    RUNET_REQUIRE(x && w && y, "null pointer");
    RUNET_REQUIRE(cin > 0 && cin % 4 == 0, "cin (channels read from x) must be a positive multiple of 4");
    RUNET_REQUIRE(cin_w > 0 && cin_w <= cin, "cin_w (rows present in the weight) must be in (0, cin]");
    RUNET_REQUIRE(cout > 0 && cout % 4 == 0, "cout must be a positive multiple of 4");
    RUNET_REQUIRE(ldx >= cin && ldx % 4 == 0 && ldy % 4 == 0, "pixel strides must be multiples of 4 floats and cover the channels");
    RUNET_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)w % 16) == 0 && ((uintptr_t)y % 16) == 0, "pointers must be 16-byte aligned");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty iteration space");
    RUNET_REQUIRE((kh == 1 && kw == 1) || (kh == 3 && kw == 3) || (kh == 2 && kw == 2), "kernel must be 1x1, 3x3 or 2x2(transposed)");
    switch (mode) {
    case RUNET_CONV_FWD:      // y[N,h,w,cout] = conv(x[N,h,w,cin], w[kh,kw,cin_w,cout]), 'same' padding = dil*(k-1)/2
        RUNET_REQUIRE(kh != 2, "2x2 kernels are transposed-conv only");
        RUNET_REQUIRE(ldy >= cout, "ldy < cout");
        break;
    case RUNET_CONV_DGRAD:    // x := dy [N,h,w,cin(=conv Cout)], y := dx [N,h,w,cout(=conv Cin)]; w is the forward weight [kh,kw,cout,cin]
        RUNET_REQUIRE(kh != 2, "use RUNET_CONVT_DGRAD for 2x2");
        RUNET_REQUIRE(cin_w == cin, "dgrad reads every output channel");
        break;
    case RUNET_CONV_DGRAD_T:  // as RUNET_CONV_DGRAD with the weight already transposed per tap: w [kh,kw,cin(conv Cout),cout(conv Cin)]
        RUNET_REQUIRE(kh != 2 && cin_w == cin, "dgrad reads every output channel; use RUNET_CONVT_DGRAD_T for 2x2");
        break;
    case RUNET_CONVT_FWD:     // y[N,2h,2w,cout] = convT_k2s2(x[N,h,w,cin]); w [2,2,cin,cout]
    case RUNET_CONVT_DGRAD:   // dx[N,h,w,cout(=convT Cin)] from dy[N,2h,2w,cin(=convT Cout)]; w [2,2,cout,cin]
    case RUNET_CONVT_DGRAD_T: // as RUNET_CONVT_DGRAD with w [2,2,cin(convT Cout),cout(convT Cin)]
        RUNET_REQUIRE(kh == 2 && kw == 2 && cin_w == cin, "transposed conv is 2x2 stride 2");
        break;
    default:
        RUNET_REQUIRE(false, "unknown mode");
    }
    IGemmArgs a = igemm_operands(x, ldx, w, bias, y, ldy, n_img, cin, cin_w, cout, accumulate);
    const int gz = conv_igemm_args(a, h, w_, kh, kw, dil, mode);
    dispatch_igemm(a, gz, (hipStream_t)stream);
    RUNET_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------ its weight gradient: one route of five
// 1x1 weight gradient = one TN GEMM over the pixels (dW[cin][cout] = x^T dy): rows per split, 16-aligned.  The split count aims at ~2048
// 64 x 64 wave tiles on the chip; wm, wn count them per block side as a removed kernel with one-, two- and four-wave blocks did (both
// GEMM kernels here use 128 x 128 blocks of four).  The formula stays: it fixes the split count, therefore the summation order of the wide
// GEMMs, and the workspace size every caller is told.
static int wgrad1x1_rows_per_split(long P, int cin, int cout) {
    const int wm = cin > 64 ? 2 : 1, wn = cout > 64 ? 2 : 1;
    const long tiles = (long)cdiv(cin, 64 * wm) * cdiv(cout, 64 * wn);
    long splits = cdiv(2048, tiles * wm * wn);
    const long maxs = P / 256 > 0 ? P / 256 : 1;
    if (splits > maxs) splits = maxs;
    return (int)((cdiv(P, splits) + 15) / 16 * 16);
}
// the transposed convolution's weight gradient on the split-operand TN GEMM: 4 taps = 4 GEMMs over the low-resolution pixels, up to
// 512 / tiles splits of at least 256 rows; -> rows per split (16-aligned)
static int convt_wgrad_x3_rows_per_split(long P, int cin, int cout) {
    const long tiles = (long)cdiv(cin, 128) * cdiv(cout, 128) * 4;
    long splits = cdiv(512, tiles);
    const long maxs = P / 256 > 0 ? P / 256 : 1;
    if (splits > maxs) splits = maxs;
    return (int)((cdiv(P, splits) + 15) / 16 * 16);
}

enum WGradKind { WG_STEM, WG_GEMM_TN, WG_CONVT_X3, WG_TILE, WG_SPLITK };
struct WGradRoute {
    WGradKind kind;
    bool x3;            // WG_GEMM_TN: gemm_split.hip's split-operand kernel, else gemm.hip's f32 one
    int rps;            // WG_GEMM_TN, WG_CONVT_X3: rows (pixels) per split
    int splits;         // partial sums as planned; WG_TILE and WG_SPLITK shrink them to the workspace they are given
    long slab;          // floats of one partial sum = of dw
    TilePlan tile;      // WG_TILE
    // Floats of workspace to announce for the route.  The stem's 64 slabs on top and the GEMMs' slab for a single split are not used by
    // the launches below; they are the sizes callers have always been told and stay.
    long workspace() const {
        if (kind == WG_STEM) return (long)splits * slab + 64 * slab;
        if (kind == WG_GEMM_TN || kind == WG_CONVT_X3) return splits * slab;
        return splits > 1 ? splits * slab : 0;
    }
};
// rows per split, splits and slab of one kind for a shape (cin_w input channels take part)
static WGradRoute wgrad_plan_as(WGradKind kind, int n_img, int h, int w_, int cin_w, int cout, int kh, int kw, int transposed) {
    const long P = (long)n_img * h * w_;
    WGradRoute r{};
    r.kind = kind;
    r.slab = (long)kh * kw * cin_w * cout;
    switch (kind) {
    case WG_STEM: r.splits = cdiv(h, STEM_ROWS) * n_img; break;
    case WG_GEMM_TN: r.rps = wgrad1x1_rows_per_split(P, cin_w, cout); r.splits = cdiv(P, r.rps); break;
    case WG_CONVT_X3: r.rps = convt_wgrad_x3_rows_per_split(P, cin_w, cout); r.splits = cdiv(P, r.rps); break;
    case WG_TILE: r.tile = wgrad_tile_plan(n_img, h, w_, cin_w, cout, transposed ? 1 : kh, transposed ? 4 : 1); r.splits = r.tile.splits; break;
    default: r.splits = wgrad_plan(P, cin_w, cout, kh * kw).splits; break;
    }
    return r;
}
// Which kernel family takes the shape, and with which plan.
//   stem: the RGB stem's 3x3 (conv_igemm.hip's stem_wgrad_kernel).
//   TN GEMM: the 1x1 weight gradient as one TN GEMM over the pixels where both channel counts fill a 128 x 128 tile; narrower layers stay
//     on wgrad_tile_kernel<1,..>, whose per-tile integer address arithmetic costs it 30-77 TFLOP/s on the wide ones.  Measured
//     (tools/conv_launches.py, 16 x 256^2 step): 256->128 @ 128^2 231 -> 159 us, 512->256 @ 64^2 223 -> 155, 1024->512 @ 32^2 220 -> 153,
//     the ten wide launches 1.13 -> 0.83 ms; 128->64 / 64->128 @ 128^2 would go 89 -> 131 us (half-empty tiles).  The step time does not
//     move (weight gradients run on the side stream); the GPU does 0.3 ms less work.  RUNET_WGRAD1X1_TILE=1: tile kernel everywhere.
//     The split-operand kernel (gemm_split.hip, BF16 matrix cores, fp32-accurate) where the pixel count is a multiple of 16, else gemm.hip's.
//   transposed x3: ConvTranspose2d(k2, s2) on the split-operand TN GEMM: image width a multiple of 16 (a k-step's rows share an image row).
//   tile kernel: the other 1x1, 3x3 at dilation 1 and transposed 2x2 shapes.   split-K: what is left, 3x3 with dilation > 1.
constexpr int WGRAD1X1_GEMM_MIN_CH = 128;      // channels the NARROWER side of a 1x1 needs for the TN GEMM (half-empty 128 x 128 tiles below)
constexpr int CONVT_X3_WGRAD_MIN_CH = 64;      // channels both sides of a transposed convolution need for the split-operand TN GEMM
static WGradRoute wgrad_route(int n_img, int h, int w_, int cin, int cin_w, int cout, int kh, int kw, int dil, int transposed) {
    static const bool no_x3 = env_flag("RUNET_NO_X3"), tile_1x1 = env_flag("RUNET_WGRAD1X1_TILE"), no_convt_x3 = env_flag("RUNET_NO_CONVT_WGRAD_X3");
    const long P = (long)n_img * h * w_;
    const bool k1 = kh == 1 && kw == 1, k2 = kh == 2 && kw == 2, k3 = kh == 3 && kw == 3;
    const int lo = cin < cout ? cin : cout;
    WGradKind kind = WG_SPLITK;
    if (!transposed && k3 && dil == 1 && cin == 4 && cout <= 1024 && 256 % (cout / 4) == 0) kind = WG_STEM;
    else if (!transposed && k1 && cin_w == cin && !tile_1x1 && P * 4 < (1L << 31) && lo >= WGRAD1X1_GEMM_MIN_CH) kind = WG_GEMM_TN;
    else if (transposed && k2 && cin_w == cin && !no_x3 && !no_convt_x3 && w_ % 16 == 0 && P % 16 == 0 && P < (1L << 31) && lo >= CONVT_X3_WGRAD_MIN_CH)
        kind = WG_CONVT_X3;
    else if (transposed ? k2 : (k1 || (k3 && dil == 1))) kind = WG_TILE;
    WGradRoute r = wgrad_plan_as(kind, n_img, h, w_, cin_w, cout, kh, kw, transposed);
    r.x3 = kind == WG_GEMM_TN && !no_x3 && P % 16 == 0;
    return r;
}

// The largest workspace any route of runet_conv_wgrad may use for the shape.  cin, the dilation and the knobs are unknown here, so every
// kind the kernel size admits counts, whether wgrad_route would pick it or not.
extern "C" long runet_conv_wgrad_workspace_floats(int n_img, int h, int w_, int cin_w, int cout, int kh, int kw) {
    const bool k1 = kh == 1 && kw == 1, k2 = kh == 2 && kw == 2, k3 = kh == 3 && kw == 3;
    auto ws = [&](WGradKind kind) { return wgrad_plan_as(kind, n_img, h, w_, cin_w, cout, kh, kw, k2).workspace(); };
    if (k1) return std::max(ws(WG_GEMM_TN), ws(WG_TILE));
    if (k3 && cin_w <= 4) return ws(WG_STEM);
    if (k2) return std::max({ws(WG_CONVT_X3), ws(WG_TILE), ws(WG_SPLITK)});
    if (k3) return std::max(ws(WG_TILE), ws(WG_SPLITK));
    return ws(WG_SPLITK);
}

extern "C" int runet_conv_wgrad(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace,
                                 long workspace_floats, int n_img, int h, int w_, int cin, int cin_w, int cout,
                                 int kh, int kw, int dil, int transposed, void* stream) {
    RUNET_REQUIRE(x && dy && dw, "null pointer");
    RUNET_REQUIRE(cin > 0 && cin % 4 == 0 && cin_w > 0 && cin_w <= cin, "cin must be a multiple of 4, cin_w in (0, cin]");
    RUNET_REQUIRE(cout > 0 && cout % 4 == 0, "cout must be a positive multiple of 4");
    RUNET_REQUIRE(ldx >= cin && ldx % 4 == 0 && ldy >= cout && ldy % 4 == 0, "bad pixel strides");
    RUNET_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)dy % 16) == 0 && ((uintptr_t)dw % 16) == 0, "pointers must be 16-byte aligned");
    RUNET_REQUIRE((kh == 1 && kw == 1) || (kh == 3 && kw == 3) || (kh == 2 && kw == 2 && transposed), "unsupported kernel size");
    hipStream_t st = (hipStream_t)stream;
    const long P = (long)n_img * h * w_;
    WGradRoute r = wgrad_route(n_img, h, w_, cin, cin_w, cout, kh, kw, dil, transposed);
    if (r.kind == WG_SPLITK) {      // plans, shrinks to the workspace and reduces on its own, as for the general and rectangular entry points
        WGradArgs a = wgrad_operands(x, ldx, dy, ldy, n_img, cin, cin_w, cout);
        wgrad_geom_conv(a, same_conv(h, w_, kh, kw, dil));
        launch_wgrad_splitk(a, P, cin_w, cout, kh * kw, dw, workspace, workspace_floats, st);
        RUNET_CHECK_LAUNCH();
    }
    const long wsize = r.slab;
    // a workspace too small for the transposed GEMM's splits: the tile kernel, which shrinks its splits to what it is given
    if (r.kind == WG_CONVT_X3 && r.splits > 1 && !(workspace && workspace_floats >= r.splits * wsize))
        r = wgrad_plan_as(WG_TILE, n_img, h, w_, cin_w, cout, kh, kw, transposed);
    int splits = r.splits;
    switch (r.kind) {
    case WG_STEM: {
        const int nblk = splits;
        RUNET_REQUIRE(workspace && workspace_floats >= nblk * wsize, "workspace too small for the stem weight gradient");
        hipLaunchKernelGGL(stem_wgrad_kernel, dim3(cdiv(h, STEM_ROWS), n_img), dim3(256), 0, st, x, ldx, dy, ldy, workspace, h, w_, cin_w, cout);
        break;
    }
    case WG_GEMM_TN: {
        RUNET_REQUIRE(splits == 1 || (workspace && workspace_floats >= splits * wsize), "workspace too small (runet_conv_wgrad_workspace_floats)");
        const int rc = r.x3 ? runet_gemm_x3_tn_batched(x, ldx, 0, dy, ldy, 0, splits > 1 ? workspace : dw, 1, (int)P, cin, cout, r.rps, stream)
                            : runet_gemm_tn_launch(x, ldx, 0, dy, ldy, 0, splits > 1 ? workspace : dw, 1, (int)P, cin, cout, r.rps, st);
        if (rc) return rc;
        break;
    }
    case WG_CONVT_X3: {
        const int rc = runet_gemm_x3_tn_convt(x, ldx, dy, ldy, splits > 1 ? workspace : dw, n_img, h, w_, cin, cout, r.rps, stream);
        if (rc) return rc;
        break;
    }
    default: {      // WG_TILE (WG_SPLITK has returned above)
        TilePlan& p = r.tile;
        if (p.splits > 1 && (workspace == nullptr || workspace_floats < p.splits * wsize)) {
            int s2 = workspace ? (int)(workspace_floats / wsize) : 1;
            if (s2 < 1) s2 = 1;
            p.tps = cdiv(p.total_tiles, s2);
            p.splits = cdiv(p.total_tiles, p.tps);
        }
        splits = p.splits;
        WGradTileArgs t{};
        t.x = x; t.ldx = ldx; t.dy = dy; t.ldy = ldy; t.out = (p.splits > 1) ? workspace : dw;
        t.Kci = cin; t.Kvalid = cin_w; t.Nco = cout; t.Nimg = n_img; t.H = h; t.W = w_;
        t.tiles_h = p.tiles_h; t.tiles_w = p.tiles_w; t.total_tiles = p.total_tiles; t.tiles_per_split = p.tps; t.co_chunks = p.co_chunks;
        t.dy_up = transposed ? 1 : 0;
        if (kh == 3) launch_wgrad_tile<3, 1, 1>(t, p, st);
        else if (p.tm == 2 && p.tn == 2) launch_wgrad_tile<1, 2, 2>(t, p, st);
        else if (p.tm == 2) launch_wgrad_tile<1, 2, 1>(t, p, st);
        else if (p.tn == 2) launch_wgrad_tile<1, 1, 2>(t, p, st);
        else launch_wgrad_tile<1, 1, 1>(t, p, st);
    }
    }
    if (r.kind == WG_STEM || splits > 1) reduce_slabs(workspace, dw, wsize, splits, st);
    RUNET_CHECK_LAUNCH();
}


// ---------------------------------------------------------------------------------------------------------------------------
// General (strided / large-kernel / k4 transposed) convolutions for the DeepLabV3+ baseline (/root/reference/Main_Final.py:325-433:
// Conv2d 7x7 s2 p3, 3x3 s2 p1, 3x3 dilation 6/12/18, ConvTranspose2d k4 s2 p1) and SegFormer-Lite (Extended_Baseline_Comparison.py:645,
// 677-688: Conv2d 7x7 s4 p3 and the key / value reductions, kernel = stride = 8, 4, 2, no padding).  Same kernels, other geometry: kernels
// up to 8x8, strides up to 8.  FWD: x [n,hin,win,cin] -> y [n,ho,wo,cout];  DGRAD: x := dy [n,ho,wo,cin(=conv Cout)] -> y := dx
// [n,hin,win,cout(=conv Cin)], w [kh,kw,cout,cin].
extern "C" int runet_conv2d_general(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int hin,
                                    int win, int cin, int cin_w, int cout, int kh, int kw, int stride, int pad, int dil, int mode,
                                    int accumulate, void* stream) {
    RUNET_REQUIRE(x && w && y, "null pointer");
    RUNET_REQUIRE(cin > 0 && cin % 4 == 0 && cin_w > 0 && cin_w <= cin && cout > 0 && cout % 4 == 0, "channel counts must be multiples of 4");
    RUNET_REQUIRE(kh >= 1 && kh <= 8 && kw >= 1 && kw <= 8 && stride >= 1 && stride <= 8 && pad >= 0 && dil >= 1, "unsupported geometry");
    RUNET_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)w % 16) == 0 && ((uintptr_t)y % 16) == 0, "alignment");
    const int ho = (hin + 2 * pad - dil * (kh - 1) - 1) / stride + 1, wo = (win + 2 * pad - dil * (kw - 1) - 1) / stride + 1;
    RUNET_REQUIRE(ho > 0 && wo > 0, "empty output");
    if (mode == RUNET_CONV_FWD) {
        RUNET_REQUIRE(ldx >= cin && ldy >= cout, "bad pixel strides");
    } else if (mode == RUNET_CONV_DGRAD) {
        RUNET_REQUIRE(cin_w == cin && ldx >= cin && ldy >= cout, "bad arguments for the data gradient");
    } else {
        RUNET_REQUIRE(false, "mode must be RUNET_CONV_FWD or RUNET_CONV_DGRAD");
    }
    IGemmArgs a = igemm_operands(x, ldx, w, bias, y, ldy, n_img, cin, cin_w, cout, accumulate);
    const int gz = conv2d_args(a, {hin, win, ho, wo, kh, kw, stride, pad, pad, dil, dil}, mode);
    dispatch_igemm(a, gz, (hipStream_t)stream);
    RUNET_CHECK_LAUNCH();
}

// ConvTranspose2d(k4, s2, p1): w [4][4][cin][cout].  FWD: x [n,h,w,cin] -> y [n,2h,2w,cout];  DGRAD: x := dy [n,2h,2w,cin(=Cout)] -> y := dx [n,h,w,cout(=Cin)]
extern "C" int runet_convt4_igemm(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int h, int w_,
                                  int cin, int cout, int mode, int accumulate, void* stream) {
    RUNET_REQUIRE(x && w && y && cin % 4 == 0 && cout % 4 == 0 && cin > 0 && cout > 0, "bad arguments");
    RUNET_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)w % 16) == 0 && ((uintptr_t)y % 16) == 0, "alignment");
    if (mode != RUNET_CONVT_FWD && mode != RUNET_CONVT_DGRAD) RUNET_REQUIRE(false, "mode must be RUNET_CONVT_FWD or RUNET_CONVT_DGRAD");
    IGemmArgs a = igemm_operands(x, ldx, w, bias, y, ldy, n_img, cin, cin, cout, accumulate);
    const int gz = convt4_args(a, h, w_, mode);
    dispatch_igemm(a, gz, (hipStream_t)stream);
    RUNET_CHECK_LAUNCH();
}

// runet_convt4_igemm(RUNET_CONVT_FWD) + the BatchNorm statistics partials of y for runet_bn_stats_finalize: one part per tile and parity
// class (the tile's output pixels of one (ph, pw) class), stats [runet_convt4_igemm_stats_parts(...)][cout][3] = (count, mean, M2).
// Same builder, same route, hence the tile variant, grid and y of the plain call; the loader is the general one (zmode4).
extern "C" int runet_convt4_igemm_stats_parts(int n_img, int h, int w_, int cout) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || cout <= 0) return 0;
    IGemmArgs a = igemm_operands(nullptr, 0, nullptr, nullptr, nullptr, 0, n_img, 4, 4, cout, 0);      // the route of this geometry does not look at cin
    const int gz = convt4_args(a, h, w_, RUNET_CONVT_FWD);
    return gz * cdiv((long)n_img * h * w_, variant_bm(igemm_route(a).variant));
}

extern "C" int runet_convt4_igemm_stats(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int h, int w_,
                                        int cin, int cout, float* stats, void* stream) {
    RUNET_REQUIRE(x && w && y && stats, "null pointer");
    RUNET_REQUIRE(cin % 4 == 0 && cout % 4 == 0 && cin > 0 && cout > 0, "cin and cout must be positive multiples of 4");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0 && ldx >= cin && ldy >= cout, "bad shape");
    RUNET_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)w % 16) == 0 && ((uintptr_t)y % 16) == 0, "alignment");
    hipStream_t st = (hipStream_t)stream;
    IGemmArgs a = igemm_operands(x, ldx, w, bias, y, ldy, n_img, cin, cin, cout, 0);
    const int gz = convt4_args(a, h, w_, RUNET_CONVT_FWD);
    with_tile(igemm_route(a).variant, [&](auto t) {
        using T = decltype(t);
        launch_igemm<T::BM, T::BN, T::WM, T::WN, false, false>(a, gz, st, stats);
    });
    RUNET_CHECK_LAUNCH();
}

// weight gradient for the general geometries (per-tap split-K kernel).  transposed4 != 0: ConvTranspose2d(k4,s2,p1), x [n,h,w,cin], dy [n,2h,2w,cout].
extern "C" long runet_conv_wgrad_general_workspace_floats(int pixels, int cin_w, int cout, int kh, int kw) {
    return wgrad_workspace(pixels, cin_w, cout, kh * kw);
}

extern "C" int runet_conv_wgrad_general(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats,
                                        int n_img, int hin, int win, int cin, int cin_w, int cout, int kh, int kw, int stride, int pad, int dil,
                                        int transposed4, void* stream) {
    RUNET_REQUIRE(x && dy && dw, "null pointer");
    RUNET_REQUIRE(cin % 4 == 0 && cin_w > 0 && cin_w <= cin && cout % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0, "channel counts / strides must be multiples of 4");
    RUNET_REQUIRE(transposed4 || (kh >= 1 && kh <= 8 && kw >= 1 && kw <= 8 && stride >= 1 && stride <= 8 && pad >= 0 && dil >= 1), "unsupported geometry");
    if (transposed4) RUNET_REQUIRE(kh == 4 && kw == 4, "transposed4 is the k4-s2-p1 transposed convolution");
    WGradArgs a = wgrad_operands(x, ldx, dy, ldy, n_img, cin, cin_w, cout);
    long P;
    if (transposed4) {
        P = wgrad_geom_convt4(a, hin, win);
    } else {
        const int ho = (hin + 2 * pad - dil * (kh - 1) - 1) / stride + 1, wo = (win + 2 * pad - dil * (kw - 1) - 1) / stride + 1;
        P = wgrad_geom_conv(a, {hin, win, ho, wo, kh, kw, stride, pad, pad, dil, dil});
    }
    launch_wgrad_splitk(a, P, cin_w, cout, kh * kw, dw, workspace, workspace_floats, (hipStream_t)stream);
    RUNET_CHECK_LAUNCH();
}

// Rectangular kernels with per-axis padding and dilation for the ENet baseline (comne.py:482-608: the asymmetric bottleneck's Conv2d (5, 1)
// padding (2, 0) and (1, 5) padding (0, 2)).  runet_conv2d_general's contract with (pad_h, pad_w) and (dil_h, dil_w): both go through
// conv2d_args, so equal pads and dilations give runet_conv2d_general's launches and bits.
extern "C" int runet_conv2d_rect(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int hin, int win,
                                 int cin, int cin_w, int cout, int kh, int kw, int stride, int pad_h, int pad_w, int dil_h, int dil_w, int mode,
                                 int accumulate, void* stream) {
    RUNET_REQUIRE(x && w && y, "null pointer");
    RUNET_REQUIRE(cin > 0 && cin % 4 == 0 && cin_w > 0 && cin_w <= cin && cout > 0 && cout % 4 == 0, "channel counts must be multiples of 4");
    RUNET_REQUIRE(kh >= 1 && kh <= 8 && kw >= 1 && kw <= 8 && stride >= 1 && stride <= 8 && pad_h >= 0 && pad_w >= 0 && dil_h >= 1 && dil_w >= 1,
                  "unsupported geometry");
    RUNET_REQUIRE(n_img > 0 && hin > 0 && win > 0, "empty shape");
    RUNET_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)w % 16) == 0 && ((uintptr_t)y % 16) == 0, "alignment");
    const int ho = (hin + 2 * pad_h - dil_h * (kh - 1) - 1) / stride + 1, wo = (win + 2 * pad_w - dil_w * (kw - 1) - 1) / stride + 1;
    RUNET_REQUIRE(hin + 2 * pad_h - dil_h * (kh - 1) > 0 && win + 2 * pad_w - dil_w * (kw - 1) > 0 && ho > 0 && wo > 0, "empty output");
    if (mode == RUNET_CONV_FWD) {
        RUNET_REQUIRE(ldx >= cin && ldy >= cout, "bad pixel strides");
    } else if (mode == RUNET_CONV_DGRAD) {
        RUNET_REQUIRE(cin_w == cin && ldx >= cin && ldy >= cout, "bad arguments for the data gradient");
    } else {
        RUNET_REQUIRE(false, "mode must be RUNET_CONV_FWD or RUNET_CONV_DGRAD");
    }
    IGemmArgs a = igemm_operands(x, ldx, w, bias, y, ldy, n_img, cin, cin_w, cout, accumulate);
    const int gz = conv2d_args(a, {hin, win, ho, wo, kh, kw, stride, pad_h, pad_w, dil_h, dil_w}, mode);
    dispatch_igemm(a, gz, (hipStream_t)stream);
    RUNET_CHECK_LAUNCH();
}

// ConvTranspose2d(k3, s2, p1, output_padding 1) forward by output parity class (ENet's decoder.0 / decoder.3): output pixel (2i + ph, 2j + pw)
// takes the taps r = 1 (ph = 0: source row i) or r = 0, 2 (ph = 1: source rows i + 1, i), likewise for columns - 1, 2, 2 or 4 live taps instead
// of the 9 (mostly dead) per output pixel that the data-gradient form of runet_conv2d_general runs: four GEMMs over the INPUT pixels whose rows
// land on the class's output pixels (o_scale = 2).  wq [9][cin][cout]: the parameter's [3][3][cin][cout] slabs in class order,
// (1,1) | (1,0) (1,2) | (0,1) (2,1) | (0,0) (0,2) (2,0) (2,2), so that tap t = rr * KW + ss of a class reads source (i + ph (1 - rr), j + pw (1 - ss)).
extern "C" int runet_convt3_pack(const float* w, float* wq, int cin, int cout, void* stream) {
    RUNET_REQUIRE(w && wq, "null pointer");
    RUNET_REQUIRE(cin > 0 && cin % 4 == 0 && cout > 0 && cout % 4 == 0, "channel counts must be multiples of 4");
    RUNET_REQUIRE(((uintptr_t)w % 16) == 0 && ((uintptr_t)wq % 16) == 0, "alignment");
    RUNET_REQUIRE(w != wq, "wq must not be w (the slabs are permuted, not moved in place)");
    static const int order[9] = {4, 3, 5, 1, 7, 0, 2, 6, 8};
    const size_t slab = (size_t)cin * cout;
    for (int t = 0; t < 9; ++t) {
        if (hipMemcpyAsync(wq + t * slab, w + order[t] * slab, slab * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) break;
    }
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_convt3_fwd(const float* x, int ldx, const float* wq, const float* bias, float* y, int ldy, int n_img, int h, int w_, int cin,
                                int cout, void* stream) {
    RUNET_REQUIRE(x && wq && y, "null pointer");
    RUNET_REQUIRE(cin > 0 && cin % 4 == 0 && cout > 0 && cout % 4 == 0, "channel counts must be multiples of 4");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty shape");
    RUNET_REQUIRE(ldx >= cin && ldy >= cout, "bad pixel strides");
    RUNET_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)wq % 16) == 0 && ((uintptr_t)y % 16) == 0, "alignment");
    static const int first_tap[4] = {0, 1, 3, 5};
    for (int cls = 0; cls < 4; ++cls) {
        IGemmArgs a = igemm_operands(x, ldx, wq + (long)first_tap[cls] * cin * cout, bias, y, ldy, n_img, cin, cin, cout, 0);
        weights_n_contig(a);
        const int gz = geom_convt3_class(a, h, w_, cls >> 1, cls & 1);
        dispatch_igemm(a, gz, (hipStream_t)stream);
    }
    RUNET_CHECK_LAUNCH();
}

extern "C" long runet_conv_wgrad_rect_workspace_floats(int pixels, int cin_w, int cout, int kh, int kw) {
    if (pixels <= 0 || cin_w <= 0 || cout <= 0 || kh < 1 || kh > 8 || kw < 1 || kw > 8) return -1;
    return wgrad_workspace(pixels, cin_w, cout, kh * kw);
}

extern "C" int runet_conv_wgrad_rect(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats,
                                     int n_img, int hin, int win, int cin, int cin_w, int cout, int kh, int kw, int stride, int pad_h, int pad_w,
                                     int dil_h, int dil_w, void* stream) {
    RUNET_REQUIRE(x && dy && dw, "null pointer");
    RUNET_REQUIRE(cin > 0 && cin % 4 == 0 && cin_w > 0 && cin_w <= cin && cout > 0 && cout % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ldx >= cin &&
                      ldy >= cout,
                  "channel counts / strides must be multiples of 4");
    RUNET_REQUIRE(kh >= 1 && kh <= 8 && kw >= 1 && kw <= 8 && stride >= 1 && stride <= 8 && pad_h >= 0 && pad_w >= 0 && dil_h >= 1 && dil_w >= 1,
                  "unsupported geometry");
    RUNET_REQUIRE(n_img > 0 && hin > 0 && win > 0, "empty shape");
    RUNET_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)dy % 16) == 0 && ((uintptr_t)dw % 16) == 0 && ((uintptr_t)workspace % 16) == 0, "alignment");
    const int ho = (hin + 2 * pad_h - dil_h * (kh - 1) - 1) / stride + 1, wo = (win + 2 * pad_w - dil_w * (kw - 1) - 1) / stride + 1;
    RUNET_REQUIRE(hin + 2 * pad_h - dil_h * (kh - 1) > 0 && win + 2 * pad_w - dil_w * (kw - 1) > 0 && ho > 0 && wo > 0, "empty output");
    WGradArgs a = wgrad_operands(x, ldx, dy, ldy, n_img, cin, cin_w, cout);
    const long P = wgrad_geom_conv(a, {hin, win, ho, wo, kh, kw, stride, pad_h, pad_w, dil_h, dil_w});
    launch_wgrad_splitk(a, P, cin_w, cout, kh * kw, dw, workspace, workspace_floats, (hipStream_t)stream);
    RUNET_CHECK_LAUNCH();
}


// ---------------------------------------------------------------------------------------------------------------------------
// Batched plain GEMMs on the same kernels (the 36 position-GEMMs of the unfused Winograd F(4x4,3x3) path, conv_winograd4.hip).
//   runet_gemm_batched   : C[z][rows][n] = A[z][rows][k] . B[z][k][n]                (blockIdx.z = z)
//   runet_gemm_tn_batched: C[split][z][k][n] = sum over the split's rows of A[z][row][k] * B[z][row][n];  splits = ceil(rows / rows_per_split)
// what runet_gemm_batched launches for a shape: an igemm tile variant, or GEMM_NN = gemm.hip's gemm_nn_kernel
constexpr int GEMM_NN = 5;
static int gemm_batched_route(int batch, int rows, int n) {
    const long b128 = (long)cdiv(rows, 128) * cdiv(n, 128) * batch;
    // 128x64 tiles where 128x128 tiles would fill the 256 CUs unevenly (e.g. 576 blocks = 2.25 per CU -> 3 rounds for 2.25 of work)
    const double per_cu = b128 / 256.0, bal = per_cu / (double)((b128 + 255) / 256);
    if (bal < 0.8 && n % 64 == 0) return V_128x64;
    if (n >= 96) return GEMM_NN;
    if (n > 32 && (long)cdiv(rows, 128) * cdiv(n, 64) * batch >= 256) return V_128x64;
    if (n > 32) return V_64x64;
    return V_128x32;
}

// which device kernel runet_gemm_batched launches for a shape (live profiling labels must match the rocprofv3 kernel names).  `fast` is the
// last template argument of either kernel; for the igemm it is what igemm_route finds for these operands, RUNET_IGEMM_GENERAL aside.
extern "C" const char* runet_gemm_batched_kernel_name(int batch, int rows, int k, int n) {
    const bool fast = k % 16 == 0 && k >= 16 && n >= 4;
    const int route = gemm_batched_route(batch, rows, n);
    if (route == GEMM_NN) return fast ? "gemm_nn_kernel<16, true>" : "gemm_nn_kernel<16, false>";
    return IGEMM_NAMES[0][fast][route];
}

extern "C" int runet_gemm_batched(const float* a, int lda, long stride_a, const float* b, long stride_b, float* c, int ldc, long stride_c,
                                  int batch, int rows, int k, int n, void* stream) {
    RUNET_REQUIRE(a && b && c && batch > 0 && batch <= 65535 && rows > 0, "bad arguments");
    RUNET_REQUIRE(k > 0 && k % 4 == 0 && n > 0 && n % 4 == 0 && lda >= k && lda % 4 == 0 && ldc >= n && ldc % 4 == 0, "k, n and the row strides must be multiples of 4");
    RUNET_REQUIRE(((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0 && ((uintptr_t)c % 16) == 0 && stride_a % 4 == 0 && stride_b % 4 == 0 && stride_c % 4 == 0,
                  "alignment");
    hipStream_t st = (hipStream_t)stream;
    const int route = gemm_batched_route(batch, rows, n);
    if (route == GEMM_NN) {
        runet_gemm_nn_launch(a, lda, stride_a, b, stride_b, c, ldc, stride_c, batch, rows, k, n, st);
        RUNET_CHECK_LAUNCH();
    }
    IGemmArgs g = igemm_operands(a, lda, b, nullptr, c, ldc, 1, k, k, n, 0);
    weights_n_contig(g);
    const int gz = geom_gemm_batch(g, rows, batch, stride_a, stride_b, stride_c);
    IGemmRoute r = igemm_route(g);      // for the loader; the tile is this function's own choice
    r.variant = (IGemmVariant)route;
    launch_route(g, r, gz, st);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_gemm_tn_batched(const float* a, int lda, long stride_a, const float* b, int ldb, long stride_b, float* c, int batch, int rows,
                                     int k, int n, int rows_per_split, void* stream) {
    RUNET_REQUIRE(a && b && c && batch > 0 && batch <= 65535 && rows > 0 && rows_per_split > 0 && rows_per_split % 16 == 0, "bad arguments (rows_per_split: multiple of 16)");
    const int splits = cdiv(rows, rows_per_split);
    RUNET_REQUIRE(splits <= 65535, "too many splits");
    RUNET_REQUIRE(k > 0 && k % 4 == 0 && n > 0 && n % 4 == 0 && lda >= k && lda % 4 == 0 && ldb >= n && ldb % 4 == 0, "k, n and the row strides must be multiples of 4");
    RUNET_REQUIRE(((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0 && ((uintptr_t)c % 16) == 0 && stride_a % 4 == 0 && stride_b % 4 == 0, "alignment");
    hipStream_t st = (hipStream_t)stream;
    if (k > 64 && n > 64) {                  // gemm.hip's 128 x 128 LDS-ring kernel where both sides fill more than half a tile
        runet_gemm_tn_launch(a, lda, stride_a, b, ldb, stride_b, c, batch, rows, k, n, rows_per_split, st);
        RUNET_CHECK_LAUNCH();
    }
    // the batch rides on the tap axis: "tap" t reads a + t stride_a and b + t stride_b, no spatial shift
    WGradArgs g = wgrad_operands(a, lda, b, ldb, 1, k, k, n);
    g.out = c;
    g.H = 1; g.W = rows; g.Hin = 1; g.Win = rows; g.a_scale = 1; g.KH = batch; g.KW = 1; g.Hout = 1; g.Wout = rows; g.o_scale = 1;
    g.tap_bs_x = stride_a; g.tap_bs_dy = stride_b;
    g.pix_per_split = rows_per_split;
    launch_wgrad_tiles(g, false, k, n, batch, splits, st);
    RUNET_CHECK_LAUNCH();
}

