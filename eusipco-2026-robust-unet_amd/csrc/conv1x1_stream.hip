// Streaming, weight-resident 1x1 convolution (forward and data gradient) for the narrow layers: cin, cout <= 128.
//
// Those launches are bound by streaming their activations, and the tiled implicit GEMM (conv_igemm.hip) runs a very short k-loop per
// block: two to eight LDS-ring steps with a block barrier each, then the `+=` read-modify-write only after the last MFMA.  Here a fixed
// number of persistent blocks (chosen from the CU count) each load the whole weight matrix ONCE into LDS, already in B-fragment order;
// after that prologue there is no block barrier.  A wave owns tiles of 32 pixels x all cout columns (cout / 32 accumulator tiles) and
// walks the pixel tiles with the grid's wave count as stride.  A fragments come straight from global memory into registers (lane (i, h)
// holds 4 consecutive channels of row i per 8-channel group, exactly the elements the implicit GEMM's ds_read_b128 hands it), double
// buffered: the loads of tile t+1 are issued before the MFMAs of tile t.  For `+=` the old destination values of tile t+1 are requested
// right after the stores of tile t, so they fly during the MFMAs of tile t+1.
//
// Bit identity with igemm_kernel: every output element is one fp32 chain on v_mfma_f32_32x32x2_f32 that starts from 0 and takes, per
// 16-channel chunk kc, per half kh and per q = 0..3, the channel pair (16 kc + 8 kh + q, 16 kc + 8 kh + 4 + q) from lane halves 0 / 1 - the
// order of igemm_kernel's loop (conv_igemm.hip, `af[kh][a][q]`) - and the value stored is acc + bias + old in that association.
#include "runet_common.h"
#include <stdlib.h>
#include "../../include/runet_hip.h"

namespace {

struct StreamArgs {
    const float* x; int ldx;
    const float* w; int w_sk, w_sn;      // B(k, n) = w[k * w_sk + n * w_sn]
    const float* bias;
    float* y; int ldy;
    long P;                              // pixels
    long ntiles;                         // ceil(P / 32)
    int cout, accumulate;
};

// KC = cin / 16, TN = ceil(cout / 32), ACC: y += result.  Registers: 2 x 8 KC (A, double buffered) + 16 TN (accumulators) + 16 TN (old
// values, ACC only) + 16 row offsets + addressing; two blocks per CU while that fits 256, else one (128 -> 97..128 channels).
template <int KC, int TN>
constexpr int stream_min_blocks() { return (16 * KC + 32 * TN <= 200) ? 2 : 1; }

template <int KC, int TN, bool ACC>
__global__ __launch_bounds__(256, (stream_min_blocks<KC, TN>())) void conv1x1_stream_kernel(StreamArgs g) {
    constexpr int NC = 2 * KC;           // 8-channel groups
    extern __shared__ __attribute__((aligned(16))) float wl[];      // [NC][TN][64 lanes][4]: lane (li, lh), q -> B(8 c + 4 lh + q, 32 b + li)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform, and known to be
    const int li = lane & 31, lh = lane >> 5;
    const int cin = 16 * KC;

    float bv[TN];
#pragma unroll
    for (int b = 0; b < TN; ++b) bv[b] = (g.bias != nullptr && b * 32 + li < g.cout) ? g.bias[b * 32 + li] : 0.f;
    const bool last_ok = (TN - 1) * 32 + li < g.cout;      // only the last 32-column tile can reach beyond cout

    // Wave-uniform tile arithmetic stays on the scalar unit: a tile's base pointers are SGPR pairs, the lane part of every address is a
    // 32-bit offset that does not change from tile to tile (only the ragged last tile clamps its A rows).  The destination goes through a
    // buffer descriptor made per tile that ends with the tile's last valid row: rows beyond the problem fall outside it (their loads give 0,
    // their stores are dropped), so the tile loop has no per-row branch.  Every tile issues the same loads - past the end a wave loads the
    // last tile again and drops it - so that the waits in the loop are counted ones on every path.
    const long nwaves = (long)gridDim.x * 4;
    const long t_last = g.ntiles - 1;
    const unsigned ldy4 = (unsigned)g.ldy * 4u;
    const unsigned y_lane4 = (unsigned)(4 * lh) * ldy4 + (unsigned)li * 4u;      // lane holds column li of each 32-column tile, rows (r & 3) + 8 (r >> 2) + 4 lh

    auto rows_of = [&](long t) -> int {      // rows of tile t inside the problem (32 except for the last tile)
        const long left = g.P - t * 32;
        return left < 32 ? (int)left : 32;
    };
    auto y_rsrc = [&](long t) {
        const int rows = rows_of(t);
        return __builtin_amdgcn_make_buffer_rsrc(g.y + t * 32 * g.ldy, 0, (int)(((unsigned)(rows - 1) * (unsigned)g.ldy + (unsigned)g.cout) * 4u), 0x00020000);
    };
    auto load_a = [&](f32x4 (&a)[NC], long t) {
        const int rows = rows_of(t);
        const int row = li < rows ? li : rows - 1;      // rows beyond the problem read the tile's last pixel: their products are never stored
        const float* ab = g.x + t * 32 * g.ldx;
        const unsigned off = (unsigned)row * (unsigned)g.ldx + (unsigned)(4 * lh);
#pragma unroll
        for (int c = 0; c < NC; ++c) a[c] = ld4(ab + (off + 8u * c));
    };
    // columns beyond cout (last 32-column tile) read what lies there inside the descriptor, or 0: those lanes store nothing
    auto load_old = [&](float (&old)[TN][16], long t) {
        const __amdgpu_buffer_rsrc_t ry = y_rsrc(t);
        int yl = (int)y_lane4;
        asm volatile("" : "+v"(yl));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int vo = yl + ((r & 3) + 8 * (r >> 2)) * (int)ldy4;
#pragma unroll
            for (int b = 0; b < TN; ++b) old[b][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, vo + 128 * b, 0, 0));
        }
    };

    float old[TN][16];
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) old[b][r] = 0.f;

    // one tile: a_cur holds tile t, a_nxt receives tile t + nwaves
    auto step = [&](f32x4 (&a_cur)[NC], f32x4 (&a_nxt)[NC], long t) {
        const long tn = t + nwaves < t_last ? t + nwaves : t_last;
        load_a(a_nxt, tn);
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc[TN];
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
        // the B fragments do not change from tile to tile, and the compiler would hoist all cin x cout / 64 registers of them out of the
        // tile loop: the lane's LDS offset is made opaque once per tile so that they are read again where they are used (the same
        // for the lane's destination offset below: hoisted, each (row, column tile) pair would keep an offset register of its own)
        int wl_lane = lane;
        asm volatile("" : "+v"(wl_lane));
        const int wlane = wl_lane * 4;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            f32x4 bf[TN];
#pragma unroll
            for (int b = 0; b < TN; ++b) bf[b] = *reinterpret_cast<const f32x4*>(wl + (c * TN + b) * 256 + wlane);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int b = 0; b < TN; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[c][q], bf[b][q], acc[b], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);      // phases stay apart: interleaving the stores' adds with the MFMAs costs registers
        const __amdgpu_buffer_rsrc_t ry = y_rsrc(t);
        int yl = (int)y_lane4;
        asm volatile("" : "+v"(yl));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int vo = yl + ((r & 3) + 8 * (r >> 2)) * (int)ldy4;
#pragma unroll
            for (int b = 0; b < TN - 1; ++b)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc[b][r] + bv[b] + old[b][r]), ry, vo + 128 * b, 0, 0);
        }
        if (last_ok) {
            constexpr int b = TN - 1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int vo = yl + ((r & 3) + 8 * (r >> 2)) * (int)ldy4;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc[b][r] + bv[b] + old[b][r]), ry, vo + 128 * b, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ACC) load_old(old, tn);
    };

    // the first tile's loads fly while the block fills LDS (a wave without a tile loads the last one and drops it)
    long t = (long)blockIdx.x * 4 + wid;
    f32x4 a0[NC], a1[NC];
    {
        const long t0 = t < t_last ? t : t_last;
        load_a(a0, t0);
        if constexpr (ACC) load_old(old, t0);
    }
    // ---- prologue: the weight matrix into LDS, read in its memory order (coalesced either way), zero beyond cout ----
    if (g.cout < 32 * TN) {
        for (int e = tid; e < NC * TN * 256; e += 256) wl[e] = 0.f;
        lds_barrier();
    }
    {
        // 16-byte loads, up to four in flight per thread before the first LDS write: one load -> wait -> write per element made this
        // fill a chain of 32..64 memory latencies, a third of a 60 us launch
        constexpr int MAXV = (KC * TN + 1) / 2;      // float4s per thread at cout = 32 TN
        const int total4 = cin * g.cout / 4;
        const bool ncontig = g.w_sn == 1;
        const int cq = g.cout >> 2;                  // float4s per weight row when cout is contiguous
        auto widx = [&](int k, int n) { return (((k >> 3) * TN + (n >> 5)) * 64 + ((k >> 2) & 1) * 32 + (n & 31)) * 4 + (k & 3); };
#pragma unroll
        for (int i0 = 0; i0 < MAXV; i0 += 4) {
            f32x4 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e4 = tid + 256 * (i0 + j);
                if (i0 + j < MAXV && e4 < total4) v[j] = ld4(g.w + 4 * (long)e4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e4 = tid + 256 * (i0 + j);
                if (i0 + j < MAXV && e4 < total4) {
                    if (ncontig) {                   // w [cin][cout]: four columns of one row (cout % 4 == 0: inside one 32-column tile)
                        const int k = e4 / cq, n = (e4 - k * cq) * 4;
#pragma unroll
                        for (int q = 0; q < 4; ++q) wl[widx(k, n + q)] = v[j][q];
                    } else {                         // w [cout][cin]: four consecutive channels of one column = one fragment quad
                        const int n = e4 / (cin / 4), k = (e4 - n * (cin / 4)) * 4;
                        st4(wl + widx(k, n), v[j]);
                    }
                }
            }
        }
    }
    lds_barrier();
    if (t >= g.ntiles) return;
    for (;;) {
        step(a0, a1, t);
        t += nwaves;
        if (t >= g.ntiles) break;
        step(a1, a0, t);
        t += nwaves;
        if (t >= g.ntiles) break;
    }
}

template <int KC, int TN>
void launch_stream(const StreamArgs& a, int blocks, hipStream_t st) {
    const size_t lds = (size_t)2 * KC * TN * 256 * sizeof(float);
    if (a.accumulate) hipLaunchKernelGGL((conv1x1_stream_kernel<KC, TN, true>), dim3(blocks), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((conv1x1_stream_kernel<KC, TN, false>), dim3(blocks), dim3(256), lds, st, a);
}

template <int KC>
void dispatch_tn(const StreamArgs& a, int blocks, hipStream_t st) {
    switch ((a.cout + 31) / 32) {
    case 1: launch_stream<KC, 1>(a, blocks, st); break;
    case 2: launch_stream<KC, 2>(a, blocks, st); break;
    case 3: launch_stream<KC, 3>(a, blocks, st); break;
    default: launch_stream<KC, 4>(a, blocks, st); break;
    }
}

int stream_cu_count() {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        return n;
    }();
    return cus;
}

bool stream_shape_ok(int cin, int cout, int mode) {
    return (mode == RUNET_CONV_FWD || mode == RUNET_CONV_DGRAD) && cin >= 16 && cin <= 128 && cin % 16 == 0 && cout >= 4 && cout <= 128 && cout % 4 == 0;
}

}  // namespace

extern "C" int runet_conv1x1_stream_supported(int cin, int cout, int mode) { return stream_shape_ok(cin, cout, mode) ? 1 : 0; }

extern "C" int runet_conv1x1_stream_blocks(int n_img, int h, int w_, int cin, int cout) {
    if (n_img <= 0 || h <= 0 || w_ <= 0 || cin <= 0 || cout <= 0) return 0;
    // measurement knob, read at call time: RUNET_CONV1X1_STREAM_BLOCKS = number of persistent blocks
    const char* e = getenv("RUNET_CONV1X1_STREAM_BLOCKS");
    const int forced = e ? atoi(e) : 0;
    if (forced > 0) return forced < 65535 ? forced : 65535;
    const int per_cu = (cin + (cout + 31) / 32 * 32 <= 200) ? 2 : 1;            // stream_min_blocks
    const long tiles = ((long)n_img * h * w_ + 31) / 32;
    long blocks = (long)stream_cu_count() * per_cu;
    const long need = (tiles + 3) / 4;                                           // four wave tiles per block
    if (blocks > need) blocks = need;
    return (int)(blocks < 1 ? 1 : blocks);
}

extern "C" const char* runet_conv1x1_stream_kernel_name(int cin, int cout, int accumulate) {
    static thread_local char name[64];
    snprintf(name, sizeof(name), "conv1x1_stream_kernel<%d, %d, %s>", cin / 16, (cout + 31) / 32, accumulate ? "true" : "false");
    return name;
}

extern "C" int runet_conv1x1_stream(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int n_img, int h, int w_,
                                    int cin, int cout, int mode, int accumulate, void* stream) {
    RUNET_REQUIRE(x && w && y, "null pointer");
    RUNET_REQUIRE(stream_shape_ok(cin, cout, mode), "needs mode FWD or DGRAD, cin a multiple of 16 and cout a multiple of 4, both <= 128");
    RUNET_REQUIRE(ldx >= cin && ldx % 4 == 0 && ldy >= cout && ldy % 4 == 0, "pixel strides must be multiples of 4 floats and cover the channels");
    RUNET_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)w % 16) == 0 && ((uintptr_t)y % 16) == 0, "pointers must be 16-byte aligned");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty iteration space");
    StreamArgs a{};
    a.x = x; a.ldx = ldx; a.w = w; a.bias = bias; a.y = y; a.ldy = ldy;
    a.P = (long)n_img * h * w_;
    a.ntiles = (a.P + 31) / 32;
    a.cout = cout; a.accumulate = accumulate != 0;
    if (mode == RUNET_CONV_FWD) { a.w_sk = cout; a.w_sn = 1; }      // w [cin][cout]
    else { a.w_sk = 1; a.w_sn = cin; }                              // the forward weight [cout (conv Cin)][cin (conv Cout)], read transposed
    const int blocks = runet_conv1x1_stream_blocks(n_img, h, w_, cin, cout);
    hipStream_t st = (hipStream_t)stream;
    switch (cin / 16) {
    case 1: dispatch_tn<1>(a, blocks, st); break;
    case 2: dispatch_tn<2>(a, blocks, st); break;
    case 3: dispatch_tn<3>(a, blocks, st); break;
    case 4: dispatch_tn<4>(a, blocks, st); break;
    case 5: dispatch_tn<5>(a, blocks, st); break;
    case 6: dispatch_tn<6>(a, blocks, st); break;
    case 7: dispatch_tn<7>(a, blocks, st); break;
    default: dispatch_tn<8>(a, blocks, st); break;
    }
    RUNET_CHECK_LAUNCH();
}


// ------------------------------------------------------------------------------------------ weight gradient of the narrow 1x1 layers
// dW[ci][co] = sum_p x[p][ci] * dy[p][co] with the pixel as the MFMA contraction.  A wave streams a contiguous pixel range with the whole
// cin x cout result in its accumulators: per MFMA step (two pixels, one per lane half) a lane loads cin / 32 consecutive channels of x and
// cout / 32 of dy with one 4-, 8- or 16-byte load each - rows are read whole and coalesced, nothing goes through LDS, and the only address
// arithmetic per load is one multiply-add (wgrad_tile_kernel recomputes image / row / column per tile).  Lane i's VA channels are rows of VA
// different accumulator tiles: tile (qa, qb) holds dW[VA i + qa][VB j + qb].  Pixels beyond the wave's range load a clamped address and
// are zeroed by a select, so every batch issues the same loads (counted waits).  The four waves of a
// block are summed through LDS in wave order into one slab; wgrad_slab_sum_kernel adds the slabs in a fixed order.  The slab count and
// the pixels per wave come from the shape alone (wgrad_stream_plan), so the bits do not depend on the device or on timing.
namespace {

struct WgStreamArgs {
    const float* x; int ldx;
    const float* dy; int ldy;
    float* slabs;                 // [gridDim.x][cin][cout]
    long P, chunk;                // pixels, pixels per wave (multiple of 16)
    int cin, cout;
};

// V consecutive channels of pixel q of the wave's range (V = 1, 2, 4: one 4-, 8- or 16-byte load); pixels beyond the range read the
// last one of the range (a valid address) - every batch issues the same loads - and are zeroed where they are used (wg_zero)
template <int V>
__device__ __forceinline__ void wg_load(float (&v)[V], const float* base, int ld, int q, int np) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const int qc = q < np ? q : (np > 0 ? np - 1 : 0);
    const float* p = base + (long)qc * ld;
    if constexpr (V == 1) {
        v[0] = *p;
    } else if constexpr (V == 2) {
        const f32x2 t = *reinterpret_cast<const f32x2*>(p);
        v[0] = t[0]; v[1] = t[1];
    } else {
        const f32x4 t = ld4(p);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = t[e];
    }
}

// VA = cin / 32, VB = cout / 32.  Registers: 16 VA VB accumulators + 2 x S (VA + VB) staged operands; no LDS until the final sum.
// At most 256 blocks are launched (one per CU) and the launch bounds keep a wave inside 256 registers, so that a block of the main
// stream's kernels still fits beside it: a side-stream kernel costs the step its footprint.
// TR: the launcher swapped the tensors (x = the layer's dy, dy = the layer's x, cin / cout likewise) so that the wider one is the A side
// (VA >= VB keeps the operand registers low); the result is then written transposed, dW[B-side channel][A-side channel].
template <int VA, int VB, bool TR>
__global__ __launch_bounds__(256, 2) void conv1x1_wgrad_stream_kernel(WgStreamArgs g) {
    constexpr int S = VA * VB >= 8 ? 4 : 8;      // MFMA steps (pixel pairs) per batch (the 128-wide pairs: 4, to stay inside 256 registers)
    extern __shared__ __attribute__((aligned(16))) float red[];      // [cin][cout], used after the pixel loop only
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;

    const long p0 = ((long)blockIdx.x * 4 + wid) * g.chunk;
    long np = g.P - p0;
    np = np < g.chunk ? np : g.chunk;
    np = np > 0 ? np : 0;
    const long pb = np > 0 ? p0 : 0;
    const int npi = (int)np;
    const float* xl = g.x + pb * g.ldx + VA * li;      // the lane's channels of the range's first pixel
    const float* yl = g.dy + pb * g.ldy + VB * li;
    const int nb = (int)((np + 2 * S - 1) / (2 * S));

    f32x16 acc[VA][VB];
#pragma unroll
    for (int a = 0; a < VA; ++a)
#pragma unroll
        for (int b = 0; b < VB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    auto load_batch = [&](float (&A)[S][VA], float (&B)[S][VB], int bi) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            wg_load<VA>(A[s], xl, g.ldx, bi * 2 * S + 2 * s + lh, npi);
            wg_load<VB>(B[s], yl, g.ldy, bi * 2 * S + 2 * s + lh, npi);
        }
    };
    // x of a pixel beyond the range counts as 0 (a select at the use: at the load it would wait for the data there)
    auto mma_batch = [&](float (&A)[S][VA], float (&B)[S][VB], int bi) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const bool ok = bi * 2 * S + 2 * s + lh < npi;
#pragma unroll
            for (int a = 0; a < VA; ++a) {
                const float av = ok ? A[s][a] : 0.f;
#pragma unroll
                for (int b = 0; b < VB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ok ? B[s][b] : 0.f, acc[a][b], 0, 0, 0);
            }
        }
    };

    // the scheduler is kept from sinking a batch's loads below the MFMAs that hide them
    float A0[S][VA], B0[S][VB], A1[S][VA], B1[S][VB];
    load_batch(A0, B0, 0);                    // past the range: zeros
    for (int bi = 0; bi < nb; bi += 2) {
        load_batch(A1, B1, bi + 1);
        __builtin_amdgcn_sched_barrier(0);
        mma_batch(A0, B0, bi);
        __builtin_amdgcn_sched_barrier(0);
        load_batch(A0, B0, bi + 2);
        __builtin_amdgcn_sched_barrier(0);
        mma_batch(A1, B1, bi + 1);            // a batch past the range adds zeros
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- the block's four partial results, added in wave order through LDS, then one slab ----
    constexpr int CA = 32 * VA, CB = 32 * VB, n_out = CA * CB;
    float* rl = red + (VA * 4 * lh) * CB + VB * li;      // [A-side channel][B-side channel]: element (a, b, r) at a compile-time offset from here
    auto to_lds = [&](bool first) {
#pragma unroll
        for (int a = 0; a < VA; ++a)
#pragma unroll
            for (int b = 0; b < VB; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float* o = rl + (VA * ((r & 3) + 8 * (r >> 2)) + a) * CB + b;
                    *o = first ? acc[a][b][r] : *o + acc[a][b][r];
                }
    };
    if (wid == 0) to_lds(true);
    lds_barrier();
#pragma unroll 1
    for (int wv = 1; wv < 4; ++wv) {
        if (wid == wv) to_lds(false);
        lds_barrier();
    }
    float* slab = g.slabs + (long)blockIdx.x * n_out;
    if constexpr (!TR) {
        for (int e = tid * 4; e < n_out; e += 1024) st4(slab + e, ld4(red + e));
    } else {      // dW[B-side channel][A-side channel]: transposed on the way out (strided LDS reads, coalesced stores; once per block)
        for (int e = tid; e < n_out; e += 256) slab[e] = red[(e % CA) * CB + e / CA];
    }
}

// out[i] = sum_k slabs[k][i], i < n (n % 4 == 0): eight lanes take the slabs k = lane, lane + 8, ... in that order, then the lane sums
// are added in lane order - the order of conv_igemm.hip's slab_reduce_kernel, but in double with one rounding at the end (as sum_parts_kernel)
__global__ __launch_bounds__(256) void wgrad_slab_sum_kernel(const float* __restrict__ slabs, int nslabs, int n, float* __restrict__ out) {
    __shared__ double part[256][4];
    const int col = threadIdx.x & 31, kl = threadIdx.x >> 5;
    const long i = ((long)blockIdx.x * 32 + col) * 4;
    double s[4] = {0., 0., 0., 0.};
    if (i < n)
        for (int k = kl; k < nslabs; k += 8) {
            const f32x4 v = ld4(slabs + (long)k * n + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += v[e];
        }
#pragma unroll
    for (int e = 0; e < 4; ++e) part[threadIdx.x][e] = s[e];
    __syncthreads();
    if (kl == 0 && i < n) {
#pragma unroll
        for (int j = 1; j < 8; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += part[j * 32 + col][e];
        const f32x4 r = {(float)s[0], (float)s[1], (float)s[2], (float)s[3]};
        st4(out + i, r);
    }
}

bool wgrad_stream_shape_ok(int cin, int cout) {
    auto w = [](int c) { return c == 32 || c == 64 || c == 128; };
    return w(cin) && w(cout) && (cin < 128 || cout < 128);      // 128 x 128 is the TN GEMM's
}

// slabs (= blocks of four waves) and pixels per wave, from the pixel count alone: a block per 256 pixels, at most 256 blocks (one per CU
// of the chip this was written for; the count does not follow the device, so the bits do not either)
void wgrad_stream_plan(long P, int& slabs, long& chunk) {
    long b = (P + 255) / 256;
    b = b < 1 ? 1 : (b > 256 ? 256 : b);
    slabs = (int)b;
    chunk = ((P + b * 4 - 1) / (b * 4) + 15) / 16 * 16;
}

template <int VA, int VB, bool TR>
void wg_launch(const WgStreamArgs& a, int blocks, hipStream_t st) {
    hipLaunchKernelGGL((conv1x1_wgrad_stream_kernel<VA, VB, TR>), dim3(blocks), dim3(256), (size_t)a.cin * a.cout * sizeof(float), st, a);
}

// a.cin >= a.cout here (the launcher swapped the sides otherwise)
template <bool TR>
void wg_dispatch(const WgStreamArgs& a, int blocks, hipStream_t st) {
    const int va = a.cin / 32, vb = a.cout / 32;
    if (va == 1) wg_launch<1, 1, TR>(a, blocks, st);
    else if (va == 2 && vb == 1) wg_launch<2, 1, TR>(a, blocks, st);
    else if (va == 2) wg_launch<2, 2, TR>(a, blocks, st);
    else if (vb == 1) wg_launch<4, 1, TR>(a, blocks, st);
    else wg_launch<4, 2, TR>(a, blocks, st);      // 128 x 128 is refused by the entry point
}

}  // namespace

extern "C" int runet_conv1x1_wgrad_stream_supported(int cin, int cout) { return wgrad_stream_shape_ok(cin, cout) ? 1 : 0; }

extern "C" int runet_conv1x1_wgrad_stream_slabs(int n_img, int h, int w_) {
    if (n_img <= 0 || h <= 0 || w_ <= 0) return 0;
    int slabs; long chunk;
    wgrad_stream_plan((long)n_img * h * w_, slabs, chunk);
    return slabs;
}

extern "C" long runet_conv1x1_wgrad_stream_workspace_floats(int n_img, int h, int w_, int cin, int cout) {
    if (cin <= 0 || cout <= 0) return 0;
    return (long)runet_conv1x1_wgrad_stream_slabs(n_img, h, w_) * cin * cout;
}

extern "C" int runet_conv1x1_wgrad_stream(const float* x, int ldx, const float* dy, int ldy, float* dw, float* workspace, long workspace_floats,
                                          int n_img, int h, int w_, int cin, int cout, void* stream) {
    RUNET_REQUIRE(x && dy && dw && workspace, "null pointer");
    RUNET_REQUIRE(wgrad_stream_shape_ok(cin, cout), "needs cin and cout of 32, 64 or 128, not both 128");
    RUNET_REQUIRE(ldx >= cin && ldx % 4 == 0 && ldy >= cout && ldy % 4 == 0, "pixel strides must be multiples of 4 floats and cover the channels");
    RUNET_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)dy % 16) == 0 && ((uintptr_t)dw % 16) == 0 && ((uintptr_t)workspace % 16) == 0,
                  "pointers must be 16-byte aligned");
    RUNET_REQUIRE(n_img > 0 && h > 0 && w_ > 0, "empty iteration space");
    WgStreamArgs a{};
    a.x = x; a.ldx = ldx; a.dy = dy; a.ldy = ldy; a.slabs = workspace; a.cin = cin; a.cout = cout;
    a.P = (long)n_img * h * w_;
    int slabs;
    wgrad_stream_plan(a.P, slabs, a.chunk);
    RUNET_REQUIRE(workspace_floats >= (long)slabs * cin * cout, "workspace too small (runet_conv1x1_wgrad_stream_workspace_floats)");
    RUNET_REQUIRE(a.chunk < (1L << 30), "a wave's pixel range exceeds 32-bit pixel indices");
    hipStream_t st = (hipStream_t)stream;
    if (cout > cin) {      // the wider tensor on the A side, the result written transposed
        a.x = dy; a.ldx = ldy; a.dy = x; a.ldy = ldx; a.cin = cout; a.cout = cin;
        wg_dispatch<true>(a, slabs, st);
    } else {
        wg_dispatch<false>(a, slabs, st);
    }
    hipLaunchKernelGGL(wgrad_slab_sum_kernel, dim3(cdiv(cin * cout, 128)), dim3(256), 0, st, workspace, slabs, cin * cout, dw);
    RUNET_CHECK_LAUNCH();
}
