// Connected-component labelling of a batch of byte masks, and what rests on it: component areas and frame contact, the area filter behind
// clean_water_mask, and the table of water bodies (components.py; include/runet_hip.h states the rules, tests/ccl_ref.py restates them).
//
// A component's label is 1 + the smallest linear index y * w + x among its pixels, so the result is defined exactly and every merge below is
// an integer minimum: whatever order the blocks and waves run in, the bytes are the same.
//
// Three plain launches.  (1) A block labels one 64 x 64 tile in LDS.  The tile is as wide as a wave, so a wave's ballot is a row's feature
// bits: every pixel starts at the first pixel of its horizontal run, and only the vertical (and, under 8-connectivity, diagonal) contacts
// between runs of adjacent rows are left to unite, one union per contact.  The tile's pixels then take the global index of their tile-local
// root.  (2) A thread per pixel of every tile border row and column unites it with its neighbours across the border, the diagonal pairs
// at tile corners included.  (3) Every pixel walks to its root.
//
// The forest: labels[p] - 1 is the parent of pixel p, a pixel of the same component with an index <= p; a root is its own parent.  Parents
// only ever decrease (atomicMin), so find() descends and ends at a pixel that was a root when it was read; union() retries from what
// atomicMin returned, which is again smaller.  No loop waits for another workgroup: each ends after at most (index) steps whatever the
// others do.  The seam pass reads parents with agent-scope relaxed atomic loads, so a read is never older than the L2's value; even a stale
// parent would only be an ancestor that has since been re-parented, and the atomicMin on it returns the newer parent to continue from.
#include "runet_common.h"
#include "../../include/runet_hip.h"

#include <limits.h>

namespace {
constexpr int T = 64;                                    // tile side = the wave width
constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int CHUNK = 4 * TPB;                           // filter, table: consecutive pixels per block
constexpr int AREA_ROUNDS = 16;                          // areas: a wave counts 16 x 64 consecutive pixels
constexpr int AREA_CHUNK = WAVES * AREA_ROUNDS * 64;
constexpr int MAX_SIDE = 32768;                          // h * w <= 2^30: index + 1 fits int32
constexpr long MAX_BLOCKS = 2147483647L;

// ---- the forest in LDS: lab[i] = the parent's tile-local index, -1 on a non-feature pixel ----
__device__ __forceinline__ int lds_parent(const int* lab, int a) { return __hip_atomic_load(lab + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(const int* lab, int a) {
    for (int p; (p = lds_parent(lab, a)) != a;) a = p;   // p < a
    return a;
}
__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
    for (;;) {                                           // a + b falls with every round
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;                                         // a had a parent already: that parent and b are still to be united
    }
}

// ---- the forest in memory: L[i] = the parent's index + 1 ----
__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// with path halving: a pixel on the way is handed to its grandparent, an ancestor like any other, again by a minimum
__device__ __forceinline__ int g_find(int* L, int a) {
    for (int p; (p = g_load(L + a) - 1) != a; a = p) {
        const int g = g_load(L + p) - 1;
        if (g != p) atomicMin(L + a, g + 1);
    }
    return a;
}
__device__ __forceinline__ void g_union(int* L, int a, int b) {
    for (;;) {
        a = g_find(L, a);
        b = g_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b + 1) - 1;
        if (old == a) return;
        a = old;
    }
}

// ---- stage 1: one tile ----
__global__ __launch_bounds__(TPB) void ccl_tile_kernel(const unsigned char* __restrict__ mask, int h, int w, long rs, long is, int invert, int conn8,
                                                        int tx, int ty, int* __restrict__ labels, int* __restrict__ tile_count) {
    __shared__ int lab[T * T];
    __shared__ unsigned long long bits[T];
    __shared__ int cnt[WAVES];
    const long blk = blockIdx.x;
    const int bx = (int)(blk % tx), by = (int)((blk / tx) % ty);
    const long img = blk / tx / ty;
    const int x0 = bx * T, y0 = by * T, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = x0 + lane;
    const unsigned char* src = mask + img * is;
    int* dst = labels + img * h * w;
    int c = 0;
    for (int r = wv; r < T; r += WAVES) {
        const int y = y0 + r;
        const bool f = y < h && x < w && ((src[(long)y * rs + x] != 0) != (invert != 0));
        const unsigned long long b = __ballot(f);
        if (lane == 0) bits[r] = b;
        const unsigned long long z = ~b & ((1ull << lane) - 1);                   // the non-features to my left
        lab[r * T + lane] = f ? r * T + (z ? 64 - __clzll((long long)z) : 0) : -1;
        c += __popcll(b);
    }
    if (lane == 0) cnt[wv] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[blk] = (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
    // One union per contact between a run and a run of the row above: the pixel whose left neighbour makes the same contact leaves it to
    // that neighbour, and a diagonal contact whose near pixel has a feature straight above is that pixel's.
    for (int r = wv ? wv : WAVES; r < T; r += WAVES) {
        const unsigned long long cur = bits[r], up = bits[r - 1];
        if (!((cur >> lane) & 1)) continue;
        const bool U = (up >> lane) & 1;
        const bool Lf = lane > 0 && ((cur >> (lane - 1)) & 1), UL = lane > 0 && ((up >> (lane - 1)) & 1);
        const bool Rf = lane < 63 && ((cur >> (lane + 1)) & 1), UR = lane < 63 && ((up >> (lane + 1)) & 1);
        const int me = r * T + lane, above = me - T;
        if (U) {
            if (!(Lf && UL)) lds_union(lab, me, above);
        } else if (conn8) {
            if (UL && !Lf) lds_union(lab, me, above - 1);
            if (UR && !Rf) lds_union(lab, me, above + 1);
        }
    }
    __syncthreads();
    for (int r = wv; r < T; r += WAVES) {
        const int y = y0 + r;
        if (y >= h || x >= w) continue;
        int v = 0;
        if ((bits[r] >> lane) & 1) {
            const int root = lds_find(lab, r * T + lane);
            v = (y0 + (root >> 6)) * w + x0 + (root & 63) + 1;
        }
        dst[(long)y * w + x] = v;
    }
}

// ---- stage 2: the tile borders ----
// Thread k of an image: first the pixels of the border columns x = 64, 128, ... (each against x - 1), then those of the border rows
// y = 64, 128, ... (each against y - 1).  A straight neighbour across the border stands for the diagonal ones next to it: they touch it
// inside their own tile, or across the other kind of border, whose own thread unites them.
__global__ __launch_bounds__(TPB) void ccl_seam_kernel(int* labels, int h, int w, int conn8, long per_image, long total) {
    const long id = (long)blockIdx.x * TPB + threadIdx.x;
    if (id >= total) return;
    const long img = id / per_image;
    long k = id - img * per_image;
    int* L = labels + img * h * w;
    const long nv = (long)((w - 1) / T) * h;
    if (k < nv) {
        const int s = (int)(k / h), y = (int)(k - (long)s * h), x = (s + 1) * T;
        const int p = y * w + x;
        if (g_load(L + p) == 0) return;
        if (g_load(L + p - 1) != 0) {
            g_union(L, p, p - 1);
        } else if (conn8) {
            if (y > 0 && g_load(L + p - w - 1) != 0) g_union(L, p, p - w - 1);
            if (y < h - 1 && g_load(L + p + w - 1) != 0) g_union(L, p, p + w - 1);
        }
    } else {
        k -= nv;
        const int s = (int)(k / w), x = (int)(k - (long)s * w), y = (s + 1) * T;
        const int p = y * w + x;
        if (g_load(L + p) == 0) return;
        if (g_load(L + p - w) != 0) {
            g_union(L, p, p - w);
        } else if (conn8) {
            if (x > 0 && g_load(L + p - w - 1) != 0) g_union(L, p, p - w - 1);
            if (x < w - 1 && g_load(L + p - w + 1) != 0) g_union(L, p, p - w + 1);
        }
    }
}

// ---- stage 3: every pixel takes its root ----
// Other blocks write roots into pixels of this walk's path meanwhile: such a pixel then holds either its old parent or its root, both
// ancestors, so the walk ends at the same root.  A root stays a root throughout this launch.
__global__ __launch_bounds__(TPB) void ccl_flatten_kernel(int* labels, int h, int w, int tx, int ty, const int* __restrict__ tile_count) {
    const long blk = blockIdx.x;
    if (tile_count[blk] == 0) return;
    const int bx = (int)(blk % tx), by = (int)((blk / tx) % ty);
    const long img = blk / tx / ty;
    const int x = bx * T + (threadIdx.x & 63);
    if (x >= w) return;
    int* L = labels + img * h * w;
    for (int r = threadIdx.x >> 6; r < T; r += WAVES) {
        const int y = by * T + r;
        if (y >= h) break;
        const int p = y * w + x, v = L[p];
        if (v == 0) continue;
        int a = v - 1;
        for (int q; (q = L[a] - 1) != a;) a = q;
        if (a + 1 != v) L[p] = a + 1;
    }
}

// ---- areas and frame contact ----
// A wave counts 16 x 64 consecutive pixels.  Per round the lanes that hold the first feature lane's label are counted at once, and that
// count is carried from round to round while the label stays: a large component costs one atomic per wave, not one per pixel.
__global__ __launch_bounds__(TPB) void ccl_area_kernel(const int* __restrict__ labels, long hw, int nblk, int* __restrict__ areas) {
    const long img = blockIdx.x / nblk, b = blockIdx.x - img * nblk;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int* L = labels + img * hw;
    int* A = areas + img * hw;
    int held = 0, held_count = 0;                        // wave-uniform
    for (int j = 0; j < AREA_ROUNDS; ++j) {
        const long p = b * AREA_CHUNK + ((long)wv * AREA_ROUNDS + j) * 64 + lane;
        const int v = p < hw ? L[p] : 0;
        const unsigned long long act = __ballot(v != 0);
        if (act == 0) continue;
        const int lead = __shfl(v, __ffsll((long long)act) - 1, 64);
        const int same = __popcll(__ballot(v == lead));
        if (lead == held) {
            held_count += same;
        } else {
            if (held_count && lane == 0) atomicAdd(A + held - 1, held_count);
            held = lead;
            held_count = same;
        }
        if (v != 0 && v != lead) atomicAdd(A + v - 1, 1);
    }
    if (held_count && lane == 0) atomicAdd(A + held - 1, held_count);
}

// One launch per side, in stream order.  Every writer of a root's byte in one launch reads the byte the launches before left and writes
// that byte with this side's bit set: the same value from all of them, so no atomic is needed and the order does not matter.
__global__ __launch_bounds__(TPB) void ccl_frame_kernel(const int* __restrict__ labels, int h, int w, int side, long len, long total,
                                                         unsigned char* frame) {
    const long id = (long)blockIdx.x * TPB + threadIdx.x;
    if (id >= total) return;
    const long img = id / len, k = id - img * len, hw = (long)h * w;
    const long p = side == 0 ? k : side == 1 ? (long)(h - 1) * w + k : side == 2 ? k * w : k * w + w - 1;
    const int v = labels[img * hw + p];
    if (v == 0) return;
    unsigned char* f = frame + img * hw + v - 1;
    *f = (unsigned char)(*f | (1 << side));
}

// ---- the area filter ----
__global__ __launch_bounds__(TPB) void ccl_filter_kernel(const int* __restrict__ labels, const int* __restrict__ areas,
                                                          const unsigned char* __restrict__ frame, long hw, int nblk, int min_area, int keep_frame,
                                                          int value, unsigned char* __restrict__ mask_out, long* __restrict__ counts) {
    __shared__ int red[WAVES][2];
    const long img = blockIdx.x / nblk, b = blockIdx.x - img * nblk;
    const long base = img * hw;
    int comps = 0, pixels = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long p = b * CHUNK + threadIdx.x + TPB * j;
        if (p >= hw) continue;
        const int v = labels[base + p];
        if (v == 0) continue;
        const long r = base + v - 1;
        if (areas[r] < min_area && !(keep_frame && frame[r] != 0)) {
            mask_out[base + p] = (unsigned char)value;
            ++pixels;
            comps += (v - 1 == p);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        comps += __shfl_xor(comps, o, 64);
        pixels += __shfl_xor(pixels, o, 64);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = comps, red[threadIdx.x >> 6][1] = pixels;
    __syncthreads();
    if (threadIdx.x < 2) {
        const int i = threadIdx.x;
        const int v = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
        // a count stays below 2^31 (h * w <= 2^30), so adding into the low word of the cleared 64-bit count never carries
        if (v) atomicAdd(reinterpret_cast<unsigned int*>(counts + img * 2 + i), (unsigned int)v);
    }
}

// ---- the table ----
// exclusive scan over the block's threads, in thread order; total: the block's sum.  Two barriers.
__device__ __forceinline__ int block_scan_excl(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(s, o, 64);
        if (lane >= o) s += t;
    }
    __syncthreads();                                     // wsum may still be read from the call before
    if (lane == 63) wsum[wv] = s;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        before += k < wv ? wsum[k] : 0;
        total += wsum[k];
    }
    return before + s - v;
}

// the roots (areas != 0) of each chunk of 1024 consecutive pixels
__global__ __launch_bounds__(TPB) void ccl_count_kernel(const int* __restrict__ areas, long hw, int nblk, int* __restrict__ chunk_count) {
    __shared__ int wsum[WAVES];
    const long img = blockIdx.x / nblk, b = blockIdx.x - img * nblk;
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long p = b * CHUNK + threadIdx.x + TPB * j;
        c += (p < hw && areas[img * hw + p] != 0);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// one block per image: the chunk counts become the number of roots before each chunk
__global__ __launch_bounds__(TPB) void ccl_scan_kernel(int* __restrict__ chunk_count, int nblk, long* __restrict__ n_components) {
    __shared__ int wsum[WAVES];
    int* cc = chunk_count + (long)blockIdx.x * nblk;
    long carry = 0;
    for (int c0 = 0; c0 < nblk; c0 += TPB) {
        const int i = c0 + threadIdx.x;
        const int v = i < nblk ? cc[i] : 0;
        int total;
        const int before = block_scan_excl(v, wsum, total);
        if (i < nblk) cc[i] = (int)(carry + before);
        carry += total;
    }
    if (threadIdx.x == 0) n_components[blockIdx.x] = carry;
}

// thread t takes the chunk's pixels 4 t .. 4 t + 3, so that thread order is pixel order: the root of rank k < capacity opens row k
__global__ __launch_bounds__(TPB) void ccl_rows_kernel(const int* __restrict__ areas, const unsigned char* __restrict__ frame, long hw, int nblk,
                                                        const int* __restrict__ chunk_before, int capacity, int* __restrict__ rank,
                                                        int* __restrict__ table) {
    __shared__ int wsum[WAVES];
    const long img = blockIdx.x / nblk, b = blockIdx.x - img * nblk;
    const long p0 = b * CHUNK + 4 * threadIdx.x;
    int a[4], c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a[j] = p0 + j < hw ? areas[img * hw + p0 + j] : 0;
        c += a[j] != 0;
    }
    int total;
    int k = chunk_before[blockIdx.x] + block_scan_excl(c, wsum, total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (a[j] == 0) continue;
        const long p = p0 + j;
        rank[img * hw + p] = k;
        if (k < capacity) {
            int* row = table + (img * capacity + k) * 8;
            row[0] = (int)p + 1, row[1] = a[j], row[2] = INT_MAX, row[3] = INT_MAX, row[4] = -1, row[5] = -1, row[6] = frame[img * hw + p], row[7] = 0;
        }
        ++k;
    }
}

// Only a pixel without a feature on one side can move that side of its component's box (a feature neighbour has the same label), and an
// atomic is issued only where the value read, which is never better than the current one, can still be improved.
__device__ __forceinline__ void box_min(int* p, int v) { if (v < g_load(p)) atomicMin(p, v); }
__device__ __forceinline__ void box_max(int* p, int v) { if (v > g_load(p)) atomicMax(p, v); }
__global__ __launch_bounds__(TPB) void ccl_box_kernel(const int* __restrict__ labels, int h, int w, int nblk, const int* __restrict__ rank,
                                                       int capacity, int* table) {
    const long img = blockIdx.x / nblk, b = blockIdx.x - img * nblk, hw = (long)h * w;
    const int* L = labels + img * hw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long p = b * CHUNK + threadIdx.x + TPB * j;
        if (p >= hw) continue;
        const int v = L[p];
        if (v == 0) continue;
        const int k = rank[img * hw + v - 1];
        if ((unsigned)k >= (unsigned)capacity) continue;  // beyond the table (or no rank at all: labels and areas that do not belong together)
        const int y = (int)(p / w), x = (int)(p - (long)y * w);
        int* row = table + (img * capacity + k) * 8;
        if (x == 0 || L[p - 1] == 0) box_min(row + 2, x);
        if (y == 0 || L[p - w] == 0) box_min(row + 3, y);
        if (x == w - 1 || L[p + 1] == 0) box_max(row + 4, x);
        if (y == h - 1 || L[p + w] == 0) box_max(row + 5, y);
    }
}

inline long chunks_of(long hw) { return (hw + CHUNK - 1) / CHUNK; }
inline long round8(long v) { return (v + 7) / 8 * 8; }
inline bool clear_async(void* p, size_t bytes, hipStream_t s, const char* what) {
    if (hipMemsetAsync(p, 0, bytes, s) == hipSuccess) return true;
    (void)hipGetLastError();
    runet_set_error(what);
    return false;
}
}  // namespace

#define CCL_REQUIRE_SHAPE()                                                                   \
    do {                                                                                      \
        RUNET_REQUIRE(n >= 1 && h >= 1 && w >= 1, "bad shape");                               \
        RUNET_REQUIRE(h <= MAX_SIDE && w <= MAX_SIDE, "h and w must not exceed 32768");       \
        RUNET_REQUIRE(runet_ccl_workspace_bytes(n, h, w) >= 0, "batch too large");            \
    } while (0)

extern "C" long runet_ccl_workspace_bytes(int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1 || h > MAX_SIDE || w > MAX_SIDE) return -1;
    const long hw = (long)h * w;
    // every launch takes one block per tile, per chunk of pixels, or per 256 border pixels: all of them fit a grid under these bounds
    const long tiles = (long)((h + T - 1) / T) * ((w + T - 1) / T);
    if (hw > (1L << 40) / n || (long)n * tiles > MAX_BLOCKS || (long)n * chunks_of(hw) > MAX_BLOCKS) return -1;
    return round8((long)n * chunks_of(hw) * 4) + round8((long)n * hw * 4);
}

extern "C" int runet_ccl_label_u8(const unsigned char* mask, int n, int h, int w, long row_stride, long image_stride, int invert, int connectivity,
                                  int* labels, void* workspace, long workspace_bytes, void* stream) {
    RUNET_REQUIRE(mask && labels && workspace, "null pointer");
    RUNET_REQUIRE(connectivity == 4 || connectivity == 8, "connectivity must be 4 or 8");
    CCL_REQUIRE_SHAPE();
    RUNET_REQUIRE(row_stride >= w, "row stride smaller than a row");
    RUNET_REQUIRE(n == 1 || image_stride >= (long)(h - 1) * row_stride + w, "image stride smaller than an image's extent");
    RUNET_REQUIRE(workspace_bytes >= runet_ccl_workspace_bytes(n, h, w), "workspace too small");
    RUNET_REQUIRE(((uintptr_t)labels & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const int tx = (w + T - 1) / T, ty = (h + T - 1) / T, conn8 = connectivity == 8;
    const long tiles = (long)n * tx * ty;
    int* tile_count = (int*)workspace;                   // n * tiles <= n * h * w words
    hipLaunchKernelGGL(ccl_tile_kernel, dim3((unsigned)tiles), dim3(TPB), 0, s, mask, h, w, row_stride, image_stride, invert, conn8, tx, ty, labels,
                       tile_count);
    const long per_image = (long)(tx - 1) * h + (long)(ty - 1) * w, total = per_image * n;
    if (total > 0)
        hipLaunchKernelGGL(ccl_seam_kernel, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, s, labels, h, w, conn8, per_image, total);
    hipLaunchKernelGGL(ccl_flatten_kernel, dim3((unsigned)tiles), dim3(TPB), 0, s, labels, h, w, tx, ty, (const int*)tile_count);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_ccl_areas(const int* labels, int n, int h, int w, int* areas, unsigned char* frame, void* stream) {
    RUNET_REQUIRE(labels && areas && frame, "null pointer");
    CCL_REQUIRE_SHAPE();
    RUNET_REQUIRE((((uintptr_t)labels | (uintptr_t)areas) & 3) == 0, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const long hw = (long)h * w;
    if (!clear_async(areas, (size_t)n * hw * sizeof(int), s, "runet_ccl_areas: clearing the areas failed")) return RUNET_ELAUNCH;
    if (!clear_async(frame, (size_t)n * hw, s, "runet_ccl_areas: clearing the frame bytes failed")) return RUNET_ELAUNCH;
    const int nblk = cdiv(hw, AREA_CHUNK);
    hipLaunchKernelGGL(ccl_area_kernel, dim3((unsigned)((long)n * nblk)), dim3(TPB), 0, s, labels, hw, nblk, areas);
    for (int side = 0; side < 4; ++side) {
        const long len = side < 2 ? w : h, total = len * n;
        hipLaunchKernelGGL(ccl_frame_kernel, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, s, labels, h, w, side, len, total, frame);
    }
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_ccl_filter_u8(const int* labels, const int* areas, const unsigned char* frame, int n, int h, int w, int min_area,
                                   int keep_frame, int value, unsigned char* mask_out, long* counts, void* stream) {
    RUNET_REQUIRE(labels && areas && frame && mask_out && counts, "null pointer");
    CCL_REQUIRE_SHAPE();
    RUNET_REQUIRE(min_area >= 0, "min_area is not negative");
    RUNET_REQUIRE(value >= 0 && value <= 255, "value is a byte");
    RUNET_REQUIRE((((uintptr_t)labels | (uintptr_t)areas) & 3) == 0 && ((uintptr_t)counts & 7) == 0, "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    if (!clear_async(counts, (size_t)n * 2 * sizeof(long), s, "runet_ccl_filter_u8: clearing the counts failed")) return RUNET_ELAUNCH;
    const long hw = (long)h * w;
    const int nblk = (int)chunks_of(hw);
    hipLaunchKernelGGL(ccl_filter_kernel, dim3((unsigned)((long)n * nblk)), dim3(TPB), 0, s, labels, areas, frame, hw, nblk, min_area, keep_frame,
                       value, mask_out, counts);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_ccl_table(const int* labels, const int* areas, const unsigned char* frame, int n, int h, int w, int capacity,
                               long* n_components, int* table, void* workspace, long workspace_bytes, void* stream) {
    RUNET_REQUIRE(labels && areas && frame && n_components && workspace, "null pointer");
    RUNET_REQUIRE(capacity >= 0, "capacity is not negative");
    RUNET_REQUIRE(capacity == 0 || table, "null pointer");
    CCL_REQUIRE_SHAPE();
    RUNET_REQUIRE(workspace_bytes >= runet_ccl_workspace_bytes(n, h, w), "workspace too small");
    RUNET_REQUIRE((((uintptr_t)labels | (uintptr_t)areas | (uintptr_t)table) & 3) == 0 && (((uintptr_t)n_components | (uintptr_t)workspace) & 7) == 0,
                  "misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    const long hw = (long)h * w;
    const int nblk = (int)chunks_of(hw);
    const unsigned grid = (unsigned)((long)n * nblk);
    int* chunk_count = (int*)workspace;
    int* rank = (int*)((char*)workspace + round8((long)n * nblk * 4));
    hipLaunchKernelGGL(ccl_count_kernel, dim3(grid), dim3(TPB), 0, s, areas, hw, nblk, chunk_count);
    hipLaunchKernelGGL(ccl_scan_kernel, dim3(n), dim3(TPB), 0, s, chunk_count, nblk, n_components);
    if (capacity > 0) {
        hipLaunchKernelGGL(ccl_rows_kernel, dim3(grid), dim3(TPB), 0, s, areas, frame, hw, nblk, (const int*)chunk_count, capacity, rank, table);
        hipLaunchKernelGGL(ccl_box_kernel, dim3(grid), dim3(TPB), 0, s, labels, h, w, nblk, (const int*)rank, capacity, table);
    }
    RUNET_CHECK_LAUNCH();
}
