// External contours of a binary mask on the device (predict_coastline.py:605-608: cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) and
// the `> 10` length filter), as parallel border following.  The host tracer (predict.trace_external_contours) walks borders one pixel at a
// time; its inner loop is a pure function of the mask, so the walk is restated as a successor map on STATES and solved by pointer jumping:
//   state     (p, d): pixel p is set and its neighbour in direction d (E, NE, N, NW, W, SW, S, SE = 0..7, y downwards) is set: "at p, having
//             come from the pixel in direction d".  An isolated pixel carries one pseudo-state (d = 8) that is its own successor.
//   successor scan e = d + 1, d + 2, ... (mod 8) to the first set neighbour q of p; p is LEFT in direction e, the successor is (q, (e + 4) % 8).
//   On the valid states this map is a bijection: the state graph is a disjoint union of cycles, one per border (outer or hole).
//   States are only materialised on CANDIDATE pixels (set, with a clear 4-neighbour; outside the image is clear): every pixel of a real border
//   is one.  A spare state whose successor lands on a non-candidate pixel becomes its own successor; such chains never hold a start state.
//   start     (p0, d1) starts a contour iff p0's west neighbour is clear and 4-connected to the outside of the zero-padded image, d1 is the
//             first set neighbour clockwise from west (W, NW, N, NE, E, SE, S, SW), and p0 is the smallest pixel index of its cycle.
//   vertex    the pixel of state (p, d) is kept iff it is left in a direction other than the one it was entered in: e != (d + 4) % 8.
// Foreground is 8-connected, background 4-connected.  Every loop on the device has a trip count bounded by the data: pointer jumping runs a
// fixed ceil(log2(n_states)) rounds, union-find walks follow strictly decreasing indices.  Integer atomics (atomicMin) only; the roots are the
// minimum index of their set, so nothing depends on arrival order and two runs give the same bytes.
#include "runet_common.h"
#include "scan.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int TPB = 256;
static_assert(TPB == SCAN_TPB, "the scans of scan.h run in this file's block shape");

__device__ __forceinline__ int ddy(int d) { return (int)((0xA901u >> (2 * d)) & 3u) - 1; }      // 0, -1, -1, -1, 0, 1, 1, 1
__device__ __forceinline__ int ddx(int d) { return (int)((0x901Au >> (2 * d)) & 3u) - 1; }      // 1, 1, 0, -1, -1, -1, 0, 1

// info word of a pixel: bit 8 = candidate, bits 0..7 = its set neighbours
__device__ __forceinline__ int state_count(unsigned int info) { return (info >> 8) ? ((info & 255u) ? __popc(info & 255u) : 1) : 0; }

// the exclusive prefix sums (excl_scan, Plain) are scan.h's
struct PixelStates {                                     // states of pixel i
    const unsigned short* info;
    __device__ int operator()(long i) const { return state_count(info[i]); }
};

// ---- (a) candidates and their set neighbours ----
__global__ void __launch_bounds__(TPB) flag_kernel(const unsigned char* __restrict__ mask, int h, int w, unsigned short* __restrict__ info) {
    const long p = (long)blockIdx.x * TPB + threadIdx.x;
    if (p >= (long)h * w) return;
    const int y = (int)(p / w), x = (int)(p - (long)y * w);
    unsigned int v = 0;
    if (mask[p]) {
        unsigned int nb = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int yy = y + ddy(d), xx = x + ddx(d);
            if (yy >= 0 && yy < h && xx >= 0 && xx < w && mask[(long)yy * w + xx]) nb |= 1u << d;
        }
        if ((nb & 0x55u) != 0x55u) v = 0x100u | nb;      // E, N, W, S not all set
    }
    info[p] = (unsigned short)v;
}

// ---- (c) background, 4-connected, the frame around the image one component: union-find, node 0 = the frame, node p + 1 = pixel p ----
// par[x] <= x always and only ever decreases (atomicMin), so every walk is strictly decreasing.  Loads go past this CU's L1.
__device__ __forceinline__ int uf_load(const int* par, int x) { return __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ int uf_find(int* par, int x) {                // with path halving; a stale parent is still an ancestor
    int q = uf_load(par, x);
    while (q != x) {
        const int g = uf_load(par, q);
        if (g != q) atomicMin(par + x, g);
        x = q;
        q = g;
    }
    return x;
}

__device__ void uf_union(int* par, int a, int b) {       // max(a, b) falls with every round
    a = uf_find(par, a);
    b = uf_find(par, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a) break;                             // a was a root and now hangs under b
        a = old;                                         // a had been linked meanwhile: join that parent with b
    }
}

// every background pixel starts under the first pixel of its run inside its 64-pixel wave segment (runs are cut at row ends by x == 0)
__global__ void __launch_bounds__(TPB) bg_init_kernel(const unsigned char* __restrict__ mask, int h, int w, int* __restrict__ par) {
    const long p = (long)blockIdx.x * TPB + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = p < (long)h * w;
    bool bg = false, first = false;
    if (in) {
        const int x = (int)(p % w);
        bg = mask[p] == 0;
        first = bg && (x == 0 || mask[p - 1] != 0);
    }
    const unsigned long long starts = __ballot(first);
    if (p == 0) par[0] = 0;
    if (!in) return;
    int node = (int)p + 1;
    if (bg) {
        const unsigned long long below = starts & ((2ull << lane) - 1ull);
        const int s = below ? 63 - __clzll(below) : 0;   // no start at or below this lane: the run reaches lane 0 and goes on to the left
        node = (int)(p - lane + s) + 1;
    }
    par[p + 1] = node;
}

__global__ void __launch_bounds__(TPB) bg_merge_kernel(const unsigned char* __restrict__ mask, int h, int w, int* __restrict__ par) {
    const long p = (long)blockIdx.x * TPB + threadIdx.x;
    if (p >= (long)h * w || mask[p] != 0) return;
    const int y = (int)(p / w), x = (int)(p - (long)y * w);
    const int node = (int)p + 1;
    const bool west_bg = x > 0 && mask[p - 1] == 0;
    if (west_bg && (p & 63) == 0) uf_union(par, node, node - 1);                       // a run that crosses a segment boundary
    if (y > 0 && mask[p - w] == 0 && (!west_bg || mask[p - w - 1] != 0)) uf_union(par, node, node - w);   // once per pair of touching runs
    if (x == 0 || y == 0 || x == w - 1 || y == h - 1) uf_union(par, node, 0);
}

// ---- (b) states and their successors ----
// (n is the caller's state count: a count that does not belong to this workspace must not write past the arrays it sized)
__global__ void __launch_bounds__(TPB) fill_states_kernel(const unsigned short* __restrict__ info, const int* __restrict__ sbase, long npix, int n,
                                                          int* __restrict__ spix, unsigned char* __restrict__ sdir) {
    const long p = (long)blockIdx.x * TPB + threadIdx.x;
    if (p >= npix) return;
    const unsigned int v = info[p];
    if (!(v >> 8)) return;
    int s = sbase[p];
    if (s < 0 || (long)s + state_count(v) > n) return;
    const unsigned int nb = v & 255u;
    if (!nb) {
        spix[s] = (int)p;
        sdir[s] = 8;
        return;
    }
#pragma unroll
    for (int d = 0; d < 8; ++d)
        if ((nb >> d) & 1u) {
            spix[s] = (int)p;
            sdir[s] = (unsigned char)d;
            ++s;
        }
}

// succ[s], the direction the pixel is left in (ldir), and the jumping start: ptr = succ, key = the state's pixel
__global__ void __launch_bounds__(TPB) succ_kernel(const unsigned short* __restrict__ info, const int* __restrict__ sbase, int w, int n,
                                                   const int* __restrict__ spix, const unsigned char* __restrict__ sdir, int* __restrict__ succ,
                                                   unsigned char* __restrict__ ldir, int* __restrict__ ptr, int* __restrict__ key) {
    const int s = blockIdx.x * TPB + threadIdx.x;
    if (s >= n) return;
    const int p = spix[s], d = sdir[s];
    int nx = s, e = 8;
    if (d < 8) {
        const unsigned int nb = info[p] & 255u;
        const unsigned int rot = ((nb | (nb << 8)) >> (d + 1)) & 255u;                // bit k = neighbour d + 1 + k; bit 7 = d itself, set
        e = (d + 1 + (__ffs(rot) - 1)) & 7;
        const int q = p + ddy(e) * w + ddx(e), back = (e + 4) & 7;
        const unsigned int vq = info[q];
        if (vq >> 8) nx = sbase[q] + __popc(vq & ((1u << back) - 1u));
        if (nx < 0 || nx >= n) nx = s;
    }
    succ[s] = nx;
    ldir[s] = (unsigned char)e;
    ptr[s] = nx;
    key[s] = p;
}

// ---- (d) the smallest pixel of every cycle: min over a window that doubles each round ----
__global__ void __launch_bounds__(TPB) jump_min_kernel(int n, const int* __restrict__ ptr_in, const int* __restrict__ key_in,
                                                       int* __restrict__ ptr_out, int* __restrict__ key_out) {
    const int s = blockIdx.x * TPB + threadIdx.x;
    if (s >= n) return;
    const int t = ptr_in[s];
    const int a = key_in[s], b = key_in[t];
    key_out[s] = a < b ? a : b;
    ptr_out[s] = ptr_in[t];
}

__global__ void __launch_bounds__(TPB) start_kernel(const unsigned short* __restrict__ info, int w, int n, const int* __restrict__ spix,
                                                    const unsigned char* __restrict__ sdir, const int* __restrict__ key, int* __restrict__ par,
                                                    int* __restrict__ start) {
    const int s = blockIdx.x * TPB + threadIdx.x;
    if (s >= n) return;
    const int p = spix[s], d = sdir[s];
    bool ok = key[s] == p;
    if (ok && d < 8) {
        const unsigned int nb = info[p] & 255u;
        ok = !(nb & 0x10u);                              // west clear
        if (ok) {
            int d1 = 8;
#pragma unroll
            for (int k = 7; k >= 1; --k) {               // last assignment wins: k = 1 (NW) first in clockwise order
                const int dd = (4 - k) & 7;
                if ((nb >> dd) & 1u) d1 = dd;
            }
            ok = d == d1;
        }
    }
    if (ok && p % w != 0) ok = uf_find(par, p) == 0;     // node p = the pixel west of p
    start[s] = ok ? 1 : 0;
}

// ---- (e) cut every kept cycle in front of its start state and rank towards the cut ----
__global__ void __launch_bounds__(TPB) rank_init_kernel(int n, const int* __restrict__ succ, const int* __restrict__ start, int* __restrict__ ptr,
                                                        unsigned int* __restrict__ rank) {
    const int s = blockIdx.x * TPB + threadIdx.x;
    if (s >= n) return;
    const int t = succ[s];
    const bool last = start[t] != 0;
    ptr[s] = last ? s : t;
    rank[s] = last ? 0u : 1u;
}

__global__ void __launch_bounds__(TPB) jump_rank_kernel(int n, const int* __restrict__ ptr_in, const unsigned int* __restrict__ rank_in,
                                                        int* __restrict__ ptr_out, unsigned int* __restrict__ rank_out) {
    const int s = blockIdx.x * TPB + threadIdx.x;
    if (s >= n) return;
    const int t = ptr_in[s];
    rank_out[s] = rank_in[s] + rank_in[t];
    ptr_out[s] = ptr_in[t];
}

__global__ void __launch_bounds__(TPB) length_kernel(int n, const int* __restrict__ start, const int* __restrict__ cid,
                                                     const unsigned int* __restrict__ rank, int* __restrict__ len) {
    const int s = blockIdx.x * TPB + threadIdx.x;
    if (s >= n || !start[s]) return;
    len[cid[s]] = (int)rank[s] + 1;
}

// ---- (f) the states of the kept cycles in contour order: slot g = cbase[contour] + position ----
__global__ void __launch_bounds__(TPB) order_kernel(int n, const int* __restrict__ succ, const int* __restrict__ start, const int* __restrict__ cid,
                                                    const int* __restrict__ ptr, const unsigned int* __restrict__ rank,
                                                    const int* __restrict__ cbase, const int* __restrict__ spix,
                                                    const unsigned char* __restrict__ sdir, const unsigned char* __restrict__ ldir,
                                                    int* __restrict__ okeep, int* __restrict__ opix, int* __restrict__ ocid) {
    const int s = blockIdx.x * TPB + threadIdx.x;
    if (s >= n) return;
    const int s0 = succ[ptr[s]];
    if (!start[s0]) return;                              // not on a kept cycle
    const int c = cid[s0];
    const long g = (long)cbase[c] + ((long)rank[s0] - (long)rank[s]);
    if (g < 0 || g >= n) return;
    const int d = sdir[s];
    okeep[g] = (d == 8 || ldir[s] != ((d + 4) & 7)) ? 1 : 0;
    opix[g] = spix[s];
    ocid[g] = c;
}

// ---- (g) lengths after run compression, the min_points filter, the packed result ----
__global__ void __launch_bounds__(TPB) count_kernel(int n, const int* __restrict__ n_raw, const int* __restrict__ cbase, const int* __restrict__ len,
                                                    const int* __restrict__ vscan, int min_points, int* __restrict__ ckeep,
                                                    int* __restrict__ cpts) {
    const int c = blockIdx.x * TPB + threadIdx.x;
    if (c >= n) return;
    int keep = 0, pts = 0;
    if (c < *n_raw) {
        pts = vscan[cbase[c] + len[c]] - vscan[cbase[c]];
        keep = pts > min_points;
    }
    ckeep[c] = keep;
    cpts[c] = keep ? pts : 0;
}

// out: int32 {n_contours, n_points, offsets [n_contours + 1], points [n_points][2] = (x, y)}
__global__ void __launch_bounds__(TPB) emit_kernel(int n, int w, const int* __restrict__ n_slots, const int* __restrict__ okeep,
                                                   const int* __restrict__ opix, const int* __restrict__ ocid, const int* __restrict__ vscan,
                                                   const int* __restrict__ cbase, const int* __restrict__ ckeep, const int* __restrict__ cnew,
                                                   const int* __restrict__ coff, int* __restrict__ out) {
    const int g = blockIdx.x * TPB + threadIdx.x;
    if (g >= n || g >= *n_slots) return;
    const int c = ocid[g];
    if (!ckeep[c]) return;
    const int nc = out[0];
    if (g == cbase[c]) out[2 + cnew[c]] = coff[c];       // the contour's first slot writes its offset
    if (!okeep[g]) return;
    const long v = (long)coff[c] + (vscan[g] - vscan[cbase[c]]);
    int* pts = out + 3 + nc;
    const int p = opix[g];
    pts[2 * v] = p % w;
    pts[2 * v + 1] = p / w;
}

__global__ void close_offsets_kernel(int* __restrict__ out) { out[2 + out[0]] = out[1]; }

inline long up256(long b) { return (b + 255) / 256 * 256; }
inline int log2_ceil(long n) {
    int r = 0;
    while ((1L << r) < n) ++r;
    return r;
}

struct PixelWs {                                         // byte offsets into the pixel workspace
    long info, sbase, par, bsum, total;
    PixelWs(long npix) {
        info = 0;
        sbase = info + up256(npix * 2);
        par = sbase + up256(npix * 4);
        bsum = par + up256((npix + 1) * 4);
        total = bsum + up256((long)cdiv(npix, SCAN_TILE) * 4);
    }
};

struct StateWs {                                         // byte offsets into the state workspace; the packed result comes first
    long out, spix, succ, start, cid, buf[4], len, cbase, okeep, vscan, opix, ocid, bsum, small, sdir, ldir, total;
    StateWs(long n) {
        long o = 0;
        auto take = [&](long bytes) { const long at = o; o += up256(bytes); return at; };
        out = take((3 * n + 3) * 4);
        spix = take(n * 4);
        succ = take(n * 4);
        start = take(n * 4);
        cid = take(n * 4);
        for (int i = 0; i < 4; ++i) buf[i] = take(n * 4);
        len = take(n * 4);
        cbase = take(n * 4);
        okeep = take((n + 1) * 4);
        vscan = take((n + 1) * 4);
        opix = take(n * 4);
        ocid = take(n * 4);
        bsum = take((long)cdiv(n + 1, SCAN_TILE) * 4);
        small = take(16);
        sdir = take(n);
        ldir = take(n);
        total = o;
    }
};
}  // namespace

extern "C" long runet_contours_workspace_bytes(int h, int w) {
    if (h <= 0 || w <= 0 || (long)h * w >= (1L << 31)) return -1;
    return PixelWs((long)h * w).total;
}

extern "C" long runet_contours_state_workspace_bytes(long n_states) {
    if (n_states <= 0 || n_states >= (1L << 31)) return -1;
    return StateWs(n_states).total;
}

extern "C" int runet_contours_count(const unsigned char* mask, int h, int w, void* workspace, long workspace_bytes, long* n_states,
                                    void* stream) {
    RUNET_REQUIRE(mask && workspace && n_states, "null pointer");
    RUNET_REQUIRE(h > 0 && w > 0, "bad shape");
    RUNET_REQUIRE((long)h * w < (1L << 31), "h * w must be below 2^31");
    RUNET_REQUIRE(RUNET_ALIGNED16(workspace) && ((uintptr_t)n_states % 8) == 0, "workspace must be 16-byte, n_states 8-byte aligned");
    const long npix = (long)h * w;
    const PixelWs L(npix);
    RUNET_REQUIRE(workspace_bytes >= L.total, "workspace too small (runet_contours_workspace_bytes)");
    char* ws = (char*)workspace;
    unsigned short* info = (unsigned short*)(ws + L.info);
    int* sbase = (int*)(ws + L.sbase);
    int* par = (int*)(ws + L.par);
    hipStream_t st = (hipStream_t)stream;
    const int blocks = cdiv(npix, TPB);
    hipLaunchKernelGGL(flag_kernel, dim3(blocks), dim3(TPB), 0, st, mask, h, w, info);
    excl_scan(PixelStates{info}, npix, sbase, (int*)(ws + L.bsum), (long long*)n_states, (int*)nullptr, st);
    hipLaunchKernelGGL(bg_init_kernel, dim3(blocks), dim3(TPB), 0, st, mask, h, w, par);
    hipLaunchKernelGGL(bg_merge_kernel, dim3(blocks), dim3(TPB), 0, st, mask, h, w, par);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_contours_trace(int h, int w, void* workspace, long workspace_bytes, long n_states, int min_points, void* state_workspace,
                                    long state_workspace_bytes, void* stream) {
    RUNET_REQUIRE(workspace && state_workspace, "null pointer");
    RUNET_REQUIRE(h > 0 && w > 0, "bad shape");
    RUNET_REQUIRE((long)h * w < (1L << 31), "h * w must be below 2^31");
    RUNET_REQUIRE(n_states >= 1 && min_points >= 0, "bad state count / min_points");
    RUNET_REQUIRE(n_states < (1L << 31), "the state count does not fit int32");
    RUNET_REQUIRE(n_states <= 8L * h * w, "more states than 8 per pixel");
    RUNET_REQUIRE(RUNET_ALIGNED16(workspace) && RUNET_ALIGNED16(state_workspace), "workspaces must be 16-byte aligned");
    const long npix = (long)h * w;
    const PixelWs L(npix);
    const StateWs S(n_states);
    RUNET_REQUIRE(workspace_bytes >= L.total, "workspace too small (runet_contours_workspace_bytes)");
    RUNET_REQUIRE(state_workspace_bytes >= S.total, "state workspace too small (runet_contours_state_workspace_bytes)");
    const int n = (int)n_states;
    char* ws = (char*)workspace;
    char* sw = (char*)state_workspace;
    const unsigned short* info = (const unsigned short*)(ws + L.info);
    const int* sbase = (const int*)(ws + L.sbase);
    int* par = (int*)(ws + L.par);
    int* out = (int*)(sw + S.out);
    int* spix = (int*)(sw + S.spix);
    int* succ = (int*)(sw + S.succ);
    int* start = (int*)(sw + S.start);
    int* cid = (int*)(sw + S.cid);
    int* buf[4];
    for (int i = 0; i < 4; ++i) buf[i] = (int*)(sw + S.buf[i]);
    int* len = (int*)(sw + S.len);
    int* cbase = (int*)(sw + S.cbase);
    int* okeep = (int*)(sw + S.okeep);
    int* vscan = (int*)(sw + S.vscan);
    int* opix = (int*)(sw + S.opix);
    int* ocid = (int*)(sw + S.ocid);
    int* bsum = (int*)(sw + S.bsum);
    int* small = (int*)(sw + S.small);                   // {contours before the filter, slots, vertices before the filter}
    unsigned char* sdir = (unsigned char*)(sw + S.sdir);
    unsigned char* ldir = (unsigned char*)(sw + S.ldir);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(len, 0, (size_t)n * 4, st) != hipSuccess || hipMemsetAsync(okeep, 0, ((size_t)n + 1) * 4, st) != hipSuccess) {
        (void)hipGetLastError();
        runet_set_error("runet_contours_trace: clearing the workspace failed");
        return RUNET_ELAUNCH;
    }
    const int pblocks = cdiv(npix, TPB), sblocks = cdiv(n, TPB);
    const int rounds = log2_ceil(n);
    hipLaunchKernelGGL(fill_states_kernel, dim3(pblocks), dim3(TPB), 0, st, info, sbase, npix, n, spix, sdir);
    int *ptr_a = buf[0], *key_a = buf[1], *ptr_b = buf[2], *key_b = buf[3];
    hipLaunchKernelGGL(succ_kernel, dim3(sblocks), dim3(TPB), 0, st, info, sbase, w, n, spix, sdir, succ, ldir, ptr_a, key_a);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(jump_min_kernel, dim3(sblocks), dim3(TPB), 0, st, n, ptr_a, key_a, ptr_b, key_b);
        int* t = ptr_a; ptr_a = ptr_b; ptr_b = t;
        t = key_a; key_a = key_b; key_b = t;
    }
    hipLaunchKernelGGL(start_kernel, dim3(sblocks), dim3(TPB), 0, st, info, w, n, spix, sdir, key_a, par, start);
    excl_scan(Plain{start}, (long)n, cid, bsum, (long long*)nullptr, small + 0, st);
    hipLaunchKernelGGL(rank_init_kernel, dim3(sblocks), dim3(TPB), 0, st, n, succ, start, ptr_a, (unsigned int*)key_a);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(jump_rank_kernel, dim3(sblocks), dim3(TPB), 0, st, n, ptr_a, (const unsigned int*)key_a, ptr_b, (unsigned int*)key_b);
        int* t = ptr_a; ptr_a = ptr_b; ptr_b = t;
        t = key_a; key_a = key_b; key_b = t;
    }
    hipLaunchKernelGGL(length_kernel, dim3(sblocks), dim3(TPB), 0, st, n, start, cid, (const unsigned int*)key_a, len);
    excl_scan(Plain{len}, (long)n, cbase, bsum, (long long*)nullptr, small + 1, st);
    hipLaunchKernelGGL(order_kernel, dim3(sblocks), dim3(TPB), 0, st, n, succ, start, cid, ptr_a, (const unsigned int*)key_a, cbase, spix, sdir, ldir,
                       okeep, opix, ocid);
    excl_scan(Plain{okeep}, (long)n + 1, vscan, bsum, (long long*)nullptr, small + 2, st);
    // the jumping buffers are free from here on
    int *ckeep = buf[0], *cpts = buf[1], *cnew = buf[2], *coff = buf[3];
    hipLaunchKernelGGL(count_kernel, dim3(sblocks), dim3(TPB), 0, st, n, small + 0, cbase, len, vscan, min_points, ckeep, cpts);
    excl_scan(Plain{ckeep}, (long)n, cnew, bsum, (long long*)nullptr, out + 0, st);
    excl_scan(Plain{cpts}, (long)n, coff, bsum, (long long*)nullptr, out + 1, st);
    hipLaunchKernelGGL(close_offsets_kernel, dim3(1), dim3(1), 0, st, out);
    hipLaunchKernelGGL(emit_kernel, dim3(sblocks), dim3(TPB), 0, st, n, w, small + 1, okeep, opix, ocid, vscan, cbase, ckeep, cnew, coff, out);
    RUNET_CHECK_LAUNCH();
}
