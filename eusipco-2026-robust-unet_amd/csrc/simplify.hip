// Douglas-Peucker on the device for the tracer's integer contours (predict_coastline.py:612-615: cv2.approxPolyDP(contour, 0.002 *
// arcLength)), by the project's EXACT rule: every decision is integer arithmetic or one correctly rounded double operation, ties go to the
// first index.  The rule is stated in include/runet_hip.h; predict.approx_poly_dp_exact restates it on the host and gives the same lists.
// Formulation: one workgroup per contour, level-synchronous rounds inside the kernel (workgroup barriers only).  Positions 0..n, q[n] = p[0].
//   state  per interior position i of an open segment (a, b): sa[i] = a, sb[i] = b; sa[i] = -1 once i is kept or its segment has closed.
//          per segment, at index a: best[a] = max N of its interior positions, bidx[a] = the first position that reaches it.
//   round  (0) clear best / bidx of the open segments, (1) atomicMax of N into best[a], (2) atomicMin of i into bidx[a] where N == best[a],
//          (3) every position reads its segment's (best, bidx), takes the decision and narrows to (a, k) or (k, b), is kept (i == k) or closes.
//   Every round splits or closes every open segment, so there are at most n rounds (the recursion depth of the contour).  64-bit and 32-bit
//   integer atomics on values that do not depend on arrival order; two runs give the same bytes.
// Contours of at most `lds_max_vertices` (<= SIMPLIFY_LDS_CAP) vertices keep the state and their points in LDS, longer ones keep the state in
// the caller's workspace and read the points from the packed input.  Then one exclusive scan over the keep flags of all vertices gives every
// kept vertex its slot and every contour its offset, and an emit pass writes the packed result.
#include "runet_common.h"
#include "scan.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int TPB = 256;
constexpr int SIMPLIFY_LDS_CAP = 2048;                   // vertices: 24 bytes of LDS each, 48 KiB per workgroup
constexpr int COORD_MAX = 46340;                         // 2 * 46340^2 < 2^32
typedef unsigned long long u64;

struct Pt {
    int x, y;
};

// den * (squared distance of p to the clipped segment a-b), den = |b - a|^2 (1 stands in for den == 0): below 2^64
__device__ __forceinline__ u64 dist_numerator(const Pt a, const Pt b, const Pt p, u64& den) {
    const long long abx = b.x - a.x, aby = b.y - a.y, apx = p.x - a.x, apy = p.y - a.y;
    const u64 d = (u64)(abx * abx + aby * aby), ap2 = (u64)(apx * apx + apy * apy);
    const long long dot = apx * abx + apy * aby;
    if (d == 0) {
        den = 1;
        return ap2;
    }
    den = d;
    if (dot <= 0) return ap2 * d;
    if ((u64)dot >= d) {
        const long long bpx = p.x - b.x, bpy = p.y - b.y;
        return (u64)(bpx * bpx + bpy * bpy) * d;
    }
    const long long cr = apx * aby - apy * abx;
    const u64 c = (u64)(cr < 0 ? -cr : cr);
    return c * c;
}

// thr = (eps_factor * (A + D sqrt2))^2 in four double operations, each rounded on its own.  __dmul_rn / __dadd_rn are plain operators to
// the compiler, which would contract the multiply and the add into one fused operation: contraction is off for these lines.
__device__ __forceinline__ double threshold_of(const u64 sum_axis, const u64 sum_diag, const double eps_factor) {
#pragma clang fp contract(off)
    const double prod = (double)sum_diag * 0x1.6a09e667f3bcdp+0;
    const double len = (double)sum_axis + prod;
    const double eps = eps_factor * len;
    return eps * eps;
}

// Points of the LDS variant: (x | y << 16) in LDS; of the workspace variant: the packed input itself.
struct LdsPoints {
    const unsigned int* xy;
    int n;
    __device__ __forceinline__ Pt operator()(int i) const {
        const unsigned int v = xy[i == n ? 0 : i];
        return Pt{(int)(v & 0xffffu), (int)(v >> 16)};
    }
};
struct GlobalPoints {
    const int* pts;
    int n;
    __device__ __forceinline__ Pt operator()(int i) const {
        const int j = i == n ? 0 : i;
        return Pt{pts[2 * j], pts[2 * j + 1]};
    }
};

// best / bidx are written by atomics of other lanes: the workspace variant reads them past this CU's L1
template <bool LDS, class T>
__device__ __forceinline__ T ld(const T* p) {
    if constexpr (LDS) return *p;
    else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// head: {contours, kept vertices, bad inputs, largest round count}
template <bool LDS>
__global__ void __launch_bounds__(TPB) simplify_kernel(const int* __restrict__ packed, int nc, int total, double eps_factor, int lds_max,
                                                       int* __restrict__ head, int* __restrict__ keep, int* __restrict__ g_sa,
                                                       int* __restrict__ g_sb, int* __restrict__ g_bidx, u64* __restrict__ g_best) {
    __shared__ u64 s_sumA, s_sumD, s_far;
    __shared__ int s_bad;
    __shared__ u64 l_best[LDS ? SIMPLIFY_LDS_CAP : 1];
    __shared__ int l_sa[LDS ? SIMPLIFY_LDS_CAP : 1], l_sb[LDS ? SIMPLIFY_LDS_CAP : 1], l_bidx[LDS ? SIMPLIFY_LDS_CAP : 1];
    __shared__ unsigned int l_xy[LDS ? SIMPLIFY_LDS_CAP : 1];

    const int c = blockIdx.x, tid = threadIdx.x;
    const int* off = packed + 2;
    const int o0 = off[c], o1 = off[c + 1];
    const bool header_ok = packed[0] == nc && packed[1] == total && (c > 0 || o0 == 0) && (c < nc - 1 || o1 == total);
    if (!(header_ok && o0 >= 0 && o0 <= o1 && o1 <= total)) {   // offsets that do not describe this input: counted, nothing of it touched
        if (!LDS && tid == 0) atomicAdd(head + 2, 1);
        return;
    }
    const int n = o1 - o0;
    if ((n <= lds_max) != LDS || n == 0) return;                // the other variant's contour
    const int* pts = packed + 3 + nc + 2 * (long)o0;
    keep += o0;

    // ---- setup: coordinates and edges checked, arc length A + D sqrt(2), the far vertex ----
    if (tid == 0) {
        s_sumA = 0;
        s_sumD = 0;
        s_far = 0;
        s_bad = 0;
    }
    __syncthreads();
    {
        u64 sumA = 0, sumD = 0, far = 0;
        int bad = 0;
        const int x0 = pts[0], y0 = pts[1];
        const bool in0 = x0 >= 0 && x0 <= COORD_MAX && y0 >= 0 && y0 <= COORD_MAX;
        for (int i = tid; i < n; i += TPB) {
            const int x = pts[2 * i], y = pts[2 * i + 1];
            if (!(x >= 0 && x <= COORD_MAX && y >= 0 && y <= COORD_MAX)) {
                ++bad;                                          // a vertex outside the coordinate range
                continue;
            }
            const int j = i + 1 == n ? 0 : i + 1;
            const int xn = pts[2 * j], yn = pts[2 * j + 1];
            if (!(xn >= 0 && xn <= COORD_MAX && yn >= 0 && yn <= COORD_MAX && in0)) continue;   // counted at that vertex
            if (LDS) l_xy[i] = (unsigned int)x | ((unsigned int)y << 16);
            const int dx = xn > x ? xn - x : x - xn, dy = yn > y ? yn - y : y - yn;
            if (dx == 0 || dy == 0) sumA += (u64)(dx + dy);
            else if (dx == dy) sumD += (u64)dx;
            else ++bad;                                         // an edge between two good vertices that is not a run
            const long long fx = x - x0, fy = y - y0;
            const u64 key = ((u64)(fx * fx + fy * fy) << 32) | (u64)(~(unsigned int)i);
            far = key > far ? key : far;
        }
        if (bad) atomicAdd(&s_bad, bad);
        if (sumA) atomicAdd(&s_sumA, sumA);
        if (sumD) atomicAdd(&s_sumD, sumD);
        if (far) atomicMax(&s_far, far);
    }
    __syncthreads();
    if (s_bad) {                                                // counted, never guessed at: the contour keeps nothing
        if (tid == 0) atomicAdd(head + 2, s_bad);
        return;
    }
    const int far = (int)(~(unsigned int)(s_far & 0xffffffffull));
    if (tid == 0) keep[0] = 1;
    if (far == 0) return;                                       // every vertex is p[0]
    if (tid == 0) keep[far] = 1;
    const double thr = threshold_of(s_sumA, s_sumD, eps_factor);

    int* sa = LDS ? l_sa : g_sa + o0;
    int* sb = LDS ? l_sb : g_sb + o0;
    int* bidx = LDS ? l_bidx : g_bidx + o0;
    u64* best = LDS ? l_best : g_best + o0;
    auto rounds_of = [&](auto q) {
        int open = 0;
        for (int i = tid; i < n; i += TPB) {
            const bool interior = i != 0 && i != far;
            sa[i] = !interior ? -1 : (i < far ? 0 : far);
            sb[i] = i < far ? far : n;
            open |= interior;
        }
        int rounds = 0;
        while (__syncthreads_or(open) && rounds < n) {
            ++rounds;
            for (int i = tid; i < n; i += TPB) {
                const int a = sa[i];
                if (a < 0) continue;
                best[a] = 0;                                    // the same two words from every position of the segment
                bidx[a] = 0x7fffffff;
            }
            __syncthreads();
            for (int i = tid; i < n; i += TPB) {
                const int a = sa[i];
                if (a < 0) continue;
                u64 den;
                atomicMax(best + a, dist_numerator(q(a), q(sb[i]), q(i), den));
            }
            __syncthreads();
            for (int i = tid; i < n; i += TPB) {
                const int a = sa[i];
                if (a < 0) continue;
                u64 den;
                if (dist_numerator(q(a), q(sb[i]), q(i), den) == ld<LDS>(best + a)) atomicMin(bidx + a, i);
            }
            __syncthreads();
            open = 0;
            for (int i = tid; i < n; i += TPB) {
                const int a = sa[i];
                if (a < 0) continue;
                const int b = sb[i], k = ld<LDS>(bidx + a);
                u64 den;
                dist_numerator(q(a), q(b), q(a), den);
                const bool split = __ull2double_rn(ld<LDS>(best + a)) > __dmul_rn(thr, __ull2double_rn(den));
                if (!split || i == k) {
                    sa[i] = -1;
                    if (split) keep[i] = 1;
                } else {
                    if (i < k) sb[i] = k;
                    else sa[i] = k;
                    open = 1;
                }
            }
        }
        return rounds;
    };
    const int rounds = LDS ? rounds_of(LdsPoints{l_xy, n}) : rounds_of(GlobalPoints{pts, n});
    if (tid == 0) atomicMax(head + 3, rounds);
}

// offsets[c] = the slot of contour c's first vertex, points[slot of a kept vertex] = that vertex; nothing is written after a bad input
__global__ void __launch_bounds__(TPB) simplify_emit_kernel(const int* __restrict__ packed, int nc, int total, const int* __restrict__ head,
                                                            const int* __restrict__ keep, const int* __restrict__ vscan, int* __restrict__ out) {
    if (head[2] != 0) return;
    const long g = (long)blockIdx.x * TPB + threadIdx.x;
    if (g <= nc) {
        const int o = packed[2 + g];                            // in [0, total]: checked by the simplify kernels
        out[2 + g] = vscan[o];
        if (g == 0) {
            out[0] = nc;
            out[1] = vscan[total];
        }
    }
    if (g < total && keep[g]) {
        const int* pts = packed + 3 + nc;
        int* opts = out + 3 + nc;
        const long v = vscan[g];
        opts[2 * v] = pts[2 * g];
        opts[2 * v + 1] = pts[2 * g + 1];
    }
}

__global__ void simplify_head_kernel(int nc, const int* __restrict__ vscan, int total, int* __restrict__ head) {
    head[0] = nc;
    head[1] = head[2] ? 0 : vscan[total];
}

inline long up256(long b) { return (b + 255) / 256 * 256; }

struct SimplifyWs {                                      // byte offsets into the workspace; the head and the packed result come first
    long head, out, keep, vscan, bsum, sa, sb, bidx, best, total;
    SimplifyWs(long n, long t) {
        long o = 0;
        auto take = [&](long bytes) { const long at = o; o += up256(bytes); return at; };
        head = take(16);
        out = take((3 + n + 2 * t) * 4);
        keep = take((t + 1) * 4);
        vscan = take((t + 1) * 4);
        bsum = take((long)cdiv(t + 1, SCAN_TILE) * 4);
        sa = take(t * 4);
        sb = take(t * 4);
        bidx = take(t * 4);
        best = take(t * 8);
        total = o;
    }
};

inline bool sizes_ok(long n, long total) { return n >= 0 && total >= n && total < (1L << 30); }
}  // namespace

extern "C" long runet_contours_simplify_workspace_bytes(long n, long total) {
    if (!sizes_ok(n, total)) return -1;
    return SimplifyWs(n, total).total;
}

extern "C" long runet_contours_simplify_result_offset(void) { return SimplifyWs(0, 0).out; }

extern "C" int runet_contours_simplify(const int* packed, long n, long total, double eps_factor, int lds_max_vertices, void* workspace,
                                       long workspace_bytes, void* stream) {
    RUNET_REQUIRE(packed && workspace, "null pointer");
    RUNET_REQUIRE(sizes_ok(n, total), "need 0 <= n <= total < 2^30");
    RUNET_REQUIRE(eps_factor >= 0.0 && eps_factor <= 1.79769313486231570815e308, "eps_factor must be finite and not negative");
    RUNET_REQUIRE(((uintptr_t)packed % 4) == 0 && RUNET_ALIGNED16(workspace), "packed must be 4-byte, the workspace 16-byte aligned");
    const SimplifyWs S(n, total);
    RUNET_REQUIRE(workspace_bytes >= S.total, "workspace too small (runet_contours_simplify_workspace_bytes)");
    char* ws = (char*)workspace;
    int* head = (int*)(ws + S.head);
    int* out = (int*)(ws + S.out);
    int* keep = (int*)(ws + S.keep);
    int* vscan = (int*)(ws + S.vscan);
    hipStream_t st = (hipStream_t)stream;
    // head = {0, 0, 0, 0}; n == 0: result = {0, 0, offsets[0] = 0}; else no vertex kept yet
    if (hipMemsetAsync(head, 0, n == 0 ? (size_t)(S.out - S.head) + 12 : 16, st) != hipSuccess ||
        (n > 0 && hipMemsetAsync(keep, 0, ((size_t)total + 1) * 4, st) != hipSuccess)) {
        (void)hipGetLastError();
        runet_set_error("runet_contours_simplify: clearing the workspace failed");
        return RUNET_ELAUNCH;
    }
    if (n == 0) return RUNET_OK;
    const int lds_max = lds_max_vertices < 0 || lds_max_vertices > SIMPLIFY_LDS_CAP ? SIMPLIFY_LDS_CAP : lds_max_vertices;
    int* sa = (int*)(ws + S.sa);
    int* sb = (int*)(ws + S.sb);
    int* bidx = (int*)(ws + S.bidx);
    u64* best = (u64*)(ws + S.best);
    const int nc = (int)n, t = (int)total;
    hipLaunchKernelGGL(simplify_kernel<true>, dim3(nc), dim3(TPB), 0, st, packed, nc, t, eps_factor, lds_max, head, keep, sa, sb, bidx, best);
    hipLaunchKernelGGL(simplify_kernel<false>, dim3(nc), dim3(TPB), 0, st, packed, nc, t, eps_factor, lds_max, head, keep, sa, sb, bidx, best);
    excl_scan(Plain{keep}, total + 1, vscan, (int*)(ws + S.bsum), (long long*)nullptr, (int*)nullptr, st);
    hipLaunchKernelGGL(simplify_head_kernel, dim3(1), dim3(1), 0, st, nc, vscan, t, head);
    const long work = total > n + 1 ? total : n + 1;
    hipLaunchKernelGGL(simplify_emit_kernel, dim3(cdiv(work, TPB)), dim3(TPB), 0, st, packed, nc, t, head, keep, vscan, out);
    RUNET_CHECK_LAUNCH();
}
