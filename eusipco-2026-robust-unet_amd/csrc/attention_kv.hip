// Reduced-KV softmax attention of SegFormer-Lite's EfficientSelfAttention (Extended_Baseline_Comparison.py:636-664): the queries are the
// q projection of every pixel, the keys / values the kv projection of the r x r-reduced map, heads split the channels contiguously
// (channel = head * 32 + j), attn = softmax((q k^T) * 32^-0.5) over the keys, out = attn v back at channel head * 32 + j.
//
// Layouts: q [n, Nq, C] and o / dq [n, Nq, C] are NHWC pixel rows (the 1x1 convolutions' outputs / inputs as they are); kv [n, Nk, 2C] with
// k = channels [0, C) and v = [C, 2C) (the reference's kv.reshape(B, 2, heads, 32, Nk)); lse [n, heads, Nq] = log-sum-exp of each query's
// scaled scores, the forward's by-product for the backward.
//
// fp32 throughout, on the vector ALUs: one lane owns one query, a 64-key tile of one (image, head)'s keys / values sits in LDS and every lane
// reads it by broadcast.  Scores never reach HBM: an online softmax runs over the 64-key tiles.  The forward launches up to 1024 one-wave
// blocks (64 per (image, head) at 16 x 256^2 stage 1, one query tile each); a block that walks several query tiles stages a single key tile
// once for all of them (Nk <= 64) and restages per query tile otherwise.  Measured at the 16 x 256^2 stage shapes this reaches 3-9 % of HBM
// bandwidth: it is latency-bound (one or two waves per SIMD), not bandwidth-bound.
//
// Backward (no float atomics, bitwise reproducible): P is recomputed from q, k and lse; delta = rowsum(dO o) [- dlse]; dS = P (dO v^T - delta).  A
// block walks all keys for its query tiles, so dq is complete in registers.  dk / dv are summed per block over its query tiles into the
// block's own workspace slot (in a fixed order), and a second kernel adds the slots in block order into dkv [n, Nk, 2C], the layout the kv
// convolution's data and weight gradients read.
#include "runet_common.h"
#include "../../include/runet_hip.h"

namespace {
constexpr int HD = 32;      // head dimension (SegFormer-Lite: dim / num_heads = 32 at every stage)
constexpr int QT = 64;      // queries per tile: one wave, one query per lane
constexpr int KT = 64;      // keys per forward tile
constexpr int KTB = 32;     // keys per backward tile
constexpr int PS = QT + 1;  // padded [key][query] row of the backward's P / dS tiles (odd stride: conflict-free both ways)
constexpr float SCALE = 0.17677669529663687f;   // the reference's (dim // num_heads) ** -0.5 = 32 ** -0.5, applied to q k^T as an fp32 factor

__device__ __forceinline__ void load_row(const float* __restrict__ p, bool ok, float (&r)[HD]) {
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) v = *reinterpret_cast<const f32x4*>(p + d);
        r[d] = v[0]; r[d + 1] = v[1]; r[d + 2] = v[2]; r[d + 3] = v[3];
    }
}

// keys [k0, k0 + nt) of one (image, head) into ks / vs [nt][HD]; rows past Nk are zeros
template <int NT>
__device__ __forceinline__ void stage_kv(const float* __restrict__ kb, const float* __restrict__ vb, int ldkv, int k0, int Nk, float* ks, float* vs) {
    for (int u = threadIdx.x; u < NT * HD / 4; u += QT) {
        const int j = u / (HD / 4), d = (u % (HD / 4)) * 4;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (k0 + j < Nk) {
            a = *reinterpret_cast<const f32x4*>(kb + (long)(k0 + j) * ldkv + d);
            b = *reinterpret_cast<const f32x4*>(vb + (long)(k0 + j) * ldkv + d);
        }
        *reinterpret_cast<f32x4*>(ks + j * HD + d) = a;
        *reinterpret_cast<f32x4*>(vs + j * HD + d) = b;
    }
}

__device__ __forceinline__ float dot_lds(const float (&r)[HD], const float* __restrict__ s) {
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < HD; d += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(s + d);
        acc = __builtin_fmaf(r[d], v[0], acc);
        acc = __builtin_fmaf(r[d + 1], v[1], acc);
        acc = __builtin_fmaf(r[d + 2], v[2], acc);
        acc = __builtin_fmaf(r[d + 3], v[3], acc);
    }
    return acc;
}

// grid (query blocks, heads, n), 64 lanes; the block walks query tiles blockIdx.x, + gridDim.x, ...
__global__ __launch_bounds__(QT) void kv_attn_fwd_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ kv, int ldkv,
                                                         float* __restrict__ o, int ldo, float* __restrict__ lse, int Nq, int Nk, int C, float scale) {
    __shared__ __attribute__((aligned(16))) float ks[KT * HD];
    __shared__ __attribute__((aligned(16))) float vs[KT * HD];
    const int lane = threadIdx.x, head = blockIdx.y, n = blockIdx.z, heads = gridDim.y;
    const float* qb = q + (long)n * Nq * ldq + head * HD;
    const float* kb = kv + (long)n * Nk * ldkv + head * HD;
    const float* vb = kb + C;
    float* ob = o + (long)n * Nq * ldo + head * HD;
    float* lb = lse + ((long)n * heads + head) * Nq;
    const int nkt = (Nk + KT - 1) / KT;
    bool staged = false;
    for (int q0 = blockIdx.x * QT; q0 < Nq; q0 += gridDim.x * QT) {
        const int i = q0 + lane;
        const bool live = i < Nq;
        float qr[HD], acc[HD];
        load_row(qb + (long)i * ldq, live, qr);
#pragma unroll
        for (int d = 0; d < HD; ++d) acc[d] = 0.f;
        float m = -INFINITY, l = 0.f;
        for (int kt = 0; kt < nkt; ++kt) {
            if (!staged) {                       // a single tile holds every key: staged once for all of the block's query tiles
                __syncthreads();
                stage_kv<KT>(kb, vb, ldkv, kt * KT, Nk, ks, vs);
                __syncthreads();
                staged = nkt == 1;
            }
            const int kn = min(KT, Nk - kt * KT);
            float s[KT];
            float mt = -INFINITY;
#pragma unroll
            for (int j = 0; j < KT; ++j) {
                s[j] = j < kn ? dot_lds(qr, ks + j * HD) * scale : -INFINITY;
                mt = fmaxf(mt, s[j]);
            }
            const float mn = fmaxf(m, mt);
            const float alpha = expf(m - mn);
            float lt = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] *= alpha;
#pragma unroll
            for (int j = 0; j < KT; ++j) {
                const float p = j < kn ? expf(s[j] - mn) : 0.f;
                lt += p;
                const float* vr = vs + j * HD;
#pragma unroll
                for (int d = 0; d < HD; d += 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(vr + d);
                    acc[d] = __builtin_fmaf(p, v[0], acc[d]);
                    acc[d + 1] = __builtin_fmaf(p, v[1], acc[d + 1]);
                    acc[d + 2] = __builtin_fmaf(p, v[2], acc[d + 2]);
                    acc[d + 3] = __builtin_fmaf(p, v[3], acc[d + 3]);
                }
            }
            l = l * alpha + lt;
            m = mn;
        }
        if (live) {
            const float inv = 1.0f / l;
            float* op = ob + (long)i * ldo;
#pragma unroll
            for (int d = 0; d < HD; d += 4) {
                f32x4 v = {acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv};
                *reinterpret_cast<f32x4*>(op + d) = v;
            }
            lb[i] = m + logf(l);
        }
    }
}

// grid (query blocks, heads, n), 64 lanes.  Slot of the block: ws[((n * heads + head) * gridDim.x + blockIdx.x) * Nk * 64 ...] = [Nk][dk 32 | dv 32]
__global__ __launch_bounds__(QT) void kv_attn_bwd_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ kv, int ldkv,
                                                         const float* __restrict__ o, int ldo, const float* __restrict__ dout, int lddo,
                                                         const float* __restrict__ lse, const float* __restrict__ dlse, float* __restrict__ dq,
                                                         int lddq, float* __restrict__ ws,
                                                         int Nq, int Nk, int C, float scale) {
    __shared__ __attribute__((aligned(16))) float ks[KTB * HD];
    __shared__ __attribute__((aligned(16))) float vs[KTB * HD];
    __shared__ __attribute__((aligned(16))) float qs[QT * HD];       // the tile's q rows (dk) and dO rows (dv)
    __shared__ __attribute__((aligned(16))) float gs[QT * HD];
    __shared__ float ps[KTB * PS];                                   // P [key][query]
    __shared__ float dss[KTB * PS];                                  // dS [key][query]
    const int lane = threadIdx.x, head = blockIdx.y, n = blockIdx.z, heads = gridDim.y;
    const float* qb = q + (long)n * Nq * ldq + head * HD;
    const float* kb = kv + (long)n * Nk * ldkv + head * HD;
    const float* vb = kb + C;
    const float* obp = o + (long)n * Nq * ldo + head * HD;
    const float* gb = dout + (long)n * Nq * lddo + head * HD;
    const float* lb = lse + ((long)n * heads + head) * Nq;
    float* dqb = dq + (long)n * Nq * lddq + head * HD;
    float* slot = ws + (((long)n * heads + head) * gridDim.x + blockIdx.x) * (long)Nk * (2 * HD);
    const int nkt = (Nk + KTB - 1) / KTB;
    // column phase: lane -> (key jc, half): half 0 sums dk_j = scale * sum_i dS_ij q_i, half 1 dv_j = sum_i P_ij dO_i
    const int jc = lane % KTB, half = lane / KTB;
    const float* csrc = half ? ps : dss;
    const float* crow = half ? gs : qs;
    const float cmul = half ? 1.0f : scale;
    bool first = true;
    for (int q0 = blockIdx.x * QT; q0 < Nq; q0 += gridDim.x * QT) {
        const int i = q0 + lane;
        const bool live = i < Nq;
        float qr[HD], gr[HD], dqa[HD];
        load_row(qb + (long)i * ldq, live, qr);
        load_row(gb + (long)i * lddo, live, gr);
        float delta = 0.f;
        {
            float orow[HD];
            load_row(obp + (long)i * ldo, live, orow);
#pragma unroll
            for (int d = 0; d < HD; ++d) delta = __builtin_fmaf(gr[d], orow[d], delta);
        }
        // an incoming lse gradient (the operator-level surface; the model passes none): d lse_i / d s_ij = P_ij, so dS = P (dP - delta + dlse)
        if (dlse && live) delta -= dlse[((long)n * heads + head) * Nq + i];
        const float li = live ? lb[i] : 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) dqa[d] = 0.f;
        __syncthreads();                                 // the previous tile's column phase is done with qs / gs
#pragma unroll
        for (int d = 0; d < HD; d += 4) {
            f32x4 a = {qr[d], qr[d + 1], qr[d + 2], qr[d + 3]}, b = {gr[d], gr[d + 1], gr[d + 2], gr[d + 3]};
            *reinterpret_cast<f32x4*>(qs + lane * HD + d) = a;
            *reinterpret_cast<f32x4*>(gs + lane * HD + d) = b;
        }
        for (int kt = 0; kt < nkt; ++kt) {
            const int k0 = kt * KTB;
            __syncthreads();                             // ks / vs / ps / dss free
            stage_kv<KTB>(kb, vb, ldkv, k0, Nk, ks, vs);
            __syncthreads();
            const int kn = min(KTB, Nk - k0);
            // row phase: this lane's query against the tile's keys
#pragma unroll 4
            for (int j = 0; j < KTB; ++j) {
                float p = 0.f, dsv = 0.f;
                if (live && j < kn) {
                    p = expf(dot_lds(qr, ks + j * HD) * scale - li);
                    dsv = p * (dot_lds(gr, vs + j * HD) - delta);
                    const float* kr = ks + j * HD;
#pragma unroll
                    for (int d = 0; d < HD; d += 4) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(kr + d);
                        dqa[d] = __builtin_fmaf(dsv, v[0], dqa[d]);
                        dqa[d + 1] = __builtin_fmaf(dsv, v[1], dqa[d + 1]);
                        dqa[d + 2] = __builtin_fmaf(dsv, v[2], dqa[d + 2]);
                        dqa[d + 3] = __builtin_fmaf(dsv, v[3], dqa[d + 3]);
                    }
                }
                ps[j * PS + lane] = p;
                dss[j * PS + lane] = dsv;
            }
            __syncthreads();
            // column phase: one key and one half per lane, the tile's 64 queries in order
            float acc[HD];
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = 0.f;
            for (int r = 0; r < QT; ++r) {
                const float wgt = csrc[jc * PS + r];
                const float* rr = crow + r * HD;
#pragma unroll
                for (int d = 0; d < HD; d += 4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(rr + d);
                    acc[d] = __builtin_fmaf(wgt, v[0], acc[d]);
                    acc[d + 1] = __builtin_fmaf(wgt, v[1], acc[d + 1]);
                    acc[d + 2] = __builtin_fmaf(wgt, v[2], acc[d + 2]);
                    acc[d + 3] = __builtin_fmaf(wgt, v[3], acc[d + 3]);
                }
            }
            if (jc < kn) {
                float* sp = slot + (long)(k0 + jc) * (2 * HD) + half * HD;
#pragma unroll
                for (int d = 0; d < HD; d += 4) {
                    f32x4 v = {acc[d] * cmul, acc[d + 1] * cmul, acc[d + 2] * cmul, acc[d + 3] * cmul};
                    if (!first) v += *reinterpret_cast<const f32x4*>(sp + d);
                    *reinterpret_cast<f32x4*>(sp + d) = v;
                }
            }
        }
        if (live) {
            float* dp = dqb + (long)i * lddq;
#pragma unroll
            for (int d = 0; d < HD; d += 4) {
                f32x4 v = {dqa[d] * scale, dqa[d + 1] * scale, dqa[d + 2] * scale, dqa[d + 3] * scale};
                *reinterpret_cast<f32x4*>(dp + d) = v;
            }
        }
        first = false;
    }
}

// dkv[n, j, c] = sum over the query blocks b (in order) of slot(n, head(c), b)[j][kind(c) * 32 + c % 32]; thread per 4 channels
__global__ __launch_bounds__(256) void kv_attn_dkv_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dkv, int lddkv, int N, int Nk,
                                                                 int C, int heads, int nb) {
    const int cv = (2 * C) / 4;
    const long total = (long)N * Nk * cv;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int c = (int)(t % cv) * 4;
        const long p = t / cv;
        const int j = (int)(p % Nk), n = (int)(p / Nk);
        const int kind = c / C, cc = c - kind * C, head = cc / HD, d = cc % HD;
        const float* s = ws + ((((long)n * heads + head) * nb) * Nk + j) * (2 * HD) + kind * HD + d;
        const long step = (long)Nk * (2 * HD);
        f32x4 acc = *reinterpret_cast<const f32x4*>(s);
        for (int b = 1; b < nb; ++b) acc += *reinterpret_cast<const f32x4*>(s + b * step);
        *reinterpret_cast<f32x4*>(dkv + p * lddkv + c) = acc;
    }
}

int fwd_blocks(int n_img, int heads, int nq) { const int nqt = cdiv(nq, QT), want = cdiv(1024, (long)n_img * heads); return nqt < want ? nqt : want; }
int bwd_blocks(int n_img, int heads, int nq) { const int nqt = cdiv(nq, QT), want = cdiv(512, (long)n_img * heads); return nqt < want ? nqt : want; }

const char* check_args(int n_img, int nq, int nk, int c, int heads) {
    if (n_img <= 0 || nq <= 0 || nk <= 0 || c <= 0 || heads <= 0) return "empty shape";
    if (c != heads * HD) return "head dimension must be 32 (c == 32 * heads)";
    if (n_img > 65535 || heads > 65535) return "too many images / heads";
    return nullptr;
}
}  // namespace

extern "C" long runet_kv_attention_bwd_workspace_floats(int n_img, int nq, int nk, int c, int heads) {
    if (check_args(n_img, nq, nk, c, heads)) return -1;
    return (long)n_img * heads * bwd_blocks(n_img, heads, nq) * nk * (2 * HD);
}

extern "C" int runet_kv_attention_fwd(const float* q, int ldq, const float* kv, int ldkv, float* o, int ldo, float* lse, int n_img, int nq, int nk,
                                      int c, int heads, void* stream) {
    RUNET_REQUIRE(q && kv && o && lse, "null pointer");
    const char* bad = check_args(n_img, nq, nk, c, heads);
    RUNET_REQUIRE(bad == nullptr, bad ? bad : "");
    RUNET_REQUIRE(ldq >= c && ldkv >= 2 * c && ldo >= c && ldq % 4 == 0 && ldkv % 4 == 0 && ldo % 4 == 0, "pixel strides must be multiples of 4 floats that cover the channels");
    RUNET_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)kv % 16) == 0 && ((uintptr_t)o % 16) == 0, "q, kv and o must be 16-byte aligned");
    const dim3 grid(fwd_blocks(n_img, heads, nq), heads, n_img);
    hipLaunchKernelGGL(kv_attn_fwd_kernel, grid, dim3(QT), 0, (hipStream_t)stream, q, ldq, kv, ldkv, o, ldo, lse, nq, nk, c,
                       SCALE);
    RUNET_CHECK_LAUNCH();
}

extern "C" int runet_kv_attention_bwd(const float* q, int ldq, const float* kv, int ldkv, const float* o, int ldo, const float* dout, int lddo,
                                      const float* lse, const float* dlse, float* dq, int lddq, float* dkv, int lddkv, float* workspace,
                                      long workspace_floats, int n_img,
                                      int nq, int nk, int c, int heads, void* stream) {
    RUNET_REQUIRE(q && kv && o && dout && lse && dq && dkv && workspace, "null pointer");
    const char* bad = check_args(n_img, nq, nk, c, heads);
    RUNET_REQUIRE(bad == nullptr, bad ? bad : "");
    RUNET_REQUIRE(ldq >= c && ldkv >= 2 * c && ldo >= c && lddo >= c && lddq >= c && lddkv >= 2 * c, "pixel strides must cover the channels");
    RUNET_REQUIRE(ldq % 4 == 0 && ldkv % 4 == 0 && ldo % 4 == 0 && lddo % 4 == 0 && lddq % 4 == 0 && lddkv % 4 == 0, "pixel strides must be multiples of 4 floats");
    RUNET_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)kv % 16) == 0 && ((uintptr_t)o % 16) == 0 && ((uintptr_t)dout % 16) == 0 &&
                  ((uintptr_t)dq % 16) == 0 && ((uintptr_t)dkv % 16) == 0 && ((uintptr_t)workspace % 16) == 0, "tensors must be 16-byte aligned");
    const int nb = bwd_blocks(n_img, heads, nq);
    RUNET_REQUIRE(workspace_floats >= (long)n_img * heads * nb * nk * (2 * HD), "workspace too small (runet_kv_attention_bwd_workspace_floats)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(kv_attn_bwd_kernel, dim3(nb, heads, n_img), dim3(QT), 0, st, q, ldq, kv, ldkv, o, ldo, dout, lddo, lse, dlse, dq, lddq, workspace,
                       nq, nk, c, SCALE);
    const long total = (long)n_img * nk * (2 * c / 4);
    const long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(kv_attn_dkv_reduce_kernel, dim3((int)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, workspace, dkv, lddkv, n_img, nk, c,
                       heads, nb);
    RUNET_CHECK_LAUNCH();
}
