// Internal pieces shared by the split-operand ("bf16x6") kernels: gemm_split.hip (batched position GEMMs) and conv_x3.hip (1x1 and k2-s2
// transposed convolutions).  See gemm_split.hip for the arithmetic.
#pragma once
#include "runet_common.h"

namespace x3 {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// x = h + m + l exactly (see gemm_split.hip) for EVERY finite x.  bf16(x) rounds to nearest even, so a finite |x| >= 0x7F7F8000 (3.3961e38,
// FLT_MAX included) would round h to +-Inf, x - h = -+Inf, Inf - Inf = NaN, and the dot product of a finite operand would be NaN.  h is
// therefore taken from x clamped to +-bf16-max (0x7F7F0000; one v_med3_f32, and the same h as the plain rounding for every |x| below the
// threshold) while the residual is taken from x itself: a finite x keeps x - h exact (at most 16 significant bits, split exactly by m and l),
// an infinite x leaves r = +-Inf in m and a NaN leaves NaN there, so a non-finite operand still gives a non-finite result.
constexpr float BF16_MAX = 3.3895313892515355e38f;      // 0x7F7F0000
constexpr float H_OVERFLOWS = 3.3961775292304601e38f;   // 0x7F7F8000
__device__ __forceinline__ void split1(const float x, __bf16& h, __bf16& m, __bf16& l) {
    h = (__bf16)__builtin_amdgcn_fmed3f(x, -BF16_MAX, BF16_MAX);
    const float r = x - (float)h;
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);
}
__device__ __forceinline__ void split1_plain(const float x, __bf16& h, __bf16& m, __bf16& l) {      // |x| < 0x7F7F8000 or non-finite only
    h = (__bf16)x;
    const float r = x - (float)h;
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);
}

// How a hot kernel splits its fp32 operand (measured per kernel, DESIGN.md 3.0 / profiles/x3_edge_accuracy.txt):
//   X3_CLAMP  the clamp on every element;   X3_WAVE  the plain rounding unless some lane of the wave holds |x| >= 0x7F7F8000 (one max
//   per element pair, one compare and one wave-uniform branch per four elements), then the clamp;   X3_PLAIN  no protection (measurement only)
enum { X3_PLAIN = 0, X3_CLAMP = 1, X3_WAVE = 2 };
#ifndef X3_MODE_NN
#define X3_MODE_NN X3_CLAMP
#endif
#ifndef X3_MODE_TN
#define X3_MODE_TN X3_CLAMP
#endif
#ifndef X3_MODE_CONV
#define X3_MODE_CONV X3_CLAMP
#endif
#ifndef X3_MODE_WINO
#define X3_MODE_WINO X3_CLAMP
#endif

template <int MODE>
__device__ __forceinline__ void split3(const f32x4 x, bf16x4& h, bf16x4& m, bf16x4& l) {
    bool clamp = MODE == X3_CLAMP;
    if constexpr (MODE == X3_WAVE) {
        const float t = fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3])));      // a NaN lane needs no care: its h is NaN either way
        clamp = __builtin_amdgcn_ballot_w64(t >= H_OVERFLOWS) != 0;
    }
    if (clamp) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            __bf16 hj, mj, lj;
            split1(x[j], hj, mj, lj);
            h[j] = hj; m[j] = mj; l[j] = lj;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            __bf16 hj, mj, lj;
            split1_plain(x[j], hj, mj, lj);
            h[j] = hj; m[j] = mj; l[j] = lj;
        }
    }
}

// contiguous-range-per-XCD remap of the linear workgroup id (bijection for any total)
__device__ __forceinline__ long xcd_remap(long b, long total) {
    const long q = total >> 3, r = total & 7;
    const long xcd = b & 7, idx = b >> 3;
    return xcd * q + (xcd < r ? xcd : r) + idx;
}

// six products of one (A tile, B tile) pair, smallest first
#define X3_MMA(ACC, AF, BF)                                                              \
    do {                                                                                 \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AF[2], BF[0], ACC, 0, 0, 0);      \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AF[1], BF[1], ACC, 0, 0, 0);      \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AF[0], BF[2], ACC, 0, 0, 0);      \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AF[1], BF[0], ACC, 0, 0, 0);      \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AF[0], BF[1], ACC, 0, 0, 0);      \
        ACC = __builtin_amdgcn_mfma_f32_32x32x16_bf16(AF[0], BF[0], ACC, 0, 0, 0);      \
    } while (0)

// LDS stage (bytes): A image [plane 3][128 rows][16 k] bf16, 32-B rows; the two 16-B k-octets of a row are swapped on rows with bit 3 set
// (ds_read_b128's 16-lane groups {0-3,12-15,20-27} / {4-11,16-19,28-31} then hit 16 distinct 16-B slots: conflict-free);
// B image [plane 3][octet 2][BN columns][8 k] bf16 = the packed global layout verbatim.
template <int BN>
struct NNX3 {
    static constexpr int A_BYTES = 3 * 128 * 32, B_BYTES = 3 * 2 * BN * 16, STAGE = A_BYTES + B_BYTES;
    static constexpr int TN = BN / 64;                  // 32-column MFMA tiles per wave
    static constexpr int BITEMS = (3 * 2 * BN + 255) / 256;
};

}  // namespace x3
