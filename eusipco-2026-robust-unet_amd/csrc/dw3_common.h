// The depthwise 3x3 convolution (padding 1, stride 1 or 2, no bias) of Fast-SCNN's DepthwiseSeparableConv (comne.py:310-311) at one output
// pixel, four channels per lane.  Shared by the stand-alone kernels (fastscnn.hip) and the fused depthwise -> pointwise kernels (dwsep.hip):
// taps in (r, s) order, one explicit FMA per tap and channel, so every kernel that evaluates it gets the same bits whatever the compiler
// contracts around it.
#pragma once
#include "runet_common.h"

// ld(ih, iw) -> the four input channels at input pixel (ih, iw) (only called inside the image); wv[r * 3 + s]: the taps' four channels
template <class Ld>
__device__ __forceinline__ f32x4 dw3_point(Ld ld, const f32x4* wv, int oh, int ow, int H, int W, int stride) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int ih = oh * stride + r - 1;
        if ((unsigned)ih >= (unsigned)H) continue;
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int iw = ow * stride + s - 1;
            if ((unsigned)iw >= (unsigned)W) continue;
            const f32x4 xv = ld(ih, iw);
            const f32x4 wt = wv[r * 3 + s];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(wt[e], xv[e], acc[e]);
        }
    }
    return acc;
}
