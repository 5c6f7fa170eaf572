// What the fused Winograd F(2x2, 3x3) kernels share: the XCD-aware block order of all four kernels (wino_conv_kernel, wino_wgrad_kernel,
// wino_wgrad_direct_kernel in conv_winograd.hip, wino_conv_x3_kernel in conv_winograd_x3.hip) and the front end of the two convolution
// kernels - tile constants, block -> patch decode, B^T d B on channel pairs.  The multiply stages and epilogues stay with their kernels.
// So does the halo loader (offsets, load_halo, store_halo) and the patch-base expression `rbase`, written out in both convolution
// kernels: from a function or a struct of this header, in every form tried, wino_conv_x3_kernel compiles to other instructions
// (DESIGN.md 3.13.5), and that kernel runs 89 % of the network's FLOPs.
#pragma once
#include "runet_common.h"

namespace wino2 {

constexpr int WT = 32;            // tiles per block: a 4 x 8 patch of 2x2 tiles
constexpr int WBN = 64;           // output channels per block
constexpr int RH = 10, RW = 18;   // input halo of the patch
constexpr int RPS = 24;           // floats per halo pixel in LDS (16 channels + pad: conflict-free ds_read_b64 in the transform)

// 1-D grid of nitems x nch blocks.  The nch blocks that share an item (an input patch, a tile range) get launch indices 8 apart: consecutive
// indices are dealt to the 8 XCDs round-robin, so they run at the same time on the SAME XCD and the item's data is fetched into one L2 once.
// Tail group (nitems not a multiple of 8): plain order over what is left.
__device__ __forceinline__ void xcd_order(int L, int nitems, int nch, int& item, int& chunk) {
    const int span = 8 * nch;
    const int grp = L / span, r = L - grp * span;
    item = grp * 8 + (r & 7);
    chunk = r >> 3;
    if (grp * 8 + 8 > nitems) {
        const int done = grp * 8, rem = nitems - done;
        item = done + r % rem;
        chunk = r / rem;
    }
}

// patch index -> (image, patch row, patch column): 8 x 16 output pixels, 10 x 18 input halo shared by the 32 tiles through LDS
struct Patch { int img, by, bx; };
__device__ __forceinline__ Patch patch_of(int bpatch, int TY, int TX) {
    const int bxs = (TX + 7) >> 3, bys = (TY + 3) >> 2;
    Patch p;
    p.img = bpatch / (bxs * bys);
    const int brem = bpatch - p.img * (bxs * bys);
    p.by = brem / bxs;
    p.bx = brem - p.by * bxs;
    return p;
}

// B^T d B of the 4x4 patch whose halo pixel (0,0) stands at R[rbase], on both channels of a pair (R: the block's halo in LDS, RPS floats
// per pixel); put(xi, value) receives position xi = 0 .. 15 in order
template <class Put>
__device__ __forceinline__ void input_transform(const float* R, int rbase, Put put) {
    float2 raw[16], tmp[16];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) raw[a * 4 + b] = *reinterpret_cast<const float2*>(&R[rbase + (a * RW + b) * RPS]);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const float2 d0 = raw[b], d1 = raw[4 + b], d2 = raw[8 + b], d3 = raw[12 + b];
        tmp[b] = make_float2(d0.x - d2.x, d0.y - d2.y);
        tmp[4 + b] = make_float2(d1.x + d2.x, d1.y + d2.y);
        tmp[8 + b] = make_float2(d2.x - d1.x, d2.y - d1.y);
        tmp[12 + b] = make_float2(d1.x - d3.x, d1.y - d3.y);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float2 v0 = tmp[a * 4], v1 = tmp[a * 4 + 1], v2 = tmp[a * 4 + 2], v3 = tmp[a * 4 + 3];
        put(a * 4 + 0, make_float2(v0.x - v2.x, v0.y - v2.y));
        put(a * 4 + 1, make_float2(v1.x + v2.x, v1.y + v2.y));
        put(a * 4 + 2, make_float2(v2.x - v1.x, v2.y - v1.y));
        put(a * 4 + 3, make_float2(v1.x - v3.x, v1.y - v3.y));
    }
}

}  // namespace wino2
