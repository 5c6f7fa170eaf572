// Exclusive int32 prefix sums over a device array or functor (internal; shared by contours.hip and simplify.hip): block sums, one block over
// the block sums, then the tiles again with their offsets.  Integer adds only, so the result does not depend on any order.
#pragma once
#include "runet_common.h"

namespace {
constexpr int SCAN_TPB = 256;
constexpr int SCAN_ITEMS = 8, SCAN_TILE = SCAN_TPB * SCAN_ITEMS;

__device__ __forceinline__ int block_excl_scan(int v, int* sm, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sm[wave] = inc;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < SCAN_TPB / 64; ++i) {
        const int t = sm[i];
        if (i < wave) off += t;
        total += t;
    }
    __syncthreads();
    return off + inc - v;
}

struct Plain {
    const int* a;
    __device__ int operator()(long i) const { return a[i]; }
};

template <class F>
__global__ void __launch_bounds__(SCAN_TPB) scan_sums_kernel(F f, long n, int* __restrict__ bsum) {
    __shared__ int sm[SCAN_TPB / 64];
    const long base = (long)blockIdx.x * SCAN_TILE + (long)threadIdx.x * SCAN_ITEMS;
    int s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j)
        if (base + j < n) s += f(base + j);
    int total;
    block_excl_scan(s, sm, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_TPB) scan_bsums_kernel(int* __restrict__ bsum, int nb, long long* __restrict__ tot64, int* __restrict__ tot32) {
    __shared__ int sm[SCAN_TPB / 64];
    long long carry = 0;
    for (int base = 0; base < nb; base += SCAN_TPB) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? bsum[i] : 0;
        int total;
        const int ex = block_excl_scan(v, sm, total);
        if (i < nb) bsum[i] = (int)(carry + ex);
        carry += total;
    }
    if (threadIdx.x == 0) {
        if (tot64) *tot64 = carry;
        if (tot32) *tot32 = (int)carry;
    }
}

template <class F>
__global__ void __launch_bounds__(SCAN_TPB) scan_write_kernel(F f, long n, const int* __restrict__ bsum, int* __restrict__ out) {
    __shared__ int sm[SCAN_TPB / 64];
    const long base = (long)blockIdx.x * SCAN_TILE + (long)threadIdx.x * SCAN_ITEMS;
    int v[SCAN_ITEMS];
    int s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        v[j] = base + j < n ? f(base + j) : 0;
        s += v[j];
    }
    int total;
    int ex = block_excl_scan(s, sm, total) + bsum[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        if (base + j < n) out[base + j] = ex;
        ex += v[j];
    }
}

// out[i] = f(0) + ... + f(i - 1) for i < n; bsum: cdiv(n, SCAN_TILE) ints of scratch; the total goes to tot64 / tot32 where given
template <class F>
void excl_scan(F f, long n, int* out, int* bsum, long long* tot64, int* tot32, hipStream_t st) {
    const int nb = cdiv(n, SCAN_TILE);
    hipLaunchKernelGGL(scan_sums_kernel<F>, dim3(nb), dim3(SCAN_TPB), 0, st, f, n, bsum);
    hipLaunchKernelGGL(scan_bsums_kernel, dim3(1), dim3(SCAN_TPB), 0, st, bsum, nb, tot64, tot32);
    hipLaunchKernelGGL(scan_write_kernel<F>, dim3(nb), dim3(SCAN_TPB), 0, st, f, n, bsum, out);
}
}  // namespace
