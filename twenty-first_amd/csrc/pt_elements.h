// pt_elements.h -- field elements of W words (1 BFieldElement, 3 XFieldElement [c0, c1, c2]) in registers: the loads, stores and
// element arithmetic that the point kernels (points_kernels.h) and the fold (fri_kernels.h) share.  Words are canonical raw
// Montgomery words.
#pragma once

#include "gl64.h"
#include "inverse_kernels.h"  // inv_mul

namespace tfk {

using gl::u32;
using gl::u64;

template <int W>
__device__ __forceinline__ void pt_load(const u64* p, long long i, u64 (&r)[W]) {
#pragma unroll
    for (int k = 0; k < W; ++k) r[k] = p[i * W + k];
}
template <int W>
__device__ __forceinline__ void pt_store(u64* p, long long i, const u64 (&r)[W]) {
#pragma unroll
    for (int k = 0; k < W; ++k) p[i * W + k] = r[k];
}
template <int W>
__device__ __forceinline__ void pt_sub(const u64 (&a)[W], const u64 (&b)[W], u64 (&r)[W]) {
#pragma unroll
    for (int k = 0; k < W; ++k) r[k] = gl::sub(a[k], b[k]);
}
template <int W>
__device__ __forceinline__ void pt_add(const u64 (&a)[W], const u64 (&b)[W], u64 (&r)[W]) {
#pragma unroll
    for (int k = 0; k < W; ++k) r[k] = gl::add(a[k], b[k]);
}
template <int W>
__device__ __forceinline__ bool pt_eq(const u64 (&a)[W], const u64 (&b)[W]) {
    u64 d = a[0] ^ b[0];
#pragma unroll
    for (int k = 1; k < W; ++k) d |= a[k] ^ b[k];
    return d == 0;
}
// y - x for a y of WY words and an x of WX <= WY words: the lift of x has zero upper limbs
template <int WX, int WY>
__device__ __forceinline__ void pt_sub_lift(const u64 (&y)[WY], const u64 (&x)[WX], u64 (&r)[WY]) {
#pragma unroll
    for (int k = 0; k < WY; ++k) r[k] = k < WX ? gl::sub(y[k], x[k]) : y[k];
}
// x * y for an x of WX words and a y of WY >= WX words (r may alias y)
template <int WX, int WY>
__device__ __forceinline__ void pt_mul_xy(const u64 (&x)[WX], const u64 (&y)[WY], u64 (&r)[WY]) {
    if constexpr (WX == WY) {
        inv_mul<WY>(x, y, r);
    } else {
#pragma unroll
        for (int k = 0; k < WY; ++k) r[k] = gl::mont_mul(y[k], x[0]);
    }
}

}  // namespace tfk
