// acc_cols.h -- the carry-deferred accumulators of the weighted sums: sum_j w_j * c_j of raw Montgomery words with ONE reduction per
// output word.  Shared by the linear combination (algebra_kernels.h) and the DEEP quotient (deep_kernels.h); a header of its own so
// that both translation units can include it without defining the kernels of algebra_kernels.h twice.
//
// Deferred reduction: with raw words, sum_j mont_mul(w_j, c_j) = montyred(sum_j w_j * c_j), so the Montgomery reduction is done once
// per output word.  The carries are deferred too: the four 32 x 32 partial products of a term are added into three 64-bit columns
// of weight 2^0, 2^32 and 2^64 (L, M, H) by v_mad_u64_u32 itself, and the carry each addition leaves goes into a 32-bit counter of
// its column (kL, kM, kH: weights 2^64, 2^96, 2^128) -- eight vector instructions per term, four of them products, against the
// fifteen of mont_mul2 plus a modular addition.  The four products are issued before the four counter updates, so every carry mask
// is read three instructions after it was written (gfx950 wants two wait states there, gl64.h).  At most three terms enter one
// accumulator per column of the sum (the middle coefficient of an XFieldElement product) and k <= 65 535, so a counter stays
// below 2 * 3 * 65 535 < 2^19.  Reduction, once: every piece times 2^-64 mod p --
//   montyred(L),  montyred(M 2^32),  H mod p,  kL,  kM 2^32 (below 2^51),  kH 2^64 = kH (2^32 - 1) (below 2^51)
// -- six canonical words, added in the field.
#pragma once

#include "gl64.h"

namespace tfk {

using gl::u32;
using gl::u64;

struct AccCols {
    u64 L, M, H;
    u32 kL, kM, kH;
};

__device__ __forceinline__ void acc_zero(AccCols& a) { a.L = 0, a.M = 0, a.H = 0, a.kL = 0, a.kM = 0, a.kH = 0; }

__device__ __forceinline__ void acc_mul_add(AccCols& a, u64 x, u64 y) {
    const u32 x0 = (u32)x, x1 = (u32)(x >> 32), y0 = (u32)y, y1 = (u32)(y >> 32);
    u64 c0, c1, c2, c3;
    asm("v_mad_u64_u32 %[L], %[c0], %[x0], %[y0], %[L]\n\t"
        "v_mad_u64_u32 %[M], %[c1], %[x0], %[y1], %[M]\n\t"
        "v_mad_u64_u32 %[H], %[c2], %[x1], %[y1], %[H]\n\t"
        "v_mad_u64_u32 %[M], %[c3], %[x1], %[y0], %[M]\n\t"
        "v_addc_co_u32_e64 %[kL], %[c0], 0, %[kL], %[c0]\n\t"
        "v_addc_co_u32_e64 %[kM], %[c1], 0, %[kM], %[c1]\n\t"
        "v_addc_co_u32_e64 %[kH], %[c2], 0, %[kH], %[c2]\n\t"
        "v_addc_co_u32_e64 %[kM], %[c3], 0, %[kM], %[c3]"
        : [L] "+v"(a.L), [M] "+v"(a.M), [H] "+v"(a.H), [kL] "+v"(a.kL), [kM] "+v"(a.kM), [kH] "+v"(a.kH), [c0] "=&s"(c0), [c1] "=&s"(c1),
          [c2] "=&s"(c2), [c3] "=&s"(c3)
        : [x0] "v"(x0), [x1] "v"(x1), [y0] "v"(y0), [y1] "v"(y1));
}

__device__ __forceinline__ u64 acc_reduce(const AccCols& a) {
    u64 r = gl::montyred(a.L, 0);
    r = gl::add(r, gl::montyred(a.M << 32, a.M >> 32));
    r = gl::add(r, a.H >= gl::P ? a.H - gl::P : a.H);
    r = gl::add(r, (u64)a.kL);
    r = gl::add(r, (u64)a.kM << 32);
    return gl::add(r, (u64)a.kH * gl::EPS);
}

}  // namespace tfk
