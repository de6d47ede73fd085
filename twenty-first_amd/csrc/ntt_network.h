// ntt_network.h -- the shift-only radix-2^k networks of the NTT kernels (device code shared by ntt_kernels.h and lat_kernels.h).
//
// 2 has order 192 in the Goldilocks field (2^96 = -1), so every twiddle inside a transform of up to 64 points is a power of two
// (b_field_element.rs:46-51: w_64 = 2^39, w_32 = 2^78, ..., w_2 = 2^96): a butterfly level costs shifts and carry chains
// (gl::Pow2Mul, gl::add_sub_lazy2) instead of Montgomery products.  Templates and inline device functions only.
#pragma once

#include "gl64.h"

namespace tfk {

using gl::u32;
using gl::u64;

// ---- radix-2^k DIT network with power-of-two twiddles --------------------------------------
// w_{2^l} = 2^(39 * 2^(6-l))  (b_field_element.rs:46-51: w_64 = 2^39, ..., w_2 = 2^96 = -1), order 192.
template <bool INV, int LVL, int J>
struct TwExp {
    static constexpr int fwd = ((39 << (6 - LVL)) * J) % 192;
    static constexpr int value = INV ? (192 - fwd) % 192 : fwd;
};

#ifndef TF_ASM_BFLY
#define TF_ASM_BFLY 1  // 0: the compiler's compare-and-select add/sub (12 VALU per butterfly instead of 10)
#endif
#ifndef TF_LDS_TW
#define TF_LDS_TW 1  // the R = 1024 instantiations stage their [32][32] inner twiddle table in LDS (0: per-thread global loads, A/B build)
#endif
// The inner table w_R^(g k1) is read by row g: 32 words = 256 contiguous bytes per THREAD, i.e. a wave-load touches up to 64
// different cache lines.  Through global memory those 16 dwordx4 loads per thread compete with the data stream for the
// texture-addresser / L1 path (measured: 2.148 -> 2.081 ms per 256 x 2^20 with the column pass alone reading it from LDS,
// profiles/r02b_ab_variants.txt); staged once per workgroup behind the exchange buffer, rows padded to 34 words (272 bytes:
// 16-byte aligned for ds_read_b128, consecutive rows 4 banks apart), the reads are conflict-free LDS traffic.
constexpr int kLdsTwStride = 34;
// exchange geometry of the R1024 instantiation (= what finish_geometry computes for 512 threads and rounds of 8 192 elements)
constexpr int kR1024Nc = 16, kR1024Cpr = 8, kR1024Rounds = 2, kR1024S1 = 264;
// LAST1024 exchange layout: element (k1, g, cc) at k1 * kL1024S1 + cc * kL1024CS + g  (see the kernel)
constexpr int kL1024S1 = 273, kL1024CS = 34;
constexpr int kL1024ExchangeWords = ((31 * kL1024S1 + 7 * kL1024CS + 32 + 1) / 2) * 2;  // 16-byte aligned end
#ifndef TF_LAZY
#define TF_LAZY 1  // 0: every network canonical (A/B build); 1: lazy butterflies in the networks that are followed by a Montgomery product
#endif

// Butterfly I (0 .. 15) of level LVL over 32 register slots: groups of 2^LVL consecutive slots, butterfly j of a group pairs
// slots (base + j, base + j + 2^(LVL-1)) with the twiddle w_{2^LVL}^j (inputs of a group in bit-reversed order, outputs natural).
template <bool INV, int LVL, int I>
struct Bf {
    static constexpr int H = 1 << (LVL - 1);
    static constexpr int j = I % H;
    static constexpr int ia = (I / H) * 2 * H + j;
    static constexpr int ib = ia + H;
    static constexpr int E = TwExp<INV, LVL, j>::value;
    static constexpr bool neg = gl::Pow2Mul<E>::negate;  // the power-of-two product comes back negated: swap the outputs
};

// x * 2^E up to the sign Bf::neg, as a CANONICAL word whatever 64-bit word x is (shl_fold / shl_monty reduce fully).
// E = 0 passes x through: canonical in a canonical network; in a lazy network only level 1 meets that case with canonical inputs
// (loaded words or Montgomery products), the levels above canonicalise the operand first (LAZY_IN).
template <int E, bool LAZY_IN>
__device__ __forceinline__ u64 tw_operand(u64 b) {
    if constexpr (E % 192 == 0) {
#if TF_ASM_POW2
        if constexpr (LAZY_IN) return gl::canonical_asm(b);  // b >= p ? b - p : b   (3 VALU)
#endif
        if constexpr (LAZY_IN) return gl::add(b, 0);  // b >= p ? b - p : b   (4 VALU)
        return b;
    } else {
        return gl::Pow2Mul<E>::apply(b);
    }
}

// Two butterflies (I, I + 1) of one level in one block of interleaved carry chains (gl::add_sub2 / gl::add_sub_lazy2).
//   LAZY = false: canonical inputs and outputs (ten VALU per butterfly).
//   LAZY = true:  the first operand of a butterfly may be any 64-bit word congruent to the element, the outputs are such words
//                 (eight VALU per butterfly); the twiddled operand is always canonical (tw_operand).
template <bool INV, int LVL, int I, bool LAZY>
__device__ __forceinline__ void butterfly_pair(u64 (&x)[32]) {
    using B0 = Bf<INV, LVL, I>;
    using B1 = Bf<INV, LVL, I + 1>;
    const u64 v0 = tw_operand<B0::E, LAZY && (LVL > 1)>(x[B0::ib]);
    const u64 v1 = tw_operand<B1::E, LAZY && (LVL > 1)>(x[B1::ib]);
    u64 s0, d0, s1, d1;
    if constexpr (LAZY) gl::add_sub_lazy2(x[B0::ia], v0, x[B1::ia], v1, s0, d0, s1, d1);
    else gl::add_sub2(x[B0::ia], v0, x[B1::ia], v1, s0, d0, s1, d1);
    x[B0::ia] = B0::neg ? d0 : s0;
    x[B0::ib] = B0::neg ? s0 : d0;
    x[B1::ia] = B1::neg ? d1 : s1;
    x[B1::ib] = B1::neg ? s1 : d1;
}

template <int E>
__device__ __forceinline__ void butterfly_pow2(u64& a, u64& b) {
    // (a, b) -> (a + b * 2^E, a - b * 2^E), canonical in and out; the sign of the power-of-two product is folded into add/sub
    const u64 v = gl::Pow2Mul<E>::apply(b);
#if TF_ASM_BFLY
    if constexpr (!gl::Pow2Mul<E>::negate) gl::add_sub(a, v, a, b);
    else gl::add_sub(a, v, b, a);
    return;
#endif
    if constexpr (!gl::Pow2Mul<E>::negate) {
        const u64 s = gl::add(a, v);
        b = gl::sub(a, v);
        a = s;
    } else {
        const u64 s = gl::sub(a, v);
        b = gl::add(a, v);
        a = s;
    }
}

#ifndef TF_POW2_WIDE
#define TF_POW2_WIDE 4  // most power-of-two products per block: 4 or 2
#endif
#if TF_ASM_BFLY && TF_ASM_POW2
// ---- a level's butterflies, grouped by the exponent class of their twiddle ---------------------------------------------------------
// The Montgomery-form products (gl::shl_monty_block) want four carry chains per block to hide the carry-mask wait states, and a
// block takes one form; neighbouring butterflies (I, I + 1) rarely share one.  The butterflies of a level touch disjoint slots, so
// they may run in any order: class by class, the twiddled operands of four (or two) butterflies are multiplied in one block and
// their butterflies follow at once (class_fused); the odd one of a class is left over and paired with another class's
// (leftover_fused).  Same words as butterfly_pair computes for the pairs (I, I + 1).
constexpr int bf_exp(bool inv, int lvl, int i) {  // = Bf<INV, LVL, I>::E
    const int fwd = ((39 << (6 - lvl)) * (i % (1 << (lvl - 1)))) % 192;
    return inv ? (192 - fwd) % 192 : fwd;
}
constexpr int bf_cls(bool inv, int lvl, int i) {  // = gl::Pow2Mul<E>::cls
    const int e96 = bf_exp(inv, lvl, i) % 96;
    return e96 == 0 ? 0 : e96 < 32 ? 1 : e96 < 64 ? 2 : 3;
}
constexpr int bf_count(bool inv, int lvl, int i0, int end, int cls) {
    int n = 0;
    for (int i = i0; i < end; ++i) n += bf_cls(inv, lvl, i) == cls;
    return n;
}
constexpr int bf_nth(bool inv, int lvl, int i0, int end, int cls, int pos) {  // the pos-th butterfly of the class in [i0, end)
    for (int i = i0; i < end; ++i)
        if (bf_cls(inv, lvl, i) == cls && pos-- == 0) return i;
    return i0;
}
// two butterflies BA, BB (any two of one level) on operands that are already multiplied
template <typename BA, typename BB, bool LAZY>
__device__ __forceinline__ void bfly2(u64 (&x)[32]) {
    u64 s0, d0, s1, d1;
    if constexpr (LAZY) gl::add_sub_lazy2(x[BA::ia], x[BA::ib], x[BB::ia], x[BB::ib], s0, d0, s1, d1);
    else gl::add_sub2(x[BA::ia], x[BA::ib], x[BB::ia], x[BB::ib], s0, d0, s1, d1);
    x[BA::ia] = BA::neg ? d0 : s0;
    x[BA::ib] = BA::neg ? s0 : d0;
    x[BB::ia] = BB::neg ? d1 : s1;
    x[BB::ib] = BB::neg ? s1 : d1;
}
// class CLS of butterflies [I0, END): blocks of four or two products, each followed at once by its butterflies; an odd one is left over
template <bool INV, int LVL, int I0, int END, int CLS, bool LAZY, int WIDE, int POS = 0>
__device__ __forceinline__ void class_fused(u64 (&x)[32]) {
    constexpr int rem = bf_count(INV, LVL, I0, END, CLS) - POS;
    if constexpr (rem >= 2) {
        constexpr int take = (rem >= 4 && WIDE >= 4) ? 4 : 2;
        using A = Bf<INV, LVL, bf_nth(INV, LVL, I0, END, CLS, POS)>;
        using B = Bf<INV, LVL, bf_nth(INV, LVL, I0, END, CLS, POS + 1)>;
        using C = Bf<INV, LVL, bf_nth(INV, LVL, I0, END, CLS, POS + (take > 2 ? 2 : 0))>;
        using D = Bf<INV, LVL, bf_nth(INV, LVL, I0, END, CLS, POS + (take > 2 ? 3 : 1))>;
        if constexpr (CLS == 0) {
            x[A::ib] = tw_operand<A::E, LAZY && (LVL > 1)>(x[A::ib]);
            x[B::ib] = tw_operand<B::E, LAZY && (LVL > 1)>(x[B::ib]);
            bfly2<A, B, LAZY>(x);
        } else if constexpr (take == 2) {
            u64 v[2] = {x[A::ib], x[B::ib]};
            gl::pow2_mul_block<A::E, B::E>(v);
            x[A::ib] = v[0], x[B::ib] = v[1];
            bfly2<A, B, LAZY>(x);
        } else {
            u64 v[4] = {x[A::ib], x[B::ib], x[C::ib], x[D::ib]};
            gl::pow2_mul_block<A::E, B::E, C::E, D::E>(v);
            x[A::ib] = v[0], x[B::ib] = v[1], x[C::ib] = v[2], x[D::ib] = v[3];
            bfly2<A, B, LAZY>(x);
            bfly2<C, D, LAZY>(x);
        }
        class_fused<INV, LVL, I0, END, CLS, LAZY, WIDE, POS + (CLS == 0 ? 2 : take)>(x);
    }
}
// the k-th left-over butterfly: the last one of each class with an odd count, classes in order
constexpr int bf_leftover(bool inv, int lvl, int i0, int end, int k) {
    for (int c = 0; c < 4; ++c) {
        const int n = bf_count(inv, lvl, i0, end, c);
        if ((n & 1) && k-- == 0) return bf_nth(inv, lvl, i0, end, c, n - 1);
    }
    return -1;
}
template <bool INV, int LVL, int I0, int END, bool LAZY, int K = 0>
__device__ __forceinline__ void leftover_fused(u64 (&x)[32]) {
    constexpr int ia = bf_leftover(INV, LVL, I0, END, K), ib = bf_leftover(INV, LVL, I0, END, K + 1);
    if constexpr (ia >= 0) {
        static_assert(ib >= 0, "an even number of butterflies leaves an even number over");
        using A = Bf<INV, LVL, ia>;
        using B = Bf<INV, LVL, (ib >= 0 ? ib : 0)>;
        x[A::ib] = tw_operand<A::E, LAZY && (LVL > 1)>(x[A::ib]);
        x[B::ib] = tw_operand<B::E, LAZY && (LVL > 1)>(x[B::ib]);
        bfly2<A, B, LAZY>(x);
        leftover_fused<INV, LVL, I0, END, LAZY, K + 2>(x);
    }
}
#endif

// butterflies [I, END) of level LVL, two at a time
template <bool INV, int LVL, int I, int END, bool LAZY, int WIDE = TF_POW2_WIDE>
struct DitRange {
    static __device__ __forceinline__ void run(u64 (&x)[32]) {
#if TF_ASM_BFLY && TF_ASM_POW2
        static_assert(bf_exp(INV, LVL, I) == Bf<INV, LVL, I>::E && bf_exp(INV, LVL, END - 1) == Bf<INV, LVL, END - 1>::E, "");
        class_fused<INV, LVL, I, END, 0, LAZY, WIDE>(x);
        class_fused<INV, LVL, I, END, 1, LAZY, WIDE>(x);
        class_fused<INV, LVL, I, END, 2, LAZY, WIDE>(x);
        class_fused<INV, LVL, I, END, 3, LAZY, WIDE>(x);
        leftover_fused<INV, LVL, I, END, LAZY>(x);
#else
#if TF_ASM_BFLY
        butterfly_pair<INV, LVL, I, LAZY>(x);
#else
        butterfly_pow2<Bf<INV, LVL, I>::E>(x[Bf<INV, LVL, I>::ia], x[Bf<INV, LVL, I>::ib]);
        butterfly_pow2<Bf<INV, LVL, I + 1>::E>(x[Bf<INV, LVL, I + 1>::ia], x[Bf<INV, LVL, I + 1>::ib]);
#endif
        if constexpr (I + 2 < END) DitRange<INV, LVL, I + 2, END, LAZY>::run(x);
#endif
    }
};
// Level LVL of a DIT network over all 32 registers.
template <bool INV, int LVL, bool LAZY = false, int WIDE = TF_POW2_WIDE>
__device__ __forceinline__ void dit_level(u64 (&x)[32]) { DitRange<INV, LVL, 0, 16, LAZY && TF_LAZY, WIDE>::run(x); }

// levels 1..4 restricted to the 16 register slots starting at FIRST (0 or 16): butterflies FIRST/2 .. FIRST/2 + 7 of each level
template <bool INV, int FIRST, bool LAZY = false, int WIDE = TF_POW2_WIDE>
__device__ __forceinline__ void dit_half(u64 (&x)[32]) {
    DitRange<INV, 1, FIRST / 2, FIRST / 2 + 8, LAZY && TF_LAZY, WIDE>::run(x);
    DitRange<INV, 2, FIRST / 2, FIRST / 2 + 8, LAZY && TF_LAZY, WIDE>::run(x);
    DitRange<INV, 3, FIRST / 2, FIRST / 2 + 8, LAZY && TF_LAZY, WIDE>::run(x);
    DitRange<INV, 4, FIRST / 2, FIRST / 2 + 8, LAZY && TF_LAZY, WIDE>::run(x);
}

// x[q0 .. q0+3] *= w[0 .. 3]  (four Montgomery products, no wait-state nops: gl::mont_mul4)
__device__ __forceinline__ void mul4_inplace(u64 (&x)[32], int q0, u64 w0, u64 w1, u64 w2, u64 w3) {
    const u64 a4[4] = {x[q0], x[q0 + 1], x[q0 + 2], x[q0 + 3]}, b4[4] = {w0, w1, w2, w3};
    u64 r4[4];
    gl::mont_mul4(a4, b4, r4);
    x[q0] = r4[0], x[q0 + 1] = r4[1], x[q0 + 2] = r4[2], x[q0 + 3] = r4[3];
}

}  // namespace tfk
