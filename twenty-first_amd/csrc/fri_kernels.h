// fri_kernels.h -- the FRI split-and-fold of codewords that stay in device memory, one to R levels per pass:
//   out[i] = Polynomial::get_colinear_y((x_i, c[i]), (-x_i, c[i + n/2]), alpha)   math/polynomial.rs:386-394, x_i = g w_n^i
//          = 1/2 [(c[i] + c[i + n/2]) + alpha x_i^-1 (c[i] - c[i + n/2])]          0 <= i < n/2
// on the codeword c of n = 2^k values over {g w_n^i}; the result lies over {g^2 w_{n/2}^i}, so the next level folds it again.
// A field element is W words (1 BFieldElement, 3 XFieldElement [c0, c1, c2]), canonical raw Montgomery words in and out.  WC is the
// width of the codeword and WA that of the challenges and the result, (WC, WA) in {(1, 1), (3, 3), (1, 3)}: in the mixed form a
// BFieldElement value stands for its lift, every product with it is three base-field products, and the levels after the first
// are (3, 3) on what the first one left.
//
// One thread owns output element i of a codeword and folds R levels in registers.  With m = n / 2^R outputs per codeword it loads
// the 2^R inputs c[i + t m]; neighbouring lanes own neighbouring i, so each of these loads covers consecutive elements of a wave.
// At the first level the pair (t, t + 2^(R-1)) sits at index i + t m of its codeword, whose inverse point is
//     x^-1 = g^-1 w_n^-(i + t m) = y w_{2^R}^-t,   y = g^-1 w_n^-i,
// and w_{2^l} = 2^(39 2^(6 - l)) (ntt_network.h), so the twiddle is a power-of-two product.  The next level runs on the squared
// offset and the squared root: its inverse points are the squares of this level's, y^2 w_{2^(R-1)}^-t.  No division anywhere:
// the host passes g^-1 and the repeated squares of w_n^-1 by value (as PowersTable for powers_kernel), a thread multiplies the
// entries of the set bits of i and then walks its stride with one product per element.  The halvings commute with everything else:
// they are taken once, as 2^-R = 2^(192 - R) on the stored element.  No LDS, no work space, no cross-lane operation.
#pragma once

#include <utility>

#include "gl64.h"
#include "pt_elements.h"  // pt_load, pt_store, pt_add, pt_sub, pt_mul_xy (inv_mul)

namespace tfk {

constexpr int kFriThreads = 256;
// levels one pass folds at the most: the fastest of the candidates 2, 3, 4, none of which needs scratch (DESIGN 7.6 has the register
// counts and the measurements; `make fri_candidates` builds a library per candidate)
#ifndef TF_FRI_MAX_LEVELS
#define TF_FRI_MAX_LEVELS 4
#endif
constexpr int kFriMaxLevels = TF_FRI_MAX_LEVELS;
static_assert(kFriMaxLevels >= 2 && kFriMaxLevels <= 4, "the candidates of DESIGN 7.6");

// what a pass knows about its evaluation domain, built on the host (tf_fri.hip) and passed by value
constexpr int kFriTableLen = 30;
struct FriPoints {
    u64 g_inv;            // the inverse of the pass's offset
    u64 w[kFriTableLen];  // w_n^-(2^j) for the pass's n
};

// one pair of a level with 2^K values per thread left: r = (a + b) + alpha (y w_{2^K}^-T) (a - b); the halving is the caller's
template <int WIN, int WA, int K, int T>
__device__ __forceinline__ void fri_pair(const u64 (&a)[WIN], const u64 (&b)[WIN], u64 y, const u64 (&alpha)[WA], u64 (&r)[WA]) {
    constexpr int E = (192 - (39 * (64 >> K) * T) % 192) % 192;  // w_{2^K}^-T = 2^E
    const u64 x = gl::mul_pow2<E>(y);
    u64 s[WA], d[WIN], sum[WIN], p[WA];
#pragma unroll
    for (int k = 0; k < WA; ++k) s[k] = gl::mont_mul(alpha[k], x);
    pt_sub<WIN>(a, b, d);
    pt_add<WIN>(a, b, sum);
    pt_mul_xy<WIN, WA>(d, s, p);
#pragma unroll
    for (int k = 0; k < WA; ++k) r[k] = k < WIN ? gl::add(sum[k], p[k]) : p[k];
}

template <int WIN, int WA, int K, int... T>
__device__ __forceinline__ void fri_level(const u64 (&in)[1 << K][WIN], u64 y, const u64 (&alpha)[WA], u64 (&out)[(1 << K) / 2][WA],
                                          std::integer_sequence<int, T...>) {
    (fri_pair<WIN, WA, K, T>(in[T], in[T + (1 << K) / 2], y, alpha, out[T]), ...);
}

// K levels on the 2^K values of a thread: level by level the challenge alpha[0], alpha[1], ... and the inverse point y, y^2, ...
template <int WIN, int WA, int K>
__device__ __forceinline__ void fri_levels(const u64 (&in)[1 << K][WIN], u64 y, const u64* alpha, u64 (&r)[WA]) {
    u64 al[WA], half[(1 << K) / 2][WA];
    pt_load<WA>(alpha, 0, al);
    fri_level<WIN, WA, K>(in, y, al, half, std::make_integer_sequence<int, (1 << K) / 2>{});
    if constexpr (K == 1) {
#pragma unroll
        for (int k = 0; k < WA; ++k) r[k] = half[0][k];
    } else {
        fri_levels<WA, WA, K - 1>(half, gl::mont_mul(y, y), alpha + WA, r);
    }
}

// `total` = batch * m outputs, flattened over the codewords (m = 2^log_m per codeword, each read from n = m 2^R inputs), on
// S = 2^log_s threads: thread t0 takes the outputs t0, t0 + S, ...  Its index inside the codeword moves by S mod m, so it either
// stays (S >= m) or walks i0, i0 + S, ... and is back at i0 in the next codeword; y follows with one product per step.
// alpha: R elements of WA words for codeword b at alpha + b * alpha_stride (alpha_stride = 0: one set for all codewords).
template <int WC, int WA, int R>
__global__ void __launch_bounds__(kFriThreads) fri_fold_kernel(const u64* in, int log_m, long long total, FriPoints pts, int log_s, const u64* alpha,
                                                               long long alpha_stride, u64* out) {
    static_assert(R >= 1 && R <= 4 && WC <= WA, "");
    const long long t0 = (long long)blockIdx.x * kFriThreads + threadIdx.x;
    if (t0 >= total) return;  // (no barrier below)
    const long long m = 1ll << log_m;
    const long long i0 = t0 & (m - 1);
    u64 y0 = pts.g_inv;
    for (int j = 0; j < log_m; ++j)
        if ((i0 >> j) & 1) y0 = gl::mont_mul(y0, pts.w[j]);
    const u64 stride = pts.w[log_s];
    u64 y = y0;
    long long i = i0;
    for (long long f = t0; f < total; f += 1ll << log_s) {
        const long long b = f >> log_m;
        const u64* c = in + ((b << log_m) << R) * WC;
        u64 v[1 << R][WC], r[WA];
#pragma unroll
        for (int t = 0; t < (1 << R); ++t) pt_load<WC>(c, i + t * m, v[t]);
        fri_levels<WC, WA, R>(v, y, alpha + b * alpha_stride, r);
#pragma unroll
        for (int k = 0; k < WA; ++k) r[k] = gl::mul_pow2<192 - R>(r[k]);
        pt_store<WA>(out, f, r);
        const long long next = (i + (1ll << log_s)) & (m - 1);
        y = next == i0 ? y0 : gl::mont_mul(y, stride);
        i = next;
    }
}

}  // namespace tfk
