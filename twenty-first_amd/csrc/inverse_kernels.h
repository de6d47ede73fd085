// inverse_kernels.h -- FiniteField::batch_inversion (math/traits.rs:93-121) and Inverse::inverse_or_zero (:39-45) over a vector of
// BFieldElements (L = 1) or XFieldElements (L = 3).
//
// Montgomery's trick, laid out for a wave: every wave owns a chunk of 64 K consecutive elements and lane l takes the elements
// l + 64 j (j < K), so each load and store instruction of the wave touches 64 consecutive elements.  No LDS, no barrier:
//   forward   s_j = x_0 ... x_(j-1) (the lane's running products, kept in registers with the x_j), t = s_K;
//   wave      inclusive prefix and suffix products of the 64 lane totals (six shuffle steps each) and ONE inversion of the wave's
//             product W, done by every lane alike: t^-1 = W^-1 * (exclusive prefix) * (exclusive suffix);
//   backward  out_j = acc * s_j, acc = acc * x_j from j = K - 1 down (traits.rs:113-118).
// Three products per element and one inversion per 64 K elements, against one inversion (mont_pow, ~127 products) per element.
// Missing tail elements are padded with ONE, and a zero element is replaced by ONE on the way in: under batch_inversion it raises
// the status (the reference's assert!, traits.rs:106), under inverse_or_zero it is written back as zero -- either way the other
// elements of its wave keep their own inverses.  The whole chunk is read before any of it is written, so in == out is safe.
#pragma once

#include "gl64.h"

namespace tfk {

using gl::u64;

template <int L>
struct InvGeom {
    static constexpr int K = L == 1 ? 16 : 8;  // elements per lane
    static constexpr long long CHUNK = 64LL * K;
};

// x_field_element.rs:512-536 with self = [c, b, a], other = [f, e, d]; r may alias s or o
template <int L>
__device__ __forceinline__ void inv_mul(const u64 (&s)[L], const u64 (&o)[L], u64 (&r)[L]) {
    if constexpr (L == 1) {
        r[0] = gl::mont_mul(s[0], o[0]);
    } else {
        const u64 c = s[0], b = s[1], a = s[2], f = o[0], e = o[1], d = o[2];
        const u64 ae = gl::mont_mul(a, e), bd = gl::mont_mul(b, d), ad = gl::mont_mul(a, d);
        const u64 r0 = gl::sub(gl::sub(gl::mont_mul(c, f), ae), bd);
        const u64 r1 = gl::add(gl::add(gl::sub(gl::add(gl::mont_mul(b, f), gl::mont_mul(c, e)), ad), ae), bd);
        const u64 r2 = gl::add(gl::add(gl::add(gl::mont_mul(a, f), gl::mont_mul(b, e)), gl::mont_mul(c, d)), ad);
        r[0] = r0, r[1] = r1, r[2] = r2;
    }
}

template <int L>
__device__ __forceinline__ void inv_set_one(u64 (&r)[L]) {
    r[0] = gl::ONE;
#pragma unroll
    for (int k = 1; k < L; ++k) r[k] = 0;
}

template <int L>
__device__ __forceinline__ bool inv_is_zero(const u64 (&a)[L]) {
    u64 o = a[0];
#pragma unroll
    for (int k = 1; k < L; ++k) o |= a[k];
    return o == 0;
}

// a^-1 for a != 0; the extension field by the cofactors of its multiplication matrix over the determinant (one base-field
// exponentiation), as poly_kernels.h: xfe_inverse
template <int L>
__device__ __forceinline__ void inv_single(const u64 (&a)[L], u64 (&r)[L]) {
    if constexpr (L == 1) {
        r[0] = gl::mont_inverse(a[0]);
    } else {
        const u64 s = gl::add(a[0], a[2]), dd = gl::sub(a[1], a[2]);
        const u64 c0 = gl::sub(gl::mont_mul(s, s), gl::mont_mul(dd, a[1]));
        const u64 c1 = gl::sub(gl::mont_mul(dd, a[2]), gl::mont_mul(a[1], s));
        const u64 c2 = gl::sub(gl::mont_mul(a[1], a[1]), gl::mont_mul(s, a[2]));
        const u64 det = gl::sub(gl::sub(gl::mont_mul(a[0], c0), gl::mont_mul(a[2], c1)), gl::mont_mul(a[1], c2));
        const u64 di = gl::mont_inverse(det);
        r[0] = gl::mont_mul(c0, di);
        r[1] = gl::mont_mul(c1, di);
        r[2] = gl::mont_mul(c2, di);
    }
}

// OR_ZERO = false: batch_inversion; a zero element makes its wave write `code` to *status (the first non-zero code stays).
// OR_ZERO = true: inverse_or_zero, element by element; status is never touched (may be null).
// Grid-stride over the chunks, one chunk per wave and step: the loop bound is the same for every lane of a wave, so the
// shuffles always run with the whole wave.
template <int L, bool OR_ZERO>
__global__ void __launch_bounds__(256) batch_inverse_kernel(const u64* in, long long n, u64* out, int* status, int code) {
    constexpr int K = InvGeom<L>::K;
    constexpr long long CHUNK = InvGeom<L>::CHUNK;
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
    const long long chunks = (n + CHUNK - 1) / CHUNK;
    for (long long c = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < chunks; c += waves) {
        const long long base = c * CHUNK + lane;
        u64 x[K][L], s[K][L], acc[L];
        unsigned zeros = 0;  // bit j: element j of this lane is zero
        inv_set_one<L>(acc);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const long long i = base + 64LL * j;
            if (i < n) {
#pragma unroll
                for (int k = 0; k < L; ++k) x[j][k] = in[i * L + k];
            } else {
                inv_set_one<L>(x[j]);
            }
            if (inv_is_zero<L>(x[j])) {
                zeros |= 1u << j;
                inv_set_one<L>(x[j]);
            }
#pragma unroll
            for (int k = 0; k < L; ++k) s[j][k] = acc[k];
            inv_mul<L>(acc, x[j], acc);
        }
        // the lane totals t_l = acc: inclusive prefix and suffix products over the wave
        u64 pre[L], suf[L];
#pragma unroll
        for (int k = 0; k < L; ++k) pre[k] = suf[k] = acc[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            u64 up[L], dn[L];
#pragma unroll
            for (int k = 0; k < L; ++k) {
                up[k] = __shfl_up(pre[k], d, 64);
                dn[k] = __shfl_down(suf[k], d, 64);
            }
            if (lane >= d) inv_mul<L>(up, pre, pre);
            if (lane + d < 64) inv_mul<L>(suf, dn, suf);
        }
        u64 w[L], wi[L], ex_pre[L], ex_suf[L];
#pragma unroll
        for (int k = 0; k < L; ++k) {
            w[k] = __shfl(pre[k], 63, 64);
            ex_pre[k] = __shfl_up(pre[k], 1, 64);
            ex_suf[k] = __shfl_down(suf[k], 1, 64);
        }
        if (lane == 0) inv_set_one<L>(ex_pre);
        if (lane == 63) inv_set_one<L>(ex_suf);
        inv_single<L>(w, wi);  // W != 0: every zero was replaced by ONE
        inv_mul<L>(wi, ex_pre, acc);
        inv_mul<L>(acc, ex_suf, acc);  // t_l^-1
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
            u64 y[L];
            inv_mul<L>(acc, s[j], y);
            inv_mul<L>(acc, x[j], acc);
            const long long i = base + 64LL * j;
            if (i < n) {
                const bool z = OR_ZERO && ((zeros >> j) & 1u);
#pragma unroll
                for (int k = 0; k < L; ++k) out[i * L + k] = z ? 0 : y[k];
            }
        }
        if constexpr (!OR_ZERO) {
            if (__any(zeros != 0) && lane == 0) atomicCAS(status, 0, code);
        }
    }
}

}  // namespace tfk
